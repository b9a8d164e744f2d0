"""Every GW_* environment knob the library reads has a decided place in the suite.

A knob selects a kernel variant or a host policy; one that no test sets leaves
its path unproven, and a default flipped later silently changes what the suite
covers.  So every getenv("GW_...") name in goworld_amd/csrc must stand in
exactly one of:

* the variant matrix and the tier tests (test_gpu_variants.MATRIX_KNOBS,
  test_gpu_tiers.TIER_KNOBS), which set it and assert the kernel it selects;
* COVERED_ELSEWHERE: an existing test file that sets it (the name must occur
  there);
* NOT_A_KERNEL_PATH, with the reason.

A new knob fails this test until someone decides where it is tested.  Knobs are
read in gw_init only (one transport timeout apart, read when its group is
made): a `static` initialised from getenv latches the first context's
environment for the whole process, so a later test's setenv is silently
ignored -- none may exist."""
import glob
import os
import re

import test_gpu_tiers
import test_gpu_variants

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "goworld_amd", "csrc")

COVERED_ELSEWHERE = {
    "GW_BK_FLAT": "test_gpu_parity.py",
    "GW_POST_SPLIT": "test_gpu_parity.py",
    "GW_PLACE_SPLIT": "test_gpu_parity.py",
    "GW_DIRTY_SPLIT": "test_gpu_parity.py",
    "GW_HALF_ROWS": "test_gpu_parity.py",
    "GW_GATE_LANE_MAX": "test_gpu_parity.py",
    "GW_GRID_CAP": "test_gpu_golden.py",
    "GW_OVERLAP_MIN": "test_gpu_step_mode.py",
    "GW_OVERLAP_COLLECT": "test_gpu_step_mode.py",
}
NOT_A_KERNEL_PATH = {
    "GW_DEBUG_STATS": "prints the statistics lines the variant tests read; selects nothing",
    "GW_LOOPBACK_TIMEOUT_S": "how long a loopback rank waits for its peers (host transport)",
    "GW_PAIR_AUTO": "host policy that sets pair_max from the last tick's size (>= 131072 movers); the kernel it "
                    "selects is the one GW_PAIR_MAX selects",
}


def _sources():
    out = {}
    for p in sorted(glob.glob(os.path.join(CSRC, "*"))):
        with open(p, encoding="utf-8") as f:
            out[os.path.basename(p)] = f.read()
    assert out
    return out


def test_every_knob_is_placed():
    names = set()
    for text in _sources().values():
        names |= set(re.findall(r'getenv\(\s*"(GW_[A-Z0-9_]+)"', text))
    assert len(names) > 20                                # the scan sees the knobs
    matrix = set(test_gpu_variants.MATRIX_KNOBS) | set(test_gpu_tiers.TIER_KNOBS)
    places = {"matrix": matrix, "elsewhere": set(COVERED_ELSEWHERE), "not a kernel path": set(NOT_A_KERNEL_PATH)}
    for n in sorted(names):
        where = [k for k, v in places.items() if n in v]
        assert len(where) == 1, f"{n}: placed in {where or 'no table'} (exactly one is required)"
    for k, v in places.items():
        assert v <= names | {"GW_DEBUG_STATS"}, f"{k}: {sorted(v - names)} are not read by the library"
    for n, fn in COVERED_ELSEWHERE.items():
        with open(os.path.join(HERE, fn), encoding="utf-8") as f:
            assert n in f.read(), f"{n} does not occur in {fn}"


def test_matrix_rows_set_what_they_list():
    """The tier tests' knob list is what their module really sets."""
    with open(os.path.join(HERE, "test_gpu_tiers.py"), encoding="utf-8") as f:
        text = f.read()
    used = set(re.findall(r'"(GW_[A-Z0-9_]+)"', text)) - {"GW_DEBUG_STATS"}
    assert used == set(test_gpu_tiers.TIER_KNOBS)


def test_no_knob_is_latched_in_a_static():
    for name, text in _sources().items():
        for i, line in enumerate(text.splitlines(), 1):
            assert not (re.search(r"\bstatic\b", line) and "getenv" in line), f"{name}:{i}: {line.strip()}"
        # ... nor one statement later: `static const bool on =` + newline + getenv
        assert not re.search(r"\bstatic\b[^;{}]*getenv", text), f"{name}: a static initialised from getenv"
