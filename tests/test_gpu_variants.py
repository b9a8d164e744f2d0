"""GPU: every kernel variant the dispatch can select, against the oracle.

The parity suite proves the kernels that the default knobs and its trace sizes
select.  The rows below set the knobs (read by gw_init) that select the others
-- the ones a size threshold picks in production (dirty-cell span, heavy-first,
walk or binary search, the general path over many spaces, the gate words of
k_mover_c) and the A/B variants behind a knob -- at the smallest traces that
still reach them, with the same bit-exact comparison as test_gpu_parity.py
(events raw, records in the documented stream order, neighbour lists).

Each run also reads the library's GW_DEBUG_STATS lines (one per tick, one per
collect, written to stderr) and asserts that the expected kernel token stands
on every one of them: a knob that stopped being read fails here instead of
leaving a green test of the default path.
"""
import functools

import numpy as np
import pytest

from goworld_amd import gpuaoi, traces as T
from oracle import pyorc

from test_gpu_parity import Harness

NWAVE = 4                 # waves per block of the dirty-cell merge (prim.hpp)
HEAVY_DEFAULT = 512       # ctx.hpp heavy_min


# --------------------------------------------------------------------------- traces
@functools.lru_cache(maxsize=None)
def _trace_a():
    return T.adversarial_trace(13, n=300, ticks=12, leave_masks=True)


def _with_gates(tr, gates):
    import copy
    tr = copy.copy(tr)                       # the ops and positions are shared, read-only
    tr.gates = gates.astype(np.uint16)
    return tr


@functools.lru_cache(maxsize=None)
def traces(name):
    """(spaces, oracle mode) of a named trace; built once per process."""
    if name == "A":                          # one space, +-1-ulp bands, churn, gate ids 0..3 (G = 4)
        return [_trace_a()], pyorc.XZLIST
    if name == "Ab":                         # A on a 21 x 21 grid: 441 cells, no multiple of a wave's dirty span
        import copy
        tr = copy.copy(_trace_a())
        tr.bounds = (-500.0, -500.0, 505.0, 505.0)
        return [tr], pyorc.XZLIST
    if name == "A1":                         # one gate id (G = 2): no split by gate
        return [_with_gates(_trace_a(), np.ones(300))], pyorc.XZLIST
    if name == "A15":                        # gate ids 0..15 (G = 16): four gate words per lane
        s = np.arange(300)
        return [_with_gates(_trace_a(), np.where(s % 11 == 10, 0, 1 + s % 15))], pyorc.XZLIST
    if name == "D":                          # dense: a few hundred candidates per mover, one gate
        return [T.dyadic_walk_trace(9, 2000, 512.0, 100.0, 4)], pyorc.XZLIST
    if name == "S":                  # 40 small spaces, three gates (small-space mode)
        trs = [T.config4_space(s, ticks=3, n=300) for s in range(40)]
        for i, tr in enumerate(trs):
            tr.gates = np.where(tr.gates > 0, 1 + (i % 3), 0).astype(np.uint16)
        return trs, pyorc.SEQRULE
    raise KeyError(name)


def n_cells(tr, cells_per_d=2):
    """W * H of a space's grid as gw_space_create lays it out."""
    b = [float(v) for v in tr.bounds]
    d = float(tr.d)
    ex, ez = b[2] - b[0], b[3] - b[1]
    span = 2.0 * d + 4e-6 * (max(abs(v) for v in b) + d) + 1e-3
    cs = max(max(d / cells_per_d, max(ex, ez) / 4096.0), span / 9.0)
    return max(1, int(np.ceil(ex / cs))) * max(1, int(np.ceil(ez / cs)))


# --------------------------------------------------------------------------- the matrix
# diff / write: the token every tick / collect line must carry (None: any known
# token; the fields below are still checked).  Default dispatch of the traces:
DIFF_DEFAULT = {"A": "k_mover_c<2,0,2>", "Ab": "k_mover_c<2,0,2>", "A1": "k_mover_c<2,0,0>", "A15": "k_mover_c<2,0,4>",
                "D": "k_mover_c<2,0,0>", "S": "k_mover_small<2,1>"}
WRITE_DEFAULT = {"A": "k_sync_write_g<4>", "Ab": "k_sync_write_g<4>", "A15": "k_sync_write_g<4>", "S": "k_sync_write_small2",
                 "A1": None, "D": None}      # one gate: k_sync_write<4> or _h<4> by the last collect's mean
DIFF_TOKENS = {"k_mover_small<2,1>", "k_mover_small<2,0>", "k_mover_pair<2>", "k_mover<2,1>", "k_mover<2,2>",
               "k_mover<2,4>"} | {f"k_mover_c<2,{l},{g}>" for l in (0, 1) for g in (0, 2, 4)}
WRITE_TOKENS = {"k_sync_write<2>", "k_sync_write<4>", "k_sync_write<8>", "k_sync_write_h<4>", "k_sync_write<4,true>",
                "k_sync_write_small<2>", "k_sync_write_small<4>", "k_sync_write_small<8>", "k_sync_write_small2",
                "k_sync_write_g<4>"}


def _row(rid, env, names, diff=None, write=None, **fields):
    return dict(id=rid, env=env, traces=names, diff=diff, write=write, fields=fields)


ROWS = []
for wpb in (1, 2, 4):                        # the one-wave-per-entry kernel, 1 / 2 / 4 waves per block
    ROWS.append(_row(f"mover-wpb{wpb}", {"GW_MOVER_COMPACT": "0", "GW_MOVER_WPB": str(wpb)}, ("A", "D"),
                     diff=f"k_mover<2,{wpb}>"))
for wm in (0, 1000000):                      # forced walk on the sparse trace, forced binary search on the dense one
    ROWS.append(_row(f"walk-min{wm}", {"GW_WALK_MIN": str(wm)}, ("A", "D")))
for rs in (0, 64):                           # no rank placement / rank placement up to a whole wave
    ROWS.append(_row(f"rank-sort{rs}", {"GW_RANK_SORT": str(rs)}, ("A", "D", "S")))
ROWS.append(_row("heavy-min0", {"GW_HEAVY_MIN": "0"}, ("A", "D"), heavy="none"))
ROWS.append(_row("heavy-min1", {"GW_HEAVY_MIN": "1"}, ("A", "D"), heavy="all"))     # pidx stays empty
ROWS.append(_row("heavy-min64", {"GW_HEAVY_MIN": "64"}, ("A", "D"), heavy="some"))
ROWS.append(_row("heavy-default", {"GW_HEAVY_MIN": str(HEAVY_DEFAULT)}, ("D",), heavy="mix"))
ROWS.append(_row("heavy-maxm0", {"GW_HEAVY_MAXM": "0"}, ("A", "D"), heavy="none"))
for cpd in (1, 3, 4):                        # S with 4: more rows per window than a half-wave holds
    ROWS.append(_row(f"cells-per-d{cpd}", {"GW_CELLS_PER_D": str(cpd)}, ("A", "D", "S")))
for span in (1, 8, 16, 64):                  # the spans the cell count selects above 128k / 1M / 2M cells
    ROWS.append(_row(f"dirty-span{span}", {"GW_DIRTY_SPAN": str(span)}, ("Ab", "D")))
for u in (2, 8):
    ROWS.append(_row(f"sync-write-nb{u}", {"GW_SW_HALVES": "0", "GW_NB_U": str(u)}, ("A1", "D"),
                     write=f"k_sync_write<{u}>", nb_u=u))
    # several gates: the per-gate count and write kernels take the records (no nb_u branch there)
    ROWS.append(_row(f"sync-gates-nb{u}", {"GW_SW_HALVES": "0", "GW_NB_U": str(u)}, ("A", "A15"), nb_u=u))
    # ... and with the direct partitions off, k_sync_write<U> under several gates
    ROWS.append(_row(f"sync-write-nb{u}-sorted", {"GW_SW_HALVES": "0", "GW_NB_U": str(u), "GW_GATE_DIRECT": "0"},
                     ("A", "A15"), write=f"k_sync_write<{u}>", nb_u=u, gdirect=0))
ROWS.append(_row("sync-write-nb4", {"GW_SW_HALVES": "0"}, ("A1", "D"), write="k_sync_write<4>"))
ROWS.append(_row("sync-write-halves", {"GW_SW_HALVES": "1"}, ("D",), write="k_sync_write_h<4>"))
ROWS.append(_row("gate-counts0", {"GW_GATE_COUNTS": "0"}, ("A15",), diff="k_mover_c<2,0,0>"))
ROWS.append(_row("gate-direct0", {"GW_GATE_DIRECT": "0"}, ("A", "A15"), write=None, gdirect=0))
ROWS.append(_row("gate-counts0-direct0", {"GW_GATE_COUNTS": "0", "GW_GATE_DIRECT": "0"}, ("A15",),
                 diff="k_mover_c<2,0,0>", write=None, gdirect=0))
ROWS.append(_row("small0", {"GW_SMALL": "0"}, ("S",), diff="k_mover_c<2,0,2>", write="k_sync_write_g<4>", small=0))
ROWS.append(_row("mover-halves0", {"GW_MOVER_HALVES": "0"}, ("S",), diff="k_mover_small<2,0>"))
for u in (2, 4, 8):
    ROWS.append(_row(f"sync-small-nb{u}", {"GW_SYNC_HALVES": "0", "GW_NB_U": str(u)}, ("S",),
                     write=f"k_sync_write_small<{u}>", nb_u=u))
ROWS.append(_row("default", {}, ("A1", "A", "A15")))        # pins the token logic itself

CASES = [pytest.param(r, name, id=f"{r['id']}-{name}") for r in ROWS for name in r["traces"]]
# every knob a row sets (tests/test_knob_inventory.py places each GW_* name)
MATRIX_KNOBS = sorted({k for r in ROWS for k in r["env"]})


# --------------------------------------------------------------------------- the debug lines
def parse_stats(err):
    """The GW_DEBUG_STATS lines of a captured stderr: (ticks, collects), each a
    dict of the line's fields ('name value' and 'name=value' pairs)."""
    ticks, cols = [], []
    for ln in err.splitlines():
        for head, dst in (("gw_tick:", ticks), ("gw_sync_collect:", cols)):
            if ln.startswith(head):
                w = ln[len(head):].split()
                f, i = {}, 0
                while i < len(w):
                    if "=" in w[i]:
                        k, v = w[i].split("=", 1)
                        f[k] = v
                        i += 1
                    else:
                        f[w[i]] = w[i + 1]
                        i += 2
                dst.append(f)
    return ticks, cols


def run_and_check(g, trs, mode, capfd, cells_per_d=2, sample=None):
    """Loads the spaces, steps every tick with a collect after each, compares
    all of it with the oracle; returns the parsed tick and collect lines."""
    capfd.readouterr()
    h = Harness(g, trs, mode=mode, cells_per_d=cells_per_d)
    h.check_collect()
    nt = len(trs[0].ticks)
    for t in range(nt):
        h.step(t)
        h.check_collect()
    h.check_lists(sample=sample)
    ticks, cols = parse_stats(capfd.readouterr().err)
    assert len(ticks) == nt and len(cols) == nt + 1, (len(ticks), len(cols))
    return ticks, cols


@pytest.mark.gpu
@pytest.mark.parametrize("row,name", CASES)
def test_variant_vs_oracle(row, name, monkeypatch, capfd):
    env = row["env"]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("GW_DEBUG_STATS", "1")
    trs, mode = traces(name)
    cpd = int(env.get("GW_CELLS_PER_D", 2))
    if "GW_DIRTY_SPAN" in env:               # the last wave's span hangs over the end of the cells
        assert n_cells(trs[0], cpd) % (int(env["GW_DIRTY_SPAN"]) * NWAVE) != 0
    with gpuaoi.GpuAOI(0) as g:              # gw_init reads the knobs
        ticks, cols = run_and_check(g, trs, mode, capfd, cells_per_d=cpd,
                                    sample=range(0, trs[0].capacity, 7) if len(trs) > 1 or name == "D" else None)
    f = row["fields"]
    diff = row["diff"] or DIFF_DEFAULT[name]
    assert [t["diff"] for t in ticks] == [diff] * len(ticks)
    write = row["write"] if row["write"] is not None or "gdirect" in f else WRITE_DEFAULT[name]
    got = [c["write"] for c in cols]
    assert set(got) <= WRITE_TOKENS
    if write is not None:
        assert got == [write] * len(cols)
    G = int(max(int(tr.gates.max()) for tr in trs)) + 1
    small = f.get("small", 1 if len(trs) > 1 else 0)
    gdirect = f.get("gdirect", 1 if 2 < G <= 16 and not small else 0)
    for c in cols:
        assert (int(c["G"]), int(c["small"]), int(c["gdirect"]), int(c["nb_u"])) == (G, small, gdirect, f.get("nb_u", 4))
    if not gdirect and not small and write is None:     # the plain write pass, whole waves or half-waves
        assert set(got) <= {"k_sync_write<4>", "k_sync_write_h<4>"}
    heavy = f.get("heavy")
    if heavy:                                # primaries listed heavy-first, of the tick's movers
        hv = [(int(t["heavy"]), int(t["movers"])) for t in ticks]
        if heavy == "none":
            assert all(h == 0 for h, m in hv)
        elif heavy in ("all", "some"):       # D: every mover has >= 64 candidates (test_dense_trace_...); A: an
            assert all(0 < h == m for h, m in hv) if name == "D" else all(h <= m for h, m in hv)   # Enter + Leave
        else:                                # both sides of the threshold in one tick (test_dense_trace_...)
            assert all(0 < h < m for h, m in hv)


def _candidate_brackets(tr):
    """Per tick, for every mover of a Moved-only one-space trace: a lower and an
    upper bound of its candidate count (k_bounds: the entries of the grid and of
    the mover grid in the cells of its old and new windows).  Lower: the
    entities whose new position is within d of the mover's on both axes (they
    lie in its new window's cells).  Upper: new positions, and movers' old
    ones, within 2 d of its old or new position (the cells of a window reach
    less than d + one cell = 1.5 d from its centre)."""
    d = float(tr.d)
    x, z = tr.init_x.astype(np.float64), tr.init_z.astype(np.float64)
    out = []
    for ops in tr.ticks:
        assert np.all(ops["kind"] == T.OP_MOVED) and len(np.unique(ops["slot"])) == len(ops)
        ox, oz = x.copy(), z.copy()
        x[ops["slot"]], z[ops["slot"]] = ops["x"], ops["z"]
        mv = ops["slot"]
        lo, hi = [], []
        for s in mv:
            lo.append(int(np.sum((abs(x - x[s]) <= d) & (abs(z - z[s]) <= d))))
            near = lambda px, pz: (((abs(px - x[s]) <= 2 * d) & (abs(pz - z[s]) <= 2 * d)) |
                                   ((abs(px - ox[s]) <= 2 * d) & (abs(pz - oz[s]) <= 2 * d)))
            hi.append(int(np.sum(near(x, z)) + np.sum(near(ox[mv], oz[mv]))))
        out.append((np.array(lo), np.array(hi)))
    return out


def test_dense_trace_straddles_heavy_threshold():
    """Trace D (n = 2000) has, in every tick, movers surely below the default
    heavy-first threshold of 512 candidates and movers surely at or above 64;
    whether some are surely above 512 cannot be told from the neighbour counts
    (at most ~320 here, the candidate cells hold about 2.25 times as many), so
    the GPU row "heavy-default" asserts the mix from the library's own count
    (0 < heavy < movers on every tick)."""
    (tr,), _ = traces("D")
    for lo, hi in _candidate_brackets(tr):
        assert (hi < HEAVY_DEFAULT).sum() >= 10          # surely not heavy
        assert (lo >= 64).all()                          # every mover is heavy at GW_HEAVY_MIN=64
        assert hi.max() >= 2 * HEAVY_DEFAULT             # ... and the dense middle is far above


@pytest.mark.gpu
def test_by_client_collect_names_the_pairs_kernel(monkeypatch, capfd):
    """GW_SYNC_BY_CLIENT on trace A: the write pass leaves (watcher, entity)
    pairs (k_sync_write<4,true>) whatever the gate layout; the records equal the
    oracle's in (gate, watcher, entity) order after every tick."""
    monkeypatch.setenv("GW_DEBUG_STATS", "1")
    (tr,), mode = traces("A")
    o = pyorc.OracleSpace(tr.capacity, tr.d, mode)
    pyorc.load_trace(o, tr)
    capfd.readouterr()
    with gpuaoi.GpuAOI(0) as g:
        gpuaoi.load_space(g, tr)
        for t in range(-1, len(tr.ticks)):
            if t >= 0:
                g.submit(tr.ticks[t])
                g.tick(copy=False)
                assert o.tick(tr.ticks[t]) == 0
            exp = o.collect()
            exp = exp[np.lexsort((exp["entity"], exp["watcher"], tr.gates[exp["watcher"]]))]
            assert g.sync_collect(by_client=True).records.tobytes() == exp.tobytes(), f"tick {t}"
    ticks, cols = parse_stats(capfd.readouterr().err)
    assert len(cols) == len(tr.ticks) + 1
    assert all(c["write"] == "k_sync_write<4,true>" and c["gdirect"] == "0" for c in cols)
