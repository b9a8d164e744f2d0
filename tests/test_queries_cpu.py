"""CPU tests of the batched InterestedIn queries (gw_set_tags,
gw_neighbors_batch, gw_nearest, gw_related): the ABI surface, and the numpy
reference model (tests/query_model.py) the GPU tests hold the kernels to,
pinned here to hand-computed answers."""
import ctypes
import os
import re

import numpy as np

import query_model as M
from goworld_amd import gpuaoi
from oracle import pyorc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY_SYMBOLS = ("gw_set_tags", "gw_neighbors_batch", "gw_nearest", "gw_related")


def test_symbols_exported_and_abi_version_unchanged():
    L = gpuaoi.lib()
    for s in QUERY_SYMBOLS:
        assert hasattr(L, s), s
        assert s in gpuaoi.EXPORTED
    assert L.gw_abi_version() == 15          # no existing struct changed layout


def test_struct_sizes_match_the_header():
    assert gpuaoi.NEAREST_DTYPE.itemsize == 16 == M.NEAREST_DTYPE.itemsize      # gw_nearest_rec
    assert gpuaoi.NEAREST_DTYPE == M.NEAREST_DTYPE
    # the header's structs compiled by the C compiler against the ctypes mirrors
    import subprocess
    import tempfile
    src = ('#include <stdio.h>\n#include "gpuaoi.h"\nint main(void){printf("%zu %zu %zu %u %u %u %u\\n",'
           "sizeof(gw_nearest_rec),sizeof(gw_nbr_out),sizeof(gw_near_out),GW_NO_SLOT,GW_QUERY_COPY_TO_HOST,"
           "GW_QUERY_GENERAL_ORDER,GW_QUERY_SLOTS_ON_DEVICE);return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, c], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:3] == [16, ctypes.sizeof(gpuaoi.NbrOut), ctypes.sizeof(gpuaoi.NearOut)]
    assert got[3:] == [gpuaoi.NO_SLOT, gpuaoi.QUERY_COPY_TO_HOST, gpuaoi.QUERY_GENERAL_ORDER,
                       gpuaoi.QUERY_SLOTS_ON_DEVICE]
    assert ctypes.sizeof(gpuaoi.NbrOut) == 64 and ctypes.sizeof(gpuaoi.NearOut) == 40


def test_tier_bounds_exposed_by_the_binding_are_the_kernels():
    src = open(os.path.join(ROOT, "goworld_amd", "csrc", "gw_internal.hpp")).read()
    wave = int(re.search(r"constexpr uint32_t QL_WAVE_MAX = (\d+);", src).group(1))
    lds = int(re.search(r"constexpr uint32_t QL_LDS_MAX = (\d+);", src).group(1))
    assert gpuaoi.QUERY_TIER_BOUNDS == (wave, lds)


def test_no_query_knob_in_the_environment():
    for f in ("query.hip", "capi.cpp"):
        src = open(os.path.join(ROOT, "goworld_amd", "csrc", f)).read()
        assert not re.search(r'getenv\("GW_Q', src)


def test_model_distance_known_answers():
    d2 = M.d2_f32((0, 0, 0), [(3, 0, 4)])
    assert d2.dtype == np.float32 and d2[0] == 25.0 and M.dist_f32(d2)[0] == 5.0
    # Y counts: (1, 1000, 1) is far although it is next to the origin in x and z
    d2 = M.d2_f32((0, 0, 0), [(1, 1000, 1), (50, 0, 50)])
    assert d2[0] == np.float32(1000002.0) and d2[1] == np.float32(5000.0) and d2[1] < d2[0]
    # the order of the float32 roundings: fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz))
    q, p = np.zeros(3, np.float32), np.array([0.1, 0.2, 0.3], np.float32)
    want = np.float32(np.float32(np.float32(p[0] * p[0]) + np.float32(p[1] * p[1])) + np.float32(p[2] * p[2]))
    assert M.d2_f32(q, [p])[0].tobytes() == want.tobytes()


def test_model_nearest_over_oracle_sets():
    """The sets come from oracle.pyorc.OracleSpace.neighbors; the candidate at
    (1, 1000, 1) is in the set (Y does not count in AOI) but loses to (50, 0, 50)."""
    o = pyorc.OracleSpace(8, 100.0, pyorc.XZLIST)
    x = np.array([0, 1, 50, 400], np.float32)
    y = np.array([0, 1000, 0, 0], np.float32)
    z = np.array([0, 1, 50, 0], np.float32)
    o.bulk_enter(np.arange(4, dtype=np.uint32), x, y, z, np.zeros(4, np.float32))
    lists = M.oracle_lists(o, 0)
    assert [l.tolist() for l in lists[:4]] == [[1, 2], [0, 2], [0, 1], []]
    pos = np.zeros((8, 3), np.float32)
    pos[:4] = np.stack([x, y, z], 1)
    tags = np.array([0, 1, 1, 1, 0, 0, 0, 0], np.uint32)
    r = M.nearest(pos, tags, [0, 3, 5], [lists[0], lists[3], lists[5]])
    assert r[0].tolist() == (2, 2, M.dist_f32(np.float32(5000.0)), 5000.0)
    assert r[1].tolist() == (M.NO_SLOT, 0, np.inf, np.inf)       # present, nobody in range
    assert r[2].tolist() == (M.NO_SLOT, 0, np.inf, np.inf)       # absent
    # tag filter: only slot 1 matches (tag & 1) == 1 and y < 1000 is not asked: it wins alone
    tags2 = np.array([0, 1, 0, 0, 0, 0, 0, 0], np.uint32)
    r = M.nearest(pos, tags2, [0], [lists[0]], mask=1, value=1)
    assert (r[0]["slot"], r[0]["count"], r[0]["d2"]) == (1, 1, np.float32(1000002.0))
    # equal d2: the lowest slot
    pos2 = np.array([[0, 0, 0], [30, 0, 0], [-30, 0, 0]], np.float32)
    assert M.nearest_one(pos2, np.zeros(3, np.uint32), 0, [1, 2])[:2] == (1, 2)
    off, nbr = M.csr(lists[:4])
    assert off.tolist() == [0, 2, 4, 6, 6] and nbr.tolist() == [1, 2, 0, 2, 0, 1]
    off, nbr = M.csr(lists[:4], tags2, 1, 1)
    assert off.tolist() == [0, 1, 1, 2, 2] and nbr.tolist() == [1, 1]


def test_vectorised_model_equals_the_per_query_one():
    rng = np.random.default_rng(4)
    n = 400
    pos = (rng.integers(-40, 40, (n, 3)) * 0.37).astype(np.float32)     # many equal distances
    tags = rng.integers(0, 4, n).astype(np.uint32)
    lists = [np.unique(rng.integers(0, n, rng.integers(0, 30))).astype(np.uint32) for _ in range(n)]
    lists = [l[l != k] for k, l in enumerate(lists)]
    q = np.arange(n)
    off, nbr = M.csr(lists)
    for mask, value in ((0, 0), (3, 1), (3, 7)):
        a = M.nearest(pos, tags, q, lists, mask, value)
        b = M.nearest_csr(pos, tags, q, off, nbr, mask, value)
        assert a.tobytes() == b.tobytes()
    assert (a["slot"] == M.NO_SLOT).all() and (M.nearest(pos, tags, q, lists)["count"] > 0).any()


def test_two_sqrt_forms_agree_on_a_seeded_million():
    rng = np.random.default_rng(20)
    d2 = (rng.random(1_000_000) * 40000.0).astype(np.float32)
    assert np.array_equal(M.dist_f32(d2), M.dist_f32_direct(d2))


def test_fma_sensitive_pair_still_flips():
    p = np.array([M.FMA_PAIR_A, M.FMA_PAIR_B], np.float32)
    plain, fused = M.d2_f32((0, 0, 0), p), M.d2_fused((0, 0, 0), p)
    assert plain[0] != plain[1] and fused[0] != fused[1]
    assert (plain[0] < plain[1]) != (fused[0] < fused[1]), (plain, fused)
