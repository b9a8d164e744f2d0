"""GPU: the per-mover sort tiers and the cell-merge tiers at their boundaries.

A mover's own events are sorted by the cheapest tier that holds them: placed by
rank up to GW_RANK_SORT (12), a wave sort up to 64, a bitonic sort in LDS up to
1024, the block sort of the `big` list above (general path; 12 / 32 / big on
the half-wave paths; 256 in LDS for k_mover_small<2,false>).  A dirty cell is
merged by rank up to 64 arrivals per tick, compacted and sorted above.  The
traces here are built by hand so that movers get exactly k events for the k on
both sides of every boundary; the counts are taken from the oracle's events
before anything is compared, and the `big` field of the library's
GW_DEBUG_STATS line must equal the number of movers above the top tier.
Events, records and neighbour lists are compared bit for bit as in
test_gpu_parity.py.
"""
import numpy as np
import pytest

from goworld_amd import gpuaoi, traces as T
from oracle import pyorc

from test_gpu_parity import Harness
from test_gpu_variants import parse_stats

pytestmark = pytest.mark.gpu

D = 10.0
SMALL_LDS_MAX = 48 * 1024          # gw_internal.hpp
GENT = 16                          # bytes of a grid entry

# knobs set here (tests/test_knob_inventory.py places each GW_* name)
TIER_KNOBS = ["GW_RANK_SORT", "GW_MOVER_COMPACT", "GW_PAIR_MAX", "GW_MOVER_HALVES", "GW_DIRTY_SPAN"]


def clump_trace(ks, bounds=None):
    """Clump i: ks[i] stationary entities at distinct dyadic positions inside a
    square of side 33/64 around (40 i, 0), a corner of four grid cells, laid
    out against the slot order: a walk meets them row by row and cell by cell,
    so a mover's own events arrive unsorted and each tier has to sort them
    (inside one cell they would arrive in slot order, already sorted).  Mover i
    is parked at (40 i, 40), more than 3 d from everything.  Tick 1: every mover jumps into its clump (k enters
    as watcher, k mirror events); tick 2: on to the next clump (k_i leaves +
    k_i+1 enters in one run); tick 3: back to its parking place.  Every entity
    has a client.  Returns (trace, mover slots)."""
    n = sum(ks) + len(ks)
    x, z = np.zeros(n, np.float32), np.zeros(n, np.float32)
    s = 0
    for i, k in enumerate(ks):
        q = k - 1 - np.arange(k)                          # positions against the slot order
        a, b = q % 33, q // 33                           # (a, b) -> (17 a mod 33, b + 5 a mod 32): distinct, and
        x[s:s + k] = 40.0 * i - 0.25 + ((17 * a) % 33) / 64.0     # a few entities already fall on both sides
        z[s:s + k] = -0.25 + ((b + 5 * a) % 32) / 64.0            # of the cell edges x = 40 i and z = 0
        s += k
    movers = np.arange(s, n, dtype=np.uint32)
    park_x = 40.0 * np.arange(len(ks), dtype=np.float32)
    x[s:], z[s:] = park_x, 40.0
    if bounds is None:
        bounds = (-1000.0, -1000.0, 1000.0, 1000.0)      # the default bounds
    tr = T.SpaceTrace(n=n, capacity=n, d=D, bounds=bounds, init_slots=np.arange(n, dtype=np.uint32),
                      init_x=x, init_y=np.zeros(n, np.float32), init_z=z, init_yaw=np.zeros(n, np.float32),
                      ticks=[], gates=np.ones(n, np.uint16))
    for dest in (np.arange(len(ks)), (np.arange(len(ks)) + 1) % len(ks), None):
        ops = T.make_ops(len(ks))
        ops["kind"] = T.OP_MOVED
        ops["sync_flags"] = 3
        ops["slot"] = movers
        if dest is None:
            ops["x"], ops["z"] = park_x, 40.0
        else:
            ops["x"], ops["z"] = 40.0 * dest + 0.125, 0.125
        tr.ticks.append(ops)
    return tr, movers


def expected_own(ks):
    """Events per mover as watcher in ticks 1..3."""
    k = np.array(ks)
    return [k, k + np.roll(k, -1), np.roll(k, -1)]


def run_clumps(g, spaces, top, capfd, diff):
    """spaces: [(trace, movers, ks)].  Counts the oracle's events per mover as
    watcher (exactly the intended k, k_i + k_i+1, k_i+1), compares everything,
    and checks `big` (movers with more than `top` own events) and the diff
    kernel on every tick line."""
    capfd.readouterr()
    h = Harness(g, [tr for tr, _, _ in spaces], mode=pyorc.XZLIST)
    h.check_collect()
    bigs = []
    for t in range(3):
        h.step(t)
        big = 0
        for (tr, movers, ks), o in zip(spaces, h.orcs):
            e, l = o.events()                            # (the tick's events stay until the next tick)
            per = np.bincount(np.concatenate([e["watcher"], l["watcher"]]), minlength=tr.capacity)[movers]
            assert np.array_equal(per, expected_own(ks)[t]), (t, per)
            big += int(np.sum(per > top))
        bigs.append(big)
        h.check_collect()
    for i, (tr, movers, ks) in enumerate(spaces):           # the movers' lists and every 13th entity's
        for s in sorted(set(movers.tolist()) | set(range(0, tr.capacity, 13))):
            got = g.neighbors(h.bases[i] + s)
            assert np.array_equal(got, h.orcs[i].neighbors(s).astype(np.uint32) + h.bases[i]), s
    ticks, cols = parse_stats(capfd.readouterr().err)
    assert [t["diff"] for t in ticks] == [diff] * 3
    assert [int(t["big"]) for t in ticks] == bigs and max(bigs) > 0
    return cols


OWN_KS = [1, 2, 12, 13, 63, 64, 65, 1023, 1024, 1025]


@pytest.mark.parametrize("env,diff", [({}, "k_mover_c<2,0,0>"), ({"GW_RANK_SORT": "0"}, "k_mover_c<2,0,0>"),
                                      ({"GW_MOVER_COMPACT": "0"}, "k_mover<2,1>")],
                         ids=["default", "rank-sort0", "compact0"])
def test_own_event_tiers(env, diff, monkeypatch, capfd):
    """General path: 12 | 13 (rank placement), 64 | 65 (wave sort), 1024 | 1025
    (LDS bitonic), both as k and as sums k_i + k_i+1 (3 .. 2049).  Ten ops
    with thousands of candidates overflow the first attempt's own-event
    regions, so the tick line reports a redone diff."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("GW_DEBUG_STATS", "1")
    tr, movers = clump_trace(OWN_KS)
    with gpuaoi.GpuAOI(0) as g:
        run_clumps(g, [(tr, movers, OWN_KS)], 1024, capfd, diff)


HALF_KS = [12, 13, 31, 32, 33]
SMALL_BOUNDS = (-20.0, -20.0, 220.0, 80.0)          # 48 x 20 cells of 5: a space's grids fit in LDS


def _small_fits(tr):
    b = tr.bounds
    cells = int(np.ceil((b[2] - b[0]) / (D / 2))) * int(np.ceil((b[3] - b[1]) / (D / 2)))
    return tr.capacity * GENT + 2 * (cells + 1) * 4 <= SMALL_LDS_MAX       # capi.cpp small_mode


def test_half_wave_tiers_small_spaces(monkeypatch, capfd):
    """k_mover_small<2,true>: two movers per wave, 12 | 13 by rank, 32 | 33 in
    the half's registers or on the big list."""
    monkeypatch.setenv("GW_DEBUG_STATS", "1")
    spaces = []
    for ks in (HALF_KS, HALF_KS[::-1]):
        tr, movers = clump_trace(ks, SMALL_BOUNDS)
        assert _small_fits(tr)
        spaces.append((tr, movers, ks))
    with gpuaoi.GpuAOI(0) as g:
        cols = run_clumps(g, spaces, 32, capfd, "k_mover_small<2,1>")
    assert all(c["small"] == "1" and c["write"] == "k_sync_write_small2" for c in cols)


def test_half_wave_tiers_pairs(monkeypatch, capfd):
    """k_mover_pair<2> (GW_PAIR_MAX=96): the same tiers in one space."""
    monkeypatch.setenv("GW_DEBUG_STATS", "1")
    monkeypatch.setenv("GW_PAIR_MAX", "96")
    tr, movers = clump_trace(HALF_KS)
    with gpuaoi.GpuAOI(0) as g:
        run_clumps(g, [(tr, movers, HALF_KS)], 32, capfd, "k_mover_pair<2>")


def test_small_sort_tier(monkeypatch, capfd):
    """k_mover_small<2,false> (GW_MOVER_HALVES=0): own events sorted in a wave's
    256 LDS words, 256 | 257 and the sums 511 .. 513 on the big list."""
    monkeypatch.setenv("GW_DEBUG_STATS", "1")
    monkeypatch.setenv("GW_MOVER_HALVES", "0")
    spaces = []
    for ks in ([255, 256, 257], [257, 255, 256]):
        tr, movers = clump_trace(ks, SMALL_BOUNDS)
        assert _small_fits(tr)
        spaces.append((tr, movers, ks))
    with gpuaoi.GpuAOI(0) as g:
        cols = run_clumps(g, spaces, 256, capfd, "k_mover_small<2,0>")
    assert all(c["small"] == "1" for c in cols)


# --------------------------------------------------------------------------- cell merge
def merge_trace(narr):
    """Cell C1 = [100, 105)^2 holds 70 entities with slots 3 j + 1; 5 of them
    leave it in tick 1, in which narr entities arrive there (slots below,
    between and above the kept ones) and narr more in the empty cell C2 =
    [300, 305)^2.  Ticks 2 and 3 move one entity inside each cell, so the
    merged cells' order (gidx) is used again."""
    kept = 3 * np.arange(70) + 1                              # 1 .. 208
    free = np.setdiff1d(np.arange(0, 3 * 70 + 2 * narr + 8), kept)
    # arrivals of C1: slot 0 (below every kept one), slots between, slots above 208
    above = free[free > kept.max()]
    between = free[(free > 0) & (free < kept.max())]
    n_mid = (narr - 1) // 2
    a1 = np.concatenate([[0], between[:n_mid], above[:narr - 1 - n_mid]])
    rest = np.setdiff1d(free, a1)
    a2 = rest[:narr]
    slots = np.concatenate([kept, a1, a2]).astype(np.uint32)
    assert len(np.unique(slots)) == len(slots) and len(a1) == len(a2) == narr
    assert a1.min() < kept.min() and (narr < 3 or (a1.max() > kept.max() and np.any((a1 > 1) & (a1 < 208))))
    cap = int(slots.max()) + 1
    j = np.arange(70)
    kx, kz = 100.25 + 0.5 * (j % 9), 100.25 + 0.5 * (j // 9)
    # the arrivals wait on a line far from both cells, 3 apart
    q = np.arange(2 * narr)
    px, pz = -600.0 + 3.0 * q, np.full(2 * narr, -500.0)
    tr = T.SpaceTrace(n=len(slots), capacity=cap, d=D, bounds=(-1000.0, -1000.0, 1000.0, 1000.0),
                      init_slots=slots, init_x=np.concatenate([kx, px]).astype(np.float32),
                      init_y=np.zeros(len(slots), np.float32), init_z=np.concatenate([kz, pz]).astype(np.float32),
                      init_yaw=np.zeros(len(slots), np.float32), ticks=[], gates=np.zeros(cap, np.uint16))
    tr.gates[slots] = 1
    i = np.arange(narr)
    ops = T.make_ops(2 * narr + 5)
    ops["kind"] = T.OP_MOVED
    ops["sync_flags"] = 3
    ops["slot"] = np.concatenate([a1[::-1], kept[[3, 20, 34, 51, 69]], a2[::-1]])   # arrival order != slot order
    ops["x"] = np.concatenate([100.0 + 0.5 * (i % 9), [700.0, 710.0, 720.0, 730.0, 740.0], 300.0 + 0.5 * (i % 9)])
    ops["z"] = np.concatenate([100.0 + 0.5 * (i // 9), [700.0] * 5, 300.0 + 0.5 * (i // 9)])
    tr.ticks.append(ops)
    for t, (s1, s2) in enumerate([(kept[0], a2[0]), (a1[-1], a2[-1])]):
        ops = T.make_ops(2)
        ops["kind"] = T.OP_MOVED
        ops["sync_flags"] = 3
        ops["slot"] = [s1, s2]
        ops["x"] = [104.5 + 0.125 * t, 304.5 + 0.125 * t]
        ops["z"] = [104.5, 304.5]
        tr.ticks.append(ops)
    return tr


@pytest.mark.parametrize("span", [None, 1, 64])
@pytest.mark.parametrize("narr", [1, 63, 64, 65])
def test_cell_merge_tiers(narr, span, monkeypatch):
    """Rank merge up to 64 arrivals of a cell in one tick, compaction + bitonic
    sort above; into a cell that keeps 65 of 70 entries and into an empty one;
    with the default dirty-cell span, one cell per wave and 64."""
    if span is not None:
        monkeypatch.setenv("GW_DIRTY_SPAN", str(span))
    tr = merge_trace(narr)
    with gpuaoi.GpuAOI(0) as g:
        h = Harness(g, [tr], mode=pyorc.XZLIST)
        h.check_collect()
        for t in range(len(tr.ticks)):
            h.step(t)
            h.check_collect()
        h.check_lists(sample=[int(s) for s in tr.init_slots])
