"""GPU tests of the batched InterestedIn queries (gw_set_tags,
gw_neighbors_batch, gw_nearest, gw_related) through the C ABI, against the CPU
oracle's sets (ORC_XZLIST on the small and adversarial inputs, ORC_SEQRULE
otherwise) and the numpy model of the reference's distance pinned in
test_queries_cpu.py.  The GPU's lists are compared raw: no re-sort here.

No test provokes a fault: every error case is one the host rejects before any
launch, and the device-resident out-of-range slot is stopped by the kernels'
own bounds check.
"""
import numpy as np
import pytest

import query_model as M
from goworld_amd import gpuaoi, traces as T
from oracle import pyorc

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
BOUNDS = (-1000.0, -1000.0, 1000.0, 1000.0)


@pytest.fixture(scope="module")
def ctx_factory():
    made = []

    def make():
        g = gpuaoi.GpuAOI(0)
        made.append(g)
        return g
    yield make
    for g in made:
        g.close()


def enter(g, base, slots, xyz, kind=T.OP_ENTER, tick=True):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    ops = T.make_ops(len(slots))
    ops["kind"] = kind
    ops["sync_flags"] = 3
    ops["slot"] = np.asarray(slots, np.uint32) + np.uint32(base)
    ops["x"], ops["y"], ops["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    g.submit(ops)
    if tick:
        g.tick(copy=False)
    return ops


def leave(g, base, slots, tick=True):
    ops = T.make_ops(len(slots))
    ops["kind"] = T.OP_LEAVE
    ops["slot"] = np.asarray(slots, np.uint32) + np.uint32(base)
    g.submit(ops)
    if tick:
        g.tick(copy=False)


def split(off, nbr):
    return [nbr[int(off[k]):int(off[k + 1])].tolist() for k in range(len(off) - 1)]


def rec_tuple(r):
    return (int(r["slot"]), int(r["count"]), r["dist"].tobytes(), r["d2"].tobytes())


def assert_nearest_equal(got, exp):
    assert np.array_equal(got["slot"], exp["slot"])
    assert np.array_equal(got["count"], exp["count"])
    assert got["d2"].tobytes() == exp["d2"].tobytes()            # by bits
    assert got["dist"].tobytes() == exp["dist"].tobytes()


class Tracker:
    """Positions (x, y, z) of global slots as of the last flush, from the ops
    (as test_gpu_parity.Harness tracks x and z): the last non-Leave op of a slot."""

    def __init__(self, slots):
        self.pos = np.zeros((slots, 3), np.float32)

    def load(self, tr, base):
        s = tr.init_slots.astype(np.int64) + base
        self.pos[s, 0], self.pos[s, 1], self.pos[s, 2] = tr.init_x, tr.init_y, tr.init_z

    def track(self, ops, base):
        sel = np.nonzero(ops["kind"] != T.OP_LEAVE)[0]
        s = ops["slot"][sel].astype(np.int64) + base
        # several ops on one slot: the last one stays
        _, last = np.unique(s[::-1], return_index=True)
        sel = sel[::-1][last]
        s = ops["slot"][sel].astype(np.int64) + base
        self.pos[s, 0], self.pos[s, 1], self.pos[s, 2] = ops["x"][sel], ops["y"][sel], ops["z"][sel]


# ---- known answers ------------------------------------------------------------

def test_known_answers_through_the_abi(ctx_factory):
    g = ctx_factory()
    sid, b = g.create_space(100.0, 8, BOUNDS)
    enter(g, b, [0, 1, 2, 3, 4], [(0, 0, 0), (1, 1000, 1), (50, 0, 50), (400, 0, 0), (403, 0, 4)])
    off, nbr = g.neighbors_batch(np.arange(8, dtype=np.uint32) + b)
    assert split(off, nbr) == [[b + 1, b + 2], [b, b + 2], [b, b + 1], [b + 4], [b + 3], [], [], []]
    r = g.nearest(np.array([0, 3, 5], np.uint32) + b)
    # (1, 1000, 1) is in the set but loses to (50, 0, 50): Y counts in the distance
    assert rec_tuple(r[0]) == (b + 2, 2, M.dist_f32(np.float32(5000.0)).tobytes(), np.float32(5000.0).tobytes())
    # (3, 0, 4) away: d2 = 25, dist = 5
    assert rec_tuple(r[1]) == (b + 4, 1, np.float32(5.0).tobytes(), np.float32(25.0).tobytes())
    assert rec_tuple(r[2]) == (gpuaoi.NO_SLOT, 0, INF.tobytes(), INF.tobytes())
    assert g.related([b, b + 1, b, b + 3], [b + 2, b, b + 3, b + 4]).tolist() == [True, True, False, True]


def test_fma_sensitive_pair(ctx_factory):
    """Two candidates whose order under the unfused float32 d2 is the reverse of
    their order under fused multiply-adds: the kernel must not contract."""
    g = ctx_factory()
    sid, b = g.create_space(100.0, 4, BOUNDS)
    pos = np.zeros((b + 4, 3), np.float32)
    pos[b + 1], pos[b + 2] = M.FMA_PAIR_A, M.FMA_PAIR_B
    enter(g, b, [0, 1, 2], pos[b:b + 3])
    exp = M.nearest(pos, np.zeros(b + 4, np.uint32), [b], [np.array([b + 1, b + 2], np.uint32)])
    fused = M.d2_fused(pos[b], pos[b + 1:b + 3])
    assert exp["slot"][0] == b + 1 + int(np.argmax(fused))       # the fused order would pick the other one
    assert_nearest_equal(g.nearest([b]), exp)


# ---- list lengths across every boundary of the implementation -----------------

def _tier_lengths():
    lens = {0, 1}
    for bound in gpuaoi.QUERY_TIER_BOUNDS:                       # read from the binding, not retyped
        lens |= {bound - 1, bound, bound + 1}
    return sorted(lens)


@pytest.fixture(scope="module")
def crowd(ctx_factory):
    """One space per list length L: L + 1 entities within d of one another but
    spread over four grid cells, so the walk's (cell, slot) order is not slot
    order; each has the L others as its list."""
    assert {0, 1, 63, 64, 65} <= set(_tier_lengths())            # a wave's width is a bound whatever the tiers
    g = ctx_factory()
    spaces = [(g.create_space(100.0, L + 1, BOUNDS)[1], L + 1) for L in _tier_lengths()]   # (base, entities)
    for b, n in spaces:
        s = np.arange(n)
        xyz = np.stack([(s * 7 % 10) * 10.0, s % 3, (s * 3 % 10) * 10.0], 1)
        enter(g, b, s, xyz, tick=False)
    g.tick(copy=False)
    return g, spaces


@pytest.mark.parametrize("general", [False, True])
def test_list_lengths_across_tier_bounds(crowd, general):
    g, spaces = crowd
    q = np.concatenate([np.arange(b, b + n, dtype=np.uint32) for b, n in spaces])
    exp = [np.delete(np.arange(b, b + n, dtype=np.uint32), i) for b, n in spaces for i in range(n)]
    off, nbr = g.neighbors_batch(q, general=general)
    eoff, enbr = M.csr(exp)
    assert np.array_equal(off, eoff)
    assert np.array_equal(nbr, enbr)                             # raw: ordered on the device
    # a filtered list of each length class, too: odd slots only
    tags = np.zeros(int(q.max()) + 1, np.uint32)
    tags[q] = q & 1
    g.set_tags(q, tags[q])
    off, nbr = g.neighbors_batch(q, mask=1, value=1, general=general)
    eoff, enbr = M.csr(exp, tags, 1, 1)
    assert np.array_equal(off, eoff) and np.array_equal(nbr, enbr)


def test_walk_order_is_not_slot_order(ctx_factory):
    """Two candidates at equal d2, the higher slot in the earlier grid cell: the
    lower slot is chosen, and the list is in slot order."""
    g = ctx_factory()
    sid, b = g.create_space(100.0, 4, BOUNDS)                    # cells are 50 wide from -1000
    enter(g, b, [0, 1, 2], [(10, 0, 10), (40, 0, 10), (-20, 0, 10)])   # slot 2: the cell before the query's
    r = g.nearest([b])[0]
    assert rec_tuple(r) == (b + 1, 2, np.float32(30.0).tobytes(), np.float32(900.0).tobytes())
    for general in (False, True):
        off, nbr = g.neighbors_batch([b], general=general)
        assert nbr.tolist() == [b + 1, b + 2]


# ---- the one-ulp band -----------------------------------------------------------

def test_adversarial_band_lists_and_pairs_vs_xzlist(ctx_factory):
    tr = T.adversarial_trace(11, n=300, ticks=4)
    g = ctx_factory()
    g.create_space(100.0, 16, BOUNDS)                            # the traced space does not start at slot 0
    sid, b = gpuaoi.load_space(g, tr)
    o = pyorc.OracleSpace(tr.capacity, tr.d, pyorc.XZLIST)
    pyorc.load_trace(o, tr)
    q = np.arange(tr.capacity, dtype=np.uint32) + np.uint32(b)
    aa, bb = np.meshgrid(q, q, indexing="ij")
    for t in range(-1, len(tr.ticks)):
        if t >= 0:
            g.submit(T.with_global_slots(tr.ticks[t], b))
            g.tick(copy=False)
            assert o.tick(tr.ticks[t]) == 0
        lists = M.oracle_lists(o, b)
        eoff, enbr = M.csr(lists)
        for general in (False, True):
            off, nbr = g.neighbors_batch(q, general=general)
            assert np.array_equal(off, eoff) and np.array_equal(nbr, enbr), f"tick {t}"
        rel = np.zeros((tr.capacity, tr.capacity), bool)
        for i, l in enumerate(lists):
            rel[i, l - b] = True
        got = g.related(aa.ravel(), bb.ravel()).reshape(rel.shape)   # all ordered pairs
        assert np.array_equal(got, rel), f"tick {t}"
    assert enbr.size > 1000


# ---- a uniform trace ------------------------------------------------------------

def test_uniform_trace_lists_and_nearest(ctx_factory):
    tr = T.config2(ticks=2, n=20_000)
    rng = np.random.default_rng(77)
    tr.init_y = (rng.random(tr.capacity) * 60 - 30).astype(np.float32)
    for ops in tr.ticks:
        ops["y"] = (rng.random(len(ops)) * 60 - 30).astype(np.float32)
    g = ctx_factory()
    sid, b = gpuaoi.load_space(g, tr)
    o = pyorc.OracleSpace(tr.capacity, tr.d, pyorc.SEQRULE)
    pyorc.load_trace(o, tr)
    trk = Tracker(b + tr.capacity)
    trk.load(tr, b)
    q = np.arange(tr.capacity, dtype=np.uint32) + np.uint32(b)
    tags = np.zeros(b + tr.capacity, np.uint32)
    tags[q] = rng.integers(0, 3, tr.capacity).astype(np.uint32) | (rng.integers(0, 2, tr.capacity) << 8).astype(np.uint32)
    g.set_tags(q, tags[q])
    for t, ops in enumerate(tr.ticks):
        g.submit(T.with_global_slots(ops, b))
        g.tick(copy=False)
        assert o.tick(ops) == 0
        trk.track(ops, b)
        lists = M.oracle_lists(o, b)
        eoff, enbr = M.csr(lists)
        off, nbr = g.neighbors_batch(q)
        assert np.array_equal(off, eoff) and np.array_equal(nbr, enbr)
        # everyone; one of the three classes; a class with its "alive" bit
        for mask, value in ((0, 0), (0xFF, 1), (0x1FF, 0x102)):
            exp = M.nearest_csr(trk.pos, tags, q, eoff, enbr, mask, value)
            assert_nearest_equal(g.nearest(q, mask, value), exp)
            assert (exp["slot"] != M.NO_SLOT).sum() > 1000
        eoff, enbr = M.csr(lists, tags, 0xFF, 2)
        off, nbr = g.neighbors_batch(q, 0xFF, 2)
        assert np.array_equal(off, eoff) and np.array_equal(nbr, enbr)


# ---- edges ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def two_spaces(ctx_factory):
    """Two spaces with different d in one context: space A (d = 100) holds slots
    0..3 of 8, space B (d = 10) slots 0..2 of 8; A's slot 3 leaves in the last tick."""
    g = ctx_factory()
    sa, a = g.create_space(100.0, 8, BOUNDS)
    sb, b = g.create_space(10.0, 8, BOUNDS)
    enter(g, a, [0, 1, 2, 3], [(0, 0, 0), (60, 5, -20), (0, 0, 90), (30, 0, 30)])
    enter(g, b, [0, 1, 2], [(0, 0, 0), (8, 0, 0), (60, 0, 0)])
    leave(g, a, [3])
    return g, a, b


def test_never_entered_and_left_this_tick(two_spaces):
    g, a, b = two_spaces
    off, nbr = g.neighbors_batch([a + 5, a + 3, a])
    assert split(off, nbr) == [[], [], [a + 1, a + 2]]
    r = g.nearest([a + 5, a + 3])
    assert [rec_tuple(x) for x in r] == [(gpuaoi.NO_SLOT, 0, INF.tobytes(), INF.tobytes())] * 2
    assert g.related([a, a + 1], [a + 3, a + 5]).tolist() == [False, False]     # an absent member


def test_duplicate_query_slots(two_spaces):
    g, a, b = two_spaces
    off, nbr = g.neighbors_batch([a, a + 1, a, a])
    assert split(off, nbr) == [[a + 1, a + 2], [a], [a + 1, a + 2], [a + 1, a + 2]]
    r = g.nearest([a, a])
    assert rec_tuple(r[0]) == rec_tuple(r[1]) and r[0]["slot"] == a + 1


def test_no_queries(two_spaces):
    g, a, b = two_spaces
    off, nbr = g.neighbors_batch(np.zeros(0, np.uint32))
    assert off.tolist() == [0] and len(nbr) == 0
    assert len(g.nearest(np.zeros(0, np.uint32))) == 0
    assert len(g.related([], [])) == 0
    g.set_tags([], [])


def test_out_of_range_slot_is_refused_and_harmless(two_spaces):
    g, a, b = two_spaces
    total = g.context_info()["total_slots"]
    for call in (lambda: g.neighbors_batch([a, total]), lambda: g.nearest([total, a]),
                 lambda: g.related([a], [total]), lambda: g.related([total], [a]),
                 lambda: g.set_tags([a, total], [7, 7])):
        with pytest.raises(gpuaoi.GwError) as e:
            call()
        assert e.value.code == -5                                # GW_ERANGE
    # the next valid calls are unaffected, and the refused set_tags changed nothing
    off, nbr = g.neighbors_batch([a])
    assert nbr.tolist() == [a + 1, a + 2]
    assert g.nearest([a + 1], mask=0xFFFFFFFF, value=7)[0]["count"] == 0
    assert g.nearest([a + 1])[0]["slot"] == a


def test_several_spaces_with_different_d_in_one_call(two_spaces):
    g, a, b = two_spaces
    off, nbr = g.neighbors_batch([b, a, b + 2, a + 2])
    assert split(off, nbr) == [[b + 1], [a + 1, a + 2], [], [a]]
    r = g.nearest([b, a + 1])
    assert (r[0]["slot"], r[0]["d2"], r[1]["slot"]) == (b + 1, 64.0, a)
    assert r[1]["d2"].tobytes() == np.float32(4025.0).tobytes()  # 60*60 + 5*5 + 20*20: Y counts


def test_related_edges(two_spaces):
    g, a, b = two_spaces
    # a == b; different spaces (same coordinates); related; 110 apart in z
    assert g.related([a, a, a, a + 1], [a, b, a + 1, a + 2]).tolist() == [False, False, True, False]


def test_nobody_matches(two_spaces):
    g, a, b = two_spaces
    r = g.nearest([a], mask=0xFFFFFFFF, value=0xDEAD)
    assert rec_tuple(r[0]) == (gpuaoi.NO_SLOT, 0, INF.tobytes(), INF.tobytes())
    off, nbr = g.neighbors_batch([a], mask=0xFFFFFFFF, value=0xDEAD)
    assert off.tolist() == [0, 0] and len(nbr) == 0
    # mask 0 with a non-zero value matches nobody either: (tag & 0) == value is false
    assert g.nearest([a], mask=0, value=1)[0]["count"] == 0


def test_device_pointers_without_copy(two_spaces):
    g, a, b = two_spaces
    q = np.array([a, b, a + 1], np.uint32)
    off, nbr = g.neighbors_batch(q)
    o = g.neighbors_batch_raw(q, copy=False)
    assert not o.nbr and not o.off and o.nbr_dev and o.off_dev and (o.n_query, o.n_nbr) == (3, len(nbr))
    off2, nbr2 = np.zeros(4, np.uint64), np.zeros(len(nbr), np.uint32)
    g.d2h(off2, o.off_dev)
    g.d2h(nbr2, o.nbr_dev)
    assert np.array_equal(off2, off) and np.array_equal(nbr2, nbr)
    assert o.device_us > 0 and o.bytes_alg >= len(nbr) * 4 + 4 * 8
    r = g.nearest(q)
    o = g.nearest_raw(q, copy=False)
    assert not o.rec and o.rec_dev and o.n_query == 3
    r2 = np.zeros(3, gpuaoi.NEAREST_DTYPE)
    g.d2h(r2, o.rec_dev)
    assert r2.tobytes() == r.tobytes()


def test_device_slots_out_of_range_reads_as_absent(two_spaces):
    g, a, b = two_spaces
    q = np.array([a, 0xFFFFFFF0, g.context_info()["total_slots"], a + 1], np.uint32)
    dev = g.dev_alloc(q.nbytes)
    try:
        g.h2d(dev, q)
        off, nbr = g.neighbors_batch(dev, n=len(q))
        assert split(off, nbr) == [[a + 1, a + 2], [], [], [a]]
        r = g.nearest(dev, n=len(q))
        assert r["slot"].tolist() == [a + 1, gpuaoi.NO_SLOT, gpuaoi.NO_SLOT, a]
        assert r["count"].tolist() == [2, 0, 0, 1]
    finally:
        g.dev_free(dev)


# ---- tags -----------------------------------------------------------------------

def test_tags_lifecycle(ctx_factory):
    g = ctx_factory()
    sa, a = g.create_space(100.0, 8, BOUNDS)
    g.set_tags([a + 1, a + 2], [5, 6])                           # before Enter
    enter(g, a, [0, 1, 2], [(0, 0, 0), (50, 0, 0), (10, 0, 0)])
    assert g.nearest([a], 0xFF, 5)[0]["slot"] == a + 1
    assert g.nearest([a])[0]["slot"] == a + 2
    leave(g, a, [1])                                             # kept across Leave ...
    assert g.nearest([a], 0xFF, 5)[0]["slot"] == gpuaoi.NO_SLOT
    enter(g, a, [1], [(-20, 0, 0)])                              # ... and re-Enter
    r = g.nearest([a], 0xFF, 5)[0]
    assert (r["slot"], r["count"], r["d2"]) == (a + 1, 1, 400.0)
    # the tags follow a grow that moves the range (a second space sits behind the first)
    sb, b = g.create_space(100.0, 8, BOUNDS)
    g.set_tags([b], [5])
    enter(g, b, [0, 1], [(0, 0, 0), (1, 0, 0)])
    na = g.grow_space(sa, 32)
    assert na != a and na >= b + 8
    r = g.nearest([na, na + 2], 0xFF, 5)
    assert r["slot"].tolist() == [na + 1, na + 1]
    off, nbr = g.neighbors_batch([na], 0xFF, 6)
    assert nbr.tolist() == [na + 2]
    assert g.nearest([b + 1], 0xFF, 5)[0]["slot"] == b           # the other space's are where they were
    # a destroyed space's range is handed out again with zero tags
    leave(g, na, [0, 1, 2])
    g.destroy_space(sa)
    sc, c = g.create_space(100.0, 32, BOUNDS)
    assert c == na                                               # the range is reused
    enter(g, c, [0, 1, 2], [(0, 0, 0), (50, 0, 0), (10, 0, 0)])
    assert g.nearest([c], 0xFFFFFFFF, 0)[0]["count"] == 2        # every tag is zero
    assert g.nearest([c], 0xFF, 5)[0]["count"] == 0 and g.nearest([c], 0xFF, 6)[0]["count"] == 0


# ---- visibility -----------------------------------------------------------------

def test_queries_see_the_last_flush(ctx_factory):
    g = ctx_factory()
    sid, b = g.create_space(100.0, 8, BOUNDS)
    enter(g, b, [0, 1, 2], [(0, 0, 0), (50, 0, 0), (300, 0, 0)])
    before = (g.neighbors_batch([b])[1].tolist(), rec_tuple(g.nearest([b])[0]), g.related([b], [b + 2]).tolist())
    assert before[0] == [b + 1] and before[2] == [False]
    enter(g, b, [2], [(10, 0, 0)], kind=T.OP_MOVED, tick=False)  # submitted, not ticked: invisible
    assert (g.neighbors_batch([b])[1].tolist(), rec_tuple(g.nearest([b])[0]),
            g.related([b], [b + 2]).tolist()) == before
    g.tick(copy=False)
    assert g.neighbors_batch([b])[1].tolist() == [b + 1, b + 2] and g.nearest([b])[0]["slot"] == b + 2
    # a deferred tick is settled by the query
    ops = T.make_ops(1)
    ops["kind"], ops["sync_flags"], ops["slot"], ops["x"] = T.OP_MOVED, 3, b + 1, 5.0
    dev = g.dev_alloc(ops.nbytes)
    try:
        g.h2d(dev, ops)
        g.submit_device(dev, 1)
        g.tick(copy=False, defer=True)
        r = g.nearest([b])[0]
        assert (r["slot"], r["d2"]) == (b + 1, 25.0)
        g.submit_device(dev, 1)
        g.tick(copy=False, defer=True)
        assert g.related([b + 1], [b]).tolist() == [True]
        g.synchronize()
    finally:
        g.dev_free(dev)


# ---- agreement with the old call --------------------------------------------------

def test_batch_equals_gw_neighbors(ctx_factory):
    tr = T.config3(ticks=1, n=20_000, side=32768.0 * (0.02 ** 0.5))
    g = ctx_factory()
    sid, b = gpuaoi.load_space(g, tr)
    g.submit(T.with_global_slots(tr.ticks[0], b))
    g.tick(copy=False)
    q = np.arange(0, tr.capacity, 131, dtype=np.uint32) + np.uint32(b)
    off, nbr = g.neighbors_batch(q)
    for k, s in enumerate(q):
        assert np.array_equal(nbr[int(off[k]):int(off[k + 1])], g.neighbors(int(s)))
    assert len(nbr) > len(q)
