"""Reference model of the batched queries (gw_neighbors_batch, gw_nearest,
gw_related), in numpy over the oracle's sets.  Helper module of
test_queries_cpu.py (which pins it to hand-computed answers) and
test_gpu_queries.py (which holds the GPU to it).

Distance is the reference's Vector3.DistanceTo (engine/entity/Vector3.go:23-28,
reached from Entity.DistanceTo, Entity.go:254-256): Coord is float32, so
  dx, dy, dz = float32 differences of the two Positions (Y included)
  d2   = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz))     no fused multiply-add
  dist = float32(sqrt(float64(d2)))
numpy's float32 array arithmetic rounds every product and sum once, which is
exactly that.  The chosen entity minimises (d2, slot).
"""
import numpy as np

NO_SLOT = 0xFFFFFFFF
NEAREST_DTYPE = np.dtype([("slot", "<u4"), ("count", "<u4"), ("dist", "<f4"), ("d2", "<f4")])

# An FMA-sensitive pair, seen from the origin: under the unfused float32 d2
# candidate A is strictly nearer than B, under fma(dz,dz,fma(dy,dy,dx*dx)) B is
# strictly nearer than A (test_queries_cpu.py asserts that it still flips).
FMA_PAIR_A = (6.6971893, -40.345596, -14.688194)
FMA_PAIR_B = (14.345741, -37.345566, -16.966759)


def d2_f32(q, p):
    """Squared distance of positions p (n, 3) from q (3,), float32, unfused."""
    q = np.asarray(q, np.float32)
    p = np.asarray(p, np.float32).reshape(-1, 3)
    dx, dy, dz = p[:, 0] - q[0], p[:, 1] - q[1], p[:, 2] - q[2]
    xx, yy, zz = dx * dx, dy * dy, dz * dz
    return (xx + yy) + zz


def d2_fused(q, p):
    """What a contracting compiler would compute: fma(dz, dz, fma(dy, dy, dx*dx)),
    each fma rounded once (the exact product of two float32 fits a float64)."""
    q = np.asarray(q, np.float32)
    p = np.asarray(p, np.float32).reshape(-1, 3)
    dx, dy, dz = (p[:, i] - q[i] for i in range(3))
    xx = dx * dx
    s = (dy.astype(np.float64) * dy.astype(np.float64) + xx.astype(np.float64)).astype(np.float32)
    return (dz.astype(np.float64) * dz.astype(np.float64) + s.astype(np.float64)).astype(np.float32)


def dist_f32(d2):
    """Coord(math.Sqrt(float64(d2)))."""
    return np.sqrt(np.asarray(d2, np.float32).astype(np.float64)).astype(np.float32)


def dist_f32_direct(d2):
    """The correctly rounded float32 square root (the same value: the double
    rounding is harmless for sqrt at 53 >= 2 * 24 + 2 bits)."""
    return np.sqrt(np.asarray(d2, np.float32))


def matches(tags, slots, mask, value):
    return (tags[slots] & np.uint32(mask)) == np.uint32(value)


def nearest_one(pos, tags, q, nbrs, mask=0, value=0):
    """(slot, count, dist, d2) of query slot q; nbrs: its InterestedIn, ascending
    global slots; pos: (slots, 3) float32 Positions; tags: uint32 per slot."""
    nbrs = np.asarray(nbrs, np.uint32)
    m = nbrs[matches(tags, nbrs, mask, value)] if len(nbrs) else nbrs
    if len(m) == 0:
        return NO_SLOT, 0, np.float32(np.inf), np.float32(np.inf)
    d2 = d2_f32(pos[q], pos[m])
    i = int(np.argmin(d2))             # the first minimum: m ascends, so the lowest slot of the nearest
    return int(m[i]), len(m), dist_f32(d2[i:i + 1])[0], d2[i]


def nearest(pos, tags, queries, lists, mask=0, value=0):
    """NEAREST_DTYPE records for query slots `queries`; lists[k]: InterestedIn of queries[k]."""
    out = np.zeros(len(queries), NEAREST_DTYPE)
    for k, (q, nb) in enumerate(zip(queries, lists)):
        out[k] = nearest_one(pos, tags, int(q), nb, mask, value)
    return out


def nearest_csr(pos, tags, queries, off, nbr, mask=0, value=0):
    """The same from the unfiltered lists as a CSR, vectorised (the large traces):
    per list the first entry in (d2, slot) order among the matching ones."""
    queries = np.asarray(queries, np.int64)
    n = len(queries)
    out = np.zeros(n, NEAREST_DTYPE)
    out["slot"], out["dist"], out["d2"] = NO_SLOT, np.inf, np.inf
    seg = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    keep = matches(tags, nbr, mask, value)
    seg, w = seg[keep], nbr[keep]
    out["count"] = np.bincount(seg, minlength=n)
    q, p = pos[queries[seg]], pos[w]
    dx, dy, dz = p[:, 0] - q[:, 0], p[:, 1] - q[:, 1], p[:, 2] - q[:, 2]
    d2 = ((dx * dx + dy * dy) + dz * dz).astype(np.float32)
    order = np.lexsort((w, d2.view(np.uint32), seg))          # d2 >= 0: its bits order like its value
    seg_s = seg[order]
    first = order[np.r_[True, seg_s[1:] != seg_s[:-1]]] if len(order) else order
    out["slot"][seg[first]] = w[first]
    out["d2"][seg[first]] = d2[first]
    out["dist"][seg[first]] = dist_f32(d2[first])
    return out


def csr(lists, tags=None, mask=0, value=0):
    """(off uint64 [n + 1], nbr uint32) of the filtered lists."""
    if tags is not None and (mask or value):
        lists = [np.asarray(l, np.uint32)[matches(tags, np.asarray(l, np.uint32), mask, value)] if len(l) else l
                 for l in lists]
    off = np.zeros(len(lists) + 1, np.uint64)
    if lists:
        off[1:] = np.cumsum([len(l) for l in lists])
    nbr = np.concatenate([np.asarray(l, np.uint32) for l in lists]) if lists else np.zeros(0, np.uint32)
    return off, nbr.astype(np.uint32)


def oracle_lists(orc, base, slots=None):
    """InterestedIn of each local slot of an OracleSpace as ascending global slots."""
    slots = range(orc.capacity) if slots is None else slots
    return [orc.neighbors(int(s)).astype(np.uint32) + np.uint32(base) for s in slots]
