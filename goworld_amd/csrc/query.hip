// query.hip — gfx950 kernels of the batched InterestedIn queries: what game
// logic reads from the sets per entity per timer (examples/unity_demo/
// Monster.go:48-98: AI walks InterestedIn for the nearest live Player, Tick
// asks IsInterestedIn(target)), for many entities in one call.
//
//   gw_neighbors_batch  InterestedIn of n query slots as a CSR, each list
//                       ascending by slot: count pass, scan, write pass
//   gw_nearest          per query slot the related entity minimising
//                       (squared distance, slot), and the number of matches
//   gw_related          Entity.IsInterestedIn for n pairs, a thread per pair
//   gw_set_tags         the 32-bit tag per slot the first two filter by
//
// There are no neighbour lists (gw_internal.hpp): a query walks its slot's
// window in the current grid with one wave (wave_neighbors_of, the collect's
// walk: rounded bounds, stamps in the one-ulp band).  The tags live in a
// slot-indexed array of their own that only these kernels read.
#include "dev_common.hpp"

namespace gw {

namespace {

static_assert(QL_WAVE_MAX == 64 && QL_LDS_MAX >= QL_WAVE_MAX, "the register tier holds an entry per lane");
constexpr uint32_t Q_MAX_BLOCKS = 8192;   // waves walk queries k, k + stride, ... (as the collect)

// statistics of one call: QS_SHARDS x {candidates walked, matches}, a wave's
// sums added to the shard of its query index (one address would serialise a
// million atomics)
__device__ __forceinline__ void qstat_add(unsigned long long* qs, uint64_t k, uint32_t cand, uint32_t match) {
    unsigned long long* p = qs + 2 * (k & (QS_SHARDS - 1));
    if (cand) atomicAdd(p, (unsigned long long)cand);
    if (match) atomicAdd(p + 1, (unsigned long long)match);
}

// the filter of a related entity ws: (tag[ws] & mask) == value, the tag
// gathered only where it can decide (rel lanes, mask != 0)
struct TagF {
    const uint32_t* __restrict__ tags;
    uint32_t mask, value;
    __device__ __forceinline__ bool all() const { return mask == 0u; }       // wave-uniform
    __device__ __forceinline__ bool take(bool rel, uint32_t ws) const {
        if (all()) return rel && value == 0u;
        return rel && (tags[ws] & mask) == value;
    }
};

// query k's slot and state; false when it has no list (a slot at or beyond
// the context's slots -- device-resident slots are not validated by the host
// -- or absent from every space)
__device__ __forceinline__ bool query_ent(const World& w, const uint32_t* __restrict__ slots, uint64_t k,
                                          uint32_t& e, AoiEnt& a) {
    e = slots[k];
    if (e >= w.cap) return false;
    a = w.rec[e].a;
    return (a.meta & PRESENT_BIT) != 0;
}

// ---- lists -----------------------------------------------------------------
// count pass: cnt[k] = |{w related to slots[k], w matches}|; lcnt[k] = the
// same when the list is longer than lmin (it takes the general ordering
// path), else 0
template <int U>
__global__ void __launch_bounds__(NT) k_query_count(World w, const uint32_t* __restrict__ slots, uint32_t n, TagF tf,
                                                    uint32_t lmin, uint32_t* __restrict__ cnt,
                                                    uint32_t* __restrict__ lcnt, unsigned long long* qs) {
    const uint64_t stride = (uint64_t)gridDim.x * NWAVE;
    for (uint64_t k = (uint64_t)blockIdx.x * NWAVE + (threadIdx.x >> 6); k < n; k += stride) {
        uint32_t e, c = 0, cand = 0;
        AoiEnt a;
        if (query_ent(w, slots, k, e, a)) {
            wave_neighbors_of<U>(w, e, a, w.sp[a.meta & SPACE_MASK], [&](bool rel, uint32_t ws, uint32_t) {
                c += (uint32_t)popc64(wave_ballot(tf.take(rel, ws)));
                cand += (uint32_t)popc64(wave_ballot(ws != e));
            });
        }
        if (lane_id() == 0) {
            cnt[k] = c;
            lcnt[k] = c > lmin ? c : 0u;
            qstat_add(qs, k, cand, c);
        }
    }
}

// write pass.  The walk meets candidates in grid order (cell, then slot), a
// list is ascending by slot:
//   up to QL_WAVE_MAX   staged in the wave's LDS buffer, sorted in registers
//                       (wave_sort64: an entry per lane), stored once
//   up to QL_LDS_MAX    sorted in the LDS buffer by the wave: runs of 64 in
//                       registers, then bitonic_inplace's merge levels
//   longer, or lmin = 0 written as (query index << 32 | slot) pairs at
//                       loff[k], ordered afterwards by two stable radix sorts
//                       (k_pairs_swap, k_pairs_place)
template <int U>
__global__ void __launch_bounds__(NT) k_query_write(World w, const uint32_t* __restrict__ slots, uint32_t n, TagF tf,
                                                    uint32_t lmin, const uint64_t* __restrict__ off,
                                                    const uint64_t* __restrict__ loff, uint32_t* __restrict__ nbr,
                                                    uint64_t* __restrict__ pairs, unsigned long long* qs) {
    __shared__ uint32_t sbuf[NWAVE][QL_LDS_MAX];
    uint32_t* buf = sbuf[threadIdx.x >> 6];
    const int ln = lane_id();
    const uint64_t lt = lanemask_lt();
    const uint64_t stride = (uint64_t)gridDim.x * NWAVE;
    for (uint64_t k = (uint64_t)blockIdx.x * NWAVE + (threadIdx.x >> 6); k < n; k += stride) {
        const uint64_t at = off[k];
        const uint32_t c = (uint32_t)(off[k + 1] - at);          // the total lands behind the offsets
        if (!c) continue;                                        // wave-uniform
        uint32_t e, cand = 0;
        AoiEnt a;
        if (!query_ent(w, slots, k, e, a)) continue;             // (c != 0: present)
        const bool general = c > lmin;
        uint64_t* pr = pairs + (general ? loff[k] : 0);
        uint32_t nb = 0;
        wave_neighbors_of<U>(w, e, a, w.sp[a.meta & SPACE_MASK], [&](bool rel, uint32_t ws, uint32_t) {
            const bool take = tf.take(rel, ws);
            const uint64_t bt = wave_ballot(take);
            const uint32_t i = nb + (uint32_t)popc64(bt & lt);
            if (take && i < c) {                                 // (i < c: the count pass saw the same grid)
                if (general) pr[i] = (k << 32) | ws;
                else buf[i] = ws;
            }
            nb += (uint32_t)popc64(bt);
            cand += (uint32_t)popc64(wave_ballot(ws != e));
        });
        if (ln == 0) qstat_add(qs, k, cand, 0);
        if (general) continue;
        wave_sync();
        if (c <= QL_WAVE_MAX) {
            uint32_t v = (uint32_t)ln < c ? buf[ln] : 0xffffffffu;
            v = wave_sort64(v);
            if ((uint32_t)ln < c) nbr[at + ln] = v;
        } else {
            // each run of 64 in registers, then the network's merge levels from 128 up in LDS
            for (uint32_t i = (uint32_t)ln; i - (uint32_t)ln < c; i += 64) {
                uint32_t v = i < c ? buf[i] : 0xffffffffu;       // (the padding sorts last and is not stored)
                v = wave_sort64(v);
                if (i < c) buf[i] = v;
            }
            wave_sync();
            bitonic_inplace<64>(buf, c, ln, [](uint32_t x) { return x; }, [] { wave_sync(); }, 2 * QL_WAVE_MAX);
            for (uint32_t i = (uint32_t)ln; i < c; i += 64) nbr[at + i] = buf[i];
        }
        wave_sync();                                             // the buffer is free for the next query
    }
}

// general path: pairs (query << 32 | slot) sorted by slot -> (slot << 32 |
// query), to be sorted by query (stable: slots stay ascending inside a query)
__global__ void __launch_bounds__(NT) k_pairs_swap(uint64_t* __restrict__ p, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const uint64_t x = p[i];
    p[i] = (x << 32) | (x >> 32);
}
// pair j of the (query, slot)-ordered stream is entry j - loff[query] of its list
__global__ void __launch_bounds__(NT) k_pairs_place(const uint64_t* __restrict__ p, uint64_t n,
                                                    const uint64_t* __restrict__ off,
                                                    const uint64_t* __restrict__ loff, uint32_t* __restrict__ nbr) {
    const uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (j >= n) return;
    const uint64_t x = p[j];
    const uint32_t k = (uint32_t)x;
    nbr[off[k] + (j - loff[k])] = (uint32_t)(x >> 32);
}

// ---- nearest ---------------------------------------------------------------
// Vector3.DistanceTo (Vector3.go:23-28) of the candidate's Position p from the
// query's q, float32, each product and sum rounded once (no fused
// multiply-add.  The build's -ffp-contract=off gives that; to keep it under
// another flag the products pass through in_vgpr, an empty asm the compiler
// cannot fuse across: HIP's __fmul_rn / __fadd_rn are plain operators and
// -ffp-contract=fast fuses in the backend whatever a local pragma says)
__device__ __forceinline__ float dist2(const float4& p, const float4& q) {
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    in_vgpr(xx);
    in_vgpr(yy);
    in_vgpr(zz);
    return (xx + yy) + zz;
}
constexpr unsigned long long NEAR_NONE = ((unsigned long long)0x7f800000u << 32) | 0xffffffffull;   // (+inf, GW_NO_SLOT)

template <int U>
__global__ void __launch_bounds__(NT) k_nearest(World w, const uint32_t* __restrict__ slots, uint32_t n, TagF tf,
                                                gw_nearest_rec* __restrict__ out, unsigned long long* qs) {
    const uint64_t stride = (uint64_t)gridDim.x * NWAVE;
    for (uint64_t k = (uint64_t)blockIdx.x * NWAVE + (threadIdx.x >> 6); k < n; k += stride) {
        uint32_t e, c = 0, cand = 0;
        AoiEnt a;
        unsigned long long best = NEAR_NONE;                     // d2 >= 0: its bits order like its value
        if (query_ent(w, slots, k, e, a)) {
            const float4 q = w.rec[e].p;                         // the query's own Position, once
            wave_neighbors_of<U>(w, e, a, w.sp[a.meta & SPACE_MASK], [&](bool rel, uint32_t ws, uint32_t) {
                const bool take = tf.take(rel, ws);
                if (take) {                                      // the 64-B line of a match only
                    const float4 p = w.rec[ws].p;
                    const unsigned long long key = ((unsigned long long)__float_as_uint(dist2(p, q)) << 32) | ws;
                    best = key < best ? key : best;
                }
                c += (uint32_t)popc64(wave_ballot(take));
                cand += (uint32_t)popc64(wave_ballot(ws != e));
            });
        }
#pragma unroll
        for (int j = 32; j > 0; j >>= 1) {
            const unsigned long long o = ((unsigned long long)(uint32_t)__shfl_xor((int)(best >> 32), j, 64) << 32) |
                                         (uint32_t)__shfl_xor((int)(uint32_t)best, j, 64);
            best = o < best ? o : best;
        }
        if (lane_id() == 0) {
            gw_nearest_rec r;
            r.slot = (uint32_t)best;
            r.count = c;
            r.d2 = __uint_as_float((uint32_t)(best >> 32));
            r.dist = (float)__dsqrt_rn((double)r.d2);            // Coord(math.Sqrt(float64(d2)))
            out[k] = r;
            qstat_add(qs, k, cand, c);
        }
    }
}

// ---- pairs -----------------------------------------------------------------
// Entity.IsInterestedIn (Entity.go:249-251) straight from the two slots'
// states: both present, one space, a != b, and each inside the other's rounded
// window; where the two tests differ the later stamp decides (resolve)
__global__ void __launch_bounds__(NT) k_related(World w, const uint32_t* __restrict__ qa,
                                                const uint32_t* __restrict__ qb, uint32_t n,
                                                uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const uint32_t sa = qa[i], sb = qb[i];
    bool rel = false;
    if (sa < w.cap && sb < w.cap && sa != sb) {
        const AoiEnt a = w.rec[sa].a, b = w.rec[sb].a;
        if ((a.meta & PRESENT_BIT) && a.meta == b.meta) {
            const float d = w.sp[a.meta & SPACE_MASK].d;
            const bool ia = in_win(a.x, a.z, d, b.x, b.z);       // b inside a's window
            const bool ib = in_win(b.x, b.z, d, a.x, a.z);
            rel = ia == ib ? ia : resolve(ia, ib, w.rec[sa].stamp, w.rec[sb].stamp);
        }
    }
    out[i] = rel ? 1 : 0;
}

// ---- tags ------------------------------------------------------------------
__global__ void __launch_bounds__(NT) k_set_tags(uint32_t* __restrict__ tags, const uint32_t* __restrict__ slots,
                                                 const uint32_t* __restrict__ vals, uint32_t n, uint32_t cap) {
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i < n && slots[i] < cap) tags[slots[i]] = vals[i];
}

inline dim3 qgrid(uint32_t n) { return dim3(std::min(nblk1(n, NWAVE), Q_MAX_BLOCKS)); }

}  // namespace

void launch_query_count(const World& w, const uint32_t* slots, uint32_t n, const uint32_t* tags, uint32_t mask,
                        uint32_t value, uint32_t lmin, uint32_t* cnt, uint32_t* lcnt, unsigned long long* qs,
                        hipStream_t s) {
    if (!n) return;
    const TagF tf{tags, mask, value};
    hipLaunchKernelGGL(k_query_count<4>, qgrid(n), dim3(NT), 0, s, w, slots, n, tf, lmin, cnt, lcnt, qs);
}
void launch_query_write(const World& w, const uint32_t* slots, uint32_t n, const uint32_t* tags, uint32_t mask,
                        uint32_t value, uint32_t lmin, const uint64_t* off, const uint64_t* loff, uint32_t* nbr,
                        uint64_t* pairs, unsigned long long* qs, hipStream_t s) {
    if (!n) return;
    const TagF tf{tags, mask, value};
    hipLaunchKernelGGL(k_query_write<4>, qgrid(n), dim3(NT), 0, s, w, slots, n, tf, lmin, off, loff, nbr, pairs, qs);
}
void launch_pairs_swap(uint64_t* p, uint64_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_pairs_swap, dim3(nblk(n, NT)), dim3(NT), 0, s, p, n);
}
void launch_pairs_place(const uint64_t* p, uint64_t n, const uint64_t* off, const uint64_t* loff, uint32_t* nbr,
                        hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_pairs_place, dim3(nblk(n, NT)), dim3(NT), 0, s, p, n, off, loff, nbr);
}
void launch_nearest(const World& w, const uint32_t* slots, uint32_t n, const uint32_t* tags, uint32_t mask,
                    uint32_t value, gw_nearest_rec* out, unsigned long long* qs, hipStream_t s) {
    if (!n) return;
    const TagF tf{tags, mask, value};
    hipLaunchKernelGGL(k_nearest<4>, qgrid(n), dim3(NT), 0, s, w, slots, n, tf, out, qs);
}
void launch_related(const World& w, const uint32_t* a, const uint32_t* b, uint32_t n, uint8_t* out, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_related, dim3(nblk(n, NT)), dim3(NT), 0, s, w, a, b, n, out);
}
void launch_set_tags(uint32_t* tags, const uint32_t* slots, const uint32_t* vals, uint32_t n, uint32_t cap,
                     hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_set_tags, dim3(nblk(n, NT)), dim3(NT), 0, s, tags, slots, vals, n, cap);
}

}  // namespace gw
