// nb_neighbors.hip.h — nb_neighbors' device side: for every owned body the bodies closer than `radius`, counted, and the k nearest
// of them ranked by (d2, index) (include/nbody.h has the contract; tests/neighbors_model.py is its numpy statement).
//   neighbors_keys<L>      one lane per body of the replica: the position rounded to float (x, y), its cell and the 64-bit cell key
//   (sort)                 nb_tree_sort_pairs on (key, body index), by the host
//   neighbors_gather       the float positions in sorted order, so that the search reads its candidates coalesced
//   neighbors_search_coop<K>   the search that ships: a workgroup takes BLOCK consecutive SORTED positions, so its queries sit in the
//                          same or adjacent cells; every lane finds the three key ranges of the 3 x 3 cells round its query by binary
//                          search on the sorted keys; the workgroup stages the union of the ranges through LDS in chunks and every
//                          lane tests the staged candidates inside its own ranges, the best k kept in registers; the row goes to the
//                          body's ORIGINAL index.  K is the capacity of the register list (4, 8, 16, 32); K = 0 counts only.
//   neighbors_search<K>    the per-lane form of the same search, every lane reading its candidates itself: the correctness anchor
//                          and the other side of the A/B (-DNB_NEIGHBORS_PER_LANE; DESIGN.md has the figures)
// THE PREDICATE is the reference's (body1->pos - body2->pos).mag_sq() < adaptiveDistanceSq (main.cpp:233-386) in fp32, one rounding
// per operation, no contraction: dx = xj - xi, dy = yj - yi, d2 = dx * dx + dy * dy, neighbour when j != i && d2 < r2.
// THE CELLS: cell_coord's rule (nb_collide.hip.h) with h = radius x (1 + 2^-16): c = floor(v * inv_h) in double, clamped to +-2^30.
// WHY A PAIR THAT PASSES IS NEVER TWO CELLS APART (per axis; x here):
//   1. fp32 addition of two non-negative numbers is monotone, so d2 >= fl(dx * dx), and the pair passes only if fl(dx * dx) < r2
//      with r2 = fl(radius * radius) > 0 (the host refuses r2 == 0 and a non-finite one).
//   2. fl(dx * dx) and r2 each carry at most 2^-24 relative error, or 2^-150 absolute where they are subnormal; either way
//      |dx| <= radius x (1 + 2^-23).  dx = fl(xj - xi) carries 2^-24 relative error and none where it is subnormal, so
//      |xj - xi| <= radius x (1 + 2^-22) < h x (1 - 2^-17).
//   3. The quotients q = v / h of the two bodies therefore differ by less than 1 - 2^-17.  The computed ones, fl(v * fl(1 / h)), are
//      a monotone function of v and carry at most 2^-51 relative error: 2^-20 absolute while |q| <= 2^31.  So where both quotients
//      are below 2^31 in size the computed ones differ by less than 1 and their floors by at most 1; the clamp is monotone and keeps
//      that.  Where one of them is beyond 2^30 + 1 in size the other is beyond 2^30, and both are clamped to the same cell.
// THE KEY is (cy + 2^30) << 32 | (cx + 2^30): both halves lie in [0, 2^31), so the cells cx - 1 .. cx + 1 of one row are ONE
// contiguous key range and a query scans three ranges, not nine.  A body with a non-finite coordinate gets the largest key
// (NEIGHBORS_NO_CELL; no cell has it: its high word would be 2^32 - 1), sorts behind every cell, is in nobody's range and, as a query,
// writes an empty row: the predicate is false on NaN and infinity, so nothing more is needed.
// THE ORDER of a row is that of the packed 64-bit integer (bits(d2) << 32) | j: d2 >= 0, so its bits order like its value.  The
// empty entry is (bits(+inf) << 32) | NB_NO_NEIGHBOR, larger than every neighbour's (d2 < r2 is finite), so a row starts as k of them.
#pragma once
#include "nb_kernels.hip.h"
#include "nb_collide.hip.h"
#include "nb_tree_prims.h"

namespace nbk {

constexpr uint64_t NEIGHBORS_NO_CELL = ~0ull;
constexpr uint64_t NEIGHBORS_EMPTY = ((uint64_t)0x7f800000u << 32) | 0xffffffffu;   // +inf, NB_NO_NEIGHBOR
constexpr double NEIGHBORS_CELL_SLACK = 1.0 + 1.0 / 65536.0;                          // h = radius x this

template <typename L>
__global__ __launch_bounds__(BLOCK)
void neighbors_keys(const typename L::vec *__restrict__ pos, uint32_t n, double inv_h, float2 *__restrict__ xy, uint64_t *__restrict__ key,
                    uint32_t *__restrict__ val)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const auto q = pos[i];
    const float x = (float)q.x, y = (float)q.y;
    xy[i] = make_float2(x, y);
    val[i] = i;
    if (!isfinite(x) || !isfinite(y)) { key[i] = NEIGHBORS_NO_CELL; return; }
    const uint32_t ux = (uint32_t)(cell_coord((double)x, inv_h) + 1073741824), uy = (uint32_t)(cell_coord((double)y, inv_h) + 1073741824);
    key[i] = (uint64_t)uy << 32 | ux;
}

__global__ __launch_bounds__(BLOCK)
void neighbors_gather(const float2 *__restrict__ xy, const uint32_t *__restrict__ sval, uint32_t n, float2 *__restrict__ sxy)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p < n) sxy[p] = xy[sval[p]];
}

// first position in [lo, hi) whose key is not below `key` (hi if none)
__device__ __forceinline__ uint32_t neighbors_lower_bound(const uint64_t *__restrict__ skey, uint32_t lo, uint32_t hi, uint64_t key)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (skey[mid] < key) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// the pragma, not the __f*_rn intrinsics (raster_pixel, nb_raster.hip.h, has the reason)
__device__ __forceinline__ float neighbors_d2(float xi, float yi, float xj, float yj)
{
#pragma clang fp contract(off)
    const float dx = xj - xi, dy = yj - yi;
    return dx * dx + dy * dy;
}

// `cand` into the ascending list best[0 .. K), the largest entry dropped; the caller has found cand < best[K - 1]
template <int K>
__device__ __forceinline__ void neighbors_insert(uint64_t (&best)[K], uint64_t cand)
{
#pragma unroll
    for (int t = K - 1; t > 0; --t) {
        const uint64_t below = best[t - 1];                               // still the old value: t - 1 is written in the next round
        best[t] = cand < below ? below : cand < best[t] ? cand : best[t];
    }
    best[0] = cand < best[0] ? cand : best[0];
}

// The key range [c0, c1) of the three cells ux - 1 .. ux + 1 of cell row uy + r (r = -1, 0, 1) for the query at sorted position p
// with key `own`: empty (c0 == c1 == 0) for the row below row 0.  The rows below the query's lie before p, its own round p, the ones
// above behind p, so every search starts from a half of the array.
__device__ __forceinline__ void neighbors_range(const uint64_t *__restrict__ skey, uint32_t n, uint32_t p, uint64_t own, int r, uint32_t &c0,
                                                uint32_t &c1)
{
    const uint32_t ux = (uint32_t)own, uy = (uint32_t)(own >> 32);
    c0 = c1 = 0u;
    if (r < 0 && uy == 0u) return;
    const uint32_t x0 = ux ? ux - 1u : 0u, x1 = ux + 1u;                   // ux < 2^31: x1 + 1 stays inside the low word
    const uint64_t rowkey = (uint64_t)(uy + (uint32_t)r) << 32;
    const uint32_t from = r > 0 ? p : 0u, to = r < 0 ? p : n;
    c0 = neighbors_lower_bound(skey, from, r == 0 ? p : to, rowkey | x0);
    c1 = neighbors_lower_bound(skey, r == 0 ? p : c0, to, (rowkey | x1) + 1u);
}

// one candidate (position q, body index *j, read only when the candidate may enter the list) against the query `me`
template <int K>
__device__ __forceinline__ void neighbors_test(float2 me, float2 q, const uint32_t *j, float r2, uint32_t &found, uint64_t (&best)[K > 0 ? K : 1])
{
    const float d2 = neighbors_d2(me.x, me.y, q.x, q.y);
    if (!(d2 < r2)) return;
    ++found;
    if constexpr (K > 0) {
        const uint32_t bits = __float_as_uint(d2);
        if (bits > (uint32_t)(best[K - 1] >> 32)) return;                 // the current worst first: a rejected candidate costs this
        const uint64_t cand = (uint64_t)bits << 32 | *j;
        if (cand < best[K - 1]) neighbors_insert<K>(best, cand);
    }
}

// idx / dist2 hold i_count rows of k entries (k <= K), count i_count entries; any of them may be null (with K = 0 the first two are)
template <int K>
__device__ __forceinline__ void neighbors_write(uint32_t row, uint32_t k, uint32_t found, const uint64_t (&best)[K > 0 ? K : 1],
                                                uint32_t *__restrict__ idx, float *__restrict__ dist2, uint32_t *__restrict__ count)
{
    if (count) count[row] = found;
    if constexpr (K > 0) {
        const size_t base = (size_t)row * k;
#pragma unroll
        for (int t = 0; t < K; ++t) {
            if ((uint32_t)t < k) {
                if (idx) idx[base + t] = (uint32_t)best[t];
                if (dist2) dist2[base + t] = __uint_as_float((uint32_t)(best[t] >> 32));
            }
        }
    }
}

// PER LANE (the correctness anchor; -DNB_NEIGHBORS_PER_LANE builds the library with it): sorted position p, the query is body
// sval[p]; every lane reads its candidates from global memory itself.  The 64 lanes of a wave sit in the same or adjacent cells, so
// their reads share cache lines.
template <int K>
__global__ __launch_bounds__(BLOCK)
void neighbors_search(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sval, const float2 *__restrict__ sxy, uint32_t n,
                      uint32_t i_begin, uint32_t i_count, float r2, uint32_t k, uint32_t *__restrict__ idx, float *__restrict__ dist2,
                      uint32_t *__restrict__ count)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t row = sval[p] - i_begin;
    if (row >= i_count) return;                                           // not owned (an index below i_begin wraps): a candidate only
    uint64_t best[K > 0 ? K : 1];
#pragma unroll
    for (int t = 0; t < (K > 0 ? K : 1); ++t) best[t] = NEIGHBORS_EMPTY;
    uint32_t found = 0;
    const uint64_t own = skey[p];
    if (own != NEIGHBORS_NO_CELL) {
        const float2 me = sxy[p];
        for (int r = -1; r <= 1; ++r) {
            uint32_t c0, c1;
            neighbors_range(skey, n, p, own, r, c0, c1);
            for (uint32_t c = c0; c < c1; ++c)
                if (c != p) neighbors_test<K>(me, sxy[c], &sval[c], r2, found, best);
        }
    }
    neighbors_write<K>(row, k, found, best, idx, dist2, count);
}

// COOPERATIVE: a workgroup takes BLOCK consecutive sorted queries.  Per cell row r its lanes' ranges lie in [u0, u1) (the smallest c0
// and the largest c1 of the lanes that have one); the workgroup walks that union in chunks of NEIGHBORS_CHUNK candidates, stages a
// chunk (positions and body indices, read coalesced, once) in LDS, and every lane tests the staged candidates inside its OWN range.
// A chunk that no lane needs (a workgroup whose queries straddle two cell rows has a union that spans the stretch between them) is
// not staged.  Every thread of the workgroup, query or not, meets every barrier: the loop bounds come from LDS and the skip from
// __syncthreads_or, both the same in every thread.  The candidates a lane tests, and so its row, are the per-lane form's; their
// order differs, which the list does not depend on.
constexpr uint32_t NEIGHBORS_CHUNK = 1024;          // 8 + 4 KiB of LDS

template <int K>
__global__ __launch_bounds__(BLOCK)
void neighbors_search_coop(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sval, const float2 *__restrict__ sxy, uint32_t n,
                           uint32_t i_begin, uint32_t i_count, float r2, uint32_t k, uint32_t *__restrict__ idx, float *__restrict__ dist2,
                           uint32_t *__restrict__ count)
{
    __shared__ float2 cxy[NEIGHBORS_CHUNK];
    __shared__ uint32_t cj[NEIGHBORS_CHUNK];
    __shared__ uint32_t u0[3], u1[3];
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t row = 0xffffffffu;
    if (p < n) row = sval[p] - i_begin;
    const bool query = row < i_count;                                     // p >= n and bodies that are not owned: no query, no return
    uint64_t best[K > 0 ? K : 1];
#pragma unroll
    for (int t = 0; t < (K > 0 ? K : 1); ++t) best[t] = NEIGHBORS_EMPTY;
    uint32_t found = 0, c0[3] = {0u, 0u, 0u}, c1[3] = {0u, 0u, 0u};
    float2 me = make_float2(0.f, 0.f);
    if (query) {
        const uint64_t own = skey[p];
        if (own != NEIGHBORS_NO_CELL) {
            me = sxy[p];
#pragma unroll
            for (int r = 0; r < 3; ++r) neighbors_range(skey, n, p, own, r - 1, c0[r], c1[r]);
        }
    }
    if (threadIdx.x < 3) { u0[threadIdx.x] = 0xffffffffu; u1[threadIdx.x] = 0u; }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 3; ++r)
        if (c0[r] < c1[r]) { atomicMin(&u0[r], c0[r]); atomicMax(&u1[r], c1[r]); }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const uint32_t begin = u0[r], end = u1[r];                        // no lane has a range: 2^32 - 1 and 0, no round
        for (uint32_t cs = begin; cs < end; cs += NEIGHBORS_CHUNK) {      // (end <= n < 2^31: cs does not wrap)
            const uint32_t ce = end - cs < NEIGHBORS_CHUNK ? end : cs + NEIGHBORS_CHUNK;
            const uint32_t m0 = c0[r] > cs ? c0[r] : cs, m1 = c1[r] < ce ? c1[r] : ce;
            // a barrier as well: the reads of the chunk before are over when the next one is staged
            if (!__syncthreads_or(m0 < m1)) continue;
            for (uint32_t t = threadIdx.x; t < ce - cs; t += BLOCK) { cxy[t] = sxy[cs + t]; cj[t] = sval[cs + t]; }
            __syncthreads();
            for (uint32_t c = m0; c < m1; ++c)
                if (c != p) neighbors_test<K>(me, cxy[c - cs], &cj[c - cs], r2, found, best);
        }
    }
    if (query) neighbors_write<K>(row, k, found, best, idx, dist2, count);
}

}  // namespace nbk
