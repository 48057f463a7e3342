// nb_pair_counts.hip.h — nb_pair_counts' device side: the histogram of pair separations DD(r), every unordered pair of bodies binned
// by its d2 between squared edges (include/nbody.h has the contract; tests/pair_counts_model.py is its numpy statement).
//   (cells)                neighbors_keys, the sort and neighbors_gather of nb_neighbors.hip.h at radius edges[nbins], by the host helper
//                          the grid queries share
//   pair_counts_coop<NB>   the sweep that ships: a workgroup takes batches of BLOCK consecutive SORTED positions; lane p owns the
//                          candidates of groups_link's two stretches; the workgroup stages the union of its lanes' stretches through
//                          LDS in chunks and every lane bins the staged candidates inside its own stretches.  NB is the bin capacity
//                          (8, 16, 32, 64), chosen on the host like K in nb_neighbors.
//   pair_counts<NB>        the per-lane form of the same sweep, every lane reading its candidates itself: the correctness anchor and
//                          the other side of the A/B (-DNB_PAIR_COUNTS_PER_LANE; DESIGN.md has the figures)
//   pair_counts_sum        adds the workgroups' rows of 64-bit partials into the NB + 1 words the host reads
// THE PREDICATE AND THE CELLS are nb_neighbors' (neighbors_d2; cell size edges[nbins] x (1 + 2^-16)): a pair with d2 < r2max =
// e2[nbins] is never two cells apart (the proof in nb_neighbors.hip.h), and a pair with d2 >= r2max is in no bin.
// WHICH LANE TESTS WHICH PAIR is groups_link's rule: lane p scans the positions behind p in its own cell row through the end of the
// next cell, and the three cells of the row above.  The proof in nb_groups.hip.h that this meets every passing pair exactly once, by
// the member that sorts first, carries over with "passes" read as d2 < r2max.  A body without a cell (a non-finite coordinate) is in
// nobody's stretch and scans nothing.
// THE BINNING is cumulative: a lane keeps C[t] += (d2 < e2[t]) for t = 0 .. NB in registers, so bin b is C[b + 1] - C[b], taken on
// the host from the reduced sums.  The e2[] arrive as a by-value kernel argument, so every compare takes a scalar operand: two VALU
// instructions per edge and candidate, no branch on r2max, no divergent table index, no LDS atomic.  Edges that are not in use are
// +inf (their counters are not read).  d2 = NaN and d2 = +inf fail every compare that is read.  A pair that is not this handle's (its
// lower global index lies outside [i_begin, i_begin + i_count)) gets d2 := +inf before the compares: one select, compiled out with ALL.
// NO COUNTER OVERFLOWS for any n < 2^31.  A lane's two stretches are disjoint ranges of sorted positions, at most n candidates per
// batch, and C[t] never exceeds the candidates the lane has tested since the last flush; the workgroup flushes before any lane's
// tested candidates could pass 2^32 - 1 (the decision is one __syncthreads_or, the same in every thread).  A flush sums the lanes of
// a wave in 64 bits by shuffles and adds the result to the wave's own 64-bit row in LDS; at the end the waves' rows are added and the
// workgroup writes ONE plain row of 64-bit partials.  pair_counts_sum adds the rows.  No global atomic anywhere, nothing depends on
// the order of arrival: the counts are integers and exact.
#pragma once
#include "nb_groups.hip.h"

namespace nbk {

template <int W>
struct PairEdges { float v[W]; };                     // e2[0 .. nbins], then +inf

// one candidate (position q, body index *j, read only for a handle that owns a block) against lane's body `mine` at `me`
template <int W, bool ALL>
__device__ __forceinline__ void pair_counts_bin(float2 me, uint32_t mine, float2 q, const uint32_t *j, uint32_t i_begin, uint32_t i_count,
                                                const PairEdges<W> &e2, uint32_t (&C)[W])
{
    float d2 = neighbors_d2(me.x, me.y, q.x, q.y);
    if constexpr (!ALL) {
        const uint32_t other = *j, lower = other < mine ? other : mine;
        if (lower - i_begin >= i_count) d2 = __uint_as_float(0x7f800000u);   // (an index below i_begin wraps)
    }
#pragma unroll
    for (int t = 0; t < W; ++t) C[t] += d2 < e2.v[t] ? 1u : 0u;
}

// the two stretches of the lane at sorted position p with key `own` (groups_link's): [c0[0], c1[0]) behind p in its own cell row
// through the end of the next cell, [c0[1], c1[1]) the three cells of the row above
__device__ __forceinline__ void pair_counts_stretches(const uint64_t *__restrict__ skey, uint32_t n, uint32_t p, uint64_t own,
                                                      uint32_t (&c0)[2], uint32_t (&c1)[2])
{
    c0[0] = p + 1u;
    c1[0] = neighbors_lower_bound(skey, c0[0], n, ((own & 0xffffffff00000000ull) | ((uint32_t)own + 1u)) + 1u);
    neighbors_range(skey, n, p, own, 1, c0[1], c1[1]);
}

// The lanes' counters into the wave's 64-bit row `mine_row` in LDS (only this wave touches it), and back to zero.
template <int W>
__device__ __forceinline__ void pair_counts_flush(uint32_t (&C)[W], unsigned long long *mine_row)
{
#pragma unroll
    for (int t = 0; t < W; ++t) {
        unsigned long long v = C[t];
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        if ((threadIdx.x & 63u) == 0u) mine_row[t] += v;
        C[t] = 0u;
    }
}

// the waves' rows into row blockIdx.x of `partial` (W words a row)
template <int W>
__device__ __forceinline__ void pair_counts_row(unsigned long long (&wsum)[BLOCK / 64][W], unsigned long long *__restrict__ partial)
{
    __syncthreads();
    if (threadIdx.x < (uint32_t)W) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) v += wsum[w][threadIdx.x];
        partial[(size_t)blockIdx.x * W + threadIdx.x] = v;
    }
}

// PER LANE (the correctness anchor; -DNB_PAIR_COUNTS_PER_LANE builds the library with it): every lane reads its candidates from
// global memory itself.  Workgroup b takes the batches b, b + gridDim.x, ... of BLOCK sorted positions.
template <int NB, bool ALL>
__global__ __launch_bounds__(BLOCK)
void pair_counts(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sval, const float2 *__restrict__ sxy, uint32_t n,
                 uint32_t i_begin, uint32_t i_count, const PairEdges<NB + 1> e2, unsigned long long *__restrict__ partial)
{
    constexpr int W = NB + 1;
    __shared__ unsigned long long wsum[BLOCK / 64][W];
    for (uint32_t t = threadIdx.x; t < (BLOCK / 64) * W; t += BLOCK) (&wsum[0][0])[t] = 0ull;
    __syncthreads();
    uint32_t C[W];
#pragma unroll
    for (int t = 0; t < W; ++t) C[t] = 0u;
    uint64_t tested = 0;
    const uint32_t batches = (n + BLOCK - 1) / BLOCK;
    for (uint32_t b = blockIdx.x; b < batches; b += gridDim.x) {          // workgroup-uniform: every thread meets every barrier
        const uint32_t p = b * BLOCK + threadIdx.x;
        uint32_t c0[2] = {0u, 0u}, c1[2] = {0u, 0u};
        const uint64_t own = p < n ? skey[p] : NEIGHBORS_NO_CELL;
        if (own != NEIGHBORS_NO_CELL) pair_counts_stretches(skey, n, p, own, c0, c1);
        const uint64_t need = (uint64_t)(c1[0] - c0[0]) + (c1[1] - c0[1]);
        if (__syncthreads_or(tested + need > 0xffffffffull)) { pair_counts_flush<W>(C, wsum[threadIdx.x >> 6]); tested = 0; }
        tested += need;
        if (need == 0) continue;
        const float2 me = sxy[p];
        const uint32_t mine = sval[p];
#pragma unroll
        for (int r = 0; r < 2; ++r)
            for (uint32_t c = c0[r]; c < c1[r]; ++c) pair_counts_bin<W, ALL>(me, mine, sxy[c], &sval[c], i_begin, i_count, e2, C);
    }
    pair_counts_flush<W>(C, wsum[threadIdx.x >> 6]);
    pair_counts_row<W>(wsum, partial);
}

// COOPERATIVE, as neighbors_search_coop: per stretch r the lanes' ranges of a batch lie in [u0, u1); the workgroup walks that union
// in chunks of NEIGHBORS_CHUNK candidates, stages a chunk (positions, and body indices for a handle that owns a block, read
// coalesced, once) in LDS, and every lane bins the staged candidates inside its OWN stretch.  A chunk that no lane needs is not
// staged.  Every thread of the workgroup meets every barrier: the batch loop and the chunk bounds are the same in every thread (the
// bounds come from LDS, the skip and the flush from __syncthreads_or).  The four bounds are read into registers behind the barrier
// that completes them, and the next batch writes them only behind its first barrier.
template <int NB, bool ALL>
__global__ __launch_bounds__(BLOCK)
void pair_counts_coop(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sval, const float2 *__restrict__ sxy, uint32_t n,
                      uint32_t i_begin, uint32_t i_count, const PairEdges<NB + 1> e2, unsigned long long *__restrict__ partial)
{
    constexpr int W = NB + 1;
    __shared__ float2 cxy[NEIGHBORS_CHUNK];
    __shared__ uint32_t cj[ALL ? 1 : NEIGHBORS_CHUNK];
    __shared__ uint32_t u0[2], u1[2];
    __shared__ unsigned long long wsum[BLOCK / 64][W];
    for (uint32_t t = threadIdx.x; t < (BLOCK / 64) * W; t += BLOCK) (&wsum[0][0])[t] = 0ull;
    __syncthreads();
    uint32_t C[W];
#pragma unroll
    for (int t = 0; t < W; ++t) C[t] = 0u;
    uint64_t tested = 0;
    const uint32_t batches = (n + BLOCK - 1) / BLOCK;
    for (uint32_t b = blockIdx.x; b < batches; b += gridDim.x) {
        const uint32_t p = b * BLOCK + threadIdx.x;
        uint32_t c0[2] = {0u, 0u}, c1[2] = {0u, 0u};
        const uint64_t own = p < n ? skey[p] : NEIGHBORS_NO_CELL;
        if (own != NEIGHBORS_NO_CELL) pair_counts_stretches(skey, n, p, own, c0, c1);
        const uint64_t need = (uint64_t)(c1[0] - c0[0]) + (c1[1] - c0[1]);
        // a barrier as well: the bounds and the chunk of the batch before have been read
        if (__syncthreads_or(tested + need > 0xffffffffull)) { pair_counts_flush<W>(C, wsum[threadIdx.x >> 6]); tested = 0; }
        tested += need;
        float2 me = make_float2(0.f, 0.f);
        uint32_t mine = 0u;
        if (need) { me = sxy[p]; mine = sval[p]; }
        if (threadIdx.x < 2) { u0[threadIdx.x] = 0xffffffffu; u1[threadIdx.x] = 0u; }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 2; ++r)
            if (c0[r] < c1[r]) { atomicMin(&u0[r], c0[r]); atomicMax(&u1[r], c1[r]); }
        __syncthreads();
        const uint32_t begin[2] = {u0[0], u0[1]}, end[2] = {u1[0], u1[1]};   // no lane has a stretch: 2^32 - 1 and 0, no round
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            for (uint32_t cs = begin[r]; cs < end[r]; cs += NEIGHBORS_CHUNK) {    // (end <= n < 2^31: cs does not wrap)
                const uint32_t ce = end[r] - cs < NEIGHBORS_CHUNK ? end[r] : cs + NEIGHBORS_CHUNK;
                const uint32_t m0 = c0[r] > cs ? c0[r] : cs, m1 = c1[r] < ce ? c1[r] : ce;
                // a barrier as well: the reads of the chunk before are over when the next one is staged
                if (!__syncthreads_or(m0 < m1)) continue;
                for (uint32_t t = threadIdx.x; t < ce - cs; t += BLOCK) {
                    cxy[t] = sxy[cs + t];
                    if constexpr (!ALL) cj[t] = sval[cs + t];
                }
                __syncthreads();
                for (uint32_t c = m0; c < m1; ++c)
                    pair_counts_bin<W, ALL>(me, mine, cxy[c - cs], &cj[ALL ? 0u : c - cs], i_begin, i_count, e2, C);
            }
        }
    }
    pair_counts_flush<W>(C, wsum[threadIdx.x >> 6]);
    pair_counts_row<W>(wsum, partial);
}

// out[t] = the sum over the `rows` rows of partial[row * W + t]: workgroup t takes word t.  Integer adds: the order is free.
__global__ __launch_bounds__(BLOCK)
void pair_counts_sum(const unsigned long long *__restrict__ partial, uint32_t rows, uint32_t W, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long ws[BLOCK / 64];
    const uint32_t t = blockIdx.x;
    unsigned long long v = 0;
    for (uint32_t r = threadIdx.x; r < rows; r += BLOCK) v += partial[(size_t)r * W + t];
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63u) == 0u) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (uint32_t w = 0; w < BLOCK / 64; ++w) total += ws[w];
        out[t] = total;
    }
}

}  // namespace nbk
