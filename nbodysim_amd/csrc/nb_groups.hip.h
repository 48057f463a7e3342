// nb_groups.hip.h — nb_groups' device side: the friends-of-friends groups of the bodies, the connected components of the graph whose
// edges are nb_neighbors' predicate (include/nbody.h has the contract; tests/groups_model.py is its numpy statement).
//   (cells)                neighbors_keys, the sort and neighbors_gather of nb_neighbors.hip.h, by the host helper both calls share
//   groups_init            parent[i] = i for all n bodies of the replica; parent[] is indexed by ORIGINAL body index
//   groups_link            the hot path: one lane per sorted position p tests the pairs it owns and unites those that pass
//   groups_flatten         parent[i] = find(i) for all n: parent[] is then the label plane (the owned block is copied out of it)
//   groups_roots           how many i have parent[i] == i: *ngroups.  Only when asked for.
//   groups_tally<COMBINE>  +1 into cnt[label] per body, the adds of a wave, then of a workgroup, that share a label combined first.
//                          Only when sizes are asked for.
//   groups_sizes           size[row] = cnt[label of owned body row]
// THE PREDICATE AND THE CELLS are nb_neighbors' (neighbors_d2, d2 < r2; cell size radius x (1 + 2^-16)); the proof in
// nb_neighbors.hip.h that a passing pair is never two cells apart holds here word for word.  The relation is symmetric: fp32
// subtraction is exactly antisymmetric and the squares lose the sign, so d2(i, j) = d2(j, i) bit for bit.
// WHICH LANE TESTS WHICH PAIR.  Take bodies a, b at sorted positions pa < pb, so key(a) <= key(b), the key being (row << 32) | column.
// If the pair passes, the cells differ by at most one per axis.  Then either row(b) = row(a), and column(a) <= column(b) <=
// column(a) + 1: pb lies in (pa, end of cell column(a) + 1 of that row), the stretch of its own row that lane pa scans; or row(b) =
// row(a) + 1 (a larger key cannot have a smaller row) with |column(b) - column(a)| <= 1: pb lies in the three cells of the row above,
// which lane pa scans whole.  Lane pb scans only positions behind pb and the row above its own, so it never meets a.  The two
// stretches of lane pa are disjoint (different rows).  Every passing pair is therefore tested exactly once, by the member that sorts
// first; the row below is never read.  A body without a cell (a non-finite coordinate, NEIGHBORS_NO_CELL) sorts behind every cell,
// is in nobody's stretch and scans nothing: it stays its own root.
// THE UNION-FIND.  INVARIANT: parent[x] <= x at all times, and a hook only ever points a ROOT (parent[x] == x) at a smaller index of
// the set it is united with.  Hence: no cycles; every find is a strictly descending walk and ends; a body that has stopped being a
// root never becomes one again; every value parent[x] ever held is, and stays, an ancestor of x; and the root of a finished
// component is its smallest index, which is what makes the labels canonical without a relabelling pass.
//   find    walks up with path halving: parent[x] = parent[parent[x]].  These are plain (relaxed, not read-modify-write) loads and
//           stores.  A load may return an old value (another compute unit's cache, another die's L2): it is still an ancestor, so
//           the walk still descends inside the set.  A halving store writes an ancestor over an ancestor, and only ever to an x that
//           was seen not to be a root, so it never collides with a hook (hooks compare-and-swap roots) and cannot make a root.
//   unite   finds both roots; equal: done (an ancestor common to both, even a stale one, proves them connected).  Otherwise
//           atomicCAS(&parent[hi], hi, lo) with hi the larger.  Success: hi, a root until this instant, hangs below lo < hi (lo may
//           no longer be a root itself; it is still a member of the other set, which is all the invariant needs).  Failure: another
//           lane hooked hi first; the value the CAS found there is an ancestor of hi and the loop goes on from it.
//   link    a lane carries `mine`, the smallest ancestor of its own body it has met, from pair to pair.  For a passing pair it loads
//           parent[j] once: equal to `mine` means connected already (most pairs, once the sets have formed: one load, no walk);
//           otherwise it unites `mine` with that parent and, if j was seen not to be a root, points j straight at the result.
//   The compare-and-swap is the only arbiter; no lane waits for another lane, there is no lock and no flag to spin on: a failed CAS
//   means someone else made progress, and each retry starts strictly lower.
// THE LOOPS ARE BOUNDED ALL THE SAME: a find of more than n + 1 hops or a unite of more than n + 1 rounds sets a bit of the fault
// word and the lane leaves; the host reports NB_EHIP.  Under the invariant neither can happen (a descending walk over n indices).
// Indices: every value stored in parent[] was read from parent[] or is a body index below n, so no walk leaves the array.
#pragma once
#include "nb_neighbors.hip.h"

namespace nbk {

constexpr uint32_t GROUPS_NONE = 0xffffffffu;         // what a find or unite returns after it set the fault word
constexpr uint32_t GROUPS_FAULT_FIND = 1u, GROUPS_FAULT_UNITE = 2u;
constexpr int GROUPS_WAVE_ROUNDS = 4;                 // as RASTER_WAVE_ROUNDS

__device__ __forceinline__ uint32_t groups_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void groups_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(BLOCK)
void groups_init(uint32_t *__restrict__ parent, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) parent[i] = i;
}

// the root of x as far as this lane can see it (see above: a stale root is an ancestor); GROUPS_NONE after n + 1 hops
template <bool HALVE>
__device__ __forceinline__ uint32_t groups_find(uint32_t *parent, uint32_t x, uint32_t n, uint32_t *fault)
{
    for (uint32_t hops = 0; hops <= n; ++hops) {
        const uint32_t p = groups_load(&parent[x]);
        if (p == x) return x;
        const uint32_t g = groups_load(&parent[p]);
        if (g == p) return p;
        if constexpr (HALVE) groups_store(&parent[x], g);                // x is not a root: p < x was seen
        x = g;
    }
    atomicOr(fault, GROUPS_FAULT_FIND);
    return GROUPS_NONE;
}

// a and b into one set; returns an ancestor of both (the caller goes on from it), GROUPS_NONE after a fault
__device__ __forceinline__ uint32_t groups_unite(uint32_t *parent, uint32_t a, uint32_t b, uint32_t n, uint32_t *fault)
{
    for (uint32_t tries = 0; tries <= n; ++tries) {
        a = groups_find<true>(parent, a, n, fault);
        if (a == GROUPS_NONE) return GROUPS_NONE;
        b = groups_find<true>(parent, b, n, fault);
        if (b == GROUPS_NONE) return GROUPS_NONE;
        if (a == b) return a;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) return lo;
        a = old;                                                          // someone else hooked hi: old < hi is its ancestor
        b = lo;
    }
    atomicOr(fault, GROUPS_FAULT_UNITE);
    return GROUPS_NONE;
}

// PER LANE, as neighbors_search: sorted position p, body sval[p]; the lane reads its candidates from global memory itself (the lanes
// of a wave sit in the same or adjacent cells and share cache lines).  d2 first: only a pair that passes touches parent[].
__global__ __launch_bounds__(BLOCK)
void groups_link(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sval, const float2 *__restrict__ sxy, uint32_t n, float r2,
                 uint32_t *parent, uint32_t *fault)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint64_t own = skey[p];
    if (own == NEIGHBORS_NO_CELL) return;
    const float2 me = sxy[p];
    uint32_t mine = sval[p];                                              // the body, later an ancestor of it: where its next find starts
    for (int r = 0; r <= 1; ++r) {
        uint32_t c0, c1;
        if (r == 0) {                                                     // behind p in its own row: the rest of its cell and the next one
            c0 = p + 1u;
            c1 = neighbors_lower_bound(skey, c0, n, ((own & 0xffffffff00000000ull) | ((uint32_t)own + 1u)) + 1u);
        } else neighbors_range(skey, n, p, own, 1, c0, c1);              // the three cells of the row above
        for (uint32_t c = c0; c < c1; ++c) {
            const float2 q = sxy[c];
            if (!(neighbors_d2(me.x, me.y, q.x, q.y) < r2)) continue;
            const uint32_t j = sval[c], pj = groups_load(&parent[j]);
            if (pj == mine) continue;                                     // the usual case late in the pass: mine is j's ancestor already
            mine = groups_unite(parent, mine, pj, n, fault);              // pj is in j's set: uniting with it unites with j
            if (mine == GROUPS_NONE) return;
            // mine is now an ancestor of j, reached by descending from pj, so mine <= pj: j, seen not to be a root, may point at it
            if (pj != j && pj != mine) groups_store(&parent[j], mine);
        }
    }
}

// After the link kernel has finished nothing hooks any more: the root a walk finds is the root.  In place: a lane that walks through
// an x already flattened reads its root, an ancestor like any other.
__global__ __launch_bounds__(BLOCK)
void groups_flatten(uint32_t *parent, uint32_t n, uint32_t *fault)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = groups_find<false>(parent, i, n, fault);
    if (r != GROUPS_NONE) groups_store(&parent[i], r);
}

// *ngroups += the bodies that are their own label; workgroup b takes the batches b, b + gridDim.x, ...; one global add per workgroup
__global__ __launch_bounds__(BLOCK)
void groups_roots(const uint32_t *__restrict__ label, uint32_t n, uint32_t *__restrict__ ngroups)
{
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0u;
    __syncthreads();
    uint32_t c = 0u;
    const uint32_t batches = (n + BLOCK - 1) / BLOCK;
    for (uint32_t b = blockIdx.x; b < batches; b += gridDim.x) {
        const uint32_t i = b * BLOCK + threadIdx.x;
        if (i < n && label[i] == i) ++c;
    }
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63u) == 0u && c) atomicAdd(&total, c);
    __syncthreads();
    if (threadIdx.x == 0 && total) atomicAdd(ngroups, total);
}

// +1 into cnt[label] for every body of the replica, taken in SORTED order: the lanes of a wave are neighbours in space and mostly share
// a group.  With COMBINE each round takes the label of the first pending lane and the lanes that share it (ballot, readlane), and the
// leader carries the count of all of them, as raster_bin does for a pixel (nb_raster.hip.h); a lane still pending after the rounds
// carries its own.  COMBINE = false: one add per body, the A/B (n serial adds on one counter when all bodies share a group).
// Workgroup b takes the batches b, b + gridDim.x, ... of BLOCK sorted positions.  What the FIRST round of a wave found (the label of
// its first lane and how many lanes share it: in a large group nearly the whole wave) does not go to memory either: the waves leave
// it in LDS, one thread per distinct label adds up the waves that agree and keeps the sum in a register for as long as the next
// batches bring the same label; it reaches memory when the label changes and at the end.  One giant group is then a few adds per
// WORKGROUP on its counter.  The later rounds and the lanes left over add for themselves.
template <bool COMBINE>
__global__ __launch_bounds__(BLOCK)
void groups_tally(const uint32_t *__restrict__ label, const uint32_t *__restrict__ sval, uint32_t n, uint32_t *__restrict__ cnt)
{
    constexpr uint32_t WAVES = BLOCK / 64;
    const uint32_t batches = (n + BLOCK - 1) / BLOCK;
    if constexpr (!COMBINE) {
        for (uint32_t b = blockIdx.x; b < batches; b += gridDim.x) {
            const uint32_t p = b * BLOCK + threadIdx.x;
            if (p < n) atomicAdd(&cnt[label[sval[p]]], 1u);
        }
    } else {
        __shared__ uint32_t wr[WAVES], wc[WAVES];
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        uint32_t held = GROUPS_NONE, sum = 0u;                           // threads 0 .. WAVES - 1: the label carried between batches
        for (uint32_t b = blockIdx.x; b < batches; b += gridDim.x) {      // workgroup-uniform: every thread meets every barrier
            const uint32_t p = b * BLOCK + threadIdx.x;
            const bool active = p < n;
            const uint32_t r = active ? label[sval[p]] : GROUPS_NONE;
            bool pending = active, carry = false;
            uint32_t c = 1u;
            if (lane == 0u) wc[wave] = 0u;                                // a wave without a body leaves nothing
            for (int round = 0; round < GROUPS_WAVE_ROUNDS; ++round) {
                const unsigned long long todo = __ballot(pending);
                if (!todo) break;                                         // wave-uniform
                const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
                const uint32_t lr = (uint32_t)__builtin_amdgcn_readlane((int)r, (int)lead);
                const bool same = pending && r == lr;
                const uint32_t members = (uint32_t)__popcll(__ballot(same));
                if (lane == lead) {
                    if (round == 0) { wr[wave] = r; wc[wave] = members; }  // (behind lane 0's store in this wave's program order)
                    else { carry = true; c = members; }
                }
                pending = pending && !same;
            }
            if (pending || carry) atomicAdd(&cnt[r], c);
            __syncthreads();
            if (threadIdx.x < WAVES) {
                const uint32_t t = threadIdx.x, lr = wr[t];
                uint32_t total = wc[t];
                bool first = total != 0u;
                for (uint32_t u = 0; u < t; ++u) first = first && !(wc[u] != 0u && wr[u] == lr);
                if (first) {                                              // the first wave with this label takes the others'
                    for (uint32_t u = t + 1u; u < WAVES; ++u)
                        if (wc[u] != 0u && wr[u] == lr) total += wc[u];
                    if (lr == held) sum += total;
                    else {
                        if (sum) atomicAdd(&cnt[held], sum);
                        held = lr;
                        sum = total;
                    }
                }
            }
            __syncthreads();                                              // the next batch writes wr / wc again
        }
        if (sum) atomicAdd(&cnt[held], sum);
    }
}

__global__ __launch_bounds__(BLOCK)
void groups_sizes(const uint32_t *__restrict__ label, const uint32_t *__restrict__ cnt, uint32_t i_begin, uint32_t i_count,
                  uint32_t *__restrict__ size)
{
    const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
    if (row < i_count) size[row] = cnt[label[i_begin + row]];
}

}  // namespace nbk
