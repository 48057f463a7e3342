// nb_collide.hip.h — hard-sphere collisions after the drift (NB_EXTRA_COLLIDE): the reference's collide() / resolve(),
// Simulation.hpp:216-346, for unsharded 2-D handles.
//
// Semantics (include/nbody.h): P = every unordered pair i < j whose discs overlap at the post-drift
// positions (fp `d.x*d.x + d.y*d.y <= (r_i + r_j)^2`, one rounding per operation), fixed before anything is resolved; then
// resolve(i, j) once per pair of P in ascending (i, j) order, each time on the current state of both bodies.
//
// Pipeline (one step, all on the handle's stream, no host sync):
//   collide_clear        cell table heads <- -1, per-body pair counts <- 0
//   collide_hash         small bodies into a hashed uniform grid (cell size h >= twice the largest small radius): a per-cell
//                        linked list built with atomicExch, whose order does not matter
//   collide_rows<false>  per small body: overlapping partners in the 3x3 cells around it, plus every large body: its count
//   collide_large_bits   per large body: a bitmap of its overlapping partners among all n (<= 64 large bodies), its count
//   collide_scan_*       exclusive scan of the counts -> row offsets (three launches, below); the touched bodies (count > 0)
//                        get consecutive local indices; capacity check, statistics
//   collide_rows<true>   per small body: its row of partners (local indices), sorted ascending
//   collide_large_fill   per large body: its bitmap compacted in index order (already sorted)
//   collide_resolve      ONE workgroup: the pairs in rounds (below)
// Every pair sits in the rows of both its bodies, so row b in ascending partner order IS body b's pairs in (i, j) key order:
// partners a < b give keys (a, b), ascending in a, and they all precede the keys (b, c), ascending in c.  Nothing depends on
// the order in which the atomics ran: counts are sums, rows are sorted, bitmaps are compacted in index order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nbk {

constexpr int COLLIDE_THREADS = 1024;                 // the one workgroup of collide_resolve
constexpr uint32_t COLLIDE_MAX_LARGE = 64;            // large bodies tested against all n; more than this: no large set
constexpr size_t COLLIDE_LDS_BYTES = 159 * 1024;      // gfx950: a workgroup may hold all 160 KiB of a CU; 1 KiB stays for __syncthreads_or
constexpr int COLLIDE_NO_CELL = INT32_MIN;            // large or non-finite bodies are in no cell

// Device-side record of the collision path (one per handle).  Written with plain stores by ONE thread of collide_scan_top
// and of collide_resolve; read by the host at the synchronising calls.
struct CollideStats {
    uint64_t pairs_last;        // |P| of the last step (also when it was over capacity)
    uint64_t pairs_total;       // pairs resolved since creation
    uint64_t overflow_steps;    // steps whose |P| exceeded the capacity (nothing resolved in them)
    uint64_t overflow_frame;    // the frame the last such step ended at ...
    uint64_t overflow_needed;   // ... and its |P|
    uint32_t touched;           // bodies in at least one pair of the last step
    uint32_t skip;              // 1: the last step was over capacity
    uint32_t rounds_last;       // resolution rounds of the last step
    uint32_t lds_last;          // 1: the last resolution staged its bodies in LDS, 0: it ran on global memory
};

// The candidate predicate, the reference's `d.mag_sq() > r * r` negated (Simulation.hpp:298-302): d = p_j - p_i.  Called
// with (lo, hi) = (min, max) of the pair whichever body asks, so both ends of a pair see the same bits.
template <typename real>
__device__ __forceinline__ bool discs_overlap(real xi, real yi, float ri, real xj, real yj, float rj)
{
#pragma clang fp contract(off)
    const real dx = xj - xi, dy = yj - yi;
    const real r = (real)ri + (real)rj;
    return dx * dx + dy * dy <= r * r;
}

template <typename vec>
__device__ __forceinline__ bool pair_overlaps(const vec *__restrict__ pos, const float *__restrict__ radius, uint32_t a, uint32_t b)
{
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    const vec p = pos[lo], q = pos[hi];
    return discs_overlap(p.x, p.y, radius[lo], q.x, q.y, radius[hi]);
}

// Cell of a coordinate: floor(v / h) in double (positions are at most doubles, so the quotient carries 2^-52 relative error
// against the 2^-16 by which h exceeds twice the largest small radius), clamped so that +-1 neighbours stay in int range.
__device__ __forceinline__ int cell_coord(double v, double inv_h)
{
    const double c = floor(v * inv_h);
    return (int)fmin(fmax(c, -1073741824.0), 1073741823.0);
}

__device__ __forceinline__ uint32_t cell_slot(int cx, int cy, uint32_t mask)
{
    uint32_t h = (uint32_t)cx * 0x9E3779B1u ^ (uint32_t)cy * 0x85EBCA77u;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 13;
    return h & mask;
}

__global__ __launch_bounds__(BLOCK)
void collide_clear(int *__restrict__ head, uint32_t slots, uint32_t *__restrict__ deg, uint32_t n)
{
    const uint32_t stride = gridDim.x * BLOCK;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < slots || i < n; i += stride) {
        if (i < slots) head[i] = -1;
        if (i < n) deg[i] = 0;
    }
}

template <typename vec>
__global__ __launch_bounds__(BLOCK)
void collide_hash(const vec *__restrict__ pos, uint32_t n, const uint8_t *__restrict__ large, double inv_h, uint32_t mask,
                  int *__restrict__ head, int *__restrict__ next, int2 *__restrict__ cell)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double x = (double)pos[i].x, y = (double)pos[i].y;
    // a non-finite coordinate never passes the predicate (inf - inf, NaN), so such a body needs no cell
    if (large[i] || !isfinite(x) || !isfinite(y)) { cell[i] = make_int2(COLLIDE_NO_CELL, COLLIDE_NO_CELL); return; }
    const int cx = cell_coord(x, inv_h), cy = cell_coord(y, inv_h);
    cell[i] = make_int2(cx, cy);
    next[i] = atomicExch(&head[cell_slot(cx, cy, mask)], (int)i);
}

// Partners of small body i: small ones from the 3x3 cells around its own (a body is visited only from its own cell, so hash
// collisions between cells cost a comparison, never a duplicate), then every large body.  FILL = false: count them into
// deg[i].  FILL = true: write them as local indices into row i (off[i] .. off[i + 1]) and sort the row.
template <typename vec, bool FILL>
__global__ __launch_bounds__(BLOCK)
void collide_rows(const vec *__restrict__ pos, const float *__restrict__ radius, uint32_t n, const uint8_t *__restrict__ large,
                  const uint32_t *__restrict__ large_list, uint32_t n_large, uint32_t mask, const int *__restrict__ head,
                  const int *__restrict__ next, const int2 *__restrict__ cell, uint32_t *__restrict__ deg,
                  const uint32_t *__restrict__ off, const uint32_t *__restrict__ tidx, uint32_t *__restrict__ adj,
                  const CollideStats *__restrict__ st)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || large[i]) return;
    uint32_t base = 0, len = 0;
    if constexpr (FILL) {
        if (st->skip) return;
        base = off[i];
        len = off[i + 1] - base;
        if (len == 0) return;
    }
    uint32_t k = 0;
    auto take = [&](uint32_t j) {
        if constexpr (FILL) { if (k < len) adj[base + k] = tidx[j]; }
        ++k;
    };
    const int2 c = cell[i];
    if (c.x != COLLIDE_NO_CELL) {
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int cx = c.x + dx, cy = c.y + dy;
                for (int j = head[cell_slot(cx, cy, mask)]; j >= 0; j = next[j]) {
                    const int2 cj = cell[j];
                    if ((uint32_t)j == i || cj.x != cx || cj.y != cy) continue;
                    if (pair_overlaps(pos, radius, i, (uint32_t)j)) take((uint32_t)j);
                }
            }
    }
    for (uint32_t l = 0; l < n_large; ++l) {
        const uint32_t j = large_list[l];
        if (pair_overlaps(pos, radius, i, j)) take(j);
    }
    if constexpr (!FILL) {
        deg[i] = k;
    } else {
        // insertion sort of the row (rows are short: the bodies one small disc touches)
        for (uint32_t a = base + 1; a < base + len; ++a) {
            const uint32_t v = adj[a];
            uint32_t b = a;
            while (b > base && adj[b - 1] > v) { adj[b] = adj[b - 1]; --b; }
            adj[b] = v;
        }
    }
}

// Large body large_list[blockIdx.y] against all n: word w of its bitmap holds bodies 32 w .. 32 w + 31.
template <typename vec>
__global__ __launch_bounds__(BLOCK)
void collide_large_bits(const vec *__restrict__ pos, const float *__restrict__ radius, uint32_t n, const uint32_t *__restrict__ large_list,
                        uint32_t words, uint32_t *__restrict__ bits, uint32_t *__restrict__ deg)
{
    const uint32_t w = blockIdx.x * BLOCK + threadIdx.x;
    if (w >= words) return;
    const uint32_t L = large_list[blockIdx.y];
    uint32_t word = 0;
    for (uint32_t b = 0; b < 32; ++b) {
        const uint32_t j = 32 * w + b;
        if (j < n && j != L && pair_overlaps(pos, radius, L, j)) word |= 1u << b;
    }
    bits[(size_t)blockIdx.y * words + w] = word;
    if (word) atomicAdd(&deg[L], (uint32_t)__popc(word));
}

// Exclusive scan over a workgroup of BLOCK (= 4 waves) threads without a barrier per step: each wave scans with lane shuffles,
// then the four wave totals go through LDS.  Returns the sum of the values of the threads before this one; *total the sum of
// all.  `sh` holds BLOCK / 64 elements.
template <typename T>
__device__ T wave_block_exclusive_scan(T v, T *sh, T *total)
{
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T inc = v;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T u = __shfl_up(inc, d, 64);
        if (lane >= d) inc += u;
    }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    T before = 0, all = 0;
    for (uint32_t k = 0; k < BLOCK / 64; ++k) {
        if (k < w) before += sh[k];
        all += sh[k];
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

// The scan of the pair counts in three launches over chunks of COLLIDE_SCAN_CHUNK bodies, every load coalesced:
//   collide_scan_blocks  per chunk: its entries (sum of deg) and its touched bodies (deg > 0)
//   collide_scan_top     one workgroup: exclusive prefixes of the chunk sums; the totals, the capacity check, the statistics
//   collide_scan_fill    per chunk: off[i] = entries before i (off[n] = all of them, two per pair), tidx[i] = local index of a
//                        touched body, tlist[local] = its body
// Over capacity (more than cap_pairs pairs): skip = 1, the fill and everything after it do nothing, the step resolves nothing.
constexpr uint32_t COLLIDE_SCAN_PER_THREAD = 16;
constexpr uint32_t COLLIDE_SCAN_CHUNK = BLOCK * COLLIDE_SCAN_PER_THREAD;

__global__ __launch_bounds__(BLOCK)
void collide_scan_blocks(const uint32_t *__restrict__ deg, uint32_t n, uint64_t *__restrict__ chunk_e, uint32_t *__restrict__ chunk_t)
{
    __shared__ uint64_t sh_e[BLOCK / 64];
    __shared__ uint32_t sh_t[BLOCK / 64];
    const size_t base = (size_t)blockIdx.x * COLLIDE_SCAN_CHUNK;
    uint64_t e = 0;
    uint32_t c = 0;
    for (uint32_t k = 0; k < COLLIDE_SCAN_PER_THREAD; ++k) {
        const size_t i = base + (size_t)k * BLOCK + threadIdx.x;
        const uint32_t d = i < n ? deg[i] : 0u;
        e += d;
        c += d != 0;
    }
    uint64_t e_all;
    uint32_t c_all;
    (void)wave_block_exclusive_scan(e, sh_e, &e_all);
    (void)wave_block_exclusive_scan(c, sh_t, &c_all);
    if (threadIdx.x == 0) { chunk_e[blockIdx.x] = e_all; chunk_t[blockIdx.x] = c_all; }
}

__global__ __launch_bounds__(BLOCK)
void collide_scan_top(uint64_t *__restrict__ chunk_e, uint32_t *__restrict__ chunk_t, uint32_t chunks, uint32_t n,
                      uint32_t *__restrict__ off, CollideStats *__restrict__ st, uint64_t cap_pairs, uint64_t frame)
{
    __shared__ uint64_t sh_e[BLOCK / 64];
    __shared__ uint32_t sh_t[BLOCK / 64];
    const uint32_t t = threadIdx.x, per = (chunks + BLOCK - 1) / BLOCK;
    const uint32_t lo = t * per < chunks ? t * per : chunks, hi = lo + per < chunks ? lo + per : chunks;
    uint64_t e = 0;
    uint32_t c = 0;
    for (uint32_t b = lo; b < hi; ++b) { e += chunk_e[b]; c += chunk_t[b]; }
    uint64_t e_all;
    uint32_t c_all;
    uint64_t e0 = wave_block_exclusive_scan(e, sh_e, &e_all);
    uint32_t c0 = wave_block_exclusive_scan(c, sh_t, &c_all);
    for (uint32_t b = lo; b < hi; ++b) {           // each chunk's sums become its exclusive prefixes
        const uint64_t de = chunk_e[b];
        const uint32_t dc = chunk_t[b];
        chunk_e[b] = e0; chunk_t[b] = c0;
        e0 += de; c0 += dc;
    }
    if (t == 0) {
        const uint64_t pairs = e_all / 2;
        const bool skip = pairs > cap_pairs;
        st->pairs_last = pairs;
        st->touched = skip ? 0u : c_all;
        st->skip = skip ? 1u : 0u;
        if (skip) {
            st->overflow_steps += 1;
            st->overflow_frame = frame;
            st->overflow_needed = pairs;
        } else {
            st->pairs_total += pairs;
            off[n] = (uint32_t)e_all;              // <= 2 x capacity < 2^32
        }
    }
}

__global__ __launch_bounds__(BLOCK)
void collide_scan_fill(const uint32_t *__restrict__ deg, uint32_t n, const uint64_t *__restrict__ chunk_e, const uint32_t *__restrict__ chunk_t,
                       uint32_t *__restrict__ off, uint32_t *__restrict__ tidx, uint32_t *__restrict__ tlist, const CollideStats *__restrict__ st)
{
    __shared__ uint64_t sh_e[BLOCK / 64];
    __shared__ uint32_t sh_t[BLOCK / 64];
    if (st->skip) return;
    const size_t base = (size_t)blockIdx.x * COLLIDE_SCAN_CHUNK;
    uint64_t e0 = chunk_e[blockIdx.x];
    uint32_t c0 = chunk_t[blockIdx.x];
    for (uint32_t k = 0; k < COLLIDE_SCAN_PER_THREAD; ++k) {
        const size_t i = base + (size_t)k * BLOCK + threadIdx.x;
        const uint32_t d = i < n ? deg[i] : 0u;
        uint64_t e_all;
        uint32_t c_all;
        const uint64_t e = e0 + wave_block_exclusive_scan((uint64_t)d, sh_e, &e_all);
        const uint32_t c = c0 + wave_block_exclusive_scan(d != 0 ? 1u : 0u, sh_t, &c_all);
        if (i < n) {
            off[i] = (uint32_t)e;
            tidx[i] = d ? c : 0xffffffffu;
            if (d) tlist[c] = (uint32_t)i;
        }
        e0 += e_all;
        c0 += c_all;
    }
}

// Large body large_list[blockIdx.x]: its bitmap compacted into its row, in index order.
__global__ __launch_bounds__(BLOCK)
void collide_large_fill(const uint32_t *__restrict__ bits, uint32_t words, const uint32_t *__restrict__ large_list,
                        const uint32_t *__restrict__ off, const uint32_t *__restrict__ tidx, uint32_t *__restrict__ adj,
                        const CollideStats *__restrict__ st)
{
    __shared__ uint32_t sh[BLOCK / 64];
    if (st->skip) return;
    const uint32_t L = large_list[blockIdx.x], end = off[L + 1];
    uint32_t base = off[L];
    const uint32_t *row = bits + (size_t)blockIdx.x * words;
    for (uint32_t w0 = 0; w0 < words; w0 += BLOCK) {
        const uint32_t w = w0 + threadIdx.x;
        uint32_t word = w < words ? row[w] : 0u;
        uint32_t total;
        uint32_t k = base + wave_block_exclusive_scan((uint32_t)__popc(word), sh, &total);
        while (word) {
            const uint32_t b = (uint32_t)__ffs(word) - 1;
            word &= word - 1;
            if (k < end) adj[k] = tidx[32 * w + b];
            ++k;
        }
        base += total;
    }
}

// resolve(i, j), Simulation.hpp:293-346, restated with one rounding per operation (no contraction): the early return, the
// two branches, the discriminant clamp, 1.5 and the weights.  Vec2::dot (_mm_dp_ps(a, b, 0x31)) rounds both products and
// then their sum: the same bits as x * ox + y * oy.  b1 / b2 are references into `bodies` there, so vel reads before the
// store of v1 / v2 see the old velocities, and new_d sees the positions moved back by vel * t.
template <typename real, typename vec>
__device__ __forceinline__ void resolve_pair(vec &p1, vec &v1, vec &p2, vec &v2, real m1, real m2, float r1, float r2)
{
#pragma clang fp contract(off)
    const real dx = p2.x - p1.x, dy = p2.y - p1.y;
    const real r = (real)r1 + (real)r2;
    if (dx * dx + dy * dy > r * r) return;
    const real vx = v2.x - v1.x, vy = v2.y - v1.y;
    const real d_dot_v = dx * vx + dy * vy;
    const real weight1 = m2 / (m1 + m2), weight2 = m1 / (m1 + m2);
    if (d_dot_v >= (real)0 && !(dx == (real)0 && dy == (real)0)) {
        const real s = r / sqrt(dx * dx + dy * dy) - (real)1;
        const real tx = dx * s, ty = dy * s;
        p1.x -= tx * weight1; p1.y -= ty * weight1;
        p2.x += tx * weight2; p2.y += ty * weight2;
        return;
    }
    const real v_sq = vx * vx + vy * vy, d_sq = dx * dx + dy * dy, r_sq = r * r;
    real disc = d_dot_v * d_dot_v - v_sq * (d_sq - r_sq);
    if (disc < (real)0) disc = (real)0;
    const real t = (d_dot_v + sqrt(disc)) / v_sq;
    p1.x -= v1.x * t; p1.y -= v1.y * t;
    p2.x -= v2.x * t; p2.y -= v2.y * t;
    const real ndx = p2.x - p1.x, ndy = p2.y - p1.y;
    const real nd_dot_v = ndx * vx + ndy * vy;
    const real nd_sq = ndx * ndx + ndy * ndy;
    const real k = (real)1.5 * nd_dot_v / nd_sq;
    const real tx = ndx * k, ty = ndy * k;
    vec n1, n2;
    n1.x = v1.x + tx * weight1; n1.y = v1.y + ty * weight1;
    n2.x = v2.x - tx * weight2; n2.y = v2.y - ty * weight2;
    v1 = n1; v2 = n2;
    p1.x += n1.x * t; p1.y += n1.y * t;
    p2.x += n2.x * t; p2.y += n2.y * t;
}

// The pairs of P in rounds, in ONE workgroup.  Every touched body b keeps a cursor into its row (its pairs in key order);
// pairs before the cursor are resolved, the rest pending.  A pair is READY when it is the pair under the cursors of both its
// bodies, i.e. the lowest pending pair of each.  Ready pairs are disjoint (a cursor names one pair), so a round resolves
// them all at once; the lower body's thread does the arithmetic, then both cursors advance.  The lowest pending pair of all
// is always ready (nothing below it is pending for either body), so each round resolves at least one pair and the loop ends
// after at most |P| rounds.  BIT-IDENTICAL TO THE SEQUENTIAL ASCENDING PASS: resolve(i, j) reads and writes only bodies i
// and j; in the sequential pass it sees each of them as left by that body's pairs with smaller keys, all of them and nothing
// else.  Here the cursors resolve each body's pairs in key order and pair (i, j) runs only when both cursors stand on it, so
// it sees exactly the same two states, whatever else ran in the same or earlier rounds.
//
// The touched bodies' positions, velocities and cursors are staged in LDS when they fit else in
// the global scratch arrays; either way one workgroup runs every round, and __syncthreads() orders the rounds (all its waves
// share one CU and its L1).
template <typename real, typename vec>
__global__ __launch_bounds__(COLLIDE_THREADS)
void collide_resolve(vec *__restrict__ pos, vec *__restrict__ vel, const real *__restrict__ mass, const float *__restrict__ radius,
                     const uint32_t *__restrict__ off, const uint32_t *__restrict__ tlist, const uint32_t *__restrict__ adj,
                     CollideStats *__restrict__ st, vec *g_pos, vec *g_vel, uint32_t *g_cur, uint8_t *g_adv)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[COLLIDE_LDS_BYTES];
    const uint32_t tid = threadIdx.x;
    const uint32_t T = st->touched;
    if (st->skip || T == 0) {
        if (tid == 0) { st->rounds_last = 0; st->lds_last = 0; }
        return;
    }
    const bool lds = (size_t)T * (2 * sizeof(vec) + sizeof(uint32_t) + 1) <= COLLIDE_LDS_BYTES;
    vec *P = lds ? (vec *)smem : g_pos;
    vec *V = lds ? (vec *)smem + T : g_vel;
    uint32_t *cur = lds ? (uint32_t *)((vec *)smem + 2 * (size_t)T) : g_cur;
    uint8_t *adv = lds ? (uint8_t *)(cur + T) : g_adv;
    for (uint32_t t = tid; t < T; t += COLLIDE_THREADS) {
        const uint32_t g = tlist[t];
        P[t] = pos[g];
        V[t] = vel[g];
        cur[t] = 0;
        adv[t] = 0;
    }
    __syncthreads();
    const uint64_t pairs = st->pairs_last;
    uint32_t rounds = 0;
    for (;;) {
        // phase A: find the ready pairs and resolve them; cursors are only read
        for (uint32_t t = tid; t < T; t += COLLIDE_THREADS) {
            const uint32_t g = tlist[t], o = off[g], c = cur[t];
            uint8_t ready = 0;
            if (c < off[g + 1] - o) {
                const uint32_t p = adj[o + c], gp = tlist[p], op = off[gp], cp = cur[p];
                if (cp < off[gp + 1] - op && adj[op + cp] == t) {
                    ready = 1;
                    if (t < p) {
                        vec p1 = P[t], v1 = V[t], p2 = P[p], v2 = V[p];
                        resolve_pair<real, vec>(p1, v1, p2, v2, mass[g], mass[gp], radius[g], radius[gp]);
                        P[t] = p1; V[t] = v1; P[p] = p2; V[p] = v2;
                    }
                }
            }
            adv[t] = ready;
        }
        __syncthreads();
        // phase B: advance the cursors of the resolved pairs' bodies
        int pending = 0;
        for (uint32_t t = tid; t < T; t += COLLIDE_THREADS) {
            const uint32_t g = tlist[t], c = cur[t] + adv[t];
            cur[t] = c;
            if (c < off[g + 1] - off[g]) pending = 1;
        }
        ++rounds;
        // at most |P| rounds (above); the bound only guards the loop against rows that were not built as described
        if (!__syncthreads_or(pending) || rounds > pairs) break;
    }
    for (uint32_t t = tid; t < T; t += COLLIDE_THREADS) {
        const uint32_t g = tlist[t];
        pos[g] = P[t];
        vel[g] = V[t];
    }
    if (tid == 0) { st->rounds_last = rounds; st->lds_last = lds ? 1u : 0u; }
}

} // namespace nbk
