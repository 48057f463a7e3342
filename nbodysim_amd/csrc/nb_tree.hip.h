// nb_tree.hip.h — Barnes-Hut force (NB_FORCE_TREE, include/nbody.h): the reference's Quadtree::build / Quadtree::acc
// (Quadtree.hpp:35-93,113-170,236-258) as a parallel build that produces the SAME cells, centres of mass and visit order,
// so that with RSQ_QUAKE every body sees the reference's arithmetic bit for bit (tests/tree_model.py is the CPU statement).
//
// Why a parallel build can be exact: with one body per leaf the reference's tree does not depend on the insertion order —
// a cell is a branch exactly when it holds two different positions, a branch has its four children in quadrant order, the
// walk is a pre-order traversal and a branch sums its children 0..3.  Only node INDICES depend on the order.
//
// One force evaluation (all on the handle's stream, no host synchronisation, no floating-point atomics):
//   tree_bounds / tree_root   min / max of the positions -> root cell, cell size^2 per depth, per-step counters reset
//   tree_keys                 one thread per body descends TREE_DEPTH_CAP levels with the reference's rounded child centres
//                             (Quad.hpp:47-57) and packs the quadrants taken into a 126-bit key (2 bits per level, most
//                             significant first; the top bit marks a massless body, which is not inserted and sorts last)
//   2 x rocprim radix sort    bodies by (key, body index): low word, then stable by the high word (nb_tree_prims.hip)
//   tree_heads + scan         equal keys = one position = one leaf ("point"); two DIFFERENT positions with equal keys are
//                             not separated within the cap: the build fails (reported like a collision overflow)
//   tree_count + scan         nodes each point contributes to the pre-order layout (below) -> its first node index
//   tree_emit                 writes the nodes: record {com.x, com.y, mass, size^2}, next (= index + subtree size), depth
//   tree_com (per level)      centres of mass bottom-up, children 0..3 in order (Quadtree.hpp:236-258); with
//                             NB_FLAG_TREE_QUADRUPOLE also the second moments about them (tree_com<true>, below)
//   tree_walk                 Quadtree::acc per body, bodies in key order so that a wave's lanes walk neighbouring paths; with
//                             NB_FLAG_TREE_RELATIVE the acceptance test also looks at the body's previous acceleration (REL, below)
//   tree_integrate            kick_drift_one (nb_kernels.hip.h) unless the build failed
// nb_energy of a NB_FLAG_TREE_ENERGY handle runs the build (bounds ... tree_com) and then tree_potential_group / _alone in place of
// the walk: the potential over the nodes the wave-uniform walk takes, in fp64 (below).
//
// Pre-order layout from the sorted points.  Let L(u) be the number of leading levels points u and u + 1 share (-1 past
// either end) and d(u) = max(L(u - 1), L(u)) + 1 the depth of point u's leaf.  Between leaf u - 1 and leaf u the traversal
//   leaves the cells of depth d(u-1) - 1 ... L(u-1) + 1 of point u - 1: the quadrants after its own are empty leaves;
//   at their common cell (depth L(u-1)) passes the empty quadrants between the two;
//   enters the cells of depth L(u-1) + 1 ... d(u) - 1 of point u: a branch, then the empty quadrants before u's own;
//   and reaches leaf u.
// Point u writes exactly these nodes (point 0 starts at the root, a virtual point U closes the cells of the last one), so
// a prefix sum of the counts gives every point its first index.  A branch ends where its last point's closing run ends.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nb_tree_prims.h"

namespace nbk {

// Levels a path is followed for.  Measured leaf depths (nb_tree_stats; DESIGN.md has the runs): the reference's 25 000 default
// bodies 16, Plummer spheres of 1 048 576 bodies 23 and of 8 388 608 bodies 28.
constexpr int TREE_DEPTH_CAP = 63;
constexpr int TREE_HI_LEVELS = 31;                 // levels 0..30 in the high word (bit 63 = massless), 31..62 in the low word
constexpr uint64_t TREE_MASSLESS = 1ull << 63;
constexpr uint32_t TREE_BOUNDS_BLOCKS = 1024;

struct TreeStats {
    uint32_t fail;               // this evaluation: 0 ok, 1 node capacity, 2 depth cap
    uint32_t massive;            // bodies inserted (mass != 0)
    uint32_t points;             // different positions among them
    uint32_t max_depth;          // deepest leaf of this evaluation
    uint64_t nodes;              // nodes of this evaluation (needed, also when over capacity)
    uint64_t overflow_steps;     // evaluations that failed since creation
    uint64_t overflow_frame;     // frame counter of the last one
    uint64_t overflow_needed;    // nodes it needed (capacity) / sorted position of the unseparated pair (depth)
    uint32_t overflow_kind;      // its `fail` value
    uint32_t _pad;
};

struct TreeRoot { float cx, cy, size, _pad; float s2[TREE_DEPTH_CAP + 1]; };

__device__ __forceinline__ uint32_t tree_digit(uint64_t hi, uint64_t lo, int l)
{
    return l < TREE_HI_LEVELS ? (uint32_t)(hi >> (60 - 2 * l)) & 3u : (uint32_t)(lo >> (62 - 2 * (l - TREE_HI_LEVELS))) & 3u;
}

// leading levels two DIFFERENT keys of inserted bodies share
__device__ __forceinline__ int tree_lcp(uint64_t ah, uint64_t al, uint64_t bh, uint64_t bl)
{
    const uint64_t x = ah ^ bh;
    if (x) return (__clzll((long long)x) - 2) >> 1;
    return TREE_HI_LEVELS + (__clzll((long long)(al ^ bl)) >> 1);
}

// ---- bounds ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void tree_bounds(const float2 *__restrict__ pos, uint32_t n, float4 *__restrict__ part)
{
    __shared__ float4 sh[256];
    float lx = 3.402823466e38f, ly = lx, hx = -lx, hy = -lx;        // Quad.hpp:32-33
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const float2 p = pos[i];
        lx = fminf(lx, p.x); ly = fminf(ly, p.y); hx = fmaxf(hx, p.x); hy = fmaxf(hy, p.y);
    }
    sh[threadIdx.x] = make_float4(lx, ly, hx, hy);
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const float4 a = sh[threadIdx.x], b = sh[threadIdx.x + s];
            sh[threadIdx.x] = make_float4(fminf(a.x, b.x), fminf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(256)
void tree_root(const float4 *__restrict__ part, uint32_t blocks, TreeRoot *__restrict__ root, TreeStats *__restrict__ st)
{
#pragma clang fp contract(off)
    __shared__ float4 sh[256];
    float lx = 3.402823466e38f, ly = lx, hx = -lx, hy = -lx;
    for (uint32_t i = threadIdx.x; i < blocks; i += 256u) {
        const float4 p = part[i];
        lx = fminf(lx, p.x); ly = fminf(ly, p.y); hx = fmaxf(hx, p.z); hy = fmaxf(hy, p.w);
    }
    sh[threadIdx.x] = make_float4(lx, ly, hx, hy);
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const float4 a = sh[threadIdx.x], b = sh[threadIdx.x + s];
            sh[threadIdx.x] = make_float4(fminf(a.x, b.x), fminf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float4 b = sh[0];
        root->cx = (b.x + b.z) * 0.5f;                               // Quad.hpp:40-44
        root->cy = (b.y + b.w) * 0.5f;
        const float ex = b.z - b.x, ey = b.w - b.y;
        float size = ex > ey ? ex : ey;
        root->size = size;
        for (int l = 0; l <= TREE_DEPTH_CAP; ++l) { root->s2[l] = size * size; size = size * 0.5f; }
        st->fail = 0; st->massive = 0; st->points = 0; st->max_depth = 0; st->nodes = 0;
    }
}

// ---- path keys ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void tree_keys(const float2 *__restrict__ pos, const float *__restrict__ mass, uint32_t n, const TreeRoot *__restrict__ root,
               uint64_t *__restrict__ khi, uint64_t *__restrict__ klo, uint32_t *__restrict__ val, TreeStats *__restrict__ st)
{
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool inserted = i < n && mass[i] != 0.0f;
    const uint64_t wave = __ballot(inserted);                                 // one counter update per wave
    if ((threadIdx.x & 63u) == 0 && wave) atomicAdd(&st->massive, (uint32_t)__popcll(wave));
    if (i >= n) return;
    val[i] = i;
    if (!inserted) { khi[i] = TREE_MASSLESS; klo[i] = 0; return; }
    const float2 p = pos[i];
    float cx = root->cx, cy = root->cy, size = root->size;
    uint64_t hi = 0, lo = 0;
    for (int l = 0; l < TREE_DEPTH_CAP; ++l) {
        const uint32_t qx = p.x > cx ? 1u : 0u, qy = p.y > cy ? 1u : 0u;      // Quad.hpp:47-49
        const uint64_t q = (uint64_t)((qy << 1) | qx);
        if (l < TREE_HI_LEVELS) hi |= q << (60 - 2 * l); else lo |= q << (62 - 2 * (l - TREE_HI_LEVELS));
        size = size * 0.5f;                                                   // Quad.hpp:51-57
        cx = cx + ((float)qx - 0.5f) * size;
        cy = cy + ((float)qy - 0.5f) * size;
    }
    khi[i] = hi; klo[i] = lo;
}

__global__ __launch_bounds__(256)
void tree_gather_hi(const uint64_t *__restrict__ khi, const uint32_t *__restrict__ val, uint32_t n, uint64_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = khi[val[i]];
}

// ---- points ---------------------------------------------------------------------------------------------------------
// head[i] = 1 where sorted position i starts a new key (i < massive); head[n] = 0 closes the scan.
__global__ __launch_bounds__(256)
void tree_heads(const uint64_t *__restrict__ shi, const uint64_t *__restrict__ klo, const uint32_t *__restrict__ val,
                const float2 *__restrict__ pos, uint32_t n, uint32_t *__restrict__ head, TreeStats *__restrict__ st, uint64_t frame)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n) return;
    uint32_t h = 0;
    if (i < st->massive) {
        h = 1;
        if (i > 0 && shi[i] == shi[i - 1] && klo[val[i]] == klo[val[i - 1]]) {
            h = 0;
            const float2 a = pos[val[i]], b = pos[val[i - 1]];
            if (!(a.x == b.x && a.y == b.y) && atomicMax(&st->fail, 2u) < 2u) {
                st->overflow_kind = 2; st->overflow_frame = frame; st->overflow_needed = i;
                atomicAdd((unsigned long long *)&st->overflow_steps, 1ull);
            }
        }
    }
    head[i] = h;
}

__global__ __launch_bounds__(256)
void tree_points(const uint64_t *__restrict__ shi, const uint64_t *__restrict__ klo, const uint32_t *__restrict__ val,
                 const uint32_t *__restrict__ head, const uint64_t *__restrict__ uidx, uint32_t n,
                 uint64_t *__restrict__ uhi, uint64_t *__restrict__ ulo, uint32_t *__restrict__ ufirst, TreeStats *__restrict__ st)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n) return;
    if (i == n) { st->points = (uint32_t)uidx[n]; return; }
    if (!head[i]) return;
    const uint32_t u = (uint32_t)uidx[i];
    uhi[u] = shi[i]; ulo[u] = klo[val[i]]; ufirst[u] = i;
}

struct TreeKeys { const uint64_t *hi, *lo; uint32_t U; };

__device__ __forceinline__ int tree_L(const TreeKeys &k, uint32_t u)      // levels shared by points u and u + 1; -1 past the ends
{
    if (u + 1u >= k.U || u == 0xffffffffu) return -1;
    return tree_lcp(k.hi[u], k.lo[u], k.hi[u + 1], k.lo[u + 1]);
}

__device__ __forceinline__ int tree_leaf_depth(const TreeKeys &k, uint32_t u)
{
    const int a = tree_L(k, u - 1u), b = tree_L(k, u);
    return (a > b ? a : b) + 1;
}

// empty quadrants passed when the traversal leaves point u's cells from its leaf up to (and including) level `from`
__device__ __forceinline__ uint32_t tree_closing(const TreeKeys &k, uint32_t u, int from, int leaf_depth)
{
    uint32_t c = 0;
    const uint64_t hi = k.hi[u], lo = k.lo[u];
    for (int l = leaf_depth; l >= from; --l) c += 3u - tree_digit(hi, lo, l - 1);
    return c;
}

// cnt[u], u = 0 .. U: nodes point u writes (U: the closing run of the last point; the empty root when there is no point);
// cnt[u] = 0 past U.  n + 2 entries.
__global__ __launch_bounds__(256)
void tree_count(const uint64_t *__restrict__ uhi, const uint64_t *__restrict__ ulo, uint32_t n, uint32_t *__restrict__ cnt,
                TreeStats *__restrict__ st)
{
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u > n + 1u) return;
    const TreeKeys k{uhi, ulo, st->points};
    uint32_t c = 0;
    if (st->fail) c = 0;
    else if (u == k.U) c = k.U ? tree_closing(k, k.U - 1u, 1, tree_leaf_depth(k, k.U - 1u)) : 1u;
    else if (u < k.U) {
        const int lp = tree_L(k, u - 1u), d = tree_leaf_depth(k, u);
        const uint64_t hi = uhi[u], lo = ulo[u];
        if (u > 0) {
            c += tree_closing(k, u - 1u, lp + 2, tree_leaf_depth(k, u - 1u));
            c += tree_digit(hi, lo, lp) - tree_digit(uhi[u - 1], ulo[u - 1], lp) - 1u;
        }
        for (int l = lp + 1; l < d; ++l) c += 1u + tree_digit(hi, lo, l);
        c += 1u;
        if ((uint32_t)d > st->max_depth) atomicMax(&st->max_depth, (uint32_t)d);
    }
    cnt[u] = c;
}

// ---- nodes ----------------------------------------------------------------------------------------------------------
constexpr uint8_t TREE_BRANCH = 0x80;

__global__ __launch_bounds__(256)
void tree_emit(const uint64_t *__restrict__ uhi, const uint64_t *__restrict__ ulo, const uint32_t *__restrict__ ufirst,
               const uint32_t *__restrict__ val, const float2 *__restrict__ pos, const float *__restrict__ mass,
               const uint64_t *__restrict__ base, uint32_t n, const TreeRoot *__restrict__ root, uint64_t cap,
               float4 *__restrict__ nd, uint32_t *__restrict__ nx, uint8_t *__restrict__ dp, TreeStats *__restrict__ st, uint64_t frame)
{
#pragma clang fp contract(off)
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (st->fail == 2u) return;
    const TreeKeys k{uhi, ulo, st->points};
    const uint64_t total = base[n + 1u];                  // exclusive scan of n + 2 counts (64-bit sums): the last entry is the total
    if (total > cap) {
        if (u == 0) {
            st->fail = 1; st->nodes = total; st->overflow_kind = 1; st->overflow_frame = frame; st->overflow_needed = total;
            st->overflow_steps += 1;
        }
        return;
    }
    if (u > k.U) return;
    if (u == 0) st->nodes = total;
    uint32_t w = (uint32_t)base[u];                     // total <= cap < 2^32 from here on
    // (w < total always: tree_count counted exactly these nodes; the bound keeps a disagreement inside the arrays)
    auto put = [&](float4 rec, uint32_t next, uint8_t depth) { if (w < total) { nd[w] = rec; nx[w] = next; dp[w] = depth; } ++w; };
    auto empty = [&](int depth) { put(make_float4(0.f, 0.f, 0.f, root->s2[depth]), w + 1u, (uint8_t)depth); };
    if (u == k.U) {
        if (k.U == 0) { empty(0); return; }
        const uint64_t hi = uhi[u - 1], lo = ulo[u - 1];
        for (int l = tree_leaf_depth(k, u - 1u); l >= 1; --l)
            for (uint32_t q = tree_digit(hi, lo, l - 1) + 1u; q < 4u; ++q) empty(l);
        return;
    }
    const int lp = tree_L(k, u - 1u), d = tree_leaf_depth(k, u);
    const uint64_t hi = uhi[u], lo = ulo[u];
    if (u > 0) {
        const uint64_t phi = uhi[u - 1], plo = ulo[u - 1];
        for (int l = tree_leaf_depth(k, u - 1u); l >= lp + 2; --l)
            for (uint32_t q = tree_digit(phi, plo, l - 1) + 1u; q < 4u; ++q) empty(l);
        for (uint32_t q = tree_digit(phi, plo, lp) + 1u; q < tree_digit(hi, lo, lp); ++q) empty(lp + 1);
    }
    for (int l = lp + 1; l < d; ++l) {
        // the branch of depth l on u's path: u is its first point; its last one is the last point sharing l levels with u
        uint32_t a = u + 1u, b = k.U - 1u;                // (a is inside: L(u) >= l because d > l)
        while (a < b) {
            const uint32_t mid = a + (b - a + 1u) / 2u;
            if (tree_lcp(hi, lo, uhi[mid], ulo[mid]) >= l) a = mid; else b = mid - 1u;
        }
        put(make_float4(0.f, 0.f, 0.f, root->s2[l]), (uint32_t)base[a + 1u] + tree_closing(k, a, l + 1, tree_leaf_depth(k, a)), (uint8_t)l | TREE_BRANCH);
        for (uint32_t q = 0; q < tree_digit(hi, lo, l); ++q) empty(l + 1);
    }
    // the leaf: the position its bodies share, their masses added in ascending body index (Quadtree.hpp:56-60)
    const uint32_t f = ufirst[u], e = u + 1u < k.U ? ufirst[u + 1u] : st->massive;
    const float2 p = pos[val[f]];
    float m = mass[val[f]];
    for (uint32_t j = f + 1u; j < e; ++j) m = m + mass[val[j]];
    put(make_float4(p.x, p.y, m, root->s2[d]), w + 1u, (uint8_t)d);
}

// Centres of mass of the branches of depth `level` (launched for level = TREE_DEPTH_CAP - 1 ... 0): Quadtree.hpp:236-258.
// QUAD (NB_FLAG_TREE_QUADRUPOLE; qm is the moment array, one {xx, xy, yy, 0} per node, +16 B per node = +256 B per body on top of
// the 535 B of a tree handle, allocated for such a handle only; without QUAD it is a null pointer nobody reads): the raw second moment
// M = sum m_k (y_k - c)(y_k - c)^T of the branch about the centre of mass c just stored, from its children's moments (the earlier
// launch) moved to c by the parallel-axis term, children 0..3 in order, no contraction (tests/tree_quad_model.py restates it bit
// for bit).  A leaf or an empty quadrant has M = 0: the pass writes its record when it visits the parent.
template <bool QUAD>
__global__ __launch_bounds__(256)
void tree_com(float4 *__restrict__ nd, const uint32_t *__restrict__ nx, const uint8_t *__restrict__ dp, uint32_t level,
              const TreeStats *__restrict__ st, float4 *__restrict__ qm)
{
#pragma clang fp contract(off)
    if (st->fail || level >= st->max_depth) return;
    const uint32_t total = (uint32_t)st->nodes;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        if (dp[i] != ((uint8_t)level | TREE_BRANCH)) continue;
        float sx = 0.f, sy = 0.f, sm = 0.f;
        uint32_t c = i + 1u;
        for (int q = 0; q < 4 && c < total; ++q) {
            const float4 ch = nd[c];
            sx = sx + ch.x * ch.z;
            sy = sy + ch.y * ch.z;
            sm = sm + ch.z;
            c = nx[c];
        }
        if (sm > 0.f) {
            const float inv = 1.0f / sm;                  // Vec2::operator/=, Vec2.hpp:159-165
            sx = sx * inv; sy = sy * inv;
        }
        nd[i] = make_float4(sx, sy, sm, nd[i].w);
        if constexpr (QUAD) {
            float xx = 0.f, xy = 0.f, yy = 0.f;
            c = i + 1u;
            for (int q = 0; q < 4 && c < total; ++q) {
                const float4 ch = nd[c];
                float4 mc = make_float4(0.f, 0.f, 0.f, 0.f);
                if (dp[c] & TREE_BRANCH) mc = qm[c]; else qm[c] = mc;
                const float ex = ch.x - sx, ey = ch.y - sy;
                xx = xx + (mc.x + ch.z * (ex * ex));
                xy = xy + (mc.y + ch.z * (ex * ey));
                yy = yy + (mc.z + ch.z * (ey * ey));
                c = nx[c];
            }
            qm[i] = make_float4(xx, xy, yy, 0.f);
        }
    }
}

// ---- walk -----------------------------------------------------------------------------------------------------------
// Quadtree::acc (Quadtree.hpp:113-155), one lane per body, bodies in key order.  The nodes are in pre-order: an accepted
// node is left through `next`, any other through index + 1 (a leaf's next IS index + 1, and a leaf adds nothing: the
// reference's leaf ranges are empty).  RSQ_QUAKE: one running sum in visit order, no contraction — the reference's bits.
// RSQ_EXACT: the same acceptance test, the term with v_rsq_f32 and FMA.
// LEAVES (NB_FLAG_TREE_LEAVES): a leaf that is not accepted adds its own term (its record is exact: one position, the summed
// mass), so every inserted body is counted once, in an accepted cell or as its leaf, and theta -> 0 is the direct sum.  The
// nodes visited are the same; an empty quadrant (mass 0) adds nothing and costs no rsqrt.
// Every walk kernel ends in (qm, alpha) and every potential kernel in (lo, qm, aprev, alpha), whatever its flags: qm, tree_com<true>'s
// moment array, is read under QUAD only, and alpha (with aprev = acc[] in the potential kernels) under REL only.  A handle without
// the flag passes a null qm and whatever alpha it holds; neither is touched.
// QUAD (NB_FLAG_TREE_QUADRUPOLE, with LEAVES): an accepted BRANCH
// adds, with d = com - body, R^2 = d^2 + eps^2, M its raw second moment,
//     d * (m R^-3 + 7.5 (d^T M d) R^-7 - 1.5 tr(M) R^-5) - 3 (M d) R^-5
// (the second-order term of the softened potential about the centre of mass; the dipole vanishes there).  The record is loaded on
// acceptance of a branch only; the nodes visited and the acceptance test are unchanged, and a leaf's term, accepted or not, is
// the monopole term above, instruction for instruction.
// REL (NB_FLAG_TREE_RELATIVE, with LEAVES): a node is accepted for a body when it passes the test above AND the
// acceleration-relative one, m size^2 < (g d^2) d^2 with g = alpha |a_prev| of that body, i.e. G m size^2 / d^4 < alpha |a_prev|
// with G = 1 (the opening criterion of GADGET-2).  a_prev is acc[] as the handle holds it: the walks read acc[b] once, before the
// loop, in the thread that overwrites it at the end (no second array, no ordering problem); g is float32, one rounding per
// operation, the square root correctly rounded (tests/tree_rel_model.py restates it with np.sqrt).  g == 0 (alpha = 0, or a body
// whose acc is zero, as in fresh initial conditions) leaves the theta test alone.  theta stays the cap: the relative walk opens
// whatever the theta walk opens and more, never less.  The vote, the windows, the terms and d^2 > 0 are unchanged: the test only
// feeds the comparison that was there.  Every walk and potential kernel takes the new test from tree_far_rel.
__device__ __forceinline__ bool tree_far_rel(float s2, float m, float d2, float g)
{
#pragma clang fp contract(off)
    return (g == 0.f) | (m * s2 < (g * d2) * d2);
}

// g of a body from its previous acceleration.  (__builtin_sqrtf is the correctly rounded square root in device code: the
// __fsqrt_rn intrinsic of this toolchain is the 1-ulp native one)
__device__ __forceinline__ float tree_rel_g(float2 a, float alpha)
{
#pragma clang fp contract(off)
    return alpha * __builtin_sqrtf(a.x * a.x + a.y * a.y);
}

// the monopole term of a node of mass m at displacement (dx, dy): the two bodies of tree_walk_one's `term`, for the group walk
template <int RSQ>
__device__ __forceinline__ void tree_mono_term(float m, float dx, float dy, float d2, float eps2, float &sx, float &sy)
{
    if constexpr (RSQ == RSQ_QUAKE) {
#pragma clang fp contract(off)
        const float inv = quake_rsqrt(d2 + eps2);
        const float inv3 = inv * inv * inv;
        const float s = m * inv3;
        sx = sx + dx * s;
        sy = sy + dy * s;
    } else {
        const float inv = __builtin_amdgcn_rsqf(d2 + eps2);
        const float s = m * (inv * inv * inv);
        sx = __builtin_fmaf(dx, s, sx);
        sy = __builtin_fmaf(dy, s, sy);
    }
}

template <int RSQ>
__device__ __forceinline__ void tree_quad_term(float4 q, float4 m, float dx, float dy, float d2, float eps2, float &sx, float &sy)
{
    if constexpr (RSQ == RSQ_QUAKE) {
#pragma clang fp contract(off)
        const float inv = quake_rsqrt(d2 + eps2);
        const float inv2 = inv * inv, inv3 = inv2 * inv, inv5 = inv3 * inv2, inv7 = inv5 * inv2;
        const float ux = m.x * dx + m.y * dy, uy = m.y * dx + m.z * dy;
        const float rMr = dx * ux + dy * uy, tr = m.x + m.z;
        const float g = q.z * inv3 + (7.5f * (rMr * inv7) - 1.5f * (tr * inv5));
        sx = sx + (dx * g - 3.0f * (ux * inv5));
        sy = sy + (dy * g - 3.0f * (uy * inv5));
    } else {
        const float inv = __builtin_amdgcn_rsqf(d2 + eps2);
        const float inv2 = inv * inv, inv3 = inv2 * inv, inv5 = inv3 * inv2, inv7 = inv5 * inv2;
        const float ux = m.x * dx + m.y * dy, uy = m.y * dx + m.z * dy;
        const float rMr = dx * ux + dy * uy, tr = m.x + m.z;
        const float g = q.z * inv3 + (7.5f * (rMr * inv7) - 1.5f * (tr * inv5));
        sx = sx + (dx * g - 3.0f * (ux * inv5));
        sy = sy + (dy * g - 3.0f * (uy * inv5));
    }
}

template <int RSQ, bool LEAVES, bool QUAD, bool REL>
__device__ __forceinline__ void tree_walk_one(uint32_t i, const float4 *__restrict__ nd, const uint32_t *__restrict__ nx,
                                              const uint32_t *__restrict__ val, const float2 *__restrict__ pos, float eps2, float theta2,
                                              float2 *__restrict__ acc, const TreeStats *__restrict__ st,
                                              const float4 *__restrict__ qm, float alpha)
{
    static_assert(LEAVES || !(QUAD || REL), "the moments and the relative test belong to the convergent walk");
    const uint32_t b = val[i];
    const float2 p = pos[b];
    const uint32_t total = (uint32_t)st->nodes;
    float g = 0.f;
    if constexpr (REL) g = tree_rel_g(acc[b], alpha);
    float sx = 0.f, sy = 0.f;
    uint32_t node = 0;
    while (node < total) {
        const float4 q = nd[node];
        float dx, dy, d2;
        bool far;
        {
#pragma clang fp contract(off)
            dx = q.x - p.x; dy = q.y - p.y;
            d2 = dx * dx + dy * dy;
            far = q.w < d2 * theta2;
            if constexpr (REL) far = far & tree_far_rel(q.w, q.z, d2, g);
        }
        auto term = [&]() {
            if constexpr (RSQ == RSQ_QUAKE) {
#pragma clang fp contract(off)
                const float inv = quake_rsqrt(d2 + eps2);
                const float inv3 = inv * inv * inv;
                const float s = q.z * inv3;
                sx = sx + dx * s;
                sy = sy + dy * s;
            } else {
                const float inv = __builtin_amdgcn_rsqf(d2 + eps2);
                const float s = q.z * (inv * inv * inv);
                sx = __builtin_fmaf(dx, s, sx);
                sy = __builtin_fmaf(dy, s, sy);
            }
        };
        if (far) {
            if constexpr (QUAD) {
                const uint32_t next = nx[node];
                if (d2 > 0.f) {
                    if (next == node + 1u) term();
                    else tree_quad_term<RSQ>(q, qm[node], dx, dy, d2, eps2, sx, sy);
                }
                node = next > node ? next : node + 1u;
            } else {
                if (d2 > 0.f) term();
                const uint32_t next = nx[node];
                node = next > node ? next : node + 1u;       // (next > node always; the walk ends whatever the array holds)
            }
        } else {
            if constexpr (LEAVES) {
                if (q.z != 0.f && d2 > 0.f && nx[node] == node + 1u) term();
            }
            node = node + 1u;
        }
    }
    acc[b] = make_float2(sx, sy);
}

template <int RSQ, bool LEAVES, bool QUAD, bool REL>
__global__ __launch_bounds__(256)
void tree_walk(const float4 *__restrict__ nd, const uint32_t *__restrict__ nx, const uint32_t *__restrict__ val,
               const float2 *__restrict__ pos, uint32_t n, float eps2, float theta2, float2 *__restrict__ acc,
               const TreeStats *__restrict__ st, const float4 *__restrict__ qm, float alpha)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || st->fail) return;
    tree_walk_one<RSQ, LEAVES, QUAD, REL>(i, nd, nx, val, pos, eps2, theta2, acc, st, qm, alpha);
}

// The wave-uniform walk of NB_FLAG_TREE_LEAVES with NB_RSQRT_EXACT: one wave is one group, the 64 bodies at sorted positions
// [64 w, 64 w + 64) of `val`; a workgroup is four independent groups (no LDS, no barrier).  The node index is the same in every
// lane (formed through readfirstlane, so that the record and `next` are loaded once per wave); every lane evaluates its own
// acceptance test with the arithmetic of tree_walk, and a cell is accepted when ALL lanes of the group accept it (lanes that
// have left do not vote).  Every lane therefore opens at least what its own walk opens, there is no divergence in the loop,
// and every inserted body is still counted once per lane.
// A body's result depends on the positions in its group, so a group must not depend on the order of the bodies.  Two kinds
// of lane would make it: massless bodies (they sort last, by index alone) and a body on a position that first appears in an
// earlier group (which of the bodies sharing the position falls behind the boundary follows the index).  These lanes leave
// the group walk (tree_lane_alone) and tree_walk_alone gives each of them its own per-lane walk afterwards.
// QUAD: `all_far` and `leaf` are the same in every lane, so the moment record of an accepted branch is loaded inside that
// wave-uniform branch, by the readfirstlane node index: once per wave, through the scalar path, and for accepted branches only.
__device__ __forceinline__ bool tree_lane_alone(uint32_t i, const uint32_t *__restrict__ head, const uint64_t *__restrict__ uidx,
                                                const uint32_t *__restrict__ ufirst, const TreeStats *__restrict__ st)
{
    if (i >= st->massive) return true;
    if (head[i]) return false;
    return (ufirst[(uint32_t)uidx[i] - 1u] >> 6) != (i >> 6);        // (not a head: at least one key starts before i)
}

template <bool QUAD, bool REL>
__global__ __launch_bounds__(256)
void tree_walk_alone(const float4 *__restrict__ nd, const uint32_t *__restrict__ nx, const uint32_t *__restrict__ val,
                     const float2 *__restrict__ pos, uint32_t n, float eps2, float theta2, float2 *__restrict__ acc,
                     const TreeStats *__restrict__ st, const uint32_t *__restrict__ head, const uint64_t *__restrict__ uidx,
                     const uint32_t *__restrict__ ufirst, const float4 *__restrict__ qm, float alpha)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || st->fail || !tree_lane_alone(i, head, uidx, ufirst, st)) return;
    tree_walk_one<RSQ_EXACT, true, QUAD, REL>(i, nd, nx, val, pos, eps2, theta2, acc, st, qm, alpha);
}

template <bool QUAD, bool REL>
__global__ __launch_bounds__(256)
void tree_walk_group(const float4 *__restrict__ nd, const uint32_t *__restrict__ nx, const uint32_t *__restrict__ val,
                     const float2 *__restrict__ pos, uint32_t n, float eps2, float theta2, float2 *__restrict__ acc,
                     const TreeStats *__restrict__ st, const uint32_t *__restrict__ head, const uint64_t *__restrict__ uidx,
                     const uint32_t *__restrict__ ufirst, const float4 *__restrict__ qm, float alpha)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || st->fail || tree_lane_alone(i, head, uidx, ufirst, st)) return;
    const uint32_t b = val[i];
    const float2 p = pos[b];
    const uint32_t total = (uint32_t)st->nodes;
    float g = 0.f;
    if constexpr (REL) g = tree_rel_g(acc[b], alpha);
    float sx = 0.f, sy = 0.f;
    uint32_t node = 0;
    while (node < total) {
        node = (uint32_t)__builtin_amdgcn_readfirstlane((int)node);
        const float4 q = nd[node];
        const uint32_t next = nx[node];
        float dx, dy, d2;
        bool far;
        {
#pragma clang fp contract(off)
            dx = q.x - p.x; dy = q.y - p.y;
            d2 = dx * dx + dy * dy;
            far = q.w < d2 * theta2;
            if constexpr (REL) far = far & tree_far_rel(q.w, q.z, d2, g);
        }
        const bool all_far = __ballot(!far) == 0ull;
        const bool leaf = next == node + 1u;
        if constexpr (QUAD) {
            if (all_far && !leaf) {
                const float4 m = qm[node];
                if (d2 > 0.f) tree_quad_term<RSQ_EXACT>(q, m, dx, dy, d2, eps2, sx, sy);
            } else if (leaf && (all_far || q.z != 0.f)) {
                if (d2 > 0.f) tree_mono_term<RSQ_EXACT>(q.z, dx, dy, d2, eps2, sx, sy);
            }
        } else if (all_far || (leaf && q.z != 0.f)) {
            if (d2 > 0.f) tree_mono_term<RSQ_EXACT>(q.z, dx, dy, d2, eps2, sx, sy);
        }
        node = all_far && next > node ? next : node + 1u;    // (a leaf's next is node + 1)
    }
    acc[b] = make_float2(sx, sy);
}

// ---- potential energy -----------------------------------------------------------------------------------------------
// nb_energy of a NB_FLAG_TREE_ENERGY handle: K = sum m v^2 / 2 and U = 1/2 sum m_i phi_i, phi_i summed over exactly the nodes the
// wave-uniform force walk above takes for body i (the same float32 acceptance test without contraction, the same windows of 64
// bodies in key order, the same tree_lane_alone rule), whatever the handle's rsqrt mode: the potential has this one walk
// (tests/tree_energy_model.py is the CPU statement).  The node records, the moments and the positions are the float32 values
// the build wrote; from the displacement on everything is float64: with d = c - body, R^2 = d^2 + eps^2
//     a leaf, or an accepted cell without QUAD:   -m / R
//     an accepted branch with QUAD:               -(m / R + 1.5 (d^T M d) / R^5 - 0.5 tr(M) / R^3)
// (the potential whose gradient in d is the force term of tree_quad_term).  A term is taken where the force walk takes one:
// d^2 > 0 in float32.  The body's own leaf therefore gives nothing, and the bodies that share its position are added one by one
// from the sorted run of that position, -m_j / eps each (never "leaf mass - own mass": the leaf's float32 sum has lost the light
// ones), so that every unordered pair counts once, as in energy_partials; with eps = 0 they are skipped and the result is finite.
// A leaf that holds several bodies is the one node whose float32 mass is a rounded SUM, and at theta = 0 every other body sees it
// as it stands: one rounding of 2^-24 there is 4e-10 of U on ic_random_333, above the 1e-10 the energy is held to against the direct
// sum.  tree_leaf_residual therefore runs after the build: per point the float64 sum of its masses in the order of the run, and
// lo[leaf] = (float)(that sum - the record's mass) into a per-node array of NB_FLAG_TREE_ENERGY handles (+4 B per node).  A leaf's
// mass in a term is (double)record + (double)lo: the float64 sum to 2^-48, and the record itself for a leaf of one body (lo = 0).
// Accepted branches keep the float32 mass of their record.  Empty leaves (mass 0) have no entry and none is read.
// Massless bodies weigh nothing in K and U and do not walk.  Each kernel ends in the wave-shuffle and LDS reduction of
// energy_partials: one (K, U) partial per block, summed on the host in block order.
__device__ __forceinline__ double tree_potential_mono(float4 q, double m, float2 p, double eps2)
{
    const double dx = (double)q.x - (double)p.x, dy = (double)q.y - (double)p.y;
    const double r2 = __builtin_fma(dy, dy, __builtin_fma(dx, dx, eps2));
    return -m * rsqrt_f64(r2, 0.375);
}

// the mass of a node in a monopole term: a leaf with bodies adds its residual (above)
__device__ __forceinline__ double tree_potential_mass(float4 q, bool leaf, uint32_t node, const float *__restrict__ lo)
{
    return leaf && q.z != 0.f ? (double)q.z + (double)lo[node] : (double)q.z;
}

// lo[leaf of point u] for every point (one thread per point; the leaf is the last node the point wrote, tree_emit)
__global__ __launch_bounds__(256)
void tree_leaf_residual(const float4 *__restrict__ nd, const uint64_t *__restrict__ base, const uint32_t *__restrict__ ufirst,
                        const uint32_t *__restrict__ val, const float *__restrict__ mass, uint32_t n, const TreeStats *__restrict__ st,
                        float *__restrict__ lo)
{
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u >= n || st->fail || u >= st->points) return;
    const uint32_t leaf = (uint32_t)base[u + 1u] - 1u;
    if (leaf >= (uint32_t)st->nodes) return;               // (never: tree_emit wrote it; the bound keeps a disagreement inside the array)
    const uint32_t f = ufirst[u], e = u + 1u < st->points ? ufirst[u + 1u] : st->massive;
    double m = (double)mass[val[f]];
    for (uint32_t j = f + 1u; j < e; ++j) m += (double)mass[val[j]];
    lo[leaf] = (float)(m - (double)nd[leaf].z);
}

__device__ __forceinline__ double tree_potential_quad(float4 q, float4 m, float2 p, double eps2)
{
    const double dx = (double)q.x - (double)p.x, dy = (double)q.y - (double)p.y;
    const double r2 = __builtin_fma(dy, dy, __builtin_fma(dx, dx, eps2));
    const double inv = rsqrt_f64(r2, 0.375);
    const double inv2 = inv * inv, inv3 = inv2 * inv, inv5 = inv3 * inv2;
    const double xx = (double)m.x, xy = (double)m.y, yy = (double)m.z;
    const double rMr = dx * (xx * dx + xy * dy) + dy * (xy * dx + yy * dy);
    return -((double)q.z * inv + 1.5 * rMr * inv5 - 0.5 * (xx + yy) * inv3);
}

// sum of -m_j / eps over the OTHER bodies of the sorted run that holds position i (i < massive)
__device__ __forceinline__ double tree_potential_shared(uint32_t i, const uint32_t *__restrict__ val, const float *__restrict__ mass,
                                                        const uint32_t *__restrict__ head, const uint64_t *__restrict__ uidx,
                                                        const uint32_t *__restrict__ ufirst, const TreeStats *__restrict__ st, double eps2)
{
    if (!(eps2 > 0.0)) return 0.0;
    const uint32_t u = (uint32_t)uidx[i] + head[i] - 1u;           // (uidx counts the key starts before i)
    const uint32_t f = ufirst[u], e = u + 1u < st->points ? ufirst[u + 1u] : st->massive;
    const double inv = rsqrt_f64(eps2, 0.375);
    double s = 0.0;
    for (uint32_t j = f; j < e; ++j)
        if (j != i) s -= (double)mass[val[j]] * inv;
    return s;
}

__device__ __forceinline__ void tree_energy_reduce(double k, double u, double *__restrict__ ksum, double *__restrict__ usum)
{
    __shared__ double red[2][4];
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        k += __shfl_down(k, off, 64);
        u += __shfl_down(u, off, 64);
    }
    if ((t & 63u) == 0) { red[0][t >> 6] = k; red[1][t >> 6] = u; }
    __syncthreads();
    if (t == 0) {
        double ks = 0.0, us = 0.0;
        for (int w = 0; w < 4; ++w) { ks += red[0][w]; us += red[1][w]; }
        ksum[blockIdx.x] = ks;
        usum[blockIdx.x] = us;
    }
}

__device__ __forceinline__ void tree_energy_of(uint32_t b, double phi, const float2 *__restrict__ vel, const float *__restrict__ mass,
                                               double &k, double &u)
{
    const double m = (double)mass[b], vx = (double)vel[b].x, vy = (double)vel[b].y;
    k = 0.5 * m * (vx * vx + vy * vy);
    u = 0.5 * m * phi;
}

// EMIT (nb_potentials): the walker's phi is the result.  It is stored to usum[body] (usum is then an array of n doubles by body
// index, ksum is not used) and nothing is reduced; the massless bodies walk too, alone as in the force walk: no partner on their
// position is added (they are not in a sorted run), and a leaf exactly under them gives no term (d^2 = 0).
// the lanes tree_lane_alone takes out of their windows, massless ones excepted: the per-lane walk of tree_walk_one<.., true, QUAD>
template <bool QUAD, bool REL, bool EMIT = false>
__global__ __launch_bounds__(256)
void tree_potential_alone(const float4 *__restrict__ nd, const uint32_t *__restrict__ nx, const uint32_t *__restrict__ val,
                          const float2 *__restrict__ pos, const float2 *__restrict__ vel, const float *__restrict__ mass, uint32_t n,
                          double eps2, float theta2, const TreeStats *__restrict__ st, const uint32_t *__restrict__ head,
                          const uint64_t *__restrict__ uidx, const uint32_t *__restrict__ ufirst, double *__restrict__ ksum,
                          double *__restrict__ usum, const float *__restrict__ lo, const float4 *__restrict__ qm,
                          const float2 *__restrict__ aprev, float alpha)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    double k = 0.0, u = 0.0;
    if (i < n && !st->fail && (EMIT || i < st->massive) && tree_lane_alone(i, head, uidx, ufirst, st)) {
        const uint32_t b = val[i];
        const float2 p = pos[b];
        const uint32_t total = (uint32_t)st->nodes;
        float g = 0.f;
        if constexpr (REL) g = tree_rel_g(aprev[b], alpha);
        double phi = 0.0;
        uint32_t node = 0;
        while (node < total) {
            const float4 q = nd[node];
            const uint32_t next = nx[node];
            float d2;
            bool far;
            {
#pragma clang fp contract(off)
                const float dx = q.x - p.x, dy = q.y - p.y;
                d2 = dx * dx + dy * dy;
                far = q.w < d2 * theta2;
                if constexpr (REL) far = far & tree_far_rel(q.w, q.z, d2, g);
            }
            const bool leaf = next == node + 1u;
            if (far) {
                if (d2 > 0.f) {
                    if constexpr (QUAD) phi += leaf ? tree_potential_mono(q, tree_potential_mass(q, leaf, node, lo), p, eps2)
                                                    : tree_potential_quad(q, qm[node], p, eps2);
                    else phi += tree_potential_mono(q, tree_potential_mass(q, leaf, node, lo), p, eps2);
                }
                node = next > node ? next : node + 1u;
            } else {
                if (leaf && q.z != 0.f && d2 > 0.f) phi += tree_potential_mono(q, tree_potential_mass(q, leaf, node, lo), p, eps2);
                node = node + 1u;
            }
        }
        if (!EMIT || i < st->massive) phi += tree_potential_shared(i, val, mass, head, uidx, ufirst, st, eps2);
        if constexpr (EMIT) usum[b] = phi;
        else tree_energy_of(b, phi, vel, mass, k, u);
    }
    if constexpr (!EMIT) tree_energy_reduce(k, u, ksum, usum);
}

// nb_field on a NB_FLAG_TREE_ENERGY handle: one per-lane walker per caller-given POINT, in caller order.  A point walks exactly as a
// massless body at that position walks: the loop above (EMIT, the theta test) with its float64 terms for phi, and in the same loop the
// float32 terms of tree_walk_one<RSQ, true, QUAD> for acc, the running float32 sums widened on store.  A leaf exactly under the point
// gives no term (d^2 = 0).  The relative test is not applied: a point has no previous acceleration.  PHI / ACC pick the planes; the
// nodes visited and every operation of a plane are the same whichever are computed.
template <int RSQ, bool QUAD, bool PHI, bool ACC>
__global__ __launch_bounds__(256)
void tree_field_walk(const float4 *__restrict__ nd, const uint32_t *__restrict__ nx, const float2 *__restrict__ points, uint32_t npoints,
                     float eps2f, double eps2, float theta2, const TreeStats *__restrict__ st, const float *__restrict__ lo,
                     const float4 *__restrict__ qm, double *__restrict__ phi_out, double2 *__restrict__ acc_out)
{
    static_assert(PHI || ACC, "a plane must be asked for");
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npoints || st->fail) return;
    const float2 p = points[i];
    const uint32_t total = (uint32_t)st->nodes;
    double phi = 0.0;
    float sx = 0.f, sy = 0.f;
    uint32_t node = 0;
    while (node < total) {
        const float4 q = nd[node];
        const uint32_t next = nx[node];
        float dx, dy, d2;
        bool far;
        {
#pragma clang fp contract(off)
            dx = q.x - p.x; dy = q.y - p.y;
            d2 = dx * dx + dy * dy;
            far = q.w < d2 * theta2;
        }
        const bool leaf = next == node + 1u;
        auto mono = [&]() {
            if constexpr (ACC) tree_mono_term<RSQ>(q.z, dx, dy, d2, eps2f, sx, sy);
            if constexpr (PHI) phi += tree_potential_mono(q, tree_potential_mass(q, leaf, node, lo), p, eps2);
        };
        if (far) {
            if (d2 > 0.f) {
                if (QUAD && !leaf) {
                    const float4 m = qm[node];
                    if constexpr (ACC) tree_quad_term<RSQ>(q, m, dx, dy, d2, eps2f, sx, sy);
                    if constexpr (PHI) phi += tree_potential_quad(q, m, p, eps2);
                } else mono();
            }
            node = next > node ? next : node + 1u;
        } else {
            if (leaf && q.z != 0.f && d2 > 0.f) mono();
            node = node + 1u;
        }
    }
    if constexpr (PHI) phi_out[i] = phi;
    if constexpr (ACC) acc_out[i] = make_double2((double)sx, (double)sy);
}

// the windows: tree_walk_group's loop (node index through readfirstlane, one ballot, the moment record loaded inside the
// wave-uniform accepted-branch path).  The lanes that take no part stay out of the loop, so they neither vote nor lead, and
// join the block reduction with zeros.
template <bool QUAD, bool REL, bool EMIT = false>
__global__ __launch_bounds__(256)
void tree_potential_group(const float4 *__restrict__ nd, const uint32_t *__restrict__ nx, const uint32_t *__restrict__ val,
                          const float2 *__restrict__ pos, const float2 *__restrict__ vel, const float *__restrict__ mass, uint32_t n,
                          double eps2, float theta2, const TreeStats *__restrict__ st, const uint32_t *__restrict__ head,
                          const uint64_t *__restrict__ uidx, const uint32_t *__restrict__ ufirst, double *__restrict__ ksum,
                          double *__restrict__ usum, const float *__restrict__ lo, const float4 *__restrict__ qm,
                          const float2 *__restrict__ aprev, float alpha)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    double k = 0.0, u = 0.0;
    if (i < n && !st->fail && !tree_lane_alone(i, head, uidx, ufirst, st)) {
        const uint32_t b = val[i];
        const float2 p = pos[b];
        const uint32_t total = (uint32_t)st->nodes;
        float g = 0.f;
        if constexpr (REL) g = tree_rel_g(aprev[b], alpha);
        double phi = 0.0;
        uint32_t node = 0;
        while (node < total) {
            node = (uint32_t)__builtin_amdgcn_readfirstlane((int)node);
            const float4 q = nd[node];
            const uint32_t next = nx[node];
            float d2;
            bool far;
            {
#pragma clang fp contract(off)
                const float dx = q.x - p.x, dy = q.y - p.y;
                d2 = dx * dx + dy * dy;
                far = q.w < d2 * theta2;
                if constexpr (REL) far = far & tree_far_rel(q.w, q.z, d2, g);
            }
            const bool all_far = __ballot(!far) == 0ull;
            const bool leaf = next == node + 1u;
            if constexpr (QUAD) {
                if (all_far && !leaf) {
                    const float4 m = qm[node];
                    if (d2 > 0.f) phi += tree_potential_quad(q, m, p, eps2);
                } else if (leaf && (all_far || q.z != 0.f)) {
                    const double m = tree_potential_mass(q, leaf, node, lo);       // (wave-uniform: one scalar load)
                    if (d2 > 0.f) phi += tree_potential_mono(q, m, p, eps2);
                }
            } else if (all_far || (leaf && q.z != 0.f)) {
                const double m = tree_potential_mass(q, leaf, node, lo);
                if (d2 > 0.f) phi += tree_potential_mono(q, m, p, eps2);
            }
            node = all_far && next > node ? next : node + 1u;    // (a leaf's next is node + 1)
        }
        phi += tree_potential_shared(i, val, mass, head, uidx, ufirst, st, eps2);
        if constexpr (EMIT) usum[b] = phi;
        else tree_energy_of(b, phi, vel, mass, k, u);
    }
    if constexpr (!EMIT) tree_energy_reduce(k, u, ksum, usum);
}

// Kick and drift with acc[] as written by tree_walk.  A failed build integrates nothing: the positions are carried over.
template <typename L, bool STRICT>
__global__ __launch_bounds__(256)
void tree_integrate(const float2 *__restrict__ pos_cur, float2 *__restrict__ pos_next, float2 *__restrict__ vel, float2 *__restrict__ acc,
                    uint32_t n, float dt_kick, float dt_drift, int extras, int flags, const TreeStats *__restrict__ st)
{
    const uint32_t li = blockIdx.x * 256u + threadIdx.x;
    if (li >= n) return;
    if (st->fail) {
        if (flags & INTEG_DRIFT) pos_next[li] = pos_cur[li];
        return;
    }
    kick_drift_one<L, STRICT>(acc[li], li, pos_cur, pos_next, vel, acc, 0u, dt_kick, dt_drift, extras, flags);
}

// ---- export ---------------------------------------------------------------------------------------------------------
// nb_tree_nodes: the tree of the last build as the reference's `Node` records (Node.hpp:31-53, 128 bytes; nb_tree_node of
// include/nbody.h), in REFERENCE FORM: node 0 is the root, the branches are ranked r = 0, 1, ... in pre-order and the four children
// of branch r are nodes 1 + 4 r ... 1 + 4 r + 3 in quadrant order, the way Quadtree::insert allocates them (Quadtree.hpp:64-75).
// These kernels read nd / nx / dp, TreeRoot and TreeStats only (never the keys) and write arrays of their own: the build's arrays,
// and so the next force evaluation, do not know they ran.
//   tree_export_flags     flag[i] = 1 where pre-order node i is a branch; an exclusive scan gives rank[i]
//   tree_export_root      record 0 and idx[0] = 0 (idx: export index of a pre-order node)
//   tree_export_level     for level = 0 ... max_depth - 1 (the host knows max_depth after the synchronisation): every branch of depth
//                         `level` reads its own exported record (centre, size, next: written by the launch before), walks its four
//                         children through nx like tree_com, and writes their complete records and their idx.  Top-down, no atomics.
// A branch's four children are one contiguous 512-byte block: 8 lanes x one 16-byte store per record, 32 lanes per branch, two
// branches per wave and round, so the block leaves as whole 128-byte lines (one lane per record would issue eight strided stores).
// A wave looks at 64 pre-order nodes at a time, one per lane, and its two halves take the branches the ballot found, two by two.
// The child centre is Quad::into_quadrant's arithmetic (Quad.hpp:51-57), the recurrence of tree_keys; size * size of depth d has the
// bits of TreeRoot::s2[d] (halving is exact).  Padding bytes are written as zero.
__global__ __launch_bounds__(256)
void tree_export_flags(const uint8_t *__restrict__ dp, uint32_t total, uint32_t *__restrict__ flag)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) flag[i] = dp[i] >> 7;
}

__global__ __launch_bounds__(64)
void tree_export_root(const float4 *__restrict__ nd, const uint8_t *__restrict__ dp, const TreeRoot *__restrict__ root, uint32_t total,
                      uint4 *__restrict__ out, uint32_t *__restrict__ idx)
{
    const uint32_t part = threadIdx.x;
    if (part >= 8u || total == 0u) return;
    const float4 rec = nd[0];
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (part == 0u) { v.x = __float_as_uint(rec.x); v.y = __float_as_uint(rec.y); idx[0] = 0u; }
    else if (part == 1u) v.x = __float_as_uint(rec.z);
    else if (part == 2u) { v.x = __float_as_uint(root->cx); v.y = __float_as_uint(root->cy); }
    else if (part == 3u) v.x = __float_as_uint(root->size);
    else if (part == 4u) v.x = dp[0] >> 7;              // children: the first child of branch 0 is node 1; next stays 0 (Quadtree.hpp:32)
    out[part] = v;
}

__global__ __launch_bounds__(256)
void tree_export_level(const float4 *__restrict__ nd, const uint32_t *__restrict__ nx, const uint8_t *__restrict__ dp,
                       const uint64_t *__restrict__ rank, uint32_t level, uint32_t total, uint4 *__restrict__ out, uint32_t *__restrict__ idx)
{
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u, half = lane >> 5, q = (lane >> 3) & 3u, part = lane & 7u;
    for (uint32_t base = blockIdx.x * 256u + (threadIdx.x & ~63u); base < total; base += gridDim.x * 256u) {   // (wave-uniform)
        const uint32_t i = base + lane;
        uint64_t todo = __ballot(i < total && dp[i] == ((uint8_t)level | TREE_BRANCH));
        while (todo) {
            const uint64_t rest = todo & (todo - 1ull);                      // the lower half takes the lowest branch, the upper the next
            const uint64_t mine = half ? rest : todo;
            todo = rest & (rest - 1ull);
            if (!mine) continue;
            const uint32_t b = base + (uint32_t)__builtin_ctzll(mine);       // the branch, a pre-order index (b < total: the ballot)
            const uint32_t pe = idx[b];                                      // its export index and record
            if (pe >= total) continue;                                       // (never: written by the launch before; keeps reads inside)
            const uint4 pc = out[8u * pe + 2u], ps = out[8u * pe + 3u], pl = out[8u * pe + 4u];
            uint32_t c = b + 1u;                                             // child q, through nx like tree_com
            for (uint32_t k = 0; k < q && c < total; ++k) c = nx[c];
            const uint32_t e = 1u + 4u * (uint32_t)rank[b] + q;              // (1 + 4 branches = total <= capacity < 2^32)
            if (c >= total || e >= total) continue;                          // (never: a branch has four children, tree_emit)
            const float4 rec = nd[c];
            const bool branch = (dp[c] & TREE_BRANCH) != 0;
            const float size = __uint_as_float(ps.x) * 0.5f;                 // Quad.hpp:51-57
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (part == 0u) { v.x = __float_as_uint(rec.x); v.y = __float_as_uint(rec.y); idx[c] = e; }
            else if (part == 1u) v.x = __float_as_uint(rec.z);
            else if (part == 2u) {
                v.x = __float_as_uint(__uint_as_float(pc.x) + ((float)(q & 1u) - 0.5f) * size);
                v.y = __float_as_uint(__uint_as_float(pc.y) + ((float)(q >> 1) - 0.5f) * size);
            }
            else if (part == 3u) v.x = __float_as_uint(size);
            else if (part == 4u) {
                if (branch) v.x = 1u + 4u * (uint32_t)rank[c];               // children
                if (q < 3u) v.z = e + 1u; else { v.z = pl.z; v.w = pl.w; }   // next (Quadtree.hpp:71-75)
            }
            else if (part == 6u) v.x = level + 1u;                           // depth
            out[8u * e + part] = v;
        }
    }
}

} // namespace nbk
