// nb_potential.hip.h — kernels of nb_potentials (host side: nb_potential_host.hip.h): the potential of every owned body,
//     phi_i = - sum_{j != i} m_j / sqrt(|x_j - x_i|^2 + eps^2)        (G = 1, the softening of the force)
// by the direct sweep over all n bodies.  (A NB_FLAG_TREE_ENERGY handle takes phi from the walk: tree_potential_* <.., EMIT>,
// nb_tree.hip.h.)  Included last by nb_sim.hip.h: nothing here is seen by the kernels before it.
//
// WHAT phi_i DEPENDS ON: the bodies, eps, the precision and i — not the owned block and not the launch geometry.  Every kernel
// walks the j-tiles from j = 0 in steps of TJ and adds its partial sums in one fixed order, so a handle that owns
// [i_begin, i_begin + i_count) returns the bits of that slice of the unsharded result.
// THE SELF TERM is left out by index (j != i), never by distance and never by subtraction: with a 1e9 central mass it is larger
// than the sum, and with eps = 0 it is infinite.  Bodies that share i's position each add -m_j / eps (the pair convention of
// nb_energy); with eps = 0 such a body gets a value that is not finite.
#pragma once
#include "nb_kernels.hip.h"

namespace nbk {

// ---------------------------------------------------------------------------
// potential_tiled_f32 — fp32 handles, 2-D and 3-D (L = Layout<float, D3>): force_tiled_f32's one-sided scheme with the pair body
// cut down to the potential.  j-records {x, y, m, m} / {x, y, z, m} through a double-buffered LDS tile of TJ, one broadcast
// ds_read_b128 per j, the next tile prefetched into registers; the TILED_F32_WS = 4 waves of a workgroup own the same 64 i-lanes
// (2P particles per lane, packed) and walk a quarter of each tile.  Per two pairs: packed sub (x2, x3 in 3-D), packed fma
// (x2, x3), 2 v_rsq_f32, one packed fma m_j * inv into the accumulator: a subset of the force body (no inv^2, no s * d).
// ACCUMULATION: fp32 for one wave's share of one tile — JW = 64 terms, all of one sign, in j order — then one cvt and one fp64 add
// per particle into the lane's fp64 sum; the four waves' fp64 sums are added through LDS in wave order; the result is fp64.
//     phi_i = -(((S_0 + S_1) + S_2) + S_3),   S_w = sum over tiles T = 0, 1, ... of (double)(fp32 run of j in [T TJ + 64 w, T TJ + 64 w + 64))
// P and the grid change which lane holds a particle, not one operation of its sum.
// THE MASK: compare and select only in the j-tiles that overlap the workgroup's own i-range (a wave-uniform branch on the tile
// index; an i-range of IT = 128 P particles that starts anywhere overlaps at most ceil(IT / TJ) + 1 tiles); every other tile runs the
// unmasked body.  The select zeroes 1/r before the multiply: with eps = 0 the self pair's v_rsq_f32(0) is infinite.
// Padding past n: PAD_XY with mass 0, as in the force kernel (r^2 stays finite, the term is 0).
// ---------------------------------------------------------------------------
template <typename L, int P>
__global__ __launch_bounds__(BLOCK)
void potential_tiled_f32(const typename L::vec *__restrict__ pos, const float *__restrict__ mass, double *__restrict__ phi,
                         uint32_t n, uint32_t i_begin, uint32_t i_count, float eps2)
{
    constexpr int WS = TILED_F32_WS, UNROLL = 8;
    constexpr uint32_t LANES_I = BLOCK / WS;          // distinct i-lanes in the workgroup
    constexpr uint32_t IT = LANES_I * 2 * P;          // particles per workgroup
    constexpr uint32_t JW = TJ / WS;                  // j's of a tile walked by one wave: the length of an fp32 run
    constexpr uint32_t RED = (WS - 1) * P * LANES_I * sizeof(double2), TILES = 2 * TJ * sizeof(v4f);
    __shared__ __attribute__((aligned(16))) unsigned char smem[TILES > RED ? TILES : RED];
    v4f (*tile)[TJ] = reinterpret_cast<v4f (*)[TJ]>(smem);
    double2 *red = reinterpret_cast<double2 *>(smem);

    const uint32_t t = threadIdx.x;
    const uint32_t lane_i = t % LANES_I;              // which i-lane
    const uint32_t w = t / LANES_I;                   // which share of every tile
    const uint32_t l_first = blockIdx.x * IT;         // the workgroup's particles: [l_first, l_first + IT) of the owned block
    if (l_first >= i_count) return;
    // their GLOBAL indices [g_lo, g_hi): the j's among which the self terms lie
    const uint32_t g_lo = i_begin + l_first, g_hi = i_begin + min(l_first + IT, i_count);

    v2f xi[P], yi[P], zi[P];                          // zi: 3-D only
    double s0[P], s1[P];                              // the fp64 sums of the lane's 2P particles
    uint32_t li[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        li[p] = l_first + (uint32_t)p * (LANES_I * 2) + 2u * lane_i;
        const uint32_t l0 = min(li[p], i_count - 1), l1 = min(li[p] + 1, i_count - 1);
        const auto p0 = pos[i_begin + l0], p1 = pos[i_begin + l1];
        xi[p] = (v2f){p0.x, p1.x};
        yi[p] = (v2f){p0.y, p1.y};
        if constexpr (L::dims3) zi[p] = (v2f){p0.z, p1.z};
        s0[p] = 0.0; s1[p] = 0.0;
    }
    const v2f e2 = {eps2, eps2};

    auto stage = [&](uint32_t j) -> v4f {
        if (j >= n) return L::dims3 ? (v4f){PAD_XY, PAD_XY, PAD_XY, 0.f} : (v4f){PAD_XY, PAD_XY, 0.f, 0.f};
        const auto pj = pos[j];
        if constexpr (L::dims3) return (v4f){pj.x, pj.y, pj.z, pj.w};
        else { const float mj = mass[j]; return (v4f){pj.x, pj.y, mj, mj}; }
    };
    // one wave's share of one tile into the fp32 runs a[]; jg0 = the global index of cur[0]
    auto run = [&](auto masked, const v4f *__restrict__ cur, uint32_t jg0, v2f (&a)[P]) {
#pragma unroll UNROLL
        for (int jj = 0; jj < (int)JW; ++jj) {
            const v4f q = cur[jj];                 // broadcast ds_read_b128
            const v2f xj = {q.x, q.x}, yj = {q.y, q.y}, zj = {q.z, q.z};
            const v2f mj = L::dims3 ? (v2f){q.w, q.w} : (v2f){q.z, q.w};
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const v2f dx = xj - xi[p], dy = yj - yi[p];
                v2f r2 = __builtin_elementwise_fma(dx, dx, e2);
                r2 = __builtin_elementwise_fma(dy, dy, r2);
                if constexpr (L::dims3) { const v2f dz = zj - zi[p]; r2 = __builtin_elementwise_fma(dz, dz, r2); }
                v2f inv = {__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
                if constexpr (masked) {
                    const uint32_t jg = jg0 + (uint32_t)jj, gi = i_begin + li[p];
                    inv.x = jg == gi ? 0.f : inv.x;
                    inv.y = jg == gi + 1u ? 0.f : inv.y;
                }
                a[p] = __builtin_elementwise_fma(mj, inv, a[p]);
            }
        }
    };

    const uint32_t ntiles = (n + TJ - 1) / TJ;
    tile[0][t] = stage(t);
    __syncthreads();
    for (uint32_t it = 0; it < ntiles; ++it) {
        // prefetch the next tile into registers while this one is consumed
        const v4f nxt = stage((it + 1) * TJ + t);
        const v4f *__restrict__ cur = tile[it & 1] + w * JW;
        const uint32_t j0 = it * TJ;
        v2f a[P];
#pragma unroll
        for (int p = 0; p < P; ++p) a[p] = (v2f){0.f, 0.f};
        if (j0 < g_hi && j0 + TJ > g_lo) run(std::true_type{}, cur, j0 + w * JW, a);     // the tile holds some of our own particles
        else run(std::false_type{}, cur, 0u, a);
#pragma unroll
        for (int p = 0; p < P; ++p) { s0[p] += (double)a[p].x; s1[p] += (double)a[p].y; }
        if (it + 1 < ntiles) tile[(it + 1) & 1][t] = nxt;
        __syncthreads();
    }

    // the WS sums of each particle in wave order 0, 1, .., WS - 1 (the tile buffers are free: the loop ended on a barrier)
    if (w > 0) {
#pragma unroll
        for (int p = 0; p < P; ++p) red[((w - 1) * P + p) * LANES_I + lane_i] = make_double2(s0[p], s1[p]);
    }
    __syncthreads();
    if (w > 0) return;
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int k = 0; k < WS - 1; ++k) {
            const double2 r = red[(k * P + p) * LANES_I + lane_i];
            s0[p] += r.x; s1[p] += r.y;
        }
        if (li[p] < i_count) phi[li[p]] = 0.0 - s0[p];             // (0 - s: a body alone gets +0)
        if (li[p] + 1 < i_count) phi[li[p] + 1] = 0.0 - s1[p];
    }
}

// ---------------------------------------------------------------------------
// potential_f64 — fp64 handles, 2-D and 3-D: the tile loop of energy_partials over ALL j-tiles from 0, one particle per thread,
// the terms m_j * rsqrt_f64(r^2) added in j order (v_rsq_f64 + third-order step: 1.4e-16 relative); the self term is left out by a
// select on the index, so that eps = 0 stays finite for a body alone on its position.
// ---------------------------------------------------------------------------
template <typename L>
__global__ __launch_bounds__(BLOCK)
void potential_f64(const typename L::vec *__restrict__ pos, const double *__restrict__ mass, double *__restrict__ phi,
                   uint32_t n, uint32_t i_begin, uint32_t i_count, double eps2)
{
    struct alignas(16) JD2 { double x, y, m, pad; };
    struct alignas(16) JD3 { double x, y, z, m; };
    using JD = std::conditional_t<L::dims3, JD3, JD2>;
    __shared__ JD tile[TJ];
    const uint32_t t = threadIdx.x;
    const uint32_t li = blockIdx.x * BLOCK + t;
    const bool live = li < i_count;
    const uint32_t gi = i_begin + (live ? li : i_count - 1);
    const double xi = pos[gi].x, yi = pos[gi].y;
    double zi = 0.0;
    if constexpr (L::dims3) zi = pos[gi].z;
    const double k0375 = vgpr_const(0.375);
    double u = 0.0;
    for (uint32_t j0 = 0; j0 < n; j0 += TJ) {
        const uint32_t j = j0 + t;
        __syncthreads();
        if (j < n) {
            if constexpr (L::dims3) tile[t] = JD{pos[j].x, pos[j].y, pos[j].z, pos[j].w};
            else tile[t] = JD{pos[j].x, pos[j].y, mass[j], 0.0};
        } else tile[t] = JD{0.0, 0.0, 0.0, 0.0};
        __syncthreads();
        const uint32_t cnt = min((uint32_t)TJ, n - j0);
        for (uint32_t jj = 0; jj < cnt; ++jj) {
            const double dx = tile[jj].x - xi, dy = tile[jj].y - yi;
            double r2 = __builtin_fma(dy, dy, __builtin_fma(dx, dx, eps2));
            if constexpr (L::dims3) { const double dz = tile[jj].z - zi; r2 = __builtin_fma(dz, dz, r2); }
            const double s = __builtin_fma(tile[jj].m, rsqrt_f64(r2, k0375), u);
            u = j0 + jj != gi ? s : u;
        }
    }
    if (live) phi[li] = 0.0 - u;
}

}  // namespace nbk
