// nb_field.hip.h — kernels of nb_field (host side: nb_field_host.hip.h): potential and acceleration at caller-given POINTS,
//     phi(p) = - sum_j m_j / sqrt(|d|^2 + eps^2)        acc(p) = sum_j m_j d / (|d|^2 + eps^2)^(3/2)        d = x_j - p   (G = 1)
// by the direct sweep over all n bodies.  (A NB_FLAG_TREE_ENERGY handle walks the tree: tree_field_walk, nb_tree.hip.h.)  These are
// nb_potential.hip.h's two kernels with the i-side taken from an array of points and the force term beside the potential term.
//
// A POINT IS NOT A BODY: no self term, no mask by index.  A point that lies on a body takes -m_j / eps into phi and nothing into
// acc (d = 0).  GUARD (handles whose eps^2 is 0 in the arithmetic of the sweep): a pair whose r^2 is exactly 0 adds nothing to
// either output: the select zeroes 1/r before any multiply, so there is no 0 x inf, for the padding record either.  Handles with
// eps^2 > 0 run the unguarded body: r^2 >= eps^2 there.
// WHAT A ROW DEPENDS ON: the bodies, eps, the precision and the point — not npoints, P, the grid or the other points.  Every
// kernel walks the j-tiles from j = 0 in steps of TJ and adds its partial sums in one fixed order.
// PHI / ACC pick the planes at compile time.  Every operation of a plane is written out (explicit fused multiply-adds, plain
// products that feed no addition), so the bits of one plane do not depend on whether the other is computed.
#pragma once
#include "nb_kernels.hip.h"

namespace nbk {

// ---------------------------------------------------------------------------
// field_tiled_f32 — fp32 handles, 2-D and 3-D: potential_tiled_f32's scheme.  j-records {x, y, m, m} / {x, y, z, m} through the
// double-buffered LDS tile of TJ, one broadcast ds_read_b128 per j, the next tile prefetched into registers; the TILED_F32_WS = 4
// waves own the same 64 i-lanes (2P points per lane, packed) and walk a quarter of each tile.  Per two pairs: packed sub, r^2 by
// packed fma onto eps^2, 2 v_rsq_f32, then
//     phi:  ph  = fma(m_j, inv, ph)                                           (potential_tiled_f32's unmasked body word for word)
//     acc:  inv2 = inv * inv    s = m_j * (inv2 * inv)    a_c = fma(d_c, s, a_c)
// ACCUMULATION: fp32 for one wave's share of one tile — 64 consecutive j, a run starts at every multiple of 64 from j = 0 — then one
// cvt and one fp64 add per output into the lane's fp64 sums; the four waves' fp64 sums are added through LDS in wave order,
// ((S_0 + S_1) + S_2) + S_3, one output plane at a time through the same 3 x P x 64 double2 of LDS.
// Padding past n: PAD_XY with mass 0 (r^2 stays finite, both terms are 0).  points: npoints rows of dims floats, packed.
// ---------------------------------------------------------------------------
template <typename L, int P, bool GUARD, bool PHI, bool ACC>
__global__ __launch_bounds__(BLOCK)
void field_tiled_f32(const typename L::vec *__restrict__ pos, const float *__restrict__ mass, const float *__restrict__ points,
                     double *__restrict__ phi, double *__restrict__ acc, uint32_t n, uint32_t npoints, float eps2)
{
    static_assert(PHI || ACC, "a plane must be asked for");
    constexpr int WS = TILED_F32_WS, UNROLL = 8;
    constexpr int D = L::dims3 ? 3 : 2;
    constexpr int NA = ACC ? D : 0, NO = (PHI ? 1 : 0) + NA;     // outputs per point; output 0 is phi where PHI
    constexpr uint32_t LANES_I = BLOCK / WS;          // distinct i-lanes in the workgroup
    constexpr uint32_t IT = LANES_I * 2 * P;          // points per workgroup
    constexpr uint32_t JW = TJ / WS;                  // j's of a tile walked by one wave: the length of an fp32 run
    constexpr uint32_t RED = (WS - 1) * P * LANES_I * sizeof(double2), TILES = 2 * TJ * sizeof(v4f);
    __shared__ __attribute__((aligned(16))) unsigned char smem[TILES > RED ? TILES : RED];
    v4f (*tile)[TJ] = reinterpret_cast<v4f (*)[TJ]>(smem);
    double2 *red = reinterpret_cast<double2 *>(smem);

    const uint32_t t = threadIdx.x;
    const uint32_t lane_i = t % LANES_I;              // which i-lane
    const uint32_t w = t / LANES_I;                   // which share of every tile
    const uint32_t l_first = blockIdx.x * IT;         // the workgroup's points: [l_first, l_first + IT)
    if (l_first >= npoints) return;

    v2f xi[P], yi[P], zi[P];                          // zi: 3-D only
    double s0[NO][P], s1[NO][P];                      // the fp64 sums of the lane's 2P points
    uint32_t li[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        li[p] = l_first + (uint32_t)p * (LANES_I * 2) + 2u * lane_i;
        const size_t l0 = min(li[p], npoints - 1), l1 = min(li[p] + 1, npoints - 1);
        xi[p] = (v2f){points[l0 * D], points[l1 * D]};
        yi[p] = (v2f){points[l0 * D + 1], points[l1 * D + 1]};
        if constexpr (L::dims3) zi[p] = (v2f){points[l0 * D + 2], points[l1 * D + 2]};
#pragma unroll
        for (int o = 0; o < NO; ++o) { s0[o][p] = 0.0; s1[o][p] = 0.0; }
    }
    const v2f e2 = {eps2, eps2};

    auto stage = [&](uint32_t j) -> v4f {
        if (j >= n) return L::dims3 ? (v4f){PAD_XY, PAD_XY, PAD_XY, 0.f} : (v4f){PAD_XY, PAD_XY, 0.f, 0.f};
        const auto pj = pos[j];
        if constexpr (L::dims3) return (v4f){pj.x, pj.y, pj.z, pj.w};
        else { const float mj = mass[j]; return (v4f){pj.x, pj.y, mj, mj}; }
    };

    const uint32_t ntiles = (n + TJ - 1) / TJ;
    tile[0][t] = stage(t);
    __syncthreads();
    for (uint32_t it = 0; it < ntiles; ++it) {
        // prefetch the next tile into registers while this one is consumed
        const v4f nxt = stage((it + 1) * TJ + t);
        const v4f *__restrict__ cur = tile[it & 1] + w * JW;
        v2f a[NO][P];                                  // one wave's share of this tile: the fp32 runs
#pragma unroll
        for (int o = 0; o < NO; ++o)
#pragma unroll
            for (int p = 0; p < P; ++p) a[o][p] = (v2f){0.f, 0.f};
#pragma unroll UNROLL
        for (int jj = 0; jj < (int)JW; ++jj) {
            const v4f q = cur[jj];                     // broadcast ds_read_b128
            const v2f xj = {q.x, q.x}, yj = {q.y, q.y}, zj = {q.z, q.z};
            const v2f mj = L::dims3 ? (v2f){q.w, q.w} : (v2f){q.z, q.w};
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const v2f dx = xj - xi[p], dy = yj - yi[p];
                v2f dz = {0.f, 0.f};
                v2f r2 = __builtin_elementwise_fma(dx, dx, e2);
                r2 = __builtin_elementwise_fma(dy, dy, r2);
                if constexpr (L::dims3) { dz = zj - zi[p]; r2 = __builtin_elementwise_fma(dz, dz, r2); }
                v2f inv = {__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
                if constexpr (GUARD) {
                    inv.x = r2.x == 0.f ? 0.f : inv.x;
                    inv.y = r2.y == 0.f ? 0.f : inv.y;
                }
                if constexpr (PHI) a[0][p] = __builtin_elementwise_fma(mj, inv, a[0][p]);
                if constexpr (ACC) {
                    constexpr int o = PHI ? 1 : 0;
                    const v2f inv2 = inv * inv;
                    const v2f s = mj * (inv2 * inv);
                    a[o][p] = __builtin_elementwise_fma(dx, s, a[o][p]);
                    a[o + 1][p] = __builtin_elementwise_fma(dy, s, a[o + 1][p]);
                    if constexpr (L::dims3) a[o + 2][p] = __builtin_elementwise_fma(dz, s, a[o + 2][p]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < NO; ++o)
#pragma unroll
            for (int p = 0; p < P; ++p) { s0[o][p] += (double)a[o][p].x; s1[o][p] += (double)a[o][p].y; }
        if (it + 1 < ntiles) tile[(it + 1) & 1][t] = nxt;
        __syncthreads();
    }

    // the WS sums of each point in wave order 0, 1, .., WS - 1, one output at a time (the tile buffers are free: the loop ended on a
    // barrier, and so does every pass)
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        if (w > 0) {
#pragma unroll
            for (int p = 0; p < P; ++p) red[((w - 1) * P + p) * LANES_I + lane_i] = make_double2(s0[o][p], s1[o][p]);
        }
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int p = 0; p < P; ++p) {
#pragma unroll
                for (int k = 0; k < WS - 1; ++k) {
                    const double2 r = red[(k * P + p) * LANES_I + lane_i];
                    s0[o][p] += r.x; s1[o][p] += r.y;
                }
                const size_t l = li[p];
                if (PHI && o == 0) {
                    if (l < npoints) phi[l] = 0.0 - s0[o][p];              // (0 - s: no body in reach gives +0)
                    if (l + 1 < npoints) phi[l + 1] = 0.0 - s1[o][p];
                } else {
                    const int c = o - (PHI ? 1 : 0);
                    if (l < npoints) acc[l * D + c] = s0[o][p];
                    if (l + 1 < npoints) acc[(l + 1) * D + c] = s1[o][p];
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// field_f64 — fp64 handles, 2-D and 3-D: potential_f64's tile loop over ALL j-tiles from 0, one point per thread (the float
// coordinates widened first), the terms added in j order with rsqrt_f64 (v_rsq_f64 + third-order step: 1.4e-16 relative):
//     phi:  u = fma(m_j, inv, u)            acc:  inv2 = inv * inv    s = m_j * (inv2 * inv)    a_c = fma(d_c, s, a_c)
// ---------------------------------------------------------------------------
template <typename L, bool GUARD, bool PHI, bool ACC>
__global__ __launch_bounds__(BLOCK)
void field_f64(const typename L::vec *__restrict__ pos, const double *__restrict__ mass, const float *__restrict__ points,
               double *__restrict__ phi, double *__restrict__ acc, uint32_t n, uint32_t npoints, double eps2)
{
    static_assert(PHI || ACC, "a plane must be asked for");
    struct alignas(16) JD2 { double x, y, m, pad; };
    struct alignas(16) JD3 { double x, y, z, m; };
    using JD = std::conditional_t<L::dims3, JD3, JD2>;
    constexpr int D = L::dims3 ? 3 : 2;
    __shared__ JD tile[TJ];
    const uint32_t t = threadIdx.x;
    const uint32_t li = blockIdx.x * BLOCK + t;
    const bool live = li < npoints;
    const size_t gi = live ? li : npoints - 1;
    const double xi = (double)points[gi * D], yi = (double)points[gi * D + 1];
    double zi = 0.0;
    if constexpr (L::dims3) zi = (double)points[gi * D + 2];
    const double k0375 = vgpr_const(0.375);
    double u = 0.0, ax = 0.0, ay = 0.0, az = 0.0;
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
            double dz = 0.0;
            double r2 = __builtin_fma(dy, dy, __builtin_fma(dx, dx, eps2));
            if constexpr (L::dims3) { dz = tile[jj].z - zi; r2 = __builtin_fma(dz, dz, r2); }
            double inv = rsqrt_f64(r2, k0375);
            if constexpr (GUARD) inv = r2 == 0.0 ? 0.0 : inv;
            const double mj = tile[jj].m;
            if constexpr (PHI) u = __builtin_fma(mj, inv, u);
            if constexpr (ACC) {
                const double inv2 = inv * inv;
                const double s = mj * (inv2 * inv);
                ax = __builtin_fma(dx, s, ax);
                ay = __builtin_fma(dy, s, ay);
                if constexpr (L::dims3) az = __builtin_fma(dz, s, az);
            }
        }
    }
    if (!live) return;
    if constexpr (PHI) phi[li] = 0.0 - u;
    if constexpr (ACC) {
        acc[(size_t)li * D] = ax;
        acc[(size_t)li * D + 1] = ay;
        if constexpr (L::dims3) acc[(size_t)li * D + 2] = az;
    }
}

}  // namespace nbk
