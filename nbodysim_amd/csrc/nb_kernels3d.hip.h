// nb_kernels3d.hip.h — the 3-D variant of the hot path (build extension).
//
// The reference is strictly 2-D (`Vec2`), but each `alignas(16) Vec2 {float x, y;}` carries 8 bytes
// of padding right after y (Nbodysim/headers/Vec2.hpp:17-20), so z fits at offset +8 of pos / vel /
// acc without moving x, y or changing sizeof(Body) = 64 (Body.hpp:6-13).  With nb_params.dims = 3
// the library reads and writes those slots and evaluates the same softened force with a third
// component (20 algorithmic flop per pair instead of 14).  There is no reference arithmetic to be
// bit-exact with here: parity is against the fp64 restatement only ("parity unpinned").
//
// Device layout: positions as real4 {x, y, z, m} (float4: one 16-byte load per particle; double4: two; the
// mass rides along), velocities / accelerations / slab rows as real4 {·, ·, ·, 0}.
// This file holds the 3-D symmetric force kernels and the gather of their slabs, in fp32 and fp64:
//   force_sym3_f32 / _f64    symmetric (Newton's third law) fast path, lane-rotated travelling particles
//   sym_gather3              sum of the symmetric slabs, one particle per thread
// The one-sided force kernels (force_tiled_f32 / _f64), integrate, kick / drift, pack / unpack, energy, momentum and
// sum_partials are shared with 2-D: the kernels of nb_kernels.hip.h keyed on Layout<real, true>.
#pragma once
#include "nb_kernels.hip.h"

namespace nbk {

// ---------------------------------------------------------------------------
// force_sym3_f32 — symmetric fast path in 3-D.  Same items / tiles / slab scheme as force_sym_f32
// (DESIGN.md §4.1): 8 stationary particles per lane as 4 packed pairs, one travelling particle per
// lane rotated with ds_bpermute_b32 (x, y, z [, m] and six accumulator halves: 9-10 per step).
// Body, both directions: 3 pk_add + 3 pk_fma + 2 rsq + 2 pk_mul + 6 pk_fma = 14 packed + 2 trans.
// ---------------------------------------------------------------------------
template <int RSQ, bool UM, bool DIAG>
__device__ __forceinline__
void sym3_chunks(const float4 *__restrict__ pos, float4 *__restrict__ slab_r_row, uint32_t n, uint32_t c0, uint32_t cnt,
                 const v2f (&xi)[SYM_P], const v2f (&yi)[SYM_P], const v2f (&zi)[SYM_P], const v2f (&mi)[SYM_P],
                 v2f (&ax)[SYM_P], v2f (&ay)[SYM_P], v2f (&az)[SYM_P], float eps2, float um_mass, float4 (*red)[4][64])
{
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const int addr = (int)(((lane + 1u) & 63u) * 4u);
    const v2f e2 = {eps2, eps2};
    float xq = PAD_XY, yq = PAD_XY, zq = PAD_XY, mq = 0.f;
    {
        const uint32_t j = c0 * SYM_CH + lane;
        if (j < n) { const float4 pj = pos[j]; xq = pj.x; yq = pj.y; zq = pj.z; mq = pj.w; }
    }
    for (uint32_t c = 0; c < cnt; ++c) {
        float xn = PAD_XY, yn = PAD_XY, zn = PAD_XY, mn = 0.f;
        {
            const uint32_t j = (c0 + c + 1) * SYM_CH + lane;
            if (c + 1 < cnt && j < n) { const float4 pj = pos[j]; xn = pj.x; yn = pj.y; zn = pj.z; mn = pj.w; }
        }
        v2f aqx = {0.f, 0.f}, aqy = {0.f, 0.f}, aqz = {0.f, 0.f};
#pragma unroll SYM_UNROLL
        for (int step = 0; step < 64; ++step) {
            const float xr = lane_rot(xq, addr), yr = lane_rot(yq, addr), zr = lane_rot(zq, addr);
            float mr = 0.f;
            if constexpr (!UM) mr = lane_rot(mq, addr);
            const v2f xj = {xq, xq}, yj = {yq, yq}, zj = {zq, zq};
#pragma unroll
            for (int p = 0; p < SYM_P; ++p) {
                const v2f dx = xj - xi[p], dy = yj - yi[p], dz = zj - zi[p];
                v2f r2 = __builtin_elementwise_fma(dx, dx, e2);
                r2 = __builtin_elementwise_fma(dy, dy, r2);
                r2 = __builtin_elementwise_fma(dz, dz, r2);
                v2f inv;
                if constexpr (RSQ == RSQ_EXACT) inv = (v2f){__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
                else inv = quake_rsqrt2(r2);
                const v2f inv3 = inv * (inv * inv);
                v2f si = inv3, sj = inv3;
                if constexpr (!UM) { si = (v2f){mq, mq} * inv3; sj = mi[p] * inv3; }
                ax[p] = __builtin_elementwise_fma(si, dx, ax[p]);
                ay[p] = __builtin_elementwise_fma(si, dy, ay[p]);
                az[p] = __builtin_elementwise_fma(si, dz, az[p]);
                if constexpr (!DIAG) {
                    aqx = __builtin_elementwise_fma(-sj, dx, aqx);
                    aqy = __builtin_elementwise_fma(-sj, dy, aqy);
                    aqz = __builtin_elementwise_fma(-sj, dz, aqz);
                }
            }
            xq = xr; yq = yr; zq = zr;
            if constexpr (!UM) mq = mr;
            if constexpr (!DIAG) {
                aqx.x = lane_rot(aqx.x, addr); aqx.y = lane_rot(aqx.y, addr);
                aqy.x = lane_rot(aqy.x, addr); aqy.y = lane_rot(aqy.y, addr);
                aqz.x = lane_rot(aqz.x, addr); aqz.y = lane_rot(aqz.y, addr);
            }
        }
        if constexpr (!DIAG) {
            float4 r = make_float4(aqx.x + aqx.y, aqy.x + aqy.y, aqz.x + aqz.y, 0.f);
            if constexpr (UM) { r.x *= um_mass; r.y *= um_mass; r.z *= um_mass; }
            float4 (*rb)[64] = red[c & 1u];
            rb[w][lane] = r;
            __syncthreads();
            if (w == 0) {
                const uint32_t j = (c0 + c) * SYM_CH + lane;
                float4 a = rb[0][lane];
#pragma unroll
                for (int k = 1; k < 4; ++k) { a.x += rb[k][lane].x; a.y += rb[k][lane].y; a.z += rb[k][lane].z; }
                if (j < n) slab_r_row[j] = a;
            }
        }
        xq = xn; yq = yn; zq = zn;
        if constexpr (!UM) mq = mn;
    }
}

// sym3_chunks2 — chunk PAIRS in 3-D (see sym_chunks2 in nb_kernels.hip.h): two travelling particles per lane in the two
// halves of the packed registers, the stationary particle broadcast; 12 ds_bpermute_b32 per 16 pairs instead of 9 per 8.
template <int RSQ, bool UM, bool DIAG>
__device__ __forceinline__
void sym3_chunks2(const float4 *__restrict__ pos, float4 *__restrict__ slab_r_row, uint32_t n, uint32_t c0, uint32_t cnt,
                  const v2f (&xi)[SYM_P], const v2f (&yi)[SYM_P], const v2f (&zi)[SYM_P], const v2f (&mi)[SYM_P],
                  v2f (&ax)[SYM_P], v2f (&ay)[SYM_P], v2f (&az)[SYM_P], float eps2, float um_mass, float4 (*red)[4][64])
{
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const int addr = (int)(((lane + 1u) & 63u) * 4u);
    const v2f e2 = {eps2, eps2};
    v2f bx[2 * SYM_P], by[2 * SYM_P], bz[2 * SYM_P];
#pragma unroll
    for (int k = 0; k < 2 * SYM_P; ++k) bx[k] = by[k] = bz[k] = (v2f){0.f, 0.f};
    auto fetch = [&](uint32_t c, v2f &x, v2f &y, v2f &z, v2f &m) {
        x = (v2f){PAD_XY, PAD_XY}; y = x; z = x; m = (v2f){0.f, 0.f};
        if (c < cnt) {
            const uint32_t j = (c0 + c) * SYM_CH + lane;
            if (j < n) { const float4 pj = pos[j]; x.x = pj.x; y.x = pj.y; z.x = pj.z; m.x = pj.w; }
        }
        if (c + 1 < cnt) {
            const uint32_t j = (c0 + c + 1) * SYM_CH + lane;
            if (j < n) { const float4 pj = pos[j]; x.y = pj.x; y.y = pj.y; z.y = pj.z; m.y = pj.w; }
        }
    };
    v2f xq, yq, zq, mq;
    fetch(0, xq, yq, zq, mq);
    for (uint32_t c = 0; c < cnt; c += 2) {
        v2f xn, yn, zn, mn;
        fetch(c + 2, xn, yn, zn, mn);
        v2f aqx = {0.f, 0.f}, aqy = {0.f, 0.f}, aqz = {0.f, 0.f};
#pragma unroll 2
        for (int step = 0; step < 64; ++step) {
            const v2f xr = {lane_rot(xq.x, addr), lane_rot(xq.y, addr)};
            const v2f yr = {lane_rot(yq.x, addr), lane_rot(yq.y, addr)};
            const v2f zr = {lane_rot(zq.x, addr), lane_rot(zq.y, addr)};
            v2f mr = {0.f, 0.f};
            if constexpr (!UM) mr = (v2f){lane_rot(mq.x, addr), lane_rot(mq.y, addr)};
#pragma unroll
            for (int p = 0; p < SYM_P; ++p) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float xs = h ? xi[p].y : xi[p].x, ys = h ? yi[p].y : yi[p].x, zs = h ? zi[p].y : zi[p].x;
                    const v2f dx = xq - (v2f){xs, xs}, dy = yq - (v2f){ys, ys}, dz = zq - (v2f){zs, zs};
                    v2f r2 = __builtin_elementwise_fma(dx, dx, e2);
                    r2 = __builtin_elementwise_fma(dy, dy, r2);
                    r2 = __builtin_elementwise_fma(dz, dz, r2);
                    v2f inv;
                    if constexpr (RSQ == RSQ_EXACT) inv = (v2f){__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
                    else inv = quake_rsqrt2(r2);
                    const v2f inv3 = inv * (inv * inv);
                    v2f si = inv3, sj = inv3;
                    if constexpr (!UM) { const float ms = h ? mi[p].y : mi[p].x; si = mq * inv3; sj = (v2f){ms, ms} * inv3; }
                    bx[2 * p + h] = __builtin_elementwise_fma(si, dx, bx[2 * p + h]);
                    by[2 * p + h] = __builtin_elementwise_fma(si, dy, by[2 * p + h]);
                    bz[2 * p + h] = __builtin_elementwise_fma(si, dz, bz[2 * p + h]);
                    if constexpr (!DIAG) {
                        aqx = __builtin_elementwise_fma(-sj, dx, aqx);
                        aqy = __builtin_elementwise_fma(-sj, dy, aqy);
                        aqz = __builtin_elementwise_fma(-sj, dz, aqz);
                    }
                }
            }
            xq = xr; yq = yr; zq = zr;
            if constexpr (!UM) mq = mr;
            if constexpr (!DIAG) {
                aqx = (v2f){lane_rot(aqx.x, addr), lane_rot(aqx.y, addr)};
                aqy = (v2f){lane_rot(aqy.x, addr), lane_rot(aqy.y, addr)};
                aqz = (v2f){lane_rot(aqz.x, addr), lane_rot(aqz.y, addr)};
            }
        }
        if constexpr (!DIAG) {
            float4 r0 = make_float4(aqx.x, aqy.x, aqz.x, 0.f), r1 = make_float4(aqx.y, aqy.y, aqz.y, 0.f);
            if constexpr (UM) { r0.x *= um_mass; r0.y *= um_mass; r0.z *= um_mass; r1.x *= um_mass; r1.y *= um_mass; r1.z *= um_mass; }
            float4 (*rb)[4][64] = red + 2u * ((c >> 1) & 1u);         // double buffered: [half q0 | half q1][4 waves][64 lanes]
            rb[0][w][lane] = r0;
            rb[1][w][lane] = r1;
            __syncthreads();
            if (w < 2 && c + w < cnt) {                                // wave 0 stores chunk c, wave 1 chunk c + 1
                const uint32_t j = (c0 + c + w) * SYM_CH + lane;
                float4 a = rb[w][0][lane];
#pragma unroll
                for (int k = 1; k < 4; ++k) { a.x += rb[w][k][lane].x; a.y += rb[w][k][lane].y; a.z += rb[w][k][lane].z; }
                if (j < n) slab_r_row[j] = a;
            }
        }
        xq = xn; yq = yn; zq = zn;
        if constexpr (!UM) mq = mn;
    }
#pragma unroll
    for (int p = 0; p < SYM_P; ++p) {
        ax[p] += (v2f){bx[2 * p].x + bx[2 * p].y, bx[2 * p + 1].x + bx[2 * p + 1].y};
        ay[p] += (v2f){by[2 * p].x + by[2 * p].y, by[2 * p + 1].x + by[2 * p + 1].y};
        az[p] += (v2f){bz[2 * p].x + bz[2 * p].y, bz[2 * p + 1].x + bz[2 * p + 1].y};
    }
}

template <int RSQ, bool UM, bool PAIRS = false>
__global__ __launch_bounds__(BLOCK)
void force_sym3_f32(const float4 *__restrict__ pos, const SymItem *__restrict__ items,
                    float4 *__restrict__ slab_s, float4 *__restrict__ slab_r, uint32_t n, float eps2, float um_mass,
                    uint32_t *ticket, uint32_t first_wave, uint32_t ticket_base)
{
    __shared__ float4 red[PAIRS ? 4 : 2][4][64];
    const SymItem it = items[sym_item_index(ticket, first_wave, ticket_base)];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    v2f xi[SYM_P], yi[SYM_P], zi[SYM_P], mi[SYM_P], ax[SYM_P], ay[SYM_P], az[SYM_P];
    uint32_t li[SYM_P];
#pragma unroll
    for (int p = 0; p < SYM_P; ++p) {
        li[p] = w * SYM_WT + (uint32_t)p * 128u + 2u * lane;
        const uint32_t g0 = it.tile * SYM_SB + li[p], g1 = g0 + 1;
        float4 p0 = make_float4(PAD_XY, PAD_XY, PAD_XY, 0.f), p1 = p0;
        if (g0 < n) p0 = pos[g0];
        if (g1 < n) p1 = pos[g1];
        xi[p] = (v2f){p0.x, p1.x}; yi[p] = (v2f){p0.y, p1.y}; zi[p] = (v2f){p0.z, p1.z}; mi[p] = (v2f){p0.w, p1.w};
        ax[p] = ay[p] = az[p] = (v2f){0.f, 0.f};
    }
    float4 *__restrict__ rrow = slab_r + it.r_base;
    if constexpr (PAIRS) {
        if (it.diag) sym3_chunks2<RSQ, UM, true>(pos, rrow, n, it.c0, it.cnt, xi, yi, zi, mi, ax, ay, az, eps2, um_mass, red);
        else         sym3_chunks2<RSQ, UM, false>(pos, rrow, n, it.c0, it.cnt, xi, yi, zi, mi, ax, ay, az, eps2, um_mass, red);
    } else {
        if (it.diag) sym3_chunks<RSQ, UM, true>(pos, rrow, n, it.c0, it.cnt, xi, yi, zi, mi, ax, ay, az, eps2, um_mass, red);
        else         sym3_chunks<RSQ, UM, false>(pos, rrow, n, it.c0, it.cnt, xi, yi, zi, mi, ax, ay, az, eps2, um_mass, red);
    }
    float4 *__restrict__ out = slab_s + (size_t)it.s_row * SYM_SB;
#pragma unroll
    for (int p = 0; p < SYM_P; ++p) {
        if constexpr (UM) { ax[p] *= um_mass; ay[p] *= um_mass; az[p] *= um_mass; }
        out[li[p]] = make_float4(ax[p].x, ay[p].x, az[p].x, 0.f);
        out[li[p] + 1] = make_float4(ax[p].y, ay[p].y, az[p].y, 0.f);
    }
}

// ---------------------------------------------------------------------------
// force_sym3_f64 — the symmetric scheme in 3-D double precision: same items, tiles and slabs as the other
// symmetric kernels; a lane holds SYM_P64 = 8 stationary particles as scalars, the travelling particle (x, y, z
// [, m]) and its accumulator rotate as pairs of 32-bit halves (12-14 ds_bpermute_b32 per step).
// Body, both directions: 3 add + 3 fma + v_rsq_f64 + 6 (cube correction) + 6 fma (+2 mul with individual masses).
// ---------------------------------------------------------------------------
template <bool UM, bool DIAG>
__device__ __forceinline__
void sym3_chunks_f64(const double4 *__restrict__ pos, double4 *__restrict__ slab_r_row, uint32_t n, uint32_t c0, uint32_t cnt,
                     const double (&xi)[SYM_P64], const double (&yi)[SYM_P64], const double (&zi)[SYM_P64], const double (&mi)[SYM_P64],
                     double (&ax)[SYM_P64], double (&ay)[SYM_P64], double (&az)[SYM_P64], double eps2, double um_mass,
                     double4 (*red)[4][64])
{
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const int addr = (int)(((lane + 1u) & 63u) * 4u);
    const double k15 = vgpr_const(1.5), k1875 = vgpr_const(1.875);
    double xq = PAD_XY64, yq = PAD_XY64, zq = PAD_XY64, mq = 0.0;
    {
        const uint32_t j = c0 * SYM_CH + lane;
        if (j < n) { const double4 pj = pos[j]; xq = pj.x; yq = pj.y; zq = pj.z; mq = pj.w; }
    }
    for (uint32_t c = 0; c < cnt; ++c) {
        double xn = PAD_XY64, yn = PAD_XY64, zn = PAD_XY64, mn = 0.0;
        {
            const uint32_t j = (c0 + c + 1) * SYM_CH + lane;
            if (c + 1 < cnt && j < n) { const double4 pj = pos[j]; xn = pj.x; yn = pj.y; zn = pj.z; mn = pj.w; }
        }
        double aqx = 0.0, aqy = 0.0, aqz = 0.0;
        for (int step = 0; step < 64; ++step) {
            const double xr = lane_rot64(xq, addr), yr = lane_rot64(yq, addr), zr = lane_rot64(zq, addr);
            double mr = 0.0;
            if constexpr (!UM) mr = lane_rot64(mq, addr);
#pragma unroll
            for (int p = 0; p < SYM_P64; ++p) {
                const double dx = xq - xi[p], dy = yq - yi[p], dz = zq - zi[p];
                const double r2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, __builtin_fma(dx, dx, eps2)));
                const double inv3 = rsqrt3_f64(r2, k15, k1875);
                double si = inv3, sj = inv3;
                if constexpr (!UM) { si = mq * inv3; sj = mi[p] * inv3; }
                ax[p] = __builtin_fma(si, dx, ax[p]);
                ay[p] = __builtin_fma(si, dy, ay[p]);
                az[p] = __builtin_fma(si, dz, az[p]);
                if constexpr (!DIAG) {
                    aqx = __builtin_fma(-sj, dx, aqx);
                    aqy = __builtin_fma(-sj, dy, aqy);
                    aqz = __builtin_fma(-sj, dz, aqz);
                }
            }
            xq = xr; yq = yr; zq = zr;
            if constexpr (!UM) mq = mr;
            if constexpr (!DIAG) { aqx = lane_rot64(aqx, addr); aqy = lane_rot64(aqy, addr); aqz = lane_rot64(aqz, addr); }
        }
        if constexpr (!DIAG) {
            double4 r = make_double4(aqx, aqy, aqz, 0.0);
            if constexpr (UM) { r.x *= um_mass; r.y *= um_mass; r.z *= um_mass; }
            double4 (*rb)[64] = red[c & 1u];
            rb[w][lane] = r;
            __syncthreads();
            if (w == 0) {
                const uint32_t j = (c0 + c) * SYM_CH + lane;
                double4 a = rb[0][lane];
#pragma unroll
                for (int k = 1; k < 4; ++k) { a.x += rb[k][lane].x; a.y += rb[k][lane].y; a.z += rb[k][lane].z; }
                if (j < n) slab_r_row[j] = a;
            }
        }
        xq = xn; yq = yn; zq = zn;
        if constexpr (!UM) mq = mn;
    }
}

template <bool UM>
__global__ __launch_bounds__(BLOCK)
void force_sym3_f64(const double4 *__restrict__ pos, const SymItem *__restrict__ items,
                    double4 *__restrict__ slab_s, double4 *__restrict__ slab_r, uint32_t n, double eps2, double um_mass,
                    uint32_t *ticket, uint32_t first_wave, uint32_t ticket_base)
{
    __shared__ double4 red[2][4][64];
    const SymItem it = items[sym_item_index(ticket, first_wave, ticket_base)];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    double xi[SYM_P64], yi[SYM_P64], zi[SYM_P64], mi[SYM_P64], ax[SYM_P64], ay[SYM_P64], az[SYM_P64];
    uint32_t li[SYM_P64];
#pragma unroll
    for (int p = 0; p < SYM_P64; ++p) {
        li[p] = w * SYM_WT + (uint32_t)p * 64u + lane;
        const uint32_t g = it.tile * SYM_SB + li[p];
        xi[p] = yi[p] = zi[p] = PAD_XY64; mi[p] = 0.0;
        if (g < n) { const double4 q = pos[g]; xi[p] = q.x; yi[p] = q.y; zi[p] = q.z; mi[p] = q.w; }
        ax[p] = ay[p] = az[p] = 0.0;
    }
    double4 *__restrict__ rrow = slab_r + it.r_base;
    if (it.diag) sym3_chunks_f64<UM, true>(pos, rrow, n, it.c0, it.cnt, xi, yi, zi, mi, ax, ay, az, eps2, um_mass, red);
    else         sym3_chunks_f64<UM, false>(pos, rrow, n, it.c0, it.cnt, xi, yi, zi, mi, ax, ay, az, eps2, um_mass, red);
    double4 *__restrict__ out = slab_s + (size_t)it.s_row * SYM_SB;
#pragma unroll
    for (int p = 0; p < SYM_P64; ++p) {
        if constexpr (UM) { ax[p] *= um_mass; ay[p] *= um_mass; az[p] *= um_mass; }
        out[li[p]] = make_double4(ax[p], ay[p], az[p], 0.0);
    }
}

// sym_gather3 — the 3-D twin of sym_gather (nb_kernels.hip.h): sum of the stationary rows of particle k's tile +
// the entries of its tile's coverage list, over particles [k0, k0 + kn); FUSE applies kick and drift (adding
// `base`, the reduce-scattered sum of a sharded rank, when given), otherwise the sum is stored to acc_sum[k].
template <typename real, bool FUSE>
__global__ __launch_bounds__(BLOCK)
void sym_gather3(const typename vec4_of<real>::type *__restrict__ slab_s, const typename vec4_of<real>::type *__restrict__ slab_r,
                 const uint32_t *__restrict__ row_lo, const uint32_t *__restrict__ row_hi,
                 const uint32_t *__restrict__ cov_begin, const SymCov *__restrict__ cov, uint32_t n, uint32_t k0, uint32_t kn,
                 typename vec4_of<real>::type *__restrict__ acc_sum, const typename vec4_of<real>::type *__restrict__ base,
                 const typename vec4_of<real>::type *__restrict__ pos_cur, typename vec4_of<real>::type *__restrict__ pos_next,
                 typename vec4_of<real>::type *__restrict__ vel, typename vec4_of<real>::type *__restrict__ acc,
                 real dt_kick, real dt_drift, int flags)
{
    typedef typename vec4_of<real>::type real4;
    __shared__ real4 part[GATHER_Q][GATHER_T];      // one particle per thread here: the elements are 16 / 32 bytes already
    const uint32_t p = threadIdx.x % GATHER_T, q = threadIdx.x / GATHER_T;
    const uint32_t li = blockIdx.x * GATHER_T + p, k = k0 + li;
    real4 a = make_real4<real>(0, 0, 0, 0);
    if (li < kn) {
        const uint32_t g = k / SYM_SB, loc = k % SYM_SB;
        const uint32_t r1 = row_hi[g];
#pragma unroll 4      // four independent loads in flight per thread; the adds keep their order
        for (uint32_t r = row_lo[g] + q; r < r1; r += GATHER_Q) {
            const real4 b = slab_s[(size_t)r * SYM_SB + loc];
            a.x += b.x; a.y += b.y; a.z += b.z;
        }
        // coverage entries four at a time, as in sym_gather_block (nb_kernels.hip.h): descriptors, then the partials they point at,
        // as independent batches; an entry that does not cover k reads element 0 of the slab and adds nothing; same order of adds
        const uint32_t c1 = cov_begin[g + 1];
        for (uint32_t i = cov_begin[g] + q; i < c1; i += 4u * GATHER_Q) {
            SymCov cv[4];
            bool in[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t idx = i + (uint32_t)u * GATHER_Q;
                in[u] = idx < c1;
                cv[u] = cov[in[u] ? idx : c1 - 1u];
            }
            real4 b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                in[u] = in[u] && k >= cv[u].lo && k < cv[u].hi;
                b[u] = slab_r[in[u] ? cv[u].base + (int64_t)k : (int64_t)0];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (in[u]) { a.x += b[u].x; a.y += b[u].y; a.z += b[u].z; }
        }
    }
    part[q][p] = a;
    __syncthreads();
    if (q == 0 && li < kn) {
        real4 s = part[0][p];
#pragma unroll
        for (int j = 1; j < GATHER_Q; ++j) { s.x += part[j][p].x; s.y += part[j][p].y; s.z += part[j][p].z; }
        if (base) { const real4 b = base[li]; s.x += b.x; s.y += b.y; s.z += b.z; }
        if constexpr (FUSE) kick_drift_one<Layout<real, true>, false>(s, li, pos_cur, pos_next, vel, acc, k0, dt_kick, dt_drift, 0, flags);
        else { s.w = 0; acc_sum[k] = s; }
    }
}

} // namespace nbk
