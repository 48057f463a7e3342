// nb_hermite.hip.h — kernels of the 4th-order Hermite integrator (NB_INTEGRATOR_HERMITE4; host side: nb_hermite_host.hip.h): the
// acceleration AND its time derivative, the jerk, of every body from one sweep over the pairs,
//     a_i = sum_j m_j d / R^3        j_i = sum_j m_j ( dv / R^3 - 3 (d.dv) d / R^5 )        d = x_j - x_i   dv = v_j - v_i   R^2 = d^2 + eps^2
// and the per-body predictor and corrector around it.
//
// THE SUM RUNS OVER ALL j, the body itself included: with d = 0 and dv = 0 every product of the term is 0, so the self pair adds
// exactly 0 to both sums while 1 / eps^3 is finite.  GUARD (handles whose eps^2 is 0 in the arithmetic of the sweep: needs_guard,
// nb_capi.hip): a pair whose r^2 is exactly 0 adds nothing to either sum: the select zeroes 1/r before any product.
// WHOLE-RANGE FORM (nb_field's): every workgroup walks the j-tiles from j = 0 in steps of TJ and leaves ONE row per body; there are
// no j-slices and no slabs.  A row depends on the bodies, eps and the precision only: not on P, the grid or the other rows.
// PADDING past n: the all-zero record (position 0, velocity 0, mass 0), not PAD_XY.  With mass 0 the factor s is exactly 0 and the
// pair adds 0 to both sums as long as c d stays finite; a record at 1e18 would put d.dv at 1e18 |v_i| and overflow it for
// |v_i| > 3e20, giving 0 x inf.  At the origin the padding pair is no larger than a pair with a real body there.
// Every operation is written out (explicit fused multiply-adds, plain products that feed no addition), so that the compiler has nothing
// to contract differently between variants.
#pragma once
#include "nb_kernels.hip.h"

namespace nbk {

// most bodies per lane (2P) of force_jerk_tiled_f32: what the register file holds without scratch at a useful occupancy
constexpr int hermite_pmax_f32(bool dims3) { return dims3 ? 2 : 4; }

// ---------------------------------------------------------------------------
// force_jerk_tiled_f32 — fp32 handles, 2-D and 3-D: force_tiled_f32's scheme in field_tiled_f32's whole-range form.  The j-record
// carries position, velocity and mass through two double-buffered LDS tiles of TJ, the next tile prefetched into registers:
//     2-D   {x, y, vx, vy} (one broadcast ds_read_b128)  +  {m} (one ds_read_b32)            20 B per j, 10 KiB
//     3-D   {x, y, z, m}   (one ds_read_b128)            +  {vx, vy, vz, 0} (one ds_read_b128)   32 B per j, 16 KiB
// (a 2-D record padded to two 128-bit words would read 12 B per j for nothing; the lone mass word costs one more LDS instruction, which
// the 18 packed operations per two pairs hide).  The TILED_F32_WS = 4 waves own the same 64 i-lanes (2P bodies per lane, packed) and walk
// a quarter of each tile.  Per two pairs, all packed, no divide:
//     d, dv (subs)   r^2 by fma onto eps^2   2 v_rsq_f32   inv2 = inv inv   s = (m inv) inv2   rv = fma(dy, dvy, dx dvx) [+ z]
//     c = (-3 rv) inv2   a_c = fma(s, d_c, a_c)   t_c = fma(c, d_c, dv_c)   j_c = fma(s, t_c, j_c)
// ACCUMULATION: fp32 for one wave's share of one tile — 64 consecutive j, a run starts at every multiple of 64 from j = 0 — then one
// cvt and one fp64 add per output into the lane's fp64 sums; the four waves' fp64 sums are added through LDS in wave order,
// ((S_0 + S_1) + S_2) + S_3, one output at a time through the same 3 x P x 64 double2 of LDS.
// Rows: acc_out and jerk_out, dims doubles per body, packed.
// ---------------------------------------------------------------------------
template <typename L, int P, bool GUARD>
__global__ __launch_bounds__(BLOCK)
void force_jerk_tiled_f32(const typename L::vec *__restrict__ pos, const float *__restrict__ mass, const typename L::vec *__restrict__ vel,
                          double *__restrict__ acc_out, double *__restrict__ jerk_out, uint32_t n, float eps2)
{
    constexpr int WS = TILED_F32_WS, UNROLL = 4;
    constexpr int D = L::dims3 ? 3 : 2, NO = 2 * D;             // outputs per body: a (D), then j (D)
    constexpr uint32_t LANES_I = BLOCK / WS;                     // distinct i-lanes in the workgroup
    constexpr uint32_t IT = LANES_I * 2 * P;                     // bodies per workgroup
    constexpr uint32_t JW = TJ / WS;                             // j's of a tile walked by one wave: the length of an fp32 run
    using rec1 = std::conditional_t<L::dims3, v4f, float>;       // the second word of a j-record
    constexpr uint32_t RED = (WS - 1) * P * LANES_I * sizeof(double2), TILES = 2 * TJ * (sizeof(v4f) + sizeof(rec1));
    __shared__ __attribute__((aligned(16))) unsigned char smem[TILES > RED ? TILES : RED];
    v4f (*tile0)[TJ] = reinterpret_cast<v4f (*)[TJ]>(smem);
    rec1 (*tile1)[TJ] = reinterpret_cast<rec1 (*)[TJ]>(smem + 2 * TJ * sizeof(v4f));
    double2 *red = reinterpret_cast<double2 *>(smem);

    const uint32_t t = threadIdx.x;
    const uint32_t lane_i = t % LANES_I;
    const uint32_t w = t / LANES_I;
    const uint32_t l_first = blockIdx.x * IT;                    // the workgroup's bodies: [l_first, l_first + IT)
    if (l_first >= n) return;

    v2f xi[P], yi[P], zi[P], ui[P], vi[P], wi[P];                // position and velocity; zi, wi: 3-D only
    double s0[NO][P], s1[NO][P];                                 // the fp64 sums of the lane's 2P bodies
    uint32_t li[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        li[p] = l_first + (uint32_t)p * (LANES_I * 2) + 2u * lane_i;
        const uint32_t l0 = min(li[p], n - 1), l1 = min(li[p] + 1, n - 1);
        const auto x0 = pos[l0], x1 = pos[l1], v0 = vel[l0], v1 = vel[l1];
        xi[p] = (v2f){x0.x, x1.x}; yi[p] = (v2f){x0.y, x1.y};
        ui[p] = (v2f){v0.x, v1.x}; vi[p] = (v2f){v0.y, v1.y};
        if constexpr (L::dims3) { zi[p] = (v2f){x0.z, x1.z}; wi[p] = (v2f){v0.z, v1.z}; }
#pragma unroll
        for (int o = 0; o < NO; ++o) { s0[o][p] = 0.0; s1[o][p] = 0.0; }
    }
    const v2f e2 = {eps2, eps2}, m3 = {-3.f, -3.f};

    auto stage = [&](uint32_t j, v4f &q0, rec1 &q1) {
        q0 = (v4f){0.f, 0.f, 0.f, 0.f};
        if constexpr (L::dims3) q1 = (v4f){0.f, 0.f, 0.f, 0.f}; else q1 = 0.f;
        if (j < n) {
            const auto pj = pos[j], vj = vel[j];
            if constexpr (L::dims3) { q0 = (v4f){pj.x, pj.y, pj.z, pj.w}; q1 = (v4f){vj.x, vj.y, vj.z, 0.f}; }
            else { q0 = (v4f){pj.x, pj.y, vj.x, vj.y}; q1 = mass[j]; }
        }
    };

    const uint32_t ntiles = (n + TJ - 1) / TJ;
    {
        v4f q0; rec1 q1;
        stage(t, q0, q1);
        tile0[0][t] = q0; tile1[0][t] = q1;
    }
    __syncthreads();
    for (uint32_t it = 0; it < ntiles; ++it) {
        // prefetch the next tile into registers while this one is consumed
        v4f n0; rec1 n1;
        stage((it + 1) * TJ + t, n0, n1);
        const v4f *__restrict__ cur0 = tile0[it & 1] + w * JW;
        const rec1 *__restrict__ cur1 = tile1[it & 1] + w * JW;
        v2f a[NO][P];                                            // one wave's share of this tile: the fp32 runs
#pragma unroll
        for (int o = 0; o < NO; ++o)
#pragma unroll
            for (int p = 0; p < P; ++p) a[o][p] = (v2f){0.f, 0.f};
#pragma unroll UNROLL
        for (int jj = 0; jj < (int)JW; ++jj) {
            const v4f q0 = cur0[jj];                             // broadcast ds_read_b128
            const rec1 q1 = cur1[jj];                            // broadcast ds_read_b32 (2-D) / ds_read_b128 (3-D)
            v2f xj, yj, zj, uj, vj, wj, mj;
            xj = (v2f){q0.x, q0.x}; yj = (v2f){q0.y, q0.y};
            if constexpr (L::dims3) {
                zj = (v2f){q0.z, q0.z}; mj = (v2f){q0.w, q0.w};
                uj = (v2f){q1.x, q1.x}; vj = (v2f){q1.y, q1.y}; wj = (v2f){q1.z, q1.z};
            } else {
                uj = (v2f){q0.z, q0.z}; vj = (v2f){q0.w, q0.w}; mj = (v2f){q1, q1};
            }
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const v2f dx = xj - xi[p], dy = yj - yi[p], du = uj - ui[p], dv = vj - vi[p];
                v2f dz = {0.f, 0.f}, dw = {0.f, 0.f};
                v2f r2 = __builtin_elementwise_fma(dx, dx, e2);
                r2 = __builtin_elementwise_fma(dy, dy, r2);
                v2f rv = __builtin_elementwise_fma(dy, dv, dx * du);
                if constexpr (L::dims3) {
                    dz = zj - zi[p]; dw = wj - wi[p];
                    r2 = __builtin_elementwise_fma(dz, dz, r2);
                    rv = __builtin_elementwise_fma(dz, dw, rv);
                }
                v2f inv = {__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
                if constexpr (GUARD) {
                    inv.x = r2.x == 0.f ? 0.f : inv.x;
                    inv.y = r2.y == 0.f ? 0.f : inv.y;
                }
                const v2f inv2 = inv * inv;
                const v2f s = (mj * inv) * inv2;
                const v2f c = (m3 * rv) * inv2;
                a[0][p] = __builtin_elementwise_fma(s, dx, a[0][p]);
                a[1][p] = __builtin_elementwise_fma(s, dy, a[1][p]);
                if constexpr (L::dims3) a[2][p] = __builtin_elementwise_fma(s, dz, a[2][p]);
                const v2f tx = __builtin_elementwise_fma(c, dx, du), ty = __builtin_elementwise_fma(c, dy, dv);
                a[D][p] = __builtin_elementwise_fma(s, tx, a[D][p]);
                a[D + 1][p] = __builtin_elementwise_fma(s, ty, a[D + 1][p]);
                if constexpr (L::dims3) {
                    const v2f tz = __builtin_elementwise_fma(c, dz, dw);
                    a[D + 2][p] = __builtin_elementwise_fma(s, tz, a[D + 2][p]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < NO; ++o)
#pragma unroll
            for (int p = 0; p < P; ++p) { s0[o][p] += (double)a[o][p].x; s1[o][p] += (double)a[o][p].y; }
        if (it + 1 < ntiles) { tile0[(it + 1) & 1][t] = n0; tile1[(it + 1) & 1][t] = n1; }
        __syncthreads();
    }

    // the WS sums of each body in wave order 0, 1, .., WS - 1, one output at a time (the tile buffers are free: the loop ended on a
    // barrier, and so does every pass)
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        if (w > 0) {
#pragma unroll
            for (int p = 0; p < P; ++p) red[((w - 1) * P + p) * LANES_I + lane_i] = make_double2(s0[o][p], s1[o][p]);
        }
        __syncthreads();
        if (w == 0) {
            double *__restrict__ out = o < D ? acc_out : jerk_out;
            const int c = o < D ? o : o - D;
#pragma unroll
            for (int p = 0; p < P; ++p) {
#pragma unroll
                for (int k = 0; k < WS - 1; ++k) {
                    const double2 r = red[(k * P + p) * LANES_I + lane_i];
                    s0[o][p] += r.x; s1[o][p] += r.y;
                }
                const size_t l = li[p];
                if (l < n) out[l * D + c] = s0[o][p];
                if (l + 1 < n) out[(l + 1) * D + c] = s1[o][p];
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// force_jerk_f64 — fp64 handles, 2-D and 3-D: force_tiled_f64's loop (a double-buffered LDS tile of TJ, the next one prefetched, P
// bodies per thread) over ALL j-tiles from 0, with rsqrt_f64 (v_rsq_f64 + third-order step: 1.4e-16 relative) and the terms above,
// added in j order.  j-records of 48 B {x, y, vx, vy, m, 0} in 2-D and 64 B {x, y, z, m, vx, vy, vz, 0} in 3-D: 24 / 32 KiB.
// ---------------------------------------------------------------------------
template <typename L, int P, bool GUARD>
__global__ __launch_bounds__(BLOCK)
void force_jerk_f64(const typename L::vec *__restrict__ pos, const double *__restrict__ mass, const typename L::vec *__restrict__ vel,
                    double *__restrict__ acc_out, double *__restrict__ jerk_out, uint32_t n, double eps2)
{
    struct alignas(16) JD2 { double x, y, u, v, m, pad; };
    struct alignas(16) JD3 { double x, y, z, m, u, v, w, pad; };
    using JD = std::conditional_t<L::dims3, JD3, JD2>;
    constexpr int D = L::dims3 ? 3 : 2, UNROLL = 2;
    constexpr uint32_t IT = BLOCK * P;
    __shared__ JD tile[2][TJ];
    const double k0375 = vgpr_const(0.375), km3 = vgpr_const(-3.0);
    const uint32_t t = threadIdx.x;
    const uint32_t l_first = blockIdx.x * IT;
    if (l_first >= n) return;

    double xi[P], yi[P], zi[P], ui[P], vi[P], wi[P];
    double ax[P], ay[P], az[P], jx[P], jy[P], jz[P];             // zi, wi, az, jz: 3-D only
    uint32_t li[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        li[p] = l_first + (uint32_t)p * BLOCK + t;
        const uint32_t l = min(li[p], n - 1);
        const auto x0 = pos[l], v0 = vel[l];
        xi[p] = x0.x; yi[p] = x0.y; ui[p] = v0.x; vi[p] = v0.y;
        ax[p] = ay[p] = jx[p] = jy[p] = 0.0;
        if constexpr (L::dims3) { zi[p] = x0.z; wi[p] = v0.z; az[p] = jz[p] = 0.0; }
    }
    // past n: the all-zero record.  The record is assigned field by field under `if`, as force_tiled_f64 does.
    auto stage = [&](uint32_t j) -> JD {
        JD q;
        q.x = q.y = q.u = q.v = q.m = q.pad = 0.0;
        if constexpr (L::dims3) q.z = q.w = 0.0;
        if (j < n) {
            const auto pj = pos[j], vj = vel[j];
            q.x = pj.x; q.y = pj.y; q.u = vj.x; q.v = vj.y;
            if constexpr (L::dims3) { q.z = pj.z; q.m = pj.w; q.w = vj.z; }
            else q.m = mass[j];
        }
        return q;
    };
    const uint32_t ntiles = (n + TJ - 1) / TJ;
    tile[0][t] = stage(t);
    __syncthreads();
    for (uint32_t it = 0; it < ntiles; ++it) {
        const JD nxt = stage((it + 1) * TJ + t);
        const JD *__restrict__ cur = tile[it & 1];
#pragma unroll UNROLL
        for (int jj = 0; jj < TJ; ++jj) {
            const JD q = cur[jj];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const double dx = q.x - xi[p], dy = q.y - yi[p], du = q.u - ui[p], dv = q.v - vi[p];
                double dz = 0.0, dw = 0.0;
                double r2 = __builtin_fma(dy, dy, __builtin_fma(dx, dx, eps2));
                double rv = __builtin_fma(dy, dv, dx * du);
                if constexpr (L::dims3) {
                    dz = q.z - zi[p]; dw = q.w - wi[p];
                    r2 = __builtin_fma(dz, dz, r2);
                    rv = __builtin_fma(dz, dw, rv);
                }
                double inv = rsqrt_f64(r2, k0375);
                if constexpr (GUARD) inv = r2 == 0.0 ? 0.0 : inv;
                const double inv2 = inv * inv;
                const double s = (q.m * inv) * inv2;
                const double c = (km3 * rv) * inv2;
                ax[p] = __builtin_fma(s, dx, ax[p]);
                ay[p] = __builtin_fma(s, dy, ay[p]);
                jx[p] = __builtin_fma(s, __builtin_fma(c, dx, du), jx[p]);
                jy[p] = __builtin_fma(s, __builtin_fma(c, dy, dv), jy[p]);
                if constexpr (L::dims3) {
                    az[p] = __builtin_fma(s, dz, az[p]);
                    jz[p] = __builtin_fma(s, __builtin_fma(c, dz, dw), jz[p]);
                }
            }
        }
        if (it + 1 < ntiles) tile[(it + 1) & 1][t] = nxt;
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        if (li[p] >= n) continue;
        const size_t o = (size_t)li[p] * D;
        acc_out[o] = ax[p]; acc_out[o + 1] = ay[p];
        jerk_out[o] = jx[p]; jerk_out[o + 1] = jy[p];
        if constexpr (L::dims3) { acc_out[o + 2] = az[p]; jerk_out[o + 2] = jz[p]; }
    }
}

// ---------------------------------------------------------------------------
// hermite_predict — x_p = x + (v h + (a0 h^2/2 + j0 h^3/6)) -> pos_next,  v_p = v + (a0 h + j0 h^2/2) -> vpred: where the pair kernel
// reads them.  The small terms are added to each other first.  In 3-D the mass travels in .w.
// ---------------------------------------------------------------------------
template <typename L>
__global__ __launch_bounds__(BLOCK)
void hermite_predict(const typename L::vec *__restrict__ pos_cur, typename L::vec *__restrict__ pos_next,
                     const typename L::vec *__restrict__ vel, typename L::vec *__restrict__ vpred,
                     const typename L::vec *__restrict__ acc, const typename L::vec *__restrict__ jerk, uint32_t n,
                     typename L::real h, typename L::real h2_2, typename L::real h3_6)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const typename L::vec x = pos_cur[i], v = vel[i], a = acc[i], j = jerk[i];
    typename L::vec xp = x, vp = v;
    xp.x = x.x + __builtin_fma(v.x, h, __builtin_fma(a.x, h2_2, j.x * h3_6));
    xp.y = x.y + __builtin_fma(v.y, h, __builtin_fma(a.y, h2_2, j.y * h3_6));
    vp.x = v.x + __builtin_fma(a.x, h, j.x * h2_2);
    vp.y = v.y + __builtin_fma(a.y, h, j.y * h2_2);
    if constexpr (L::dims3) {
        xp.z = x.z + __builtin_fma(v.z, h, __builtin_fma(a.z, h2_2, j.z * h3_6));
        vp.z = v.z + __builtin_fma(a.z, h, j.z * h2_2);
    }
    pos_next[i] = xp;
    vpred[i] = vp;
}

// ---------------------------------------------------------------------------
// hermite_correct — takes the evaluation's one row per body (a1, j1: fp64, rounded once to the handle's real), and with `advance`
//     v1 = v + ((a0 + a1) h/2 + (j0 - j1) h^2/12)        x1 = x + ((v + v1) h/2 + (a0 - a1) h^2/12)
// -> vel, pos_next; then the carried pair and acc[] <- (a1, j1).  advance = 0: only the last (the first evaluation after an upload).
// ---------------------------------------------------------------------------
template <typename L>
__global__ __launch_bounds__(BLOCK)
void hermite_correct(const typename L::vec *__restrict__ pos_cur, typename L::vec *__restrict__ pos_next,
                     typename L::vec *__restrict__ vel, typename L::vec *__restrict__ acc, typename L::vec *__restrict__ jerk,
                     const double *__restrict__ acc_row, const double *__restrict__ jerk_row, uint32_t n,
                     typename L::real h_2, typename L::real h2_12, int advance)
{
    using real = typename L::real;
    constexpr int D = L::dims3 ? 3 : 2;
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)i * D;
    typename L::vec a1 = acc[i], j1 = jerk[i];                    // (.w of the 3-D records stays what it was)
    const typename L::vec a0 = a1, j0 = j1;
    a1.x = (real)acc_row[o]; a1.y = (real)acc_row[o + 1];
    j1.x = (real)jerk_row[o]; j1.y = (real)jerk_row[o + 1];
    if constexpr (L::dims3) { a1.z = (real)acc_row[o + 2]; j1.z = (real)jerk_row[o + 2]; }
    if (advance) {
        const typename L::vec x = pos_cur[i], v = vel[i];
        typename L::vec x1 = x, v1 = v;
        v1.x = v.x + __builtin_fma(a0.x + a1.x, h_2, (j0.x - j1.x) * h2_12);
        v1.y = v.y + __builtin_fma(a0.y + a1.y, h_2, (j0.y - j1.y) * h2_12);
        x1.x = x.x + __builtin_fma(v.x + v1.x, h_2, (a0.x - a1.x) * h2_12);
        x1.y = x.y + __builtin_fma(v.y + v1.y, h_2, (a0.y - a1.y) * h2_12);
        if constexpr (L::dims3) {
            v1.z = v.z + __builtin_fma(a0.z + a1.z, h_2, (j0.z - j1.z) * h2_12);
            x1.z = x.z + __builtin_fma(v.z + v1.z, h_2, (a0.z - a1.z) * h2_12);
        }
        vel[i] = v1;
        pos_next[i] = x1;
    }
    acc[i] = a1;
    jerk[i] = j1;
}

}  // namespace nbk
