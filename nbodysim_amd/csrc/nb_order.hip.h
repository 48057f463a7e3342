// nb_order.hip.h — the body order of the symmetric direct path: the kernels (host side: nb_order_host.hip.h).
//
// The symmetric force kernel is VALU-bound and power-limited: the clock the part holds under its power cap sets the step time
// (DESIGN.md §4.1).  What an instruction costs in energy depends on its operands.  Bodies in the caller's index order are
// uncorrelated: the sign, exponent and mantissa of every displacement flip from lane to lane and from body to body.  Swept in
// the order of a space-filling curve, a tile and a chunk are compact patches and the displacement between them is nearly the
// same for every pair: the same instructions switch fewer bits and the part holds a higher clock (+3.5 % at 262 144 bodies,
// profiles/body_order_ceiling.log).
//
// The handle's arrays keep the caller's order.  The order lives beside them: perm[k] = the caller's index of the k-th body
// along the curve, and copies of the positions (masses, sigma) in that order, which the force kernel reads in place of the
// originals; the gather hands every summed row back to its body through perm.
//
// Key: 16 bits per axis of (x - lo) / (hi - lo) over the bounding box, a true division, the two interleaved (Morton) in the
// high word of a 64-bit key whose low word is the body index: keys are distinct, the order is the same run to run, ties go
// by index.  A scaling of all coordinates by a power of two scales x - lo and hi - lo exactly and leaves every key alone.
// A degenerate axis (hi == lo) and a coordinate that is not a number key as 0.
#pragma once
#include "nb_kernels.hip.h"

// Force evaluations from one sort to the next.  Bodies move a small fraction of a patch per step, so the order decays slowly; a sort
// of 262 144 keys (bounds, keys, rocPRIM's block and merge sort: 146 us) amortised over 16 evaluations is 9 us = 0.13 % of a step
// (DESIGN.md §4.1).  nb_body_order changes it per handle.
#ifndef NB_ORDER_EVERY
#define NB_ORDER_EVERY 16
#endif

namespace nbk {

constexpr uint32_t ORDER_PARTS = 256;      // partial boxes of order_bounds: one per workgroup, reduced again by every workgroup of order_keys

__device__ __forceinline__ float order_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double order_div(double a, double b) { return __ddiv_rn(a, b); }

// min / max of a workgroup's values through LDS; every thread returns the result.  Order-independent: the same bits whatever the launch.
template <typename real>
__device__ __forceinline__ void order_block_box(real &lx, real &ly, real &hx, real &hy)
{
    __shared__ real sh[4][BLOCK];
    const uint32_t t = threadIdx.x;
    sh[0][t] = lx; sh[1][t] = ly; sh[2][t] = hx; sh[3][t] = hy;
    __syncthreads();
    for (uint32_t s = BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) {
            sh[0][t] = fmin(sh[0][t], sh[0][t + s]); sh[1][t] = fmin(sh[1][t], sh[1][t + s]);
            sh[2][t] = fmax(sh[2][t], sh[2][t + s]); sh[3][t] = fmax(sh[3][t], sh[3][t + s]);
        }
        __syncthreads();
    }
    lx = sh[0][0]; ly = sh[1][0]; hx = sh[2][0]; hy = sh[3][0];
    __syncthreads();
}

// part[4 b .. 4 b + 3] = {lo.x, lo.y, hi.x, hi.y} of the bodies workgroup b strides over (an empty share leaves +inf / -inf)
template <typename real>
__global__ __launch_bounds__(BLOCK)
void order_bounds(const typename vec2_of<real>::type *__restrict__ pos, uint32_t n, real *__restrict__ part)
{
    real lx = INFINITY, ly = INFINITY, hx = -INFINITY, hy = -INFINITY;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const auto p = pos[i];
        lx = fmin(lx, p.x); ly = fmin(ly, p.y); hx = fmax(hx, p.x); hy = fmax(hy, p.y);
    }
    order_block_box(lx, ly, hx, hy);
    if (threadIdx.x == 0) { part[4u * blockIdx.x] = lx; part[4u * blockIdx.x + 1] = ly; part[4u * blockIdx.x + 2] = hx; part[4u * blockIdx.x + 3] = hy; }
}

// 16 bits -> the even bits of 32
__device__ __forceinline__ uint32_t order_spread(uint32_t v)
{
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

template <typename real>
__device__ __forceinline__ uint32_t order_axis(real x, real lo, real hi)
{
    if (!(hi > lo)) return 0u;
    const real t = order_div(x - lo, hi - lo) * (real)65536;      // in [0, 65536]; the product by a power of two is exact
    if (!(t >= (real)0)) return 0u;                               // not a number
    return t >= (real)65535 ? 65535u : (uint32_t)t;
}

// key[i] = Morton(x, y) << 32 | i, val[i] = i.  nparts <= ORDER_PARTS partial boxes are reduced by every workgroup.
template <typename real>
__global__ __launch_bounds__(BLOCK)
void order_keys(const typename vec2_of<real>::type *__restrict__ pos, uint32_t n, const real *__restrict__ part, uint32_t nparts,
                uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    static_assert(ORDER_PARTS <= (uint32_t)BLOCK, "one partial box per thread");
    real lx = INFINITY, ly = INFINITY, hx = -INFINITY, hy = -INFINITY;
    if (threadIdx.x < nparts) { lx = part[4u * threadIdx.x]; ly = part[4u * threadIdx.x + 1]; hx = part[4u * threadIdx.x + 2]; hy = part[4u * threadIdx.x + 3]; }
    order_block_box(lx, ly, hx, hy);
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const auto p = pos[i];
    const uint32_t m = order_spread(order_axis(p.x, lx, hx)) | (order_spread(order_axis(p.y, ly, hy)) << 1);
    key[i] = ((uint64_t)m << 32) | i;
    val[i] = i;
}

// dst[k] = src[perm[k]]
template <typename T>
__global__ __launch_bounds__(BLOCK)
void order_permute(const T *__restrict__ src, const uint32_t *__restrict__ perm, uint32_t n, T *__restrict__ dst)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k < n) dst[k] = src[perm[k]];
}

}  // namespace nbk
