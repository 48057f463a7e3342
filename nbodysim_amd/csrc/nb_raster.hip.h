// nb_raster.hip.h — nb_raster's device side: the owned bodies binned into a width x height image (include/nbody.h has the contract).
//   raster_bin<L, COUNT, MASS, COMBINE>   one lane per body: the reference's worldToScreen (main.cpp:196-201) in fp32 without
//                                         contraction, the inside test BEFORE the conversion, then integer adds: +1 into count[pixel],
//                                         +units into units[pixel] (64-bit).  Integer sums: the planes do not depend on any order.
//   raster_finish                         units -> the float mass plane, (float)((double)U * (double)quantum)
// The hot path is contention (a zoomed-out Plummer core puts 10^5 bodies into a handful of pixels; one word takes about 10^2
// device-scope adds per microsecond), so with COMBINE adds that share a pixel meet on chip before they leave:
//   wave        up to RASTER_WAVE_ROUNDS times: the pixel of the first pending lane (ballot, readlane), the lanes that share it
//               (ballot); a group of two or more is summed across the wave and ONE lane carries count and units on.  A lane that
//               is alone with its pixel, or still pending after the rounds, carries its own.
//   workgroup   what the lanes carry goes into an open-addressing table in LDS (RASTER_SLOTS pixels: key by compare-and-swap,
//               count and units by LDS integer adds), which the workgroup keeps over all its bodies.  The table is emptied into
//               global memory, one add per plane and occupied slot, at the end, and between two batches of BLOCK bodies whenever
//               more than half of it is in use: the next batch then always finds room within RASTER_PROBES slots.  An add that
//               finds none (it cannot happen under that rule; the kernel does not rely on it) goes to global memory itself.
// COMBINE = false is the plainest form, one global add per body and plane, no LDS: the A/B of DESIGN.md (-DNB_RASTER_PLAIN builds it).
// Plain HIP atomics on LDS and global memory only; no floating-point atomics.
#pragma once
#include "nb_kernels.hip.h"

namespace nbk {

constexpr uint32_t RASTER_OUTSIDE = 0xffffffffu;    // no pixel (width * height <= 2^24); also the empty key of the LDS table
constexpr int RASTER_WAVE_ROUNDS = 4;
constexpr int RASTER_SLOTS_LOG2 = 11;
constexpr uint32_t RASTER_SLOTS = 1u << RASTER_SLOTS_LOG2;   // 2048 x (4 + 4 + 8) B = 32 KiB of LDS with a mass plane, 16 KiB without
constexpr int RASTER_PROBES = 16;
static_assert(RASTER_SLOTS % BLOCK == 0 && RASTER_SLOTS / 2 + BLOCK <= RASTER_SLOTS, "a batch fits the half the flush rule leaves free");

struct RasterView { uint32_t width, height; float cx, cy, scale, quantum; };

// pixel of (x, y), or RASTER_OUTSIDE: sx = (x - cx) * scale + width * 0.5f, one rounding per operation (width <= 16384: the
// conversion and the halving are exact); NaN and infinities fail the comparisons.  The pragma, not the __f*_rn intrinsics: those are
// plain operators to the compiler, which fuses __fadd_rn(__fmul_rn(a, b), c) into one fma: a body 10^-4 of a pixel from an edge then
// lands on the other side (tests/test_raster_gpu.py, the 6 M-body case: 3 bodies in 10^5 did).
__device__ __forceinline__ uint32_t raster_pixel(float x, float y, const RasterView &v)
{
#pragma clang fp contract(off)
    const float sx = (x - v.cx) * v.scale + (float)v.width * 0.5f;
    const float sy = (y - v.cy) * v.scale + (float)v.height * 0.5f;
    const bool inside = sx >= 0.0f && sx < (float)v.width && sy >= 0.0f && sy < (float)v.height;
    return inside ? (uint32_t)sy * v.width + (uint32_t)sx : RASTER_OUTSIDE;
}

// mass in whole quanta, ties to even, saturated at 2^32 - 1; nothing for m <= 0 and NaN
__device__ __forceinline__ uint32_t raster_units(float m, float quantum)
{
    if (!(m > 0.0f)) return 0u;
    const float r = __fdiv_rn(m, quantum);      // one correctly rounded division (no fast-math in this build)
    return r >= 4294967296.0f ? 4294967295u : (uint32_t)rintf(r);
}

template <bool COUNT, bool MASS>
__device__ __forceinline__ void raster_global_add(uint32_t *__restrict__ count, unsigned long long *__restrict__ units, uint32_t p, uint32_t c,
                                                  unsigned long long u)
{
    if constexpr (COUNT) atomicAdd(&count[p], c);
    if constexpr (MASS) { if (u) atomicAdd(&units[p], u); }
}

// returns true when the add took a slot that was empty (the caller keeps the table's fill)
template <bool COUNT, bool MASS>
__device__ __forceinline__ bool raster_table_add(uint32_t *keys, uint32_t *cnts, unsigned long long *sums, uint32_t *__restrict__ count,
                                                 unsigned long long *__restrict__ units, uint32_t p, uint32_t c, unsigned long long u)
{
    uint32_t h = (p * 2654435761u) >> (32 - RASTER_SLOTS_LOG2);
    for (int probe = 0; probe < RASTER_PROBES; ++probe) {
        const uint32_t old = atomicCAS(&keys[h], RASTER_OUTSIDE, p);
        if (old == RASTER_OUTSIDE || old == p) {
            if constexpr (COUNT) atomicAdd(&cnts[h], c);
            if constexpr (MASS) { if (u) atomicAdd(&sums[h], u); }
            return old == RASTER_OUTSIDE;
        }
        h = (h + 1u) & (RASTER_SLOTS - 1u);
    }
    raster_global_add<COUNT, MASS>(count, units, p, c, u);
    return false;
}

// every occupied slot: one global add per plane, and the slot is empty again (the caller puts barriers around it)
template <bool COUNT, bool MASS>
__device__ __forceinline__ void raster_table_flush(uint32_t *keys, uint32_t *cnts, unsigned long long *sums, uint32_t *__restrict__ count,
                                                   unsigned long long *__restrict__ units)
{
    for (uint32_t h = threadIdx.x; h < RASTER_SLOTS; h += BLOCK) {
        const uint32_t p = keys[h];
        if (p == RASTER_OUTSIDE) continue;
        unsigned long long u = 0;
        uint32_t c = 0;
        if constexpr (COUNT) { c = cnts[h]; cnts[h] = 0u; }
        if constexpr (MASS) { u = sums[h]; sums[h] = 0ull; }
        keys[h] = RASTER_OUTSIDE;
        raster_global_add<COUNT, MASS>(count, units, p, c, u);
    }
}

// bodies [i_begin, i_begin + i_count) of pos / mass; workgroup b takes the batches b, b + gridDim.x, ... of BLOCK bodies each
template <typename L, bool COUNT, bool MASS, bool COMBINE>
__global__ __launch_bounds__(BLOCK)
void raster_bin(const typename L::vec *__restrict__ pos, const typename L::real *__restrict__ mass, uint32_t i_begin, uint32_t i_count,
                RasterView view, uint32_t *__restrict__ count, unsigned long long *__restrict__ units)
{
    const uint32_t batches = (i_count + BLOCK - 1) / BLOCK;
    if constexpr (!COMBINE) {                                              // the plainest form: no LDS, no barrier
        for (uint32_t b = blockIdx.x; b < batches; b += gridDim.x) {
            const uint32_t li = b * BLOCK + threadIdx.x;
            if (li >= i_count) continue;
            const auto q = pos[i_begin + li];
            const uint32_t p = raster_pixel((float)q.x, (float)q.y, view);
            if (p == RASTER_OUTSIDE) continue;
            uint32_t u = 0u;
            if constexpr (MASS) u = raster_units((float)mass_at<L>(pos, mass, i_begin + li), view.quantum);
            raster_global_add<COUNT, MASS>(count, units, p, 1u, u);
        }
    } else {
        __shared__ uint32_t keys[RASTER_SLOTS];
        __shared__ uint32_t cnts[COUNT ? RASTER_SLOTS : 1];
        __shared__ unsigned long long sums[MASS ? RASTER_SLOTS : 1];
        __shared__ uint32_t used;
        for (uint32_t h = threadIdx.x; h < RASTER_SLOTS; h += BLOCK) {
            keys[h] = RASTER_OUTSIDE;
            if constexpr (COUNT) cnts[h] = 0u;
            if constexpr (MASS) sums[h] = 0ull;
        }
        if (threadIdx.x == 0) used = 0u;
        __syncthreads();
        for (uint32_t b = blockIdx.x; b < batches; b += gridDim.x) {       // workgroup-uniform: every thread meets every barrier
            const uint32_t li = b * BLOCK + threadIdx.x;
            uint32_t p = RASTER_OUTSIDE, u = 0u;
            if (li < i_count) {
                const auto q = pos[i_begin + li];
                p = raster_pixel((float)q.x, (float)q.y, view);
                if constexpr (MASS) {
                    if (p != RASTER_OUTSIDE) u = raster_units((float)mass_at<L>(pos, mass, i_begin + li), view.quantum);
                }
            }
            // wave: each round takes the pixel of the first pending lane and the lanes that share it
            const uint32_t lane = threadIdx.x & 63u;
            bool pending = p != RASTER_OUTSIDE, carry = false;
            uint32_t c = 1u;
            unsigned long long us = u;
            for (int round = 0; round < RASTER_WAVE_ROUNDS; ++round) {
                const unsigned long long todo = __ballot(pending);
                if (!todo) break;                                       // wave-uniform
                const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
                const uint32_t lp = (uint32_t)__builtin_amdgcn_readlane((int)p, (int)lead);
                const bool same = pending && p == lp;
                const unsigned long long grp = __ballot(same);
                const uint32_t members = (uint32_t)__popcll(grp);
                if (members >= 2u) {                                    // wave-uniform: every lane takes part in the sum
                    unsigned long long t = same ? (unsigned long long)u : 0ull;
                    if constexpr (MASS) {
                        for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d, 64);
                    }
                    if (lane == lead) { carry = true; c = members; us = t; }
                } else if (same) carry = true;
                pending = pending && !same;
            }
            bool fresh = false;
            if (pending || carry) fresh = raster_table_add<COUNT, MASS>(keys, cnts, sums, count, units, p, c, us);
            const uint32_t taken = (uint32_t)__popcll(__ballot(fresh));     // slots this wave filled: one add per wave, not one per lane
            if (lane == 0 && taken) atomicAdd(&used, taken);
            __syncthreads();
            const bool crowded = used > RASTER_SLOTS / 2;              // the same value in every thread: nothing writes `used` here
            __syncthreads();
            if (crowded) {
                raster_table_flush<COUNT, MASS>(keys, cnts, sums, count, units);
                if (threadIdx.x == 0) used = 0u;
                __syncthreads();
            }
        }
        raster_table_flush<COUNT, MASS>(keys, cnts, sums, count, units);
    }
}

// the mass plane from the unit sums
__global__ __launch_bounds__(BLOCK)
void raster_finish(const unsigned long long *__restrict__ units, float *__restrict__ out, uint32_t pixels, float quantum)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < pixels) out[i] = (float)((double)units[i] * (double)quantum);
}

}  // namespace nbk
