// nb_group_binding.hip.h — nb_group_binding's device side: the potential of every body due to the OTHER MEMBERS OF ITS OWN
// friends-of-friends group, its energy in the group's rest frame, and per group the bound count, the most bound member and the
// self-potential energy (include/nbody.h has the contract; tests/group_binding_model.py is its numpy statement).  The groups, the
// sort by (label, index), the rows and the mean velocities are nb_group_catalog's (nb_group_catalog.hip.h): in the sorted order a
// group is one SEGMENT of consecutive positions, and everything here works in that order.
//   binding_starts         a head writes its sorted position at start[label]
//   binding_gather<L>      position p: the j-record of its body (fp32 {x, y, m, m} / {x, y, z, m}; fp64 {x, y, z, m}) and its segment
//                          seg[p] = {start, length}, length 0 where the group is not kept; a body of such a group gets its NaNs here
//   group_potential<L, P>  THE HOT PATH, fp32 handles: the segmented n^2 sweep (below)
//   group_potential_f64<L> fp64 handles: one position per thread, potential_f64's loop over the segment
//   binding_records<L>     e = |v - vel|^2 / 2 + phi, both planes scattered back to body order, and catalog_pass' segmented scan of
//                          BindingVal: sum of w phi, count of e < 0, argmin of (e, body index); catalog_carry<BindingVal> behind it
//   binding_finish         one lane per record
// THE SWEEP.  The sorted positions are cut twice, both times by n alone: into TILES of T = 512 P positions, one per workgroup (each
// of the four waves owns 128 P consecutive positions, 2 P per lane, packed; the host launches P = 1), and into RUNS of 64 positions
// [64 k, 64 k + 64), four to a CHUNK of 256.  The j-range of a workgroup is the union [start of its first kept segment, end of its last), walked in chunks:
// the 256 threads stage one j-record each into LDS, the next chunk is prefetched into registers behind the barrier, and every wave
// walks the staged chunk run by run with one broadcast ds_read_b128 per j.  Staging and barriers are workgroup-uniform: EVERY THREAD
// MEETS EVERY BARRIER, and the chunk loop ends below n.  A wave classifies each run (wave-uniform values only):
//   skipped    the run lies outside [smallest start, largest end) of the wave's kept positions;
//   unmasked   all of the wave's positions belong to ONE kept segment, the run lies wholly inside it and outside the wave's own
//              positions: no compare, no select — the interior of a giant group runs potential_tiled_f32's body at its rate;
//   masked     anything else: the term is kept where j lies in the lane's segment and j != the lane's position.  The select takes
//              the accumulator before or after the fused multiply-add: a pair that does not count contributes NOTHING, whatever its
//              values (eps = 0 gives the self pair 1/r = infinity; a foreign body may hold a NaN).
// ARITHMETIC AND ORDER (nb_potentials' rules inside the segment): fp32 displacement, r^2 by fused multiply-adds onto eps^2, v_rsq_f32,
// m_j * inv added by FMA into an fp32 accumulator that starts at 0 with every run, so an fp32 run has at most 64 terms, in ascending j;
// behind each run one cvt and one fp64 add per position.  phi of position p = 0 - (fp64 sum over the runs k that meet its segment, in
// ascending k, of the fp32 sum over the j of run k inside the segment, j != p).  That order is a function of the sorted order and of
// the multiples of 64 alone: P, the tile and the chunk change which lane and which iteration hold a term, not one operation.
// THE WASTE is what the masked runs evaluate for positions of other segments.  A segment is met in full by the tiles inside it; only
// the tile that holds its first position and the tile that holds its last also hold lanes of foreign segments, at most T each: at
// most sum_g 2 T n_g wasted lane-pairs, and the skip by wave cuts it further.  All singletons: a wave walks the 2 P runs that cover
// its own 128 P positions.
// Indices: a position read or written is below n; a staged j is below n or padded (PAD_XY, mass 0: only a masked run can meet one,
// and masks it); start + length <= n by catalog_heads, and the loop bound is clamped to n all the same; LDS reads stay below 256.
#pragma once
#include "nb_group_catalog.hip.h"

namespace nbk {

constexpr uint32_t BINDING_RUN = 64, BINDING_CHUNK = BLOCK;
static_assert(BINDING_CHUNK % BINDING_RUN == 0 && BINDING_RUN == 64, "a chunk is whole runs, a run is one wave wide");

struct alignas(16) BindingRec64 { double x, y, z, m; };

// {sum of w phi, members with e < 0, the smallest e, the body index that holds it}: the last two are an argmin, kept EARLIER unless
// the later e is strictly smaller, so ties go to the smaller body index and a NaN never wins.  Counts and indices are exact in a double.
struct BindingVal {
    static constexpr int fields = 4;
    double v[4];
    __device__ __forceinline__ static BindingVal zero()
    {
        BindingVal z;
        z.v[0] = 0.0; z.v[1] = 0.0; z.v[2] = __builtin_huge_val(); z.v[3] = (double)0xffffffffu;     // NB_NO_NEIGHBOR
        return z;
    }
    // a before b in the sorted order
    __device__ __forceinline__ static BindingVal combine(const BindingVal &a, const BindingVal &b)
    {
        BindingVal r;
        r.v[0] = a.v[0] + b.v[0];
        r.v[1] = a.v[1] + b.v[1];
        const bool later = b.v[2] < a.v[2];
        r.v[2] = later ? b.v[2] : a.v[2];
        r.v[3] = later ? b.v[3] : a.v[3];
        return r;
    }
};
static_assert(BindingVal::fields <= CATALOG_FIELDS, "the catalogue's sums and slots hold a BindingVal");

__global__ __launch_bounds__(BLOCK)
void binding_starts(const uint64_t *__restrict__ skey, uint32_t n, uint32_t *__restrict__ start)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint64_t key = skey[p];
    if (p == 0u || skey[p - 1u] != key) start[(uint32_t)key] = p;         // only the head touches start[label]
}

template <typename L>
__global__ __launch_bounds__(BLOCK)
void binding_gather(const typename L::vec *__restrict__ pos, const typename L::real *__restrict__ mass, const uint64_t *__restrict__ skey,
                    const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ row_of, const uint32_t *__restrict__ start,
                    const nb_group *__restrict__ rec, uint32_t n, void *__restrict__ srec, uint2 *__restrict__ seg,
                    double *__restrict__ phi, double *__restrict__ e)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t label = (uint32_t)skey[p], i = sidx[p], row = row_of[label];
    const auto q = pos[i];
    const auto m = mass_at<L>(pos, mass, i);
    if constexpr (std::is_same_v<typename L::real, double>) {
        double z = 0.0;
        if constexpr (L::dims3) z = q.z;
        ((BindingRec64 *)srec)[p] = BindingRec64{q.x, q.y, z, m};
    } else {
        if constexpr (L::dims3) ((v4f *)srec)[p] = (v4f){q.x, q.y, q.z, m};
        else ((v4f *)srec)[p] = (v4f){q.x, q.y, m, m};
    }
    if (row == CATALOG_NO_ROW) {
        seg[p] = make_uint2(0u, 0u);
        phi[i] = e[i] = __builtin_nan("");
    } else seg[p] = make_uint2(start[label], rec[row].members);
}

__device__ __forceinline__ uint32_t binding_wave_min(uint32_t v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}
__device__ __forceinline__ uint32_t binding_wave_max(uint32_t v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}

// [lo, hi) of the workgroup's j-range from the waves' (empty: lo >= hi), clamped to n.  Every thread calls it (one barrier).
__device__ __forceinline__ void binding_range(uint32_t wmin, uint32_t wmax, uint32_t n, uint32_t *wlo, uint32_t *whi, uint32_t &lo, uint32_t &hi)
{
    constexpr uint32_t WAVES = BLOCK / 64;
    if ((threadIdx.x & 63u) == 0u) { wlo[threadIdx.x >> 6] = wmin; whi[threadIdx.x >> 6] = wmax; }
    __syncthreads();
    lo = wlo[0]; hi = whi[0];
#pragma unroll
    for (uint32_t u = 1; u < WAVES; ++u) { lo = min(lo, wlo[u]); hi = max(hi, whi[u]); }
    hi = min(hi, n);
}

// ---------------------------------------------------------------------------
// group_potential — fp32 handles, 2-D and 3-D (L = Layout<float, D3>); the head of the file has the scheme.
// ---------------------------------------------------------------------------
template <typename L, int P>
__global__ __launch_bounds__(BLOCK)
void group_potential(const v4f *__restrict__ srec, const uint2 *__restrict__ seg, double *__restrict__ sphi, uint32_t n, float eps2)
{
    constexpr int UNROLL = 8;
    constexpr uint32_t WAVES = BLOCK / 64, WP = 128u * P, T = WAVES * WP, CH = BINDING_CHUNK, RUN = BINDING_RUN;
    __shared__ __attribute__((aligned(16))) v4f tile[2][CH];
    __shared__ uint32_t wlo[WAVES], whi[WAVES];

    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint64_t wbase = (uint64_t)blockIdx.x * T + (uint64_t)wave * WP;    // the wave's positions: [wbase, wbase + WP)

    v2f xi[P], yi[P], zi[P];                          // zi: 3-D only
    double s0[P], s1[P];                              // the fp64 sums of the lane's 2P positions
    uint64_t pa[P];                                   // the position in .x; .y holds pa + 1
    uint32_t sa[P], la[P], sb[P], lb[P];              // start and length of the two segments; length 0: no term counts
    uint32_t wmin = 0xffffffffu, wmax = 0u;
    bool one = true;
#pragma unroll
    for (int q = 0; q < P; ++q) {
        pa[q] = wbase + (uint32_t)q * 128u + 2u * lane;
        v4f r0 = (v4f){0.f, 0.f, 0.f, 0.f}, r1 = r0;
        uint2 g0 = make_uint2(0u, 0u), g1 = g0;
        if (pa[q] < n) { r0 = srec[pa[q]]; g0 = seg[pa[q]]; }
        if (pa[q] + 1u < n) { r1 = srec[pa[q] + 1u]; g1 = seg[pa[q] + 1u]; }
        xi[q] = (v2f){r0.x, r1.x};
        yi[q] = (v2f){r0.y, r1.y};
        if constexpr (L::dims3) zi[q] = (v2f){r0.z, r1.z};
        sa[q] = g0.x; la[q] = g0.y; sb[q] = g1.x; lb[q] = g1.y;
        s0[q] = 0.0; s1[q] = 0.0;
        if (la[q]) { wmin = min(wmin, sa[q]); wmax = max(wmax, sa[q] + la[q]); }
        if (lb[q]) { wmin = min(wmin, sb[q]); wmax = max(wmax, sb[q] + lb[q]); }
    }
    // wave-uniform: the kept range of the wave, and whether all its positions are one kept segment [ws, we)
    wmin = binding_wave_min(wmin);
    wmax = binding_wave_max(wmax);
    const uint32_t ws = __builtin_amdgcn_readfirstlane(sa[0]), we = ws + __builtin_amdgcn_readfirstlane(la[0]);
#pragma unroll
    for (int q = 0; q < P; ++q) one = one && la[q] != 0u && lb[q] != 0u && sa[q] == ws && sb[q] == ws;
    const bool uniform = __all(one) != 0;
    uint32_t j_lo, j_hi;
    binding_range(wmin, wmax, n, wlo, whi, j_lo, j_hi);
    const v2f e2 = {eps2, eps2};

    auto stage = [&](uint64_t j) -> v4f {
        if (j >= n) return L::dims3 ? (v4f){PAD_XY, PAD_XY, PAD_XY, 0.f} : (v4f){PAD_XY, PAD_XY, 0.f, 0.f};
        return srec[j];
    };
    // one run into the fp32 sums a[]; jg0 = the sorted position of cur[0]
    auto run = [&](auto masked, const v4f *__restrict__ cur, uint32_t jg0, v2f (&a)[P]) {
#pragma unroll UNROLL
        for (int jj = 0; jj < (int)RUN; ++jj) {
            const v4f r = cur[jj];                 // broadcast ds_read_b128
            const v2f xj = {r.x, r.x}, yj = {r.y, r.y}, zj = {r.z, r.z};
            const v2f mj = L::dims3 ? (v2f){r.w, r.w} : (v2f){r.z, r.w};
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const v2f dx = xj - xi[q], dy = yj - yi[q];
                v2f r2 = __builtin_elementwise_fma(dx, dx, e2);
                r2 = __builtin_elementwise_fma(dy, dy, r2);
                if constexpr (L::dims3) { const v2f dz = zj - zi[q]; r2 = __builtin_elementwise_fma(dz, dz, r2); }
                const v2f inv = {__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
                const v2f sum = __builtin_elementwise_fma(mj, inv, a[q]);
                if constexpr (masked) {
                    const uint32_t jg = jg0 + (uint32_t)jj, me = (uint32_t)pa[q];       // (a position that counts is below n < 2^32)
                    a[q].x = jg - sa[q] < la[q] && jg != me ? sum.x : a[q].x;
                    a[q].y = jg - sb[q] < lb[q] && jg != me + 1u ? sum.y : a[q].y;
                } else a[q] = sum;
            }
        }
    };

    if (j_lo < j_hi) {                                // workgroup-uniform: no kept position, no chunk
        uint64_t c = j_lo & ~(uint64_t)(CH - 1u);
        tile[0][t] = stage(c + t);
        __syncthreads();
        for (uint32_t buf = 0; c < j_hi; c += CH, buf ^= 1u) {
            const bool more = c + CH < j_hi;
            v4f nxt = (v4f){0.f, 0.f, 0.f, 0.f};
            if (more) nxt = stage(c + CH + t);        // prefetch the next chunk into registers while this one is consumed
#pragma unroll 1
            for (uint32_t k = 0; k < CH / RUN; ++k) {
                const uint64_t r0 = c + k * RUN, r1 = r0 + RUN;
                if (r0 >= wmax || r1 <= wmin) continue;                                  // wave-uniform: none of the wave's lanes needs it
                v2f a[P];
#pragma unroll
                for (int q = 0; q < P; ++q) a[q] = (v2f){0.f, 0.f};
                const v4f *__restrict__ cur = tile[buf] + k * RUN;
                if (uniform && r0 >= ws && r1 <= we && (r1 <= wbase || r0 >= wbase + WP)) run(std::false_type{}, cur, 0u, a);
                else run(std::true_type{}, cur, (uint32_t)r0, a);
#pragma unroll
                for (int q = 0; q < P; ++q) { s0[q] += (double)a[q].x; s1[q] += (double)a[q].y; }
            }
            if (more) tile[buf ^ 1u][t] = nxt;
            __syncthreads();
        }
    }
#pragma unroll
    for (int q = 0; q < P; ++q) {
        if (la[q]) sphi[pa[q]] = 0.0 - s0[q];                                            // (0 - s: a body alone gets +0)
        if (lb[q]) sphi[pa[q] + 1u] = 0.0 - s1[q];
    }
}

// ---------------------------------------------------------------------------
// group_potential_f64 — fp64 handles, 2-D and 3-D: one sorted position per thread, the j-range of the workgroup's BLOCK positions in
// chunks of BLOCK through LDS, the terms m_j * rsqrt_f64(r^2) added in ascending j (segment order) under potential_f64's select.  A
// wave skips a chunk that none of its lanes needs; every thread meets both barriers of every chunk.
// ---------------------------------------------------------------------------
template <typename L>
__global__ __launch_bounds__(BLOCK)
void group_potential_f64(const BindingRec64 *__restrict__ srec, const uint2 *__restrict__ seg, double *__restrict__ sphi, uint32_t n, double eps2)
{
    constexpr uint32_t WAVES = BLOCK / 64;
    __shared__ BindingRec64 tile[BLOCK];
    __shared__ uint32_t wlo[WAVES], whi[WAVES];
    const uint32_t t = threadIdx.x;
    const uint64_t p = (uint64_t)blockIdx.x * BLOCK + t;
    BindingRec64 me = {0.0, 0.0, 0.0, 0.0};
    uint2 g = make_uint2(0u, 0u);
    if (p < n) { me = srec[p]; g = seg[p]; }
    const uint32_t wmin = binding_wave_min(g.y ? g.x : 0xffffffffu), wmax = binding_wave_max(g.y ? g.x + g.y : 0u);
    uint32_t j_lo, j_hi;
    binding_range(wmin, wmax, n, wlo, whi, j_lo, j_hi);
    const double k0375 = vgpr_const(0.375);
    double u = 0.0;
    for (uint64_t c = j_lo & ~(uint64_t)(BLOCK - 1); c < j_hi; c += BLOCK) {          // workgroup-uniform
        __syncthreads();
        tile[t] = c + t < n ? srec[c + t] : BindingRec64{0.0, 0.0, 0.0, 0.0};
        __syncthreads();
        if (c >= wmax || c + BLOCK <= wmin) continue;                                  // wave-uniform, behind the barriers
        const uint32_t cnt = (uint32_t)min((uint64_t)BLOCK, (uint64_t)n - c);
        for (uint32_t jj = 0; jj < cnt; ++jj) {
            const double dx = tile[jj].x - me.x, dy = tile[jj].y - me.y;
            double r2 = __builtin_fma(dy, dy, __builtin_fma(dx, dx, eps2));
            if constexpr (L::dims3) { const double dz = tile[jj].z - me.z; r2 = __builtin_fma(dz, dz, r2); }
            const double s = __builtin_fma(tile[jj].m, rsqrt_f64(r2, k0375), u);
            const uint32_t jg = (uint32_t)c + jj;
            u = jg - g.x < g.y && jg != (uint32_t)p ? s : u;
        }
    }
    if (g.y) sphi[p] = 0.0 - u;
}

// e and the planes in body order, and the records' scan.  v_i and w_i as the catalogue takes them (catalog_body).
template <typename L>
__global__ __launch_bounds__(BLOCK)
void binding_records(const typename L::vec *__restrict__ pos, const typename L::real *__restrict__ mass, const typename L::vec *__restrict__ vel,
                     const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ row_of, uint32_t n,
                     const nb_group *__restrict__ rec, const double *__restrict__ sphi, double *__restrict__ phi, double *__restrict__ e,
                     CatalogSums *__restrict__ sums, CatalogSlot *__restrict__ slot)
{
    constexpr int D = L::dims3 ? 3 : 2;
    catalog_pass<BindingVal>(skey, row_of, n, sums, slot, [&](uint32_t p, uint32_t row) {
        const uint32_t i = sidx[p];
        double x[3], v[3], w;
        catalog_body<L>(pos, mass, vel, i, x, v, w);
        const nb_group &g = rec[row];
        double dv2 = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) { const double dv = v[d] - g.vel[d]; dv2 += dv * dv; }
        const double f = sphi[p], en = 0.5 * dv2 + f;
        phi[i] = f;
        e[i] = en;
        BindingVal r;
        r.v[0] = w * f;
        r.v[1] = en < 0.0 ? 1.0 : 0.0;
        const bool ordered = en == en;                                    // a NaN takes no part in the argmin
        r.v[2] = ordered ? en : __builtin_huge_val();
        r.v[3] = ordered ? (double)i : (double)0xffffffffu;
        return r;
    });
}

__global__ __launch_bounds__(BLOCK)
void binding_finish(const CatalogSums *__restrict__ sums, const nb_group *__restrict__ rec, uint32_t count, nb_group_energy *__restrict__ out)
{
    const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
    if (row >= count) return;
    const CatalogSums &s = sums[row];
    nb_group_energy g;
    g.label = rec[row].label;
    g.members = rec[row].members;
    g.bound = (uint32_t)s.v[1];
    g.most_bound = s.v[2] < __builtin_huge_val() ? (uint32_t)s.v[3] : 0xffffffffu;       // no member's e compares: NB_NO_NEIGHBOR, +inf
    g.e_min = s.v[2];
    g.potential = 0.5 * s.v[0];
    out[row] = g;
}

}  // namespace nbk
