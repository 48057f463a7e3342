// nb_profiles.hip.h — nb_radial_profiles' device side: for every one of ncenters POINTS, per spherical (dims = 3) or circular shell
// about it, the count of bodies and the fp64 sums of mass and velocity moments (include/nbody.h has the contract;
// tests/radial_profiles_model.py is its numpy statement).
//   (cells)                neighbors_keys, the sort and neighbors_gather of nb_neighbors.hip.h at radius edges[nbins], by the host helper
//                          the grid queries share
//   profiles_ranges        one WAVE per centre: the centre's cell, the three key ranges of the 3 x 3 cells round it (64-ary searches on
//                          the sorted keys, four probes deep at 16 M bodies), the number of candidates T and of PIECES, ceil(T / P)
//   (scans)                nb_tree_scan of the piece counts (first[]) and of the piece counts of the centres that are split (prow[])
//   profiles_sweep<L, NS>  the hot path: ONE WAVE PER PIECE of P = PROFILES_PIECE candidates, a workgroup being one wave.  NS x 8 is
//                          the shell capacity (8, 16, 32, 64), chosen on the host like K in nb_neighbors
//   profiles_combine       adds the partial rows of the centres that were cut into several pieces, in a fixed order
// THE PREDICATE AND THE CELLS are nb_neighbors' (neighbors_d2; cell size edges[nbins] x (1 + 2^-16); cell_coord for the centre as
// for a body, the same code path as neighbors_keys).  A centre is a float position like any body's, so the proof in
// nb_neighbors.hip.h that a pair with d2 < r2max is never two cells apart covers centre and body.  It covers the 3-D distance too:
// fp32 addition of non-negative numbers is monotone, so d2 = fl(fl(dx^2 + dy^2) + dz^2) >= fl(dx^2 + dy^2); a body inside r2max in
// 3-D is inside it in projection, and the projected cells hold a superset.  A candidate whose projected d2 is not below r2max is
// dropped before its record (z, v, m) is read.
// THE PIECE MAP.  A centre's candidates are the concatenation of its three ranges, row -1 first, each in ascending sorted position:
// the virtual offsets 0 .. T - 1.  Piece k of the centre holds the offsets [k P, min(T, (k + 1) P)).  first[] is the exclusive scan of
// the piece counts over the centres (ncenters + 1 entries, the last one the total); wave `piece` finds its centre as the last c with
// first[c] <= piece by one more 64-ary search, and k = piece - first[c].  So ONE centre that covers n bodies is n / P waves spread
// over the chip by the dispatcher, and 65 536 centres with a few dozen candidates each are 65 536 single waves; a centre that has no
// candidate has no wave.  A centre that is ONE piece writes its shells into `out` directly.  Only a centre with K > 1 pieces writes
// partial rows, at row prow[c] + k of `partial` (prow[]: the exclusive scan of K where K > 1, else 0): the scratch is sized by the
// pieces of split centres, never by ncenters x nbins.
// THE ORDER OF EVERY SUM (a function of the bodies, the centres and the edges alone):
//   inside a piece     the wave takes its candidates 64 at a time in ascending offset.  The lanes whose candidate falls in a shell
//                      stage (shell, eight values) in LDS, compacted in ascending offset (ballot and prefix count); the values are
//                      {1, w, w r, w r^2, w v_r, w v_r^2, w |u|^2, w l_z}.  Lane (g = lane / 8, f = lane % 8) owns field f of the
//                      shells g, g + 8, ...; it walks the staged entries in order and adds the ones of its shells to accumulators
//                      that start at +0: acc += (shell == mine ? value : +0).  Adding +0 to a sum that started at +0 never changes
//                      it, so a shell's sum is the left-to-right fp64 sum of its terms in ascending offset.  Reading one LDS
//                      address from many lanes is a broadcast: no bank conflict.  The count is summed as a double (at most P, exact)
//   across pieces      thread (s = 0 .. 31, f) of a workgroup adds the rows k = s, s + 32, s + 64, ... of its (centre, shell) in
//                      ascending k starting from the first, and the 32 sums are added by the tree x[s] += x[s + h], h = 16, 8, 4, 2,
//                      1.  The counts are added as integers.
// There is no atomic on a double and no float atomic anywhere; nothing depends on the order of arrival.
// Indices: a sorted position read is below n (the ranges lie in [0, n]); a centre index is below ncenters (first[ncenters] = total
// > piece); a partial row is below the total of prow[]; `out` holds ncenters x nbins records and a shell index is below nbins.  Every
// thread of a workgroup meets every barrier: the loops of the sweep have wave-uniform bounds (a workgroup is one wave), and those
// of the combine kernel depend on the (centre, shell) item alone.
#pragma once
#include "nb_group_catalog.hip.h"

namespace nbk {

constexpr uint32_t PROFILES_PIECE = 1024;             // candidates per wave
constexpr uint32_t PROFILES_SUBS = 32;                // partial sums per (centre, shell) in the combine kernel: BLOCK / 8
static_assert(PROFILES_PIECE % 64 == 0, "a piece is whole rounds of a wave");
static_assert(PROFILES_SUBS * 8 == BLOCK, "one thread per (sub, field)");
static_assert(sizeof(nb_shell) == 64, "eight words a record");

template <int W>
struct ProfileEdges { float v[W]; };                  // e2[0 .. nbins], then +inf
// per centre: the position and the velocity as the caller passed them (`dims` values a centre, packed), the three ranges
struct ProfileCentre { float x[3]; };
struct ProfileVelocity { double v[3]; };
struct ProfileRanges { uint32_t r[6]; };

// The first position in [lo, hi) whose key is not below `key` (hi if none), found by the whole wave: 64 probes a level.  The result
// is the same in every lane.
__device__ __forceinline__ uint32_t profiles_wave_lower_bound(const uint64_t *__restrict__ a, uint32_t lo, uint32_t hi, uint64_t key)
{
    const uint32_t lane = threadIdx.x & 63u;
    while (lo < hi) {
        const uint32_t step = (hi - lo + 63u) / 64u;
        const uint64_t at = (uint64_t)lo + (uint64_t)lane * step;
        const bool below = at < hi && a[at] < key;
        const uint32_t k = (uint32_t)__popcll(__ballot(below));           // sorted: the lanes 0 .. k - 1
        if (k == 0u) return lo;
        const uint64_t next = (uint64_t)lo + (uint64_t)k * step;           // a[next] >= key, or next >= hi
        lo = lo + (k - 1u) * step + 1u;
        hi = next < hi ? (uint32_t)next : hi;
    }
    return lo;
}

// One wave per centre, and one more for entry ncenters of the two piece counts (zero: the scans end with the totals).
// rng[6 c ..] = c0, c1 of the rows -1, 0, +1.
__global__ __launch_bounds__(BLOCK)
void profiles_ranges(const uint64_t *__restrict__ skey, uint32_t n, const float *__restrict__ cen, uint32_t stride, uint32_t ncenters,
                     double inv_h, uint32_t *__restrict__ rng, uint32_t *__restrict__ pieces, uint32_t *__restrict__ split)
{
    const uint32_t c = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (c > ncenters) return;                                             // (wave-uniform)
    if (c == ncenters) {
        if (lane == 0u) pieces[c] = split[c] = 0u;
        return;
    }
    const float x = cen[(size_t)c * stride], y = cen[(size_t)c * stride + 1];      // finite: the host has looked
    const uint32_t ux = (uint32_t)(cell_coord((double)x, inv_h) + 1073741824), uy = (uint32_t)(cell_coord((double)y, inv_h) + 1073741824);
    const uint32_t x0 = ux ? ux - 1u : 0u, x1 = ux + 1u;                   // ux < 2^31: x1 + 1 stays inside the low word
    uint32_t total = 0u, r6[6];
#pragma unroll
    for (int r = -1; r <= 1; ++r) {
        uint32_t c0 = 0u, c1 = 0u;
        if (!(r < 0 && uy == 0u)) {                                       // the row below row 0 is empty
            const uint64_t rowkey = (uint64_t)(uy + (uint32_t)r) << 32;    // (uy + 1 <= 2^31: no body has that row, the range is empty)
            c0 = profiles_wave_lower_bound(skey, 0u, n, rowkey | x0);
            c1 = profiles_wave_lower_bound(skey, c0, n, (rowkey | x1) + 1u);
        }
        r6[2 * (r + 1)] = c0;
        r6[2 * (r + 1) + 1] = c1;
        total += c1 - c0;                                                 // disjoint ranges: at most n
    }
    if (lane < 6u) {
        uint32_t v = r6[0];
#pragma unroll
        for (int t = 1; t < 6; ++t) v = lane == (uint32_t)t ? r6[t] : v;
        rng[(size_t)c * 6 + lane] = v;
    }
    if (lane == 0u) {
        const uint32_t k = (total + PROFILES_PIECE - 1u) / PROFILES_PIECE;
        pieces[c] = k;
        split[c] = k > 1u ? k : 0u;
    }
}

// the shell of d2: the number of edges e2[1 ..] it is not below, or -1 where it lies in no shell (NaN, +inf, below e2[0], not below
// e2[nbins]; the edges that are not in use are +inf)
template <int CAP>
__device__ __forceinline__ int profiles_shell(float d2, const ProfileEdges<CAP + 1> &e2, float r2max)
{
    if (!(d2 >= e2.v[0] && d2 < r2max)) return -1;
    int b = 0;
#pragma unroll
    for (int t = 1; t <= CAP; ++t) b += d2 >= e2.v[t] ? 1 : 0;
    return b;
}

// The eight values of one body in a shell, fp64, one rounding per operation (the pragma: no contraction).  x, v, w are
// catalog_body's: the float values nb_sync returns, widened; c and vc the centre.
template <int D>
__device__ __forceinline__ void profiles_terms(const double (&x)[3], const double (&v)[3], double w, const double (&c)[3], const double (&vc)[3],
                                               double (&t)[8])
{
#pragma clang fp contract(off)
    double X[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int d = 0; d < D; ++d) { X[d] = x[d] - c[d]; u[d] = v[d] - vc[d]; }
    double r2 = X[0] * X[0] + X[1] * X[1], xu = X[0] * u[0] + X[1] * u[1], u2 = u[0] * u[0] + u[1] * u[1];
    if constexpr (D == 3) { r2 = r2 + X[2] * X[2]; xu = xu + X[2] * u[2]; u2 = u2 + u[2] * u[2]; }
    const double r = sqrt(r2);
    const bool on = r == 0.0;                                             // on the centre: count, mass and |u|^2 only, the rest +0
    const double vr = xu / r, lz = X[0] * u[1] - X[1] * u[0];
    t[0] = 1.0;
    t[1] = w;
    t[2] = on ? 0.0 : w * r;
    t[3] = on ? 0.0 : w * r2;
    t[4] = on ? 0.0 : w * vr;
    t[5] = on ? 0.0 : (w * vr) * vr;
    t[6] = w * u2;
    t[7] = on ? 0.0 : w * lz;
}

// ONE WAVE PER PIECE (launched with 64 threads a workgroup).  L is the handle's layout, NS the shells a lane owns: capacity 8 NS.
template <typename L, int NS>
__global__ __launch_bounds__(64)
void profiles_sweep(const typename L::vec *__restrict__ pos, const typename L::real *__restrict__ mass, const typename L::vec *__restrict__ vel,
                    const uint32_t *__restrict__ sval, const float2 *__restrict__ sxy, const float *__restrict__ cen,
                    const double *__restrict__ vcen, uint32_t ncenters, const uint32_t *__restrict__ rng, const uint64_t *__restrict__ first,
                    const uint64_t *__restrict__ prow, const ProfileEdges<8 * NS + 1> e2, float r2max, uint32_t nbins,
                    nb_shell *__restrict__ out, nb_shell *__restrict__ partial)
{
    constexpr int D = L::dims3 ? 3 : 2, CAP = 8 * NS;
    __shared__ int sh_shell[64];
    __shared__ double sh_val[64][8];
    const uint32_t lane = threadIdx.x, g = lane >> 3, f = lane & 7u;
    const uint64_t piece = blockIdx.x;
    const uint32_t c = profiles_wave_lower_bound(first, 0u, ncenters + 1u, piece + 1u) - 1u;   // first[0] = 0 <= piece < first[ncenters]
    const uint64_t base = first[c];
    const uint32_t k = (uint32_t)(piece - base), K = (uint32_t)(first[c + 1u] - base);
    const uint32_t a0 = rng[(size_t)c * 6], a1 = rng[(size_t)c * 6 + 2], a2 = rng[(size_t)c * 6 + 4];
    const uint32_t l0 = rng[(size_t)c * 6 + 1] - a0, l1 = rng[(size_t)c * 6 + 3] - a1, l2 = rng[(size_t)c * 6 + 5] - a2;
    const uint32_t total = l0 + l1 + l2, off0 = k * PROFILES_PIECE, off1 = total - off0 < PROFILES_PIECE ? total : off0 + PROFILES_PIECE;
    float cf[3] = {cen[(size_t)c * D], cen[(size_t)c * D + 1], 0.f};
    double cd[3], vc[3] = {0.0, 0.0, 0.0};
    if constexpr (D == 3) cf[2] = cen[(size_t)c * D + 2];
#pragma unroll
    for (int d = 0; d < 3; ++d) cd[d] = (double)cf[d];
    if (vcen) {
#pragma unroll
        for (int d = 0; d < D; ++d) vc[d] = vcen[(size_t)c * D + d];
    }
    double acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0.0;
    for (uint32_t round = off0; round < off1; round += 64u) {            // wave-uniform
        const uint32_t o = round + lane;
        int shell = -1;
        uint32_t p = 0u;
        if (o < off1) {
            p = o < l0 ? a0 + o : o - l0 < l1 ? a1 + (o - l0) : a2 + (o - l0 - l1);
            const float2 q = sxy[p];
            const float d2 = neighbors_d2(cf[0], cf[1], q.x, q.y);
            if constexpr (D == 2) shell = profiles_shell<CAP>(d2, e2, r2max);
            else if (d2 < r2max) shell = 0;                               // its z is worth reading
        }
        double x[3], v[3], w = 0.0;
        if (shell >= 0) {
            catalog_body<L>(pos, mass, vel, sval[p], x, v, w);
            if constexpr (D == 3) {
#pragma clang fp contract(off)
                const float2 q = sxy[p];
                const float dz = (float)x[2] - cf[2];
                shell = profiles_shell<CAP>(neighbors_d2(cf[0], cf[1], q.x, q.y) + dz * dz, e2, r2max);
            }
        }
        const unsigned long long in = __ballot(shell >= 0);
        const uint32_t staged = (uint32_t)__popcll(in);
        if (shell >= 0) {
            const uint32_t slot = (uint32_t)__popcll(in & ((1ull << lane) - 1ull));
            double t[8];
            profiles_terms<D>(x, v, w, cd, vc, t);
            sh_shell[slot] = shell;
#pragma unroll
            for (int e = 0; e < 8; ++e) sh_val[slot][e] = t[e];
        }
        __syncthreads();
        for (uint32_t e = 0; e < staged; ++e) {
            const int sh = sh_shell[e];
            const double val = sh_val[e][f];
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s] += sh == (int)g + 8 * s ? val : 0.0;
        }
        __syncthreads();                                                  // the next round stages again
    }
    nb_shell *row = K == 1u ? out + (size_t)c * nbins : partial + (size_t)(prow[c] + k) * nbins;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const uint32_t b = g + 8u * (uint32_t)s;
        if (b < nbins) {
            if (f == 0u) row[b].count = (uint64_t)acc[s];
            else ((double *)&row[b])[f] = acc[s];
        }
    }
}

// The rows of the split centres.  Workgroups take the (centre, shell) items c * nbins + b in a grid-stride loop; an item of a centre
// that is not split is passed over.  Thread (s, f): s = threadIdx.x / 8.
__global__ __launch_bounds__(BLOCK)
void profiles_combine(const uint64_t *__restrict__ first, const uint64_t *__restrict__ prow, uint32_t ncenters, uint32_t nbins,
                      const nb_shell *__restrict__ partial, nb_shell *__restrict__ out)
{
    __shared__ uint64_t red[PROFILES_SUBS][8];
    const uint32_t s = threadIdx.x >> 3, f = threadIdx.x & 7u;
    const uint64_t items = (uint64_t)ncenters * nbins;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {  // workgroup-uniform, and so is the skip
        const uint32_t c = (uint32_t)(item / nbins), b = (uint32_t)(item % nbins);
        const uint32_t K = (uint32_t)(first[c + 1u] - first[c]);
        if (K <= 1u) continue;
        const uint64_t *words = (const uint64_t *)(partial + (size_t)prow[c] * nbins + b) + f;   // row k: + 8 k nbins words
        uint64_t bits = 0ull;                                             // +0.0, or the count 0
        if (s < K) {
            bits = words[(size_t)s * 8u * nbins];
            if (f == 0u) for (uint32_t k = s + PROFILES_SUBS; k < K; k += PROFILES_SUBS) bits += words[(size_t)k * 8u * nbins];
            else {
                double a = __longlong_as_double((long long)bits);
                for (uint32_t k = s + PROFILES_SUBS; k < K; k += PROFILES_SUBS) a += __longlong_as_double((long long)words[(size_t)k * 8u * nbins]);
                bits = (uint64_t)__double_as_longlong(a);
            }
        }
        red[s][f] = bits;
        __syncthreads();
        for (uint32_t h = PROFILES_SUBS / 2; h >= 1u; h >>= 1) {
            if (s < h) {
                if (f == 0u) red[s][f] += red[s + h][f];
                else red[s][f] = (uint64_t)__double_as_longlong(__longlong_as_double((long long)red[s][f]) + __longlong_as_double((long long)red[s + h][f]));
            }
            __syncthreads();
        }
        if (s == 0u) ((uint64_t *)(out + (size_t)c * nbins + b))[f] = red[0][f];
        __syncthreads();                                                  // the next item writes red again
    }
}

}  // namespace nbk
