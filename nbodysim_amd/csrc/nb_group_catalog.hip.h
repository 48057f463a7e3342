// nb_group_catalog.hip.h — nb_group_catalog's device side: mass, centre, motion, dispersion and radius of every friends-of-friends
// group (include/nbody.h has the contract; tests/group_catalog_model.py is its numpy statement).  The labels are nb_groups'
// (parent[] after groups_flatten, nb_groups.hip.h); everything here is a SEGMENTED REDUCTION in fp64 over the bodies sorted by label.
//   catalog_labels         key[i] = label of body i, val[i] = i, the input of the stable sort (nb_tree_sort_pairs): in the sorted order
//                          a group is one SEGMENT of consecutive positions, its members in ascending body index, its head first
//   catalog_heads          a head is a position whose label differs from its predecessor's; a head finds its segment's end (galloping,
//                          then a binary search: one probe for a singleton, 2 log2(length) for the giant group), leaves the length at
//                          len_row[label] and flag[p] = length >= min_members.  nb_tree_scan of the flags: rank[p], and rank[n] = *count
//   catalog_rows           a kept head writes label and members of record rank[p] and turns len_row[label] into that row; the head of
//                          a group that is not kept writes CATALOG_NO_ROW there.  Every position finds its row as len_row[label]
//   catalog_sums<L>        PASS A, the hot path: sum of {w, w x, w v, x, v} per segment (1 + 4 x dims doubles)
//   catalog_spread<L>      PASS B: sum of w |v - vel|^2 and max of |x - pos|^2 about the finished means
//   catalog_carry<V>       the second launch of either pass (below)
//   catalog_means<D>, catalog_finish    one lane per record: the divisions by W, the square root
// THE REDUCTION IS BALANCED OVER SORTED POSITIONS, NOT OVER GROUPS.  Workgroup b takes the RUN of CATALOG_RUN consecutive positions
// [b R, (b + 1) R), tile by tile (BLOCK positions, one per lane), whatever segments they hold.  Inside a tile the lanes are combined
// by a head-flagged segmented inclusive scan: (f1, v1) (+) (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2), six shuffle steps inside a wave,
// the four waves' totals through LDS, and the value carried from tile to tile in registers.  The position at a segment's end then
// holds the sum of the piece of its segment that lies in the run:
//   - a segment that lies wholly inside the run (its head was seen there) writes its sums directly;
//   - the FIRST segment of a run may have begun in an earlier run and the LAST may go on into the next: such a piece goes to one of
//     the two CARRY SLOTS of the workgroup: slot 2b = the piece of a segment that began before the run (flagged END where the segment
//     ends in this run), slot 2b + 1 = the piece of a segment that began in the run and leaves it.  A segment that covers the whole
//     run is one piece, in slot 2b.
// catalog_carry is ONE workgroup that runs the same scan over the slots in order: an odd slot is a head, an even one continues, a
// slot that is not valid is zero; the slot flagged END holds the segment's total and writes it.  Its work is 2 n / R slots whatever
// the partition, so all bodies in one group cost what all singletons cost; no lane and no workgroup ever walks a group.
// THE ORDER OF EVERY SUM IS FIXED by the sorted order (a function of the labels alone), the tile and run boundaries (of n alone) and
// the scan's tree: there is no atomic on a double anywhere, and a position of a group that is not kept contributes zeros.
// Indices: every position read is below n (the successor p + 1 only where p + 1 < n); label < n; a row is below *count; slots are
// 2 x gridDim.x.  A lane past n holds zeros and is no head.
#pragma once
#include "nb_groups.hip.h"

namespace nbk {

constexpr uint32_t CATALOG_RUN = 1024;                // sorted positions per workgroup: 4 tiles of BLOCK
constexpr uint32_t CATALOG_NO_ROW = 0xffffffffu;
constexpr int CATALOG_FIELDS = 13;                    // 1 + 4 x 3: what a slot and a row of sums hold at the most
constexpr uint32_t CATALOG_SLOT_VALID = 1u, CATALOG_SLOT_END = 2u;
static_assert(CATALOG_RUN % BLOCK == 0, "a run is whole tiles");

struct CatalogSums { double v[CATALOG_FIELDS]; };
struct CatalogSlot { double v[CATALOG_FIELDS]; uint32_t label, flags; };

// F doubles: the first F - M are summed, the last M take the maximum
template <int F, int M>
struct CatalogVal {
    static constexpr int fields = F;
    double v[F];
    __device__ __forceinline__ static CatalogVal zero()
    {
        CatalogVal z;
#pragma unroll
        for (int k = 0; k < F; ++k) z.v[k] = 0.0;
        return z;
    }
    // a before b in the sorted order
    __device__ __forceinline__ static CatalogVal combine(const CatalogVal &a, const CatalogVal &b)
    {
        CatalogVal r;
#pragma unroll
        for (int k = 0; k < F - M; ++k) r.v[k] = a.v[k] + b.v[k];
#pragma unroll
        for (int k = F - M; k < F; ++k) r.v[k] = a.v[k] > b.v[k] ? a.v[k] : b.v[k];
        return r;
    }
};

__global__ __launch_bounds__(BLOCK)
void catalog_labels(const uint32_t *__restrict__ label, uint32_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    key[i] = label[i];
    val[i] = i;
}

// n + 1 lanes: flag[n] = 0, so that the exclusive scan ends with the count
__global__ __launch_bounds__(BLOCK)
void catalog_heads(const uint64_t *__restrict__ skey, uint32_t n, uint32_t min_members, uint32_t *__restrict__ flag, uint32_t *__restrict__ len_row)
{
    const uint64_t p64 = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p64 > n) return;
    const uint32_t p = (uint32_t)p64;
    uint32_t f = 0u;
    if (p < n) {
        const uint64_t key = skey[p];
        if (p == 0u || skey[p - 1u] != key) {
            uint64_t d = 1u;                                              // skey[p + d / 2] == key is known
            while (p + d < n && skey[p + d] == key) d <<= 1;
            const uint32_t lo = (uint32_t)(p + d / 2u + 1u), hi = (uint32_t)(p + d < n ? p + d : n);
            const uint32_t len = neighbors_lower_bound(skey, lo, hi, key + 1u) - p;
            len_row[(uint32_t)key] = len;
            f = len >= min_members ? 1u : 0u;
        }
    }
    flag[p] = f;
}

__global__ __launch_bounds__(BLOCK)
void catalog_rows(const uint64_t *__restrict__ skey, uint32_t n, const uint32_t *__restrict__ flag, const uint64_t *__restrict__ rank,
                  uint32_t *__restrict__ len_row, nb_group *__restrict__ rec)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint64_t key = skey[p];
    if (p != 0u && skey[p - 1u] == key) return;
    const uint32_t label = (uint32_t)key;                                 // only this lane touches len_row[label]
    if (flag[p]) {
        const uint32_t row = (uint32_t)rank[p];
        rec[row].label = label;
        rec[row].members = len_row[label];
        len_row[label] = row;
    } else len_row[label] = CATALOG_NO_ROW;
}

// One tile of the segmented scan.  In: the lane's value and whether it is a head; carry / carry_head = the scan of everything the
// workgroup has seen before this tile.  Out: val = the sum from the lane's segment head (or from the first position the workgroup
// saw, if the head lies before it) up to the lane; head = the segment's head has been seen; the carry moved behind the tile.
// Every thread of the workgroup calls it (two barriers).
template <typename V>
__device__ __forceinline__ void catalog_tile_scan(V &val, bool &head, V &carry, bool &carry_head, double (*agg)[V::fields], uint32_t *aggf)
{
    constexpr int WAVES = BLOCK / 64;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool f = head;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        V up;
#pragma unroll
        for (int k = 0; k < V::fields; ++k) up.v[k] = __shfl_up(val.v[k], d, 64);
        const bool uf = __shfl_up((int)f, d, 64) != 0;
        if (lane >= d) {
            if (!f) val = V::combine(up, val);
            f = f || uf;
        }
    }
    if (lane == 63u) {
#pragma unroll
        for (int k = 0; k < V::fields; ++k) agg[wave][k] = val.v[k];
        aggf[wave] = f ? 1u : 0u;
    }
    __syncthreads();
    V pre = carry, mine = carry;
    bool pf = carry_head, mine_f = carry_head;
#pragma unroll
    for (uint32_t u = 0; u < (uint32_t)WAVES; ++u) {
        if (u == wave) { mine = pre; mine_f = pf; }
        V a;
#pragma unroll
        for (int k = 0; k < V::fields; ++k) a.v[k] = agg[u][k];
        const bool af = aggf[u] != 0u;
        pre = af ? a : V::combine(pre, a);
        pf = pf || af;
    }
    if (!f) val = V::combine(mine, val);
    head = f || mine_f;
    carry = pre;
    carry_head = pf;
    __syncthreads();                                                      // the next tile writes agg / aggf again
}

// The run of workgroup blockIdx.x.  load(p, row) is the value of sorted position p, asked only for positions of kept groups.
template <typename V, typename Load>
__device__ __forceinline__ void catalog_pass(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ row_of, uint32_t n,
                                             CatalogSums *__restrict__ sums, CatalogSlot *__restrict__ slot, Load load)
{
    __shared__ double agg[BLOCK / 64][V::fields];
    __shared__ uint32_t aggf[BLOCK / 64];
    __shared__ uint32_t meta[4];                                          // label and flags of the two slots
    if (threadIdx.x < 4u) meta[threadIdx.x] = 0u;                          // (ahead of the first tile's barriers)
    const uint64_t base = (uint64_t)blockIdx.x * CATALOG_RUN;
    const uint64_t last = (base + CATALOG_RUN < n ? base + CATALOG_RUN : n) - 1u;   // the run's last position; base < n by the grid
    V carry = V::zero();
    bool carry_head = false;
    for (uint64_t tile = base; tile <= last; tile += BLOCK) {             // workgroup-uniform
        const uint64_t p64 = tile + threadIdx.x;
        const bool active = p64 < n;
        const uint32_t p = (uint32_t)p64;
        V val = V::zero();
        bool head = false, true_end = false;
        uint32_t label = 0u, row = CATALOG_NO_ROW;
        if (active) {
            const uint64_t key = skey[p];
            label = (uint32_t)key;
            head = p == 0u || skey[p - 1u] != key;
            true_end = p == n - 1u || skey[p + 1u] != key;
            row = row_of[label];
            if (row != CATALOG_NO_ROW) val = load(p, row);
        }
        catalog_tile_scan<V>(val, head, carry, carry_head, agg, aggf);    // head: the segment began in this run
        if (active && row != CATALOG_NO_ROW && (true_end || p64 == last)) {
            if (true_end && head) {
#pragma unroll
                for (int k = 0; k < V::fields; ++k) sums[row].v[k] = val.v[k];
            } else {
                const uint32_t which = head ? 1u : 0u;                    // began here and leaves the run | began before the run
                CatalogSlot &c = slot[2u * blockIdx.x + which];
#pragma unroll
                for (int k = 0; k < V::fields; ++k) c.v[k] = val.v[k];
                meta[2u * which] = label;
                meta[2u * which + 1u] = CATALOG_SLOT_VALID | (true_end ? CATALOG_SLOT_END : 0u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 2u) {
        slot[2u * blockIdx.x + threadIdx.x].label = meta[2u * threadIdx.x];
        slot[2u * blockIdx.x + threadIdx.x].flags = meta[2u * threadIdx.x + 1u];
    }
}

// the float values nb_sync returns (pack_bodies), widened
template <typename L>
__device__ __forceinline__ void catalog_body(const typename L::vec *__restrict__ pos, const typename L::real *__restrict__ mass,
                                             const typename L::vec *__restrict__ vel, uint32_t i, double (&x)[3], double (&v)[3], double &w)
{
    const auto q = pos[i];
    const auto u = vel[i];
    x[0] = (double)(float)q.x; x[1] = (double)(float)q.y; x[2] = 0.0;
    v[0] = (double)(float)u.x; v[1] = (double)(float)u.y; v[2] = 0.0;
    if constexpr (L::dims3) { x[2] = (double)(float)q.z; v[2] = (double)(float)u.z; }
    const float m = (float)mass_at<L>(pos, mass, i);
    w = m > 0.0f ? (double)m : 0.0;
}

// PASS A.  v[0] = w; v[1 ..] = w x; then w v; then x; then v (the unweighted sums serve a group without mass)
template <typename L>
__global__ __launch_bounds__(BLOCK)
void catalog_sums(const typename L::vec *__restrict__ pos, const typename L::real *__restrict__ mass, const typename L::vec *__restrict__ vel,
                  const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ row_of, uint32_t n,
                  CatalogSums *__restrict__ sums, CatalogSlot *__restrict__ slot)
{
    constexpr int D = L::dims3 ? 3 : 2;
    using V = CatalogVal<1 + 4 * D, 0>;
    catalog_pass<V>(skey, row_of, n, sums, slot, [&](uint32_t p, uint32_t) {
        double x[3], v[3], w;
        catalog_body<L>(pos, mass, vel, sidx[p], x, v, w);
        V r;
        r.v[0] = w;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            r.v[1 + d] = w * x[d];                                        // exact: 24 x 24 bits
            r.v[1 + D + d] = w * v[d];
            r.v[1 + 2 * D + d] = x[d];
            r.v[1 + 3 * D + d] = v[d];
        }
        return r;
    });
}

// PASS B about the means catalog_means left in the records.  v[0] = w |v - vel|^2 (w = 1 in a group without mass), v[1] = |x - pos|^2
template <typename L>
__global__ __launch_bounds__(BLOCK)
void catalog_spread(const typename L::vec *__restrict__ pos, const typename L::real *__restrict__ mass, const typename L::vec *__restrict__ vel,
                    const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ row_of, uint32_t n,
                    const nb_group *__restrict__ rec, CatalogSums *__restrict__ sums, CatalogSlot *__restrict__ slot)
{
    constexpr int D = L::dims3 ? 3 : 2;
    using V = CatalogVal<2, 1>;
    catalog_pass<V>(skey, row_of, n, sums, slot, [&](uint32_t p, uint32_t row) {
        double x[3], v[3], w;
        catalog_body<L>(pos, mass, vel, sidx[p], x, v, w);
        const nb_group &g = rec[row];
        if (!(g.mass > 0.0)) w = 1.0;
        double dv2 = 0.0, dx2 = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double dv = v[d] - g.vel[d], dx = x[d] - g.pos[d];
            dv2 += dv * dv;
            dx2 += dx * dx;
        }
        V r;
        r.v[0] = w * dv2;
        r.v[1] = dx2;
        return r;
    });
}

// The second launch of a pass: ONE workgroup scans the `slots` carry slots in order and writes the totals of the segments that
// reach across runs.  An END slot is valid, and valid slots belong to kept groups: row_of[label] is a row.
template <typename V>
__global__ __launch_bounds__(BLOCK)
void catalog_carry(const CatalogSlot *__restrict__ slot, uint32_t slots, const uint32_t *__restrict__ row_of, CatalogSums *__restrict__ sums)
{
    __shared__ double agg[BLOCK / 64][V::fields];
    __shared__ uint32_t aggf[BLOCK / 64];
    V carry = V::zero();
    bool carry_head = false;
    for (uint32_t tile = 0; tile < slots; tile += BLOCK) {
        const uint32_t q = tile + threadIdx.x;
        V val = V::zero();
        bool head = false;
        uint32_t flags = 0u, label = 0u;
        if (q < slots) {
            flags = slot[q].flags;
            label = slot[q].label;
            if (flags & CATALOG_SLOT_VALID) {
#pragma unroll
                for (int k = 0; k < V::fields; ++k) val.v[k] = slot[q].v[k];
                head = (q & 1u) != 0u;
            }
        }
        catalog_tile_scan<V>(val, head, carry, carry_head, agg, aggf);
        if (flags & CATALOG_SLOT_END) {
            const uint32_t row = row_of[label];
#pragma unroll
            for (int k = 0; k < V::fields; ++k) sums[row].v[k] = val.v[k];
        }
    }
}

// W = mass when mass > 0, else the members (every w = 1: the unweighted means)
template <int D>
__global__ __launch_bounds__(BLOCK)
void catalog_means(const CatalogSums *__restrict__ sums, uint32_t count, nb_group *__restrict__ rec)
{
    const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
    if (row >= count) return;
    const CatalogSums &s = sums[row];
    nb_group g = rec[row];                                                // label and members are catalog_rows'
    const double m = s.v[0];
    const bool heavy = m > 0.0;
    const double W = heavy ? m : (double)g.members;
    const int at = heavy ? 1 : 1 + 2 * D;
    g.mass = m;
    g.pos[2] = g.vel[2] = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        g.pos[d] = s.v[at + d] / W;
        g.vel[d] = s.v[at + D + d] / W;
    }
    g.sigma2 = g.r_max = 0.0;
    rec[row] = g;
}

__global__ __launch_bounds__(BLOCK)
void catalog_finish(const CatalogSums *__restrict__ sums, uint32_t count, nb_group *__restrict__ rec)
{
    const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
    if (row >= count) return;
    const double m = rec[row].mass, W = m > 0.0 ? m : (double)rec[row].members;
    rec[row].sigma2 = sums[row].v[0] / W;
    rec[row].r_max = sqrt(sums[row].v[1]);
}

}  // namespace nbk
