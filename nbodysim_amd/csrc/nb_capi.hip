// nb_capi.hip — the C ABI of include/nbody.h over the gfx950 kernels.
//
// One nb_sim stands for one `Simulation` of the reference
// (Nbodysim/headers/Simulation.hpp:49-75).  Device state is SoA:
//   pos[2]   full-n (x,y) replicas, double buffered (step n reads cur, writes next)
//   mass     full n            radius  full n (carried, float)
//   vel,acc  owned block only  partial [slabs][i_count] force partial sums
// No CPU fallback exists: every entry that computes needs a HIP device.
#include "nb_sim.hip.h"

extern "C" int nb_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

// ---- launch geometry and step path ----
// Launch geometry of one one-sided force job.  The kernel is VALU-bound, so what
// matters is (a) enough independent work per lane — 2P particles per lane, P = 4 measured best — and
// (b) enough workgroups in flight to keep 5-8 waves per SIMD issuing and to even out the tail: about
// 32 workgroups per CU (profiles/history/r01_force_tiled_geometry_sweep.log).  When i-particles are scarce (sharded or small runs)
// the j range is cut into more tile-aligned slices (at most 128: every slice is a slab that
// `integrate` re-reads), and P drops only when even that cannot fill half the target.
// Slices are whole LDS tiles and none is empty: js = ceil(tiles / ceil(tiles / want)).
static uint32_t even_slices(uint32_t jn, uint32_t want)
{
    const uint32_t tiles = (jn + TJ - 1) / TJ;
    if (want < 1) want = 1;
    if (want > tiles) want = tiles;
    const uint32_t per = (tiles + want - 1) / want;
    return (tiles + per - 1) / per;
}

static ForceJob plan_job(const nb_sim *s, uint32_t jb, uint32_t je, uint32_t slab0,
                         uint32_t gap_begin = 0xffffffffu, uint32_t gap_len = 0)
{
    ForceJob j{jb, je, 0, slab0, 1, 0, gap_begin, gap_len};
    const uint32_t ic = (uint32_t)s->i_count;
    if (je <= jb) return j;
    const uint32_t jn = je - jb;
    if (s->p.sum_order == NB_SUM_SEQUENTIAL) { j.js = 1; j.P = 1; j.i_tiles = (ic + BLOCK - 1) / BLOCK; return j; }
    // fp32: the 4 waves of a workgroup share 64 i-lanes and split each j-tile (WS = 4), a lane owns 2P
    // particles -> 128P particles per workgroup; fp64: 256 i-lanes, P particles per lane.
    const uint32_t lanes_i = s->fp64 ? 1u : 2u;                 // particles per lane per P
    const uint32_t ilanes = s->fp64 ? (uint32_t)BLOCK : (uint32_t)BLOCK / TILED_F32_WS;
    const uint32_t target = 32u * (uint32_t)s->cus;             // workgroups wanted in the grid (profiles/history/r01_force_tiled_geometry_sweep.log)
    const uint32_t max_slices = 128;                            // bounds the slab traffic of `integrate`
    const uint32_t tiles = (jn + TJ - 1) / TJ;
    const int forced_p = s->p.lanes_p > 0 ? s->p.lanes_p : 0;
    const int pmax = s->fp64 ? 2 : 4;
    // Largest P (most independent chains per lane, fewest LDS reads per pair) that still yields
    // at least half the wanted workgroups; P halves only when both i and j are scarce.
    for (int P = pmax; P >= 1; P >>= 1) {
        if (forced_p > 0 && P != (forced_p > pmax ? pmax : forced_p)) continue;
        const uint32_t i_tiles = (ic + ilanes * lanes_i * P - 1) / (ilanes * lanes_i * P);
        uint32_t want = (target + i_tiles - 1) / i_tiles;
        if (want > max_slices) want = max_slices;
        if (s->p.j_slices > 0) want = (uint32_t)s->p.j_slices;
        j.P = P;
        j.i_tiles = i_tiles;
        j.js = even_slices(jn, want);
        if (forced_p > 0 || s->p.j_slices > 0 || P == 1) break;
        const uint32_t reach = i_tiles * (tiles < max_slices ? tiles : max_slices);   // most workgroups this P can give
        if (reach >= target / 2) break;
    }
    return j;
}

static void plan(nb_sim *s)
{
    const uint32_t n = (uint32_t)s->n, ib = (uint32_t)s->i_begin, ic = (uint32_t)s->i_count;
    s->job_all = plan_job(s, 0, n, 0);
    s->slabs_all = s->path == StepPath::SYM ? 1 : s->job_all.js;   // the symmetric path leaves one summed slab
    s->job_local = plan_job(s, ib, ib + ic, 0);
    // everything but the owned block, in one launch: virtual j range [0, n - ic) with a gap at the block
    s->job_remote = plan_job(s, 0, n - ic, s->job_local.js, ib, ic);
    s->slabs_two_phase = s->job_local.js + s->job_remote.js;
}

// Symmetric path: tiled runs with eps > 0 that are big enough to fill the chip with (tile, chunk-range)
// items — either the whole system on one GPU, or (shard_world > 1) this rank's share of the pairs of a
// sharded run.  NB_FLAG_NO_SYMMETRY forces the one-sided kernels.
// The branch-free pair body lets a particle meet itself (and coincident particles meet): r = 0 gives
// 0 x (eps^2)^(-3/2), which is exactly 0 only while (1/eps)^3 is finite — in fp32 down to eps ~ 1.5e-13.
// Below that (and for eps = 0) the one-sided kernels keep the reference's `if (r_sq > 0)` guard (Quadtree.hpp:139).
static bool needs_guard(const nb_sim *s) { return s->fp64 ? !(s->p.eps > 0.0f) : !(s->p.eps >= 1e-12f); }

// Block-tile of a handle's symmetric plan.  The WAVE-SPLIT kernels (force_sym_f32<..., WS>: tiles of 512, the 4 waves of a
// workgroup share the stationary particles and split the chunks) give the planner work units a quarter the size, items
// whose stationary row is 4 KiB instead of 16, and a sweep without barriers — what small and mid-size systems need to
// fill 1024 resident workgroup slots evenly — for four times the travelling partials per pair, which large systems do not
// pay back.  Measured (profiles/history/r04_ws_sweep.log): -3 ... -4 % step time at N = 25 000 (reference
// workload), -2.5 % at 16 384 and 32 768, neutral at 65 536, +1.3 ... +2.6 % at 131 072: used below 49 152 bodies.
// fp32 2-D, single handle (a rank of a sharded run keeps the classic tiles: its blocks are whole 2048-particle tiles).
// nb_params.sym_tile = 512 / 2048 forces one.  Rank-independent (n and parameters only).
static uint32_t sym_tile_of(const nb_params &p, size_t n)
{
    if (p.precision == NB_FP64 || p.dims == 3 || p.shard_world > 1 || (p.flags & NB_FLAG_SHARD_SINGLE)) return SYM_SB;
    if (p.sym_tile) return (uint32_t)p.sym_tile;
    return n < SYM_WS_MAX_N ? SYM_SB_WS : SYM_SB;
}

// Body order (nb_order.hip.h): the whole-system symmetric launch sweeps the bodies along a Morton curve instead of in the caller's
// index order, for the clock the part then holds.  For unsharded 2-D direct-sum handles on the symmetric path, fp32 or fp64, from
// ORDER_MIN_N bodies on.  Measured on Plummer spheres in index order, order on against off in interleaved rounds on one device
// (profiles/body_order_ab.log): the force launch is 3.4 % shorter at 262 144 bodies, 3.4 % at 131 072 and 3.1 % at 65 536; the copy of
// the positions, the redirected gather and a sixteenth of a sort take 29 / 12 / 8 us of that back, which leaves 2.9 % / 2.6 % / 1.3 %
// of a step.  The smallest gain this kernel has been changed for is 1.4 % of a step: on from 131 072 bodies, off at 65 536.
// NB_FLAG_NO_BODY_ORDER switches it off; NB_FLAG_BODY_ORDER switches it on at ANY size — and, so that the small systems of the tests
// reach it, lifts the lower size limit of the symmetric scheme itself (order_forced) where the handle is otherwise eligible.
// And UP TO ORDER_MAX_N bodies: the order costs accuracy.  The terms a lane adds into one fp32 accumulator over an item are then
// nearly equal, so their rounding errors are no longer random but of one sign, and they grow with the chunks per item of the plan.
// Largest error of the accelerations against an fp64 handle, in units of max |a|, order off -> on: 2.6e-7 -> 1.4e-6 at 131 072 bodies
// (16 chunks per item), 2.9e-7 -> 3.0e-6 at 262 144 (44), 5.5e-7 -> 3.1e-5 at 524 288 (172), 1.1e-6 -> 7.8e-5 at 1 048 576 (684); the
// momentum sum 2.4e-10 -> 1.3e-8 of sum |m a| at 262 144.  The bar of this project is 2e-5 of max |a|: met to 262 144 bodies with
// room, missed from 524 288 on, not measured in between.
constexpr size_t ORDER_MIN_N = 131072, ORDER_MAX_N = 262144;

static bool order_possible(const nb_params &p, size_t n, size_t i_count)
{
    return !(p.flags & NB_FLAG_NO_BODY_ORDER) && p.force == NB_FORCE_DIRECT && p.dims != 3 && p.shard_world <= 1 &&
           !(p.flags & NB_FLAG_SHARD_SINGLE) && i_count == n;
}

static bool order_forced(const nb_sim *s) { return (s->p.flags & NB_FLAG_BODY_ORDER) && order_possible(s->p, s->n, s->i_count); }

static bool order_wanted(const nb_sim *s)
{
    if (s->path != StepPath::SYM || !order_possible(s->p, s->n, s->i_count)) return false;
    if (s->p.flags & NB_FLAG_BODY_ORDER) return true;
    // Not by itself where the caller asks for the mass-scaled body (NB_FLAG_MASS_SCALING / _MEASURED): the rounding of its pre-multiplied
    // position sigma_j x_j is the same for every partner of a travelling body, and along the curve those partners are its neighbours —
    // the errors add up instead of averaging out.  Measured at 262 144 equal-ish masses: the scaled body is 4.1e-7 of the force scale
    // from the general one in index order, 7.0e-6 along the curve (above the 2e-6 of the measured rule, which then declines).
    const bool scaling = (s->p.flags & (NB_FLAG_MASS_SCALING | NB_FLAG_MASS_SCALING_MEASURED)) && !(s->p.flags & NB_FLAG_NO_MASS_SCALING);
    return s->n >= ORDER_MIN_N && s->n <= ORDER_MAX_N && !scaling;
}

static bool sym_eligible(const nb_sim *s)
{
    if (s->p.flags & NB_FLAG_NO_SYMMETRY) return false;
    if (s->p.integrator == NB_INTEGRATOR_HERMITE4) return false;      // its one force kernel is one-sided (nb_hermite.hip.h)
    if (s->p.sum_order != NB_SUM_TILED || needs_guard(s)) return false;
    if (s->fp64 && s->p.rsqrt_mode != NB_RSQRT_EXACT) return false;
    if (s->p.integrator != NB_INTEGRATOR_KICK_DRIFT && s->i_count != s->n) return false;
    // smallest system worth the symmetric scheme: 16 384 bodies with the classic tiles (rounds 1-3); with the wave-split tiles and
    // their uniform one-chunk-per-wave plans it overtakes the one-sided kernel from ~5 600 bodies on (-4 ... -8 % at 5 632, -14 ... -17 %
    // at 6 144, -24 ... -28 % at 7 168, -32 ... -34 % at 10 000; +1 ... +6 % at 5 120, +25 % at 4 096:
    // profiles/history/r04_small_n_plans.log)
    if (!order_forced(s) && s->n < (sym_tile_of(s->p, s->n) == SYM_SB_WS ? (size_t)5632 : 8 * (size_t)SYM_SB)) return false;
    const uint32_t world = s->p.shard_world > 1 ? (uint32_t)s->p.shard_world : 1u;
    // Travelling partials: one element per (tile, later particle) pair the handle evaluates — tiles x n / 2 for a
    // whole system (1 GiB at N = 524 288 fp32, 2 GiB at 1 048 576, 32 GiB at 4 194 304), 1/world of that for a rank.
    // Sized for the 288 GB of an MI355X: up to 96 GiB and a third of what is free now (N ~ 7 million fp32 is the
    // largest symmetric run; beyond that the one-sided kernel).  Ranks of a sharded run must all take the same
    // decision (it selects the exchange protocol), so there the limit does not look at this device's free memory
    // and uses the rank-independent bound; an allocation that does not fit fails nb_create loudly (NB_ENOMEM).
    size_t cap = (size_t)96 << 30;
    if (world == 1) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)24 << 30; }
        if (free_b / 3 < cap) cap = free_b / 3;
    }
    if (sym_slab_r_bound((uint32_t)s->n, world, sym_tile_of(s->p, s->n)) * s->esz > cap) return false;
    return true;
}

// NB_FLAG_SHARD_SINGLE: the sharded protocols with one rank (shard_world = 1, the handle owns everything): the rank's
// "share" is every pair, all of them local; the host-side exchange degenerates to copies.  Lets a one-GPU box run the
// whole split-step + collective path (nb_comm_*, nb_exchange_*).
static bool single_rank(const nb_sim *s)
{
    return (s->p.flags & NB_FLAG_SHARD_SINGLE) && s->p.shard_world == 1 && s->p.shard_rank == 0 && s->i_count == s->n;
}

// Decided once, before nb_create allocates the handle's buffers (sym_eligible looks at the free device memory, which they change).
static StepPath step_path_of(const nb_sim *s)
{
    const bool whole = s->i_count == s->n;
    if (s->p.force == NB_FORCE_TREE) return StepPath::ONE_SIDED;      // its force launch is launch_tree_force
    if (sym_eligible(s)) {
        const bool kick_drift = s->p.integrator == NB_INTEGRATOR_KICK_DRIFT, allreduce = (s->p.flags & NB_FLAG_SHARD_ALLREDUCE) != 0;
        const size_t w = (size_t)s->p.shard_world;
        if (single_rank(s)) {
            if (kick_drift) return allreduce ? StepPath::SYM_REPLICATED : StepPath::SYM_SHARDED;
        } else if (s->p.shard_world <= 1) {
            if (whole) return StepPath::SYM;                   // single handle owns everything
        } else if (s->n / w >= 2 * (size_t)SYM_SB && s->n % (w * SYM_SB) == 0) {
            // replicated: every rank holds (and integrates) everything; sharded: equal blocks of whole tiles
            if (whole && allreduce && kick_drift) return StepPath::SYM_REPLICATED;
            if (!whole && s->i_count == s->n / w && s->i_begin == (size_t)s->p.shard_rank * s->i_count) return StepPath::SYM_SHARDED;
        }
    }
    return !whole && s->p.sum_order != NB_SUM_SEQUENTIAL ? StepPath::TWO_PHASE : StepPath::ONE_SIDED;
}

static bool symmetric(const nb_sim *s) { return s->path == StepPath::SYM || s->path == StepPath::SYM_SHARDED || s->path == StepPath::SYM_REPLICATED; }

// Chunk-units of local work a rank holds back to run beside the reduce-scatter: 40 us of whole-chip work at the
// measured 35 units/us (fp32) or 14 (fp64) of 256 CUs.  Alone on the chip those items take 50-60 us and the
// hand-over between the streams ~15 us, so the split pays when the collective is exposed for longer than that
// share of a step: from 8 ranks on (a rank's step at N = 262 144 is ~1 ms there; at 2-4 ranks it measured
// neutral to -2 %, profiles/history/r01_late_items_ab.log).  nb_params.sym_late_us > 0 forces it for any world size,
// < 0 disables it.
static uint32_t late_units_for(const nb_params &p, bool fp64, int cus, uint32_t world)
{
    const double us = p.sym_late_us > 0.0f ? (double)p.sym_late_us : p.sym_late_us < 0.0f ? 0.0 : (world >= 8 ? 40.0 : 0.0);
    if (!(us > 0.0)) return 0;
    return (uint32_t)(us * (fp64 ? 14.0 : 35.0) * (double)cus / 256.0);
}

// Chunk PAIRS (sym_chunks2: two travelling particles per lane) pay from ~65 536 bodies on (-2 ... -3 % at 131 072 - 262 144,
// neutral at 65 536; below that the coarser items and the lower occupancy — 146-158 VGPRs, 3 waves per SIMD — cost more
// than the saved rotations: profiles/history/r03_chunk_pairs_sweep.log).  fp32 2-D only.  nb_params.sym_chunk_pairs = 1 / -1 forces it.
// Rank-independent (n and parameters only): it shapes the plan every rank must agree on.
static bool want_pairs(const nb_params &p, size_t n)
{
    if (p.precision == NB_FP64) return false;
    if (p.sym_chunk_pairs) return p.sym_chunk_pairs > 0;
    return n >= 65536;                           // 2-D and 3-D (3-D with individual masses keeps the single-chunk kernel: sym_uses_pairs)
}

// Whether the symmetric launch runs the chunk-pair kernel (any plan, even chunk counts included, runs on either kernel).
// 2-D: not with MM_SCALED.  3-D: chunk pairs pay with equal masses only (-1 ... -3 %); with individual masses the pair body
// needs 216 VGPRs (2 waves per SIMD) and loses 4 % (profiles/history/r03_chunk_pairs_3d.log): that case keeps the
// single-chunk sweep unless nb_params.sym_chunk_pairs = 1 forces it.
static bool sym_uses_pairs(const nb_sim *s)
{
    if (!s->sym_pairs) return false;
    return s->dims3 ? s->uniform_mass || s->p.sym_chunk_pairs > 0 : !s->mass_scaled;
}

static SymTuning tuning_of(const nb_params &p, bool fp64, int cus, uint32_t world, bool sharded, size_t n)
{
    SymTuning t;
    t.forced_L = p.sym_chunks_per_item > 0 ? (uint32_t)p.sym_chunks_per_item : 0u;
    t.late_units = sharded ? late_units_for(p, fp64, cus, world) : 0u;
    t.wg_per_cu = sharded ? 24u : 0u;             // reduce-scatter protocol: two launches per step (nb_plan.cpp)
    t.late_chunks = fp64 ? 1u : 2u;
    t.even_chunks = want_pairs(p, n);            // the kernel sweeps chunk pairs: even chunk counts
    t.sb = sym_tile_of(p, n);
    t.guided_tail = !(p.flags & NB_FLAG_NO_GUIDED_TAIL);
    if (p.sym_tail[0] > 0.0f || p.sym_tail[1] > 0.0f || p.sym_tail[2] > 0.0f)
        { for (int k = 0; k < 3; ++k) t.tail_at[k] = (double)p.sym_tail[k]; t.tail_given = true; }
    return t;
}

static void fill_sym_info(const SymPlan &pl, uint32_t n, uint32_t world, int cus, size_t esz, bool enabled, nb_sym_info *out)
{
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out);
    out->struct_size = sz;
    out->enabled = enabled ? 1 : 0;
    out->chunks_per_item = pl.L;
    out->items = (uint32_t)pl.items.size();
    out->items_local = pl.n_local; out->items_cross = pl.n_cross; out->items_late = pl.n_late;
    out->tiles = pl.tiles;
    out->rows_s = pl.rowbase.empty() ? 0u : pl.rowbase[pl.tiles];
    out->segments = (uint32_t)pl.segs.size();
    out->cus = (uint32_t)cus;
    out->units_local = pl.units_local; out->units_cross = pl.units_cross; out->units_late = pl.units_late;
    sym_units(n, world, nullptr, &out->cross_units_total, pl.sb);
    out->slab_s_bytes = (uint64_t)out->rows_s * pl.sb * esz;
    out->tile_particles = pl.sb;
    out->slab_r_bytes = pl.slab_r_elems * esz;
    out->coverage_entries = pl.cov_main.size() + pl.cov_late.size();
}

#ifdef NB_TEST_HOOKS   /* include/nbody_debug.h: test build only */
// CPU-testable view of the planner (no device call).
extern "C" int nb_debug_sym_plan(size_t n, int cus, int rank, int world, const nb_params *tuning,
                                 nb_sym_item *items_out, size_t cap, nb_sym_info *info)
{
    static_assert(sizeof(nb_sym_item) == sizeof(SymItem) && offsetof(nb_sym_item, r_base) == offsetof(SymItem, r_base) &&
                  offsetof(nb_sym_item, group) == offsetof(SymItem, group), "nb_sym_item mirrors SymItem");
    if (n == 0 || n > 0x7fffff00u || cus < 1 || world < 1 || rank < 0 || rank >= world ||
        (world > 1 && (n % ((size_t)world * SYM_SB)) != 0)) return nb_fail(NB_EINVAL, "nb_debug_sym_plan: bad arguments");
    if (tuning && tuning->struct_size != sizeof(nb_params)) return nb_fail(NB_EINVAL, "nb_debug_sym_plan: tuning->struct_size");
    if (info && info->struct_size != sizeof(nb_sym_info)) return nb_fail(NB_EINVAL, "nb_debug_sym_plan: info->struct_size");
    nb_params p;
    if (tuning) p = *tuning; else nb_params_default(&p);
    p.shard_rank = rank; p.shard_world = world;        // what a handle of this (rank, world) would carry: selects the tile size too
    const bool fp64 = p.precision == NB_FP64;
    SymPlan pl;
    build_sym_plan((uint32_t)n, (uint32_t)cus, (uint32_t)rank, (uint32_t)world, tuning_of(p, fp64, cus, (uint32_t)world, world > 1, n), pl);
    if (info) fill_sym_info(pl, (uint32_t)n, (uint32_t)world, cus, fp64 ? 16 : 8, true, info);
    if (items_out) memcpy(items_out, pl.items.data(), (pl.items.size() < cap ? pl.items.size() : cap) * sizeof(SymItem));
    return NB_OK;
}
#endif

// ---------------------------------------------------------------------------
// host memory
// ---------------------------------------------------------------------------
// The copy engine is only ever pointed at host memory this library KNOWS to be page-locked over the whole transfer:
// its own buffers (hipHostMalloc) and the ranges in the registry below — whole pages registered through
// nb_host_register, or blocks handed out by nb_host_alloc.  Everything else (caller arrays, std::vector storage,
// numpy arrays) moves through the handle's page-locked bounce buffer in pipelined chunks.
// Why so strict: hipHostRegister / the runtime's own pinning of pageable copy sources work on whole
// PAGES; a malloc'ed array shares its first and last page with whatever the heap put next to it, and a registration
// that outlives the array (a std::vector that reallocated) keeps pinning pages that now belong to someone else.
// Round 2 saw one process abort inside nb_upload right after nb_host_register of an unaligned numpy array.  CAUSE
// UNKNOWN: no log of that run exists, and none of the nine deterministic constructions of round 3's pin probe (shared
// pages, overlapping registrations, freed-while-registered memory reused at the same address ...) aborts on this
// runtime (profiles/history/r03_pin_probe.log).  The rules above are therefore a DEFENSIVE change, not the fix of a known bug.
struct PinnedRange { uintptr_t lo, hi; bool owned; };
static std::mutex g_pin_mutex;
static std::vector<PinnedRange> g_pinned;

static bool pinned_covers(const void *p, size_t bytes)
{
    const uintptr_t a = (uintptr_t)p, b = a + bytes;
    std::lock_guard<std::mutex> lock(g_pin_mutex);
    for (const PinnedRange &r : g_pinned)
        if (a >= r.lo && b <= r.hi && b >= a) return true;
    return false;
}

static size_t host_page_size()
{
    const long ps = sysconf(_SC_PAGESIZE);
    return ps > 0 ? (size_t)ps : 4096;
}

constexpr size_t BOUNCE_SLOTS = 4;
constexpr size_t BOUNCE_SLOT_BYTES = (size_t)2 << 20;       // 4 x 2 MiB: a DMA, a host memcpy and two slots of slack in flight
constexpr size_t BOUNCE_BYTES = BOUNCE_SLOTS * BOUNCE_SLOT_BYTES;
#ifndef NB_SMALL_SYNC_BYTES
#define NB_SMALL_SYNC_BYTES ((size_t)4 << 20)           // (A/B builds: -DNB_SMALL_SYNC_BYTES=0 keeps the copy-engine path for every size)
#endif
constexpr size_t SMALL_SYNC_BYTES = NB_SMALL_SYNC_BYTES;   // nb_sync: below this the pack kernel writes the host staging buffer itself (no DMA)

static int ensure_bounce(nb_sim *s)
{
    if (!s->bounce) HIPCHK(s->pool.alloc_pinned(s->bounce, BOUNCE_BYTES));
    for (size_t k = 0; k < BOUNCE_SLOTS; ++k)
        if (!s->ev_bounce[k]) HIPCHK(hipEventCreateWithFlags(&s->ev_bounce[k], hipEventDisableTiming));
    return NB_OK;
}

// Host -> device on `st`; returns when the data has left `src` (the caller may free it).  Pageable sources are
// copied slot by slot into the bounce buffer; slot k is reused only after its DMA (event) is complete, so the
// host memcpy of chunk c + 1 overlaps the DMA of chunk c.
static int copy_h2d(nb_sim *s, void *dst, const void *src, size_t bytes)
{
    if (bytes == 0) return NB_OK;
    if (pinned_covers(src, bytes)) {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        return NB_OK;
    }
    { const int rc = ensure_bounce(s); if (rc) return rc; }
    size_t c = 0;
    for (size_t off = 0; off < bytes; off += BOUNCE_SLOT_BYTES, ++c) {
        const size_t k = c % BOUNCE_SLOTS, len = bytes - off < BOUNCE_SLOT_BYTES ? bytes - off : BOUNCE_SLOT_BYTES;
        char *slot = (char *)s->bounce + k * BOUNCE_SLOT_BYTES;
        if (c >= BOUNCE_SLOTS) HIPCHK(hipEventSynchronize(s->ev_bounce[k]));
        memcpy(slot, (const char *)src + off, len);
        HIPCHK(hipMemcpyAsync((char *)dst + off, slot, len, hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipEventRecord(s->ev_bounce[k], s->stream));
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    return NB_OK;
}

// Device -> host on `st` (ordered after the work enqueued there), blocking.  Pageable destinations: all chunk DMAs
// are enqueued at once into the slots of `stage` (page-locked, >= bytes, or the bounce ring when stage is NULL) and
// the host copies chunk c out while chunk c + 1 is still in flight.
static int copy_d2h(nb_sim *s, void *dst, const void *src, size_t bytes, hipStream_t st = nullptr, void *stage = nullptr)
{
    if (bytes == 0) return NB_OK;
    if (!st) st = s->stream;
    if (pinned_covers(dst, bytes)) {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return NB_OK;
    }
    { const int rc = ensure_bounce(s); if (rc) return rc; }
    if (stage) {
        // whole transfer staged: BOUNCE_SLOTS equal pieces, one event each — one piece where the transfer is so short (<= 1 MiB: the
        // positions of a small system, nb_sync_positions) that three more DMA launches and events cost more than the overlap buys
        const size_t pieces = bytes <= ((size_t)1 << 20) ? 1 : BOUNCE_SLOTS;
        const size_t piece = ((bytes + pieces - 1) / pieces + 63) & ~(size_t)63;
        size_t k = 0;
        for (size_t off = 0; off < bytes; off += piece, ++k) {
            const size_t len = bytes - off < piece ? bytes - off : piece;
            HIPCHK(hipMemcpyAsync((char *)stage + off, (const char *)src + off, len, hipMemcpyDeviceToHost, st));
            HIPCHK(hipEventRecord(s->ev_bounce[k], st));
        }
        // Copy-out on the calling thread, piece k as soon as its DMA has landed (the copy of piece k overlaps the DMA of piece k + 1).
        // Round 4 tried helper threads for pieces 1 .. 3 (9.68 -> 9.31 ms per frame of the reference caller's loop at N = 262 144):
        // dropped — after threads that had touched HIP exited, RCCL's ncclCommInitAll failed in the same process ("unhandled cuda
        // error", tests/test_host_gpu.py, twice in two runs); a caller that wants the 0.35 ms keeps `bodies` in nb_host_alloc memory
        // (direct DMA) or uses the pipelined snapshot.
        k = 0;
        for (size_t off = 0; off < bytes; off += piece, ++k) {
            const size_t len = bytes - off < piece ? bytes - off : piece;
            HIPCHK(hipEventSynchronize(s->ev_bounce[k]));
            memcpy((char *)dst + off, (const char *)stage + off, len);
        }
        return NB_OK;
    }
    size_t issued = 0, done = 0;
    const size_t chunks = (bytes + BOUNCE_SLOT_BYTES - 1) / BOUNCE_SLOT_BYTES;
    while (done < chunks) {
        while (issued < chunks && issued < done + BOUNCE_SLOTS) {
            const size_t off = issued * BOUNCE_SLOT_BYTES, len = bytes - off < BOUNCE_SLOT_BYTES ? bytes - off : BOUNCE_SLOT_BYTES;
            const size_t k = issued % BOUNCE_SLOTS;
            HIPCHK(hipMemcpyAsync((char *)s->bounce + k * BOUNCE_SLOT_BYTES, (const char *)src + off, len, hipMemcpyDeviceToHost, st));
            HIPCHK(hipEventRecord(s->ev_bounce[k], st));
            ++issued;
        }
        const size_t off = done * BOUNCE_SLOT_BYTES, len = bytes - off < BOUNCE_SLOT_BYTES ? bytes - off : BOUNCE_SLOT_BYTES;
        const size_t k = done % BOUNCE_SLOTS;
        HIPCHK(hipEventSynchronize(s->ev_bounce[k]));
        memcpy((char *)dst + off, (const char *)s->bounce + k * BOUNCE_SLOT_BYTES, len);
        ++done;
    }
    return NB_OK;
}

static int plan_sym(nb_sim *s)
{
    const uint32_t n = (uint32_t)s->n;
    const bool sharded = s->path == StepPath::SYM_SHARDED, split = s->path != StepPath::SYM;
    const uint32_t world = split ? (uint32_t)s->p.shard_world : 1u;
    const uint32_t rank = split ? (uint32_t)s->p.shard_rank : 0u;
    SymPlan pl;
    build_sym_plan(n, (uint32_t)s->cus, rank, world, tuning_of(s->p, s->fp64, s->cus, world, sharded, s->n), pl);   // late items: sharded only
    s->sym_pairs = want_pairs(s->p, s->n);
    const uint32_t tiles = pl.tiles, row = pl.rowbase[tiles];
    s->sym_info.struct_size = (uint32_t)sizeof(nb_sym_info);
    fill_sym_info(pl, n, world, s->cus, s->esz, true, &s->sym_info);
    s->sym_items_local = pl.n_local; s->sym_items_cross = pl.n_cross; s->sym_items_late = pl.n_late;
    s->sym_items = (uint32_t)pl.items.size(); s->sym_tiles = tiles; s->sym_rows = row; s->sym_L = pl.L;
    s->sym_sb = pl.sb; s->sym_sb_shift = pl.sb == SYM_SB_WS ? 9u : 11u;
    // row bounds for the gathers: [lo | mid | hi] = rowbase[0..tiles), rowmid[0..tiles), rowbase[1..tiles]
    std::vector<uint32_t> bounds(3 * (size_t)tiles);
    for (uint32_t g = 0; g < tiles; ++g) { bounds[g] = pl.rowbase[g]; bounds[tiles + g] = pl.rowmid[g]; bounds[2 * (size_t)tiles + g] = pl.rowbase[g + 1]; }
    // coverage lists of the main and the late gather: [begin_main (tiles + 1) | begin_late (tiles + 1)], entries of both back to back
    std::vector<uint32_t> cbegin(pl.cov_main_begin);
    cbegin.insert(cbegin.end(), pl.cov_late_begin.begin(), pl.cov_late_begin.end());
    std::vector<SymCov> cov(pl.cov_main);
    cov.insert(cov.end(), pl.cov_late.begin(), pl.cov_late.end());
    s->sym_cov_late_off = (uint32_t)pl.cov_main.size();
    HIPCHK(s->pool.alloc(s->sym_items_dev, pl.items.size()));
    HIPCHK(s->pool.alloc(s->sym_rowbase_dev, bounds.size()));
    HIPCHK(s->pool.alloc(s->sym_cov_begin_dev, cbegin.size()));
    HIPCHK(s->pool.alloc(s->sym_cov_dev, cov.size() ? cov.size() : 1));
    HIPCHK(s->pool.alloc(s->sym_slab_s, (size_t)(row ? row : 1) * pl.sb * s->esz));
    HIPCHK(s->pool.alloc(s->sym_slab_r, (size_t)(pl.slab_r_elems ? pl.slab_r_elems : 1) * s->esz));
    int rc;
    if ((rc = copy_h2d(s, s->sym_items_dev, pl.items.data(), pl.items.size() * sizeof(SymItem)))) return rc;
    if ((rc = copy_h2d(s, s->sym_rowbase_dev, bounds.data(), bounds.size() * sizeof(uint32_t)))) return rc;
    if ((rc = copy_h2d(s, s->sym_cov_begin_dev, cbegin.data(), cbegin.size() * sizeof(uint32_t)))) return rc;
    if ((rc = copy_h2d(s, s->sym_cov_dev, cov.data(), cov.size() * sizeof(SymCov)))) return rc;
    HIPCHK(s->pool.alloc(s->sym_ticket, 3 * 128 / sizeof(uint32_t)));
    HIPCHK(hipMemsetAsync(s->sym_ticket, 0, 3 * 128, s->stream));
    // Side stream for the local items when they are about one wave of workgroups (P = 8 at N = 262 144: 615 items
    // on 512 resident slots, 150 us where 128 us of work is due): run concurrently, the cross items fill the CUs
    // the last local workgroups leave idle (-1.7 % step time; with two LONG launches sharing the chip, P = 2, the
    // same trick costs 4 % — profiles/history/r01_aux_stream_ab.log — hence the bound).  nb_params.sym_aux_stream = 1 / -1 forces it.
    s->aux_local = sharded && (s->p.sym_aux_stream ? s->p.sym_aux_stream > 0 : s->sym_items_local <= 4u * (uint32_t)s->cus);
    if (s->aux_local || s->sym_items_late) {         // the late items always run on the side stream
        HIPCHK(hipStreamCreateWithFlags(&s->aux, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&s->ev_late, hipEventDisableTiming));
    }
    if (split) {
        if (s->p.acc_buffers[0]) { s->acc_full = s->p.acc_buffers[0]; s->acc_owned = s->p.acc_buffers[1]; s->own_acc = false; }
        else {
            HIPCHK(s->pool.alloc(s->acc_full, (size_t)n * s->esz));
            if (sharded) HIPCHK(s->pool.alloc(s->acc_owned, s->i_count * s->esz));
        }
    }
    return NB_OK;
}

static void free_all(nb_sim *s)
{
    if (!s) return;
    (void)hipSetDevice(s->dev);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (auto &e : s->ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (auto &e : s->ev_used) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    if (s->copy_stream) { (void)hipStreamSynchronize(s->copy_stream); (void)hipStreamDestroy(s->copy_stream); }
    if (s->ev_packed) (void)hipEventDestroy(s->ev_packed);
    if (s->ev_copied) (void)hipEventDestroy(s->ev_copied);
    for (hipEvent_t e : s->ev_bounce) if (e) (void)hipEventDestroy(e);
    if (s->aux) { (void)hipStreamSynchronize(s->aux); (void)hipStreamDestroy(s->aux); }
    if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    if (s->ev_join) (void)hipEventDestroy(s->ev_join);
    if (s->ev_late) (void)hipEventDestroy(s->ev_late);
    for (hipEvent_t e : s->ev_x) if (e) (void)hipEventDestroy(e);
    s->pool.release_all();           // every buffer of the handle, once its three streams have drained; the caller's pos_buffers /
                                     // acc_buffers were never in the pool
    if (s->own_stream && s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

static int launch_force(nb_sim *s, const ForceJob &j);
static int integrate_slabs(nb_sim *s, uint32_t nslabs, double dt_kick, double dt_drift, int flags);

// The MEASURED rule of the mass-scaled body (NB_FLAG_MASS_SCALING_MEASURED; opt-in since ABI 6): decided per upload FROM THE
// DATA.  The accelerations of the uploaded bodies are evaluated twice — with the per-pair mass multiplies (MM_GENERAL) and with
// the masses folded into the pair geometry (MM_SCALED) — and the scaled body is taken only if the two agree to MASS_SCALING_TOL
// of the force scale (max |a|): 2e-6, a fifth of north_star's 1e-5.  Equal-ish light masses pass (Plummer spheres at the headline
// size: 4e-7, the two bodies' ordinary rounding difference); THE REFERENCE'S OWN BODIES DO NOT (Simulation.hpp:347-603: 4.0e-5 —
// its light bodies sit 1e3 ... 1e5 from the origin with eps = 1, so sigma * x is rounded at that magnitude while close pairs
// are a unit apart) and keep MM_GENERAL; a four-decade mixture with close heavy pairs fails likewise (6e-5:
// tests/test_headline_gpu.py).  What the measure is NOT (why it is no longer the default): it is a global absolute figure at
// t = 0 — a body whose own |a| is far below max |a| can carry a larger relative error and still pass, and a system that
// passes at upload and later drifts from the origin or forms close heavy pairs is not measured again.
// Cost: two force evaluations per upload (14 ms at N = 262 144).
constexpr float MASS_SCALING_TOL = 2e-6f;
// the two evaluations and the verdict; its temporaries live in a pool of its own, released on every way out
static int measure_mass_scaling(nb_sim *s)
{
    const size_t bytes = s->i_count * s->esz;
    const uint32_t n = (uint32_t)s->i_count;
    MemPool<HipMem> tmp;
    void *saved = nullptr, *ref = nullptr;
    uint32_t *out = nullptr, *host = nullptr;
    HIPCHK(tmp.alloc(saved, bytes));
    HIPCHK(tmp.alloc(ref, bytes));
    HIPCHK(tmp.alloc(out, 2));
    HIPCHK(hipMemcpyAsync(saved, s->acc, bytes, hipMemcpyDeviceToDevice, s->stream));      // the uploaded acc field survives the check
    HIPCHK(hipMemsetAsync(out, 0, 2 * sizeof(uint32_t), s->stream));
    int r;
    s->mass_scaled = false;
    if ((r = launch_force(s, s->job_all)) || (r = integrate_slabs(s, s->slabs_all, 0.0, 0.0, 0))) return r;
    HIPCHK(hipMemcpyAsync(ref, s->acc, bytes, hipMemcpyDeviceToDevice, s->stream));
    s->mass_scaled = true;
    if ((r = launch_force(s, s->job_all)) || (r = integrate_slabs(s, s->slabs_all, 0.0, 0.0, 0))) return r;
    max_deviation_f32<<<(n + BLOCK - 1) / BLOCK, BLOCK, 0, s->stream>>>((const float2 *)s->acc, (const float2 *)ref, n, out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s->acc, saved, bytes, hipMemcpyDeviceToDevice, s->stream));
    HIPCHK(tmp.alloc_pinned(host, 2));
    hipError_t e = hipMemcpyAsync(host, out, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) return nb_fail(hip_code(e), "nb_upload: mass-scaling check: %s", hipGetErrorString(e));
    float dev = 0.f, scale = 0.f;
    memcpy(&dev, &host[0], sizeof dev);
    memcpy(&scale, &host[1], sizeof scale);
    const bool comparable = dev == dev && scale == scale && scale > 0.f && scale < 3.0e38f;
    s->mass_scaling_dev = comparable ? dev / scale : HUGE_VALF;
    s->mass_scaled = comparable && dev <= MASS_SCALING_TOL * scale;
    return NB_OK;
}

static int choose_mass_scaling(nb_sim *s)
{
    const bool prof = s->prof;
    s->prof = false;                  // the check's two force launches are not the caller's: keep them out of nb_profile_read
    const int rc = measure_mass_scaling(s);
    s->prof = prof;
    if (rc) s->mass_scaled = false;
    s->acc_valid = false;
    return rc;
}

// Caller-owned device memory (params.pos_buffers / acc_buffers) or a caller's stream: whatever the caller enqueued on those
// buffers before handing them over — a fill on another stream, a collective still in flight — must be THROUGH before the
// upload writes them.  The handle's stream is non-blocking (or foreign), so nothing orders it against that work; a zero-fill
// queued on the caller's stream could land after the upload and wipe the positions (found in round 5 by the sharded host's
// start-up validation).  One device-wide fence per creation / upload; never on the step path.
static int fence_foreign_work(nb_sim *s)
{
    if (s->own_pos && s->own_acc && s->own_stream) return NB_OK;
    HIPCHK(hipDeviceSynchronize());
    return NB_OK;
}

// ---- what the query calls (nb_tree_nodes, nb_raster, nb_potentials, nb_neighbors, nb_groups, nb_group_catalog, nb_group_binding, nb_pair_counts,
// nb_radial_profiles, nb_field) share ----
static int snapshot_wait(nb_sim *s);

// The opening of a query call, behind its argument checks: no split step in flight, the device bound, (nb_potentials: the staging
// buffer of nb_sync back from a pipelined snapshot,) and step_check, which synchronises: a pending once-only report leaves through
// here with nothing written.
static int query_enter(nb_sim *s, const char *name, bool wait_snapshot = false)
{
    if (s->in_step) return nb_fail(NB_ESTATE, "%s: a split step is in flight", name);
    if (bind(s)) return NB_EHIP;
    if (wait_snapshot && snapshot_wait(s)) return nb_last_error_code();
    return step_check(s);
}

static int check_radius(const char *name, float radius, float *r2)
{
    if (!std::isfinite(radius) || !(radius > 0.0f)) return nb_fail(NB_EINVAL, "%s: radius must be finite and > 0 (got %g)", name, (double)radius);
    *r2 = radius * radius;                                        // one fp32 rounding: the kernel's operand
    if (!std::isfinite(*r2) || *r2 == 0.0f)
        return nb_fail(NB_EINVAL, "%s: radius * radius must be finite and > 0 in float (radius %g gives %g)", name, (double)radius, (double)*r2);
    return NB_OK;
}

// Bytes of the query staging buffer a plane of `bytes` for `dst` asks for: none where there is no plane or the copy engine reaches dst.
static size_t stage_need(const void *dst, size_t bytes) { return dst && !pinned_covers(dst, bytes) ? bytes : 0; }

// Grow the query staging buffer to `bytes`, before the call's kernels are launched.  Nothing is in flight through it: copy_d2h blocks.
static int query_stage(nb_sim *s, size_t bytes)
{
    HIPCHK(s->pool.regrow_pinned(s->qstage_cap, bytes, s->qstage));
    return NB_OK;
}

static int copy_plane(nb_sim *s, void *dst, const void *src, size_t bytes) { return copy_d2h(s, dst, src, bytes, s->stream, s->qstage); }

// ---- the subsystems' host code (it moves its data with copy_h2d / copy_d2h above) ----
#include "nb_collide_host.hip.h"
#include "nb_tree_host.hip.h"
#include "nb_raster_host.hip.h"
#include "nb_potential_host.hip.h"
#include "nb_neighbors_host.hip.h"
#include "nb_groups_host.hip.h"
#include "nb_group_catalog_host.hip.h"
#include "nb_group_binding_host.hip.h"
#include "nb_pair_counts_host.hip.h"
#include "nb_profiles_host.hip.h"
#include "nb_field_host.hip.h"
#include "nb_hermite_host.hip.h"
#include "nb_order_host.hip.h"

// what every synchronising call reports once: a collision step over capacity, a failed tree build
static int step_check(nb_sim *s)
{
    const int rc = collide_check(s);
    return rc ? rc : tree_check(s);
}

static int do_upload(nb_sim *s, const nb_body *in)
{
    { const int rc = fence_foreign_work(s); if (rc) return rc; }
    // Equal masses (the synthetic Plummer workload, most N-body ICs) let the force kernel hoist the
    // per-pair mass multiply: 8 instead of 9 packed ops per two pairs.  NB_FLAG_NO_UNIFORM_MASS disables it.
    // (a tree handle has none of the direct-sum specialisations: the flags that select them are ignored, include/nbody.h)
    // (nor has a Hermite handle: its one pair kernel takes individual masses)
    s->uniform_mass = s->n > 0 && !s->tree && !hermite(s) && !(s->p.flags & NB_FLAG_NO_UNIFORM_MASS) && s->p.sum_order == NB_SUM_TILED;
    for (size_t i = 1; s->uniform_mass && i < s->n; ++i)
        if (memcmp(&in[i].mass, &in[0].mass, sizeof(float)) != 0) s->uniform_mass = false;
    s->um_mass = in[0].mass;
    // Mass scaling: individual masses folded into the pair geometry (MM_SCALED: 11 + 2 instead of 12 + 2 instructions per body of
    // the symmetric kernel, 8 + 2 instead of 9 + 2 in the one-sided one).  REPRESENTABLE when every mass is positive and
    // sigma = m^(-1/2), sigma * (the kernels' padding coordinate 1e18) and g^3 <= (sqrt(m_max) / eps)^3 all stay finite floats
    // with room to spare; exact rsqrt only (the Quake mode keeps the reference's arithmetic).  Whether it is also HARMLESS — its
    // displacement is rounded once more, 6e-8 |x_j| / |d| per pair force, which heavy close pairs turn into several 1e-5 of the
    // force scale — depends on the data, so it is the CALLER's decision (ABI 6: off unless asked for — the same pair arithmetic on
    // one GPU and on N, at t = 0 and later): NB_FLAG_MASS_SCALING takes it wherever representable, NB_FLAG_MASS_SCALING_MEASURED
    // lets choose_mass_scaling() above measure it on the uploaded bodies (unsharded handles), NB_FLAG_NO_MASS_SCALING overrides both.
    s->mass_scaled = false;
    s->mass_scaling_dev = -1.0f;
    bool scalable = false;
    if (!s->tree && !hermite(s) && !s->uniform_mass && s->p.sum_order == NB_SUM_TILED && !needs_guard(s) && !s->fp64 && !s->dims3 &&
        s->p.rsqrt_mode == NB_RSQRT_EXACT && (s->p.flags & (NB_FLAG_MASS_SCALING | NB_FLAG_MASS_SCALING_MEASURED)) && !(s->p.flags & NB_FLAG_NO_MASS_SCALING)) {
        double mmin = HUGE_VAL, mmax = 0.0;
        bool finite = true;
        for (size_t i = 0; i < s->n; ++i) {
            const double m = (double)in[i].mass;
            if (!(m == m) || m > 3.0e38) finite = false;
            if (m < mmin) mmin = m;
            if (m > mmax) mmax = m;
        }
        const double eps = (double)s->p.eps;
        scalable = finite && mmin >= 1e-30 && std::pow(mmax, 1.5) / (eps * eps * eps) <= 1e36;
    }
    const bool forced_scaling = scalable && (s->p.flags & NB_FLAG_MASS_SCALING);
    const bool auto_scaling = scalable && !forced_scaling && (s->p.flags & NB_FLAG_MASS_SCALING_MEASURED) && s->i_count == s->n &&
                             s->path != StepPath::SYM_SHARDED && s->path != StepPath::SYM_REPLICATED;
    const bool was_uniform = s->sym_first_wave_uniform, was_scaled = s->sym_first_wave_scaled;
    { const int rc = copy_h2d(s, s->aos_dev, in, s->n * sizeof(nb_body)); if (rc) return rc; }
    const uint32_t n = (uint32_t)s->n, g = (n + BLOCK - 1) / BLOCK, ib = (uint32_t)s->i_begin, ic = (uint32_t)s->i_count;
    with_layout(s, [&](auto L) {
        using real = typename decltype(L)::real;
        using vec = typename decltype(L)::vec;
        for (int b = 0; b < 2; ++b)        // both replicas get the full initial positions
            unpack_bodies<decltype(L)><<<g, BLOCK, 0, s->stream>>>(s->aos_dev, n, (vec *)s->pos[b], (real *)s->mass, (vec *)s->vel, (vec *)s->acc,
                                                                   s->radius, ib, ic);
    });
    HIPCHK(hipGetLastError());
    if (forced_scaling || auto_scaling) {
        if (!s->sigma) HIPCHK(s->pool.alloc(s->sigma, s->n));
        mass_sigma<<<g, BLOCK, 0, s->stream>>>((const float *)s->mass, s->sigma, n);
        HIPCHK(hipGetLastError());
    }
    s->mass_scaled = forced_scaling;
    if (s->ord.on) { const int rc = order_upload(s); if (rc) return rc; }
    if (s->collide) { const int rc = collide_classify(s, in); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(s->stream));  // `in` may be pageable and freed by the caller
    s->acc_valid = false;
    s->herm.valid = false;                    // a Hermite handle evaluates (a0, j0) at the uploaded state before its next step
    if (auto_scaling) { const int rc = choose_mass_scaling(s); if (rc) return rc; }
    // the resident-slot count behind the static / dynamic item split belongs to ONE kernel instantiation (its VGPR count sets the
    // occupancy): the check above launches MM_GENERAL whatever the verdict, and a re-upload can flip uniform_mass — ask again
    if (auto_scaling || was_uniform != s->uniform_mass || was_scaled != s->mass_scaled) s->sym_first_wave = 0;
    s->sym_first_wave_uniform = s->uniform_mass;
    s->sym_first_wave_scaled = s->mass_scaled;
    return NB_OK;
}

// The composed integrators (NB_INTEGRATOR_DKD, NB_INTEGRATOR_FR4: step_composed below) by name; NULL for the other two.
static const char *composed_name(int integrator)
{
    return integrator == NB_INTEGRATOR_DKD ? "DKD" : integrator == NB_INTEGRATOR_FR4 ? "FR4" : nullptr;
}

extern "C" nb_sim *nb_create(const nb_body *init, size_t n, const nb_params *params)
{
    nb_clear_error();
    nb_params p;
    if (params) {
        if (params->struct_size != sizeof(nb_params)) {
            nb_set_error("nb_create: params->struct_size %u != %zu (use nb_params_default)", params->struct_size, sizeof(nb_params));
            return nullptr;
        }
        p = *params;
    } else nb_params_default(&p);
    if (!init || n == 0) { nb_set_error("nb_create: no bodies"); return nullptr; }
    if (n > 0x7fffff00u) { nb_set_error("nb_create: n=%zu exceeds the 32-bit index range of the kernels", n); return nullptr; }
    if (!(p.eps >= 0.0f)) { nb_set_error("nb_create: eps must be >= 0"); return nullptr; }
    if (p.precision != NB_FP32 && p.precision != NB_FP64) { nb_set_error("nb_create: bad precision %d", p.precision); return nullptr; }
    if (p.rsqrt_mode != NB_RSQRT_EXACT && p.rsqrt_mode != NB_RSQRT_QUAKE) { nb_set_error("nb_create: bad rsqrt_mode %d", p.rsqrt_mode); return nullptr; }
    if (p.sum_order != NB_SUM_TILED && p.sum_order != NB_SUM_SEQUENTIAL) { nb_set_error("nb_create: bad sum_order %d", p.sum_order); return nullptr; }
    if (p.integrator < NB_INTEGRATOR_KICK_DRIFT || (p.integrator > NB_INTEGRATOR_FR4 && p.integrator != NB_INTEGRATOR_HERMITE4)) { nb_set_error("nb_create: bad integrator %d", p.integrator); return nullptr; }
    if (p.precision == NB_FP64 && (p.rsqrt_mode == NB_RSQRT_QUAKE || p.sum_order == NB_SUM_SEQUENTIAL)) {
        nb_set_error("nb_create: quake rsqrt / sequential order are fp32 (reference arithmetic) modes");
        return nullptr;
    }
    if (p.flags & ~NB_FLAGS_KNOWN) { nb_set_error("nb_create: unknown bits in flags 0x%x", (unsigned)p.flags); return nullptr; }
    if (p.extras & ~(NB_EXTRA_VCLAMP | NB_EXTRA_BOUNDARY | NB_EXTRA_COLLIDE)) { nb_set_error("nb_create: unknown bits in extras 0x%x", (unsigned)p.extras); return nullptr; }
    if (const char *name = composed_name(p.integrator)) {
        // the composed integrators (step_composed): whole unsharded systems, and only extras that their kicks can carry
        const char *why = p.shard_world > 1 ? "shard_world > 1" : (p.i_count != 0 && p.i_count < n) ? "i_count < n"
                        : (p.flags & NB_FLAG_SHARD_SINGLE) ? "NB_FLAG_SHARD_SINGLE" : (p.flags & NB_FLAG_SHARD_ALLREDUCE) ? "NB_FLAG_SHARD_ALLREDUCE"
                        : (p.extras & NB_EXTRA_COLLIDE) ? "NB_EXTRA_COLLIDE (collisions need the kick-drift integrator)"
                        : (p.extras && p.integrator == NB_INTEGRATOR_FR4) ? "extras (its middle kick is negative: the velocity clamp and the damped boundary "
                                                                            "are not maps that can be run backwards)" : nullptr;
        if (why) { nb_set_error("nb_create: the %s integrator steps whole unsharded handles; not supported with %s", name, why); return nullptr; }
    }
    if (p.integrator == NB_INTEGRATOR_HERMITE4) {
        // the Hermite integrator (step_hermite, nb_hermite_host.hip.h): whole unsharded direct-sum handles, tiled sum, hardware rsqrt, no extras
        const char *why = p.force == NB_FORCE_TREE ? "NB_FORCE_TREE (a walk has no jerk)" : p.shard_world > 1 ? "shard_world > 1"
                        : (p.i_count != 0 && p.i_count < n) ? "i_count < n"
                        : (p.flags & NB_FLAG_SHARD_SINGLE) ? "NB_FLAG_SHARD_SINGLE" : (p.flags & NB_FLAG_SHARD_ALLREDUCE) ? "NB_FLAG_SHARD_ALLREDUCE"
                        : p.extras ? "extras (the velocity clamp, the damped boundary and the collisions are not differentiable: there is no jerk of them)"
                        : p.sum_order == NB_SUM_SEQUENTIAL ? "NB_SUM_SEQUENTIAL"
                        : p.rsqrt_mode == NB_RSQRT_QUAKE ? "NB_RSQRT_QUAKE (the reference's arithmetic has no Hermite to match)" : nullptr;
        if (why) { nb_set_error("nb_create: the HERMITE4 integrator steps whole unsharded direct-sum handles; not supported with %s", why); return nullptr; }
    }
    if (p.extras & NB_EXTRA_COLLIDE) {
        const char *why = p.dims == 3 ? "dims = 3" : p.integrator != NB_INTEGRATOR_KICK_DRIFT ? "the KDK integrator"
                        : p.shard_world > 1 ? "shard_world > 1" : (p.i_count != 0 && p.i_count < n) ? "i_count < n" : (p.flags & NB_FLAG_SHARD_SINGLE) ? "NB_FLAG_SHARD_SINGLE" : nullptr;
        if (why) {
            nb_set_error("nb_create: collisions (NB_EXTRA_COLLIDE) need an unsharded 2-D kick-drift handle; not supported with %s", why);
            return nullptr;
        }
    }
    if (p.force != NB_FORCE_DIRECT && p.force != NB_FORCE_TREE) { nb_set_error("nb_create: bad force %d", p.force); return nullptr; }
    if (!(p.theta >= 0.0f) || !std::isfinite(p.theta)) { nb_set_error("nb_create: theta must be >= 0 and finite"); return nullptr; }
    // flags of the convergent Barnes-Hut force: each needs NB_FORCE_TREE with NB_FLAG_TREE_LEAVES (checked in this order)
    static const struct { int32_t flag; const char *name, *sentence; } tree_flags[3] = {
        {NB_FLAG_TREE_RELATIVE, "NB_FLAG_TREE_RELATIVE",
         "the flag adds an acceleration-relative opening test to the walks of the convergent Barnes-Hut force (NB_FORCE_TREE with NB_FLAG_TREE_LEAVES)"},
        {NB_FLAG_TREE_ENERGY, "NB_FLAG_TREE_ENERGY",
         "the flag makes nb_energy walk the tree of the convergent Barnes-Hut force (NB_FORCE_TREE with NB_FLAG_TREE_LEAVES; without the leaves "
         "a walk has no near field and no meaningful potential)"},
        {NB_FLAG_TREE_QUADRUPOLE, "NB_FLAG_TREE_QUADRUPOLE",
         "the flag adds the second moment of an accepted cell to the convergent Barnes-Hut force (NB_FORCE_TREE with NB_FLAG_TREE_LEAVES)"},
    };
    for (const auto &f : tree_flags)
        if ((p.flags & f.flag) && (p.force != NB_FORCE_TREE || !(p.flags & NB_FLAG_TREE_LEAVES))) {
            nb_set_error("nb_create: %s %s: %s", f.name,
                         p.force == NB_FORCE_TREE ? "without NB_FLAG_TREE_LEAVES" : (p.flags & NB_FLAG_TREE_LEAVES) ? "with NB_FORCE_DIRECT"
                                                    : "with NB_FORCE_DIRECT and without NB_FLAG_TREE_LEAVES", f.sentence);
            return nullptr;
        }
    if ((p.flags & NB_FLAG_TREE_LEAVES) && p.force != NB_FORCE_TREE) {
        nb_set_error("nb_create: NB_FLAG_TREE_LEAVES with NB_FORCE_DIRECT: the flag selects a walk of the Barnes-Hut force (NB_FORCE_TREE)");
        return nullptr;
    }
    if (p.force == NB_FORCE_TREE) {
        const char *why = p.precision == NB_FP64 ? "NB_FP64" : p.dims == 3 ? "dims = 3" : p.integrator == NB_INTEGRATOR_KDK ? "the KDK integrator"
                        : p.shard_world > 1 ? "shard_world > 1" : (p.i_count != 0 && p.i_count < n) ? "i_count < n"
                        : (p.flags & (NB_FLAG_SHARD_SINGLE | NB_FLAG_SHARD_ALLREDUCE)) ? "NB_FLAG_SHARD_SINGLE / NB_FLAG_SHARD_ALLREDUCE"
                        : p.sum_order != NB_SUM_TILED ? "NB_SUM_SEQUENTIAL (the walk has one order: the reference's)" : nullptr;
        if (why) {
            nb_set_error("nb_create: the Barnes-Hut force (NB_FORCE_TREE) needs an unsharded 2-D fp32 kick-drift, DKD or FR4 handle; not supported with %s", why);
            return nullptr;
        }
    }
    if (p.sym_chunks_per_item < 0 || p.sym_aux_stream < -1 || p.sym_aux_stream > 1 || p.j_slices < 0 || p.sym_chunk_pairs < -1 || p.sym_chunk_pairs > 1 ||
        (p.sym_tile != 0 && p.sym_tile != (int32_t)SYM_SB_WS && p.sym_tile != (int32_t)SYM_SB) ||
        (p.lanes_p != 0 && p.lanes_p != 1 && p.lanes_p != 2 && p.lanes_p != 4) || !(p.sym_late_us == p.sym_late_us)) {
        nb_set_error("nb_create: tuning field out of range (sym_chunks_per_item >= 0, sym_aux_stream in -1..1, lanes_p in {0,1,2,4}, j_slices >= 0, sym_tile in {0,512,2048})");
        return nullptr;
    }
    if (p.sym_tail[0] != 0.0f || p.sym_tail[1] != 0.0f || p.sym_tail[2] != 0.0f) {
        if (!(p.sym_tail[0] > 0.0f && p.sym_tail[0] <= p.sym_tail[1] && p.sym_tail[1] <= p.sym_tail[2] && p.sym_tail[2] <= 1.0f)) {
            nb_set_error("nb_create: sym_tail must be 0 < a <= b <= c <= 1 (or all 0 for the defaults)");
            return nullptr;
        }
    }
    if (p._reserved0 != 0) { nb_set_error("nb_create: params->_reserved0 must be 0 (use nb_params_default)"); return nullptr; }
    if (p.dims == 0) p.dims = 2;
    if (p.dims != 2 && p.dims != 3) { nb_set_error("nb_create: dims must be 2 or 3"); return nullptr; }
    if (p.dims == 3 && (p.sum_order != NB_SUM_TILED || p.extras != 0)) {
        nb_set_error("nb_create: dims = 3 supports the tiled sum without extras (the reference defines its sequential order and "
                     "iterate()'s clamp / boundary in the plane only)");
        return nullptr;
    }
    if (p.i_count == 0) { p.i_begin = 0; p.i_count = n; }
    if (p.i_begin + p.i_count > n) { nb_set_error("nb_create: owned block [%llu,+%llu) exceeds n=%zu", (unsigned long long)p.i_begin, (unsigned long long)p.i_count, n); return nullptr; }
    if ((p.pos_buffers[0] == nullptr) != (p.pos_buffers[1] == nullptr)) { nb_set_error("nb_create: give both pos_buffers or none"); return nullptr; }
    if (p.pos_rows != 0 && (!p.pos_buffers[0] || p.pos_rows < n)) { nb_set_error("nb_create: pos_rows describes caller-owned pos_buffers and must be >= n"); return nullptr; }
    if ((p.acc_buffers[0] == nullptr) != (p.acc_buffers[1] == nullptr)) { nb_set_error("nb_create: give both acc_buffers or none"); return nullptr; }
    if (p.shard_world < 0 || (p.shard_world > 1 && (p.shard_rank < 0 || p.shard_rank >= p.shard_world))) { nb_set_error("nb_create: bad shard_rank/shard_world %d/%d", p.shard_rank, p.shard_world); return nullptr; }

    int ndev = nb_device_count();
    if (ndev <= 0) { nb_fail(NB_ENODEVICE, "nb_create: no HIP device visible (this library has no CPU path)"); return nullptr; }
    int dev = p.device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= ndev) { nb_set_error("nb_create: device %d out of range (%d visible)", dev, ndev); return nullptr; }

    nb_sim *s = new (std::nothrow) nb_sim;
    if (!s) { nb_fail(NB_ENOMEM, "nb_create: out of host memory"); return nullptr; }
    s->p = p; s->n = n; s->i_begin = (size_t)p.i_begin; s->i_count = (size_t)p.i_count; s->dev = dev;
    s->frame = p.first_frame;
    s->fp64 = p.precision == NB_FP64;
    s->rsz = s->fp64 ? 8 : 4;
    s->dims3 = p.dims == 3;
    s->esz = (s->dims3 ? 4 : 2) * s->rsz;      // one position / velocity / acceleration / slab element: real2 or real4

    auto fail = [&](const char *what, hipError_t e) -> nb_sim * {
        free_all(s);
        (void)hipGetLastError();        // do not leave the failure sticky for the next handle's launch checks
        nb_fail(hip_code(e), "nb_create: %s: %s", what, hipGetErrorString(e));
        return nullptr;
    };
    hipError_t e;
    if ((e = hipSetDevice(dev)) != hipSuccess) return fail("hipSetDevice", e);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, dev)) != hipSuccess) return fail("hipGetDeviceProperties", e);
    s->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (p.stream) { s->stream = (hipStream_t)p.stream; s->own_stream = false; }
    else { if ((e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e); s->own_stream = true; }

    s->path = step_path_of(s);
    plan(s);
    const size_t r2 = s->esz;
    if (p.pos_buffers[0]) { s->pos[0] = p.pos_buffers[0]; s->pos[1] = p.pos_buffers[1]; s->own_pos = false; s->pos_rows = p.pos_rows ? (size_t)p.pos_rows : n; }
    else {
        // a sharded handle's replicas hold world * ceil(n / world) rows: an all-gather over ragged blocks moves equal counts
        const size_t w = p.shard_world > 1 ? (size_t)p.shard_world : 1;
        s->pos_rows = w * ((n + w - 1) / w);
        if ((e = s->pool.alloc(s->pos[0], s->pos_rows * r2)) != hipSuccess) return fail("allocating pos", e);
        if ((e = s->pool.alloc(s->pos[1], s->pos_rows * r2)) != hipSuccess) return fail("allocating pos", e);
        if (s->pos_rows > n) {          // the padding rows travel with the last block: keep them defined
            if ((e = hipMemsetAsync((char *)s->pos[0] + n * r2, 0, (s->pos_rows - n) * r2, s->stream)) != hipSuccess) return fail("hipMemset pos", e);
            if ((e = hipMemsetAsync((char *)s->pos[1] + n * r2, 0, (s->pos_rows - n) * r2, s->stream)) != hipSuccess) return fail("hipMemset pos", e);
        }
    }
    s->slabs_cap = s->slabs_all > s->slabs_two_phase ? s->slabs_all : s->slabs_two_phase;
    s->tree = p.force == NB_FORCE_TREE;
    s->bh.theta2 = p.theta * p.theta;
    s->bh.leaves = s->tree && (p.flags & NB_FLAG_TREE_LEAVES) != 0;
    s->bh.quad = s->bh.leaves && (p.flags & NB_FLAG_TREE_QUADRUPOLE) != 0;
    s->bh.energy = s->bh.leaves && (p.flags & NB_FLAG_TREE_ENERGY) != 0;
    s->bh.rel = s->bh.leaves && (p.flags & NB_FLAG_TREE_RELATIVE) != 0;
    if ((e = s->pool.alloc(s->mass, n * s->rsz)) != hipSuccess) return fail("allocating mass", e);
    if ((e = s->pool.alloc(s->radius, n)) != hipSuccess) return fail("allocating radius", e);
    if ((e = s->pool.alloc(s->vel, s->i_count * r2)) != hipSuccess) return fail("allocating vel", e);
    if ((e = s->pool.alloc(s->acc, s->i_count * r2)) != hipSuccess) return fail("allocating acc", e);
    // (a tree handle has no one-sided partials: its walk writes acc[] itself)
    if ((e = s->pool.alloc(s->partial, s->tree ? r2 : (size_t)s->slabs_cap * s->i_count * r2)) != hipSuccess) return fail("allocating partial", e);
    if ((e = s->pool.alloc(s->aos_dev, n)) != hipSuccess) return fail("allocating aos", e);
    s->ered_blocks = (s->i_count + BLOCK - 1) / BLOCK;
    if ((e = s->pool.alloc(s->ered_dev, (s->bh.energy ? 4 : 2) * s->ered_blocks)) != hipSuccess) return fail("allocating energy", e);

    s->collide = (p.extras & NB_EXTRA_COLLIDE) != 0;
    s->ord.on = order_wanted(s);
    if ((symmetric(s) && plan_sym(s) != NB_OK) || (s->ord.on && order_alloc(s) != NB_OK) || (s->collide && collide_alloc(s) != NB_OK) ||
        (s->tree && tree_alloc(s) != NB_OK) || (hermite(s) && hermite_alloc(s) != NB_OK) || do_upload(s, init) != NB_OK) { free_all(s); (void)hipGetLastError(); return nullptr; }     // (nb_fail has said why)
    return s;
}

extern "C" void nb_destroy(nb_sim *s) { free_all(s); }

extern "C" int nb_upload(nb_sim *s, const nb_body *in)
{
    if (!s || !in) return nb_fail(NB_EINVAL, "nb_upload: NULL argument");
    if (bind(s)) return NB_EHIP;
    if (snapshot_wait(s)) return nb_last_error_code();         // the AoS staging array may still feed a pipelined snapshot
    return do_upload(s, in);
}

// ---------------------------------------------------------------------------
// profiling events
// ---------------------------------------------------------------------------
static int prof_begin(nb_sim *s, std::pair<hipEvent_t, hipEvent_t> *pr, hipStream_t st)
{
    if (s->ev_pool.empty()) {
        hipEvent_t a, b;
        HIPCHK(hipEventCreate(&a));
        HIPCHK(hipEventCreate(&b));
        s->ev_pool.push_back({a, b});
    }
    *pr = s->ev_pool.back();
    s->ev_pool.pop_back();
    HIPCHK(hipEventRecord(pr->first, st ? st : s->stream));
    return NB_OK;
}

static int prof_end(nb_sim *s, const std::pair<hipEvent_t, hipEvent_t> &pr, hipStream_t st, uint32_t passes)
{
    HIPCHK(hipEventRecord(pr.second, st ? st : s->stream));
    s->ev_used.push_back(pr);
    s->ev_weight.push_back(passes);
    return NB_OK;
}

static int prof_collect(nb_sim *s)
{
    for (size_t k = 0; k < s->ev_used.size(); ++k) {
        auto &pr = s->ev_used[k];
        HIPCHK(hipEventSynchronize(pr.second));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, pr.first, pr.second));
        s->prof_ms += ms;
        s->prof_launches += s->ev_weight[k];          // a pipeline launch counts as the force passes (steps) it holds
        s->ev_pool.push_back(pr);
    }
    s->ev_used.clear();
    s->ev_weight.clear();
    return NB_OK;
}

// ---------------------------------------------------------------------------
// force launch
// ---------------------------------------------------------------------------
// Launch of one symmetric force kernel over `count` items, with its dynamic work items (sym_item_index, nb_kernels.hip.h): past
// the first resident wave — the resident slots of THIS kernel — a workgroup draws its item when it starts.  One counter per launch
// kind of the handle (`slot`), monotonic: `tb` = what the launches of that kind have drawn so far.
template <typename... KArgs, typename... Args>
static int launch_sym_kernel(nb_sim *s, void (*kernel)(KArgs...), uint32_t count, uint32_t slot, hipStream_t st, Args... args)
{
    uint32_t *tk = nullptr;
    uint32_t fw = 0, tb = 0, drawn = 0;      // drawn: tickets this launch will take — committed to the host's record only once the launch is known to be enqueued
    if (s->sym_ticket != nullptr && !(s->p.flags & NB_FLAG_STATIC_ITEMS)) {
        if (!s->sym_first_wave) {
            int per_cu = 0;
            HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, BLOCK, 0));
            s->sym_first_wave = (uint32_t)(per_cu > 0 ? per_cu : 1) * (uint32_t)s->cus;
        }
        fw = s->sym_first_wave < count ? s->sym_first_wave : count;
        tk = s->sym_ticket + slot * 32u; tb = s->sym_ticket_base[slot];
        drawn = count - fw;
    }
    kernel<<<count, BLOCK, 0, st>>>(args..., tk, fw, tb);
    // The host's record of the tickets advances only with a launch that was accepted: if this one was refused, the device
    // counter did not move either, but a kernel of an EARLIER launch may still be drawing — nothing sound can follow on
    // this handle, so it is refused from here on (nb_step_begin) instead of indexing items[] with a base that may be off.
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        s->broken = true;
        return nb_fail(hip_code(e), "launch of the symmetric force kernel failed: %s; the handle is unusable from here on", hipGetErrorString(e));
    }
    s->sym_ticket_base[slot] += drawn;
    return NB_OK;
}

// Symmetric kernel over items [first, first + count) of this handle (HIP events around the launch
// when profiling).
static int launch_sym_items(nb_sim *s, uint32_t first, uint32_t count, hipStream_t st = nullptr)
{
    if (count == 0) return NB_OK;
    if (!st) st = s->stream;
    std::pair<hipEvent_t, hipEvent_t> pr;
    if (s->prof && prof_begin(s, &pr, st)) return NB_EHIP;
    const uint32_t n = (uint32_t)s->n;
    const SymItem *items = s->sym_items_dev + first;
    const uint32_t slot = first == 0 ? 0u : (first == s->sym_items_local ? 1u : 2u);   // the launch kind: told by where its items begin
    const bool quake = s->p.rsqrt_mode == NB_RSQRT_QUAKE, um = s->uniform_mass, pairs = sym_uses_pairs(s);
    const int rc = with_layout(s, [&](auto L) -> int {
        using real = typename decltype(L)::real;
        using vec = typename decltype(L)::vec;
        const real eps2 = (real)s->p.eps * (real)s->p.eps, umv = um ? (real)s->um_mass : (real)1;
        const vec *pos = (const vec *)sym_positions(s);     // an ordered handle: the sorted copies (nb_order_host.hip.h)
        vec *ss = (vec *)s->sym_slab_s, *sr = (vec *)s->sym_slab_r;
        // the kernels' leading arguments: (pos, mass) in fp64 (3-D reads pos.w and not `mass`), (pos, mass, sigma) in fp32 2-D, (pos) in fp32 3-D
        auto go = [&](auto kernel, auto... lead) { return launch_sym_kernel(s, kernel, count, slot, st, lead..., items, ss, sr, n, eps2, umv); };
        if constexpr (std::is_same_v<real, double>)
            return with_flags([&](auto u) { return go(force_sym_f64<decltype(L), u>, pos, (const double *)sym_masses(s)); }, um);
        else if constexpr (L.dims3)
            return with_flags([&](auto q, auto u, auto pp) { return go(force_sym3_f32<q ? RSQ_QUAKE : RSQ_EXACT, u, pp>, pos); }, quake, um, pairs);
        else
            return with_flags([&](auto q, auto pp, auto ws) {
                constexpr int RQ = q ? RSQ_QUAKE : RSQ_EXACT;
                const float *mass = (const float *)sym_masses(s), *sigma = sym_sigma(s);
                if (um) return go(force_sym_f32<RQ, MM_UNIFORM, pp, ws>, pos, mass, sigma);
                if constexpr (RQ == RSQ_EXACT && !pp)           // MM_SCALED: exact rsqrt only (decided at upload), no chunk pairs
                    if (s->mass_scaled) return go(force_sym_f32<RSQ_EXACT, MM_SCALED, false, ws>, pos, mass, sigma);
                return go(force_sym_f32<RQ, MM_GENERAL, pp, ws>, pos, mass, sigma);
            }, quake, pairs, s->sym_sb == SYM_SB_WS);
    });
    if (rc) return rc;
    if (s->prof && prof_end(s, pr, st)) return NB_EHIP;
    return NB_OK;
}

// One gather launch over particles [first, first + cnt): the slabs of rows [lo, hi) of every tile along the coverage lists
// (cb, cov), plus `add` when given, stored to `dst` — or, fused, kick and drift applied in the same kernel.
static int launch_gather(nb_sim *s, bool fuse, const uint32_t *lo, const uint32_t *hi, const uint32_t *cb, const SymCov *cov,
                         uint32_t first, uint32_t cnt, void *dst, const void *add, double dt_kick, double dt_drift)
{
    const uint32_t n = (uint32_t)s->n, per = s->dims3 ? (uint32_t)GATHER_T : (uint32_t)GATHER_P, gg = (cnt + per - 1) / per;
    const int extras = fuse ? s->p.extras : 0, kd = fuse ? INTEG_KICK | INTEG_DRIFT : 0;
    with_layout(s, [&](auto L) {
        using real = typename decltype(L)::real;
        using vec = typename decltype(L)::vec;
        const vec *ss = (const vec *)s->sym_slab_s, *sr = (const vec *)s->sym_slab_r;
        const vec *pc = fuse ? (const vec *)s->pos[s->cur] : nullptr;
        vec *pn = fuse ? (vec *)s->pos[s->cur ^ 1] : nullptr, *vel = fuse ? (vec *)s->vel : nullptr, *acc = fuse ? (vec *)s->acc : nullptr;
        const real hk = fuse ? (real)dt_kick : (real)0, hd = fuse ? (real)dt_drift : (real)0;
        with_flags([&](auto f) {
            if constexpr (L.dims3)
                sym_gather3<real, f><<<gg, BLOCK, 0, s->stream>>>(ss, sr, lo, hi, cb, cov, n, first, cnt, (vec *)dst, (const vec *)add,
                                                                  pc, pn, vel, acc, hk, hd, kd);
            else
                with_flags([&](auto o) {        // an ordered handle (whole system: first = 0): row k belongs to body perm[k]
                    sym_gather<real, f, o><<<gg, BLOCK, 0, s->stream>>>(ss, sr, lo, hi, cb, cov, n, first, cnt, (vec *)dst, (const vec *)add,
                                                                        pc, pn, vel, acc, hk, hd, extras, kd, s->sym_sb_shift, o ? s->ord.perm : nullptr);
                }, s->ord.on);
        }, fuse);
    });
    HIPCHK(hipGetLastError());
    return NB_OK;
}

// Sum of the slabs.  fuse_step (whole-system handles): apply kick and drift in the same kernel; otherwise the
// summed (unsharded) or partial (sharded rank) acceleration of every particle is stored: slab 0 / acc_full.
// A sharded rank's late items are left out here (launch_sym_gather_late folds them in).
static int launch_sym_gather(nb_sim *s, bool fuse_step, double dt_kick, double dt_drift)
{
    void *dst = s->path == StepPath::SYM ? s->partial : s->acc_full;
    return launch_gather(s, fuse_step, s->sym_rowbase_dev, s->sym_rowbase_dev + s->sym_tiles,     // [first row, first late row)
                         s->sym_cov_begin_dev, s->sym_cov_dev, 0u, (uint32_t)s->n, dst, nullptr, dt_kick, dt_drift);
}

// Sharded rank, after the reduce-scatter: acceleration of the owned block = acc_owned (the summed partials of all
// ranks) + the slabs of this rank's late items; kick and drift applied in the same kernel.
static int launch_sym_gather_late(nb_sim *s, double dt)
{
    const uint32_t tiles = s->sym_tiles;
    return launch_gather(s, true, s->sym_rowbase_dev + tiles, s->sym_rowbase_dev + 2 * (size_t)tiles,   // [first late row, end row)
                         s->sym_cov_begin_dev + (tiles + 1), s->sym_cov_dev + s->sym_cov_late_off,      // coverage lists of the late segments
                         (uint32_t)s->i_begin, (uint32_t)s->i_count, nullptr, s->acc_owned, dt, dt);
}

// Whole-system symmetric force (+ optionally the kick/drift).
static int launch_force_sym(nb_sim *s, bool fuse_step = false, double dt_kick = 0.0, double dt_drift = 0.0)
{
    int rc;
    if (s->ord.on && (rc = order_prepare(s))) return rc;
    if ((rc = launch_sym_items(s, 0, s->sym_items))) return rc;
    return launch_sym_gather(s, fuse_step, dt_kick, dt_drift);
}

static int launch_force(nb_sim *s, const ForceJob &j)
{
    if (j.j_end <= j.j_begin || j.js == 0) return NB_OK;
    if (s->tree) return nb_fail(NB_ESTATE, "internal: a direct-sum force launch on a NB_FORCE_TREE handle (it has no partial slabs)");
    if (s->path == StepPath::SYM && &j == &s->job_all) return launch_force_sym(s);
    std::pair<hipEvent_t, hipEvent_t> pr;
    if (s->prof && prof_begin(s, &pr)) return NB_EHIP;
    const bool guard = needs_guard(s), quake = s->p.rsqrt_mode == NB_RSQRT_QUAKE;
    // the hoisted-mass and mass-scaled bodies have no guard form; mass_scaled implies exact rsqrt (decided at upload)
    const bool um = s->uniform_mass && !guard, scaled = s->mass_scaled && !guard;
    const uint32_t ib = (uint32_t)s->i_begin, ic = (uint32_t)s->i_count, grid = grid_blocks(j.i_tiles, j.js);
    with_layout(s, [&](auto L) {
        using Lt = decltype(L);
        using real = typename Lt::real;
        using vec = typename Lt::vec;
        const real eps2 = (real)s->p.eps * (real)s->p.eps;   // Quadtree.hpp:19  e_sq(epsilon * epsilon)
        const vec *pos = (const vec *)s->pos[s->cur];
        vec *out = (vec *)s->partial + (size_t)j.slab0 * s->i_count;
        if constexpr (std::is_same_v<real, double>) {
            with_lanes<2>(j.P, [&](auto P) { with_flags([&](auto g) {
                force_tiled_f64<Lt, P, g><<<grid, BLOCK, 0, s->stream>>>(pos, (const double *)s->mass, out, ib, ic, j.j_begin, j.j_end,
                                                                         j.js, j.i_tiles, eps2, j.gap_begin, j.gap_len);
            }, guard); });
        } else {
            if constexpr (!L.dims3)      // nb_create refuses 3-D with the sequential order
                if (s->p.sum_order == NB_SUM_SEQUENTIAL) {
                    with_flags([&](auto q) {
                        force_seq_f32<q ? RSQ_QUAKE : RSQ_EXACT><<<(ic + BLOCK - 1) / BLOCK, BLOCK, 0, s->stream>>>(
                            pos, (const float *)s->mass, out, ib, ic, j.j_begin, j.j_end, eps2);
                    }, quake);
                    return;
                }
            with_lanes<4>(j.P, [&](auto P) { with_flags([&](auto q, auto g) {
                constexpr int RQ = q ? RSQ_QUAKE : RSQ_EXACT;
                auto go = [&](auto kernel, float umv) {
                    kernel<<<grid, BLOCK, 0, s->stream>>>(pos, (const float *)s->mass, s->sigma, out, ib, ic, j.j_begin, j.j_end, j.js,
                                                          j.i_tiles, eps2, umv, j.gap_begin, j.gap_len);
                };
                if constexpr (!g) {
                    if (um) return go(force_tiled_f32<Lt, P, RQ, false, true>, s->um_mass);
                    if constexpr (RQ == RSQ_EXACT && !L.dims3)     // individual masses folded into the pair geometry: no mass multiply in the body
                        if (scaled) return go(force_tiled_f32<Lt, P, RSQ_EXACT, false, false, true>, 1.0f);
                }
                go(force_tiled_f32<Lt, P, RQ, g, false>, 1.0f);
            }, quake, guard); });
        }
    });
    HIPCHK(hipGetLastError());
    if (s->prof && prof_end(s, pr)) return NB_EHIP;
    return NB_OK;
}

// Kick and drift (as `flags` ask) of particles [first, first + cnt) with the sum of `nslabs` slabs of `src` as their
// acceleration: the one-sided kernels' partials, or the one summed slab of a sharded or replicated handle's exchange.
static int launch_integrate(nb_sim *s, const void *src, uint32_t nslabs, uint32_t first, uint32_t cnt, double dt_kick, double dt_drift, int flags)
{
    const uint32_t g = (cnt + BLOCK - 1) / BLOCK;
    const bool strict = s->p.sum_order == NB_SUM_SEQUENTIAL;
    with_layout(s, [&](auto L) {
        using real = typename decltype(L)::real;
        using vec = typename decltype(L)::vec;
        const vec *pc = (const vec *)s->pos[s->cur], *sl = (const vec *)src;
        vec *pn = (vec *)s->pos[s->cur ^ 1], *vel = (vec *)s->vel, *acc = (vec *)s->acc;
        auto go = [&](auto kernel) {
            kernel<<<g, BLOCK, 0, s->stream>>>(pc, pn, vel, acc, sl, nslabs, first, cnt, (real)dt_kick, (real)dt_drift, s->p.extras, flags);
        };
        if constexpr (std::is_same_v<real, float> && !L.dims3)
            if (strict) return go(integrate<decltype(L), true>);   // the sequential order's strict form: fp32 2-D only
        go(integrate<decltype(L), false>);
    });
    HIPCHK(hipGetLastError());
    return NB_OK;
}

// The one-sided form: the force partials of the owned block.
static int integrate_slabs(nb_sim *s, uint32_t nslabs, double dt_kick, double dt_drift, int flags)
{
    if (s->tree) return nb_fail(NB_ESTATE, "internal: a slab integration on a NB_FORCE_TREE handle (it has no partial slabs)");
    return launch_integrate(s, s->partial, nslabs, (uint32_t)s->i_begin, (uint32_t)s->i_count, dt_kick, dt_drift, flags);
}

// ---------------------------------------------------------------------------
// stepping
// ---------------------------------------------------------------------------
static int step_begin_enqueue(nb_sim *s)
{
    switch (s->path) {
    case StepPath::SYM_REPLICATED: {
        // every position is already here (each rank integrates everything): all items in one launch, then this rank's
        // PARTIAL acceleration of every particle -> acc_full, which the host all-reduces before nb_step_finish
        int rc = launch_sym_items(s, 0, s->sym_items);
        if (rc) return rc;
        return launch_sym_gather(s, false, 0.0, 0.0);
    }
    case StepPath::SYM_SHARDED: {
        // pairs inside my own block: no remote data needed.  On the side stream (ordered after everything
        // enqueued so far), so the cross items of nb_step_mid fill the CUs its last workgroups leave idle.
        if (!s->aux_local) return launch_sym_items(s, 0, s->sym_items_local);
        HIPCHK(hipEventRecord(s->ev_fork, s->stream));
        HIPCHK(hipStreamWaitEvent(s->aux, s->ev_fork, 0));
        const int rc = launch_sym_items(s, 0, s->sym_items_local, s->aux);
        if (rc) return rc;
        HIPCHK(hipEventRecord(s->ev_join, s->aux));
        return NB_OK;
    }
    case StepPath::TWO_PHASE:
        // local j-block first: its positions are already resident, so this overlaps the exchange
        return launch_force(s, s->job_local);
    case StepPath::SYM:
    case StepPath::ONE_SIDED:
        break;
    }
    return NB_OK;
}

extern "C" int nb_step_begin(nb_sim *s, float dt)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_step_begin: NULL handle");
    if (s->in_step) return nb_fail(NB_ESTATE, "nb_step_begin: previous step not finished");
    if (s->broken) return nb_fail(NB_ESTATE, "nb_step_begin: an earlier force launch of this handle was refused by the runtime; destroy the handle");
    if (hermite(s)) return nb_fail(NB_EINVAL, "nb_step_begin: split stepping is the kick-drift integrator's (a HERMITE4 handle steps with nb_step)");
    if (const char *name = composed_name(s->p.integrator)) return nb_fail(NB_EINVAL, "nb_step_begin: split stepping is the kick-drift integrator's (a %s handle steps with nb_step)", name);
    if (s->p.integrator != NB_INTEGRATOR_KICK_DRIFT) return nb_fail(NB_EINVAL, "nb_step_begin: split stepping is the kick-drift integrator's (a KDK handle steps with nb_step)");
    if (bind(s)) return NB_EHIP;
    s->pending_dt = dt > 0.0f ? dt : s->p.dt;
    const int rc = step_begin_enqueue(s);
    if (rc) return rc;              // the handle is NOT left "in step": the caller sees the real error and may retry or destroy it
    s->in_step = true;
    return NB_OK;
}

extern "C" int nb_step_mid(nb_sim *s)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_step_mid: NULL handle");
    if (!s->in_step) return nb_fail(NB_ESTATE, "nb_step_mid: no step in flight");
    if (s->path != StepPath::SYM_SHARDED) return NB_OK;   // nothing between begin and finish in the other protocols
    if (s->mid_done) return nb_fail(NB_ESTATE, "nb_step_mid: already called for this step");
    if (bind(s)) return NB_EHIP;
    int rc = launch_sym_items(s, s->sym_items_local, s->sym_items_cross);   // cross-block pairs: need the gathered positions
    if (rc) return rc;
    if (s->sym_items_late) {
        // the held-back local items go to the side stream once the cross items are through: they run while the
        // host's reduce-scatter of acc_full is in flight and are folded in by nb_step_finish
        HIPCHK(hipEventRecord(s->ev_fork, s->stream));
        HIPCHK(hipStreamWaitEvent(s->aux, s->ev_fork, 0));
        if ((rc = launch_sym_items(s, s->sym_items_local + s->sym_items_cross, s->sym_items_late, s->aux))) return rc;
        HIPCHK(hipEventRecord(s->ev_late, s->aux));
    }
    if (s->aux_local) HIPCHK(hipStreamWaitEvent(s->stream, s->ev_join, 0));   // the local items' slabs
    if ((rc = launch_sym_gather(s, false, 0.0, 0.0))) return rc;                   // partial acceleration of every particle -> acc_full
    s->mid_done = true;                                // only once everything was enqueued: a failed call can be seen and repeated
    return NB_OK;
}

extern "C" int nb_step_finish(nb_sim *s)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_step_finish: NULL handle");
    if (!s->in_step) return nb_fail(NB_ESTATE, "nb_step_finish: no step in flight");
    if (bind(s)) return NB_EHIP;
    s->in_step = false;
    const double dt = s->pending_dt;
    int rc;
    switch (s->path) {
    case StepPath::SYM_REPLICATED:
        // acc_full holds the all-reduced acceleration of every particle: kick and drift them all
        if ((rc = launch_integrate(s, s->acc_full, 1, 0u, (uint32_t)s->n, dt, dt, INTEG_KICK | INTEG_DRIFT))) return rc;
        break;
    case StepPath::SYM_SHARDED:
        if (!s->mid_done) { s->in_step = true; return nb_fail(NB_ESTATE, "nb_step_finish: symmetric sharded handle needs nb_step_mid (and the reduce-scatter) first"); }
        s->mid_done = false;
        // the host has reduce-scattered acc_full into acc_owned: it is the one slab of the owned block
        if (s->sym_items_late) {
            HIPCHK(hipStreamWaitEvent(s->stream, s->ev_late, 0));
            if ((rc = launch_sym_gather_late(s, dt))) return rc;
        } else if ((rc = launch_integrate(s, s->acc_owned, 1, (uint32_t)s->i_begin, (uint32_t)s->i_count, dt, dt, INTEG_KICK | INTEG_DRIFT))) {
            return rc;
        }
        break;
    case StepPath::SYM:
        // whole system, symmetric kernel: the gather launch applies the kick and the drift itself
        if ((rc = launch_force_sym(s, true, dt, dt))) return rc;
        break;
    case StepPath::TWO_PHASE:
        if ((rc = launch_force(s, s->job_remote)) || (rc = integrate_slabs(s, s->slabs_two_phase, dt, dt, INTEG_KICK | INTEG_DRIFT))) return rc;
        break;
    case StepPath::ONE_SIDED:
        if (s->tree) { if ((rc = launch_tree_force(s)) || (rc = launch_tree_integrate(s, dt, dt, INTEG_KICK | INTEG_DRIFT))) return rc; break; }
        if ((rc = launch_force(s, s->job_all)) || (rc = integrate_slabs(s, s->slabs_all, dt, dt, INTEG_KICK | INTEG_DRIFT))) return rc;
        break;
    }
    s->cur ^= 1;
    s->frame += 1;                                  // Simulation.hpp:74
    s->acc_valid = false;
    // Simulation.hpp:72: collide() after iterate(), on the drifted positions (the frame counter is host-side: the order of
    // the two lines above and this launch is not observable)
    if (s->collide && (rc = launch_collide(s))) return rc;
    return NB_OK;
}

static int step_kdk(nb_sim *s, double dt)
{
    int rc;
    if (!s->acc_valid) {                            // a(x_n), first step only
        if ((rc = launch_force(s, s->job_all))) return rc;
        if ((rc = integrate_slabs(s, s->slabs_all, 0.0, 0.0, 0))) return rc;   // acc <- slabs only
    } else {
        // acc already holds a(x_n): re-present it as the single slab 0
        HIPCHK(hipMemcpyAsync(s->partial, s->acc, s->i_count * s->esz, hipMemcpyDeviceToDevice, s->stream));
    }
    // half kick + drift (acc from slab(s)), then force at x_{n+1} and the second half kick
    if ((rc = integrate_slabs(s, s->acc_valid ? 1 : s->slabs_all, 0.5 * dt, dt, INTEG_KICK | INTEG_DRIFT))) return rc;
    s->cur ^= 1;
    if ((rc = launch_force(s, s->job_all))) return rc;
    if ((rc = integrate_slabs(s, s->slabs_all, 0.5 * dt, 0.0, INTEG_KICK))) return rc;
    s->acc_valid = true;
    s->frame += 1;
    return NB_OK;
}

// ---- the composed integrators: NB_INTEGRATOR_DKD and NB_INTEGRATOR_FR4 (include/nbody.h) ----
// One step of size h = a leading drift, then stages of (force at the current x; v += a k h; x += v d h).  A stage is the path's
// own fused "force -> kick(dt_kick) -> drift(dt_drift)" launch with two different steps, so a DKD step costs a kick-drift step
// plus one pass over positions and velocities, and an FR4 step three of them plus that pass.
struct ComposedStage { double k, d; };
constexpr double FR4_THETA = 1.3512071919596576340476878089715;           // 1 / (2 - 2^(1/3))
constexpr double DKD_LEAD = 0.5, FR4_LEAD = 0.5 * FR4_THETA;
static const ComposedStage DKD_STAGES[1] = {{1.0, 0.5}};
static const ComposedStage FR4_STAGES[3] = {{FR4_THETA, 0.5 * (1.0 - FR4_THETA)}, {1.0 - 2.0 * FR4_THETA, 0.5 * (1.0 - FR4_THETA)}, {FR4_THETA, 0.5 * FR4_THETA}};

// x <- x + v h for every body, pos[cur] -> pos[cur ^ 1]; flips cur.  The strict form where the handle's kick and drift are strict.
static int launch_drift(nb_sim *s, double h)
{
    const uint32_t n = (uint32_t)s->n, g = (n + BLOCK - 1) / BLOCK;
    const bool strict = s->tree ? s->p.rsqrt_mode == NB_RSQRT_QUAKE : s->p.sum_order == NB_SUM_SEQUENTIAL;
    with_layout(s, [&](auto L) {
        using real = typename decltype(L)::real;
        using vec = typename decltype(L)::vec;
        auto go = [&](auto kernel) {
            kernel<<<g, BLOCK, 0, s->stream>>>((const vec *)s->pos[s->cur], (vec *)s->pos[s->cur ^ 1], (const vec *)s->vel, n, (real)h);
        };
        if constexpr (std::is_same_v<real, float> && !L.dims3)
            if (strict) return go(drift<decltype(L), true>);        // fp32 2-D only, as launch_integrate
        go(drift<decltype(L), false>);
    });
    HIPCHK(hipGetLastError());
    s->cur ^= 1;
    return NB_OK;
}

// Every coefficient * h is formed in double from the float h and rounded once to the handle's real (by the launches).  On a tree
// handle a stage whose build fails applies neither its kick nor its drift (tree_integrate carries the positions over); the
// leading drift is unconditional.  acc[] is left as the last stage's evaluation.
static int step_composed(nb_sim *s, float h, double lead, const ComposedStage *stages, int nstages)
{
    const double hd = (double)h;
    int rc;
    if ((rc = launch_drift(s, lead * hd))) return rc;
    for (int k = 0; k < nstages; ++k) {
        const double hk = stages[k].k * hd, hx = stages[k].d * hd;
        if (s->tree) { if ((rc = launch_tree_force(s)) || (rc = launch_tree_integrate(s, hk, hx, INTEG_KICK | INTEG_DRIFT))) return rc; }
        else if (s->path == StepPath::SYM) { if ((rc = launch_force_sym(s, true, hk, hx))) return rc; }
        else if ((rc = launch_force(s, s->job_all)) || (rc = integrate_slabs(s, s->slabs_all, hk, hx, INTEG_KICK | INTEG_DRIFT))) return rc;
        s->cur ^= 1;
    }
    s->frame += 1;
    s->acc_valid = false;
    return NB_OK;
}

extern "C" int nb_step(nb_sim *s, float dt, int nsteps)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_step: NULL handle");
    if (nsteps < 0) return nb_fail(NB_EINVAL, "nb_step: nsteps < 0");
    if (s->i_count != s->n || s->path == StepPath::SYM_REPLICATED || s->path == StepPath::SYM_SHARDED) return nb_fail(NB_ESTATE, "nb_step: sharded handle — drive it with nb_step_begin / exchange / nb_step_finish");
    if (s->in_step) return nb_fail(NB_ESTATE, "nb_step: a split step is in flight");
    if (bind(s)) return NB_EHIP;
    const float h = dt > 0.0f ? dt : s->p.dt;
    for (int k = 0; k < nsteps; ++k) {
        int rc;
        if (s->p.integrator == NB_INTEGRATOR_KDK) { if ((rc = step_kdk(s, h))) return rc; continue; }
        if (s->p.integrator == NB_INTEGRATOR_DKD || s->p.integrator == NB_INTEGRATOR_FR4) {
            if (s->broken) return nb_fail(NB_ESTATE, "nb_step: an earlier force launch of this handle was refused by the runtime; destroy the handle");
            const bool dkd = s->p.integrator == NB_INTEGRATOR_DKD;
            if ((rc = step_composed(s, h, dkd ? DKD_LEAD : FR4_LEAD, dkd ? DKD_STAGES : FR4_STAGES, dkd ? 1 : 3))) return rc;
            if (s->prof && s->ev_used.size() >= 2048 && (rc = prof_collect(s))) return rc;
            continue;
        }
        if (hermite(s)) {
            if ((rc = step_hermite(s, h))) return rc;
            if (s->prof && s->ev_used.size() >= 2048 && (rc = prof_collect(s))) return rc;
            continue;
        }
        if ((rc = nb_step_begin(s, h))) return rc;
        if ((rc = nb_step_finish(s))) return rc;
        // keep the event list bounded on long runs
        if (s->prof && s->ev_used.size() >= 2048 && (rc = prof_collect(s))) return rc;
    }
    return NB_OK;
}

extern "C" int nb_accelerations(nb_sim *s)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_accelerations: NULL handle");
    if (s->in_step) return nb_fail(NB_ESTATE, "nb_accelerations: a split step is in flight");
    if (bind(s)) return NB_EHIP;
    int rc;
    if (s->tree) return (rc = launch_tree_force(s)) ? rc : launch_tree_integrate(s, 0.0, 0.0, 0);
    s->herm.valid = false;            // acc[] is rewritten: a Hermite handle's carried pair is gone, its next step evaluates again
    // job_all: a sharded or replicated handle has no whole-system plan, so this takes the one-sided kernels
    if ((rc = launch_force(s, s->job_all))) return rc;
    return integrate_slabs(s, s->slabs_all, 0.0, 0.0, 0);   // acc <- sum of slabs, nothing else
}

extern "C" int nb_wait(nb_sim *s)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_wait: NULL handle");
    if (bind(s)) return NB_EHIP;
    if (s->aux) HIPCHK(hipStreamSynchronize(s->aux));
    HIPCHK(hipStreamSynchronize(s->stream));
    return step_check(s);
}

// ---------------------------------------------------------------------------
// host views
// ---------------------------------------------------------------------------
static int ensure_staging(nb_sim *s)
{
    if (!s->staging) HIPCHK(s->pool.alloc_pinned(s->staging, s->i_count * sizeof(nb_body)));
    return NB_OK;
}

// Page-locked host memory the library may DMA into / out of directly.  Whole pages only: a registration pins every
// page it touches, and pages shared with unrelated heap data (the first and last page of a malloc'ed array) must not be
// pinned on behalf of one array — so an unaligned range is REFUSED, not rounded (the caller does not own the rest of
// those pages).  Page-aligned storage comes from nb_host_alloc, posix_memalign / aligned_alloc or mmap.
extern "C" int nb_host_register(void *ptr, size_t bytes)
{
    if (!ptr || !bytes) return nb_fail(NB_EINVAL, "nb_host_register: NULL argument");
    const size_t ps = host_page_size();
    if (((uintptr_t)ptr % ps) != 0 || (bytes % ps) != 0)
        return nb_fail(NB_EINVAL, "nb_host_register: [%p, +%zu) is not a whole number of %zu-byte pages; registration pins whole pages, "
                                  "and the pages an unaligned array shares with its heap neighbours are not the caller's to pin "
                                  "(use nb_host_alloc, or page-aligned storage)", ptr, bytes, ps);
    if (pinned_covers(ptr, 1)) return nb_fail(NB_ESTATE, "nb_host_register: %p is already registered", ptr);
    HIPCHK(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    std::lock_guard<std::mutex> lock(g_pin_mutex);
    g_pinned.push_back(PinnedRange{(uintptr_t)ptr, (uintptr_t)ptr + bytes, false});
    return NB_OK;
}

// Only ranges registered through nb_host_register, by their start address, and before their storage is released.
extern "C" int nb_host_unregister(void *ptr)
{
    if (!ptr) return nb_fail(NB_EINVAL, "nb_host_unregister: NULL argument");
    {
        std::lock_guard<std::mutex> lock(g_pin_mutex);
        size_t k = 0;
        while (k < g_pinned.size() && !(g_pinned[k].lo == (uintptr_t)ptr && !g_pinned[k].owned)) ++k;
        if (k == g_pinned.size()) return nb_fail(NB_EINVAL, "nb_host_unregister: %p was not registered with nb_host_register", ptr);
        g_pinned.erase(g_pinned.begin() + (long)k);
    }
    HIPCHK(hipHostUnregister(ptr));
    return NB_OK;
}

// Page-locked, page-aligned host memory owned by the library (hipHostMalloc): the simplest destination for
// nb_sync / nb_snapshot_begin that the copy engine writes directly.  NULL on failure (nb_last_error).
extern "C" void *nb_host_alloc(size_t bytes)
{
    if (!bytes) { nb_fail(NB_EINVAL, "nb_host_alloc: zero bytes"); return nullptr; }
    if (nb_device_count() <= 0) { nb_fail(NB_ENODEVICE, "nb_host_alloc: no HIP device visible"); return nullptr; }
    void *p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); nb_fail(hip_code(e), "nb_host_alloc: hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e)); return nullptr; }
    std::lock_guard<std::mutex> lock(g_pin_mutex);
    g_pinned.push_back(PinnedRange{(uintptr_t)p, (uintptr_t)p + bytes, true});
    return p;
}

extern "C" int nb_host_free(void *ptr)
{
    if (!ptr) return NB_OK;
    {
        std::lock_guard<std::mutex> lock(g_pin_mutex);
        size_t k = 0;
        while (k < g_pinned.size() && !(g_pinned[k].lo == (uintptr_t)ptr && g_pinned[k].owned)) ++k;
        if (k == g_pinned.size()) return nb_fail(NB_EINVAL, "nb_host_free: %p did not come from nb_host_alloc", ptr);
        g_pinned.erase(g_pinned.begin() + (long)k);
    }
    HIPCHK(hipHostFree(ptr));
    return NB_OK;
}

// AoS view of the owned block into aos_dev, on the handle's stream
// SoA -> 64-byte Body records of `cnt` owned particles from offset `o` of the owned block, written to `out` (device memory, or
// page-locked host memory the device can address: the small-transfer path of nb_sync writes the staging buffer directly).
static int launch_pack_range(nb_sim *s, BodyRec *out, uint32_t o, uint32_t cnt)
{
    if (cnt == 0) return NB_OK;
    const uint32_t g = (cnt + BLOCK - 1) / BLOCK, ib = (uint32_t)s->i_begin + o;
    const size_t e = s->esz * (size_t)o;                 // vel / acc are indexed from the start of the owned block
    const char *vel = (const char *)s->vel + e, *acc = (const char *)s->acc + e;
    with_layout(s, [&](auto L) {
        using real = typename decltype(L)::real;
        using vec = typename decltype(L)::vec;
        const vec *pos = (const vec *)s->pos[s->cur];
        pack_bodies<decltype(L)><<<g, BLOCK, 0, s->stream>>>(out, pos, (const real *)s->mass, (const vec *)vel, (const vec *)acc, s->radius,
                                                             ib, cnt);
    });
    HIPCHK(hipGetLastError());
    return NB_OK;
}

static int launch_pack(nb_sim *s) { return launch_pack_range(s, s->aos_dev, 0, (uint32_t)s->i_count); }

static int snapshot_wait(nb_sim *s)
{
    if (!s->snap_pending) return NB_OK;
    if (bind(s)) return NB_EHIP;
    HIPCHK(hipEventSynchronize(s->ev_copied));
    if (!s->snap_direct) memcpy(s->snap_out, s->staging, s->i_count * sizeof(nb_body));
    s->snap_pending = false;
    s->snap_out = nullptr;
    return NB_OK;
}

extern "C" int nb_snapshot_wait(nb_sim *s)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_snapshot_wait: NULL handle");
    const int rc = snapshot_wait(s);
    return rc ? rc : collide_report(s);        // the record nb_snapshot_begin copied beside the bodies: no wait for later steps
}

extern "C" int nb_snapshot_begin(nb_sim *s, nb_body *out)
{
    if (!s || !out) return nb_fail(NB_EINVAL, "nb_snapshot_begin: NULL argument");
    if (s->snap_pending) return nb_fail(NB_ESTATE, "nb_snapshot_begin: a snapshot is already in flight (call nb_snapshot_wait)");
    if (s->in_step) return nb_fail(NB_ESTATE, "nb_snapshot_begin: a split step is in flight");
    if (bind(s)) return NB_EHIP;
    if (!s->copy_stream) {
        HIPCHK(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&s->ev_packed, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&s->ev_copied, hipEventDisableTiming));
    }
    s->snap_direct = pinned_covers(out, s->i_count * sizeof(nb_body));
    if (!s->snap_direct && ensure_staging(s)) return NB_EHIP;
    // aos_dev is free again: the previous snapshot was waited for, and nb_sync / nb_upload synchronise before returning
    int rc = launch_pack(s);
    if (rc) return rc;
    if (s->collide) HIPCHK(hipMemcpyAsync(s->coll.host, s->coll.stats, sizeof(CollideStats), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipEventRecord(s->ev_packed, s->stream));
    HIPCHK(hipStreamWaitEvent(s->copy_stream, s->ev_packed, 0));
    HIPCHK(hipMemcpyAsync(s->snap_direct ? (void *)out : s->staging, s->aos_dev, s->i_count * sizeof(nb_body), hipMemcpyDeviceToHost, s->copy_stream));
    HIPCHK(hipEventRecord(s->ev_copied, s->copy_stream));
    s->snap_out = out;
    s->snap_pending = true;
    return NB_OK;
}

extern "C" int nb_sync(nb_sim *s, nb_body *out)
{
    if (!s || !out) return nb_fail(NB_EINVAL, "nb_sync: NULL argument");
    if (bind(s)) return NB_EHIP;
    int rc = snapshot_wait(s);                        // aos_dev / staging may still be feeding a pipelined snapshot
    if (rc || (rc = step_check(s))) return rc;
    const size_t bytes = s->i_count * sizeof(nb_body);
    const bool direct = pinned_covers(out, bytes);
    if (!direct && ensure_staging(s)) return NB_EHIP;
    if (!direct && bytes <= SMALL_SYNC_BYTES) {
        // Small systems (the reference's own 25 000 bodies = 1.6 MB per frame, main.cpp:621-627): the copy engine's start-up costs
        // as much as the transfer.  The pack kernel writes the records STRAIGHT INTO the page-locked staging buffer over PCIe, in
        // two halves with an event each; the host copies half 0 into the caller's (pageable) array while half 1 is on the wire.
        // No DMA, no device-side AoS round trip.  (Measured on the reference's default start: profiles/r06_frames_*.)
        { const int e = ensure_bounce(s); if (e) return e; }
        const uint32_t ic = (uint32_t)s->i_count, c0 = ic < 2 * BLOCK ? ic : ((ic / 2 + BLOCK - 1) / BLOCK) * BLOCK;
        BodyRec *stage = (BodyRec *)s->staging;
        if ((rc = launch_pack_range(s, stage, 0, c0))) return rc;
        HIPCHK(hipEventRecord(s->ev_bounce[0], s->stream));
        if ((rc = launch_pack_range(s, stage + c0, c0, ic - c0))) return rc;
        HIPCHK(hipEventRecord(s->ev_bounce[1], s->stream));
        HIPCHK(hipEventSynchronize(s->ev_bounce[0]));
        memcpy(out, stage, (size_t)c0 * sizeof(nb_body));
        HIPCHK(hipEventSynchronize(s->ev_bounce[1]));
        memcpy(out + c0, stage + c0, (size_t)(ic - c0) * sizeof(nb_body));
        return NB_OK;
    }
    if ((rc = launch_pack(s))) return rc;
    // registered destination: one DMA; pageable destination: staged in pieces, the host copies piece k out while
    // piece k + 1 is still in flight
    return copy_d2h(s, out, s->aos_dev, bytes, s->stream, s->staging);
}

extern "C" int nb_sync_positions(nb_sim *s, float *out_xy)
{
    if (!s || !out_xy) return nb_fail(NB_EINVAL, "nb_sync_positions: NULL argument");
    if (bind(s)) return NB_EHIP;
    if (snapshot_wait(s)) return nb_last_error_code();
    { const int rc = step_check(s); if (rc) return rc; }
    if (ensure_staging(s)) return NB_EHIP;
    const uint32_t ic = (uint32_t)s->i_count, g = (ic + BLOCK - 1) / BLOCK;
    const size_t bytes = s->i_count * (s->dims3 ? 3 : 2) * sizeof(float);       // (x, y) or (x, y, z) per body
    const void *src = s->aos_dev;
    with_layout(s, [&](auto L) {
        using real = typename decltype(L)::real;
        using vec = typename decltype(L)::vec;
        const vec *pos = (const vec *)s->pos[s->cur];
        if constexpr (L.dims3 || std::is_same_v<real, double>)
            pack_positions<decltype(L)><<<g, BLOCK, 0, s->stream>>>((float *)s->aos_dev, pos, (uint32_t)s->i_begin, ic);
        else
            src = pos + s->i_begin;                        // fp32 2-D positions are already (x, y) floats: no kernel
    });
    if (src == s->aos_dev) HIPCHK(hipGetLastError());      // a pack kernel ran
    return copy_d2h(s, out_xy, src, bytes, s->stream, s->staging);
}

extern "C" int nb_energy(nb_sim *s, double *kinetic, double *potential)
{
    if (!s || !kinetic || !potential) return nb_fail(NB_EINVAL, "nb_energy: NULL argument");
    if (bind(s)) return NB_EHIP;
    { const int rc = step_check(s); if (rc) return rc; }
    const uint32_t g = (uint32_t)s->ered_blocks, sets = s->bh.energy ? 2u : 1u;     // sets of partials [K (g) | U (g)] the kernels leave
    if (s->bh.energy) {       // O(n log n): the tree of the current positions and its potential walk; a failed build is reported by THIS call
        { const int rc = launch_tree_potential(s); if (rc) return rc; }
        { const int rc = tree_check(s); if (rc) return rc; }
    } else {
        const double eps2 = (double)s->p.eps * (double)s->p.eps;
        with_layout(s, [&](auto L) {
            using real = typename decltype(L)::real;
            using vec = typename decltype(L)::vec;
            const vec *pos = (const vec *)s->pos[s->cur], *vel = (const vec *)s->vel;
            energy_partials<decltype(L)><<<g, BLOCK, 0, s->stream>>>(pos, (const real *)s->mass, vel, (uint32_t)s->n, (uint32_t)s->i_begin,
                                                                     (uint32_t)s->i_count, eps2, s->ered_dev, s->ered_dev + g);
        });
        HIPCHK(hipGetLastError());
    }
    std::vector<double> h(2 * (size_t)sets * g);
    { const int rc = copy_d2h(s, h.data(), s->ered_dev, h.size() * sizeof(double)); if (rc) return rc; }
    double K = 0.0, U = 0.0;
    for (uint32_t q = 0; q < sets; ++q)
        for (uint32_t b = 0; b < g; ++b) { K += h[2 * (size_t)q * g + b]; U += h[(2 * (size_t)q + 1) * g + b]; }
    *kinetic = K;
    *potential = U;
    return NB_OK;
}

extern "C" int nb_momentum(nb_sim *s, double *p_xyz, double *l_z)
{
    if (!s || !p_xyz) return nb_fail(NB_EINVAL, "nb_momentum: NULL argument");
    if (bind(s)) return NB_EHIP;
    { const int rc = step_check(s); if (rc) return rc; }
    const uint32_t g = (uint32_t)s->ered_blocks;
    if (!s->pred_dev) HIPCHK(s->pool.alloc(s->pred_dev, 4 * (size_t)g));
    with_layout(s, [&](auto L) {
        using real = typename decltype(L)::real;
        using vec = typename decltype(L)::vec;
        const vec *pos = (const vec *)s->pos[s->cur], *vel = (const vec *)s->vel;
        momentum_partials<decltype(L)><<<g, BLOCK, 0, s->stream>>>(pos, (const real *)s->mass, vel, (uint32_t)s->i_begin, (uint32_t)s->i_count,
                                                                   s->pred_dev);
    });
    HIPCHK(hipGetLastError());
    std::vector<double> h(4 * (size_t)g);
    { const int rc = copy_d2h(s, h.data(), s->pred_dev, h.size() * sizeof(double)); if (rc) return rc; }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < 4; ++c)
        for (uint32_t b = 0; b < g; ++b) acc[c] += h[(size_t)c * g + b];
    p_xyz[0] = acc[0]; p_xyz[1] = acc[1]; p_xyz[2] = acc[2];
    if (l_z) *l_z = acc[3];
    return NB_OK;
}

extern "C" uint64_t nb_frame(const nb_sim *s) { return s ? s->frame : 0; }
extern "C" size_t nb_count(const nb_sim *s) { return s ? s->n : 0; }
extern "C" size_t nb_owned_begin(const nb_sim *s) { return s ? s->i_begin : 0; }
extern "C" size_t nb_owned_count(const nb_sim *s) { return s ? s->i_count : 0; }
extern "C" void *nb_pos_buffer(nb_sim *s, int which) { return s ? s->pos[which == NB_POS_NEXT ? (s->cur ^ 1) : s->cur] : nullptr; }
extern "C" void *nb_stream(nb_sim *s) { return s ? (void *)s->stream : nullptr; }
extern "C" size_t nb_pos_rows(const nb_sim *s) { return s ? s->pos_rows : 0; }
extern "C" int nb_device(const nb_sim *s) { return s ? s->dev : -1; }
extern "C" int nb_shard_rank(const nb_sim *s, int *world)
{
    if (world) *world = s ? s->p.shard_world : 0;
    return s ? s->p.shard_rank : -1;
}
extern "C" int nb_element_layout(const nb_sim *s, int *reals_per_element, int *bytes_per_real)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_element_layout: NULL handle");
    if (reals_per_element) *reals_per_element = s->dims3 ? 4 : 2;
    if (bytes_per_real) *bytes_per_real = (int)s->rsz;
    return NB_OK;
}
// ---- in-process exchanges (one host process drives all the handles; no RCCL) -------------------------------------
// Everything below is STREAM-ORDERED: the handles' streams wait for each other through events, the host never blocks.
// cross_fence: every handle's stream waits for the work enqueued so far on every other handle's stream.
static int cross_fence(nb_sim *const *sims, int count, int which)
{
    for (int a = 0; a < count; ++a) {
        nb_sim *s = sims[a];
        if (bind(s)) return NB_EHIP;
        if (!s->ev_x[which]) HIPCHK(hipEventCreateWithFlags(&s->ev_x[which], hipEventDisableTiming));
        HIPCHK(hipEventRecord(s->ev_x[which], s->stream));
    }
    for (int a = 0; a < count; ++a) {
        if (bind(sims[a])) return NB_EHIP;
        for (int b = 0; b < count; ++b)
            if (b != a) HIPCHK(hipStreamWaitEvent(sims[a]->stream, sims[b]->ev_x[which], 0));
    }
    return NB_OK;
}

// Kernels of handle s read the peers' buffers directly: map them.  Only "already enabled" is not an error — on a node
// that refuses peer access the caller gets NB_EHIP here instead of a faulting kernel later.
static int enable_peers(nb_sim *s, nb_sim *const *sims, int count)
{
    for (int r = 0; r < count; ++r) {
        const int d = sims[r]->dev;
        if (d == s->dev || d >= 64 || (s->peers_enabled >> d & 1u)) continue;
        int can = 0;
        HIPCHK(hipDeviceCanAccessPeer(&can, s->dev, d));
        if (!can) return nb_fail(NB_EHIP, "device %d cannot access device %d's memory (no peer access): in-process exchange impossible", s->dev, d);
        const hipError_t e = hipDeviceEnablePeerAccess(d, 0);
        if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
        else if (e != hipSuccess) { (void)hipGetLastError(); return nb_fail(NB_EHIP, "hipDeviceEnablePeerAccess(%d) on device %d: %s", d, s->dev, hipGetErrorString(e)); }
        s->peers_enabled |= (uint64_t)1 << d;
    }
    return NB_OK;
}

extern "C" int nb_exchange_positions(nb_sim *const *sims, int count)
{
    if (!sims || count < 1) return nb_fail(NB_EINVAL, "nb_exchange_positions: no handles");
    for (int a = 0; a < count; ++a)
        if (!sims[a] || sims[a]->n != sims[0]->n || sims[a]->esz != sims[0]->esz)
            return nb_fail(NB_EINVAL, "nb_exchange_positions: handles must shard the same system");
    int rc = cross_fence(sims, count, 0);                        // every owner's new block is complete before anyone copies it
    if (rc) return rc;
    for (int o = 0; o < count; ++o) {
        const nb_sim *own = sims[o];
        const char *src = (const char *)own->pos[own->cur] + own->i_begin * own->esz;
        for (int d = 0; d < count; ++d) {
            if (d == o) continue;
            nb_sim *dst = sims[d];
            if (bind(dst)) return NB_EHIP;
            HIPCHK(hipMemcpyPeerAsync((char *)dst->pos[dst->cur] + own->i_begin * own->esz, dst->dev, src, own->dev,
                                      own->i_count * own->esz, dst->stream));
        }
    }
    return cross_fence(sims, count, 1);                          // nobody overwrites a block that is still being copied
}

extern "C" int nb_exchange_accelerations(nb_sim *const *sims, int count)
{
    if (!sims || count < 1 || count > 64) return nb_fail(NB_EINVAL, "nb_exchange_accelerations: 1..64 handles");
    PartialPtrs src;
    for (int a = 0; a < count; ++a) {
        if (!sims[a] || sims[a]->path != StepPath::SYM_SHARDED || sims[a]->n != sims[0]->n || sims[a]->esz != sims[0]->esz ||
            sims[a]->p.shard_world != count || sims[a]->p.shard_rank != a) {
            return nb_fail(NB_EINVAL, "nb_exchange_accelerations: needs the `count` handles of one symmetric sharded run, in rank order");
        }
        src.p[a] = sims[a]->acc_full;
    }
    int rc = cross_fence(sims, count, 0);                        // all partial accelerations are complete
    if (rc) return rc;
    for (int o = 0; o < count; ++o) {
        nb_sim *s = sims[o];
        if (bind(s)) return NB_EHIP;
        if ((rc = enable_peers(s, sims, count))) return rc;
        const uint32_t ic = (uint32_t)s->i_count, g = (ic + BLOCK - 1) / BLOCK;
        with_layout(s, [&](auto L) {
            using vec = typename decltype(L)::vec;
            sum_partials<vec><<<g, BLOCK, 0, s->stream>>>(src, count, (uint32_t)s->i_begin, ic, (vec *)s->acc_owned);
        });
        HIPCHK(hipGetLastError());
    }
    return cross_fence(sims, count, 1);                          // acc_full may be rewritten only after every peer has read it
}

extern "C" int nb_shard_protocol(const nb_sim *s)
{
    if (!s) return NB_SHARD_NONE;
    if (s->path == StepPath::SYM_REPLICATED) return NB_SHARD_ALLREDUCE;
    if (s->path == StepPath::SYM_SHARDED) return NB_SHARD_SYMMETRIC;   // also the single-rank form (NB_FLAG_SHARD_SINGLE: i_count == n)
    return s->i_count == s->n ? NB_SHARD_NONE : NB_SHARD_ALLGATHER;    // TWO_PHASE, and a sharded ONE_SIDED handle (sequential order)
}

// In-process all-reduce of the replicated protocol (a host that drives all `count` handles of one run itself):
// every handle's nb_acc_buffer(0) receives the sum, in rank order, of all handles' partial accelerations — the same
// bits everywhere, so the replicas stay identical.  Call it between nb_step_begin and nb_step_finish.
extern "C" int nb_exchange_allreduce(nb_sim *const *sims, int count)
{
    if (!sims || count < 1 || count > 64) return nb_fail(NB_EINVAL, "nb_exchange_allreduce: 1..64 handles");
    PartialPtrs src;
    for (int a = 0; a < count; ++a) {
        if (!sims[a] || sims[a]->path != StepPath::SYM_REPLICATED || sims[a]->n != sims[0]->n || sims[a]->esz != sims[0]->esz ||
            sims[a]->p.shard_world != count || sims[a]->p.shard_rank != a)
            return nb_fail(NB_EINVAL, "nb_exchange_allreduce: needs the `count` handles of one replicated (NB_FLAG_SHARD_ALLREDUCE) run, in rank order");
        src.p[a] = sims[a]->acc_full;
    }
    int rc = cross_fence(sims, count, 0);
    if (rc) return rc;
    for (int o = 0; o < count; ++o) {               // sums into each handle's scratch (its `partial` array) ...
        nb_sim *s = sims[o];
        if (bind(s)) return NB_EHIP;
        if ((rc = enable_peers(s, sims, count))) return rc;
        const uint32_t nn = (uint32_t)s->n, g = (nn + BLOCK - 1) / BLOCK;
        with_layout(s, [&](auto L) {
            using vec = typename decltype(L)::vec;
            sum_partials<vec><<<g, BLOCK, 0, s->stream>>>(src, count, 0u, nn, (vec *)s->partial);
        });
        HIPCHK(hipGetLastError());
    }
    if ((rc = cross_fence(sims, count, 1))) return rc;           // ... and only when every handle has read every input
    for (int o = 0; o < count; ++o) {               // over the inputs
        nb_sim *s = sims[o];
        if (bind(s)) return NB_EHIP;
        HIPCHK(hipMemcpyAsync(s->acc_full, s->partial, s->n * s->esz, hipMemcpyDeviceToDevice, s->stream));
    }
    return NB_OK;
}
extern "C" void *nb_acc_buffer(nb_sim *s, int which)
{
    if (!s || (s->path != StepPath::SYM_SHARDED && s->path != StepPath::SYM_REPLICATED)) return nullptr;
    return which == 0 ? s->acc_full : s->acc_owned;
}

extern "C" int nb_dump(nb_sim *s, const char *path)
{
    if (!s || !path) return nb_fail(NB_EINVAL, "nb_dump: NULL argument");
    if (s->i_count != s->n) return nb_fail(NB_ESTATE, "nb_dump: sharded handle holds only its block; gather on the host and use nb_write_bodies");
    std::vector<nb_body> host(s->n);
    int rc = nb_sync(s, host.data());
    if (rc) return rc;
    return nb_write_bodies(path, host.data(), s->n, s->frame, &s->p);
}

// ---------------------------------------------------------------------------
// measurement
// ---------------------------------------------------------------------------
extern "C" int nb_profile_enable(nb_sim *s, int on)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_profile_enable: NULL handle");
    s->prof = on != 0;
    return NB_OK;
}

extern "C" int nb_profile_read(nb_sim *s, double *force_ms_total, uint64_t *force_launches, int reset)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_profile_read: NULL handle");
    if (bind(s)) return NB_EHIP;
    int rc = prof_collect(s);
    if (rc) return rc;
    if (force_ms_total) *force_ms_total = s->prof_ms;
    if (force_launches) *force_launches = s->prof_launches;
    if (reset) { s->prof_ms = 0.0; s->prof_launches = 0; }
    return NB_OK;
}

#ifdef NB_TEST_HOOKS   /* include/nbody_debug.h: test build only */
// Quadtree::fast_inv_sqrt (Quadtree.hpp:106-111) as the device evaluates it, on an array: y_scalar from the scalar form
// used by the sequential kernel, y_packed from the packed form of the tiled / symmetric kernels.  n must be even.
extern "C" int nb_debug_fast_inv_sqrt(const float *x, float *y_scalar, float *y_packed, size_t n)
{
    if (!x || !y_scalar || !y_packed || n == 0 || (n & 1) || n > 0x7fffff00u) return nb_fail(NB_EINVAL, "nb_debug_fast_inv_sqrt: bad arguments (n even)");
    if (nb_device_count() <= 0) return nb_fail(NB_ENODEVICE, "nb_debug_fast_inv_sqrt: no HIP device visible");
    MemPool<HipMem> tmp;
    float *dx = nullptr, *ds = nullptr, *dp = nullptr, *host = nullptr;
    hipError_t e;
    // page-locked staging: pageable caller memory is never handed to HIP (see copy_h2d)
    if ((e = tmp.alloc_pinned(host, 3 * n)) != hipSuccess || (e = tmp.alloc(dx, n)) != hipSuccess || (e = tmp.alloc(ds, n)) != hipSuccess ||
        (e = tmp.alloc(dp, n)) != hipSuccess)
        return nb_fail(hip_code(e), "nb_debug_fast_inv_sqrt: allocation: %s", hipGetErrorString(e));
    memcpy(host, x, n * sizeof(float));
    if ((e = hipMemcpy(dx, host, n * sizeof(float), hipMemcpyHostToDevice)) == hipSuccess) {
        quake_rsqrt_array<<<(unsigned)((n + BLOCK - 1) / BLOCK), BLOCK>>>(dx, ds, dp, (uint32_t)n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(host + n, ds, n * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(host + 2 * n, dp, n * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return nb_fail(hip_code(e), "nb_debug_fast_inv_sqrt: %s", hipGetErrorString(e));
    memcpy(y_scalar, host + n, n * sizeof(float));
    memcpy(y_packed, host + 2 * n, n * sizeof(float));
    return NB_OK;
}

// Test hook: move the handle's item-ticket counters (device) and the host's record of them to `value`, as if the launches so far
// had drawn that many items — so that a test can step a handle ACROSS the 2^32 wrap of the counters (580 000 steps away at
// N = 262 144) in a few steps.
extern "C" int nb_debug_ticket_seed(nb_sim *s, uint32_t value)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_debug_ticket_seed: NULL handle");
    if (!s->sym_ticket) return nb_fail(NB_ESTATE, "nb_debug_ticket_seed: the handle has no symmetric plan");
    if (bind(s)) return NB_EHIP;
    if (s->aux) HIPCHK(hipStreamSynchronize(s->aux));
    HIPCHK(hipStreamSynchronize(s->stream));
    uint32_t words[3 * 32];
    memset(words, 0, sizeof words);
    for (int k = 0; k < 3; ++k) { words[k * 32] = value; s->sym_ticket_base[k] = value; }
    HIPCHK(hipMemcpy(s->sym_ticket, words, sizeof words, hipMemcpyHostToDevice));
    return NB_OK;
}
#endif

extern "C" int nb_sym_plan_info(const nb_sim *s, nb_sym_info *out)
{
    if (!s || !out) return nb_fail(NB_EINVAL, "nb_sym_plan_info: NULL argument");
    if (out->struct_size != sizeof(nb_sym_info)) return nb_fail(NB_EINVAL, "nb_sym_plan_info: out->struct_size %u != %zu", out->struct_size, sizeof(nb_sym_info));
    if (symmetric(s)) *out = s->sym_info;
    else { memset(out, 0, sizeof *out); out->struct_size = (uint32_t)sizeof(nb_sym_info); out->cus = (uint32_t)s->cus; }
    return NB_OK;
}

extern "C" int nb_describe(nb_sim *s, char *buf, size_t buflen)
{
    if (!s || !buf || !buflen) return nb_fail(NB_EINVAL, "nb_describe: NULL argument");
    const ForceJob &a = s->job_all;
    const bool seq = s->p.sum_order == NB_SUM_SEQUENTIAL;
    const char *resolve = "none";
    if (s->collide) {
        if (bind(s) || collide_read(s)) return nb_last_error_code();     // the last step's record (an overflow stays unreported)
        resolve = s->coll.host->touched == 0 ? "none" : s->coll.host->lds_last ? "lds" : "global";
    }
    int used = snprintf(buf, buflen,
             "n=%zu owned=[%zu,+%zu) %s%s rsqrt=%s sum=%s | force: block=%d waves/i-set=%d i/lane=%d i_tiles=%u j_slices(all)=%u grid=%u tile_j=%d | "
             "two-phase P/slices local=%d/%u remote=%d/%u | uniform_mass=%d mass_scaled=%d mass_scaling_check=%.1e | symmetric=%d tile=%u chunk_pairs=%d items=%u chunks/item=%u late=%u slabs=%.1f+%.1f MiB | CUs=%d",
             s->n, s->i_begin, s->i_count, s->fp64 ? "fp64" : "fp32", s->dims3 ? " 3-D" : "",
             s->p.rsqrt_mode == NB_RSQRT_QUAKE ? "quake" : "exact", seq ? "sequential" : "tiled",
             BLOCK, (seq || s->fp64) ? 1 : TILED_F32_WS, seq ? 1 : (s->fp64 ? a.P : 2 * a.P), a.i_tiles, a.js,
             seq ? a.i_tiles : grid_blocks(a.i_tiles, a.js), TJ,
             s->job_local.P, s->job_local.js, s->job_remote.P, s->job_remote.js, (int)s->uniform_mass, (int)s->mass_scaled, (double)s->mass_scaling_dev,
             (int)symmetric(s), s->sym_sb, (int)sym_uses_pairs(s), s->sym_items, s->sym_L, s->sym_items_late,
             (double)s->sym_info.slab_s_bytes / 1048576.0, (double)s->sym_info.slab_r_bytes / 1048576.0, s->cus);
    if (used >= 0 && (size_t)used < buflen) {       // the order the symmetric launch sweeps the bodies in: the Morton curve / its re-sort cadence, or the caller's
        if (s->ord.on) used += snprintf(buf + used, buflen - (size_t)used, " order=morton/%u", s->ord.every);
        else used += snprintf(buf + used, buflen - (size_t)used, " order=0");
    }
    if (used >= 0 && (size_t)used < buflen)
        snprintf(buf + used, buflen - (size_t)used, " | collide=%d h=%.6g large=%u capacity=%llu resolve=%s", (int)s->collide, s->coll.h,
                 s->coll.large_n, (unsigned long long)s->coll.cap, resolve);
    const size_t len = strlen(buf);
    if (len < buflen) {
        if (s->tree) snprintf(buf + len, buflen - len, " | force=tree theta=%.6g node_capacity=%llu depth_cap=%d%s%s%s", (double)s->p.theta,
                              (unsigned long long)s->bh.cap, TREE_DEPTH_CAP,
                              !s->bh.leaves ? "" : tree_walk_is_group(s) ? " leaves=1 walk=group" : " leaves=1 walk=lane",
                              s->bh.quad ? " quad=1" : "", s->bh.energy ? " energy=tree" : "");
        else snprintf(buf + len, buflen - len, " | force=direct");
        const size_t len2 = strlen(buf);
        if (s->bh.rel && len2 < buflen) snprintf(buf + len2, buflen - len2, " alpha=%.6g", (double)s->bh.alpha);
        const size_t len3 = strlen(buf);
        if (composed_name(s->p.integrator) && len3 < buflen)
            snprintf(buf + len3, buflen - len3, " integrator=%s", s->p.integrator == NB_INTEGRATOR_DKD ? "dkd" : "fr4");
        else if (hermite(s) && len3 < buflen) snprintf(buf + len3, buflen - len3, " integrator=hermite4");
    }
    return NB_OK;
}
