// nb_sim.hip.h — the handle behind the C ABI, and what every piece of host code around it needs: the HIP error check, the
// device binding, the dispatchers from run-time choices to template arguments.  Included by nb_capi.hip (the one device
// translation unit) ahead of the host sides of the subsystems, nb_collide_host.hip.h, nb_tree_host.hip.h, nb_raster_host.hip.h,
// nb_potential_host.hip.h, nb_neighbors_host.hip.h, nb_groups_host.hip.h, nb_group_catalog_host.hip.h, nb_group_binding_host.hip.h, nb_pair_counts_host.hip.h,
// nb_profiles_host.hip.h, nb_field_host.hip.h, nb_hermite_host.hip.h and nb_order_host.hip.h.
#pragma once
#include "nbody.h"
#include "nbody_debug.h"
#include "nb_internal.h"
#include "nb_kernels.hip.h"
#include "nb_collide.hip.h"
#include "nb_tree.hip.h"
#include "nb_raster.hip.h"
#include "nb_potential.hip.h"
#include "nb_neighbors.hip.h"
#include "nb_groups.hip.h"
#include "nb_group_catalog.hip.h"
#include "nb_group_binding.hip.h"
#include "nb_pair_counts.hip.h"
#include "nb_profiles.hip.h"
#include "nb_field.hip.h"
#include "nb_hermite.hip.h"
#include "nb_order.hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include <unistd.h>

#include "nb_mem.h"

using namespace nbk;

// ---- errors (the thread-local error text / code and nb_params_default live in nb_host.c: plain C, shared with the CPU-only build) ----
static int hip_code(hipError_t e) { return e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation ? NB_ENOMEM : NB_EHIP; }

#define HIPCHK(call)                                                                  \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess)                                                         \
            return nb_fail(hip_code(e_), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// ---- handle ----
// j_begin/j_end are virtual indices that skip [gap_begin, gap_begin + gap_len)
struct ForceJob { uint32_t j_begin, j_end, js, slab0; int P; uint32_t i_tiles; uint32_t gap_begin, gap_len; };

// How a handle computes a step: chosen once by nb_create (step_path_of) and never changed.
enum class StepPath {
    SYM,              // the whole system on this handle, symmetric kernel (force_sym_*)
    SYM_SHARDED,      // symmetric, this rank's share of the pairs; the host reduce-scatters acc_full into acc_owned
    SYM_REPLICATED,   // symmetric, this rank's share of the pairs; the host all-reduces acc_full and every rank integrates all n
    TWO_PHASE,        // one-sided, sharded: the owned j-block first (beside the exchange), then the rest
    ONE_SIDED,        // one-sided over job_all
};

// the pool's backend: the only callers of the HIP allocator besides nb_host_alloc / nb_host_free
struct HipMem {
    using error = hipError_t;
    static constexpr error ok = hipSuccess, misuse = hipErrorInvalidValue;
    static error device(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static error pinned(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free_device(void *p) { (void)hipFree(p); }
    static void free_pinned(void *p) { (void)hipHostFree(p); }
};

struct nb_sim {
    nb_params p;
    size_t n = 0, i_begin = 0, i_count = 0;
    int dev = 0;
    int cus = 256;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool fp64 = false;
    bool dims3 = false;        // 3-D variant: real4 {x,y,z,m} positions, real4 velocities / accelerations / slabs
    size_t rsz = 4;            // sizeof(real)
    size_t esz = 8;            // bytes of one position / velocity / acceleration / slab element

    void *pos[2] = {nullptr, nullptr};
    bool own_pos = true;
    size_t pos_rows = 0;       // rows each replica holds (>= n: padded to world * ceil(n / world) for a sharded handle)
    int cur = 0;
    void *mass = nullptr;
    float *radius = nullptr;
    void *vel = nullptr, *acc = nullptr;
    void *partial = nullptr;
    uint32_t slabs_cap = 0;
    BodyRec *aos_dev = nullptr;     // n records (upload) / i_count records (sync)
    void *staging = nullptr;        // pinned host, i_count * 64 B
    void *bounce = nullptr;         // pinned host bounce ring (BOUNCE_SLOTS x BOUNCE_SLOT_BYTES): pageable caller memory never reaches HIP
    hipEvent_t ev_bounce[4] = {nullptr, nullptr, nullptr, nullptr};   // one per slot / per staged piece
    double *ered_dev = nullptr;     // energy partials
    double *pred_dev = nullptr;     // momentum partials (nb_momentum), allocated on first use
    double *phi_dev = nullptr;      // i_count potentials (nb_potentials), allocated on first use
    size_t ered_blocks = 0;

    // launch geometry (per job: particles per lane and j-slices)
    ForceJob job_all{}, job_local{}, job_remote{};
    uint32_t slabs_all = 0, slabs_two_phase = 0;

    uint64_t frame = 0;
    float pending_dt = 0.f;
    bool in_step = false;
    bool mid_done = false;          // symmetric sharded protocol: nb_step_mid has run for the step in flight
    bool acc_valid = false;         // KDK: acc holds a(x_cur)
    bool uniform_mass = false;      // every body has the same mass: the per-pair mass multiply is hoisted
    float um_mass = 0.f;
    bool sym_pairs = false;         // the symmetric plan has even chunk counts (want_pairs); sym_uses_pairs decides the kernel
    bool mass_scaled = false;       // individual masses folded into the pair geometry (MM_SCALED, nb_kernels.hip.h)
    float *sigma = nullptr;         // m^(-1/2) per particle, for mass_scaled
    float mass_scaling_dev = -1.0f; // what the upload-time check measured: max |a_scaled - a_general| / max |a_general| (-1: not measured)

    StepPath path = StepPath::ONE_SIDED;
    // symmetric paths (force_sym_f32): work items and its two slab sets
    uint32_t sym_items = 0, sym_items_local = 0, sym_items_cross = 0, sym_items_late = 0;   // [local | cross | late]
    uint32_t sym_tiles = 0, sym_rows = 0, sym_L = 0, sym_cov_late_off = 0;
    uint32_t sym_sb = SYM_SB, sym_sb_shift = 11;   // particles per block-tile of the plan: 2048 (classic) or 512 (wave-split kernels)
    SymItem *sym_items_dev = nullptr;          // local items first, then the cross-block items
    uint32_t *sym_rowbase_dev = nullptr;       // 3 x tiles: first row / first late row / end row of every tile
    uint32_t *sym_cov_begin_dev = nullptr;     // 2 x (tiles + 1): coverage-list bounds of the main and the late gather
    SymCov *sym_cov_dev = nullptr;             // coverage entries: main lists, then (from sym_cov_late_off) the late ones
    nb_sym_info sym_info{};
    void *sym_slab_s = nullptr, *sym_slab_r = nullptr;       // float2 / double2 by precision
    bool broken = false;                       // a force launch was refused by the runtime: every later step returns NB_ESTATE
    // dynamic item tickets of the whole-system symmetric launch (sym_item_index, nb_kernels.hip.h)
    uint32_t *sym_ticket = nullptr;            // device: one counter on a line of its own, monotonic modulo 2^32
    uint32_t sym_ticket_base[3] = {0, 0, 0};   // what the launches so far have drawn, per launch kind (local or whole | cross | late: one counter each,
                                               // 128 bytes apart — a sharded rank's launches may run side by side)
    uint32_t sym_first_wave = 0;               // workgroups that keep their static item (the resident slots of the kernel variant); 0 = not yet known
    bool sym_first_wave_uniform = false, sym_first_wave_scaled = false;   // the mass model of the instantiation it was asked for (do_upload resets it on a change)
    // SYM_SHARDED: this rank holds the items of the tiles dealt to it.  SYM_REPLICATED (NB_FLAG_SHARD_ALLREDUCE): the handle
    // holds this rank's share of the pairs like a sharded one, but integrates ALL n particles itself after the host has
    // all-reduced the partial accelerations: one collective per step, every rank keeps the whole (bit-identical) state
    void *acc_full = nullptr, *acc_owned = nullptr;     // reduce-scatter input (n) / output (i_count), (ax,ay) reals
    bool own_acc = true;
    // the local items run on a side stream so that their tail and the head of the cross items share the chip
    // and the late items run there while the reduce-scatter is in flight
    // pipelined snapshot (nb_snapshot_begin / _wait): D2H on its own stream, beside the steps that follow
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_packed = nullptr, ev_copied = nullptr;
    nb_body *snap_out = nullptr;
    bool snap_direct = false, snap_pending = false;
    hipStream_t aux = nullptr;
    bool aux_local = false;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_late = nullptr;
    hipEvent_t ev_x[2] = {nullptr, nullptr};   // in-process exchanges: fences between the handles' streams
    uint64_t peers_enabled = 0;                // devices whose memory this handle's device has mapped

    MemPool<HipMem> pool;                      // every device / page-locked block of the handle (not the caller's pos_buffers / acc_buffers)

    // the query calls (nb_tree_nodes, nb_raster, nb_neighbors, nb_groups) share one page-locked staging buffer for destinations the
    // library does not know to be page-locked: one plane at a time goes through it, and every copy-out blocks (query_stage, nb_capi.hip)
    void *qstage = nullptr;
    size_t qstage_cap = 0;                     // bytes it holds: the largest plane any of them had to stage

    // hard-sphere collisions (NB_EXTRA_COLLIDE, nb_collide.hip.h): nothing in `coll` is allocated when the bit is off
    bool collide = false;
    struct Collide {
        double h = 0.0;                        // grid cell size: a little over twice the largest small radius
        uint32_t large_n = 0;                  // large bodies (tested against all n), <= COLLIDE_MAX_LARGE
        uint32_t slots = 0;                    // cell table slots (power of two >= 2n)
        uint32_t words = 0;                    // 32-body words of one large body's bitmap
        uint64_t cap = 0;                      // pair capacity
        uint64_t ovf_reported = 0;             // overflow steps already reported by a synchronising call
        uint8_t *large = nullptr;              // n flags: 1 = large body
        uint32_t *large_list = nullptr;        // COLLIDE_MAX_LARGE body indices
        int *head = nullptr, *next = nullptr;
        int2 *cell = nullptr;
        uint32_t *deg = nullptr, *off = nullptr, *tidx = nullptr, *tlist = nullptr;
        uint32_t *adj = nullptr, *bits = nullptr;
        uint64_t *chunk_e = nullptr;           // the scan's per-chunk sums / prefixes (collide_scan_*)
        uint32_t *chunk_t = nullptr;
        void *spos = nullptr, *svel = nullptr; // global-memory resolution: touched bodies' state
        uint32_t *scur = nullptr;
        uint8_t *sadv = nullptr;
        CollideStats *stats = nullptr;         // device
        CollideStats *host = nullptr;          // page-locked mirror
    } coll;

    // Barnes-Hut force (NB_FORCE_TREE, nb_tree.hip.h): nothing in `bh` is allocated for a direct-sum handle
    bool tree = false;
    struct BarnesHut {
        float theta2 = 1.0f;                   // theta * theta, Quadtree.hpp:18
        bool leaves = false;                   // NB_FLAG_TREE_LEAVES: leaves that are not accepted contribute
        bool quad = false;                     // NB_FLAG_TREE_QUADRUPOLE: accepted branches add their second moment
        bool energy = false;                   // NB_FLAG_TREE_ENERGY: nb_energy walks the tree (ered_dev then holds 4 x ered_blocks)
        bool rel = false;                      // NB_FLAG_TREE_RELATIVE: the walks also test m size^2 < alpha |a_prev| d^4 (nb_tree_alpha)
        float alpha = 0.005f;                  // GADGET-2's customary setting; 0 switches the test off
        uint64_t cap = 0;                      // node capacity: nodes allocated
        uint64_t ovf_reported = 0;             // failed evaluations already reported by a synchronising call
        uint64_t *k64[4] = {nullptr, nullptr, nullptr, nullptr};   // key words by body: high, low; two sort buffers
        uint32_t *v32[3] = {nullptr, nullptr, nullptr};            // body indices: identity, after the low-word sort, sorted
        uint32_t *head = nullptr;                                  // n + 1: key starts ...
        uint64_t *uidx = nullptr;                                  // ... and their prefix sum
        uint64_t *uhi = nullptr, *ulo = nullptr;                   // keys of the points (different positions)
        uint32_t *ufirst = nullptr;                                // first sorted position of every point
        uint32_t *cnt = nullptr;                                   // n + 2: nodes per point ...
        uint64_t *base = nullptr;                                  // ... and their prefix sum (64-bit: 440 nodes per point x 2^31 bodies)
        float4 *part = nullptr;                // bounds partials
        TreeRoot *root_dev = nullptr;
        float4 *nd = nullptr;                  // node records {com.x, com.y, mass, size^2}
        uint32_t *nx = nullptr;                // next: index + subtree size
        uint8_t *dp = nullptr;                 // depth | TREE_BRANCH
        float4 *qm = nullptr;                  // second moments {xx, xy, yy, 0} per node: NB_FLAG_TREE_QUADRUPOLE handles only
        float *lo = nullptr;                   // float64 mass sum - record mass per leaf with bodies: NB_FLAG_TREE_ENERGY handles only
        void *tmp = nullptr;                   // rocprim temporary storage (sort, scan)
        size_t tmp_bytes = 0;
        TreeStats *stats = nullptr;            // device
        TreeStats *host = nullptr;             // page-locked mirror
        // nb_tree_nodes (the export kernels of nb_tree.hip.h): nothing in `exp` exists before the first call; grown by the node count exported
        struct Export {
            uint64_t cap = 0;                  // nodes the four arrays below hold
            nb_tree_node *rec = nullptr;       // the records, 128 B per node (the kernels write them as eight uint4)
            uint32_t *flag = nullptr;          // 1 where a pre-order node is a branch ...
            uint64_t *rank = nullptr;          // ... and the prefix sum: its rank among the branches
            uint32_t *idx = nullptr;           // export index of a pre-order node
            void *tmp = nullptr;               // rocprim temporary storage of that scan (asked for this element count)
            size_t tmp_bytes = 0;
        } exp;
    } bh;

    // nb_raster (nb_raster.hip.h): nothing in `ras` exists before the first call; grown by the largest view seen
    struct Raster {
        uint64_t cap = 0;                      // pixels `cnt` holds
        uint32_t *cnt = nullptr;               // the count plane
        uint64_t mass_cap = 0;                 // pixels `units` and `massf` hold: nothing before the first mass plane
        unsigned long long *units = nullptr;   // mass in quanta, summed as integers
        float *massf = nullptr;                // the mass plane
    } ras;

    // nb_neighbors (nb_neighbors.hip.h): nothing in `nbr` exists before the first call; the tree's key arrays are not borrowed
    struct Neighbors {
        uint64_t cap = 0;                      // bodies the six per-body arrays hold: n from the first call on
        float2 *xy = nullptr, *sxy = nullptr;  // positions rounded to float: by body, in sorted order
        uint64_t *key = nullptr, *skey = nullptr;   // cell keys: by body, sorted
        uint32_t *val = nullptr, *sval = nullptr;   // body indices: identity, in sorted order
        void *tmp = nullptr;                   // rocprim temporary storage of the sort (asked for n pairs)
        size_t tmp_bytes = 0;
        uint32_t *cnt = nullptr;               // i_count counts, once a count is asked for
        uint64_t idx_cap = 0, d2_cap = 0;      // entries (owned bodies x k) the two row planes hold: grown by the largest k seen
        uint32_t *idx = nullptr;
        float *d2 = nullptr;
    } nbr;

    // nb_groups (nb_groups.hip.h): nothing in `grp` exists before the first call; the cells and the sort are `nbr`'s
    struct Groups {
        uint64_t cap = 0;                      // bodies `parent` holds: n from the first call on
        uint32_t *parent = nullptr;            // the union-find by body index; after the flatten pass the labels of all n
        uint32_t *cnt = nullptr;               // n member counts by label, once sizes are asked for ...
        uint32_t *size = nullptr;              // ... and the i_count sizes of the owned block
        uint32_t *words = nullptr;             // device: the fault word, the number of groups
        uint32_t *host = nullptr;              // page-locked mirror of the two
    } grp;

    // nb_group_catalog (nb_group_catalog.hip.h): nothing in `cat` exists before the first call; the labels are `grp`'s, the sort's
    // arrays and storage `nbr`'s (key / skey / val / sval are free again once the link kernel has run)
    struct GroupCatalog {
        uint64_t cap = 0;                      // the three per-body arrays hold cap entries: n + 1 from the first call on
        uint32_t *flag = nullptr;              // 1 at the head of a group that is kept ...
        uint64_t *rank = nullptr;              // ... and the prefix sum: its row; rank[n] is the count
        uint32_t *len_row = nullptr;           // by label: the group's length, then its row (CATALOG_NO_ROW: not kept)
        void *tmp = nullptr;                   // rocprim temporary storage of the scan (asked for n + 1 elements)
        size_t tmp_bytes = 0;
        uint64_t slot_cap = 0;                 // carry slots: two per run of CATALOG_RUN sorted positions
        CatalogSlot *slot = nullptr;
        uint64_t rec_cap = 0;                  // groups `sums` and `rec` hold: grown by the count of a filling call, not by n
        CatalogSums *sums = nullptr;
        nb_group *rec = nullptr;
        uint64_t *host = nullptr;              // page-locked: the count
    } cat;

    // nb_group_binding (nb_group_binding.hip.h): nothing in `gbind` exists before the first filling call; groups, sort, rows and means
    // are `cat`'s, and the start of a segment by label lives in cat.flag behind catalog_rows
    struct GroupBinding {
        uint64_t cap = 0;                      // bodies the four per-body arrays hold: n from the first filling call on
        uint2 *seg = nullptr;                  // by sorted position: {start, length} of its segment; length 0: the group is not kept
        double *sphi = nullptr;                // phi by sorted position
        double *phi = nullptr, *e = nullptr;   // the two planes by body
        uint64_t rec_bytes = 0;                // bytes `srec` holds: n j-records in sorted order, 16 B (fp32 handle) or 32 B (fp64)
        void *srec = nullptr;
        uint64_t out_cap = 0;                  // records `out` holds: cat.rec_cap of the largest filling call
        nb_group_energy *out = nullptr;
    } gbind;

    // nb_pair_counts (nb_pair_counts.hip.h): nothing in `pairs` exists before the first call; the cells and the sort are `nbr`'s
    struct PairCounts {
        uint64_t cap = 0;                      // words `partial` holds: 65 per workgroup of the largest count launch seen
        uint64_t *partial = nullptr;           // one row of cumulative 64-bit counters per workgroup
        uint64_t *words = nullptr;             // device: the 65 cumulative counters, the rows added up
        uint64_t *host = nullptr;              // page-locked mirror of them
    } pairs;

    // nb_radial_profiles (nb_profiles.hip.h): nothing in `prf` exists before the first call; the cells and the sort are `nbr`'s
    struct Profiles {
        uint64_t cap = 0;                      // entries the seven per-centre arrays hold: ncenters + 1 of the largest call seen
        ProfileCentre *cen = nullptr;          // the centres as passed, `dims` floats each, packed
        ProfileVelocity *vcen = nullptr;       // their velocities, `dims` doubles each, packed
        ProfileRanges *rng = nullptr;          // the three key ranges of a centre
        uint32_t *pieces = nullptr, *split = nullptr;   // pieces of a centre; the same where it is more than one, else 0
        uint64_t *first = nullptr, *prow = nullptr;     // their exclusive scans: a centre's first piece, its first partial row
        void *tmp = nullptr;                   // rocprim temporary storage of the scans (asked for cap elements)
        size_t tmp_bytes = 0;
        uint64_t out_cap = 0;                  // records `out` holds: the largest ncenters x nbins seen
        nb_shell *out = nullptr;
        uint64_t part_cap = 0;                 // records `partial` holds: nbins per piece of the split centres of the largest call seen
        nb_shell *partial = nullptr;
        uint64_t *host = nullptr;              // page-locked: the two totals
    } prf;

    // nb_field (nb_field.hip.h): nothing in `fld` exists before the first call; one block, grown by the largest npoints seen
    struct Field {
        uint64_t bytes = 0;                    // bytes `buf` holds: 8 (dims + 1) + 4 dims per point
        void *buf = nullptr;                   // the call's phi plane, then its acc plane, then its points
    } fld;

    // NB_INTEGRATOR_HERMITE4 (nb_hermite.hip.h): nothing in `herm` is allocated for a handle of another integrator
    struct Hermite {
        bool valid = false;                    // acc[] and jerk hold the carried pair (a0, j0): false after nb_create / nb_upload
        void *jerk = nullptr;                  // the carried jerk, one vec per body
        void *vpred = nullptr;                 // the predicted velocities, one vec per body (the predicted positions go to pos[cur ^ 1])
        double *rows = nullptr;                // the evaluation's rows: the acc plane, then the jerk plane, dims doubles per body each
    } herm;

    // body order of the whole-system symmetric path (nb_order.hip.h): nothing in `ord` is allocated unless `on`
    struct Order {
        bool on = false;
        uint32_t every = NB_ORDER_EVERY;       // force evaluations from one sort to the next
        uint64_t evals = 0;                    // force evaluations since the last upload: a sort goes ahead of every `every`-th
        uint32_t *perm = nullptr, *val = nullptr;   // sorted position -> body index; the identity the sort permutes
        uint64_t *key = nullptr, *skey = nullptr;   // keys by body, sorted
        void *part = nullptr;                  // ORDER_PARTS partial boxes, 4 reals each
        void *xs = nullptr, *ms = nullptr;     // positions (every evaluation) and masses (every sort; individual masses only) in sorted order
        float *sigma_s = nullptr;              // sigma in sorted order, where the handle has a sigma
        void *tmp = nullptr;                   // rocprim temporary storage of the sort (asked for n pairs)
        size_t tmp_bytes = 0;
    } ord;

    // profiling
    bool prof = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool, ev_used;
    std::vector<uint32_t> ev_weight;           // force passes each used event pair brackets (a pipeline launch: its steps)
    double prof_ms = 0.0;
    uint64_t prof_launches = 0;
};

static int bind(const nb_sim *s)
{
    int d = -1;
    HIPCHK(hipGetDevice(&d));
    if (d != s->dev) HIPCHK(hipSetDevice(s->dev));
    return NB_OK;
}

// ---- dispatch: run-time choices -> template arguments ----
// f(Layout<...>{}) for the handle's precision and dimensionality: the one place that maps them to types.
template <typename F>
static auto with_layout(const nb_sim *s, F &&f)
{
    if (s->dims3) return s->fp64 ? f(Layout<double, true>{}) : f(Layout<float, true>{});
    return s->fp64 ? f(Layout<double, false>{}) : f(Layout<float, false>{});
}

// f(std::bool_constant<b>...) for the run-time flags b...
template <typename F>
static auto with_flags(F &&f) { return f(); }

template <typename F, typename... B>
static auto with_flags(F &&f, bool b, B... rest)
{
    if (b) return with_flags([&](auto... c) { return f(std::true_type{}, c...); }, rest...);
    return with_flags([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

// f(std::integral_constant<int, P>{}) for P in {1, 2, 4}; PMAX = 2 for the fp64 kernels, which have no P = 4.
template <int PMAX, typename F>
static auto with_lanes(int P, F &&f)
{
    if constexpr (PMAX >= 4)
        if (P == 4) return f(std::integral_constant<int, 4>{});
    if (P == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 1>{});
}

// ---- defined in nb_capi.hip below the subsystems' host code, which uses them (as it does copy_h2d / copy_d2h / pinned_covers and the
// query calls' query_enter / check_radius / stage_need / query_stage / copy_plane above it) ----
static int prof_begin(nb_sim *s, std::pair<hipEvent_t, hipEvent_t> *pr, hipStream_t st = nullptr);
static int prof_end(nb_sim *s, const std::pair<hipEvent_t, hipEvent_t> &pr, hipStream_t st = nullptr, uint32_t passes = 1);
static int step_check(nb_sim *s);       // what every synchronising call reports once: a collision step over capacity, a failed tree build
