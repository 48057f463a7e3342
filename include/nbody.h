/* include/nbody.h — C ABI of libnbody_hip.so, the MI355X (gfx950) drop-in for the
 * reference's pairwise-gravity + kick/drift path.
 *
 * The reference (7IBBE77S/nbodysim, paths relative to Nbodysim/) has no FFI: its
 * boundary is the public surface of `class Simulation`
 * (headers/Simulation.hpp:49-75): a constructor, `void step()`, and the public
 * `std::vector<Body> bodies`, driven by one caller, `simulation_thread`
 * (source/main.cpp:612-635).  Every entry point below names the piece of that
 * surface it replaces.  Plain C types only: pointers, sizes, scalars.
 *
 * Error convention (the reference has none — void returns, no exceptions):
 * int-returning functions give 0 on success and a negative NB_E* code on
 * failure; pointer-returning functions give NULL; nb_last_error() holds the
 * text and nb_last_error_code() the NB_E* code of the last failure on the
 * calling thread (so a NULL from nb_create still tells NB_ENODEVICE from
 * NB_ENOMEM from NB_EINVAL).  A handle is not thread-safe (the reference's
 * Simulation is single-caller too, main.cpp:621).
 *
 * There is NO CPU fallback: without a HIP device nb_create() fails with
 * NB_ENODEVICE.  The library reads NO environment variables: every switch is a
 * field of nb_params.
 */
#ifndef NBODY_H
#define NBODY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: what this header declares is ALL it exports (`nm -D` shows exactly these
 * nb_* symbols; tests/test_abi.py).  Test hooks live in include/nbody_debug.h and exist only in a -DNB_TEST_HOOKS build. */
#pragma GCC visibility push(default)

#define NB_ABI_VERSION 8

/* ---- particle record -------------------------------------------------------
 * Bit-compatible with the reference's `struct alignas(16) Body`
 * (headers/Body.hpp:6-13) built on `struct alignas(16) Vec2 {float x, y;}`
 * (headers/Vec2.hpp:17-20).  The source comments claim 32 bytes; the real
 * sizeof is 64 because each Vec2 is padded to 16 (measured with g++ 11.4 and
 * clang 22 — tests/golden/layout.json).  Padding is indeterminate in the
 * reference (Vec2's copy-ctor copies x,y only, Vec2.hpp:26); this library
 * always writes it as zero and never reads it. */
typedef struct nb_vec2 {
    float x, y;
    float _pad[2];
} nb_vec2;

/* z component of a 3-D handle (nb_params.dims = 3): the 8 bytes of padding that follow y in the
 * reference's alignas(16) Vec2 (Vec2.hpp:17-20). */
#define NB_Z(v) ((v)._pad[0])

typedef struct nb_body {
    nb_vec2 pos;     /* offset  0  Body::pos    */
    nb_vec2 vel;     /* offset 16  Body::vel    */
    nb_vec2 acc;     /* offset 32  Body::acc    */
    float   mass;    /* offset 48  Body::mass   */
    float   radius;  /* offset 52  Body::radius (carried, unused by gravity) */
    float   _pad[2];
} nb_body;

#if defined(__cplusplus)
static_assert(sizeof(nb_vec2) == 16, "Vec2 is 16 bytes (Vec2.hpp:17)");
static_assert(sizeof(nb_body) == 64, "Body is 64 bytes (Body.hpp:6)");
static_assert(offsetof(nb_body, vel) == 16 && offsetof(nb_body, acc) == 32 &&
              offsetof(nb_body, mass) == 48 && offsetof(nb_body, radius) == 52,
              "Body field offsets");
#else
_Static_assert(sizeof(nb_vec2) == 16, "Vec2 is 16 bytes (Vec2.hpp:17)");
_Static_assert(sizeof(nb_body) == 64, "Body is 64 bytes (Body.hpp:6)");
_Static_assert(offsetof(nb_body, vel) == 16 && offsetof(nb_body, acc) == 32 &&
               offsetof(nb_body, mass) == 48 && offsetof(nb_body, radius) == 52,
               "Body field offsets");
#endif

/* ---- tree node record -----------------------------------------------------
 * Bit-compatible with the reference's `struct alignas(32) Node` (headers/Node.hpp:31-53): the anonymous alignas(16)
 * `data` {Vec2 pos; float mass; Quad quad}, Quad = {Vec2 center; float size} (headers/Quad.hpp), then five size_t.
 * sizeof 128, alignof 32 (measured with g++ and clang, -std=c++20 — tests/golden/node_layout.json).  nb_tree_nodes
 * (below) fills these; the library writes every padding byte as zero. */
typedef struct nb_tree_node {
    nb_vec2  pos;           /* offset   0  Node::data.pos: centre of mass (branch) / position (leaf) / (0, 0) (empty quadrant) */
    float    mass;          /* offset  16  Node::data.mass */
    float    _pad0[3];
    nb_vec2  center;        /* offset  32  Node::data.quad.center */
    float    size;          /* offset  48  Node::data.quad.size */
    float    _pad1[3];
    uint64_t children;      /* offset  64  Node::children: index of the first of four consecutive children; 0 = leaf / empty quadrant */
    uint64_t next;          /* offset  72  Node::next: the node a walk goes to when it skips this subtree; 0 = none (the end) */
    uint64_t bodies_start;  /* offset  80  Node::bodies.start: 0 (the reference's leaf ranges are empty) */
    uint64_t bodies_end;    /* offset  88  Node::bodies.end:   0 */
    uint64_t depth;         /* offset  96  Node::depth: 0 for the root */
    uint64_t _pad2[3];      /* tail padding of alignas(32) */
} nb_tree_node;

#if defined(__cplusplus)
static_assert(sizeof(nb_tree_node) == 128, "Node is 128 bytes (Node.hpp:31)");
static_assert(offsetof(nb_tree_node, mass) == 16 && offsetof(nb_tree_node, center) == 32 && offsetof(nb_tree_node, size) == 48 &&
              offsetof(nb_tree_node, children) == 64 && offsetof(nb_tree_node, next) == 72 &&
              offsetof(nb_tree_node, bodies_start) == 80 && offsetof(nb_tree_node, bodies_end) == 88 &&
              offsetof(nb_tree_node, depth) == 96,
              "Node field offsets");
#else
_Static_assert(sizeof(nb_tree_node) == 128, "Node is 128 bytes (Node.hpp:31)");
_Static_assert(offsetof(nb_tree_node, mass) == 16 && offsetof(nb_tree_node, center) == 32 && offsetof(nb_tree_node, size) == 48 &&
               offsetof(nb_tree_node, children) == 64 && offsetof(nb_tree_node, next) == 72 &&
               offsetof(nb_tree_node, bodies_start) == 80 && offsetof(nb_tree_node, bodies_end) == 88 &&
               offsetof(nb_tree_node, depth) == 96,
               "Node field offsets");
#endif

/* ---- group record ---------------------------------------------------------
 * One friends-of-friends group as nb_group_catalog (below) reports it.  80 bytes, no padding. */
typedef struct nb_group {
    uint32_t label;         /* offset   0  smallest global body index of the group: nb_groups' label */
    uint32_t members;       /* offset   4  bodies in the group: nb_groups' size */
    double   mass;          /* offset   8  M = sum w_i */
    double   pos[3];        /* offset  16  centre of mass, sum w_i x_i / W;  [2] = 0 on a 2-D handle */
    double   vel[3];        /* offset  40  sum w_i v_i / W */
    double   sigma2;        /* offset  64  sum w_i |v_i - vel|^2 / W: velocity dispersion */
    double   r_max;         /* offset  72  max_i |x_i - pos|: the radius that holds the group */
} nb_group;

#if defined(__cplusplus)
static_assert(sizeof(nb_group) == 80, "nb_group is 80 bytes");
static_assert(offsetof(nb_group, members) == 4 && offsetof(nb_group, mass) == 8 && offsetof(nb_group, pos) == 16 &&
              offsetof(nb_group, vel) == 40 && offsetof(nb_group, sigma2) == 64 && offsetof(nb_group, r_max) == 72,
              "nb_group field offsets");
#else
_Static_assert(sizeof(nb_group) == 80, "nb_group is 80 bytes");
_Static_assert(offsetof(nb_group, members) == 4 && offsetof(nb_group, mass) == 8 && offsetof(nb_group, pos) == 16 &&
               offsetof(nb_group, vel) == 40 && offsetof(nb_group, sigma2) == 64 && offsetof(nb_group, r_max) == 72,
               "nb_group field offsets");
#endif

/* ---- shell record ----------------------------------------------------------
 * One shell about one centre as nb_radial_profiles (below) reports it.  64 bytes, no padding.  w = m > 0 ? m : 0; r, v_r, u and the
 * l_z term are defined there. */
typedef struct nb_shell {
    uint64_t count;         /* offset   0  bodies in the shell, massless ones included */
    double   mass;          /* offset   8  sum w */
    double   mr;            /* offset  16  sum w r */
    double   mr2;           /* offset  24  sum w r^2 */
    double   mvr;           /* offset  32  sum w v_r */
    double   mvr2;          /* offset  40  sum w v_r^2 */
    double   mv2;           /* offset  48  sum w |u|^2 */
    double   mlz;           /* offset  56  sum w (dx u_y - dy u_x) */
} nb_shell;

#if defined(__cplusplus)
static_assert(sizeof(nb_shell) == 64, "nb_shell is 64 bytes");
static_assert(offsetof(nb_shell, mass) == 8 && offsetof(nb_shell, mr) == 16 && offsetof(nb_shell, mr2) == 24 && offsetof(nb_shell, mvr) == 32 &&
              offsetof(nb_shell, mvr2) == 40 && offsetof(nb_shell, mv2) == 48 && offsetof(nb_shell, mlz) == 56,
              "nb_shell field offsets");
#else
_Static_assert(sizeof(nb_shell) == 64, "nb_shell is 64 bytes");
_Static_assert(offsetof(nb_shell, mass) == 8 && offsetof(nb_shell, mr) == 16 && offsetof(nb_shell, mr2) == 24 && offsetof(nb_shell, mvr) == 32 &&
               offsetof(nb_shell, mvr2) == 40 && offsetof(nb_shell, mv2) == 48 && offsetof(nb_shell, mlz) == 56,
               "nb_shell field offsets");
#endif

/* ---- group energy record --------------------------------------------------
 * One friends-of-friends group as nb_group_binding (below) reports it: row r describes the group of row r of nb_group_catalog.
 * 32 bytes, no padding. */
typedef struct nb_group_energy {
    uint32_t label;         /* offset   0  nb_group_catalog's label */
    uint32_t members;       /* offset   4  nb_group_catalog's members */
    uint32_t bound;         /* offset   8  members with e < 0 */
    uint32_t most_bound;    /* offset  12  global index of the member with the smallest e; NB_NO_NEIGHBOR if no member's e compares */
    double   e_min;         /* offset  16  its e; +inf with NB_NO_NEIGHBOR */
    double   potential;     /* offset  24  U = 1/2 sum w_i phi[i] over the members: the group's self-potential energy */
} nb_group_energy;

#if defined(__cplusplus)
static_assert(sizeof(nb_group_energy) == 32, "nb_group_energy is 32 bytes");
static_assert(offsetof(nb_group_energy, members) == 4 && offsetof(nb_group_energy, bound) == 8 && offsetof(nb_group_energy, most_bound) == 12 &&
              offsetof(nb_group_energy, e_min) == 16 && offsetof(nb_group_energy, potential) == 24,
              "nb_group_energy field offsets");
#else
_Static_assert(sizeof(nb_group_energy) == 32, "nb_group_energy is 32 bytes");
_Static_assert(offsetof(nb_group_energy, members) == 4 && offsetof(nb_group_energy, bound) == 8 && offsetof(nb_group_energy, most_bound) == 12 &&
               offsetof(nb_group_energy, e_min) == 16 && offsetof(nb_group_energy, potential) == 24,
               "nb_group_energy field offsets");
#endif

/* ---- enums ---------------------------------------------------------------- */
enum { NB_OK = 0, NB_EINVAL = -1, NB_ENODEVICE = -2, NB_EHIP = -3, NB_ENOMEM = -4,
       NB_EIO = -5, NB_EFORMAT = -6, NB_ESTATE = -7 };

/* arithmetic type of the device path */
enum { NB_FP32 = 0,   /* the reference's type (everything is float, Vec2.hpp:20) */
       NB_FP64 = 1 }; /* build extension (BASELINE config 5) */

/* inverse square root flavour */
enum { NB_RSQRT_EXACT = 0,   /* hardware v_rsq_f32 (fp32) / 1/sqrt (fp64): headline mode */
       NB_RSQRT_QUAKE = 1 }; /* Quadtree::fast_inv_sqrt, Quadtree.hpp:106-111: reference arithmetic */

/* order in which one particle's j-terms are summed */
enum { NB_SUM_TILED = 0,       /* LDS-tiled, packed FP32, FMA-contracted: fast path */
       NB_SUM_SEQUENTIAL = 1 };/* j ascending, one running sum, no FMA — the order of
                                  Quadtree.hpp:134-144; with NB_RSQRT_QUAKE this is
                                  bit-identical to the compiled reference */

/* nb_params.extras bit flags: the non-gravity parts of Simulation::iterate */
enum { NB_EXTRA_VCLAMP   = 1,   /* |v| <= 1000,            Simulation.hpp:133-137 */
       NB_EXTRA_BOUNDARY = 2,   /* soft boundary + damping, Simulation.hpp:140-155 */
       NB_EXTRA_COLLIDE  = 4 }; /* hard-sphere collisions after the drift, collide() / resolve(), Simulation.hpp:216-346 (ABI 7).
                                   Each step then ends with: P = every pair i < j whose discs overlap at the drifted positions
                                   (d = p_j - p_i, d.x*d.x + d.y*d.y <= (r_i + r_j)^2, one rounding per operation; coincident
                                   bodies count, radius 0 included), fixed first; then the reference's resolve(i, j) once per pair
                                   of P in ascending (i, j) order, each on the current state of both bodies.  acc is untouched.
                                   Unsharded 2-D kick-drift handles only (nb_create: NB_EINVAL otherwise).  Where no body is in
                                   two pairs and each pair lies in one of the reference's 600-unit cells, the result is the
                                   reference's own step() bit for bit (INTEGRATION.md §2 has the differences otherwise).
                                   Pair capacity: max(8 n, 65536) pairs; a step with more resolves nothing, and the next
                                   synchronising call (nb_wait, nb_sync, nb_sync_positions, nb_snapshot_wait, nb_energy,
                                   nb_momentum, nb_collision_stats) returns NB_ENOMEM once, naming the frame and the pairs
                                   needed; nb_collide_capacity raises it */

/* nb_params.force: how the accelerations are evaluated (ABI 8) */
enum { NB_FORCE_DIRECT = 0,    /* every pair: the kernels this library is built around (default) */
       NB_FORCE_TREE = 1 };    /* the reference's own algorithm: Barnes-Hut quadtree, Quadtree::build / Quadtree::acc
                                  (Quadtree.hpp:35-93,113-170,236-258), opening parameter nb_params.theta.  Per force evaluation:
                                  root cell = Quad::new_containing of all bodies; one position per leaf (coincident bodies share a
                                  leaf, masses added in ascending index); a cell holding two different positions has its four
                                  children; centres of mass summed over the children in quadrant order; every body walks the nodes
                                  in pre-order and adds d * (mass * inv^3) for each node with size^2 < d^2 * theta^2 and d^2 > 0, whose
                                  subtree it then skips; a leaf that is not accepted adds nothing (the reference's leaf ranges are
                                  empty, the body's own leaf included).  With NB_RSQRT_QUAKE the result is the compiled reference's
                                  bit for bit, whatever the order of the bodies; with NB_RSQRT_EXACT the same nodes are accepted and
                                  the term uses the hardware rsqrt and FMA.  A body with mass == 0 is not inserted (it is still
                                  accelerated and integrated); positions must be finite.
                                  Unsharded 2-D fp32 handles of the kick-drift, DKD or FR4 integrator only (nb_create: NB_EINVAL
                                  otherwise, naming the combination); any rsqrt_mode, any extras the integrator takes.  REFUSED with it: NB_FP64, dims = 3, NB_INTEGRATOR_KDK,
                                  shard_world > 1, i_count < n, NB_FLAG_SHARD_SINGLE / _ALLREDUCE, NB_SUM_SEQUENTIAL.  IGNORED with
                                  it (they select or shape the direct-sum launches, none of which a tree handle ever runs; range
                                  checks still apply): NB_FLAG_NO_SYMMETRY, _NO_UNIFORM_MASS, _NO_GUIDED_TAIL, _MASS_SCALING,
                                  _MASS_SCALING_MEASURED, _NO_MASS_SCALING, _STATIC_ITEMS, j_slices, lanes_p, the sym_* tuning fields
                                  and acc_buffers.  Caller-owned pos_buffers are accepted as for any unsharded handle.
                                  Device memory is O(n): no symmetric plan, slabs or partials.  Node capacity 16 n + 4096, paths are
                                  followed for 63 levels; an evaluation that needs more integrates nothing (positions and velocities
                                  stay; with NB_EXTRA_COLLIDE the collision pass of that step still runs, on the unchanged
                                  positions), and the next synchronising call (nb_wait, nb_sync, nb_sync_positions, nb_energy,
                                  nb_momentum, nb_tree_stats, nb_tree_nodes) returns NB_ENOMEM once, naming the frame and what was needed.
                                  nb_momentum stays the exact O(n) diagnostic.  nb_energy is the exact O(n^2) fp64 pair sweep of a
                                  direct-sum handle (at the sizes the tree exists for one reading costs as much as many steps)
                                  unless the handle has NB_FLAG_TREE_ENERGY (flags, below): it then walks the tree, O(n log n) */

/* integrator */
enum { NB_INTEGRATOR_KICK_DRIFT = 0, /* Simulation.hpp:129-131,160-163 (reference) */
       NB_INTEGRATOR_KDK = 1,        /* kick-drift-kick leapfrog (build extension) */
       /* Compositions of a leading drift and stages (force at the current x; v += a k h; x += v d h) — one step of size h:
            DKD   drift 1/2;      stage (1, 1/2):  second order, time-reversible, x and v synchronised, ONE force evaluation per step
            FR4   drift theta/2;  stages (theta, (1 - theta)/2), (1 - 2 theta, (1 - theta)/2), (theta, theta/2) with
                  theta = 1 / (2 - 2^(1/3)): Forest-Ruth, fourth order, three force evaluations per step
          Every coefficient * h is formed in double from the float h that nb_step resolved and rounded once to the handle's real.
          nb_frame grows by 1 per step; acc[] is the last stage's evaluation; every step is self-contained (nb_step(1) then nb_step(3)
          gives the bits of nb_step(4)).  Every UNSHARDED handle takes them: fp32 and fp64, dims 2 and 3, the symmetric and the
          one-sided path, NB_SUM_SEQUENTIAL, either rsqrt mode, the Morton body order, NB_FORCE_TREE with any of its flags (where a
          stage's build fails, that stage applies neither its kick nor its drift; the leading drift is unconditional).  nb_create
          refuses them (NB_EINVAL, naming both parts) with shard_world > 1, i_count < n, NB_FLAG_SHARD_SINGLE, NB_FLAG_SHARD_ALLREDUCE and
          NB_EXTRA_COLLIDE; FR4 with any extras (its middle kick runs backwards, which the clamp and the damped boundary cannot).
          DKD applies NB_EXTRA_VCLAMP / NB_EXTRA_BOUNDARY in its one kick, at the midpoint position.  nb_step only (nb_step_begin
          refuses them, as it refuses KDK). */
       NB_INTEGRATOR_DKD = 2,        /* drift-kick-drift leapfrog */
       NB_INTEGRATOR_FR4 = 3,        /* Forest-Ruth 4th-order composition */
       /* (4 is unassigned: nb_create refuses it with "bad integrator", like any value outside this enum) */
       /* 4th-order Hermite predictor-corrector (Makino & Aarseth 1992): ONE force evaluation per step, and that evaluation returns
          the acceleration and its time derivative, the jerk, from one sweep over the pairs.  With d = x_j - x_i, dv = v_j - v_i and
          R^2 = d^2 + eps^2, the sums over ALL j:
              a_i = sum_j m_j d / R^3        j_i = sum_j m_j ( dv / R^3 - 3 (d.dv) d / R^5 )
          The pair of a body with itself adds exactly 0 to both sums.  A body on the position of another adds 0 to a and, with
          eps > 0, the formula's m_j dv / eps^3 to j; on handles whose eps^2 is 0 in the sweep's arithmetic a pair with r^2 == 0
          adds exactly 0 to both (1/r is set to 0 before any product, the rule of the one-sided force kernels).
          One step of size h from the state (x, v) and the CARRIED pair (a0, j0):
              predict   x_p = x + v h + a0 h^2/2 + j0 h^3/6        v_p = v + a0 h + j0 h^2/2
              evaluate  (a1, j1) at (x_p, v_p)                                                      one launch
              correct   v1 = v + (a0 + a1) h/2 + (j0 - j1) h^2/12      x1 = x + (v + v1) h/2 + (a0 - a1) h^2/12
              carry     (a0, j0) <- (a1, j1);  acc[] = a1;  nb_frame grows by 1
          h/2, h^2/2, h^3/6 and h^2/12 are formed in double from the float h that nb_step resolved and each rounded once to the
          handle's real.  This is the standard PEC form: the next step starts from the evaluation at the predicted point.  A one-step
          scheme: dt may change on every nb_step call with no loss of order.  The carried pair is state between steps and is INVALID
          after nb_create, nb_upload and nb_accelerations: the first step after any of them first evaluates (a0, j0) at (x, v), so k
          steps on a fresh handle are k + 1 launches and k afterwards.  Hence: nb_step(1) then nb_step(3) gives the bits of
          nb_step(4); two handles of the same bodies agree bit for bit; a handle restarted from nb_dump (or re-uploaded from its own
          nb_sync records) re-evaluates at the CORRECTED state and follows the original run to the scheme's order, NOT bit for bit;
          acc of nb_sync is a1, "the last force evaluation".
          ACCEPTED: unsharded direct-sum handles, fp32 and fp64, dims 2 and 3, the tiled sum, the hardware rsqrt.  Such a handle never
          runs the symmetric kernels: it plans as a one-sided handle, nb_describe says symmetric=0 and ends with " integrator=hermite4".
          IGNORED with it (they shape direct launches it never runs; range checks still apply): NB_FLAG_MASS_SCALING / _MEASURED /
          NB_FLAG_NO_MASS_SCALING, NB_FLAG_NO_UNIFORM_MASS, NB_FLAG_BODY_ORDER / _NO_BODY_ORDER and the sym_* fields.  REFUSED by
          nb_create (NB_EINVAL, naming HERMITE4 and the partner, before a device is looked for): NB_FORCE_TREE, shard_world > 1,
          i_count < n, NB_FLAG_SHARD_SINGLE, NB_FLAG_SHARD_ALLREDUCE, any extras (the clamp, the damped boundary and the collisions are
          not differentiable: there is no jerk of them), NB_SUM_SEQUENTIAL, NB_RSQRT_QUAKE.  nb_step only (nb_step_begin refuses it).
          ARITHMETIC of the evaluation (nb_jerks below returns it): fp32 handles add the terms of 64 consecutive j in float32 and those
          runs in float64, in a fixed order; fp64 handles add in j order.  The order does not depend on timing or launch geometry.
          MEMORY beyond a one-sided handle: a jerk array and a predicted-velocity array of one element each (8 B per body each for fp32
          2-D, 16 B for fp64 2-D and fp32 3-D, 32 B for fp64 3-D) and the evaluation's rows, 16 dims bytes per body. */
       NB_INTEGRATOR_HERMITE4 = 5 };

/* nb_params.flags bit mask: algorithm switches (all 0 = the fast defaults) */
enum { NB_FLAG_NO_SYMMETRY     = 1,   /* one-sided kernels only (every ordered pair evaluated); a sharded
                                         handle then uses the NB_SHARD_ALLGATHER protocol */
       NB_FLAG_NO_UNIFORM_MASS = 2,   /* keep the per-pair mass multiply even when all masses are equal */
       NB_FLAG_NO_GUIDED_TAIL  = 4,   /* symmetric planner: uniform work items (no finer items at the end) */
       NB_FLAG_SHARD_ALLREDUCE = 8,   /* with shard_world > 1 and i_count = n: the NB_SHARD_ALLREDUCE protocol below */
       NB_FLAG_MASS_SCALING    = 32,  /* individual masses, fp32, exact rsqrt, tiled sum, eps > 0: fold the masses into the pair
                                         geometry (nb_kernels.hip.h MM_SCALED: the travelling particle carries m^(-1/2) and its
                                         pre-multiplied position, one multiply less per pair in the symmetric kernel, none at all
                                         in the one-sided one: 2.5 % of kernel time).  The pair displacement is then no longer an exact
                                         difference of two floats (relative error 6e-8 |x_j| / |d| per pair force), and a body's pair with
                                         ITSELF no longer cancels exactly (a spurious self-acceleration of up to 6e-8 |x| m / eps^3; total
                                         momentum is conserved to that level only) — harmless for light, similar masses, several 1e-5 of the
                                         force scale for a broad mass spectrum with close heavy pairs (tests/test_headline_gpu.py).
                                         OFF BY DEFAULT (ABI 6): the same pair arithmetic on one GPU and on N, at t = 0 and later.
                                         THIS BIT: fold wherever representable (m > 0 everywhere, m_max^(3/2) / eps^3 inside the float
                                         range), whatever the data — the caller's decision; the ranks of a sharded run must agree on it */
       NB_FLAG_MASS_SCALING_MEASURED = 1024, /* fold only if harmless FOR THE BODIES UPLOADED: at nb_create / nb_upload of an unsharded
                                         handle the library evaluates their accelerations with and without the folding (two force
                                         evaluations) and folds only if they agree to 2e-6 of the force scale, max |a| (nb_describe:
                                         mass_scaled, mass_scaling_check).  A global figure at upload time: it does not bound the relative
                                         error of a body whose own |a| is far below the largest, and it is not repeated as the system
                                         evolves — the default of ABI 5, opt-in since.  The reference's own bodies (Simulation.hpp:347-603)
                                         fail it (4e-5) and keep both multiplies.  Ignored by sharded handles (no folding) */
       NB_FLAG_NO_MASS_SCALING = 512, /* never fold: both per-pair mass multiplies stay (12 + 2 instructions per body).  The default; the bit
                                         overrides the two above (a host that passes a caller's flags through and must not fold) */
       /* 64 and 128 were NB_FLAG_PIPELINE / NB_FLAG_ONE_LAUNCH_STEP of ABI 4: two in-launch fusions of the step (a persistent step
          pipeline, one launch per step) that measured level or slower than two launches per step (docs/rounds/r04.md) and were removed
          in ABI 5 — nb_create rejects the bits like any unknown one */
       NB_FLAG_STATIC_ITEMS    = 256, /* the symmetric launches normally hand out their work items dynamically (every workgroup past the first
                                         resident wave draws the next item of the list when it starts, so that the XCDs of a part, which are not
                                         equally fast, end together: -1.4 ... -2.3 % per step from 65 536 bodies up, same bits); this bit keeps
                                         item = workgroup index (A/B runs) */
       NB_FLAG_SHARD_SINGLE    = 16,  /* shard_world = 1, i_count = n: run the sharded symmetric protocol (or, with
                                         NB_FLAG_SHARD_ALLREDUCE, the replicated one) with ONE rank — every pair is "local",
                                         the reduce-scatter / all-gather degenerate to copies.  For rehearsing the exchange
                                         path (nb_comm_*, nb_exchange_*) on a single GPU; never faster than a plain handle */
       /* 2048 is unassigned (4096, 8192, 16384 and 32768 are the four tree bits below): nb_create rejects it like any unknown bit */
       NB_FLAG_TREE_LEAVES     = 4096,  /* NB_FORCE_TREE only (with NB_FORCE_DIRECT nb_create returns NB_EINVAL, naming the combination):
                                         the CONVERGENT Barnes-Hut force.  Cells, centres of mass, node order and the acceptance test
                                         size^2 < d^2 * theta^2 are those of NB_FORCE_TREE without the bit; a leaf that is not accepted adds
                                         its own term d * (mass * inv^3) when d^2 > 0 (its record is exact: one position, the summed mass).
                                         Every inserted body is then counted exactly once per walker, inside an accepted cell or as its own
                                         leaf, and the result converges to the direct sum as theta -> 0: theta = 0 IS the softened direct
                                         sum over the distinct positions (a body's own leaf and the bodies coincident with it have d^2 = 0
                                         and add nothing, as in the direct sum).  THIS IS NOT THE REFERENCE'S ARITHMETIC: the reference's
                                         leaves add nothing, so every body there loses its nearest neighbours' pull and theta = 0 gives
                                         zero; without the bit that behaviour is kept bit for bit.  With NB_RSQRT_QUAKE every body walks on
                                         its own, one running sum in visit order (tests/tree_leaves_model.py restates it bit for bit).  With
                                         NB_RSQRT_EXACT the walk the measurements chose runs (nb_describe: walk=lane, or walk=group where the
                                         64 bodies of a wave walk together and a cell is accepted when all of them accept it: never coarser
                                         than a body's own walk; massless bodies and bodies on a position that first appears in an earlier
                                         window walk on their own).  Deterministic either way: two handles agree bit for bit, and permuting
                                         the bodies permutes the bits.  nb_describe appends " leaves=1 walk=lane|group".
                                         Everything the handle refuses or ignores as a tree handle it refuses or ignores with the bit too */
       NB_FLAG_TREE_QUADRUPOLE = 8192,  /* NB_FORCE_TREE with NB_FLAG_TREE_LEAVES only (alone, with NB_FORCE_DIRECT or without
                                         NB_FLAG_TREE_LEAVES nb_create returns NB_EINVAL, naming the flag and the missing partner): accepted
                                         cells carry the next multipole term.  Every branch keeps, beside its centre of mass c, the raw second
                                         moment M = sum m_k (y_k - c)(y_k - c)^T over the inserted positions of its subtree (xx, xy, yy; raw,
                                         not traceless, because the kernel is softened), computed bottom-up in the centre-of-mass pass from
                                         the children's moments in quadrant order 0..3 (parallel-axis form, fp32, no contraction).  The nodes
                                         visited, the acceptance test, the group vote and the "walks alone" rule are those of
                                         NB_FLAG_TREE_LEAVES; only the term of an accepted BRANCH changes: with d = c - body position,
                                         R^2 = d^2 + eps^2 and m its mass it adds
                                             d * (m R^-3 + 7.5 (d^T M d) R^-7 - 1.5 tr(M) R^-5) - 3 (M d) R^-5
                                         (the dipole vanishes about c; with eps = 0 the textbook quadrupole, Q = 3 M - tr(M) I).  A leaf has
                                         M = 0: its term, accepted or not, is the monopole term, instruction for instruction.  theta = 0
                                         never accepts a cell, so the result is that of the NB_FLAG_TREE_LEAVES handle bit for bit.  With
                                         NB_RSQRT_QUAKE the per-lane walk runs with one running sum and no contraction
                                         (tests/tree_quad_model.py restates it bit for bit); with NB_RSQRT_EXACT the walk nb_describe names,
                                         where the moment record of a cell the whole wave accepts arrives once per wave.  Deterministic as
                                         before: two handles agree bit for bit, permuting the bodies permutes the bits.  Memory: one 16-byte
                                         record per node in an array of its own, 16 B x (16 n + 4096) = +256 B per body on top of the 535 B
                                         per body of a tree handle, allocated only with the bit.  nb_describe appends " quad=1" after
                                         "walk=...".  Without the bit nothing changes: same bits, same launches, same memory.  Everything a
                                         NB_FLAG_TREE_LEAVES handle refuses or ignores it refuses or ignores with the bit too */
       NB_FLAG_TREE_ENERGY = 16384,     /* NB_FORCE_TREE with NB_FLAG_TREE_LEAVES only, with or without NB_FLAG_TREE_QUADRUPOLE (with
                                         NB_FORCE_DIRECT or without NB_FLAG_TREE_LEAVES nb_create returns NB_EINVAL, naming the flag and the
                                         missing or conflicting partner; a walk without the leaves has no near field and no meaningful
                                         potential): nb_energy becomes an O(n log n) diagnostic.  It rebuilds the tree at the current
                                         positions and walks it: *potential = 1/2 sum m_i phi_i, phi_i summed over exactly the nodes the
                                         wave-uniform force walk takes for body i (the fp32 acceptance test, windows of 64 bodies in key
                                         order, the "walks alone" rule), whatever rsqrt_mode the handle has: the potential has one walk.
                                         With d = c - body position and R^2 = d^2 + eps^2 a leaf, or an accepted cell without
                                         NB_FLAG_TREE_QUADRUPOLE, adds -m / R; an accepted branch with it adds
                                             -(m / R + 1.5 (d^T M d) / R^5 - 0.5 tr(M) / R^3)
                                         (the potential whose gradient is the force term above).  Node records, moments and positions are
                                         the fp32 values of the build, except that a leaf holding several bodies weighs the fp64 sum of
                                         their masses (its fp32 record plus an fp32 residual kept per node for this walk; +4 bytes per
                                         node); every term, the per-body sums and the reductions are fp64.
                                         *kinetic is sum m v^2 / 2 as before.  THE SAME PAIRS as nb_energy without the flag: every unordered
                                         pair once, the bodies sharing one position included (-m_i m_j / eps each, added body by body, not
                                         from the leaf's fp32 mass sum); massless bodies weigh nothing; theta = 0 IS the direct energy.
                                         ONE DIFFERENCE: with eps = 0 the pairs on one position are skipped and the result is finite,
                                         where the direct form gives inf.  No effect on the trajectory: acc[], positions, velocities and
                                         the frame counter are untouched; the tree arrays are rebuilt (the next force evaluation rebuilds
                                         them anyway) and nb_tree_stats then describes this build.  A build that fails (node capacity,
                                         depth cap) makes THIS call return NB_ENOMEM, through the once-only report above, and *kinetic /
                                         *potential are not written.  nb_describe appends " energy=tree".  Without the bit nb_energy is
                                         unchanged on every kind of handle.  +64 bytes per body (the leaf residuals) and +16 bytes per 256
                                         bodies (the partials of the second launch) */
       NB_FLAG_TREE_RELATIVE = 32768 }; /* NB_FORCE_TREE with NB_FLAG_TREE_LEAVES only, with or without NB_FLAG_TREE_QUADRUPOLE and
                                         NB_FLAG_TREE_ENERGY (with NB_FORCE_DIRECT or without NB_FLAG_TREE_LEAVES nb_create returns NB_EINVAL,
                                         naming the flag and the missing or conflicting partner): an opening test relative to the body's own
                                         last acceleration, the criterion of GADGET-2, on top of the geometric one.  Per body i let (ax, ay)
                                         be acc[i] AS THE HANDLE HOLDS IT: the acc field of the record after nb_create / nb_upload, the
                                         result of the last successful force evaluation afterwards.  g_i = alpha * sqrt(ax ax + ay ay),
                                         fp32, one rounding per operation, the square root correctly rounded, computed once before the walk.
                                         A node {c, m, size^2} at d = c - body position is accepted ("far") for body i when BOTH hold
                                             size^2 < d^2 * theta^2                            (the test of every tree handle: theta is the cap)
                                             g_i == 0  ||  m * size^2 < (g_i * d^2) * d^2      (fp32, this order, no contraction)
                                         i.e. G m size^2 / d^4 < alpha |a_prev| with G = 1.  alpha is set with nb_tree_alpha (below); at
                                         creation it is 0.005, GADGET-2's customary setting, not a value measured for this library.
                                         The relative walk opens whatever the theta walk opens and more: never coarser.  The group vote, the
                                         windows of 64 in key order, the "walks alone" rule, the leaf terms, d^2 > 0 and the quadrupole term
                                         are unchanged; the new test only feeds the vote.  With NB_RSQRT_QUAKE the per-lane walk runs
                                         (tests/tree_rel_model.py restates it bit for bit).  CONSEQUENCES: fresh initial conditions (acc = 0)
                                         make the first evaluation the plain theta walk, and every later one uses its predecessor; a caller
                                         who wants the criterion active from step 1 calls nb_accelerations once before stepping (a second
                                         call on fresh initial conditions already uses the first one's result).  A handle created from
                                         nb_sync's records of a running handle, with first_frame set, continues that run bit for bit: a_prev
                                         travels in the record.  A failed build leaves acc[], and so a_prev, untouched.  alpha = 0 switches
                                         the test off: the bits of the same handle without the flag.  Deterministic as before: two handles
                                         agree bit for bit, permuting the bodies (records included) permutes the bits.  With
                                         NB_FLAG_TREE_ENERGY nb_energy walks with the same predicate and the acc[] of that moment: the nodes
                                         a force evaluation issued now would take; it still touches nothing, and theta = 0 is still the
                                         direct energy.  No memory is added.  nb_describe appends " alpha=<value>" after "walk=...", "quad=1"
                                         and "energy=tree".  Without the bit nothing changes: same bits, same launches, same memory.
                                         Everything a NB_FLAG_TREE_LEAVES handle refuses or ignores it refuses or ignores with the bit too */
/* Body order of the whole-system symmetric kernel.  An unsharded 2-D direct-sum handle on the symmetric path (fp32 or fp64) with
 * 131 072 to 262 144 bodies sweeps its bodies along a Morton curve over their bounding box instead of in the caller's index order: tiles
 * and chunks are then compact patches, the operands of neighbouring lanes and consecutive pairs are alike, and the power-limited part
 * holds a higher clock (the force launch is 3.4 % shorter at 262 144 bodies, a step 2.9 %).  Nothing the caller sees is reordered: every array, nb_sync,
 * the queries and every other kernel keep the caller's indices.  Results differ from the unordered handle's by summation order only,
 * BUT NOT FOR FREE: the terms a lane sums are then nearly equal and their rounding errors of one sign.  Largest error of the
 * accelerations against fp64, of max |a|: 2.9e-7 in index order, 3.0e-6 along the curve at 262 144 bodies (1.4e-6 at 131 072); it grows
 * with the plan's chunks per item and passes 2e-5 from 524 288 bodies on, which is why the rule stops at 262 144.
 * The order is taken anew at nb_create / nb_upload and then ahead of every 16th force evaluation counted from there (not per nb_step
 * call: nb_step(1) + nb_step(3) and nb_step(4) give the same bits); it is deterministic: two handles of the same bodies agree bit
 * for bit.  nb_describe says "order=morton/<evaluations per sort>" or "order=0"; nb_body_order (below) reads the permutation.
 * Sequential-sum handles, the one-sided kernels, sharded ranks, 3-D and tree handles keep the caller's order whatever the bits.
 * A handle that asks for the mass-scaled body (NB_FLAG_MASS_SCALING, NB_FLAG_MASS_SCALING_MEASURED) keeps the caller's order unless
 * NB_FLAG_BODY_ORDER is set: the extra rounding of that body adds up along the curve (7.0e-6 of the force scale at 262 144 bodies
 * where index order gives 4.1e-7); with both, NB_FLAG_MASS_SCALING_MEASURED measures the ordered sweep it would run. */
enum { NB_FLAG_BODY_ORDER    = 131072,  /* the order at ANY size: it also lifts the lower size limit of the symmetric scheme for an
                                         otherwise eligible handle (small systems are slower that way: for tests and measurements) */
       NB_FLAG_NO_BODY_ORDER = 262144 };/* never: the caller's order (wins over NB_FLAG_BODY_ORDER) */
/* every bit above: nb_create refuses any other (NB_EINVAL) */
enum { NB_FLAGS_KNOWN = NB_FLAG_NO_SYMMETRY | NB_FLAG_NO_UNIFORM_MASS | NB_FLAG_NO_GUIDED_TAIL | NB_FLAG_SHARD_ALLREDUCE | NB_FLAG_SHARD_SINGLE |
                        NB_FLAG_MASS_SCALING | NB_FLAG_NO_MASS_SCALING | NB_FLAG_STATIC_ITEMS | NB_FLAG_MASS_SCALING_MEASURED |
                        NB_FLAG_TREE_LEAVES | NB_FLAG_TREE_QUADRUPOLE | NB_FLAG_TREE_ENERGY | NB_FLAG_TREE_RELATIVE |
                        NB_FLAG_BODY_ORDER | NB_FLAG_NO_BODY_ORDER };

/* ---- parameters ----------------------------------------------------------- */
typedef struct nb_params {
    uint32_t struct_size;  /* = sizeof(nb_params); set by nb_params_default */
    float    eps;          /* softening length; reference: 1.0f (Simulation.hpp:59 -> Quadtree.hpp:19) */
    float    dt;           /* default time step; reference: SIMULATION_DT = 0.01f (main.cpp:39) */
    int32_t  precision;    /* NB_FP32 | NB_FP64 */
    int32_t  rsqrt_mode;   /* NB_RSQRT_* */
    int32_t  sum_order;    /* NB_SUM_* */
    int32_t  integrator;   /* NB_INTEGRATOR_* */
    int32_t  extras;       /* NB_EXTRA_* bit mask; 0 = pure gravity */
    int32_t  device;       /* HIP device ordinal, -1 = current device */
    int32_t  j_slices;     /* 0 = auto; >0 forces the number of j-slices of the force grid */
    uint64_t i_begin;      /* first particle this handle integrates (sharding) */
    uint64_t i_count;      /* number of particles it integrates; 0 = all n */
    void    *stream;       /* hipStream_t to enqueue on, NULL = a private stream */
    void    *pos_buffers[2];/* optional caller-owned device buffers for the two full-n
                              position replicas (n * 2 * sizeof(real) bytes each, (x,y)
                              interleaved) so that a host-side collective can fill them;
                              NULL = allocated by the library.  ORDERING (this, acc_buffers and
                              `stream`): nb_create and nb_upload write these buffers on the handle's
                              stream, which nothing orders against the caller's other streams — so
                              when any of the three is the caller's, both calls first wait for ALL
                              work previously enqueued on the device (one hipDeviceSynchronize per
                              call, never on the step path): a fill or a collective the caller
                              queued on those buffers beforehand cannot land after the upload.
                              Both return with the upload complete.  Between steps the ordering is
                              the caller's, as described at nb_step_begin */
    int32_t  shard_rank;   /* this handle's rank and the number of ranks of a sharded run     */
    int32_t  shard_world;  /* (0/0 or x/1 = not sharded by the library's symmetric protocol)  */
    void    *acc_buffers[2];/* optional caller-owned device buffers of the symmetric sharded
                              protocol: [0] n*(ax,ay) floats = this rank's PARTIAL acceleration
                              of every particle (reduce-scatter input), [1] i_count*(ax,ay) =
                              the summed acceleration of the owned block (its output);
                              NULL = allocated by the library */
    int32_t  dims;         /* 2 (default, the reference) or 3: build extension — z of
                              pos / vel / acc lives in the first padding float of each vector
                              (macro NB_Z), sizeof of a body stays 64; tiled sum, no extras */
    int32_t  flags;        /* NB_FLAG_* bit mask */
    /* Tuning of the launch geometry; 0 = automatic everywhere (what the measurements in profiles/ chose).
     * Ranks of one sharded run must pass identical values: they select the pair split (nb_sym_info). */
    int32_t  sym_chunks_per_item; /* symmetric kernel: 64-particle chunks per work item (L) */
    int32_t  sym_aux_stream;      /* sharded symmetric: local items on a side stream: 0 auto, 1 always, -1 never */
    float    sym_late_us;         /* sharded symmetric: whole-chip microseconds of local work held back to run
                                     beside the reduce-scatter: 0 auto (40 us from 8 ranks on), < 0 none */
    int32_t  lanes_p;             /* one-sided kernel: packed particle pairs per lane (1, 2, 4) */
    float    sym_tail[3];         /* guided-tail thresholds (fractions of a launch's work from which items are cut
                                     into L/2, L/4, L/8 chunks); all 0 = 0.85, 0.94, 0.98 */
    int32_t  sym_chunk_pairs;     /* symmetric fp32 kernels: sweep the travelling chunks in PAIRS (two particles per lane, items
                                     cut into even chunk counts): 0 auto (from 65 536 bodies on; in 3-D with equal masses only),
                                     1 always, -1 never */
    uint64_t first_frame;         /* value nb_frame() starts from: 0 for a new run, the dump header's frame for a restart
                                     (the reference's Simulation::frame, Simulation.hpp:53, starts at 0: :60) */
    int32_t  sym_tile;            /* symmetric fp32 2-D kernels, single handle: stationary particles per work-item tile.  2048 = the
                                     classic form (4 waves x 512 different particles); 512 = the wave-split form (the 4 waves share 512
                                     particles and split the item's chunks: finer work units and 4-KiB slab rows for small and
                                     mid-size systems, 4x the travelling partials per pair); 0 = automatic (512 below 49 152 bodies) */
    int32_t  _reserved0;          /* keeps sizeof(nb_params) a multiple of 8 whatever the compiler; must be 0 */
    uint64_t pos_rows;            /* rows (particles) each caller-owned pos_buffers[] holds; 0 = n.  A sharded run whose world size does
                                     not divide n all-gathers ceil(n / world) rows per rank, so its replicas need world * ceil(n / world)
                                     rows: replicas the library allocates itself are sized that way, caller-owned ones must be and say so
                                     here (rows past n are never read by the kernels) */
    int32_t  force;               /* NB_FORCE_*; default NB_FORCE_DIRECT (ABI 8) */
    float    theta;               /* NB_FORCE_TREE: opening parameter, >= 0 and finite; default 1.0f, the reference's
                                     quadtree(1.0f, 1.0f, 16) (Simulation.hpp:59).  0 opens every branch */
} nb_params;

typedef struct nb_sim nb_sim; /* opaque; stands for one `Simulation` (Simulation.hpp:49) */

/* Fill *p with the reference's defaults (eps 1.0, dt 0.01, fp32, exact rsqrt, tiled sum). */
void nb_params_default(nb_params *p);

/* Replaces Simulation::Simulation() (Simulation.hpp:58-65) minus the hard-coded
 * ICs: the caller supplies the n initial bodies (AoS, 64-B records); they are
 * unpacked to SoA device arrays.  frame starts at 0. */
nb_sim *nb_create(const nb_body *init, size_t n, const nb_params *params);

/* Releases everything (the reference relies on ~Simulation via shared_ptr, main.cpp:657). */
void nb_destroy(nb_sim *s);

/* Replaces Simulation::step() (Simulation.hpp:67-75) called nsteps times with
 * time step dt (dt <= 0 -> params.dt; the reference reads the global
 * SIMULATION_DT once per step, Simulation.hpp:69).  Each step = force
 * evaluation at x_n (attract, :176) -> v += a dt -> x += v dt (iterate,
 * :129-163), ++frame (:74).  collide() (:72) is performed only with
 * NB_EXTRA_COLLIDE (off by default: it is not gravity).  Work is ENQUEUED on
 * the handle's stream; nb_wait / nb_sync / nb_energy order after it. */
int nb_step(nb_sim *s, float dt, int nsteps);

/* Block until all enqueued work of the handle is complete. */
int nb_wait(nb_sim *s);

/* Bring the host view up to date: writes the owned block (i_begin..i_begin+i_count)
 * into out[0..i_count) — pos, vel, acc (of the last force evaluation), mass,
 * radius, padding zeroed.  This is what makes `Simulation::bodies`
 * (Simulation.hpp:54) coherent after step() for the snapshot copy at
 * main.cpp:623-627. */
int nb_sync(nb_sim *s, nb_body *out);

/* Host memory the copy engine may read / write DIRECTLY (nb_sync, nb_snapshot_begin, nb_sync_positions, nb_create,
 * nb_upload): only ranges this library knows to be page-locked over the WHOLE transfer — blocks from nb_host_alloc and
 * ranges registered here.  Any other pointer (malloc'ed arrays, `std::vector<Body>` storage — what the reference's
 * caller holds, main.cpp:623-627 — numpy arrays) is always legal and moves through the handle's page-locked staging
 * buffer in pipelined pieces (the host copy of piece k overlaps the DMA of piece k + 1).
 *
 * nb_host_register page-locks [ptr, ptr + bytes) in place.  ptr must be page-aligned and bytes a whole number of
 * pages (sysconf(_SC_PAGESIZE)); anything else is refused with NB_EINVAL: a registration pins whole pages, and the
 * first / last page of an unaligned heap array also holds its neighbours' data, which is not the caller's to pin.
 * Unregister (by the same ptr) BEFORE the storage is released; never register storage that may be reallocated
 * behind your back (a std::vector's).  nb_host_alloc / nb_host_free hand out page-locked blocks owned by the library. */
int   nb_host_register(void *ptr, size_t bytes);
int   nb_host_unregister(void *ptr);
void *nb_host_alloc(size_t bytes);
int   nb_host_free(void *ptr);

/* Positions only (8 bytes/body instead of 64): the fast path for a viewer that
 * only draws (main.cpp:623-627 consumer).  out holds 2*i_count floats (x,y) — 3*i_count
 * (x,y,z) for a dims = 3 handle.  For NB_FP64 handles values are rounded to float. */
int nb_sync_positions(nb_sim *s, float *out_xy);

/* Pipelined snapshot for a caller that does `step(); copy bodies` every frame (main.cpp:621-627) and can take the
 * copy one step late: nb_snapshot_begin packs the owned block as of the work enqueued so far and starts its D2H
 * copy on a separate copy stream, then returns; steps enqueued afterwards run concurrently with the transfer
 * (16.8 MB per frame at N = 262 144).  nb_snapshot_wait blocks until `out` is complete.  One snapshot in flight
 * per handle.  If `out` is page-locked memory known to the library (nb_host_alloc / nb_host_register) the copy engine
 * writes it directly; otherwise the data lands in the library's staging buffer and is copied to `out` inside
 * nb_snapshot_wait — which a caller issues after enqueueing the next step, so that host copy overlaps the GPU too.
 * nb_sync stays the simple blocking form. */
int nb_snapshot_begin(nb_sim *s, nb_body *out);
int nb_snapshot_wait(nb_sim *s);

/* Push host-side edits of the bodies back (the reference's `bodies` is public
 * and the GUI appends to it through SPAWN_QUEUE, main.cpp:43).  in holds the n
 * bodies of the whole system. */
int nb_upload(nb_sim *s, const nb_body *in);

/* Evaluate accelerations at the current positions without integrating
 * (Simulation::attract(), Simulation.hpp:176-214, as a direct sum). */
int nb_accelerations(nb_sim *s);

/* Total energy, fp64 accumulation on the device, softening-consistent with the
 * force (Quadtree.hpp:140-142): K = sum m v^2/2, U = -sum_{i<j} m_i m_j/sqrt(r^2+eps^2).
 * Replaces the unusable calculateMetrics (main.cpp:91-194) / Body::kinetic_energy
 * (Body.hpp:98-101).  On a sharded handle K and U are the owned block's share
 * (U of block B = - sum_{i in B} sum_{j > i} m_i m_j / sqrt(...): every unordered pair is
 * counted by the handle that owns its lower index), so the shares of all ranks add up to the total. */
int nb_energy(nb_sim *s, double *kinetic, double *potential);

/* Total linear momentum sum m v (the reference's Body::momentum, Body.hpp:103-106, summed) into p_xyz[3] (p_xyz[2] = 0
 * for a 2-D handle) and, if l_z is not NULL, the angular momentum about the origin sum m (x vy - y vx); fp64
 * accumulation on the device in a fixed order.  Both are conserved by the pairwise force (Newton's third law) up to
 * rounding, whatever the softening; a sharded handle returns its owned block's share (the shares add up). */
int nb_momentum(nb_sim *s, double *p_xyz, double *l_z);

/* The potential of every owned body, the per-body counterpart of nb_energy:
 *     phi[i] = - sum_{j != i} m_j / sqrt(|x_j - x_i|^2 + eps^2)        (G = 1, the softening of the force)
 * so that the binding energy of body i is v_i^2 / 2 + phi[i], the bound members are those below 0 and the most-bound body is a
 * centre; 1/2 sum m_i phi[i] over all bodies is the *potential of nb_energy.
 * WHICH BODIES: phi[0 .. nb_owned_count(s)), the owned block of the handle at the positions of all work enqueued so far, exactly as
 * nb_sync_positions defines them; the j-sum runs over all n bodies of the CURRENT replica (on a sharded handle it must be
 * complete, as for nb_energy).  Every kind of handle: fp32 and fp64, dims 2 and 3, either integrator, sharded or not, direct or
 * tree with any flags.  A massless body gets a phi too: the field potential at a tracer.
 * THE SELF TERM is left out by index (j != i), not by distance: bodies that share i's position each add -m_j / eps, nb_energy's
 * pair convention.  With eps = 0 a body that shares its position with another gets a value that is NOT FINITE (nb_energy's
 * infinity); every other body's value is finite.
 * ARITHMETIC of the direct sweep (every handle but a NB_FLAG_TREE_ENERGY one; a tree handle without that flag, the reference-
 * arithmetic one without leaves included, runs it too: "exact O(n^2) unless the handle has the flag", as nb_energy).  NB_FP64: fp64
 * throughout, the terms added in j order (1.4e-16 per reciprocal square root): within n x 1.1e-16 of the exact sum.  NB_FP32
 * (whatever rsqrt_mode and sum_order): fp32 terms m_j x v_rsq_f32(r^2) summed in fp32 over runs of 64 consecutive j, the runs added in
 * fp64, the result fp64: within 4e-6 relative of the fp64 sum of the same float positions (3.5 ulp per term and the 63 roundings of
 * a same-signed run; tests/potential_model.py is the numpy statement).
 * DETERMINISM: two handles agree bit for bit.  On the direct sweep phi[i] depends on the bodies, eps, the precision and i only, not
 * on the owned block or the launch geometry (the j-tiles always start at j = 0 and the partial sums are added in one fixed order): a
 * handle that owns [i_begin, i_begin + i_count) returns the bits of that slice of the unsharded handle's result.
 * NB_FLAG_TREE_ENERGY handles: the tree build and the potential walk of nb_energy run, and phi[i] is the walker's value (the bodies on
 * its own position included), written instead of reduced: the cells, the windows of 64, the "walks alone" rule, the quadrupole and
 * relative tests, the fp64 terms and the leaf residual are nb_energy's (tests/tree_energy_model.py, phi).  eps = 0 skips the pairs
 * on one position (finite), as nb_energy does there.  Massless bodies walk alone, as in the force walk (in nb_energy they do not
 * walk); one that lies exactly on an inserted position takes no term from that leaf (d^2 = 0): the one difference from the direct
 * sweep.  Permuting the bodies leaves the visited terms unchanged; phi changes through the order of the sum only.  As for nb_energy
 * the tree arrays are rebuilt, nb_tree_stats describes this build, and a failed build makes THIS call return NB_ENOMEM through the
 * once-only report, phi not written.
 * Nothing else of the handle changes: positions, velocities, acc[] and the frame counter are untouched, and the next step is
 * bit-identical to one on a handle that never called this.
 * ERRORS: NB_EINVAL for a NULL handle or a NULL phi, before any device work; NB_ESTATE while a split step is in flight.  The call
 * synchronises; a pending once-only report (collision capacity, failed tree build) leaves through it as through nb_sync_positions
 * (NB_ENOMEM, once), and nothing is written to phi then.  phi may be any host memory, as for nb_sync: ranges known to be page-locked
 * (nb_host_alloc / nb_host_register) are written by the copy engine directly, anything else moves through the staging buffer of
 * nb_sync.  Memory: 8 bytes per owned body on the device from the first call on (freed by nb_destroy).  With nb_profile_enable the
 * sweep (the two walk kernels on a NB_FLAG_TREE_ENERGY handle) is bracketed like a force launch and counts as one (nb_profile_read).
 * Cost on an MI355X, fp32 2-D, into a pageable array (profiles/potential_bench.log): the direct sweep 10.4 ms at 262 144 bodies and
 * 145 ms at 1 048 576 (a one-sided force evaluation of the same handles: 12.1 and 195 ms); a NB_FLAG_TREE_ENERGY handle at
 * theta = 0.5: 2.9 ms at 1 048 576 and 20 ms at 8 388 608. */
int nb_potentials(nb_sim *s, double *phi);

/* Collisions (NB_EXTRA_COLLIDE).  nb_collide_capacity sets the pair capacity (1 .. 2^31 - 1) between steps; NB_ESTATE on a
 * handle created without the bit.  nb_collision_stats synchronises and returns the pairs of the last step, the pairs resolved
 * since creation, the resolution rounds of the last step (ready pairs are resolved together; a chain of k touching discs
 * costs k - 1 rounds) and the steps that were over capacity; any pointer may be NULL; all zero without the bit. */
int nb_collide_capacity(nb_sim *s, size_t max_pairs);
int nb_collision_stats(nb_sim *s, uint64_t *pairs_last_step, uint64_t *pairs_total, uint32_t *rounds_last_step,
                       uint64_t *overflow_steps);

/* Barnes-Hut force (NB_FORCE_TREE).  nb_tree_stats synchronises and returns the nodes and the deepest leaf of the last force
 * evaluation and the evaluations that failed (node capacity, depth cap) since creation; any pointer may be NULL; NB_ESTATE
 * on a NB_FORCE_DIRECT handle. */
int nb_tree_stats(nb_sim *s, uint64_t *nodes, uint32_t *max_depth, uint64_t *overflow_steps);

/* The reference's `quadtree.nodes` (Quadtree.hpp:14; copied by its caller every frame, main.cpp:626, and drawn by
 * drawQuadtreeNode, main.cpp:394-475): the tree of the MOST RECENT BUILD on the handle as Node records.  The most recent build is
 * the force evaluation of the last nb_step / nb_accelerations, or an nb_energy / nb_potentials on a NB_FLAG_TREE_ENERGY handle; after nb_step that
 * is the tree of the positions BEFORE the drift, as the reference's quadtree.nodes after step().  Any tree handle, any of the four
 * tree flags, either rsqrt mode: the tree does not depend on them (quadrupole moments are not exported: Node has no field).
 * REFERENCE FORM (the reference's own indices follow the insertion order and cannot be reproduced; this is the one numbering with
 * its invariants that does not depend on the order of the bodies): node 0 is the root; the branches are ranked r = 0, 1, ... in
 * pre-order and the children of branch r are nodes 1 + 4 r ... 1 + 4 r + 3 in quadrant order, so *count = 1 + 4 x branches = the
 * `nodes` of nb_tree_stats; children = index of the first child, 0 for a leaf or an empty quadrant; next = own index + 1 for
 * quadrants 0..2 and the parent's next for quadrant 3, 0 for the root (Quadtree.hpp:71-75); depth as the reference counts it;
 * bodies = {0, 0}; pos / mass the node's record as the build holds it (a branch: centre of mass and mass; a leaf: its position and
 * summed mass; an empty quadrant: 0, 0, 0); size = the root size halved depth times (size * size has the bits the walk tests);
 * center = the root centre carried down with Quad::into_quadrant's arithmetic (Quad.hpp:51-57).  The tree is the reference's own
 * (same cells, same records, following `children`), and Quadtree::acc over this array gives the bits of the handle's walk
 * (tests/tree_nodes_model.py).
 * The call synchronises.  count may not be NULL and is written whenever the call returns NB_OK or NB_EINVAL for the capacity:
 * out == NULL is the count query (NB_OK); out != NULL with capacity < *count is NB_EINVAL naming both numbers, nothing written to
 * out; before any build *count = 0, NB_OK.  NB_ESTATE on a NB_FORCE_DIRECT handle.  A pending failed-build report (node capacity,
 * depth cap) is delivered by this call like by nb_wait: NB_ENOMEM, once; while the last build is a failed one, later calls return
 * NB_ESTATE ("no tree to export").  out may be any host memory, as for nb_sync: ranges known to be page-locked (nb_host_alloc /
 * nb_host_register) are written by the copy engine directly, anything else moves through the page-locked staging buffer that the
 * query calls of a handle share (nb_tree_nodes, nb_raster, nb_neighbors, nb_groups: one buffer, as large as the largest plane any of
 * them had to stage; one plane at a time goes through it).  Nothing of the handle changes: tree arrays, acc[], positions, velocities, frame counter and nb_tree_stats are
 * untouched, and the next force evaluation is bit-identical to one on a handle that never called this.
 * Memory: nothing until the first call with out != NULL; then, sized by the node count of the build exported (growth only, freed by
 * nb_destroy; NOT by the node capacity 16 n + 4096): 144 bytes per node on the device (the record 128, branch flag 4, branch rank 8,
 * export index 4) plus the scan's temporary storage; the shared staging buffer is grown to 128 bytes per node once a destination
 * needs it.  With nb_profile_enable the export kernels are bracketed like a force launch and count as one (nb_profile_read). */
int nb_tree_nodes(nb_sim *s, nb_tree_node *out, size_t capacity, size_t *count);

/* The frame whose size is the screen's: how many bodies, and how much mass, fall into each pixel of a view, binned on the device and
 * copied out as width x height values whatever n is.  Replaces, for systems too large to copy and draw body by body, the reference's
 * render loop (main.cpp:745-835: one quad per visible body after worldToScreen / isInScreenBounds, :196-213) and the copy of the
 * bodies that feeds it: the caller uploads one texture.
 * WHICH BODIES: the owned block of the handle, at the positions of all work enqueued so far, exactly as nb_sync_positions defines
 * them; an NB_FP64 handle's positions and masses are rounded to float first; a dims = 3 handle is projected on (x, y).  Every kind of
 * handle: direct or tree, any flags, sharded or not (the count planes of the ranks of a sharded run add up to the unsharded one).
 * PIXEL OF A BODY: fp32, one rounding per operation, no contraction, the reference's worldToScreen:
 *     sx = (x - center_x) * scale + width * 0.5f        sy = (y - center_y) * scale + height * 0.5f
 * The body is inside when sx >= 0 && sx < (float)width && sy >= 0 && sy < (float)height, tested BEFORE any conversion (sx = -0.5 is
 * outside; a NaN or infinite coordinate is outside); its pixel is then p = (uint32_t)sy * width + (uint32_t)sx: rows in y order,
 * row-major.  The reference's 1000-pixel culling margin is not reproduced: the image is the screen.
 * OUTPUTS: count[p] = bodies in pixel p, massless ones included.  mass[p] is built in exact integer units: a body contributes u = 0
 * when !(m > 0) (zero, negative, NaN), otherwise r = m / mass_quantum (fp32) and u = r >= 4294967296.0f ? 4294967295 :
 * (uint32_t)rintf(r) (ties to even); the units of a pixel are summed as 64-bit integers U_p (n <= 2^31 bodies of at most 2^32 - 1
 * units cannot overflow) and mass[p] = (float)((double)U_p * (double)mass_quantum).  No floating-point atomics anywhere.  CONSEQUENCES:
 * two handles agree bit for bit, and permuting the bodies leaves both planes unchanged bit for bit.
 * Either of count / mass may be NULL, not both; a plane that is not asked for costs no pass and no copy, and is not written.  The
 * destinations (width * height elements each) may be any host memory, as for nb_sync: ranges known to be page-locked (nb_host_alloc /
 * nb_host_register) are written by the copy engine directly, anything else moves through the query calls' shared staging buffer
 * (nb_tree_nodes).
 * ERRORS: NB_EINVAL, naming the field, before any device work: NULL handle, view or both planes; struct_size != sizeof(nb_view);
 * width or height 0 or above 16384, or width * height > 2^24; scale not finite or <= 0; a non-finite centre; _reserved0 != 0;
 * mass != NULL with mass_quantum not finite or <= 0.  NB_ESTATE while a split step is in flight.  The call synchronises; a pending
 * once-only report (collision capacity, failed tree build) leaves through it as through nb_sync_positions (NB_ENOMEM, once), and
 * nothing is written to the planes then.
 * Nothing of the handle changes: positions, velocities, acc[], frame counter, tree arrays and nb_tree_stats are untouched, and the
 * next step is bit-identical to one on a handle that never called this.
 * Memory: nothing until the first call; then, per pixel of the largest view seen (growth only, freed by nb_destroy): 4 bytes on the
 * device for the counts; 8 + 4 bytes more (unit sums, float plane) once a mass plane is asked for: 4 / 12 MiB for a 1024 x 1024 view;
 * the shared staging buffer is grown to 4 bytes per pixel (4 MiB) once a destination needs it.  Cost: adds that share a pixel are combined inside the wave and
 * inside the workgroup (LDS) before they reach memory, so the worst case for atomics, every body in ONE pixel, is not the slow one:
 * on an MI355X the bin pass of a 1024 x 1024 view at scale 1e-3 (all bodies in the four pixels round the centre) takes 0.052 ms at
 * 1 048 576 bodies and 0.066 ms (counts) / 0.123 ms (both planes) at 8 388 608, where one global add per body takes 3.1 ms at
 * 1 048 576; the whole call, both planes into pageable memory, 0.45 and 0.51 ms (profiles/raster_bench.log).
 * With nb_profile_enable the bin pass is bracketed like a force launch and counts as one (nb_profile_read). */
typedef struct nb_view {
    uint32_t struct_size;      /* = sizeof(nb_view), set by the caller */
    uint32_t width, height;    /* pixels: 1 .. 16384 each, width * height <= 2^24 */
    float    center_x, center_y, scale;   /* the reference's worldToScreen, main.cpp:196-201 */
    float    mass_quantum;     /* > 0 and finite when a mass plane is asked for; ignored otherwise */
    uint32_t _reserved0;       /* must be 0 */
} nb_view;
int nb_raster(nb_sim *s, const nb_view *view, uint32_t *count, float *mass);

/* Who is near every body, how many, and the k nearest: the query behind the reference's drawConnections (main.cpp:233-386: a uniform
 * grid of MAX_DISTANCE cells, getGridKey :67-78, and up to MAX_CONNECTIONS links per body to the bodies of the 3 x 3 cells round it
 * with distSq < adaptiveDistanceSq), without nb_sync of 64 B per body and a hash-map pass on the host every frame; also the local
 * density estimate, the linking step of friends-of-friends and the nearest-neighbour distance of an analysis.  The reference's own
 * selection (the first 16 bodies per cell in insertion order, the first hits in unordered_map order, truncating cell keys) depends on
 * the order of the bodies and is not reproduced: this is the one order-independent definition with the same predicate.
 * WHICH BODIES: the queries are the owned block, nb_owned_count(s) rows, at the positions of all work enqueued so far, exactly as
 * nb_sync_positions defines them; the candidates are all n bodies of the CURRENT replica (on a sharded handle it must be complete, as
 * for nb_energy).  An NB_FP64 handle's positions are rounded to float first; a dims = 3 handle is projected on (x, y): nb_raster's
 * rules.  Every kind of handle: direct or tree, any flags, sharded or not.
 * PREDICATE: fp32, one rounding per operation, no contraction, the reference's (body1->pos - body2->pos).mag_sq() < adaptiveDistanceSq:
 *     dx = x_j - x_i      dy = y_j - y_i      d2 = dx * dx + dy * dy      r2 = radius * radius
 * j is a neighbour of i when j != i && d2 < r2: the self term is left out by index, the comparison is strict, and bodies that share
 * i's position are its neighbours at d2 = 0.  A body with a non-finite coordinate has no neighbours and is nobody's neighbour (the
 * predicate is false on NaN and infinity).
 * OUTPUTS: count[i] = the number of ALL neighbours of owned body i, not capped at k.  Row i of idx holds k entries: the
 * min(count[i], k) neighbours that come first in ascending order of (d2, j), as global body indices, then NB_NO_NEIGHBOR; dist2 has
 * the same shape and holds their d2, then +inf.  Since d2 >= 0 its bits order like its value, so the order is that of the 64-bit
 * integer (bits(d2) << 32) | j: ties in d2 are broken by the index and the result is unique.  CONSEQUENCES: two handles agree bit for
 * bit, and permuting the bodies permutes the rows and relabels the indices wherever the kept entries and the first one left out have
 * distinct d2.  Any of idx / dist2 / count may be NULL, not all three; a plane that is not asked for is not written and not copied.
 * k is ignored for a count-only call.  The destinations may be any host memory, as for nb_sync: ranges known to be page-locked
 * (nb_host_alloc / nb_host_register) are written by the copy engine directly, anything else moves through the query calls' shared
 * staging buffer (nb_tree_nodes).
 * ERRORS: NB_EINVAL, naming the argument, before any device work: a NULL handle; idx, dist2 and count all NULL; radius not finite or
 * <= 0; radius * radius (fp32) not finite or equal to 0; k outside 1 .. 32 when idx or dist2 is asked for.  NB_ESTATE while a split
 * step is in flight.  The call synchronises; a pending once-only report (collision capacity, failed tree build) leaves through it as
 * through nb_raster (NB_ENOMEM, once), and nothing is written to the destinations then.
 * Nothing of the handle changes: positions, velocities, acc[], frame counter, tree arrays and nb_tree_stats are untouched (the query
 * has scratch of its own and does not borrow the tree's key arrays), and the next step is bit-identical to one on a handle that
 * never called this.
 * Memory: nothing until the first call; then (growth only, freed by nb_destroy) 40 bytes per body of the replica on the device (the
 * float position, the cell key and the body index, each by body and in sorted order) plus the sort's temporary storage; 4 bytes per
 * owned body once a count is asked for; 4 bytes per owned body x k for idx and 4 for dist2, each once asked for, for the largest k
 * seen; the shared staging buffer is grown to the largest plane a destination needs.
 * Cost: the bodies are sorted by the cell of a grid of cell size radius x (1 + 2^-16) and every query tests the bodies of the 3 x 3
 * cells round it, so the cost is proportional to the bodies in those cells; a radius that covers the whole system is the n^2 sweep.
 * The caller chooses the radius.  The search is cooperative: a workgroup stages the candidates of 256 neighbouring queries through LDS.
 * On an MI355X, Plummer spheres with a radius that gives a mean count of 29 - 31, idx and count (profiles/neighbors_bench.log): at
 * 1 048 576 bodies k = 5 takes 0.93 ms into nb_host_alloc memory and 1.53 ms into a pageable array (k = 16: 2.04 / 3.76 ms), of which
 * the search kernel 0.23 ms (0.52) and the sort 0.20 ms; at 262 144 bodies 0.39 / 0.57 ms, at 8 388 608 (tree handle) 6.1 / 10.2 ms;
 * nb_sync of the same handles takes 0.71 / 2.68 / 21.6 ms.  16 384 bodies in ONE cell: 2.2 ms, 1.2e11 pairs per second.
 * With nb_profile_enable the search kernel is bracketed like a force launch and counts as one (nb_profile_read). */
#define NB_NO_NEIGHBOR 0xFFFFFFFFu
int nb_neighbors(nb_sim *s, float radius, uint32_t k, uint32_t *idx, float *dist2, uint32_t *count);

/* Which bodies form a clump: the friends-of-friends groups of the bodies at linking length `radius`, the standard group finder of
 * N-body work, found on the device; the answer is 4 bytes per body.  Without it a caller copies out neighbour rows (k <= 32 truncates
 * the link graph in any dense region) or nb_syncs 64 B per body and runs a union-find on the host every frame.  With nb_potentials
 * the most-bound body of a group is its centre.
 * LINK: bodies i != j are linked when nb_neighbors' predicate holds, word for word: fp32, one rounding per operation, no contraction,
 *     dx = x_j - x_i      dy = y_j - y_i      d2 = dx * dx + dy * dy      r2 = radius * radius      linked when d2 < r2
 * The comparison is strict; bodies on one position are linked (d2 = 0); massless bodies take part; a body with a non-finite
 * coordinate links to nobody.  The relation is symmetric: fp32 subtraction is exactly antisymmetric, so d2(i, j) = d2(j, i) bit for
 * bit.
 * WHICH BODIES: nb_neighbors' rules.  The groups are the connected components of that graph over ALL n bodies of the CURRENT replica
 * (on a sharded handle it must be complete, as for nb_energy), at the positions of all work enqueued so far, exactly as
 * nb_sync_positions defines them.  An NB_FP64 handle's positions are rounded to float first; a dims = 3 handle is projected on
 * (x, y).  Every kind of handle: direct or tree, any flags, sharded or not.
 * OUTPUTS, for the owned block, nb_owned_count(s) rows: label[i] = the smallest global body index in i's group; size[i] = the number
 * of members of i's group, over all n bodies; *ngroups = the number of groups among all n bodies, singletons included, which is the
 * number of bodies whose label is their own index.  A body with a non-finite coordinate is a group of its own.  Any of the three may
 * be NULL, not all three; a plane that is not asked for costs no pass and no copy, and is not written.  CONSEQUENCES: the result is a
 * function of the bodies and the radius alone, whatever order the device links in; two handles agree bit for bit; permuting the
 * bodies permutes the partition, and each label is the smallest NEW index of its group.
 * label and size may be any host memory, as for nb_sync: ranges known to be page-locked (nb_host_alloc / nb_host_register) are
 * written by the copy engine directly, anything else moves through the query calls' shared staging buffer (nb_tree_nodes).
 * ERRORS: NB_EINVAL, naming the argument, before any device work: a NULL handle; label, size and ngroups all NULL; radius not finite
 * or <= 0; radius * radius (fp32) not finite or equal to 0.  NB_ESTATE while a split step is in flight.  The call synchronises; a
 * pending once-only report (collision capacity, failed tree build) leaves through it as through nb_neighbors (NB_ENOMEM, once), and
 * nothing is written to the destinations then.  NB_EHIP, nothing written, if the union-find ever left its loop bounds (every loop of
 * the link kernel is bounded by n + 1; the bound cannot be reached while the structure is a forest).
 * Nothing of the handle changes: positions, velocities, acc[], frame counter, tree arrays and nb_tree_stats are untouched, and the
 * next step is bit-identical to one on a handle that never called this.  The cells and the sort are the scratch of
 * nb_neighbors: the two calls may alternate on one handle at any radii.
 * Memory: nothing until the first call; then (growth only, freed by nb_destroy) nb_neighbors' 40 bytes per body of the replica and
 * its sort storage, if that call has not made them yet, plus 4 bytes per body of the replica (the union-find, then the labels); 4
 * bytes per body of the replica and 4 per owned body more once sizes are asked for; the shared staging buffer is grown to 4 bytes
 * per owned body once a destination needs it.
 * Cost: the bodies are sorted by cell as for nb_neighbors and every unordered pair of bodies in the same or adjacent cells is tested
 * once (half the pairs nb_neighbors tests); a pair that passes is united in a lock-free union-find (compare-and-swap, no lane waits
 * for another).  The cost is proportional to the pairs inside adjacent cells: a radius that covers the whole system is the n^2
 * sweep.  The caller chooses the radius.  What a linked pair costs depends on the partition: cheap while the groups are small, and
 * dearest when one giant group forms, whose n - 1 hooks each walk to two roots.  On an MI355X, Plummer spheres, all three outputs
 * into nb_host_alloc memory (profiles/groups_bench.log): at 1 048 576 bodies with a mean of 1 / 5 / 31 links per body (largest
 * group 192 / 463 238 / 831 606 bodies) 0.60 / 1.25 / 2.71 ms, of which the link kernel 0.11 / 0.67 / 2.14 ms and the sort 0.20 ms,
 * where nb_neighbors' count-only call takes 0.52 - 0.55 ms; into pageable arrays 0.78 / 1.44 / 2.85 ms; at 262 144 bodies 0.29 /
 * 0.65 / 0.80 ms; at 8 388 608 (tree handle) 3.33 / 4.97 / 7.72 ms, where nb_sync takes 21.6 ms.  The size pass combines the adds
 * of a wave and of a workgroup that share a group: all 1 048 576 bodies in ONE group cost it 0.020 ms, one add per body 11.9 ms.
 * With nb_profile_enable the link kernel is bracketed like a force launch and counts as one (nb_profile_read). */
int nb_groups(nb_sim *s, float radius, uint32_t *label, uint32_t *size, uint64_t *ngroups);

/* The group catalogue: mass, centre, motion, velocity dispersion and radius of every friends-of-friends group of at least min_members
 * bodies, reduced on the device; the answer is 80 bytes per GROUP (nb_group above).  Without it a caller takes nb_groups' labels,
 * nb_syncs 64 B per body and runs a bincount pass on the host every frame.
 * GROUPS: exactly nb_groups' at the same radius: its predicate, all n bodies of the current replica at the positions of all work
 * enqueued so far, an NB_FP64 handle's positions rounded to float for the grouping, a dims = 3 handle grouped on its (x, y)
 * projection, a body with a non-finite coordinate a group of its own.  The catalogue holds the groups with members >= min_members in
 * ascending order of label; *count is their number.
 * VALUES: x, v and m of a body are the float values nb_sync returns for it, widened to double (an NB_FP64 handle's are rounded to float
 * first); on a dims = 3 handle z takes part in pos, vel, sigma2 and r_max.  w_i = m_i when m_i > 0, else 0.  mass = sum w_i.
 * W = mass when mass > 0; otherwise every w_i = 1 and W = members (the unweighted means of a massless group; mass stays 0).  The
 * products w_i x_i are exact in double (24 x 24 bits).  Every sum is fp64 in an order that is fixed for given bodies, radius and
 * min_members: a segmented scan over the bodies sorted by (label, index); there is no floating-point atomic anywhere.  sigma2 and
 * r_max come from a second pass about the finished vel / pos, not from raw second moments minus squares.  A group that holds a body
 * with a non-finite value gets what the arithmetic gives.  CONSEQUENCES: two handles, and two calls on one handle, agree byte for byte;
 * permuting the bodies relabels the groups (label is the smallest NEW index), leaves members exact and the double fields equal up to
 * the order of summation: a sum of k terms differs from the exact one by at most about k 2^-53 sum |terms|.
 * COUNT QUERY AND CAPACITY, as nb_tree_nodes: count may not be NULL; out == NULL writes *count and returns NB_OK (the passes that
 * reduce are not run); out != NULL with capacity < *count is NB_EINVAL naming both numbers, *count is written and out is untouched.
 * Only the first *count records of out are written.
 * out may be any host memory: a range known to be page-locked (nb_host_alloc / nb_host_register) is written by the copy engine
 * directly, anything else moves through the query calls' shared staging buffer (nb_tree_nodes), 80 B per group.
 * ERRORS: NB_EINVAL, naming the argument, before any device work: a NULL handle; a NULL count; nb_groups' rules for the radius;
 * min_members == 0.  NB_ESTATE while a split step is in flight.  NB_ESTATE on a handle that does not own all n bodies
 * (nb_owned_count(s) < n: a block handle holds the velocities of its block only, and the catalogue is about whole groups); all-reduce
 * and single-rank sharded handles own all n and are served.  The call synchronises; a pending once-only report leaves through it as
 * through nb_groups (NB_ENOMEM, once): nothing is written then, *count included.  NB_EHIP, nothing written, if the union-find left
 * its bound, as in nb_groups.
 * Nothing of the handle changes: positions, velocities, acc[], frame counter, tree arrays and nb_tree_stats are untouched, and the
 * next step is bit-identical to one on a handle that never called this.  nb_groups, nb_neighbors and this call share their scratch
 * and may alternate on one handle at any radii.
 * Memory: nothing until the first call; then (growth only, freed by nb_destroy) nb_groups' 44 bytes per body of the replica and sort
 * storage, if those calls have not made them yet (the sort by label runs in the same arrays), plus 16 bytes per body (head flag,
 * rank, length / row by label), the scan's temporary storage and 224 bytes per 1024 bodies (the carries); once a filling call has run,
 * 184 bytes per group of the largest catalogue seen plus an eighth (the 13 sums and the record); the shared staging buffer is grown
 * to 80 bytes per group once a destination needs it.  Nothing is sized by n that depends on the count.
 * Cost: nb_groups' grouping, one more sort of n (label, index) pairs, and two reduction passes that are balanced over sorted
 * positions, not over groups: a workgroup reduces a fixed run of 1024 consecutive positions with a head-flagged segmented scan, and a
 * second, small launch adds the pieces of the groups that reach across runs, in run order.  All bodies in one group cost what all
 * singletons cost.  On an MI355X, Plummer spheres, min_members 2, records into nb_host_alloc memory (profiles/group_catalog_bench.log): at
 * 1 048 576 bodies with a mean of 1 / 5 / 31 links per body (145 091 / 73 466 / 28 567 groups in the catalogue) 0.94 / 1.44 / 2.69 ms,
 * of which the two reduction passes 0.12 / 0.11 / 0.10 ms, where nb_groups(label, size) alone takes 0.59 / 1.30 / 2.62 ms and the host
 * route (nb_groups' labels, nb_sync, numpy bincount with weights, one thread) 36 / 33 / 37 ms; the count query 0.58 / 1.23 / 2.54 ms;
 * into a pageable array 1.23 / 1.60 / 2.78 ms; at 262 144 bodies 0.45 / 0.88 / 0.87 ms (host route 5.1 - 7.4); at 8 388 608 (tree
 * handle, 1 148 923 / 565 389 / 227 560 groups) 5.20 / 5.67 / 7.98 ms (host route 314 - 327).  The reduction passes at 1 048 576 bodies
 * with every body a singleton: 0.21 ms; with all bodies in ONE group: 0.09 ms.
 * With nb_profile_enable the reduction passes (both, with their carry launches) are bracketed like a force launch and count as one
 * (nb_profile_read); the link kernel is not bracketed in this call. */
int nb_group_catalog(nb_sim *s, float radius, uint32_t min_members, nb_group *out, size_t capacity, size_t *count);

/* Unbinding: the potential of every body due to the OTHER MEMBERS OF ITS OWN friends-of-friends group, its energy in the group's rest
 * frame, and per group how many members are bound, which one is the most bound (the group's centre) and the group's self-potential
 * energy (with nb_group_catalog's mass x sigma2, the virial ratio: INTEGRATION.md has the recipe).  nb_potentials is the potential of the
 * whole system, the wrong quantity for unbinding; without this call a caller takes nb_groups' labels, nb_syncs 64 B per body and runs an
 * O(n_g^2) pass per group on the host.
 * GROUPS AND ROWS: exactly nb_group_catalog's at the same radius and min_members.  Row r of out describes the group of row r of the
 * catalogue: same label, same members, same order, same *count.
 * PLANES: phi and e hold n doubles each, indexed by body.  For a body i of a kept group G
 *     phi[i] = - sum_{j in G, j != i} m_j / sqrt(|x_j - x_i|^2 + eps^2)        e[i] = 1/2 |v_i - vel_G|^2 + phi[i]
 * vel_G is the vel of the catalogue's record, bit for bit; v_i and the weights w_i are taken as the catalogue takes them (the float
 * values widened to double, w_i = m_i > 0 ? m_i : 0).  On a dims = 3 handle z takes part in the distance and in |v - vel|^2; the grouping
 * stays the (x, y) projection.  A body whose group is not kept gets a quiet NaN in both planes.  The self term is left out by INDEX,
 * never by distance: members on one position each add -m_j / eps, and with eps = 0 only those bodies get values that are not finite.  A
 * singleton kept with min_members = 1 has phi = +0 and e = +0.
 * ARITHMETIC of phi: nb_potentials' rules inside the group; eps^2 is squared as the force launch squares it.  NB_FP32 handles: fp32
 * displacement, r^2 by fused multiply-adds onto eps^2, v_rsq_f32, the terms m_j * inv added by FMA into fp32 runs of at most 64 terms, the
 * runs added in fp64, the result fp64.  That gives nb_potentials' bar, which is derived and not measured: within 4e-6 relative of the fp64
 * sum of the same float values for masses >= 0.  NB_FP64 handles: fp64 throughout from the handle's own positions and masses, the terms
 * in the order of the sorted members (ascending body index).  THE ORDER of every sum is a function of the labels and n alone: the bodies
 * are sorted by (label, index), the sorted positions are cut into runs [64 k, 64 k + 64), an fp32 run sums the members of i's group
 * inside one run in ascending position, and the runs are added in ascending k (tests/group_binding_model.py).
 * RECORDS: bound, most_bound, e_min and potential come from one head-flagged segmented scan over the sorted order, fp64, no float atomic.
 * bound counts e < 0.  The argmin keeps the earlier position unless the later e is strictly smaller: ties go to the smallest body index,
 * a NaN e is never chosen, and a group none of whose e is below +inf reports NB_NO_NEIGHBOR and e_min = +inf.
 * COUNT QUERY AND CAPACITY: count may not be NULL.  With phi, e and out all NULL the call is the count query: NB_OK, *count written, the
 * sweep not run, the cost that of nb_group_catalog's count query.  out != NULL with capacity < *count is NB_EINVAL naming both numbers;
 * *count is written and nothing else.  Any of phi, e, out may be NULL on its own: a plane that is not asked for is not copied and not
 * written; the sweep runs if any of the three is asked for.  Only the first *count records of out are written.
 * CONSEQUENCES: two handles, and two calls on one handle, agree byte for byte.  Permuting the bodies relabels the groups and permutes the
 * planes, leaves members exact, leaves bound and most_bound equal wherever no e is within rounding of 0 or of the minimum, and changes
 * the doubles through the order of summation only.
 * WHICH HANDLES: every handle nb_group_catalog serves: fp32 and fp64, dims 2 and 3, direct and tree with any flags, all-reduce and
 * single-rank sharded handles.  NB_ESTATE, with the catalogue's message, on a handle with nb_owned_count(s) < n.
 * ERRORS: NB_EINVAL, naming the argument, before any device work: a NULL handle; a NULL count; nb_groups' rules for the radius;
 * min_members == 0.  NB_ESTATE while a split step is in flight.  The call synchronises; a pending once-only report leaves through it as
 * through nb_groups (NB_ENOMEM, once): nothing is written then, *count included.  NB_EHIP, nothing written, if the union-find left its
 * bound, as in nb_groups.
 * Nothing of the handle changes: positions, velocities, acc[], frame counter, tree arrays and nb_tree_stats are untouched, and the next
 * step is bit-identical to one on a handle that never called this.  It may alternate with nb_neighbors, nb_groups, nb_group_catalog and
 * nb_pair_counts on one handle at any radii.
 * phi, e and out may be any host memory: ranges known to be page-locked (nb_host_alloc / nb_host_register) are written by the copy engine
 * directly, anything else moves through the query calls' shared staging buffer.
 * Memory: nothing until the first call; the count query makes what nb_group_catalog's makes.  From the first filling call on (growth
 * only, freed by nb_destroy) 48 bytes per body of the replica on an fp32 handle, 64 on an fp64 one (the body's record in sorted order
 * 16 / 32, its segment 8, phi in sorted order 8, the two planes 16); per group of the largest catalogue seen plus an eighth, the
 * catalogue's 184 bytes and 32 for the record; the shared staging buffer is grown to 8 bytes per body or 32 per group once a
 * destination needs it.  Nothing sized by n depends on the count.
 * Cost: nb_group_catalog's front half (grouping, sort by label, pass A for vel), then a sweep proportional to the sum of n_g^2 over the
 * kept groups.  A linking length that percolates makes it the n^2 sweep: the caller chooses the radius, and nb_group_catalog's members
 * tells the cost beforehand.  A workgroup owns a tile of T = 512 consecutive sorted positions and walks the union of their segments
 * in LDS chunks; inside a giant group the chunks run nb_potentials' unmasked pair body, and only the two tiles at a segment's ends
 * evaluate pairs for foreign lanes: at most sum_g 2 T n_g wasted lane-pairs, T the tile.  On an MI355X, Plummer spheres, min_members 2,
 * e and records into nb_host_alloc memory (profiles/group_binding_bench.log; DESIGN.md section 6, "Group binding"): at 1 048 576 bodies
 * with a mean of 1 / 5 / 31 links per body (largest group 192 / 463 238 / 831 606; sum n_g^2 3.9e6 / 2.1e11 / 6.9e11) 1.06 / 44.1 /
 * 117.2 ms, of which the sweep 0.07 / 42.6 / 114.3 ms (5.0e12 / 6.1e12 pairs per second in the last two), where nb_group_catalog takes
 * 0.93 / 1.46 / 2.71 ms and the count query 0.56 / 1.22 / 2.54 ms; into pageable arrays 0.2 - 0.3 ms more; at 262 144 bodies 0.52 / 5.85 /
 * 13.2 ms (the host route at 1 link: nb_groups' labels, nb_sync, numpy per group, 528 ms); at 8 388 608 (tree handle) 6.17 ms at 1 link,
 * and the two percolated radii (sum n_g^2 1.5e13 / 4.3e13) were not run.  THE YARDSTICK: on a handle whose 262 144 bodies are ONE group
 * the sweep takes 10.60 ms where nb_potentials' direct sweep of the same pairs takes 9.80 ms, a ratio of 1.08; with 16 384 bodies in one
 * cell 0.61 against 0.18 ms: 32 workgroups, so a giant group in a SMALL system underfills the chip (a smaller tile has not been
 * written).  1 048 576 singletons / 524 288 pairs, min_members 1: 1.57 / 1.31 ms beside the catalogue's 2.21 / 1.49 ms.
 * With nb_profile_enable the sweep is bracketed like a force launch and counts as one (nb_profile_read); the count query brackets
 * nothing. */
int nb_group_binding(nb_sim *s, float radius, uint32_t min_members, double *phi, double *e,
                     nb_group_energy *out, size_t capacity, size_t *count);

/* The histogram of pair separations, DD(r): how many unordered pairs of bodies lie in each of nbins distance bins, counted on the
 * device; the answer is at most 64 integers however many bodies there are.  It is the raw material of the two-point correlation
 * function xi(r), the radial distribution function g(r) and a correlation dimension (INTEGRATION.md has the recipe).  Without it a
 * caller takes nb_neighbors' rows, which k <= 32 truncates exactly in the dense regions, or nb_syncs 8 - 64 B per body and runs a tree
 * or grid pass on the host every frame.
 * BINS: edges holds nbins + 1 floats, 1 <= nbins <= NB_PAIR_BINS_MAX.  e2[t] = edges[t] * edges[t], one fp32 multiply on the host, and
 * r2max = e2[nbins].  Bin b holds the pairs with e2[b] <= d2 < e2[b + 1]: closed below, open above.  counts[b] is exact, 64-bit; only
 * the nbins entries of counts are written.
 * PAIRS: d2 is nb_neighbors' predicate word for word: fp32, one rounding per operation, no contraction,
 *     dx = x_j - x_i      dy = y_j - y_i      d2 = dx * dx + dy * dy
 * Every unordered pair {i, j}, i != j, is counted once (d2(i, j) = d2(j, i) bit for bit).  Bodies on one position are a pair at
 * d2 = 0: counted in bin 0 when edges[0] == 0, in no bin otherwise.  Massless bodies take part.  A body with a non-finite coordinate
 * is in no pair; a pair whose d2 overflows to +inf is in no bin.
 * WHICH BODIES: nb_neighbors' rules.  All n bodies of the CURRENT replica (on a sharded handle it must be complete, as for nb_energy),
 * at the positions of all work enqueued so far, exactly as nb_sync_positions defines them.  An NB_FP64 handle's positions are rounded
 * to float first; a dims = 3 handle is projected on (x, y).  Every kind of handle: direct or tree, any flags, sharded or not.  A handle
 * that owns [i_begin, i_begin + i_count) counts the pairs whose LOWER global index lies in its block, nb_energy's convention: the
 * counts of the ranks of a sharded run add up to the unsharded counts; an all-reduce or single-rank handle owns all n and returns the
 * total.  CONSEQUENCES: the counts are integers and do not depend on the order of the sweep: two handles, and two calls on one
 * handle, agree bit for bit; permuting the bodies leaves every count unchanged on a handle that owns all n; and the counts add up to
 * n_finite (n_finite - 1) / 2, n_finite the bodies with finite coordinates, when edges[0] == 0 and r2max exceeds every d2.
 * ERRORS: NB_EINVAL, naming the argument and the offending index, before any device work, in this order: a NULL handle, edges or
 * counts; nbins outside 1 .. 64; a non-finite edge; edges[0] < 0 (-0 is 0); edges not strictly ascending; e2[t] >= e2[t + 1] for some
 * t (edges whose squares tie or vanish in fp32, such as 1e-30f and 2e-30f, are refused: an empty or inverted bin is not silently
 * produced); r2max not finite or 0 (nb_neighbors' rule for its radius, applied to edges[nbins]).  NB_ESTATE while a split step is in
 * flight.  The call synchronises; a pending once-only report (collision capacity, failed tree build) leaves through it as through
 * nb_neighbors (NB_ENOMEM, once), and nothing is written to counts then.
 * Nothing of the handle changes: positions, velocities, acc[], frame counter, tree arrays and nb_tree_stats are untouched, and the
 * next step is bit-identical to one on a handle that never called this.  nb_neighbors, nb_groups, nb_group_catalog and this call
 * share the cell scratch and may alternate on one handle at any radii.
 * Memory: nothing until the first call; then (growth only, freed by nb_destroy) nb_neighbors' 40 bytes per body of the replica and its
 * sort storage, if that call has not made them yet; one row of 65 64-bit partials per workgroup of the count kernel, at most 8
 * workgroups per compute unit (sized by the launch, not by n: 1.02 MiB on an MI355X); 65 words on the device and 65 page-locked ones.
 * No staging buffer: the answer is at most 520 bytes.
 * Cost: the bodies are sorted by the cell of a grid of cell size edges[nbins] x (1 + 2^-16) and every unordered pair of bodies in the
 * same or adjacent cells is tested once (half the pairs nb_neighbors tests), each against every edge of the bin capacity in use (8,
 * 16, 32 or 64, the smallest that holds nbins): the cost is proportional to those pairs times that capacity.  A last edge that
 * covers the system is the n^2 sweep.  The caller chooses the edges.  On an MI355X, Plummer spheres, last edge for a mean of
 * 5 / 31 neighbours per body, the whole call (profiles/pair_counts_bench.log): at 1 048 576 bodies 8 bins 0.31 / 0.35 ms, 16 bins 0.32 /
 * 0.39 ms, 64 bins 0.66 / 1.30 ms, of which the count kernel 0.07 / 0.12, 0.08 / 0.16 and 0.43 / 1.06 ms, where the yardstick,
 * nb_neighbors' count-only call at the same radius on the same handle, takes 0.59 / 0.61 ms (its search kernel 0.13 / 0.14 ms, and it
 * copies 4 bytes per body out); at 262 144 bodies 16 bins 0.18 / 0.20 ms (64 bins 0.27 / 0.46; count-only call 0.26 / 0.29); at
 * 8 388 608 (tree handle) 16 bins 1.53 / 1.99 ms, 64 bins 4.08 / 8.58 ms (count-only call 3.77 / 3.79).  The count kernel of capacity
 * 64 takes 3.4 - 7.1 times that of capacity 16 for 3.8 times the edges: its 65 counters leave 2 waves per SIMD and its edges no longer
 * fit the scalar registers ("Pair counts").  16 384 bodies in ONE cell, 16 bins: 2.4 ms, 5.6e10 pairs per second.
 * The per-lane build's count kernel is within 0.02 ms of the cooperative one at 8 and 16 bins on these spheres (faster in seven rows
 * of eight) and 1.4 - 1.5 times slower at 64.  A binary search with a per-wave LDS histogram in place of the cumulative counters has
 * not been tried; neither has the capacity of 32 been timed.
 * With nb_profile_enable the count kernel is bracketed like a force launch and counts as one (nb_profile_read). */
#define NB_PAIR_BINS_MAX 64
int nb_pair_counts(nb_sim *s, const float *edges, uint32_t nbins, uint64_t *counts);

/* Radial profiles: for each of ncenters POINTS, per shell about it, how many bodies there are and the fp64 sums of mass and velocity
 * moments, reduced on the device.  It is what a caller does with a group once nb_group_catalog has said where it is and
 * nb_group_binding which body is its centre: the surface or volume density profile, the enclosed mass and the half-mass radius, the
 * radial and tangential velocity dispersion, the rotation curve (INTEGRATION.md has the recipe).  Without it a caller nb_syncs 64 B per
 * body and runs a numpy pass per centre.
 * INPUTS: centers holds ncenters rows of dims floats, (x, y), or (x, y, z) on a dims = 3 handle: nb_sync_positions' stride.  vcenters
 * holds the same shape in doubles; NULL means all zero.  edges holds nbins + 1 floats, 1 <= nbins <= NB_PROFILE_BINS_MAX.
 * out[c * nbins + b] is shell b of centre c; every one of the ncenters * nbins records is written, an empty shell is all zero.
 * SHELLS AND DISTANCE: nb_pair_counts' rule word for word.  e2[t] = edges[t] * edges[t], one fp32 multiply on the host; shell b holds
 * the bodies with e2[b] <= d2 < e2[b + 1]: closed below, open above.  d2 is fp32, one rounding per operation, no contraction:
 *     dx = x_j - c_x      dy = y_j - c_y      d2 = dx * dx + dy * dy
 * and on a dims = 3 handle dz = z_j - c_z, d2 = (dx * dx + dy * dy) + dz * dz: a profile wants the 3-D radius (nb_group_binding also
 * lets z into its distance).  A centre is a point, not a body: there is no self term.  A body that lies on a centre is in shell 0
 * when edges[0] == 0 and in no shell otherwise.  A body with a non-finite coordinate is in no shell; so is a d2 that overflows to
 * +inf.  count is exact.
 * MOMENTS, all fp64, one rounding per operation, no contraction.  A body's values are the float values nb_sync returns for it,
 * widened to double (an NB_FP64 handle's values are rounded to float first: the catalogue's rule); w = m > 0 ? m : 0;
 *     X = (double)x_j - (double)c_x, Y, Z likewise      r2 = (X X + Y Y) + Z Z      r = sqrt(r2)
 *     u = (double)v_j - vcenter      v_r = ((X u_x + Y u_y) + Z u_z) / r      |u|^2 = (u_x u_x + u_y u_y) + u_z u_z
 * and a body adds 1 to count, w to mass, w r to mr, w r2 to mr2, w v_r to mvr, (w v_r) v_r to mvr2, w |u|^2 to mv2 and
 * w (X u_y - Y u_x) to mlz: the z component of the angular momentum on either kind of handle (the Z terms are absent in 2-D).  Where
 * r == 0 the body adds to count, mass and mv2 only; its other terms are +0.  A massless, negative-mass or NaN-mass body is counted
 * and weighs nothing.  A shell that holds a body with a non-finite mass or velocity gets what the arithmetic gives.
 * ORDER: every sum is taken in an order that is a function of the bodies, the centres and the edges alone, and there is no
 * floating-point atomic anywhere.  The bodies are sorted by the cell of a grid of cell size edges[nbins] x (1 + 2^-16) with a stable
 * sort, (cell key, body index) ascending; a centre's CANDIDATES are the bodies of the 3 x 3 cells round its own cell, the cell row below
 * first, each row in sorted order.  The candidates are cut into pieces of 1024.  Inside a piece a shell's sum starts at +0 and takes
 * the terms of its bodies from left to right in candidate order.  A centre with at most 1024 candidates is one piece.  Otherwise
 * the pieces k = 0 .. K - 1 are added so: S_s = piece s + piece (s + 32) + piece (s + 64) + ..., left to right, for s = 0 .. 31 (+0
 * where s >= K), then S_s += S_(s + h) for h = 16, 8, 4, 2, 1, and the sum is S_0 (tests/radial_profiles_model.py states the contract,
 * not this order).  CONSEQUENCES: two handles, and two calls on one handle, agree byte for byte; permuting the bodies leaves every
 * count unchanged and changes the doubles through the order of summation only; permuting the centres permutes the rows of out byte
 * for byte, and a centre's row does not depend on the other centres of the call.
 * WHICH BODIES: all n bodies of the CURRENT replica, at the positions of all work enqueued so far: nb_neighbors' rules.  Every kind
 * of handle nb_group_catalog serves: fp32 and fp64, dims 2 and 3, direct and tree with any flags, all-reduce and single-rank sharded
 * handles.  NB_ESTATE, with the catalogue's message, on a handle with nb_owned_count(s) < n: a block handle holds only its block's
 * velocities.
 * ERRORS: NB_EINVAL, naming the argument and the offending index, before any device work, in this order: a NULL handle, centers,
 * edges or out; ncenters outside 1 .. 1 048 576; nbins outside 1 .. 64; ncenters * nbins > 1 048 576 (64 MiB of records: the cap is a
 * condition, not a measurement; it keeps the device plane and the staging buffer bounded); nb_pair_counts' edge rules word for word
 * (finite, edges[0] >= 0, strictly ascending, squares strictly ascending in float, r2max finite and not 0); a non-finite centre
 * coordinate; a non-finite vcenters value.  NB_ESTATE while a split step is in flight.  The call synchronises; a pending once-only
 * report leaves through it as through nb_neighbors (NB_ENOMEM, once), and nothing is written then.  NB_ENOMEM if the centres see
 * more than 2^31 - 1 pieces of candidates between them.
 * Nothing of the handle changes: positions, velocities, acc[], frame counter, tree arrays and nb_tree_stats are untouched, and the
 * next step is bit-identical to one on a handle that never called this.  It may alternate with nb_neighbors, nb_groups,
 * nb_group_catalog, nb_group_binding and nb_pair_counts on one handle at any radii.
 * out may be any host memory: ranges known to be page-locked (nb_host_alloc / nb_host_register) are written by the copy engine
 * directly, anything else moves through the query calls' shared staging buffer.
 * Memory: nothing until the first call; then (growth only, freed by nb_destroy) nb_neighbors' 40 bytes per body of the replica and its
 * sort storage, if that call has not made them yet; 84 bytes per centre of the largest call seen (the centre 12, its velocity 24,
 * its three cell ranges 24, two piece counts 8 and their prefix sums 16) and the scans' temporary storage; 64 bytes per record of
 * the largest ncenters * nbins seen, at most 64 MiB, and as much page-locked staging once a destination needs it; and 64 bytes x nbins
 * per PIECE OF A CENTRE THAT IS SPLIT, which no cap bounds: a centre whose last edge covers all n bodies takes n / 1024 rows of nbins
 * records (8 MiB at 8 388 608 bodies and 16 shells), and m such centres take m times that.  The caller chooses the edges.
 * Cost: the cell sort of nb_pair_counts, one small launch that finds every centre's ranges, two prefix sums over the centres, one
 * read-back of their totals, then the sweep: ONE WAVE PER PIECE, so one centre that covers the system is n / 1024 waves all over the
 * chip and 65 536 small centres are 65 536 single waves; a second launch adds the rows of the split centres.  The cost of the sweep
 * is proportional to the candidates, the bodies in the 3 x 3 cells round each centre.  On an MI355X, Plummer spheres, 16 shells, records
 * into nb_host_alloc memory (profiles/radial_profiles_bench.log; DESIGN.md section 6, "Radial profiles"): ONE centre at the origin whose
 * last edge lies beyond the whole sphere, at 262 144 / 1 048 576 / 8 388 608 (tree handle) bodies 0.22 / 0.32 / 1.14 ms, of which the
 * sweep 0.06 / 0.09 / 0.31 ms, where nb_raster's call on the same handle takes 0.52 / 0.64 / 1.57 ms and the host route (nb_sync, numpy
 * histograms with weights, one thread) 43 / 170 / 1 430 ms; into a pageable array the same within 0.01 ms.  65 536 centres, the most
 * bound bodies of nb_group_binding's groups at 1 048 576 bodies and a mean of 1 link per body, last edge 4 linking lengths: 2.01 ms,
 * of which the sweep 0.12 ms and most of the rest the 64 MiB of records (4.55 ms into a pageable array), where the host route (nb_sync,
 * scipy's cKDTree, numpy per centre) takes 1 685 ms.  16 384 bodies in ONE cell: one centre 0.15 ms (sweep 0.06 ms: 16 waves do not
 * fill the chip); every body a centre 4.96 ms, 6.0e10 body-centre tests per second (256 MiB of partial rows).  The other form of the
 * per-shell sum, a masked wave reduction per occupied shell, has not been written.
 * With nb_profile_enable the sweep (with its second launch) is bracketed like a force launch and counts as one (nb_profile_read). */
#define NB_PROFILE_BINS_MAX 64
int nb_radial_profiles(nb_sim *s, const float *centers, const double *vcenters, size_t ncenters, const float *edges, uint32_t nbins,
                       nb_shell *out);

/* The field at arbitrary POINTS: potential and acceleration where the caller asks, not only at the bodies (nb_potentials,
 * nb_accelerations).  With d = x_j - p:
 *     phi(p) = - sum_j m_j / sqrt(|d|^2 + eps^2)        acc(p) = sum_j m_j d / (|d|^2 + eps^2)^(3/2)        (G = 1, the handle's eps)
 * It is the potential or acceleration map under nb_raster's view, the circular velocity v_c^2 = r |a_r| beside nb_radial_profiles'
 * shells, the tidal field across a group of nb_group_catalog, the force on a probe before it is spawned (INTEGRATION.md has recipes).
 * Without it a caller adds massless tracer bodies and creates the handle again (another n, plan, root cell and set of indices), or
 * nb_syncs 64 B per body and sums on the host.
 * INPUTS: points holds npoints rows of dims floats, (x, y), or (x, y, z) on a dims = 3 handle: nb_sync_positions' stride and
 * nb_radial_profiles' centers.  phi receives npoints doubles, acc npoints x dims doubles.  Either of phi / acc may be NULL, not
 * both; a plane that is not asked for is neither computed, written nor copied, and the bits of one plane do not depend on whether
 * the other was asked for.
 * WHICH BODIES: all n bodies of the CURRENT replica at the positions of all work enqueued so far: nb_potentials' rules (on a
 * sharded handle the replica must be complete).  Every kind of handle: fp32 and fp64, dims 2 and 3, either integrator, sharded or
 * not, direct or tree with any flags.
 * A POINT IS NOT A BODY: there is no self term and no mask by index.  A point that lies on a body takes -m_j / eps into phi and
 * nothing into acc (d = 0).  With eps = 0 a pair whose r^2, in the arithmetic of the sweep, is exactly 0 adds nothing to either
 * output, and the result stays finite.
 * ARITHMETIC of the direct sweep (every handle but a NB_FLAG_TREE_ENERGY one: nb_potentials' split).  NB_FP32: per pair a float
 * displacement, r^2 by fused multiply-adds onto eps^2, inv = v_rsq_f32(r^2), then phi += m_j inv and, with s = m_j ((inv inv) inv),
 * a_c += d_c s, each a fused multiply-add in fp32 over runs of 64 consecutive j (a run starts at every multiple of 64 from j = 0),
 * the runs added in fp64, the result fp64.  phi is nb_potentials' arithmetic word for word: within 4e-6 relative of the fp64 sum,
 * and, with eps > 0, phi at the position of a massless body has the bits of that body's nb_potentials value.  Each component of
 * acc is within 4.2e-6 of S_c = sum_j |term_j| of that component (6.5 ulp per term and the 63 roundings of a run;
 * tests/field_model.py is the numpy statement): the bound is on the cancellation-free scale, not on |a|.  NB_FP64: the float points
 * widened, fp64 throughout, the terms added in j order (1.4e-16 per reciprocal square root).
 * DETERMINISM: a point's row depends on the bodies, eps, the precision and that point only: not on npoints, on the launch
 * geometry or on the other points.  Two handles agree bit for bit, and permuting the points permutes the rows byte for byte.
 * NB_FLAG_TREE_ENERGY handles: the tree build of nb_energy and the leaf residual run, then one per-lane walker per point.  A point
 * walks exactly as a massless body at that position walks: nb_potentials' float64 terms for phi (quadrupole and leaf residual
 * included) and, in the same loop, the float32 terms of the force walk for acc with the handle's own rsqrt_mode, widened on
 * store: phi has the bits nb_potentials gives a massless body there, and acc those nb_accelerations gives it.  A leaf exactly under
 * the point gives no term (d^2 = 0): the one difference from the direct sweep.  NB_FLAG_TREE_RELATIVE is not applied (a point has
 * no previous acceleration): the walk is the theta walk.  The points are walked in caller order, 64 consecutive points to a wave:
 * a row-major image is coherent enough for the per-lane walk; sorting the points and a wave-uniform group walk have not been
 * written.  As for nb_potentials the tree arrays are rebuilt, nb_tree_stats describes this build, and a failed build makes THIS
 * call return NB_ENOMEM through the once-only report, with nothing written.
 * Nothing else of the handle changes: positions, velocities, acc[] and the frame counter are untouched, and the next step is
 * bit-identical to one on a handle that never called this.
 * ERRORS: NB_EINVAL before any device work, in this order: a NULL handle; NULL points; phi and acc both NULL; npoints outside
 * 1 .. NB_FIELD_POINTS_MAX (the cap is a condition that bounds the scratch, not a measurement); the first non-finite coordinate,
 * named by index and axis.  NB_ESTATE while a split step is in flight.  The call synchronises; a pending once-only report leaves
 * through it as through nb_radial_profiles (NB_ENOMEM, once), and nothing is written then.  phi and acc may be any host memory:
 * ranges known to be page-locked (nb_host_alloc / nb_host_register) are written by the copy engine directly, anything else moves
 * through the query calls' shared staging buffer.
 * Memory: nothing until the first call; then (growth only, freed by nb_destroy) 4 dims + 8 (dims + 1) bytes per point of the largest
 * call seen (128 MiB at the cap in 2-D), and as much page-locked staging as the larger plane once a destination needs it.
 * Cost: npoints x n pairs on the direct sweep.  On an MI355X, fp32 2-D Plummer spheres, as many points as bodies, 262 144 / 1 048 576
 * (profiles/field_bench.log; DESIGN.md section 6, "Field at points"): the sweep alone, phi 9.93 / 140.2 ms, acc 14.67 / 204.6 ms, both
 * 15.80 / 222.4 ms, where on the same handle nb_potentials' sweep takes 9.92 / 139.9 ms and a one-sided force launch 11.17 / 179.7 ms:
 * the joint sweep takes less than those two together, the acc plane alone more than the force launch (general masses, and an fp64
 * add per output per run of 64).  The whole call, both planes, into a pageable array 16.41 / 224.1 ms, into nb_host_alloc memory
 * 16.08 / 223.4 ms.  NB_FLAG_TREE_ENERGY handles at theta = 0.5, a 1024 x 1024 row-major grid over the half-mass square, both planes
 * into a pageable array, at 1 048 576 / 8 388 608 bodies: 5.02 / 13.59 ms, of which the walk kernel 2.02 / 4.07 ms; the same points
 * shuffled: 8.46 / 19.43 ms, walk 5.48 / 9.94 ms.
 * With nb_profile_enable the sweep (the walk kernel on a NB_FLAG_TREE_ENERGY handle) is bracketed like a force launch and counts as
 * one (nb_profile_read). */
#define NB_FIELD_POINTS_MAX 4194304
int nb_field(nb_sim *s, const float *points, size_t npoints, double *phi, double *acc);

/* Acceleration and jerk of every body at the handle's CURRENT positions and velocities, as fp64: the evaluation of
 * NB_INTEGRATOR_HERMITE4 (see the enum), by the step's own kernel.  What a time-step criterion starts from: dt ~ eta |a| / |j|.
 * acc, jerk: dims * n doubles each, packed per body (nb_field's acc plane); either may be NULL, both NULL is NB_EINVAL.
 * NB_INTEGRATOR_HERMITE4 handles only: NB_EINVAL on any other, naming its integrator.  NB_ESTATE while a split step is in flight.
 * It touches nothing: acc[], the carried pair, positions, velocities and the frame stay as they are, and the next step is
 * bit-identical to one on a handle that never called this.  Either plane alone has the bits it has in the joint call (both are
 * always computed).  Note that between steps acc[] holds a1, the evaluation at the PREDICTED point, while this call evaluates at
 * the corrected state.  The call synchronises; the planes move out like nb_field's (page-locked destinations directly, others through
 * the query calls' shared staging buffer).  With nb_profile_enable the sweep counts as one force launch. */
int nb_jerks(nb_sim *s, double *acc, double *jerk);

/* NB_FLAG_TREE_RELATIVE: set alpha of the acceleration-relative opening test between steps (the evaluations already enqueued keep
 * theirs).  alpha must be finite and >= 0 (NB_EINVAL otherwise); 0 switches the test off.  NB_ESTATE on a handle created without
 * the flag.  At creation alpha is 0.005: GADGET-2's customary ErrTolForceAcc, not a number measured for this library.  A setter
 * and not an nb_params field: sizeof(nb_params) and the ABI number stay. */
int nb_tree_alpha(nb_sim *s, float alpha);

/* The body order of the handle (NB_FLAG_BODY_ORDER above), read and tuned.  *every_out (may be NULL) receives the force evaluations
 * from one sort to the next, 0 on a handle that sweeps its bodies in the caller's order.  every > 0 sets that cadence from the next
 * evaluation on (0 keeps it; the count of evaluations since the upload is kept, so set it before stepping for reproducible bits).
 * perm_out (may be NULL; n entries; synchronises) receives the order of the last sort: perm_out[k] is the caller's index of the k-th
 * body along the curve, a permutation of 0 .. n-1; before the first evaluation after an upload it is the order of the uploaded
 * bodies.  NB_ESTATE when every or perm_out is given and the handle has no order.  A setter and not an nb_params field:
 * sizeof(nb_params) and the ABI number stay. */
int nb_body_order(nb_sim *s, uint32_t every, uint32_t *perm_out, uint32_t *every_out);

/* Counters: Simulation::frame (Simulation.hpp:53) and sizes. */
uint64_t nb_frame(const nb_sim *s);
size_t   nb_count(const nb_sim *s);        /* n of the whole system */
size_t   nb_owned_begin(const nb_sim *s);
size_t   nb_owned_count(const nb_sim *s);

/* ---- dump / restore (build-defined: the reference has no file I/O) ----
 * File = 64-byte header {"NBODYAMD", u32 version, u32 sizeof(nb_body), u64 n,
 * u64 frame, f32 eps, f32 dt, i32 precision, i32 rsqrt_mode, zero pad} followed
 * by n raw nb_body records (padding zeroed) — the reference's only externally
 * visible state, `std::vector<Body>`. */
int nb_dump(nb_sim *s, const char *path);
/* Host-only halves of the same format (usable without a GPU). */
int nb_write_bodies(const char *path, const nb_body *bodies, size_t n, uint64_t frame,
                    const nb_params *params);
int nb_read_header(const char *path, size_t *n, uint64_t *frame, nb_params *params);
int nb_read_bodies(const char *path, nb_body *out, size_t n);

/* ---- sharded stepping (one process per GPU) ----------------------
 * A handle created with i_count < n integrates its block only and needs the
 * other blocks' positions each step.  The exchange itself is the host's
 * (torch.distributed / RCCL all-gather writing straight into the device
 * position replica), overlapped with the local-tile force:
 *
 *   nb_step_begin(s, dt)   enqueue: force from the OWNED j-block (already resident)
 *   ... host runs the all-gather into nb_pos_buffer(s, NB_POS_CURRENT) on its comm stream ...
 *   nb_step_finish(s)      enqueue: force from the remote j-blocks (one launch over
 *                          "everything but my block"), kick, drift;
 *                          new owned positions land in the NEXT replica, which
 *                          becomes CURRENT.
 * Stream ordering between the two calls and the collective is the caller's
 * (they share params.stream, or use events). */
enum { NB_POS_CURRENT = 0, NB_POS_NEXT = 1 };
/* Which exchange a sharded handle needs between nb_step_begin and nb_step_finish:
 *   NB_SHARD_ALLGATHER   (i_count < n): begin = local-tile force; host all-gathers the positions
 *                        into nb_pos_buffer(CURRENT) (may overlap begin); finish = remote force,
 *                        kick, drift.  One-sided kernels; one collective per step.
 *   NB_SHARD_SYMMETRIC   (shard_world > 1, tiled, eps >= 1e-12 (fp32) / > 0 (fp64), large n, equal blocks of whole 2048-particle
 *                        tiles): every rank evaluates 1/world of the UNORDERED pairs with the symmetric
 *                        kernel: begin = the pairs inside its own block (overlaps the all-gather still in
 *                        flight); host waits for the all-gather; nb_step_mid = its share of the cross-block
 *                        pairs, then the partial acceleration of ALL particles into nb_acc_buffer(0); host
 *                        reduce-scatters it (sum) into nb_acc_buffer(1); finish = kick, drift of the owned
 *                        block; host starts the all-gather of the new positions.  (From 8 ranks on,
 *                        nb_step_mid also starts a held-back share of the own-block pairs on a side stream;
 *                        it runs while the reduce-scatter is in flight and nb_step_finish adds its result to
 *                        nb_acc_buffer(1) — nothing changes for the host.)
 *   NB_SHARD_ALLREDUCE   (NB_FLAG_SHARD_ALLREDUCE, shard_world > 1, i_begin = 0, i_count = n, otherwise as
 *                        NB_SHARD_SYMMETRIC): every rank evaluates its 1/world of the unordered pairs and then
 *                        integrates ALL n particles itself: begin = all its items, then its partial acceleration of
 *                        every particle into nb_acc_buffer(0); the host ALL-REDUCES that buffer in place (sum; every
 *                        rank must receive the same bits, which ring / tree all-reduces deliver); finish = kick, drift of
 *                        all n.  One collective per step, no position exchange; every rank holds the whole state
 *                        (nb_sync returns all n bodies, nb_energy the total). */
enum { NB_SHARD_NONE = 0, NB_SHARD_ALLGATHER = 1, NB_SHARD_SYMMETRIC = 2, NB_SHARD_ALLREDUCE = 3 };
int   nb_shard_protocol(const nb_sim *s);
/* Exchange for a host that drives SEVERAL sharded handles from one process (e.g. one per GPU of
 * the node, no RCCL): every handle's owned block of its CURRENT replica is copied into the CURRENT
 * replica of every other handle (peer copies; the handles may sit on different devices).  Call it
 * after nb_step_finish (before the next nb_step_finish / nb_step_mid); it waits for the handles'
 * enqueued work and returns when the copies are done. */
int   nb_exchange_positions(nb_sim *const *sims, int count);
/* Same host, NB_SHARD_SYMMETRIC handles (all `count` ranks of the run, in rank order): the in-process
 * reduce-scatter — every handle's nb_acc_buffer(1) receives the sum, in rank order, of all handles'
 * partial accelerations of its block.  Call it between nb_step_mid and nb_step_finish. */
int   nb_exchange_accelerations(nb_sim *const *sims, int count);
/* Same host, NB_SHARD_ALLREDUCE handles: the in-process all-reduce — every handle's nb_acc_buffer(0) receives the sum,
 * in rank order, of all handles' partial accelerations.  Call it between nb_step_begin and nb_step_finish. */
int   nb_exchange_allreduce(nb_sim *const *sims, int count);
void *nb_acc_buffer(nb_sim *s, int which);   /* 0: full-n partial, 1: owned block sum (NULL if unused) */
int   nb_step_begin(nb_sim *s, float dt);
int   nb_step_mid(nb_sim *s);      /* NB_SHARD_SYMMETRIC only (no-op otherwise): see below */
int   nb_step_finish(nb_sim *s);
void *nb_pos_buffer(nb_sim *s, int which);   /* device pointer, n*(x,y) reals */
size_t nb_pos_rows(const nb_sim *s);         /* rows each position replica holds: >= n (padded to world * ceil(n / world) for a sharded handle) */
void *nb_stream(nb_sim *s);                  /* hipStream_t in use */

/* Element layout of the device buffers above: positions / accelerations are `reals_per_element` reals per particle
 * (2: (x, y); 4 for dims = 3: {x, y, z, m} / {ax, ay, az, 0}) of `bytes_per_real` bytes (4 or 8). */
int   nb_element_layout(const nb_sim *s, int *reals_per_element, int *bytes_per_real);
int   nb_device(const nb_sim *s);            /* HIP device ordinal the handle lives on */
int   nb_shard_rank(const nb_sim *s, int *world);   /* nb_params.shard_rank (and shard_world) the handle was created with */

/* ---- C-level multi-GPU exchange over RCCL -----------------------------------------
 * north_star / SURVEY §8e: "host code stays in C ... an RCCL all-gather of positions over xGMI each step, overlapped
 * with local-tile force compute on a second HIP stream".  Replaces the reference's only fan-out, std::async over
 * i-chunks inside one process (Simulation.hpp:180-213).  An nb_comm binds sharded handles to an RCCL communicator,
 * gives each a communication stream, and runs the step loop of their protocol (nb_shard_protocol) entirely
 * STREAM-ORDERED: force / kick / drift on the handle's stream, ncclAllGather / ncclReduceScatter / ncclAllReduce on
 * the communication stream, HIP events between the two; the host only enqueues and never blocks inside the loop.
 * Two ways to form the communicator:
 *   nb_comm_create_all   ONE process drives all ranks, one handle per device (ncclCommInitAll); the collectives of a
 *                        step are issued as one ncclGroup;
 *   nb_comm_create_rank  one process per GPU (ncclCommInitRank): rank 0 calls nb_comm_unique_id and hands the
 *                        NB_COMM_ID_BYTES to the other ranks out of band (a file, MPI, a torch.distributed broadcast).
 * Handles: created with shard_rank / shard_world, rank r owning the block [r n/world, +n/world) (equal blocks, which
 * the in-place all-gather and the reduce-scatter need; in the all-gather protocol world need not divide n: blocks of
 * ceil(n / world) particles, the last one shorter, equal counts moved over padded replicas — nb_params.pos_rows),
 * or all n particles for NB_SHARD_ALLREDUCE; an unsharded
 * handle forms a communicator of one rank (its all-gather is RCCL's one-rank no-op).  RCCL is loaded at first use
 * (librccl.so.1); without it nb_comm_create_* fail with NB_ENODEVICE — there is no other transport behind this API.
 * Like a handle, an nb_comm is driven by ONE thread, and its handles must outlive it (nb_comm_destroy first).  Between
 * nb_comm_step calls the handles may be read (nb_comm_flush, then nb_sync / nb_energy / nb_momentum) but not stepped by
 * other means.  If a call fails half-way through a step (a HIP or RCCL error), the run cannot be continued: the communicator is
 * marked failed (an open ncclGroup is closed, further nb_comm_step / _flush / _wait return NB_ESTATE) and nb_comm_destroy
 * then ABORTS the RCCL communicator (ncclCommAbort) instead of synchronising with peers that may never arrive; destroy the
 * communicator and the handles.  A FAILED communicator leaks on purpose what could block if released: its communication
 * stream always, and the RCCL communicator itself where the transport has no ncclCommAbort (ncclCommDestroy may wait for
 * the very peers that never arrived). */
typedef struct nb_comm nb_comm;
#define NB_COMM_ID_BYTES 128
int      nb_comm_unique_id(void *id_out /* NB_COMM_ID_BYTES */);
nb_comm *nb_comm_create_rank(nb_sim *s, const void *id, int rank, int world);
nb_comm *nb_comm_create_all(nb_sim *const *sims, int count);
/* Enqueue nsteps steps (dt <= 0 -> each handle's params.dt).  Returns as soon as everything is enqueued. */
int      nb_comm_step(nb_comm *c, float dt, int nsteps);
/* Make the handles' compute streams wait (on the device) for the collectives still in flight, so that nb_sync /
 * nb_energy / nb_momentum / nb_wait on a handle see complete replicas; nb_comm_wait also blocks the host until
 * everything enqueued on the compute and communication streams is done. */
int      nb_comm_flush(nb_comm *c);
int      nb_comm_wait(nb_comm *c);
void     nb_comm_destroy(nb_comm *c);        /* waits; the handles stay valid and are destroyed by their owner */
int      nb_comm_info(const nb_comm *c, int *protocol, int *world, int *local_handles, int *rccl_version);
/* NB_OK iff the transport (librccl) can be loaded in this process; every rank of a one-process-per-GPU job checks this, and
 * the ranks agree on the answer, BEFORE any of them enters the blocking communicator formation of nb_comm_create_rank. */
int      nb_comm_available(int *rccl_version);
/* Per-phase timing inside the library's loop (attribution of a sharded step when no Python driver is around to time it):
 * with profiling on, HIP events are recorded on each handle's COMPUTE stream around every compute-stream operation of the
 * schedule; nb_comm_phase_read returns, for local handle `handle`, the milliseconds summed over the steps since the last
 * reset — as the compute stream sees them, waits for the collectives included:
 *   NB_PH_LOCAL    nb_step_begin: pairs inside the own block / local j-block / (all-reduce protocol) all of the rank's pairs
 *   NB_PH_AG_WAIT  waiting for the all-gather of the previous step
 *   NB_PH_CROSS    nb_step_mid: the rank's cross-block pairs + gather of the slabs (symmetric protocol)
 *   NB_PH_REDUCE   waiting for the reduce-scatter / all-reduce of the accelerations
 *   NB_PH_FINISH   nb_step_finish: (all-gather protocol: remote blocks' force,) kick, drift
 * and the number of steps they cover.  The host runs at most 128 marked steps ahead of the device.  Off by default. */
enum { NB_PH_LOCAL = 0, NB_PH_AG_WAIT = 1, NB_PH_CROSS = 2, NB_PH_REDUCE = 3, NB_PH_FINISH = 4, NB_COMM_PHASES = 5 };
int      nb_comm_profile(nb_comm *c, int on);
int      nb_comm_phase_read(nb_comm *c, int handle, double *phase_ms /* NB_COMM_PHASES */, uint64_t *steps, int reset);
/* The RCCL id of a one-process-per-GPU launch travelling through a FILE (hosts without MPI or a torch process group):
 * rank 0 publishes {magic, nonce, id} atomically (temporary file + rename; a stale file of an earlier launch is removed
 * first), the other ranks wait for a file that carries THEIR launch's nonce — a left-over file of a crashed run, or one
 * still being replaced, is ignored — at most timeout_ms (NB_EIO after that).  Host-only (no GPU needed). */
int      nb_comm_id_publish(const char *path, uint64_t nonce, const void *id /* NB_COMM_ID_BYTES */);
int      nb_comm_id_await(const char *path, uint64_t nonce, void *id_out /* NB_COMM_ID_BYTES */, int timeout_ms);

/* ---- measurement ------------------------------------------------------------ */
/* When enabled, every force-kernel launch is bracketed by HIP events on the
 * handle's stream; nb_profile_read returns the summed kernel time and launch
 * count since the last reset (it synchronises). */
int nb_profile_enable(nb_sim *s, int on);
int nb_profile_read(nb_sim *s, double *force_ms_total, uint64_t *force_launches, int reset);

/* Describe the launch geometry chosen for the force kernel (for logs/DESIGN). */
int nb_describe(nb_sim *s, char *buf, size_t buflen);

/* ---- host utilities ----------------------------------------------------------- */
/* Synthetic workload: 3-D Plummer sphere (a = M = G = 1,
 * Aarseth-Henon-Wielen sampling, r <= 20) projected on (x,y),(vx,vy); equal
 * masses 1/n, radius 0, acc 0.  mt19937(seed) raw outputs mapped (u+0.5)/2^32. */
int nb_plummer_2d(nb_body *out, size_t n, uint32_t seed);
/* The same sample without the projection: a true 3-D Plummer sphere (z in NB_Z) for dims = 3. */
int nb_plummer_3d(nb_body *out, size_t n, uint32_t seed);
/* The bodies the reference's `Simulation()` starts from — Simulation.hpp:58-65 -> uniform_disc(n),
 * :347-603 (n = 25 000 there): 1e9 central mass, a Lorenz-attractor trace of light bodies, sorted by
 * radius, near-circular speeds; bit-identical to the compiled reference (tests/golden/default_ics.json). */
int nb_default_ics(nb_body *out, size_t n);

/* ---- the symmetric kernel's work plan ------------------------------------------ */
/* One work item (= one workgroup of force_sym_*): tile `tile` (nb_sym_info.tile_particles particles) against the 64-particle
 * chunks [c0, c0 + cnt).  s_row: row of the stationary slab it writes; the travelling partial of particle
 * j goes to element r_base + j of the travelling slab (diag items write none); group: 0 = local (pairs
 * inside the rank's own block), 1 = cross-block, 2 = late (held-back local). */
typedef struct nb_sym_item {
    uint32_t tile, c0, cnt, s_row;
    int64_t  r_base;
    uint32_t diag, group;
} nb_sym_item;

/* Figures of a plan.  Everything that must agree between the ranks of a sharded run (they split one set of
 * pairs between them) is here, so a host can verify the agreement before the first step. */
typedef struct nb_sym_info {
    uint32_t struct_size;       /* = sizeof(nb_sym_info), set by the caller */
    int32_t  enabled;           /* 1 = the handle runs the symmetric kernel */
    uint32_t chunks_per_item;   /* L */
    uint32_t items, items_local, items_cross, items_late;
    uint32_t tiles, rows_s, segments, cus;
    uint64_t units_local, units_cross, units_late;   /* (tile, chunk) units of each group */
    uint64_t cross_units_total; /* cross-block units of ALL ranks: equal on every rank of a run */
    uint64_t slab_s_bytes, slab_r_bytes;             /* the two partial-sum slab sets (written once, read once per step) */
    uint64_t coverage_entries;
    uint32_t tile_particles;    /* stationary particles per tile of this plan: 2048 (classic) or 512 (wave-split kernels) */
    uint32_t _reserved0;
} nb_sym_info;
int nb_sym_plan_info(const nb_sim *s, nb_sym_info *out);

/* Number of visible HIP devices (0 if none / runtime unavailable). */
int nb_device_count(void);

/* Text of the last error on this thread ("" if none) and its NB_E* code (NB_OK if none). */
const char *nb_last_error(void);
int nb_last_error_code(void);

/* NB_ABI_VERSION the library was built with. */
int nb_abi_version(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* NBODY_H */
