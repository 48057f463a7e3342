// nb_tree_host.hip.h — Barnes-Hut force (NB_FORCE_TREE): the host side of nb_tree.hip.h.  Part of nb_capi.hip's translation unit.
#pragma once
#include "nb_sim.hip.h"

// Node capacity: 16 n + 4096.  Measured (DESIGN.md "Barnes-Hut force"): the reference's default bodies need 2.8 n nodes, Plummer
// spheres of 1 048 576 and 8 388 608 bodies 2.9 n; a pair of bodies much closer than its neighbours adds four nodes per level it
// takes to part them (the 256 isolated touching pairs of tests/golden/collide_isolated_ic.npy: 10.2 n).
static int tree_alloc(nb_sim *s)
{
    const size_t n = s->n;
    s->bh.cap = std::min<uint64_t>(16 * (uint64_t)n + 4096, 0xfffffff0u);
    for (auto &q : s->bh.k64) HIPCHK(s->pool.alloc(q, n));
    for (auto &q : s->bh.v32) HIPCHK(s->pool.alloc(q, n));
    HIPCHK(s->pool.alloc(s->bh.head, n + 1));
    HIPCHK(s->pool.alloc(s->bh.uidx, n + 1));
    HIPCHK(s->pool.alloc(s->bh.uhi, n));
    HIPCHK(s->pool.alloc(s->bh.ulo, n));
    HIPCHK(s->pool.alloc(s->bh.ufirst, n));
    HIPCHK(s->pool.alloc(s->bh.cnt, n + 2));
    HIPCHK(s->pool.alloc(s->bh.base, n + 2));
    HIPCHK(s->pool.alloc(s->bh.part, TREE_BOUNDS_BLOCKS));
    HIPCHK(s->pool.alloc(s->bh.root_dev, 1));
    HIPCHK(s->pool.alloc(s->bh.nd, s->bh.cap));
    HIPCHK(s->pool.alloc(s->bh.nx, s->bh.cap));
    HIPCHK(s->pool.alloc(s->bh.dp, s->bh.cap));
    if (s->bh.quad) {     // +16 B per node (+256 B per body); zeroed once: the build writes every record a walk can read
        HIPCHK(s->pool.alloc(s->bh.qm, s->bh.cap));
        HIPCHK(hipMemsetAsync(s->bh.qm, 0, s->bh.cap * sizeof(float4), s->stream));
    }
    if (s->bh.energy) HIPCHK(s->pool.alloc(s->bh.lo, s->bh.cap));   // +4 B per node; written per build
    size_t sort_bytes = 0, scan_bytes = 0;
    HIPCHK(nb_tree_sort_pairs(nullptr, sort_bytes, s->bh.k64[0], s->bh.k64[2], s->bh.v32[0], s->bh.v32[1], n, s->stream));
    HIPCHK(nb_tree_scan(nullptr, scan_bytes, s->bh.cnt, s->bh.base, n + 2, s->stream));
    s->bh.tmp_bytes = std::max<size_t>(std::max(sort_bytes, scan_bytes), 256);
    HIPCHK(s->pool.alloc(s->bh.tmp, s->bh.tmp_bytes));
    HIPCHK(s->pool.alloc(s->bh.stats, 1));
    HIPCHK(s->pool.alloc_pinned(s->bh.host, 1));
    HIPCHK(hipMemsetAsync(s->bh.stats, 0, sizeof(TreeStats), s->stream));
    memset(s->bh.host, 0, sizeof(TreeStats));
    return NB_OK;
}

// The walk of a NB_FLAG_TREE_LEAVES handle: the wave-uniform one with the hardware rsqrt, the per-lane one (the form the CPU
// model restates bit for bit) with the Quake rsqrt.
static bool tree_walk_is_group(const nb_sim *s) { return s->bh.leaves && s->p.rsqrt_mode != NB_RSQRT_QUAKE; }

// NB_FLAG_TREE_RELATIVE with alpha != 0.  alpha = 0 switches the test off: the handle then runs the launches of the handle without
// the flag, and so produces its bits.
static bool tree_rel_active(const nb_sim *s) { return s->bh.rel && s->bh.alpha != 0.0f; }

// The tree of pos[cur] (nb_tree.hip.h has the pipeline): bounds ... tree_com.  A force evaluation and, on a NB_FLAG_TREE_ENERGY
// handle, nb_energy start with it.
static int launch_tree_build(nb_sim *s)
{
    const uint32_t n = (uint32_t)s->n, g = (n + 255u) / 256u, g2 = (n + 2u + 255u) / 256u;
    const float2 *pos = (const float2 *)s->pos[s->cur];
    const float *mass = (const float *)s->mass;
    uint64_t *khi = s->bh.k64[0], *klo = s->bh.k64[1], *ka = s->bh.k64[2], *kb = s->bh.k64[3];
    uint32_t *v0 = s->bh.v32[0], *v1 = s->bh.v32[1], *v2 = s->bh.v32[2];
    TreeStats *st = s->bh.stats;
    size_t tmp = s->bh.tmp_bytes;
    tree_bounds<<<std::min(g, TREE_BOUNDS_BLOCKS), 256, 0, s->stream>>>(pos, n, s->bh.part);
    tree_root<<<1, 256, 0, s->stream>>>(s->bh.part, std::min(g, TREE_BOUNDS_BLOCKS), s->bh.root_dev, st);
    tree_keys<<<g, 256, 0, s->stream>>>(pos, mass, n, s->bh.root_dev, khi, klo, v0, st);
    HIPCHK(hipGetLastError());
    HIPCHK(nb_tree_sort_pairs(s->bh.tmp, tmp, klo, ka, v0, v1, n, s->stream));          // by the low word ...
    tree_gather_hi<<<g, 256, 0, s->stream>>>(khi, v1, n, kb);
    HIPCHK(nb_tree_sort_pairs(s->bh.tmp, tmp, kb, ka, v1, v2, n, s->stream));           // ... then, stable, by the high one
    tree_heads<<<g2, 256, 0, s->stream>>>(ka, klo, v2, pos, n, s->bh.head, st, s->frame);
    HIPCHK(hipGetLastError());
    HIPCHK(nb_tree_scan(s->bh.tmp, tmp, s->bh.head, s->bh.uidx, (size_t)n + 1, s->stream));
    tree_points<<<g2, 256, 0, s->stream>>>(ka, klo, v2, s->bh.head, s->bh.uidx, n, s->bh.uhi, s->bh.ulo, s->bh.ufirst, st);
    tree_count<<<g2, 256, 0, s->stream>>>(s->bh.uhi, s->bh.ulo, n, s->bh.cnt, st);
    HIPCHK(hipGetLastError());
    HIPCHK(nb_tree_scan(s->bh.tmp, tmp, s->bh.cnt, s->bh.base, (size_t)n + 2, s->stream));
    tree_emit<<<g2, 256, 0, s->stream>>>(s->bh.uhi, s->bh.ulo, s->bh.ufirst, v2, pos, mass, s->bh.base, n, s->bh.root_dev, s->bh.cap,
                                         s->bh.nd, s->bh.nx, s->bh.dp, st, s->frame);
    const uint32_t gc = (uint32_t)std::min<uint64_t>((s->bh.cap + 255u) / 256u, 8u * (uint32_t)s->cus);
    with_flags([&](auto quad) {
        for (int level = TREE_DEPTH_CAP - 1; level >= 0; --level)
            tree_com<quad><<<gc, 256, 0, s->stream>>>(s->bh.nd, s->bh.nx, s->bh.dp, (uint32_t)level, st, s->bh.qm);
    }, s->bh.quad);
    HIPCHK(hipGetLastError());
    return NB_OK;
}

// One force evaluation at pos[cur] into acc[]: the build, then the walk.  The walk is "the force kernel" of nb_profile_read.
static int launch_tree_force(nb_sim *s)
{
    { const int rc = launch_tree_build(s); if (rc) return rc; }
    const uint32_t n = (uint32_t)s->n, g = (n + 255u) / 256u;
    const float2 *pos = (const float2 *)s->pos[s->cur];
    uint32_t *v2 = s->bh.v32[2];
    TreeStats *st = s->bh.stats;
    std::pair<hipEvent_t, hipEvent_t> pr;
    if (s->prof && prof_begin(s, &pr, nullptr)) return NB_EHIP;
    const float eps2 = s->p.eps * s->p.eps, alpha = s->bh.alpha;
    const float4 *qm = s->bh.qm;
    const bool quake = s->p.rsqrt_mode == NB_RSQRT_QUAKE;
    auto lanes = [&](auto kernel) {         // a per-lane walk
        kernel<<<g, 256, 0, s->stream>>>(s->bh.nd, s->bh.nx, v2, pos, n, eps2, s->bh.theta2, (float2 *)s->acc, st, qm, alpha);
    };
    auto windows = [&](auto kernel) {       // tree_walk_group and tree_walk_alone: the same with the three arrays of tree_lane_alone
        kernel<<<g, 256, 0, s->stream>>>(s->bh.nd, s->bh.nx, v2, pos, n, eps2, s->bh.theta2, (float2 *)s->acc, st,
                                         s->bh.head, s->bh.uidx, s->bh.ufirst, qm, alpha);
    };
    if (tree_walk_is_group(s)) {            // the group walk, then the few lanes that left it (nb_tree.hip.h): one "force kernel" interval
        with_flags([&](auto quad, auto rel) {
            windows(tree_walk_group<quad, rel>);
            windows(tree_walk_alone<quad, rel>);
        }, s->bh.quad, tree_rel_active(s));
    } else if (s->bh.leaves) {            // per lane (the Quake rsqrt: tree_walk_is_group): QUAD and REL exist with RSQ_QUAKE only
        with_flags([&](auto q, auto quad, auto rel) {
            if constexpr (q || !(quad || rel)) lanes(tree_walk<q ? RSQ_QUAKE : RSQ_EXACT, true, quad, rel>);
        }, quake, s->bh.quad, tree_rel_active(s));
    } else {                                // the reference's walk
        with_flags([&](auto q) { lanes(tree_walk<q ? RSQ_QUAKE : RSQ_EXACT, false, false, false>); }, quake);
    }
    HIPCHK(hipGetLastError());
    if (s->prof && prof_end(s, pr, nullptr, 1)) return NB_EHIP;
    return NB_OK;
}

// nb_energy of a NB_FLAG_TREE_ENERGY handle: the tree of the current positions, the float64 mass residuals of its leaves, then the
// potential walk (nb_tree.hip.h): the
// windows into partials [0, g) (K) and [g, 2g) (U), the lanes that left them into [2g, 3g) and [3g, 4g).  Touches neither acc[]
// nor the state; the tree arrays are this build's afterwards.
// With `phi` (nb_potentials: n doubles by body index) the same build and walk, EMIT: every walker, the massless ones included, stores
// its phi there and nothing is reduced; the two walk kernels are then bracketed like a force launch for nb_profile_read.
static int launch_tree_potential(nb_sim *s, double *phi = nullptr)
{
    { const int rc = launch_tree_build(s); if (rc) return rc; }
    const uint32_t n = (uint32_t)s->n, g = (n + 255u) / 256u;
    const float2 *pos = (const float2 *)s->pos[s->cur], *vel = (const float2 *)s->vel;
    const float *mass = (const float *)s->mass;
    const uint32_t *v2 = s->bh.v32[2];
    const TreeStats *st = s->bh.stats;
    const double eps2 = (double)s->p.eps * (double)s->p.eps;
    double *e = s->ered_dev;
    const float4 *qm = s->bh.qm;
    const float *lo = s->bh.lo;
    tree_leaf_residual<<<g, 256, 0, s->stream>>>(s->bh.nd, s->bh.base, s->bh.ufirst, v2, mass, n, st, s->bh.lo);
    const float2 *aprev = (const float2 *)s->acc;           // REL: the predicate of a force evaluation issued now: acc[] of this moment, read only
    if (phi) {
        std::pair<hipEvent_t, hipEvent_t> pr;
        if (s->prof && prof_begin(s, &pr, nullptr)) return NB_EHIP;
        with_flags([&](auto quad, auto rel) {
            tree_potential_group<quad, rel, true><<<g, 256, 0, s->stream>>>(s->bh.nd, s->bh.nx, v2, pos, vel, mass, n, eps2, s->bh.theta2, st,
                                                                            s->bh.head, s->bh.uidx, s->bh.ufirst, (double *)nullptr, phi, lo, qm, aprev, s->bh.alpha);
            tree_potential_alone<quad, rel, true><<<g, 256, 0, s->stream>>>(s->bh.nd, s->bh.nx, v2, pos, vel, mass, n, eps2, s->bh.theta2, st,
                                                                            s->bh.head, s->bh.uidx, s->bh.ufirst, (double *)nullptr, phi, lo, qm, aprev, s->bh.alpha);
        }, s->bh.quad, tree_rel_active(s));
        HIPCHK(hipGetLastError());
        if (s->prof && prof_end(s, pr, nullptr, 1)) return NB_EHIP;
        return NB_OK;
    }
    with_flags([&](auto quad, auto rel) {
        tree_potential_group<quad, rel><<<g, 256, 0, s->stream>>>(s->bh.nd, s->bh.nx, v2, pos, vel, mass, n, eps2, s->bh.theta2, st,
                                                                  s->bh.head, s->bh.uidx, s->bh.ufirst, e, e + g, lo, qm, aprev, s->bh.alpha);
        tree_potential_alone<quad, rel><<<g, 256, 0, s->stream>>>(s->bh.nd, s->bh.nx, v2, pos, vel, mass, n, eps2, s->bh.theta2, st,
                                                                  s->bh.head, s->bh.uidx, s->bh.ufirst, e + 2 * (size_t)g,
                                                                  e + 3 * (size_t)g, lo, qm, aprev, s->bh.alpha);
    }, s->bh.quad, tree_rel_active(s));
    HIPCHK(hipGetLastError());
    return NB_OK;
}

// acc[] of the tree walk -> kick, drift (or acc only): the reference-order form with the Quake rsqrt, the fused one otherwise
static int launch_tree_integrate(nb_sim *s, double dt_kick, double dt_drift, int flags)
{
    const uint32_t n = (uint32_t)s->n, g = (n + 255u) / 256u;
    using L2 = Layout<float, false>;
    with_flags([&](auto strict) {
        tree_integrate<L2, strict><<<g, 256, 0, s->stream>>>((const float2 *)s->pos[s->cur], (float2 *)s->pos[s->cur ^ 1], (float2 *)s->vel,
                                                              (float2 *)s->acc, n, (float)dt_kick, (float)dt_drift, s->p.extras, flags, s->bh.stats);
    }, s->p.rsqrt_mode == NB_RSQRT_QUAKE);
    HIPCHK(hipGetLastError());
    return NB_OK;
}

// A failed build (node capacity, depth cap) is reported ONCE, by the first synchronising call after it, like a collision overflow.
static int tree_check(nb_sim *s)
{
    if (!s->tree) return NB_OK;
    HIPCHK(hipMemcpyAsync(s->bh.host, s->bh.stats, sizeof(TreeStats), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    const TreeStats &t = *s->bh.host;
    if (t.overflow_steps <= s->bh.ovf_reported) return NB_OK;
    const unsigned long long steps = (unsigned long long)(t.overflow_steps - s->bh.ovf_reported);
    s->bh.ovf_reported = t.overflow_steps;
    if (t.overflow_kind == 1)
        return nb_fail(NB_ENOMEM, "tree: the force evaluation at frame %llu needed %llu nodes, more than the capacity of %llu; nothing was "
                                  "integrated (%llu evaluation(s) failed since the last report)",
                       (unsigned long long)t.overflow_frame, (unsigned long long)t.overflow_needed, (unsigned long long)s->bh.cap, steps);
    return nb_fail(NB_ENOMEM, "tree: at frame %llu two different positions (sorted position %llu) are not separated within %d levels; nothing "
                              "was integrated (%llu evaluation(s) failed since the last report)",
                   (unsigned long long)t.overflow_frame, (unsigned long long)t.overflow_needed, TREE_DEPTH_CAP, steps);
}

extern "C" int nb_tree_stats(nb_sim *s, uint64_t *nodes, uint32_t *max_depth, uint64_t *overflow_steps)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_tree_stats: NULL handle");
    if (!s->tree) return nb_fail(NB_ESTATE, "nb_tree_stats: the handle was created with NB_FORCE_DIRECT");
    if (bind(s)) return NB_EHIP;
    const int rc = tree_check(s);
    if (rc && nb_last_error_code() != NB_ENOMEM) return rc;
    if (nodes) *nodes = s->bh.host->nodes;
    if (max_depth) *max_depth = s->bh.host->max_depth;
    if (overflow_steps) *overflow_steps = s->bh.host->overflow_steps;
    return rc;
}

// Scratch of nb_tree_nodes for `total` nodes: 144 B per node on the device (record 128, flag 4, rank 8, index 4) plus the scan's
// temporary storage, asked from nb_tree_scan for THIS element count (bh.tmp was sized for n + 2 elements).  Growth only, with an
// eighth of slack so that a tree that grows a little every frame does not reallocate every frame; never above the node capacity.
static int tree_export_alloc(nb_sim *s, uint64_t total)
{
    nb_sim::BarnesHut::Export &x = s->bh.exp;
    if (total <= x.cap && x.tmp) return NB_OK;                    // (no tmp: an earlier attempt ran out of memory at its last request)
    HIPCHK(hipStreamSynchronize(s->stream));
    s->pool.release(x.tmp);
    const uint64_t want = std::max<uint64_t>(total, std::min<uint64_t>(total + total / 8 + 1024, s->bh.cap));
    HIPCHK(s->pool.regrow(x.cap, (size_t)want, x.rec, x.flag, x.rank, x.idx));
    size_t bytes = 0;
    HIPCHK(nb_tree_scan(nullptr, bytes, x.flag, x.rank, (size_t)x.cap, s->stream));
    x.tmp_bytes = std::max<size_t>(bytes, 256);
    HIPCHK(s->pool.alloc(x.tmp, x.tmp_bytes));
    return NB_OK;
}

// The reference's `quadtree.nodes` (main.cpp:626, drawQuadtreeNode main.cpp:394-475) for the tree of the last build.
extern "C" int nb_tree_nodes(nb_sim *s, nb_tree_node *out, size_t capacity, size_t *count)
{
    if (!s || !count) return nb_fail(NB_EINVAL, "nb_tree_nodes: NULL %s", !s ? "handle" : "count");
    if (!s->tree) return nb_fail(NB_ESTATE, "nb_tree_nodes: the handle was created with NB_FORCE_DIRECT");
    { const int rc = query_enter(s, "nb_tree_nodes"); if (rc) return rc; }
    const TreeStats &t = *s->bh.host;
    if (t.fail)
        return nb_fail(NB_ESTATE, "nb_tree_nodes: no tree to export: the last build failed (%s)", t.fail == 1 ? "node capacity" : "depth cap");
    const uint64_t total = t.nodes;                               // 0 before any build; <= bh.cap < 2^32 after a good one
    if (total > s->bh.cap) return nb_fail(NB_ESTATE, "internal: nb_tree_nodes: %llu nodes in a capacity of %llu", (unsigned long long)total, (unsigned long long)s->bh.cap);
    *count = (size_t)total;
    if (!out || total == 0) return NB_OK;
    if (capacity < total)
        return nb_fail(NB_EINVAL, "nb_tree_nodes: the tree has %llu nodes, out holds %zu", (unsigned long long)total, capacity);
    { const int rc = tree_export_alloc(s, total); if (rc) return rc; }
    const size_t bytes = (size_t)total * sizeof(nb_tree_node);
    // staging for the whole scratch, slack included: it regrows when the scratch does, not with every tree that is a little larger
    { const int rc = query_stage(s, stage_need(out, bytes) ? (size_t)s->bh.exp.cap * sizeof(nb_tree_node) : 0); if (rc) return rc; }
    const uint32_t tot = (uint32_t)total;
    const uint32_t g = (uint32_t)std::min<uint64_t>((total + 255u) / 256u, 8u * (uint32_t)s->cus);
    std::pair<hipEvent_t, hipEvent_t> pr;                         // with nb_profile_enable the export kernels count as one launch
    if (s->prof && prof_begin(s, &pr, nullptr)) return NB_EHIP;
    tree_export_flags<<<g, 256, 0, s->stream>>>(s->bh.dp, tot, s->bh.exp.flag);
    HIPCHK(hipGetLastError());
    size_t tmp = s->bh.exp.tmp_bytes;
    HIPCHK(nb_tree_scan(s->bh.exp.tmp, tmp, s->bh.exp.flag, s->bh.exp.rank, (size_t)total, s->stream));
    tree_export_root<<<1, 64, 0, s->stream>>>(s->bh.nd, s->bh.dp, s->bh.root_dev, tot, (uint4 *)s->bh.exp.rec, s->bh.exp.idx);
    for (uint32_t level = 0; level < t.max_depth && level < (uint32_t)TREE_DEPTH_CAP; ++level)
        tree_export_level<<<g, 256, 0, s->stream>>>(s->bh.nd, s->bh.nx, s->bh.dp, s->bh.exp.rank, level, tot,
                                                    (uint4 *)s->bh.exp.rec, s->bh.exp.idx);
    HIPCHK(hipGetLastError());
    if (s->prof && prof_end(s, pr, nullptr, 1)) return NB_EHIP;
    return copy_plane(s, out, s->bh.exp.rec, bytes);
}

// alpha travels to the walks as a kernel argument: the evaluations enqueued so far keep theirs, the next one takes the new value
extern "C" int nb_tree_alpha(nb_sim *s, float alpha)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_tree_alpha: NULL handle");
    if (!s->bh.rel) return nb_fail(NB_ESTATE, "nb_tree_alpha: the handle was created without NB_FLAG_TREE_RELATIVE");
    if (!(alpha >= 0.0f) || std::isinf(alpha)) return nb_fail(NB_EINVAL, "nb_tree_alpha: alpha must be finite and >= 0 (got %g)", (double)alpha);
    if (s->in_step) return nb_fail(NB_ESTATE, "nb_tree_alpha: a split step is in flight");
    s->bh.alpha = alpha;
    return NB_OK;
}
