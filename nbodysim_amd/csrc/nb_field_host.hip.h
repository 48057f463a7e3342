// nb_field_host.hip.h — host side of nb_field (kernels: nb_field.hip.h; the walk of a NB_FLAG_TREE_ENERGY handle: tree_field_walk,
// nb_tree.hip.h).  Included by nb_capi.hip behind the profiles' host.  It opens with query_enter and moves its planes with copy_plane
// through the query staging buffer, like nb_radial_profiles.
#pragma once

constexpr size_t FIELD_POINTS_MAX = NB_FIELD_POINTS_MAX;

// One block for the largest call seen: 8 B per point for phi, 8 dims for acc, 4 dims for the points.  Growth only.
static int field_alloc(nb_sim *s, size_t npoints)
{
    const size_t D = s->dims3 ? 3 : 2, bytes = npoints * (8 * (D + 1) + 4 * D);
    if (s->fld.bytes >= bytes) return NB_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(s->pool.regrow(s->fld.bytes, bytes, s->fld.buf));
    return NB_OK;
}

// The direct sweep.  Points per lane on an fp32 handle: launch_potential_sweep's rule on npoints (P moves a point to another lane and
// changes no operation of its sums); nb_params.lanes_p forces P.  A handle whose eps^2 is 0 in the arithmetic of the sweep runs the
// guarded variant.
static void launch_field_sweep(nb_sim *s, const float *pts, uint32_t np, double *phi, double *acc)
{
    const uint32_t n = (uint32_t)s->n;
    with_layout(s, [&](auto L) {
        using LT = decltype(L);
        using real = typename LT::real;
        using vec = typename LT::vec;
        const vec *pos = (const vec *)s->pos[s->cur];
        const real eps2 = (real)s->p.eps * (real)s->p.eps;        // as the force launch squares it
        with_flags([&](auto guard, auto ph, auto ac) {
            if constexpr (ph || ac) {
                if constexpr (std::is_same_v<real, double>) {
                    field_f64<LT, guard, ph, ac><<<(np + BLOCK - 1) / BLOCK, BLOCK, 0, s->stream>>>(pos, (const double *)s->mass, pts, phi, acc, n, np, eps2);
                } else {
                    constexpr uint32_t per = (BLOCK / TILED_F32_WS) * 2;  // points per workgroup per P
                    const uint32_t want = 4u * (uint32_t)s->cus;
                    const int P = s->p.lanes_p > 0 ? s->p.lanes_p : np / (per * 4) >= want ? 4 : np / (per * 2) >= want ? 2 : 1;
                    with_lanes<4>(P, [&](auto p) {
                        field_tiled_f32<LT, p, guard, ph, ac><<<(np + per * p - 1) / (per * p), BLOCK, 0, s->stream>>>(pos, (const float *)s->mass, pts,
                                                                                                                    phi, acc, n, np, eps2);
                    });
                }
            }
        }, !(eps2 > (real)0), phi != nullptr, acc != nullptr);
    });
}

// The walk of a NB_FLAG_TREE_ENERGY handle, behind launch_tree_build and the leaf residual: the theta walk with the handle's rsqrt_mode.
static void launch_field_walk(nb_sim *s, const float *pts, uint32_t np, double *phi, double *acc)
{
    const float eps2f = s->p.eps * s->p.eps;
    const double eps2 = (double)s->p.eps * (double)s->p.eps;
    with_flags([&](auto q, auto quad, auto ph, auto ac) {
        if constexpr (ph || ac)
            tree_field_walk<q ? RSQ_QUAKE : RSQ_EXACT, quad, ph, ac><<<(np + 255u) / 256u, 256, 0, s->stream>>>(
                s->bh.nd, s->bh.nx, (const float2 *)pts, np, eps2f, eps2, s->bh.theta2, s->bh.stats, s->bh.lo, s->bh.qm, phi, (double2 *)acc);
    }, s->p.rsqrt_mode == NB_RSQRT_QUAKE, s->bh.quad, phi != nullptr, acc != nullptr);
}

// Potential and acceleration at caller-given points: the field under a raster, beside a radial profile, across a group, on a probe
// (include/nbody.h has the contract).
extern "C" int nb_field(nb_sim *s, const float *points, size_t npoints, double *phi, double *acc)
{
    const char *name = "nb_field";
    if (!s) return nb_fail(NB_EINVAL, "%s: NULL handle", name);
    if (!points) return nb_fail(NB_EINVAL, "%s: NULL points", name);
    if (!phi && !acc) return nb_fail(NB_EINVAL, "%s: phi and acc are both NULL", name);
    if (npoints < 1 || npoints > FIELD_POINTS_MAX)
        return nb_fail(NB_EINVAL, "%s: npoints must be 1 .. %zu (got %zu)", name, FIELD_POINTS_MAX, npoints);
    const size_t D = s->dims3 ? 3 : 2;
    for (size_t t = 0; t < npoints * D; ++t)
        if (!std::isfinite(points[t]))
            return nb_fail(NB_EINVAL, "%s: points[%zu] (point %zu, axis %zu) is not finite (%g)", name, t, t / D, t % D, (double)points[t]);
    { const int rc = query_enter(s, name); if (rc) return rc; }           // no snapshot wait: the planes move through the query staging buffer
    { const int rc = field_alloc(s, npoints); if (rc) return rc; }
    const size_t phi_bytes = npoints * sizeof(double), acc_bytes = npoints * D * sizeof(double);
    { const int rc = query_stage(s, std::max(stage_need(phi, phi_bytes), stage_need(acc, acc_bytes))); if (rc) return rc; }
    double *phi_dev = (double *)s->fld.buf, *acc_dev = phi_dev + npoints;
    float *pts = (float *)(acc_dev + npoints * D);
    { const int rc = copy_h2d(s, pts, points, npoints * D * sizeof(float)); if (rc) return rc; }
    const uint32_t np = (uint32_t)npoints;
    std::pair<hipEvent_t, hipEvent_t> pr;                         // with nb_profile_enable the sweep (the walk kernel) counts as one launch
    if (s->bh.energy) {       // the build of nb_energy; a failed build is reported by THIS call, nothing written
        { const int rc = launch_tree_build(s); if (rc) return rc; }
        tree_leaf_residual<<<((uint32_t)s->n + 255u) / 256u, 256, 0, s->stream>>>(s->bh.nd, s->bh.base, s->bh.ufirst, s->bh.v32[2], (const float *)s->mass,
                                                                                 (uint32_t)s->n, s->bh.stats, s->bh.lo);
        HIPCHK(hipGetLastError());
        if (s->prof && prof_begin(s, &pr, nullptr)) return NB_EHIP;
        launch_field_walk(s, pts, np, phi ? phi_dev : nullptr, acc ? acc_dev : nullptr);
        HIPCHK(hipGetLastError());
        if (s->prof && prof_end(s, pr, nullptr, 1)) return NB_EHIP;
        { const int rc = tree_check(s); if (rc) return rc; }
    } else {
        if (s->prof && prof_begin(s, &pr, nullptr)) return NB_EHIP;
        launch_field_sweep(s, pts, np, phi ? phi_dev : nullptr, acc ? acc_dev : nullptr);
        HIPCHK(hipGetLastError());
        if (s->prof && prof_end(s, pr, nullptr, 1)) return NB_EHIP;
    }
    if (phi) { const int rc = copy_plane(s, phi, phi_dev, phi_bytes); if (rc) return rc; }
    if (acc) { const int rc = copy_plane(s, acc, acc_dev, acc_bytes); if (rc) return rc; }
    return NB_OK;
}
