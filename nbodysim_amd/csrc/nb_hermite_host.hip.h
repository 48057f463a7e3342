// nb_hermite_host.hip.h — host side of NB_INTEGRATOR_HERMITE4 (kernels: nb_hermite.hip.h): the launch of the acc+jerk sweep, one
// step of the predictor-corrector, and nb_jerks.  Included by nb_capi.hip behind the field's host.  nb_jerks opens with query_enter and
// moves its planes with copy_plane through the query staging buffer, like nb_field.
#pragma once

static bool hermite(const nb_sim *s) { return s->p.integrator == NB_INTEGRATOR_HERMITE4; }

// What a Hermite handle holds beyond a one-sided handle: the jerk array and the predicted velocities (one vec per body each), and
// the evaluation's rows (2 dims doubles per body).  The jerk array is cleared: the first corrector pass reads its records whole.
static int hermite_alloc(nb_sim *s)
{
    const size_t D = s->dims3 ? 3 : 2;
    HIPCHK(s->pool.alloc(s->herm.jerk, s->n * s->esz));
    HIPCHK(s->pool.alloc(s->herm.vpred, s->n * s->esz));
    HIPCHK(s->pool.alloc(s->herm.rows, 2 * D * s->n));
    HIPCHK(hipMemsetAsync(s->herm.jerk, 0, s->n * s->esz, s->stream));
    return NB_OK;
}

// The acc+jerk sweep at (pos, vel) into the rows: ONE launch, counted as one force launch with nb_profile_enable.  Bodies per lane on
// an fp32 handle: launch_field_sweep's rule on n (P moves a body to another lane and changes no operation of its sums), at most 2 in
// 3-D; nb_params.lanes_p forces P.  fp64: two bodies per thread where that still fills the chip.  A handle whose eps^2 is 0 in the
// arithmetic of the sweep runs the guarded variant.
static int launch_force_jerk(nb_sim *s, const void *pos_v, const void *vel_v)
{
    const uint32_t n = (uint32_t)s->n;
    const size_t D = s->dims3 ? 3 : 2;
    double *arow = s->herm.rows, *jrow = arow + D * s->n;
    std::pair<hipEvent_t, hipEvent_t> pr;
    if (s->prof && prof_begin(s, &pr)) return NB_EHIP;
    with_layout(s, [&](auto L) {
        using LT = decltype(L);
        using real = typename LT::real;
        using vec = typename LT::vec;
        const vec *pos = (const vec *)pos_v, *vel = (const vec *)vel_v;
        const real eps2 = (real)s->p.eps * (real)s->p.eps;        // as the force launch squares it
        const uint32_t want = 4u * (uint32_t)s->cus;
        with_flags([&](auto guard) {
            if constexpr (std::is_same_v<real, double>) {
                const int P = s->p.lanes_p > 0 ? (s->p.lanes_p > 1 ? 2 : 1) : n / (BLOCK * 2) >= want ? 2 : 1;
                with_lanes<2>(P, [&](auto p) {
                    force_jerk_f64<LT, p, guard><<<(n + BLOCK * p - 1) / (BLOCK * p), BLOCK, 0, s->stream>>>(pos, (const double *)s->mass, vel, arow, jrow, n, eps2);
                });
            } else {
                constexpr uint32_t per = (BLOCK / TILED_F32_WS) * 2;  // bodies per workgroup per P
                constexpr int PMAX = hermite_pmax_f32(LT::dims3);
                int P = s->p.lanes_p > 0 ? s->p.lanes_p : n / (per * 4) >= want ? 4 : n / (per * 2) >= want ? 2 : 1;
                if (P > PMAX) P = PMAX;
                with_lanes<PMAX>(P, [&](auto p) {
                    force_jerk_tiled_f32<LT, p, guard><<<(n + per * p - 1) / (per * p), BLOCK, 0, s->stream>>>(pos, (const float *)s->mass, vel, arow, jrow, n, eps2);
                });
            }
        }, needs_guard(s));
    });
    HIPCHK(hipGetLastError());
    if (s->prof && prof_end(s, pr)) return NB_EHIP;
    return NB_OK;
}

// The rows -> (a1, j1) in the handle's real, and with `advance` the corrector's two formulas; the carried pair and acc[] <- (a1, j1).
static int launch_hermite_correct(nb_sim *s, double h_2, double h2_12, int advance)
{
    const uint32_t n = (uint32_t)s->n, g = (n + BLOCK - 1) / BLOCK;
    const size_t D = s->dims3 ? 3 : 2;
    const double *arow = s->herm.rows, *jrow = arow + D * s->n;
    with_layout(s, [&](auto L) {
        using real = typename decltype(L)::real;
        using vec = typename decltype(L)::vec;
        hermite_correct<decltype(L)><<<g, BLOCK, 0, s->stream>>>((const vec *)s->pos[s->cur], (vec *)s->pos[s->cur ^ 1], (vec *)s->vel, (vec *)s->acc,
                                                                (vec *)s->herm.jerk, arow, jrow, n, (real)h_2, (real)h2_12, advance);
    });
    HIPCHK(hipGetLastError());
    return NB_OK;
}

// One step of size h (include/nbody.h has the scheme).  The coefficients are formed in double from the float h and rounded once to
// the handle's real by the launches.  The carried pair is invalid after nb_create / nb_upload (and after nb_accelerations, which
// rewrites acc[]): the step then first evaluates (a0, j0) at (x, v).
static int step_hermite(nb_sim *s, float h)
{
    const double hd = (double)h;
    const uint32_t n = (uint32_t)s->n, g = (n + BLOCK - 1) / BLOCK;
    int rc;
    if (!s->herm.valid) {
        if ((rc = launch_force_jerk(s, s->pos[s->cur], s->vel)) || (rc = launch_hermite_correct(s, 0.0, 0.0, 0))) return rc;
        s->herm.valid = true;
    }
    with_layout(s, [&](auto L) {
        using real = typename decltype(L)::real;
        using vec = typename decltype(L)::vec;
        hermite_predict<decltype(L)><<<g, BLOCK, 0, s->stream>>>((const vec *)s->pos[s->cur], (vec *)s->pos[s->cur ^ 1], (const vec *)s->vel,
                                                                (vec *)s->herm.vpred, (const vec *)s->acc, (const vec *)s->herm.jerk, n,
                                                                (real)hd, (real)(hd * hd / 2.0), (real)(hd * hd * hd / 6.0));
    });
    HIPCHK(hipGetLastError());
    if ((rc = launch_force_jerk(s, s->pos[s->cur ^ 1], s->herm.vpred))) return rc;
    if ((rc = launch_hermite_correct(s, hd / 2.0, hd * hd / 12.0, 1))) return rc;
    s->cur ^= 1;
    s->frame += 1;
    s->acc_valid = false;
    return NB_OK;
}

// Acceleration and jerk of every body at the handle's CURRENT positions and velocities, by the step's own kernel, as fp64 (include/nbody.h
// has the contract).  The rows are scratch between steps (the corrector has consumed them), so nothing of the handle's state is touched.
extern "C" int nb_jerks(nb_sim *s, double *acc, double *jerk)
{
    const char *name = "nb_jerks";
    if (!s) return nb_fail(NB_EINVAL, "%s: NULL handle", name);
    if (!acc && !jerk) return nb_fail(NB_EINVAL, "%s: acc and jerk are both NULL", name);
    if (!hermite(s)) return nb_fail(NB_EINVAL, "%s: the call is the NB_INTEGRATOR_HERMITE4 integrator's (this handle's integrator is %d)", name, s->p.integrator);
    { const int rc = query_enter(s, name); if (rc) return rc; }
    const size_t D = s->dims3 ? 3 : 2, bytes = s->n * D * sizeof(double);
    { const int rc = query_stage(s, std::max(stage_need(acc, bytes), stage_need(jerk, bytes))); if (rc) return rc; }
    { const int rc = launch_force_jerk(s, s->pos[s->cur], s->vel); if (rc) return rc; }
    if (acc) { const int rc = copy_plane(s, acc, s->herm.rows, bytes); if (rc) return rc; }
    if (jerk) { const int rc = copy_plane(s, jerk, s->herm.rows + D * s->n, bytes); if (rc) return rc; }
    return NB_OK;
}
