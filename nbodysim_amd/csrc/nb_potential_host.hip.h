// nb_potential_host.hip.h — host side of nb_potentials (kernels: nb_potential.hip.h; the walk of a NB_FLAG_TREE_ENERGY handle:
// tree_potential_* <.., EMIT>, nb_tree.hip.h).  Included by nb_capi.hip beside the tree and raster hosts; it opens with query_enter like
// the other query calls, but moves its result with copy_d2h through the staging buffer of nb_sync, hence the snapshot wait.
#pragma once

static int ensure_staging(nb_sim *s);     // nb_capi.hip, below: the page-locked i_count x 64 B of nb_sync / nb_sync_positions

// The direct sweep into s->phi_dev.  Particles per lane: the largest P that still gives four workgroups per CU (P moves a
// particle to another lane and changes no operation of its sum: nb_potential.hip.h), so small and sharded handles fill the chip
// with P = 1 and large ones read each j-record for eight particles.  nb_params.lanes_p forces P, as in the force launch.
static int launch_potential_sweep(nb_sim *s)
{
    const uint32_t n = (uint32_t)s->n, ib = (uint32_t)s->i_begin, ic = (uint32_t)s->i_count;
    std::pair<hipEvent_t, hipEvent_t> pr;                         // with nb_profile_enable the sweep counts as one launch
    if (s->prof && prof_begin(s, &pr, nullptr)) return NB_EHIP;
    with_layout(s, [&](auto L) {
        using LT = decltype(L);
        using real = typename LT::real;
        using vec = typename LT::vec;
        const vec *pos = (const vec *)s->pos[s->cur];
        const real eps2 = (real)s->p.eps * (real)s->p.eps;        // as the force launch squares it
        if constexpr (std::is_same_v<real, double>) {
            potential_f64<LT><<<(ic + BLOCK - 1) / BLOCK, BLOCK, 0, s->stream>>>(pos, (const double *)s->mass, s->phi_dev, n, ib, ic, eps2);
        } else {
            constexpr uint32_t per = (BLOCK / TILED_F32_WS) * 2;  // particles per workgroup per P
            const uint32_t want = 4u * (uint32_t)s->cus;
            const int P = s->p.lanes_p > 0 ? s->p.lanes_p : ic / (per * 4) >= want ? 4 : ic / (per * 2) >= want ? 2 : 1;
            with_lanes<4>(P, [&](auto p) {
                potential_tiled_f32<LT, p><<<(ic + per * p - 1) / (per * p), BLOCK, 0, s->stream>>>(pos, (const float *)s->mass, s->phi_dev,
                                                                                                 n, ib, ic, eps2);
            });
        }
    });
    HIPCHK(hipGetLastError());
    if (s->prof && prof_end(s, pr, nullptr, 1)) return NB_EHIP;
    return NB_OK;
}

// The binding energy of a body is v^2 / 2 + phi: the per-body counterpart of nb_energy (include/nbody.h has the contract).
extern "C" int nb_potentials(nb_sim *s, double *phi)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_potentials: NULL handle");
    if (!phi) return nb_fail(NB_EINVAL, "nb_potentials: NULL phi");
    { const int rc = query_enter(s, "nb_potentials", true); if (rc) return rc; }   // (the staging buffer may still feed a pipelined snapshot)
    const size_t bytes = s->i_count * sizeof(double);
    if (stage_need(phi, bytes) && ensure_staging(s)) return NB_EHIP;
    if (!s->phi_dev) HIPCHK(s->pool.alloc(s->phi_dev, s->i_count));
    if (s->bh.energy) {       // the build and the potential walk of nb_energy; a failed build is reported by THIS call, phi untouched
        { const int rc = launch_tree_potential(s, s->phi_dev); if (rc) return rc; }
        { const int rc = tree_check(s); if (rc) return rc; }
    } else {
        const int rc = launch_potential_sweep(s);
        if (rc) return rc;
    }
    return copy_d2h(s, phi, s->phi_dev, bytes, s->stream, s->staging);
}
