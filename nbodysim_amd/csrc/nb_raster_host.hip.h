// nb_raster_host.hip.h — host side of nb_raster (kernels: nb_raster.hip.h).  Included by nb_capi.hip beside the tree and collide
// hosts; it opens with query_enter and moves its planes with copy_plane through the query staging buffer, like nb_tree_nodes.
#pragma once

#ifdef NB_RASTER_PLAIN                         // A/B builds (tools/raster_bench.py): one global add per body, no combining
constexpr bool RASTER_COMBINE = false;
#else
constexpr bool RASTER_COMBINE = true;
#endif

// Scratch for a view of `pixels`: 4 B per pixel for the counts, 8 + 4 B for the unit sums and the float plane once a mass plane is
// asked for.  Growth only.
static int raster_alloc(nb_sim *s, uint64_t pixels, bool want_count, bool want_mass)
{
    nb_sim::Raster &r = s->ras;
    const bool grow_c = want_count && r.cap < pixels, grow_m = want_mass && r.mass_cap < pixels;
    if (!grow_c && !grow_m) return NB_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    if (grow_c) HIPCHK(s->pool.regrow(r.cap, (size_t)pixels, r.cnt));
    if (grow_m) HIPCHK(s->pool.regrow(r.mass_cap, (size_t)pixels, r.units, r.massf));
    return NB_OK;
}

// The viewer's frame whose size is the screen's: replaces the per-body draw loop of main.cpp:745-835 (worldToScreen / isInScreenBounds,
// :196-213) and the copy of all bodies that feeds it.
extern "C" int nb_raster(nb_sim *s, const nb_view *view, uint32_t *count, float *mass)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_raster: NULL handle");
    if (!view) return nb_fail(NB_EINVAL, "nb_raster: NULL view");
    if (!count && !mass) return nb_fail(NB_EINVAL, "nb_raster: count and mass are both NULL");
    if (view->struct_size != sizeof(nb_view))
        return nb_fail(NB_EINVAL, "nb_raster: view->struct_size is %u, sizeof(nb_view) is %zu", view->struct_size, sizeof(nb_view));
    if (view->width < 1 || view->width > 16384) return nb_fail(NB_EINVAL, "nb_raster: view->width must be 1 .. 16384 (got %u)", view->width);
    if (view->height < 1 || view->height > 16384) return nb_fail(NB_EINVAL, "nb_raster: view->height must be 1 .. 16384 (got %u)", view->height);
    const uint64_t pixels = (uint64_t)view->width * view->height;
    if (pixels > ((uint64_t)1 << 24))
        return nb_fail(NB_EINVAL, "nb_raster: view->width * view->height must be <= 2^24 (got %u x %u)", view->width, view->height);
    if (!std::isfinite(view->scale) || !(view->scale > 0.0f))
        return nb_fail(NB_EINVAL, "nb_raster: view->scale must be finite and > 0 (got %g)", (double)view->scale);
    if (!std::isfinite(view->center_x)) return nb_fail(NB_EINVAL, "nb_raster: view->center_x must be finite (got %g)", (double)view->center_x);
    if (!std::isfinite(view->center_y)) return nb_fail(NB_EINVAL, "nb_raster: view->center_y must be finite (got %g)", (double)view->center_y);
    if (view->_reserved0 != 0) return nb_fail(NB_EINVAL, "nb_raster: view->_reserved0 must be 0 (got %u)", view->_reserved0);
    if (mass && (!std::isfinite(view->mass_quantum) || !(view->mass_quantum > 0.0f)))
        return nb_fail(NB_EINVAL, "nb_raster: view->mass_quantum must be finite and > 0 for a mass plane (got %g)", (double)view->mass_quantum);
    // no snapshot wait (nb_sync_positions has one for its staging): a pending snapshot reads aos_dev and never writes pos, and the
    // query calls have scratch and staging of their own
    { const int rc = query_enter(s, "nb_raster"); if (rc) return rc; }
    const size_t bytes = (size_t)pixels * sizeof(uint32_t);       // of either plane
    { const int rc = raster_alloc(s, pixels, count != nullptr, mass != nullptr); if (rc) return rc; }
    { const int rc = query_stage(s, std::max(stage_need(count, bytes), stage_need(mass, bytes))); if (rc) return rc; }
    nb_sim::Raster &r = s->ras;
    if (count) HIPCHK(hipMemsetAsync(r.cnt, 0, bytes, s->stream));
    if (mass) HIPCHK(hipMemsetAsync(r.units, 0, (size_t)pixels * sizeof(unsigned long long), s->stream));
    const uint32_t ic = (uint32_t)s->i_count, batches = (ic + BLOCK - 1) / BLOCK;
    // workgroups that stay: a table per workgroup pays when it sees many bodies; enough of them to fill the chip several times over
    const uint32_t g = RASTER_COMBINE ? std::max(1u, std::min(batches, 16u * (uint32_t)s->cus)) : std::max(1u, batches);
    const RasterView v{view->width, view->height, view->center_x, view->center_y, view->scale, mass ? view->mass_quantum : 1.0f};
    std::pair<hipEvent_t, hipEvent_t> pr;                         // with nb_profile_enable the bin pass counts as one launch
    if (s->prof && prof_begin(s, &pr, nullptr)) return NB_EHIP;
    with_layout(s, [&](auto L) {
        using LT = decltype(L);
        using real = typename LT::real;
        using vec = typename LT::vec;
        const vec *pos = (const vec *)s->pos[s->cur];
        const uint32_t ib = (uint32_t)s->i_begin;
        if (count && mass)
            raster_bin<LT, true, true, RASTER_COMBINE><<<g, BLOCK, 0, s->stream>>>(pos, (const real *)s->mass, ib, ic, v, r.cnt, r.units);
        else if (count)
            raster_bin<LT, true, false, RASTER_COMBINE><<<g, BLOCK, 0, s->stream>>>(pos, (const real *)s->mass, ib, ic, v, r.cnt, nullptr);
        else
            raster_bin<LT, false, true, RASTER_COMBINE><<<g, BLOCK, 0, s->stream>>>(pos, (const real *)s->mass, ib, ic, v, nullptr, r.units);
    });
    HIPCHK(hipGetLastError());
    if (s->prof && prof_end(s, pr, nullptr, 1)) return NB_EHIP;
    if (mass) {
        raster_finish<<<(uint32_t)((pixels + BLOCK - 1) / BLOCK), BLOCK, 0, s->stream>>>(r.units, r.massf, (uint32_t)pixels, view->mass_quantum);
        HIPCHK(hipGetLastError());
    }
    if (count) {
        const int rc = copy_plane(s, count, r.cnt, bytes);
        if (rc) return rc;
    }
    return mass ? copy_plane(s, mass, r.massf, bytes) : NB_OK;
}
