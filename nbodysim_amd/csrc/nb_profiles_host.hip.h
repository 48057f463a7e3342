// nb_profiles_host.hip.h — host side of nb_radial_profiles (kernels: nb_profiles.hip.h).  Included by nb_capi.hip behind the pair
// counts' host, whose edge rules it shares (pair_counts_edges); the front half is the neighbours' (neighbors_alloc for the per-body
// arrays and the sort's storage, neighbors_cells for the keys, the sort and the gather).  It opens with query_enter and moves its
// records with copy_plane through the query staging buffer, like nb_group_catalog.
#pragma once

constexpr size_t PROFILES_CENTERS_MAX = (size_t)1 << 20, PROFILES_RECORDS_MAX = (size_t)1 << 20;

// Scratch of its own, beside nb_neighbors' 40 B per body and sort storage.  Per centre of the largest call seen, and for one entry
// more: 84 B (the centre 12, its velocity 24, the three ranges 24, the two piece counts and their scans 8 + 16) plus the scan's
// temporary storage; 64 B per record of the largest ncenters x nbins seen; two page-locked words.  Growth only.  The partial rows
// of the split centres are sized in the call, once their number is known.
static int profiles_alloc(nb_sim *s, size_t ncenters, size_t records)
{
    nb_sim::Profiles &f = s->prf;
    const size_t c1 = ncenters + 1;
    if (f.cap >= c1 && f.tmp && f.out_cap >= records && f.host) return NB_OK;   // (no tmp: an earlier attempt ran out of memory at its last request)
    HIPCHK(hipStreamSynchronize(s->stream));
    if (f.cap < c1 || !f.tmp) {
        s->pool.release(f.tmp);
        HIPCHK(s->pool.regrow(f.cap, c1, f.cen, f.vcen, f.rng, f.pieces, f.split, f.first, f.prow));
        size_t bytes = 0;
        HIPCHK(nb_tree_scan(nullptr, bytes, f.pieces, f.first, (size_t)f.cap, s->stream));
        f.tmp_bytes = std::max<size_t>(bytes, 256);
        HIPCHK(s->pool.alloc(f.tmp, f.tmp_bytes));
    }
    HIPCHK(s->pool.regrow(f.out_cap, records, f.out));
    if (!f.host) HIPCHK(s->pool.alloc_pinned(f.host, 2));
    return NB_OK;
}

template <typename LT, int NS>
static void launch_profiles_sweep(nb_sim *s, uint32_t pieces, const double *vcen, uint32_t ncenters, const float *e2, uint32_t nbins)
{
    using real = typename LT::real;
    using vec = typename LT::vec;
    const nb_sim::Neighbors &q = s->nbr;
    const nb_sim::Profiles &f = s->prf;
    ProfileEdges<8 * NS + 1> e;
    for (uint32_t t = 0; t <= 8u * NS; ++t) e.v[t] = t <= nbins ? e2[t] : HUGE_VALF;
    // the handle owns all n: vel[] is indexed by body
    profiles_sweep<LT, NS><<<pieces, 64, 0, s->stream>>>((const vec *)s->pos[s->cur], (const real *)s->mass, (const vec *)s->vel, q.sval, q.sxy,
                                                         (const float *)f.cen, vcen, ncenters, (const uint32_t *)f.rng, f.first, f.prow, e, e2[nbins], nbins, f.out,
                                                         f.partial);
}

// Shell sums about many centres: what a caller does with a group's centre once nb_group_catalog or nb_group_binding has found it,
// without nb_sync and a numpy pass per centre.
extern "C" int nb_radial_profiles(nb_sim *s, const float *centers, const double *vcenters, size_t ncenters, const float *edges, uint32_t nbins,
                                  nb_shell *out)
{
    const char *name = "nb_radial_profiles";
    if (!s || !centers || !edges || !out)
        return nb_fail(NB_EINVAL, "%s: NULL %s", name, !s ? "handle" : !centers ? "centers" : !edges ? "edges" : "out");
    if (ncenters < 1 || ncenters > PROFILES_CENTERS_MAX)
        return nb_fail(NB_EINVAL, "%s: ncenters must be 1 .. %zu (got %zu)", name, PROFILES_CENTERS_MAX, ncenters);
    if (nbins < 1 || nbins > NB_PROFILE_BINS_MAX) return nb_fail(NB_EINVAL, "%s: nbins must be 1 .. %d (got %u)", name, NB_PROFILE_BINS_MAX, nbins);
    const size_t records = ncenters * nbins;
    if (records > PROFILES_RECORDS_MAX)
        return nb_fail(NB_EINVAL, "%s: ncenters * nbins must be at most %zu records (%zu * %u = %zu)", name, PROFILES_RECORDS_MAX, ncenters, nbins, records);
    float e2[NB_PROFILE_BINS_MAX + 1];
    { const int rc = pair_counts_edges(name, edges, nbins, e2); if (rc) return rc; }
    const size_t D = s->dims3 ? 3 : 2;
    for (size_t t = 0; t < ncenters * D; ++t)
        if (!std::isfinite(centers[t]))
            return nb_fail(NB_EINVAL, "%s: centers[%zu] (centre %zu, axis %zu) is not finite (%g)", name, t, t / D, t % D, (double)centers[t]);
    if (vcenters)
        for (size_t t = 0; t < ncenters * D; ++t)
            if (!std::isfinite(vcenters[t]))
                return nb_fail(NB_EINVAL, "%s: vcenters[%zu] (centre %zu, axis %zu) is not finite (%g)", name, t, t / D, t % D, vcenters[t]);
    if (s->i_count < s->n)
        return nb_fail(NB_ESTATE, "%s: the handle owns %zu of the %zu bodies (a block handle holds the velocities of its block "
                                  "only); the catalogue is about whole groups and needs a handle that owns all n", name, s->i_count, s->n);
    { const int rc = query_enter(s, name); if (rc) return rc; }           // no snapshot wait, as in nb_neighbors
    { const int rc = neighbors_alloc(s, 0, false, false, false); if (rc) return rc; }
    { const int rc = profiles_alloc(s, ncenters, records); if (rc) return rc; }
    const size_t bytes = records * sizeof(nb_shell);
    { const int rc = query_stage(s, stage_need(out, bytes)); if (rc) return rc; }
    nb_sim::Neighbors &q = s->nbr;
    nb_sim::Profiles &f = s->prf;
    { const int rc = copy_h2d(s, f.cen, centers, ncenters * D * sizeof(float)); if (rc) return rc; }
    if (vcenters) { const int rc = copy_h2d(s, f.vcen, vcenters, ncenters * D * sizeof(double)); if (rc) return rc; }
    { const int rc = neighbors_cells(s, edges[nbins]); if (rc) return rc; }
    // 1. ranges and piece counts, the two scans, the totals
    const uint32_t n = (uint32_t)s->n, nc = (uint32_t)ncenters, waves = nc + 1u;
    const double inv_h = 1.0 / ((double)edges[nbins] * NEIGHBORS_CELL_SLACK);
    profiles_ranges<<<(waves + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, s->stream>>>(q.skey, n, (const float *)f.cen, (uint32_t)D, nc, inv_h, (uint32_t *)f.rng,
                                                                                      f.pieces, f.split);
    HIPCHK(hipGetLastError());
    size_t tmp = f.tmp_bytes;
    HIPCHK(nb_tree_scan(f.tmp, tmp, f.pieces, f.first, ncenters + 1, s->stream));
    tmp = f.tmp_bytes;
    HIPCHK(nb_tree_scan(f.tmp, tmp, f.split, f.prow, ncenters + 1, s->stream));
    HIPCHK(hipMemcpyAsync(&f.host[0], f.first + ncenters, sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(&f.host[1], f.prow + ncenters, sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    const uint64_t pieces = f.host[0], rows = f.host[1];
    if (pieces > 0x7fffffffull)
        return nb_fail(NB_ENOMEM, "%s: %llu pieces of %u candidates: the centres see more body-centre pairs than one launch takes", name,
                       (unsigned long long)pieces, PROFILES_PIECE);
    // 2. partial rows for the centres that are split: 64 B x nbins per piece of theirs
    HIPCHK(s->pool.regrow(f.part_cap, (size_t)rows * nbins, f.partial));    // (the stream is idle: the totals have just been read)
    std::pair<hipEvent_t, hipEvent_t> pr;                         // with nb_profile_enable the sweep and its combine launch count as one launch
    if (s->prof && prof_begin(s, &pr, nullptr)) return NB_EHIP;
    HIPCHK(hipMemsetAsync(f.out, 0, bytes, s->stream));           // a centre without candidates has no wave: its row is all zero
    if (pieces) {
        const double *vcen = vcenters ? (const double *)f.vcen : nullptr;
        const uint32_t g = (uint32_t)pieces, ns = nbins <= 8 ? 1u : nbins <= 16 ? 2u : nbins <= 32 ? 4u : 8u;
        with_layout(s, [&](auto L) {
            using LT = decltype(L);
            if (ns == 1) launch_profiles_sweep<LT, 1>(s, g, vcen, nc, e2, nbins);
            else if (ns == 2) launch_profiles_sweep<LT, 2>(s, g, vcen, nc, e2, nbins);
            else if (ns == 4) launch_profiles_sweep<LT, 4>(s, g, vcen, nc, e2, nbins);
            else launch_profiles_sweep<LT, 8>(s, g, vcen, nc, e2, nbins);
        });
        HIPCHK(hipGetLastError());
        if (rows) {
            const uint32_t gc = (uint32_t)std::min<uint64_t>(records, 16ull * (uint64_t)s->cus);
            profiles_combine<<<gc, BLOCK, 0, s->stream>>>(f.first, f.prow, nc, nbins, f.partial, f.out);
            HIPCHK(hipGetLastError());
        }
    }
    if (s->prof && prof_end(s, pr, nullptr, 1)) return NB_EHIP;
    return copy_plane(s, out, f.out, bytes);
}
