// nb_group_binding_host.hip.h — host side of nb_group_binding (kernels: nb_group_binding.hip.h).  Included by nb_capi.hip behind the
// catalogue's host, whose front half it shares: catalog_count (argument checks, query_enter, labels, sort by label, heads, scan, the
// count), catalog_alloc_records, catalog_launch_rows and catalog_launch_means (pass A: the records' vel).  Pass B is not run.  It
// moves its planes and records with copy_plane through the query staging buffer, like nb_groups.
#pragma once

// Scratch of its own, beside the catalogue's.  Per body of the replica, from the first filling call on: the j-record in sorted order
// (16 B on an fp32 handle, 32 B on an fp64 one), the segment {start, length} 8 B, phi in sorted order 8 B and the two planes in body
// order 16 B: 48 / 64 B.  The start by label lives in cat.flag, which is free once catalog_rows has read it.  Growth only.
static int binding_alloc(nb_sim *s)
{
    nb_sim::GroupBinding &b = s->gbind;
    const size_t n = s->n, rec_bytes = n * (s->fp64 ? sizeof(BindingRec64) : sizeof(v4f));
    if (b.cap >= n && b.rec_bytes >= rec_bytes) return NB_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(s->pool.regrow(b.cap, n, b.seg, b.sphi, b.phi, b.e));
    HIPCHK(s->pool.regrow(b.rec_bytes, rec_bytes, b.srec));
    return NB_OK;
}

// Per group: 32 B (the record), grown with the catalogue's records (184 B, of which this call uses the sums and label, members, vel)
static int binding_alloc_records(nb_sim *s, uint64_t count)
{
    { const int rc = catalog_alloc_records(s, count); if (rc) return rc; }
    HIPCHK(s->pool.regrow(s->gbind.out_cap, (size_t)s->cat.rec_cap, s->gbind.out));
    return NB_OK;
}

// The sweep into gbind.sphi.  Positions per lane: 2 P with P = 1, a tile of 512.  P moves a position to another lane and changes no
// operation of its sum (nb_group_binding.hip.h), but P = 2 at 1 048 576 bodies measured 1.35 - 2.4 times SLOWER on Plummer spheres
// ("Group binding"): the work sits in the tiles of the large groups, and half as many tiles fill the chip worse.
static int launch_group_potential(nb_sim *s)
{
    nb_sim::GroupBinding &b = s->gbind;
    const uint32_t n = (uint32_t)s->n;
    std::pair<hipEvent_t, hipEvent_t> pr;                         // with nb_profile_enable the sweep counts as one launch
    if (s->prof && prof_begin(s, &pr, nullptr)) return NB_EHIP;
    with_layout(s, [&](auto L) {
        using LT = decltype(L);
        using real = typename LT::real;
        const real eps2 = (real)s->p.eps * (real)s->p.eps;        // as the force launch squares it
        if constexpr (std::is_same_v<real, double>) {
            group_potential_f64<LT><<<(n + BLOCK - 1) / BLOCK, BLOCK, 0, s->stream>>>((const BindingRec64 *)b.srec, b.seg, b.sphi, n, eps2);
        } else {
            constexpr uint32_t T = (BLOCK / 64) * 128;            // positions per workgroup
            group_potential<LT, 1><<<(uint32_t)(((uint64_t)n + T - 1) / T), BLOCK, 0, s->stream>>>((const v4f *)b.srec, b.seg, b.sphi, n, eps2);
        }
    });
    HIPCHK(hipGetLastError());
    if (s->prof && prof_end(s, pr, nullptr, 1)) return NB_EHIP;
    return NB_OK;
}

// Unbinding: which members of a group are bound to it, which one is its centre, and what its self-potential energy is.
extern "C" int nb_group_binding(nb_sim *s, float radius, uint32_t min_members, double *phi, double *e,
                                nb_group_energy *out, size_t capacity, size_t *count)
{
    if (!s || !count) return nb_fail(NB_EINVAL, "nb_group_binding: NULL %s", !s ? "handle" : "count");
    uint64_t total = 0;
    { const int rc = catalog_count(s, "nb_group_binding", radius, min_members, &total); if (rc) return rc; }
    *count = (size_t)total;
    if (!phi && !e && !out) return NB_OK;                         // the count query: no sweep
    if (out && capacity < total)
        return nb_fail(NB_EINVAL, "nb_group_binding: %llu groups of at least %u members, out holds %zu", (unsigned long long)total, min_members, capacity);
    { const int rc = binding_alloc(s); if (rc) return rc; }
    { const int rc = binding_alloc_records(s, total); if (rc) return rc; }
    nb_sim::Neighbors &q = s->nbr;
    nb_sim::GroupCatalog &c = s->cat;
    nb_sim::GroupBinding &b = s->gbind;
    const uint32_t n = (uint32_t)s->n, blocks = (n + BLOCK - 1) / BLOCK, cnt = (uint32_t)total, gb = (cnt + BLOCK - 1) / BLOCK;
    const uint32_t runs = (n + CATALOG_RUN - 1) / CATALOG_RUN, slots = 2 * runs;
    const size_t plane = (size_t)n * sizeof(double), bytes = (size_t)total * sizeof(nb_group_energy);
    // staging for the largest plane that needs it; for the records the whole scratch, slack included, as in nb_group_catalog
    { const int rc = query_stage(s, std::max({stage_need(phi, plane), stage_need(e, plane),
                                              stage_need(out, bytes) ? (size_t)b.out_cap * sizeof(nb_group_energy) : (size_t)0}));
      if (rc) return rc; }
    // 1. the rows, the start of every segment by label (in cat.flag, which catalog_rows has read by then), the records' vel
    { const int rc = catalog_launch_rows(s); if (rc) return rc; }
    binding_starts<<<blocks, BLOCK, 0, s->stream>>>(q.skey, n, c.flag);
    HIPCHK(hipGetLastError());
    if (cnt) with_layout(s, [&](auto L) { catalog_launch_means<decltype(L)>(s, cnt); });
    HIPCHK(hipGetLastError());
    // 2. j-records and segments in sorted order; NaN for the bodies of groups that are not kept
    with_layout(s, [&](auto L) {
        using LT = decltype(L);
        binding_gather<LT><<<blocks, BLOCK, 0, s->stream>>>((const typename LT::vec *)s->pos[s->cur], (const typename LT::real *)s->mass, q.skey, q.sval,
                                                            c.len_row, c.flag, c.rec, n, b.srec, b.seg, b.phi, b.e);
    });
    HIPCHK(hipGetLastError());
    if (cnt) {
        // 3. the sweep
        { const int rc = launch_group_potential(s); if (rc) return rc; }
        // 4. e, the planes in body order, the records
        with_layout(s, [&](auto L) {
            using LT = decltype(L);
            using vec = typename LT::vec;
            binding_records<LT><<<runs, BLOCK, 0, s->stream>>>((const vec *)s->pos[s->cur], (const typename LT::real *)s->mass, (const vec *)s->vel,
                                                               q.skey, q.sval, c.len_row, n, c.rec, b.sphi, b.phi, b.e, c.sums, c.slot);
        });
        catalog_carry<BindingVal><<<1, BLOCK, 0, s->stream>>>(c.slot, slots, c.len_row, c.sums);
        binding_finish<<<gb, BLOCK, 0, s->stream>>>(c.sums, c.rec, cnt, b.out);
        HIPCHK(hipGetLastError());
    }
    if (phi) { const int rc = copy_plane(s, phi, b.phi, plane); if (rc) return rc; }
    if (e) { const int rc = copy_plane(s, e, b.e, plane); if (rc) return rc; }
    if (out) { const int rc = copy_plane(s, out, b.out, bytes); if (rc) return rc; }
    return NB_OK;
}
