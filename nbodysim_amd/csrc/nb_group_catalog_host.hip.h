// nb_group_catalog_host.hip.h — host side of nb_group_catalog (kernels: nb_group_catalog.hip.h).  Included by nb_capi.hip behind the
// groups' host, whose front half it shares (groups_labels: scratch, cells, union-find, flattened labels; groups_fault).  Its own front
// half (catalog_count, catalog_launch_rows, catalog_launch_means) is shared with nb_group_binding (nb_group_binding_host.hip.h).  The sort by
// label runs in nb_neighbors' key / value arrays and sort storage, which are free again once the link kernel has read them.  It opens
// with query_enter and moves its records with copy_plane through the query staging buffer, like nb_tree_nodes.
#pragma once

// Scratch of its own, beside nb_groups' (44 B per body and the sort storage).  Per body of the replica, from the first call on: 16 B
// (head flag 4, rank 8, length / row by label 4) plus the scan's temporary storage, and 224 B per 1024 bodies (two carry slots per
// run); one page-locked word.  Growth only.
static int catalog_alloc(nb_sim *s)
{
    nb_sim::GroupCatalog &c = s->cat;
    const size_t n1 = s->n + 1, slots = 2 * ((s->n + CATALOG_RUN - 1) / CATALOG_RUN);
    if (c.cap >= n1 && c.tmp && c.slot_cap >= slots && c.host) return NB_OK;      // (no tmp: an earlier attempt ran out of memory at its last request)
    HIPCHK(hipStreamSynchronize(s->stream));
    if (c.cap < n1 || !c.tmp) {
        s->pool.release(c.tmp);
        HIPCHK(s->pool.regrow(c.cap, n1, c.flag, c.rank, c.len_row));
        size_t bytes = 0;
        HIPCHK(nb_tree_scan(nullptr, bytes, c.flag, c.rank, (size_t)c.cap, s->stream));
        c.tmp_bytes = std::max<size_t>(bytes, 256);
        HIPCHK(s->pool.alloc(c.tmp, c.tmp_bytes));
    }
    HIPCHK(s->pool.regrow(c.slot_cap, slots, c.slot));
    if (!c.host) HIPCHK(s->pool.alloc_pinned(c.host, 1));
    return NB_OK;
}

// Per group of a filling call: 184 B (the 13 sums 104, the record 80), with an eighth of slack so that a catalogue that grows a
// little every frame does not reallocate every frame; never more groups than bodies.
static int catalog_alloc_records(nb_sim *s, uint64_t count)
{
    nb_sim::GroupCatalog &c = s->cat;
    if (count <= c.rec_cap) return NB_OK;
    const uint64_t want = std::max<uint64_t>(count, std::min<uint64_t>(count + count / 8 + 1024, s->n));
    HIPCHK(s->pool.regrow(c.rec_cap, (size_t)want, c.sums, c.rec));              // (the stream is idle: the count has just been read)
    return NB_OK;
}

// The front half that nb_group_catalog and nb_group_binding share (nb_group_binding_host.hip.h), behind the NULL checks: the argument
// checks, query_enter, nb_groups' labels, the sort by label, heads, lengths, which groups are kept and their number.  It synchronises;
// afterwards *total is the count, nbr.skey / nbr.sval the sorted (label, index) pairs, cat.flag / cat.rank / cat.len_row what
// catalog_rows reads.
static int catalog_count(nb_sim *s, const char *name, float radius, uint32_t min_members, uint64_t *total)
{
    float r2;
    { const int rc = check_radius(name, radius, &r2); if (rc) return rc; }
    if (min_members == 0) return nb_fail(NB_EINVAL, "%s: min_members must be at least 1 (got 0)", name);
    if (s->i_count < s->n)
        return nb_fail(NB_ESTATE, "%s: the handle owns %zu of the %zu bodies (a block handle holds the velocities of its block "
                                  "only); the catalogue is about whole groups and needs a handle that owns all n", name, s->i_count, s->n);
    { const int rc = query_enter(s, name); if (rc) return rc; }    // no snapshot wait, as in nb_groups
    { const int rc = groups_labels(s, radius, r2, false, false); if (rc) return rc; }
    { const int rc = catalog_alloc(s); if (rc) return rc; }
    nb_sim::Neighbors &q = s->nbr;
    nb_sim::Groups &g = s->grp;
    nb_sim::GroupCatalog &c = s->cat;
    const uint32_t n = (uint32_t)s->n, blocks = (n + BLOCK - 1) / BLOCK, blocks1 = (uint32_t)(((uint64_t)n + 1 + BLOCK - 1) / BLOCK);
    // 1. the bodies by label; the sort is stable, so a group's members come out in ascending index
    catalog_labels<<<blocks, BLOCK, 0, s->stream>>>(g.parent, n, q.key, q.val);
    HIPCHK(hipGetLastError());
    size_t tmp = q.tmp_bytes;
    HIPCHK(nb_tree_sort_pairs(q.tmp, tmp, q.key, q.skey, q.val, q.sval, n, s->stream));
    // 2. heads, lengths, which groups are kept, their rows and their number
    catalog_heads<<<blocks1, BLOCK, 0, s->stream>>>(q.skey, n, min_members, c.flag, c.len_row);
    HIPCHK(hipGetLastError());
    tmp = c.tmp_bytes;
    HIPCHK(nb_tree_scan(c.tmp, tmp, c.flag, c.rank, (size_t)n + 1, s->stream));
    HIPCHK(hipMemcpyAsync(g.host, g.words, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(c.host, c.rank + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    { const int rc = groups_fault(s, name); if (rc) return rc; }
    *total = c.host[0];
    return NB_OK;
}

// label and members of the `count` records, and len_row[label] turned into the row (CATALOG_NO_ROW: not kept)
static int catalog_launch_rows(nb_sim *s)
{
    const uint32_t n = (uint32_t)s->n;
    catalog_rows<<<(n + BLOCK - 1) / BLOCK, BLOCK, 0, s->stream>>>(s->nbr.skey, n, s->cat.flag, s->cat.rank, s->cat.len_row, s->cat.rec);
    HIPCHK(hipGetLastError());
    return NB_OK;
}

// 3. pass A and its carries, then the means: mass, pos and vel of the `cnt` records (called inside with_layout)
template <typename LT>
static void catalog_launch_means(nb_sim *s, uint32_t cnt)
{
    using real = typename LT::real;
    using vec = typename LT::vec;
    constexpr int D = LT::dims3 ? 3 : 2;
    nb_sim::Neighbors &q = s->nbr;
    nb_sim::GroupCatalog &c = s->cat;
    const uint32_t n = (uint32_t)s->n, gb = (cnt + BLOCK - 1) / BLOCK, runs = (n + CATALOG_RUN - 1) / CATALOG_RUN, slots = 2 * runs;
    const vec *pos = (const vec *)s->pos[s->cur], *vel = (const vec *)s->vel;    // the handle owns all n: vel[] is indexed by body
    const real *mass = (const real *)s->mass;
    catalog_sums<LT><<<runs, BLOCK, 0, s->stream>>>(pos, mass, vel, q.skey, q.sval, c.len_row, n, c.sums, c.slot);
    catalog_carry<CatalogVal<1 + 4 * D, 0>><<<1, BLOCK, 0, s->stream>>>(c.slot, slots, c.len_row, c.sums);
    catalog_means<D><<<gb, BLOCK, 0, s->stream>>>(c.sums, cnt, c.rec);
}

// The group catalogue: what a caller of a group finder wants next, without nb_sync and a bincount pass on the host.
extern "C" int nb_group_catalog(nb_sim *s, float radius, uint32_t min_members, nb_group *out, size_t capacity, size_t *count)
{
    if (!s || !count) return nb_fail(NB_EINVAL, "nb_group_catalog: NULL %s", !s ? "handle" : "count");
    uint64_t total = 0;
    { const int rc = catalog_count(s, "nb_group_catalog", radius, min_members, &total); if (rc) return rc; }
    nb_sim::Neighbors &q = s->nbr;
    nb_sim::GroupCatalog &c = s->cat;
    const uint32_t n = (uint32_t)s->n;
    *count = (size_t)total;
    if (!out || total == 0) return NB_OK;
    if (capacity < total)
        return nb_fail(NB_EINVAL, "nb_group_catalog: %llu groups of at least %u members, out holds %zu", (unsigned long long)total, min_members, capacity);
    { const int rc = catalog_alloc_records(s, total); if (rc) return rc; }
    const size_t bytes = (size_t)total * sizeof(nb_group);
    // staging for the whole scratch, slack included, as nb_tree_nodes does
    { const int rc = query_stage(s, stage_need(out, bytes) ? (size_t)c.rec_cap * sizeof(nb_group) : 0); if (rc) return rc; }
    const uint32_t cnt = (uint32_t)total, gb = (cnt + BLOCK - 1) / BLOCK, runs = (n + CATALOG_RUN - 1) / CATALOG_RUN, slots = 2 * runs;
    { const int rc = catalog_launch_rows(s); if (rc) return rc; }
    std::pair<hipEvent_t, hipEvent_t> pr;                         // with nb_profile_enable the reduction passes count as one launch
    if (s->prof && prof_begin(s, &pr, nullptr)) return NB_EHIP;
    with_layout(s, [&](auto L) {
        using LT = decltype(L);
        using real = typename LT::real;
        using vec = typename LT::vec;
        const vec *pos = (const vec *)s->pos[s->cur], *vel = (const vec *)s->vel;
        const real *mass = (const real *)s->mass;
        catalog_launch_means<LT>(s, cnt);
        // 4. pass B about them, its carries, the division and the root
        catalog_spread<LT><<<runs, BLOCK, 0, s->stream>>>(pos, mass, vel, q.skey, q.sval, c.len_row, n, c.rec, c.sums, c.slot);
        catalog_carry<CatalogVal<2, 1>><<<1, BLOCK, 0, s->stream>>>(c.slot, slots, c.len_row, c.sums);
        catalog_finish<<<gb, BLOCK, 0, s->stream>>>(c.sums, cnt, c.rec);
    });
    HIPCHK(hipGetLastError());
    if (s->prof && prof_end(s, pr, nullptr, 1)) return NB_EHIP;
    return copy_plane(s, out, c.rec, bytes);
}
