// nb_groups_host.hip.h — host side of nb_groups (kernels: nb_groups.hip.h).  Included by nb_capi.hip behind the neighbours' host, whose
// front half it shares: neighbors_alloc for the per-body arrays and the sort's storage, neighbors_cells for the keys, the sort and the
// gather.  It opens with query_enter and moves its planes with copy_plane through the query staging buffer, like nb_neighbors.
// Its own front half (groups_labels, groups_fault) is shared with nb_group_catalog (nb_group_catalog_host.hip.h).
#pragma once

#ifdef NB_GROUPS_PLAIN_TALLY                   // A/B builds (tools/groups_bench.py): one global add per body in the size pass
constexpr bool GROUPS_COMBINE = false;
#else
constexpr bool GROUPS_COMBINE = true;
#endif

// Scratch of its own, beside nb_neighbors' 40 B per body and sort storage: 4 B per body of the replica (parent[], then the labels)
// from the first call on; 4 B per body of the replica (member counts) and 4 B per owned body (the size plane) once sizes are asked
// for; two words on the device and two page-locked ones (fault word, number of groups).  Growth only.
static int groups_alloc(nb_sim *s, bool want_size)
{
    nb_sim::Groups &g = s->grp;
    const size_t n = s->n;
    const bool grow_s = want_size && !g.size;
    if (g.cap >= n && g.words && g.host && !grow_s) return NB_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(s->pool.regrow(g.cap, n, g.parent));
    if (!g.words) HIPCHK(s->pool.alloc(g.words, 2));
    if (!g.host) HIPCHK(s->pool.alloc_pinned(g.host, 2));
    if (grow_s) {
        s->pool.release(g.cnt);
        HIPCHK(s->pool.alloc(g.cnt, n));
        HIPCHK(s->pool.alloc(g.size, s->i_count));
    }
    return NB_OK;
}

// The front half that nb_groups and nb_group_catalog share: the scratch, the cells, and the union-find down to the flattened labels.
// Afterwards grp.parent[i] is the label of body i for all n bodies of the replica and grp.words[0] the fault word (still on the device:
// the caller copies grp.words to grp.host behind its own launches, synchronises and asks groups_fault).
static int groups_labels(nb_sim *s, float radius, float r2, bool want_size, bool profile_link)
{
    { const int rc = neighbors_alloc(s, 0, false, false, false); if (rc) return rc; }
    { const int rc = groups_alloc(s, want_size); if (rc) return rc; }
    nb_sim::Neighbors &q = s->nbr;
    nb_sim::Groups &g = s->grp;
    const uint32_t n = (uint32_t)s->n, blocks = (n + BLOCK - 1) / BLOCK;
    HIPCHK(hipMemsetAsync(g.words, 0, 2 * sizeof(uint32_t), s->stream));
    { const int rc = neighbors_cells(s, radius); if (rc) return rc; }
    groups_init<<<blocks, BLOCK, 0, s->stream>>>(g.parent, n);
    HIPCHK(hipGetLastError());
    std::pair<hipEvent_t, hipEvent_t> pr;                         // nb_groups: with nb_profile_enable the link kernel counts as one launch
    if (profile_link && s->prof && prof_begin(s, &pr, nullptr)) return NB_EHIP;
    groups_link<<<blocks, BLOCK, 0, s->stream>>>(q.skey, q.sval, q.sxy, n, r2, g.parent, &g.words[0]);
    HIPCHK(hipGetLastError());
    if (profile_link && s->prof && prof_end(s, pr, nullptr, 1)) return NB_EHIP;
    groups_flatten<<<blocks, BLOCK, 0, s->stream>>>(g.parent, n, &g.words[0]);
    HIPCHK(hipGetLastError());
    return NB_OK;
}

// the fault word, once it has reached grp.host: cannot be set while parent[x] <= x holds (nb_groups.hip.h); nothing is written
static int groups_fault(const nb_sim *s, const char *name)
{
    const uint32_t f = s->grp.host[0];
    if (!f) return NB_OK;
    return nb_fail(NB_EHIP, "%s: the union-find left its bound (%s): parent[] is no forest", name,
                   f & GROUPS_FAULT_FIND ? "a find of more than n + 1 hops" : "a unite of more than n + 1 rounds");
}

// Which bodies form a clump: the friends-of-friends groups at linking length `radius`, labelled by their smallest body index.
extern "C" int nb_groups(nb_sim *s, float radius, uint32_t *label, uint32_t *size, uint64_t *ngroups)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_groups: NULL handle");
    if (!label && !size && !ngroups) return nb_fail(NB_EINVAL, "nb_groups: label, size and ngroups are all NULL");
    float r2;
    { const int rc = check_radius("nb_groups", radius, &r2); if (rc) return rc; }
    { const int rc = query_enter(s, "nb_groups"); if (rc) return rc; }        // no snapshot wait, as in nb_neighbors
    const size_t bytes = s->i_count * sizeof(uint32_t);           // of either plane
    { const int rc = query_stage(s, std::max(stage_need(label, bytes), stage_need(size, bytes))); if (rc) return rc; }
    { const int rc = groups_labels(s, radius, r2, size != nullptr, true); if (rc) return rc; }
    nb_sim::Neighbors &q = s->nbr;
    nb_sim::Groups &g = s->grp;
    const uint32_t n = (uint32_t)s->n, blocks = (n + BLOCK - 1) / BLOCK, ib = (uint32_t)s->i_begin, ic = (uint32_t)s->i_count;
    if (ngroups) {
        groups_roots<<<std::min(blocks, 1024u), BLOCK, 0, s->stream>>>(g.parent, n, &g.words[1]);
        HIPCHK(hipGetLastError());
    }
    if (size) {
        HIPCHK(hipMemsetAsync(g.cnt, 0, (size_t)n * sizeof(uint32_t), s->stream));
        // workgroups that stay (all of them resident at once): the sum a workgroup carries from batch to batch pays when it sees several
        const uint32_t tg = GROUPS_COMBINE ? std::max(1u, std::min(blocks, 4u * (uint32_t)s->cus)) : blocks;
        groups_tally<GROUPS_COMBINE><<<tg, BLOCK, 0, s->stream>>>(g.parent, q.sval, n, g.cnt);
        HIPCHK(hipGetLastError());
        groups_sizes<<<(ic + BLOCK - 1) / BLOCK, BLOCK, 0, s->stream>>>(g.parent, g.cnt, ib, ic, g.size);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(g.host, g.words, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    { const int rc = groups_fault(s, "nb_groups"); if (rc) return rc; }
    if (label) {
        const int rc = copy_plane(s, label, g.parent + ib, bytes);
        if (rc) return rc;
    }
    if (size) {
        const int rc = copy_plane(s, size, g.size, bytes);
        if (rc) return rc;
    }
    if (ngroups) *ngroups = g.host[1];
    return NB_OK;
}
