// nb_neighbors_host.hip.h — host side of nb_neighbors (kernels: nb_neighbors.hip.h).  Included by nb_capi.hip beside the raster and
// potential hosts; it sorts with nb_tree_sort_pairs (temporary storage of its own: the tree's key arrays are not borrowed), opens with
// query_enter and moves its planes with copy_plane through the query staging buffer, like nb_raster.
#pragma once

#ifdef NB_NEIGHBORS_PER_LANE                   // A/B builds (tools/neighbors_bench.py): every lane reads its candidates itself, no LDS
constexpr bool NEIGHBORS_COOPERATIVE = false;
#else
constexpr bool NEIGHBORS_COOPERATIVE = true;
#endif

template <int K>
static void launch_neighbors_search(nb_sim *s, uint32_t g, float r2, uint32_t k, uint32_t *idx, float *dist2, uint32_t *count)
{
    const nb_sim::Neighbors &q = s->nbr;
    const uint32_t n = (uint32_t)s->n, ib = (uint32_t)s->i_begin, ic = (uint32_t)s->i_count;
    if constexpr (NEIGHBORS_COOPERATIVE) neighbors_search_coop<K><<<g, BLOCK, 0, s->stream>>>(q.skey, q.sval, q.sxy, n, ib, ic, r2, k, idx, dist2, count);
    else neighbors_search<K><<<g, BLOCK, 0, s->stream>>>(q.skey, q.sval, q.sxy, n, ib, ic, r2, k, idx, dist2, count);
}

// Scratch.  Per body of the replica, from the first call on: 40 B (float position 8, cell key 8, body index 4, and the three again
// in sorted order) plus the sort's temporary storage.  Per owned body: 4 B once a count is asked for; per owned body x k: 4 B once
// indices, 4 B once distances are asked for.  Growth only.
static int neighbors_alloc(nb_sim *s, size_t entries, bool want_idx, bool want_d2, bool want_cnt)
{
    nb_sim::Neighbors &q = s->nbr;
    const size_t n = s->n;
    const bool grow_n = q.cap < n || !q.tmp;                     // (no tmp: a first attempt ran out of memory at its last request)
    const bool grow_i = want_idx && q.idx_cap < entries, grow_d = want_d2 && q.d2_cap < entries, grow_c = want_cnt && !q.cnt;
    if (!grow_n && !grow_i && !grow_d && !grow_c) return NB_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    if (grow_n) {
        s->pool.release(q.tmp);
        HIPCHK(s->pool.regrow(q.cap, n, q.xy, q.sxy, q.key, q.skey, q.val, q.sval));
        size_t bytes = 0;
        HIPCHK(nb_tree_sort_pairs(nullptr, bytes, q.key, q.skey, q.val, q.sval, n, s->stream));
        q.tmp_bytes = std::max<size_t>(bytes, 256);
        HIPCHK(s->pool.alloc(q.tmp, q.tmp_bytes));
    }
    if (grow_c) HIPCHK(s->pool.alloc(q.cnt, s->i_count));
    if (grow_i) HIPCHK(s->pool.regrow(q.idx_cap, entries, q.idx));
    if (grow_d) HIPCHK(s->pool.regrow(q.d2_cap, entries, q.d2));
    return NB_OK;
}

// The front half that nb_neighbors and nb_groups share: all n bodies of the current replica keyed by the cell of a grid of cell size
// radius x NEIGHBORS_CELL_SLACK, sorted, their float positions gathered in that order (skey, sval, sxy of `nbr`; neighbors_alloc first).
static int neighbors_cells(nb_sim *s, float radius)
{
    nb_sim::Neighbors &q = s->nbr;
    const uint32_t n = (uint32_t)s->n, g = (n + BLOCK - 1) / BLOCK;
    const double inv_h = 1.0 / ((double)radius * NEIGHBORS_CELL_SLACK);
    with_layout(s, [&](auto L) {
        using LT = decltype(L);
        neighbors_keys<LT><<<g, BLOCK, 0, s->stream>>>((const typename LT::vec *)s->pos[s->cur], n, inv_h, q.xy, q.key, q.val);
    });
    HIPCHK(hipGetLastError());
    size_t tmp = q.tmp_bytes;
    HIPCHK(nb_tree_sort_pairs(q.tmp, tmp, q.key, q.skey, q.val, q.sval, n, s->stream));
    neighbors_gather<<<g, BLOCK, 0, s->stream>>>(q.xy, q.sval, n, q.sxy);
    HIPCHK(hipGetLastError());
    return NB_OK;
}

// The reference's drawConnections (main.cpp:233-386) without the copy of all bodies and the host's hash-map pass: who is near every
// body, how many, and the k nearest of them.
extern "C" int nb_neighbors(nb_sim *s, float radius, uint32_t k, uint32_t *idx, float *dist2, uint32_t *count)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_neighbors: NULL handle");
    if (!idx && !dist2 && !count) return nb_fail(NB_EINVAL, "nb_neighbors: idx, dist2 and count are all NULL");
    float r2;
    { const int rc = check_radius("nb_neighbors", radius, &r2); if (rc) return rc; }
    const bool rows = idx || dist2;
    if (rows && (k < 1 || k > 32)) return nb_fail(NB_EINVAL, "nb_neighbors: k must be 1 .. 32 when idx or dist2 is asked for (got %u)", k);
    { const int rc = query_enter(s, "nb_neighbors"); if (rc) return rc; }     // no snapshot wait, as in nb_raster
    const size_t ic = s->i_count, entries = rows ? ic * k : 0, row_bytes = entries * sizeof(uint32_t), cnt_bytes = ic * sizeof(uint32_t);
    { const int rc = neighbors_alloc(s, entries, idx != nullptr, dist2 != nullptr, count != nullptr); if (rc) return rc; }
    { const int rc = query_stage(s, std::max({stage_need(idx, row_bytes), stage_need(dist2, row_bytes), stage_need(count, cnt_bytes)})); if (rc) return rc; }
    nb_sim::Neighbors &q = s->nbr;
    const uint32_t n = (uint32_t)s->n, g = (n + BLOCK - 1) / BLOCK;
    { const int rc = neighbors_cells(s, radius); if (rc) return rc; }
    std::pair<hipEvent_t, hipEvent_t> pr;                         // with nb_profile_enable the search counts as one launch
    if (s->prof && prof_begin(s, &pr, nullptr)) return NB_EHIP;
    uint32_t *di = idx ? q.idx : nullptr, *dc = count ? q.cnt : nullptr;
    float *dd = dist2 ? q.d2 : nullptr;
    // the capacity of the register list: the smallest of 4, 8, 16, 32 that holds k; 0 for a count-only call
    if (!rows) launch_neighbors_search<0>(s, g, r2, 0u, nullptr, nullptr, dc);
    else if (k <= 4) launch_neighbors_search<4>(s, g, r2, k, di, dd, dc);
    else if (k <= 8) launch_neighbors_search<8>(s, g, r2, k, di, dd, dc);
    else if (k <= 16) launch_neighbors_search<16>(s, g, r2, k, di, dd, dc);
    else launch_neighbors_search<32>(s, g, r2, k, di, dd, dc);
    HIPCHK(hipGetLastError());
    if (s->prof && prof_end(s, pr, nullptr, 1)) return NB_EHIP;
    if (idx) {
        const int rc = copy_plane(s, idx, q.idx, row_bytes);
        if (rc) return rc;
    }
    if (dist2) {
        const int rc = copy_plane(s, dist2, q.d2, row_bytes);
        if (rc) return rc;
    }
    return count ? copy_plane(s, count, q.cnt, cnt_bytes) : NB_OK;
}
