// nb_neighbors_host.hip.h — host side of nb_neighbors (kernels: nb_neighbors.hip.h).  Included by nb_capi.hip beside the raster and
// potential hosts; it sorts with nb_tree_sort_pairs (temporary storage of its own: the tree's key arrays are not borrowed) and moves
// its planes with copy_d2h / pinned_covers like nb_raster.
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
// indices, 4 B once distances are asked for.  Page-locked staging for the largest plane a destination needed.  Growth only.
static int neighbors_alloc(nb_sim *s, size_t entries, bool want_idx, bool want_d2, bool want_cnt, size_t stage_bytes)
{
    nb_sim::Neighbors &q = s->nbr;
    const size_t n = s->n;
    const bool grow_i = want_idx && q.idx_cap < entries, grow_d = want_d2 && q.d2_cap < entries, grow_c = want_cnt && !q.cnt;
    const bool grow_s = q.stage_cap < stage_bytes;
    if (q.cap >= n && !grow_i && !grow_d && !grow_c && !grow_s) return NB_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    if (q.cap < n) {                                             // (a first attempt that ran out of memory half way left some of them)
        s->pool.release(q.xy); s->pool.release(q.sxy); s->pool.release(q.key); s->pool.release(q.skey);
        s->pool.release(q.val); s->pool.release(q.sval); s->pool.release(q.tmp);
        HIPCHK(s->pool.alloc(q.xy, n));
        HIPCHK(s->pool.alloc(q.sxy, n));
        HIPCHK(s->pool.alloc(q.key, n));
        HIPCHK(s->pool.alloc(q.skey, n));
        HIPCHK(s->pool.alloc(q.val, n));
        HIPCHK(s->pool.alloc(q.sval, n));
        size_t bytes = 0;
        HIPCHK(nb_tree_sort_pairs(nullptr, bytes, q.key, q.skey, q.val, q.sval, n, s->stream));
        q.tmp_bytes = std::max<size_t>(bytes, 256);
        HIPCHK(s->pool.alloc(q.tmp, q.tmp_bytes));
        q.cap = n;
    }
    if (grow_c) HIPCHK(s->pool.alloc(q.cnt, s->i_count));
    if (grow_i) {
        s->pool.release(q.idx);
        q.idx_cap = 0;
        HIPCHK(s->pool.alloc(q.idx, entries));
        q.idx_cap = entries;
    }
    if (grow_d) {
        s->pool.release(q.d2);
        q.d2_cap = 0;
        HIPCHK(s->pool.alloc(q.d2, entries));
        q.d2_cap = entries;
    }
    if (grow_s) {
        s->pool.release(q.stage);
        q.stage_cap = 0;
        HIPCHK(s->pool.alloc_pinned(q.stage, stage_bytes));
        q.stage_cap = stage_bytes;
    }
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
    if (!std::isfinite(radius) || !(radius > 0.0f)) return nb_fail(NB_EINVAL, "nb_neighbors: radius must be finite and > 0 (got %g)", (double)radius);
    const float r2 = radius * radius;                             // one fp32 rounding: the kernel's operand
    if (!std::isfinite(r2) || r2 == 0.0f)
        return nb_fail(NB_EINVAL, "nb_neighbors: radius * radius must be finite and > 0 in float (radius %g gives %g)", (double)radius, (double)r2);
    const bool rows = idx || dist2;
    if (rows && (k < 1 || k > 32)) return nb_fail(NB_EINVAL, "nb_neighbors: k must be 1 .. 32 when idx or dist2 is asked for (got %u)", k);
    if (s->in_step) return nb_fail(NB_ESTATE, "nb_neighbors: a split step is in flight");
    if (bind(s)) return NB_EHIP;
    // no snapshot_wait(), as in nb_raster: a pending snapshot reads aos_dev and never writes pos, and this call has scratch and staging of its own
    { const int rc = step_check(s); if (rc) return rc; }          // synchronises; a pending once-only report leaves through here, nothing written
    const size_t ic = s->i_count, entries = rows ? ic * k : 0, row_bytes = entries * sizeof(uint32_t), cnt_bytes = ic * sizeof(uint32_t);
    size_t stage_bytes = 0;
    if (idx && !pinned_covers(idx, row_bytes)) stage_bytes = std::max(stage_bytes, row_bytes);
    if (dist2 && !pinned_covers(dist2, row_bytes)) stage_bytes = std::max(stage_bytes, row_bytes);
    if (count && !pinned_covers(count, cnt_bytes)) stage_bytes = std::max(stage_bytes, cnt_bytes);
    { const int rc = neighbors_alloc(s, entries, idx != nullptr, dist2 != nullptr, count != nullptr, stage_bytes); if (rc) return rc; }
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
        const int rc = copy_d2h(s, idx, q.idx, row_bytes, s->stream, pinned_covers(idx, row_bytes) ? nullptr : q.stage);
        if (rc) return rc;
    }
    if (dist2) {
        const int rc = copy_d2h(s, dist2, q.d2, row_bytes, s->stream, pinned_covers(dist2, row_bytes) ? nullptr : q.stage);
        if (rc) return rc;
    }
    if (count) return copy_d2h(s, count, q.cnt, cnt_bytes, s->stream, pinned_covers(count, cnt_bytes) ? nullptr : q.stage);
    return NB_OK;
}
