// nb_pair_counts_host.hip.h — host side of nb_pair_counts (kernels: nb_pair_counts.hip.h).  Included by nb_capi.hip behind the groups'
// hosts; it shares the neighbours' front half (neighbors_alloc for the per-body arrays and the sort's storage, neighbors_cells for the
// keys, the sort and the gather) and opens with query_enter.  The answer is at most 520 bytes: it moves through a page-locked block
// of the call's own, not through the query staging buffer.
#pragma once

#ifdef NB_PAIR_COUNTS_PER_LANE                 // A/B builds (tools/pair_counts_bench.py): every lane reads its candidates itself, no LDS
constexpr bool PAIR_COUNTS_COOPERATIVE = false;
#else
constexpr bool PAIR_COUNTS_COOPERATIVE = true;
#endif

constexpr uint32_t PAIR_COUNTS_WORDS = NB_PAIR_BINS_MAX + 1;      // cumulative counters of the widest call

// Scratch of its own, beside nb_neighbors' 40 B per body and sort storage: one row of 65 64-bit partials per workgroup of the count
// launch (at most 8 per compute unit: sized by the launch, not by n), 65 words on the device and 65 page-locked ones.  Growth only.
static int pair_counts_alloc(nb_sim *s, uint32_t rows)
{
    nb_sim::PairCounts &c = s->pairs;
    const size_t want = (size_t)rows * PAIR_COUNTS_WORDS;
    if (c.cap >= want && c.words && c.host) return NB_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(s->pool.regrow(c.cap, want, c.partial));
    if (!c.words) HIPCHK(s->pool.alloc(c.words, PAIR_COUNTS_WORDS));
    if (!c.host) HIPCHK(s->pool.alloc_pinned(c.host, PAIR_COUNTS_WORDS));
    return NB_OK;
}

template <int NB>
static void launch_pair_counts(nb_sim *s, uint32_t g, const float *e2, uint32_t nbins)
{
    const nb_sim::Neighbors &q = s->nbr;
    const uint32_t n = (uint32_t)s->n, ib = (uint32_t)s->i_begin, ic = (uint32_t)s->i_count;
    PairEdges<NB + 1> e;
    for (uint32_t t = 0; t <= (uint32_t)NB; ++t) e.v[t] = t <= nbins ? e2[t] : HUGE_VALF;
    unsigned long long *partial = (unsigned long long *)s->pairs.partial;
    with_flags([&](auto all) {
        constexpr bool ALL = decltype(all)::value;
        if constexpr (PAIR_COUNTS_COOPERATIVE) pair_counts_coop<NB, ALL><<<g, BLOCK, 0, s->stream>>>(q.skey, q.sval, q.sxy, n, ib, ic, e, partial);
        else pair_counts<NB, ALL><<<g, BLOCK, 0, s->stream>>>(q.skey, q.sval, q.sxy, n, ib, ic, e, partial);
    }, s->i_count == s->n);
}

// The edge rules nb_pair_counts and nb_radial_profiles share, behind the check of nbins: finite, edges[0] >= 0, strictly ascending, squares
// strictly ascending in float, r2max finite and not 0.  e2[0 .. nbins] receives the squares.
static int pair_counts_edges(const char *name, const float *edges, uint32_t nbins, float *e2)
{
    for (uint32_t t = 0; t <= nbins; ++t)
        if (!std::isfinite(edges[t])) return nb_fail(NB_EINVAL, "%s: edges[%u] is not finite (%g)", name, t, (double)edges[t]);
    if (edges[0] < 0.0f) return nb_fail(NB_EINVAL, "%s: edges[0] must be >= 0 (got %g)", name, (double)edges[0]);
    for (uint32_t t = 0; t < nbins; ++t)
        if (!(edges[t] < edges[t + 1]))
            return nb_fail(NB_EINVAL, "%s: edges must be strictly ascending (edges[%u] = %g, edges[%u] = %g)", name, t, (double)edges[t], t + 1,
                           (double)edges[t + 1]);
    for (uint32_t t = 0; t <= nbins; ++t) e2[t] = edges[t] * edges[t];      // one fp32 rounding: the kernel's operands
    for (uint32_t t = 0; t < nbins; ++t)
        if (!(e2[t] < e2[t + 1]))
            return nb_fail(NB_EINVAL, "%s: the squares of edges[%u] = %g and edges[%u] = %g are not ascending in float (%g, %g): the bin "
                                      "between them would be empty or inverted", name, t, (double)edges[t], t + 1, (double)edges[t + 1], (double)e2[t], (double)e2[t + 1]);
    // r2max finite and not 0: the same fp32 product as e2[nbins], which it overwrites with itself
    { const int rc = check_radius(name, edges[nbins], &e2[nbins]); if (rc) return rc; }
    return NB_OK;
}

// The histogram of pair separations, DD(r): what a two-point correlation function, a radial distribution function or a correlation
// dimension is made of, without neighbour rows capped at k or a copy of all bodies and a tree pass on the host.
extern "C" int nb_pair_counts(nb_sim *s, const float *edges, uint32_t nbins, uint64_t *counts)
{
    if (!s || !edges || !counts) return nb_fail(NB_EINVAL, "nb_pair_counts: NULL %s", !s ? "handle" : !edges ? "edges" : "counts");
    if (nbins < 1 || nbins > NB_PAIR_BINS_MAX) return nb_fail(NB_EINVAL, "nb_pair_counts: nbins must be 1 .. %d (got %u)", NB_PAIR_BINS_MAX, nbins);
    float e2[PAIR_COUNTS_WORDS];
    { const int rc = pair_counts_edges("nb_pair_counts", edges, nbins, e2); if (rc) return rc; }
    { const int rc = query_enter(s, "nb_pair_counts"); if (rc) return rc; }     // no snapshot wait, as in nb_neighbors
    const uint32_t n = (uint32_t)s->n, blocks = (n + BLOCK - 1) / BLOCK;
    // workgroups that stay: a workgroup reduces its lanes' counters once, behind its last batch
    const uint32_t g = std::max(1u, std::min(blocks, 8u * (uint32_t)s->cus));
    { const int rc = neighbors_alloc(s, 0, false, false, false); if (rc) return rc; }
    { const int rc = pair_counts_alloc(s, g); if (rc) return rc; }
    { const int rc = neighbors_cells(s, edges[nbins]); if (rc) return rc; }
    nb_sim::PairCounts &c = s->pairs;
    std::pair<hipEvent_t, hipEvent_t> pr;                         // with nb_profile_enable the count kernel counts as one launch
    if (s->prof && prof_begin(s, &pr, nullptr)) return NB_EHIP;
    // the bin capacity: the smallest of 8, 16, 32, 64 that holds nbins
    const uint32_t cap = nbins <= 8 ? 8u : nbins <= 16 ? 16u : nbins <= 32 ? 32u : 64u;
    if (cap == 8) launch_pair_counts<8>(s, g, e2, nbins);
    else if (cap == 16) launch_pair_counts<16>(s, g, e2, nbins);
    else if (cap == 32) launch_pair_counts<32>(s, g, e2, nbins);
    else launch_pair_counts<64>(s, g, e2, nbins);
    HIPCHK(hipGetLastError());
    if (s->prof && prof_end(s, pr, nullptr, 1)) return NB_EHIP;
    pair_counts_sum<<<cap + 1, BLOCK, 0, s->stream>>>((const unsigned long long *)c.partial, g, cap + 1, (unsigned long long *)c.words);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c.host, c.words, PAIR_COUNTS_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    for (uint32_t b = 0; b < nbins; ++b) counts[b] = c.host[b + 1] - c.host[b];
    return NB_OK;
}
