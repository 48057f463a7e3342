// nb_collide_host.hip.h — collisions (NB_EXTRA_COLLIDE): the host side of nb_collide.hip.h.  Part of nb_capi.hip's translation unit.
#pragma once
#include "nb_sim.hip.h"

static int collide_alloc_pairs(nb_sim *s, uint64_t cap)
{
    s->coll.cap = 0;                                // not grow-only: nb_collide_capacity may lower it, so this is always a new block
    HIPCHK(s->pool.regrow(s->coll.cap, 2 * cap, s->coll.adj));    // every pair sits in two rows ...
    s->coll.cap = cap;                              // ... and the capacity counts pairs
    return NB_OK;
}

// Everything the collision path needs, sized by n once (nb_create): radii never change on the device.
static int collide_alloc(nb_sim *s)
{
    const size_t n = s->n;
    uint32_t slots = 1024;
    while (slots < 2 * n) slots <<= 1;
    s->coll.slots = slots;
    s->coll.words = (uint32_t)((n + 31) / 32);
    HIPCHK(s->pool.alloc(s->coll.large, n));
    HIPCHK(s->pool.alloc(s->coll.large_list, COLLIDE_MAX_LARGE));
    HIPCHK(s->pool.alloc(s->coll.head, slots));
    HIPCHK(s->pool.alloc(s->coll.next, n));
    HIPCHK(s->pool.alloc(s->coll.cell, n));
    HIPCHK(s->pool.alloc(s->coll.deg, n));
    HIPCHK(s->pool.alloc(s->coll.off, n + 1));
    HIPCHK(s->pool.alloc(s->coll.tidx, n));
    HIPCHK(s->pool.alloc(s->coll.tlist, n));
    const size_t chunks = (n + COLLIDE_SCAN_CHUNK - 1) / COLLIDE_SCAN_CHUNK;
    HIPCHK(s->pool.alloc(s->coll.chunk_e, chunks));
    HIPCHK(s->pool.alloc(s->coll.chunk_t, chunks));
    HIPCHK(s->pool.alloc(s->coll.bits, (size_t)COLLIDE_MAX_LARGE * s->coll.words));
    HIPCHK(s->pool.alloc(s->coll.spos, n * s->esz));
    HIPCHK(s->pool.alloc(s->coll.svel, n * s->esz));
    HIPCHK(s->pool.alloc(s->coll.scur, n));
    HIPCHK(s->pool.alloc(s->coll.sadv, n));
    HIPCHK(s->pool.alloc(s->coll.stats, 1));
    HIPCHK(s->pool.alloc_pinned(s->coll.host, 1));
    HIPCHK(hipMemsetAsync(s->coll.stats, 0, sizeof(CollideStats), s->stream));
    memset(s->coll.host, 0, sizeof(CollideStats));
    const uint64_t cap = std::max<uint64_t>(8 * (uint64_t)n, 65536);
    return collide_alloc_pairs(s, cap);
}

// Size classes of the uploaded radii (magnitudes: the predicate squares r_i + r_j): r_q = the 99th percentile; bodies above
// 2 r_q are LARGE (at most COLLIDE_MAX_LARGE, else there is no large set) and are tested against all n; the grid cell is
// h = 2 x the largest small radius, raised by 2^-16 relative so that no pair the rounded predicate accepts (a few ulps past
// r_i + r_j) or the rounded cell quotient places can lie beyond the neighbouring cell.
static int collide_classify(nb_sim *s, const nb_body *in)
{
    const size_t n = s->n;
    std::vector<float> r(n);
    for (size_t i = 0; i < n; ++i) r[i] = std::fabs(in[i].radius);
    std::vector<float> sorted(r);
    const size_t q = (size_t)(0.99 * (double)(n - 1));
    std::nth_element(sorted.begin(), sorted.begin() + (long)q, sorted.end(),
                     [](float a, float b) { return a < b || (a == a && b != b); });   // NaN last
    const float rq = sorted[q];
    std::vector<uint8_t> large(n, 0);
    std::vector<uint32_t> list;
    for (size_t i = 0; i < n; ++i)
        if (r[i] > 2.0f * rq) { large[i] = 1; list.push_back((uint32_t)i); }
    if (list.size() > COLLIDE_MAX_LARGE) { std::fill(large.begin(), large.end(), 0); list.clear(); }
    double rmax = 0.0;
    for (size_t i = 0; i < n; ++i)
        if (!large[i] && r[i] == r[i]) rmax = std::max(rmax, (double)r[i]);
    s->coll.h = rmax > 0.0 ? 2.0 * rmax * (1.0 + 0x1p-16) : 1.0;      // radii all 0: only coincident bodies meet, any cell does
    s->coll.large_n = (uint32_t)list.size();
    { const int rc = copy_h2d(s, s->coll.large, large.data(), n); if (rc) return rc; }
    if (!list.empty()) { const int rc = copy_h2d(s, s->coll.large_list, list.data(), list.size() * sizeof(uint32_t)); if (rc) return rc; }
    return NB_OK;
}

// The collision pass of one step, on the post-drift state pos[cur] / vel (nb_collide.hip.h): `frame` is the frame it ends.
static int launch_collide(nb_sim *s)
{
    const uint32_t n = (uint32_t)s->n, g = (n + BLOCK - 1) / BLOCK;
    const uint32_t gc = std::min<uint32_t>((std::max(s->coll.slots, n) + BLOCK - 1) / BLOCK, 4096);
    const double inv_h = std::isfinite(s->coll.h) ? 1.0 / s->coll.h : 0.0;   // an infinite radius: one cell holds everybody
    const uint32_t mask = s->coll.slots - 1;
    collide_clear<<<gc, BLOCK, 0, s->stream>>>(s->coll.head, s->coll.slots, s->coll.deg, n);
    with_layout(s, [&](auto L) {
        using real = typename decltype(L)::real;
        using vec = typename decltype(L)::vec;
        if constexpr (!L.dims3) {
            vec *pos = (vec *)s->pos[s->cur], *vel = (vec *)s->vel;
            collide_hash<vec><<<g, BLOCK, 0, s->stream>>>(pos, n, s->coll.large, inv_h, mask, s->coll.head, s->coll.next, s->coll.cell);
            collide_rows<vec, false><<<g, BLOCK, 0, s->stream>>>(pos, s->radius, n, s->coll.large, s->coll.large_list, s->coll.large_n, mask,
                                                                 s->coll.head, s->coll.next, s->coll.cell, s->coll.deg, nullptr, nullptr,
                                                                 nullptr, s->coll.stats);
            if (s->coll.large_n)
                collide_large_bits<vec><<<dim3((s->coll.words + BLOCK - 1) / BLOCK, s->coll.large_n), BLOCK, 0, s->stream>>>(
                    pos, s->radius, n, s->coll.large_list, s->coll.words, s->coll.bits, s->coll.deg);
            const uint32_t chunks = (n + COLLIDE_SCAN_CHUNK - 1) / COLLIDE_SCAN_CHUNK;
            collide_scan_blocks<<<chunks, BLOCK, 0, s->stream>>>(s->coll.deg, n, s->coll.chunk_e, s->coll.chunk_t);
            collide_scan_top<<<1, BLOCK, 0, s->stream>>>(s->coll.chunk_e, s->coll.chunk_t, chunks, n, s->coll.off, s->coll.stats, s->coll.cap,
                                                         s->frame);
            collide_scan_fill<<<chunks, BLOCK, 0, s->stream>>>(s->coll.deg, n, s->coll.chunk_e, s->coll.chunk_t, s->coll.off, s->coll.tidx,
                                                               s->coll.tlist, s->coll.stats);
            collide_rows<vec, true><<<g, BLOCK, 0, s->stream>>>(pos, s->radius, n, s->coll.large, s->coll.large_list, s->coll.large_n, mask,
                                                                s->coll.head, s->coll.next, s->coll.cell, nullptr, s->coll.off, s->coll.tidx,
                                                                s->coll.adj, s->coll.stats);
            if (s->coll.large_n)
                collide_large_fill<<<s->coll.large_n, BLOCK, 0, s->stream>>>(s->coll.bits, s->coll.words, s->coll.large_list, s->coll.off,
                                                                             s->coll.tidx, s->coll.adj, s->coll.stats);
            collide_resolve<real, vec><<<1, COLLIDE_THREADS, 0, s->stream>>>(pos, vel, (const real *)s->mass, s->radius, s->coll.off,
                                                                              s->coll.tlist, s->coll.adj, s->coll.stats, (vec *)s->coll.spos,
                                                                              (vec *)s->coll.svel, s->coll.scur, s->coll.sadv);
        }
    });
    HIPCHK(hipGetLastError());
    return NB_OK;
}

// Reads the device record (waits for the handle's stream).  A step over capacity is reported ONCE, by the first synchronising
// call after it: NB_ENOMEM naming the frame, the pairs needed and the capacity.
static int collide_read(nb_sim *s)
{
    HIPCHK(hipMemcpyAsync(s->coll.host, s->coll.stats, sizeof(CollideStats), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return NB_OK;
}

// the report itself, from the host mirror as last read
static int collide_report(nb_sim *s)
{
    if (!s->collide) return NB_OK;
    const CollideStats &c = *s->coll.host;
    if (c.overflow_steps <= s->coll.ovf_reported) return NB_OK;
    const unsigned long long steps = (unsigned long long)(c.overflow_steps - s->coll.ovf_reported);
    s->coll.ovf_reported = c.overflow_steps;
    return nb_fail(NB_ENOMEM, "collisions: the step ending at frame %llu found %llu overlapping pairs, more than the capacity of %llu, "
                              "and resolved none (%llu step(s) over capacity since the last report); raise it with nb_collide_capacity",
                   (unsigned long long)c.overflow_frame, (unsigned long long)c.overflow_needed, (unsigned long long)s->coll.cap, steps);
}

static int collide_check(nb_sim *s)
{
    if (!s->collide) return NB_OK;
    const int rc = collide_read(s);
    return rc ? rc : collide_report(s);
}

extern "C" int nb_collide_capacity(nb_sim *s, size_t max_pairs)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_collide_capacity: NULL handle");
    if (!s->collide) return nb_fail(NB_ESTATE, "nb_collide_capacity: the handle was created without NB_EXTRA_COLLIDE");
    if (max_pairs == 0 || max_pairs > 0x7fffffffu) return nb_fail(NB_EINVAL, "nb_collide_capacity: max_pairs must be 1 .. 2^31 - 1");
    if (s->in_step) return nb_fail(NB_ESTATE, "nb_collide_capacity: a split step is in flight");
    if (bind(s)) return NB_EHIP;
    HIPCHK(hipStreamSynchronize(s->stream));          // the pair rows of the steps enqueued so far
    return collide_alloc_pairs(s, max_pairs);
}

extern "C" int nb_collision_stats(nb_sim *s, uint64_t *pairs_last_step, uint64_t *pairs_total, uint32_t *rounds_last_step,
                                  uint64_t *overflow_steps)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_collision_stats: NULL handle");
    if (bind(s)) return NB_EHIP;
    CollideStats c{};
    int rc = NB_OK;
    if (s->collide) {
        rc = collide_check(s);
        c = *s->coll.host;
        if (rc && nb_last_error_code() != NB_ENOMEM) return rc;
    }
    if (pairs_last_step) *pairs_last_step = c.pairs_last;
    if (pairs_total) *pairs_total = c.pairs_total;
    if (rounds_last_step) *rounds_last_step = c.rounds_last;
    if (overflow_steps) *overflow_steps = c.overflow_steps;
    return rc;
}
