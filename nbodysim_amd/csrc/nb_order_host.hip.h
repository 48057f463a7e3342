// nb_order_host.hip.h — host side of the body order of the whole-system symmetric path (kernels and the reasons: nb_order.hip.h).
// Included by nb_capi.hip beside the other split hosts.  Who gets an order is decided next to the size rules of the symmetric scheme
// (order_wanted, nb_capi.hip); here are its memory, the sort, and what runs ahead of every symmetric force evaluation.
#pragma once

// Per body: 4 + 4 B (perm, identity), 8 + 8 B (keys), one position in sorted order, plus the sort's temporary storage; with
// individual masses one mass more (order_masses).  Once, at nb_create.
static int order_alloc(nb_sim *s)
{
    nb_sim::Order &o = s->ord;
    const size_t n = s->n;
    HIPCHK(s->pool.alloc(o.perm, n));
    HIPCHK(s->pool.alloc(o.val, n));
    HIPCHK(s->pool.alloc(o.key, n));
    HIPCHK(s->pool.alloc(o.skey, n));
    HIPCHK(s->pool.alloc(o.part, (size_t)ORDER_PARTS * 4 * s->rsz));
    HIPCHK(s->pool.alloc(o.xs, n * s->esz));
    size_t bytes = 0;
    HIPCHK(nb_tree_sort_pairs(nullptr, bytes, o.key, o.skey, o.val, o.perm, n, s->stream));
    o.tmp_bytes = std::max<size_t>(bytes, 256);
    HIPCHK(s->pool.alloc(o.tmp, o.tmp_bytes));
    return NB_OK;
}

// nb_upload: the sorted copies the uploaded bodies' mass mode needs, and the count of evaluations starts over — the next force
// evaluation sorts the uploaded positions first.
static int order_upload(nb_sim *s)
{
    nb_sim::Order &o = s->ord;
    if (!s->uniform_mass && !o.ms) HIPCHK(s->pool.alloc(o.ms, s->n * s->rsz));
    if (s->sigma && !o.sigma_s) HIPCHK(s->pool.alloc(o.sigma_s, s->n));
    o.evals = 0;
    return NB_OK;
}

// perm <- the bodies along the curve at the current positions; the masses (and sigma) follow it now: they change with an upload only.
static int order_sort(nb_sim *s)
{
    nb_sim::Order &o = s->ord;
    const uint32_t n = (uint32_t)s->n, g = (n + BLOCK - 1) / BLOCK, parts = g < ORDER_PARTS ? g : ORDER_PARTS;
    with_layout(s, [&](auto L) {
        using real = typename decltype(L)::real;
        if constexpr (!L.dims3) {               // (order_wanted: 2-D handles only)
            using vec = typename decltype(L)::vec;
            const vec *pos = (const vec *)s->pos[s->cur];
            order_bounds<real><<<parts, BLOCK, 0, s->stream>>>(pos, n, (real *)o.part);
            order_keys<real><<<g, BLOCK, 0, s->stream>>>(pos, n, (const real *)o.part, parts, o.key, o.val);
        }
    });
    HIPCHK(hipGetLastError());
    size_t tmp = o.tmp_bytes;
    HIPCHK(nb_tree_sort_pairs(o.tmp, tmp, o.key, o.skey, o.val, o.perm, n, s->stream));
    if (!s->uniform_mass) {
        if (s->fp64) order_permute<double><<<g, BLOCK, 0, s->stream>>>((const double *)s->mass, o.perm, n, (double *)o.ms);
        else order_permute<float><<<g, BLOCK, 0, s->stream>>>((const float *)s->mass, o.perm, n, (float *)o.ms);
    }
    if (s->sigma) order_permute<float><<<g, BLOCK, 0, s->stream>>>(s->sigma, o.perm, n, o.sigma_s);
    HIPCHK(hipGetLastError());
    return NB_OK;
}

// Ahead of EVERY symmetric force evaluation of an ordered handle: a sort when one is due, then xs[k] = pos_cur[perm[k]].  The copy is
// unconditional — whatever moved the bodies since the last evaluation (the fused gather, a KDK drift, the collision pass, an upload),
// the kernel sees where they are now; 2 MB at 262 144 bodies.
static int order_prepare(nb_sim *s)
{
    nb_sim::Order &o = s->ord;
    if (o.evals % o.every == 0) { const int rc = order_sort(s); if (rc) return rc; }
    ++o.evals;
    const uint32_t n = (uint32_t)s->n, g = (n + BLOCK - 1) / BLOCK;
    if (s->fp64) order_permute<double2><<<g, BLOCK, 0, s->stream>>>((const double2 *)s->pos[s->cur], o.perm, n, (double2 *)o.xs);
    else order_permute<float2><<<g, BLOCK, 0, s->stream>>>((const float2 *)s->pos[s->cur], o.perm, n, (float2 *)o.xs);
    HIPCHK(hipGetLastError());
    return NB_OK;
}

// What the symmetric force kernel reads on this handle: the sorted copies of an ordered handle, the handle's own arrays otherwise.
static const void *sym_positions(const nb_sim *s) { return s->ord.on ? s->ord.xs : s->pos[s->cur]; }
static const void *sym_masses(const nb_sim *s) { return s->ord.on && !s->uniform_mass ? s->ord.ms : s->mass; }
static const float *sym_sigma(const nb_sim *s) { return s->ord.on && s->sigma ? s->ord.sigma_s : s->sigma; }

extern "C" int nb_body_order(nb_sim *s, uint32_t every, uint32_t *perm_out, uint32_t *every_out)
{
    if (!s) return nb_fail(NB_EINVAL, "nb_body_order: NULL handle");
    if (!s->ord.on) {
        if (every_out) *every_out = 0u;
        if (every || perm_out) return nb_fail(NB_ESTATE, "nb_body_order: the handle sweeps its bodies in the caller's order (nb_describe: order=0)");
        return NB_OK;
    }
    if (every) s->ord.every = every;
    if (every_out) *every_out = s->ord.every;
    if (!perm_out) return NB_OK;
    { const int rc = query_enter(s, "nb_body_order"); if (rc) return rc; }
    if (s->ord.evals == 0) { const int rc = order_sort(s); if (rc) return rc; }      // nothing evaluated since the upload: the order of the uploaded bodies
    const size_t bytes = s->n * sizeof(uint32_t);
    { const int rc = query_stage(s, stage_need(perm_out, bytes)); if (rc) return rc; }
    return copy_plane(s, perm_out, s->ord.perm, bytes);
}
