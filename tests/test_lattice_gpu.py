"""GPU: exact pair coverage of the tiled force paths on an integer lattice (tests/lattice_model.py).

For lattice bodies (x = k 2^-22 or k 2^-40, small integer masses, eps = 1, exact inverse square root) the softened direct sum is
an integer computation in the kernels' own arithmetic, so ANY summation order, fma contraction, slab split or rank split must
give the bits of the int64 closed form  a_i = u (sum_j m_j k_j - k_i sum_j m_j).  Every comparison here is np.array_equal on the
uint32 views against that closed form — nothing is compared with another output of the library.  A single pair that is dropped,
counted twice, given the wrong partner's mass or applied to one side only changes an integer and fails; the report names the
first differing body and the difference in lattice units (the missing or extra m_j (k_j - k_i)).

The premise tests come first: everything else rests on v_rsq_f32(4^k) = 2^-k exactly and rsqrt3_f64(1.0) = 1.  Every case takes
every layout (seed) that tests/test_lattice_cpu.py proves the magnitude bound and the blind cap for, and asserts through
describe() / sym_info() that the intended kernel variant ran.  One process; handles are closed in `finally` / `with`; after a
HIP error nothing more is started (every later test fails at once, naming the first error).
"""
import ctypes

import numpy as np
import pytest

import lattice_model as lm

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

pytestmark = pytest.mark.gpu

DT = 2.0 ** -10
_HIP_ERROR = []          # first HIP error of the module: nothing runs on the GPU after it


def _guard():
    if _HIP_ERROR:
        pytest.fail(f"not run: an earlier test of this module met a HIP error ({_HIP_ERROR[0]})")


class _watch:
    """Remember a HIP error raised inside the block (NB_EHIP) so that no later test touches the GPU."""

    def __enter__(self):
        _guard()
        return self

    def __exit__(self, et, ev, tb):
        if et is not None and issubclass(et, nb.NBodyError) and getattr(ev, "code", 0) == L.NB_EHIP:
            _HIP_ERROR.append(str(ev))
        return False


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_exact(got, k, m, unit_log2, desc, what, i0=0, scale=1.0):
    """got (rows i0 .. i0 + len(got) of the system) must carry the bits of the closed form times ``scale`` (a power of two)."""
    want = lm.exact_acc(k, m, unit_log2)[i0:i0 + got.shape[0]] * np.float32(scale)
    got = np.ascontiguousarray(got, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(bits(got), bits(want)):
        return
    same = bits(got) == bits(want)
    bad = np.argwhere(~same.all(axis=1)).ravel()
    i = int(bad[0])
    u = np.ldexp(1.0, unit_log2) * scale
    g_units, w_units = got[i].astype(np.float64) / u, want[i].astype(np.float64) / u
    msg = (f"{what}: {bad.size} of {got.shape[0]} bodies differ from the lattice sum; first: body {i0 + i} (site {k[i0 + i].tolist()}, "
           f"mass {int(m[i0 + i])}) got {g_units.tolist()} want {w_units.tolist()} lattice units, difference {(g_units - w_units).tolist()} "
           f"= the missing (-) or extra (+) sum of m_j (k_j - k_i); differing bodies {bad[:16].tolist()}{' ...' if bad.size > 16 else ''}\n{desc}")
    print(msg)
    pytest.fail(msg)


# ------------------------------------------------------------------------------------------------------- premises ---
PREMISES = [
    # id, precision, dims, masses of the four bodies, Simulation arguments, describe tokens
    ("fp32-uniform", "fp32", 2, (1, 1, 1, 1), {}, "uniform_mass=1 mass_scaled=0"),
    ("fp32-general", "fp32", 2, (2, 3, 1, 3), {}, "uniform_mass=0 mass_scaled=0"),
    ("fp32-folded", "fp32", 2, (1, 4, 16, 4), {"mass_scaling": True}, "uniform_mass=0 mass_scaled=1"),
    ("fp32-3d-uniform", "fp32", 3, (1, 1, 1, 1), {}, "uniform_mass=1 mass_scaled=0"),
    ("fp32-3d-general", "fp32", 3, (2, 3, 1, 3), {}, "uniform_mass=0 mass_scaled=0"),
    ("fp64-uniform", "fp64", 2, (1, 1, 1, 1), {}, "uniform_mass=1 mass_scaled=0"),
    ("fp64-general", "fp64", 2, (2, 3, 1, 3), {}, "uniform_mass=0 mass_scaled=0"),
    ("fp64-3d-uniform", "fp64", 3, (1, 1, 1, 1), {}, "uniform_mass=1 mass_scaled=0"),
    ("fp64-3d-general", "fp64", 3, (2, 3, 1, 3), {}, "uniform_mass=0 mass_scaled=0"),
]


def _premise_bodies(sites, masses, dims, unit):
    k = np.array(sites, np.int64)[:, :dims]
    m = np.array(masses, np.int64)
    b = nb.bodies_array(len(m))
    if dims == 3:
        b = b.view(nb.BODY3_DTYPE)
    b["pos"] = np.ldexp(k.astype(np.float64), unit).astype(np.float32)
    b["mass"] = m.astype(np.float32)
    return b, k, m


@pytest.mark.parametrize("name,precision,dims,masses,kw,tokens", PREMISES, ids=[p[0] for p in PREMISES])
def test_premise_two_bodies_and_a_coincident_pair_give_m_times_d_exactly(name, precision, dims, masses, kw, tokens):
    """What the whole module rests on, per precision x mass mode: the hardware inverse square root of 1 (and of 4, 16, 1/4, 1/16
    for the folded masses) is an exact power of two, so the acceleration of a pair a few lattice steps apart is m d to the bit —
    and a coincident pair contributes exactly 0."""
    unit = lm.UNIT_F64 if precision == "fp64" else lm.UNIT_F32
    with _watch():
        # (a) two bodies, 7 and 3 (and 2) lattice steps apart
        b, k, m = _premise_bodies([(3, 5, 9), (10, 2, 11)], masses[:2], dims, unit)
        with nb.Simulation(b, eps=1.0, precision=precision, dims=dims, **kw) as sim:
            desc = sim.describe()
            acc = sim.accelerations()
        d = (k[1] - k[0]).astype(np.float64)
        want = np.stack([m[1] * d, -m[0] * d]) * 2.0 ** unit
        assert np.array_equal(bits(acc), bits(want.astype(np.float32))), (name, (acc.astype(np.float64) / 2.0 ** unit).tolist(), (want / 2.0 ** unit).tolist(), desc)
        assert tokens in desc, desc
        # (b) the same two plus a coincident pair
        b, k, m = _premise_bodies([(3, 5, 9), (10, 2, 11), (100, 200, 300), (100, 200, 300)], masses, dims, unit)
        with nb.Simulation(b, eps=1.0, precision=precision, dims=dims, **kw) as sim:
            desc = sim.describe()
            assert tokens in desc, desc
            acc = sim.accelerations()
        assert not np.array_equal(acc[2], np.zeros(dims, np.float32))
        check_exact(acc, k, m, unit, desc, f"premise {name}")


# ---------------------------------------------------------------------------------------------- what a case expects ---
def expected_tokens(c, m):
    """The describe() fragments that prove the intended variant ran: derived from the documented selection rules
    (include/nbody.h: thresholds of the symmetric scheme, tile and chunk-pair switches), not read back from the handle."""
    kw = c.kw
    fp32_2d = c.precision == "fp32" and c.dims == 2
    uniform = kw.get("uniform_mass", True) and np.unique(m).size == 1
    scaled = bool(kw.get("mass_scaling")) and fp32_2d and not uniform
    sharded = c.shard is not None and c.shard[0] != "allgather"
    tile = 2048 if (not fp32_2d or sharded) else (kw.get("sym_tile", 0) or (512 if c.n < 49152 else 2048))
    sym = kw.get("symmetry", True) and c.n >= (5632 if tile == 512 else 16384) and not (c.shard and c.shard[0] == "allgather")
    out = [f"uniform_mass={int(uniform)} mass_scaled={int(scaled)}", f"symmetric={int(sym)}"]
    if sym:
        p = kw.get("sym_chunk_pairs", 0)
        want_pairs = c.precision == "fp32" and (p > 0 if p else c.n >= 65536)
        pairs = want_pairs and ((uniform or p > 0) if c.dims == 3 else not scaled)
        out.append(f"symmetric=1 tile={tile} chunk_pairs={int(pairs)}")
        if kw.get("sym_chunks_per_item", 0):
            out.append(f"chunks/item={kw['sym_chunks_per_item']} ")
    else:
        if kw.get("j_slices"):                                    # slices are whole LDS tiles of 256, evened out
            tiles = -(-c.n // 256)
            per = -(-tiles // min(kw["j_slices"], tiles))
            out.append(f"j_slices(all)={-(-tiles // per)} ")
        if kw.get("lanes_p"):
            out.append(f"i/lane={2 * kw['lanes_p']} ")
    return out, sym, tile


def plain_items(n, tile, L_):
    """Items of a whole-system plan without a guided tail: every tile's diagonal chunks and its later chunks, cut every L."""
    chunks, cpt = -(-n // 64), tile // 64
    items = 0
    for t in range(-(-n // tile)):
        d0, dend = t * cpt, min((t + 1) * cpt, chunks)
        items += -(-(dend - d0) // L_) + -(-(chunks - dend) // L_)
    return items


def assert_variant(c, m, sim):
    desc = sim.describe()
    tokens, sym, tile = expected_tokens(c, m)
    for t in tokens:
        assert t in desc, (c.id, t, desc)
    info = sim.sym_info()
    assert info["enabled"] == int(sym), (c.id, info)
    if sym and c.shard is None:
        assert info["tile_particles"] == tile and info["items_late"] == 0
        plain = plain_items(c.n, tile, info["chunks_per_item"])
        if not c.kw.get("guided_tail", True):
            assert info["items"] == plain, (c.id, info["items"], plain, desc)       # no tail: the uniform cut
        elif "sym_tail" in c.kw:
            assert info["items"] > plain, (c.id, info["items"], plain, desc)        # an early tail did cut items finer
    return desc


def run_case(c):
    """Every layout of the case on one unsharded handle."""
    for seed, b, k, m in lm.layouts(c):
        with _watch():
            with nb.Simulation(b, eps=1.0, precision=c.precision, dims=c.dims, **c.kw) as sim:
                desc = assert_variant(c, m, sim)
                if c.step:
                    sim.advance(1, DT)
                    got = sim.sync()
                    acc, vel = got["acc"].copy(), got["vel"].copy()
                else:
                    acc, vel = sim.accelerations(), None
        check_exact(acc, k, m, c.unit_log2, desc, f"{c.id} seed {seed}: acc")
        if vel is not None:                                       # the fused gather + kick: v = 0 + a dt, dt a power of two
            check_exact(vel, k, m, c.unit_log2, desc, f"{c.id} seed {seed}: vel", scale=DT)


def _ids(group):
    return [c.id for c in lm.cases(group)]


@pytest.mark.parametrize("c", lm.cases("one_sided"), ids=_ids("one_sided"))
def test_one_sided_and_lds_tiled_kernels_cover_every_pair(c):
    run_case(c)


@pytest.mark.parametrize("c", lm.cases("sym_f32"), ids=_ids("sym_f32"))
def test_symmetric_fp32_kernels_cover_every_pair(c):
    run_case(c)


@pytest.mark.parametrize("c", lm.cases("fp64"), ids=_ids("fp64"))
def test_fp64_kernels_cover_every_pair(c):
    run_case(c)


@pytest.mark.parametrize("c", lm.cases("3d"), ids=_ids("3d"))
def test_three_d_kernels_cover_every_pair(c):
    run_case(c)


@pytest.mark.parametrize("c", lm.cases("full"), ids=_ids("full"))
def test_full_size_every_single_pair_of_a_million_bodies(c):
    assert c.n == 1 << 20 and c.K == 16
    run_case(c)


# -------------------------------------------------------------------------------------------------------- sharded ---
def _drive_allgather(c, b, m, parts):
    """The loop of test_parity_gpu._run_sharded: P handles of contiguous blocks, the library's in-process all-gather."""
    lib = nb.load()
    bounds = np.linspace(0, c.n, parts + 1).astype(int)
    sims = []
    try:
        for r in range(parts):
            sims.append(nb.Simulation(b, eps=1.0, precision=c.precision, dims=c.dims, i_begin=int(bounds[r]),
                                      i_count=int(bounds[r + 1] - bounds[r]), **c.kw))
        assert all(s.shard_protocol == L.NB_SHARD_ALLGATHER and "symmetric=0" in s.describe() for s in sims), sims[0].describe()
        handles = (ctypes.c_void_p * parts)(*[s._h for s in sims])
        for s in sims:
            s.step_begin(DT)
        for s in sims:
            s.step_finish()
        L.check("nb_exchange_positions", lib.nb_exchange_positions(handles, parts))
        return [(s.i_begin, s.sync().copy(), s.describe()) for s in sims]
    finally:
        for s in sims:
            s.close()


def _drive_symmetric(c, b, m, parts):
    """The loop of test_symmetric_sharded_handles_in_process_match_unsharded: NB_SHARD_SYMMETRIC ranks of equal blocks."""
    lib = nb.load()
    blk = c.n // parts
    late = c.kw.get("sym_late_us", 0.0)
    sims = []
    try:
        for r in range(parts):
            sims.append(nb.Simulation(b, eps=1.0, precision=c.precision, dims=c.dims, i_begin=r * blk, i_count=blk, shard_rank=r,
                                      shard_world=parts, **c.kw))
        assert all(s.shard_protocol == L.NB_SHARD_SYMMETRIC for s in sims)
        for s in sims:
            assert_variant(c, m, s)
            # held-back local items: forced by sym_late_us > 0, off for < 0, the library's own choice (from 8 ranks on) for 0
            assert (s.sym_info()["items_late"] > 0) == (late > 0 or (late == 0 and parts >= 8)), (c.id, s.sym_info())
        handles = (ctypes.c_void_p * parts)(*[s._h for s in sims])
        for s in sims:
            s.step_begin(DT)
        for s in sims:
            s.step_mid()
        L.check("nb_exchange_accelerations", lib.nb_exchange_accelerations(handles, parts))
        for s in sims:
            s.step_finish()
        L.check("nb_exchange_positions", lib.nb_exchange_positions(handles, parts))
        return [(s.i_begin, s.sync().copy(), s.describe()) for s in sims]
    finally:
        for s in sims:
            s.close()


def _drive_allreduce(c, b, m, parts):
    """The loop of test_replicated_allreduce_protocol_in_process: every rank holds and integrates everything."""
    lib = nb.load()
    sims = []
    try:
        for r in range(parts):
            sims.append(nb.Simulation(b, eps=1.0, precision=c.precision, dims=c.dims, shard_rank=r, shard_world=parts,
                                      shard_allreduce=True, **c.kw))
        assert all(s.shard_protocol == L.NB_SHARD_ALLREDUCE and s.i_count == c.n for s in sims)
        infos = [s.sym_info() for s in sims]
        assert sum(i["units_cross"] for i in infos) == infos[0]["cross_units_total"] and all(i["items_late"] == 0 for i in infos)
        for s in sims:
            assert_variant(c, m, s)
        handles = (ctypes.c_void_p * parts)(*[s._h for s in sims])
        for s in sims:
            s.step_begin(DT)
        L.check("nb_exchange_allreduce", lib.nb_exchange_allreduce(handles, parts))
        for s in sims:
            s.step_finish()
        return [(0, s.sync().copy(), s.describe()) for s in sims]
    finally:
        for s in sims:
            s.close()


def _drive_single(c, b, m, parts):
    """NB_FLAG_SHARD_SINGLE: one rank runs a sharded protocol alone (the loop of test_dynamic_items_gpu)."""
    lib = nb.load()
    allreduce = c.kw.get("shard_allreduce", False)
    with nb.Simulation(b, eps=1.0, precision=c.precision, dims=c.dims, shard_rank=0, shard_world=1, shard_single=True, **c.kw) as s:
        assert s.shard_protocol == (L.NB_SHARD_ALLREDUCE if allreduce else L.NB_SHARD_SYMMETRIC), s.describe()
        assert_variant(c, m, s)
        assert s.sym_info()["items_late"] == 0, s.sym_info()      # the planner holds items back for world > 1 only (nb_plan.cpp)
        arr = (ctypes.c_void_p * 1)(s._h)
        s.step_begin(DT)
        if allreduce:
            L.check("nb_exchange_allreduce", lib.nb_exchange_allreduce(arr, 1))
        else:
            s.step_mid()
            L.check("nb_exchange_accelerations", lib.nb_exchange_accelerations(arr, 1))
        s.step_finish()
        if not allreduce:
            L.check("nb_exchange_positions", lib.nb_exchange_positions(arr, 1))
        s.wait()
        return [(0, s.sync().copy(), s.describe())]


DRIVERS = {"allgather": _drive_allgather, "symmetric": _drive_symmetric, "allreduce": _drive_allreduce, "single": _drive_single}


@pytest.mark.parametrize("c", lm.cases("sharded"), ids=_ids("sharded"))
def test_sharded_protocols_in_process_cover_every_pair(c):
    """One step with dt = 2^-10 through each exchange protocol, all ranks in this process on one GPU: the accelerations of every
    owned block (partial sums added across ranks are integers too) and the kick they produced."""
    protocol, parts = c.shard
    for seed, b, k, m in lm.layouts(c):
        with _watch():
            blocks = DRIVERS[protocol](c, b, m, parts)
        covered = 0
        for r, (i0, got, desc) in enumerate(blocks):
            check_exact(got["acc"], k, m, c.unit_log2, desc, f"{c.id} seed {seed} rank {r}: acc", i0=i0)
            check_exact(got["vel"], k, m, c.unit_log2, desc, f"{c.id} seed {seed} rank {r}: vel", i0=i0, scale=DT)
            covered += got.shape[0]
        assert covered == c.n * (parts if protocol == "allreduce" else 1)
