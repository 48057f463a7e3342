"""GPU: nb_potentials — the direct sweeps against the float64 sum (tests/potential_model.py), the walk of a NB_FLAG_TREE_ENERGY handle
against its numpy statement (tests/tree_energy_model.py, phi), and what the call must leave alone."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import potential_model as pm  # noqa: E402
import tree_energy_model as tem  # noqa: E402
import tree_leaves_model as tlm  # noqa: E402
import tree_model as tm  # noqa: E402
import tree_quad_model as tqm  # noqa: E402
import tree_rel_model as trm  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parents[1] / "tests" / "golden"
BAR_F32 = 4e-6        # tests/test_potential_cpu.py has the derivation: 3.5 ulp per term + the 63 roundings of a float32 run of 64
BAR_F64 = 1e-12       # n x 1.1e-16 of sequential same-signed float64 adds (n <= 777) + the 1.4e-16 reciprocal square root
BAR_TREE = 1e-10      # the project's energy bar (ENERGY_BAR, tests/test_tree_energy_gpu.py)
SENTINEL = -12345.678


def bodies_of(pos, m, vel=None) -> np.ndarray:
    pos = np.asarray(pos, np.float32)
    b = nb.bodies_array(pos.shape[0])
    v = b.view(L.BODY3_DTYPE) if pos.shape[1] == 3 else b
    v["pos"] = pos
    if vel is not None:
        v["vel"] = vel
    b["mass"] = m
    return b


@functools.lru_cache(maxsize=None)
def gold(name):
    """(pos (n, 2), m, vel) of a golden fixture, read once, shared, read-only."""
    flat = np.load(GOLD / f"{name}.npy").astype(np.float32)
    out = (flat[:, 0:2].copy(), flat[:, 6].copy(), flat[:, 2:4].copy())
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cloud(n, dims=2, seed=3):
    """n bodies with individual masses (no two on one position), shared, read-only."""
    rng = np.random.default_rng(seed)
    pos = rng.normal(0, 1, (n, dims)).astype(np.float32)
    m = rng.uniform(0.5, 2.0, n).astype(np.float32)
    pos.setflags(write=False); m.setflags(write=False)
    return pos, m


def direct(bodies, eps=0.05, **kw):
    return nb.Simulation(bodies, eps=eps, device=0, **kw)


def tree_sim(bodies, eps, theta, **kw):
    kw.setdefault("tree_energy", True)
    kw.setdefault("tree_leaves", True)
    return nb.Simulation(bodies, eps=eps, theta=theta, force="tree", device=0, **kw)


def within(got, want, bar, what):
    err = pm.rel_err(got, want)
    print(f"{what}: max relative error {err.max():.3g} at body {int(err.argmax())}, median {np.median(err):.3g} (bar {bar:g})")
    return bool(err.max() <= bar)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the fp32 sweep, 2-D
# ---------------------------------------------------------------------------------------------------------------------
def input_2d(n):
    if n == 333:
        return gold("ic_random_333")[:2]
    if n == 4096:
        return gold("ic_plummer_4096")[:2]
    return cloud(n)


@pytest.mark.parametrize("n", [2, 255, 257, 333, 1000, 4096])
def test_fp32_2d_against_the_fp64_sum(n):
    """One tile and a part of one, two tiles, 333 = a ragged last wave with a shared position, several workgroups."""
    pos, m = input_2d(n)
    with direct(bodies_of(pos, m)) as sim:
        got = sim.potentials()
    assert got.dtype == np.float64 and got.shape == (n,)
    assert within(got, pm.phi_f64(pos, m, 0.05), BAR_F32, f"fp32 2-D n {n}")


def test_fp32_2d_on_the_reference_start_with_its_central_mass():
    """default_ics_first4096 at eps = 1: body 0 weighs 1e9, so a wrong self-mask is off by 1e9 there."""
    pos, m, _ = gold("default_ics_first4096")
    assert m[0] == 1e9
    with direct(bodies_of(pos, m), eps=1.0) as sim:
        got = sim.potentials()
    assert within(got, pm.phi_f64(pos, m, 1.0), BAR_F32, "the reference's first 4096 bodies")


def test_one_body_has_potential_zero():
    for kw in (dict(), dict(precision="fp64"), dict(dims=3)):
        pos, m = cloud(2, kw.get("dims", 2))
        with direct(bodies_of(pos[:1], m[:1]), **kw) as sim:
            got = sim.potentials()
        assert got.shape == (1,) and got[0] == 0.0 and not np.signbit(got[0]), kw


# ---------------------------------------------------------------------------------------------------------------------
# 2. coverage: one massive body at j, everything else a tracer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", [0, 255, 256, 511, 999])
def test_one_hot_mass_reaches_every_body_once(j):
    """phi_i = -1 / R_ij for every i != j and exactly 0 at i = j: every tile edge, and the mask in both tiles a workgroup's
    i-range overlaps."""
    n, eps = 1000, 0.05
    pos, _ = cloud(n)
    m = np.zeros(n, np.float32)
    m[j] = 1.0
    with direct(bodies_of(pos, m), eps=eps) as sim:
        got = sim.potentials()
    d = pos.astype(np.float64) - pos[j].astype(np.float64)
    want = -1.0 / np.sqrt((d * d).sum(1) + pm.eps_of(eps) ** 2)
    want[j] = 0.0
    assert got[j] == 0.0
    assert within(got, want, BAR_F32, f"one-hot mass at {j}")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the owned block, two handles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(precision="fp64"), dict(dims=3)], ids=["fp32", "fp64", "fp32-3d"])
def test_owned_block_returns_the_bits_of_its_slice(kw):
    """[300, 800) of 1000 straddles two j-tiles and starts on no tile or workgroup boundary."""
    pos, m = cloud(1000, kw.get("dims", 2))
    b = bodies_of(pos, m)
    with direct(b, **kw) as one, direct(b, **kw) as two, direct(b, i_begin=300, i_count=500, **kw) as part:
        whole, again, got = one.potentials(), two.potentials(), part.potentials()
    assert got.shape == (500,) and np.isfinite(whole).all() and (whole < 0).all()
    assert np.array_equal(bits(whole), bits(again))
    assert np.array_equal(bits(got), bits(whole[300:800]))


@pytest.mark.parametrize("dims", [2, 3])
def test_particles_per_lane_do_not_change_a_bit(dims):
    """The library picks P = 1, 2 or 4 by the size of the owned block (P = 2 from 262 144 bodies on, P = 4 from 524 288, on 256 CUs);
    nb_params.lanes_p forces each here.  1000 bodies: one workgroup at P = 4 (its i-range overlaps all four j-tiles), two at P = 2."""
    pos, m = cloud(1000, dims)
    b = bodies_of(pos, m)
    out = {}
    for p in (0, 1, 2, 4):
        with direct(b, dims=dims, lanes_p=p) as sim, direct(b, dims=dims, lanes_p=p, i_begin=300, i_count=500) as part:
            out[p] = sim.potentials()
            assert np.array_equal(bits(part.potentials()), bits(out[p][300:800])), p
    assert within(out[4], pm.phi_f64(pos, m, 0.05), BAR_F32, f"{dims}-D, four particle pairs per lane")
    for p in (1, 2, 4):
        assert np.array_equal(bits(out[p]), bits(out[0])), p


# ---------------------------------------------------------------------------------------------------------------------
# 4. shared positions, eps = 0
# ---------------------------------------------------------------------------------------------------------------------
def shared_pair():
    pos, m, _ = gold("ic_random_333")
    same = [(a, b) for a in range(333) for b in range(a + 1, 333) if (pos[a] == pos[b]).all()]
    assert same == [(7, 8)]                                    # (tests/test_tree_energy_gpu.py names the pair)
    return pos, m


def test_bodies_on_one_position_see_each_other_through_the_softening():
    pos, m = shared_pair()
    eps = 0.05
    with direct(bodies_of(pos, m), eps=eps) as sim:
        got = sim.potentials()
    want = pm.phi_f64(pos, m, eps)
    assert within(got, want, BAR_F32, "ic_random_333 with its shared position")
    for a, b in ((7, 8), (8, 7)):                              # the -m / eps term is there, and leaving it out would miss the bar
        term = float(m[b]) / pm.eps_of(eps)
        assert got[a] < -term and term > 1e3 * BAR_F32 * abs(want[a])


@pytest.mark.parametrize("kw", [dict(), dict(precision="fp64")], ids=["fp32", "fp64"])
def test_without_softening(kw):
    bar = BAR_F64 if kw else BAR_F32
    pos, m, _ = gold("ic_plummer_1024")
    with direct(bodies_of(pos, m), eps=0.0, **kw) as sim:
        got = sim.potentials()
    assert np.isfinite(got).all() and within(got, pm.phi_f64(pos, m, 0.0), bar, "eps 0, no shared position")
    pos, m = shared_pair()
    with direct(bodies_of(pos, m), eps=0.0, **kw) as sim:
        got = sim.potentials()
    assert not np.isfinite(got[[7, 8]]).any()
    rest = np.delete(np.arange(333), [7, 8])
    assert np.isfinite(got[rest]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. 3-D, fp64
# ---------------------------------------------------------------------------------------------------------------------
def test_fp32_3d_against_the_fp64_sum():
    b = nb.plummer_3d(1500, 9)
    v = b.view(L.BODY3_DTYPE)
    with direct(b, dims=3) as sim:
        got = sim.potentials()
    assert v["pos"][:, 2].std() > 0.1
    assert within(got, pm.phi_f64(v["pos"], v["mass"], 0.05), BAR_F32, "fp32 3-D plummer 1500")


@pytest.mark.parametrize("dims,n", [(2, 777), (3, 500)])
def test_fp64_against_the_fp64_sum(dims, n):
    pos, m = cloud(n, dims)
    with direct(bodies_of(pos, m), precision="fp64", dims=dims) as sim:
        got = sim.potentials()
    assert within(got, pm.phi_f64(pos, m, 0.05), BAR_F64, f"fp64 {dims}-D n {n}")


# ---------------------------------------------------------------------------------------------------------------------
# 6. 1/2 sum m phi is nb_energy's potential
# ---------------------------------------------------------------------------------------------------------------------
def half_sum(m, phi):
    w = np.asarray(m, np.float64)
    return float(0.5 * np.sum(np.where(w != 0, w * phi, 0.0)))


def close(got, want, bar, what):
    rel = abs(got - want) / abs(want)
    print(f"{what}: got {got:.15e} want {want:.15e} relative {rel:.3g} (bar {bar:g})")
    return rel <= bar


def test_identity_with_the_energy():
    pos, m = cloud(777)
    with direct(bodies_of(pos, m), precision="fp64") as sim:
        assert close(half_sum(m, sim.potentials()), sim.energy()[1], BAR_F64, "fp64")
    pos, m = cloud(1000)
    with direct(bodies_of(pos, m)) as sim:
        assert close(half_sum(m, sim.potentials()), sim.energy()[1], BAR_F32, "fp32")
    pos, m, _ = gold("ic_plummer_1024")
    with tree_sim(bodies_of(pos, m), 0.05, 0.5) as sim:
        assert close(half_sum(m, sim.potentials()), sim.energy()[1], BAR_TREE, "tree energy handle")


# ---------------------------------------------------------------------------------------------------------------------
# 7. NB_FLAG_TREE_ENERGY handles: the walker's phi
# ---------------------------------------------------------------------------------------------------------------------
TREE_FIXTURES = {"ic_random_333": 0.5, "ic_plummer_1024": 0.05}      # the softenings of tests/test_tree_energy_gpu.py


@functools.lru_cache(maxsize=None)
def tree_of(name):
    pos, m, _ = gold(name)
    x, y, mm = pos[:, 0].copy(), pos[:, 1].copy(), m.copy()
    tree = tm.build_canonical(x, y, mm)
    return x, y, mm, tree, tqm.moments(tree)


@pytest.mark.parametrize("name", list(TREE_FIXTURES))
def test_tree_walk_against_the_model(name):
    eps = TREE_FIXTURES[name]
    x, y, m, tree, mom = tree_of(name)
    b = bodies_of(np.stack([x, y], 1), m)
    ok = []
    with tree_sim(b, eps, 0.5) as sim:
        ok.append(within(sim.potentials(), tem.phi(tree, mom, x, y, m, eps, 0.5, False), BAR_TREE, f"{name} theta 0.5"))
    with tree_sim(b, eps, 0.7, tree_quadrupole=True) as sim:
        ok.append(within(sim.potentials(), tem.phi(tree, mom, x, y, m, eps, 0.7, True), BAR_TREE, f"{name} theta 0.7 quadrupole"))
    with tree_sim(b, eps, 1.0, tree_alpha=0.005) as sim:
        aprev = sim.accelerations()
        assert aprev.any()
        got = sim.potentials()
        pairs = trm.pairs_of(tree, x, y, m, aprev, eps, 1.0, 0.005, 64)[0]
        ok.append(within(got, tem.phi(tree, mom, x, y, m, eps, 1.0, False, pairs), BAR_TREE, f"{name} theta 1 relative"))
        plain = tem.phi(tree, mom, x, y, m, eps, 1.0, False)
        assert pm.rel_err(got, plain).max() > BAR_TREE               # ... and not the theta walk's value
    with tree_sim(b, eps, 0.0) as sim:
        ok.append(within(sim.potentials(), pm.phi_f64(np.stack([x, y], 1), m, eps), BAR_TREE, f"{name} theta 0 against the direct sum"))
    assert all(ok)


def test_tree_walk_gives_massless_tracers_the_models_phi():
    pos, m, _ = gold("ic_plummer_1024")
    m = m.copy()
    tracers = [5, 77, 299, 1023]
    m[tracers] = 0.0
    x, y = pos[:, 0].copy(), pos[:, 1].copy()
    tree = tm.build_canonical(x, y, m)
    want = tem.phi(tree, tqm.moments(tree), x, y, m, 0.05, 0.5, False)
    with tree_sim(bodies_of(pos, m), 0.05, 0.5) as sim:
        got = sim.potentials()
    assert (want[tracers] < 0).all()
    assert within(got, want, BAR_TREE, "with four massless tracers")
    assert within(got[tracers], want[tracers], BAR_TREE, "the tracers")


def test_tree_walk_does_not_depend_on_the_rsqrt_mode_and_permutes():
    pos, m, _ = gold("ic_plummer_1024")
    perm = np.random.default_rng(18).permutation(1024)
    out = []
    for rsqrt, p, mm in (("exact", pos, m), ("quake", pos, m), ("exact", pos, m), ("exact", pos[perm], m[perm])):
        with tree_sim(bodies_of(p, mm), 0.05, 0.5, rsqrt=rsqrt, tree_quadrupole=True) as sim:
            out.append(sim.potentials())
    assert np.array_equal(bits(out[0]), bits(out[1])) and np.array_equal(bits(out[0]), bits(out[2]))
    assert within(out[3], out[0][perm], 1e-12, "permuted bodies: the same terms in another order")


@pytest.mark.parametrize("kw", [dict(), dict(tree_leaves=True), dict(tree_leaves=True, tree_quadrupole=True, rsqrt="quake")],
                         ids=["reference-walk", "leaves", "leaves-quad-quake"])
def test_tree_handle_without_the_energy_flag_runs_the_direct_sweep(kw):
    pos, m, _ = gold("ic_plummer_1024")
    b = bodies_of(pos, m)
    with nb.Simulation(b, eps=0.05, theta=0.5, force="tree", device=0, **kw) as t, direct(b) as d:
        got, want = t.potentials(), d.potentials()
    assert (want < 0).all() and np.array_equal(bits(got), bits(want))


# ---------------------------------------------------------------------------------------------------------------------
# 8. nothing of the handle changes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [lambda b: direct(b), lambda b: direct(b, integrator="kdk"),
                                  lambda b: tree_sim(b, 0.05, 0.5, tree_quadrupole=True)], ids=["direct", "direct-kdk", "tree-energy"])
def test_the_trajectory_does_not_notice_the_call(make):
    pos, m, vel = gold("ic_plummer_1024")
    b = bodies_of(pos, m, vel)
    end = []
    for call in (True, False):
        with make(b) as sim:
            sim.advance(1, 1e-3)
            before = {f: sim.sync()[f].copy() for f in ("pos", "vel", "acc")}
            assert before["acc"].any()
            if call:
                assert (sim.potentials() < 0).all()
                after = sim.sync()
                for f in ("pos", "vel", "acc"):
                    assert np.array_equal(bits(after[f]), bits(before[f])), f
                assert sim.frame == 1
            sim.advance(1, 1e-3)
            assert sim.frame == 2
            end.append({f: sim.sync()[f].copy() for f in ("pos", "vel", "acc")})
    for f in ("pos", "vel", "acc"):
        assert np.array_equal(bits(end[0][f]), bits(end[1][f])), f


# ---------------------------------------------------------------------------------------------------------------------
# 9. reports, refusals
# ---------------------------------------------------------------------------------------------------------------------
def unbuildable():
    """Pairs of positions one ulp apart that no rounded child centre separates (tests/test_tree_energy_gpu.py, its failed build)."""
    n = 512
    j = np.arange(n // 2)
    pos = np.zeros((n, 2), np.float32)
    pos[0::2, 0], pos[0::2, 1] = (j % 16) - 7.25, (j // 16) - 7.25
    pos[1::2, 0], pos[1::2, 1] = np.nextafter(pos[0::2, 0], np.float32(99)), pos[0::2, 1]
    return pos, np.full(n, 1.0 / n, np.float32)


def test_a_failed_build_is_reported_by_this_call_once():
    pos, m = unbuildable()
    with pytest.raises(OverflowError):
        tm.build_canonical(pos[:, 0].copy(), pos[:, 1].copy(), m.copy())
    phi = np.full(512, SENTINEL)
    with tree_sim(bodies_of(pos, m), 0.05, 1.0) as sim, tree_sim(bodies_of(pos, m), 0.05, 1.0) as twin:
        with pytest.raises(L.NBodyError) as e:
            sim.potentials(out=phi)
        assert e.value.code == L.NB_ENOMEM and "not separated within 63 levels" in str(e.value)
        assert (phi == SENTINEL).all()
        got = sim.sync()                                       # reported once: the next synchronising call passes
        assert np.array_equal(got["pos"], pos) and sim.frame == 0
        assert sim.tree_stats()["overflow_steps"] == 1
        # the next call on the same bodies: whatever nb_energy does in that place (it builds again)
        with pytest.raises(L.NBodyError):
            twin.energy()
        lib = nb.load()
        k, u = C.c_double(), C.c_double()
        want = lib.nb_energy(twin._h, C.byref(k), C.byref(u))
        assert lib.nb_potentials(sim._h, phi.ctypes.data) == want and want in (L.NB_ENOMEM, L.NB_ESTATE, L.NB_OK)
        if want != L.NB_OK:
            assert (phi == SENTINEL).all()
        good_pos, good_m, _ = gold("ic_plummer_1024")
        sim.upload(bodies_of(good_pos[:512], good_m[:512]))
        got = sim.potentials(out=phi)
        assert got is phi and np.isfinite(phi).all() and (phi < 0).all()


def test_a_pending_report_leaves_through_this_call_and_phi_is_not_written():
    """The failed build of a STEP, pending when nb_potentials is called on a tree handle without the energy flag."""
    pos, m = unbuildable()
    phi = np.full(512, SENTINEL)
    with tree_sim(bodies_of(pos, m), 0.05, 1.0, tree_energy=False) as sim:
        sim.advance(1, 1e-3)
        with pytest.raises(L.NBodyError) as e:
            sim.potentials(out=phi)
        assert e.value.code == L.NB_ENOMEM and (phi == SENTINEL).all()
        assert (sim.potentials(out=phi) < 0).all()             # once: the direct sweep of the positions, which did not move


def test_refusals():
    pos, m = cloud(1000)
    lib = nb.load()
    phi = np.full(1000, SENTINEL)
    with direct(bodies_of(pos, m), shard_rank=0, shard_world=1, shard_single=True) as sim:
        assert lib.nb_potentials(sim._h, None) == L.NB_EINVAL and b"nb_potentials: NULL phi" in lib.nb_last_error()
        assert lib.nb_potentials(None, phi.ctypes.data) == L.NB_EINVAL and b"nb_potentials: NULL handle" in lib.nb_last_error()
        for bad in (np.zeros(999), np.zeros(1000, np.float32), np.zeros((1000, 1)), np.zeros(2000)[::2]):
            with pytest.raises(TypeError):
                sim.potentials(out=bad)
        sim.step_begin(1e-3)
        assert lib.nb_potentials(sim._h, phi.ctypes.data) == L.NB_ESTATE and b"a split step is in flight" in lib.nb_last_error()
        assert (phi == SENTINEL).all()
        sim.step_mid()
        sim.step_finish()
        assert lib.nb_potentials(sim._h, phi.ctypes.data) == L.NB_OK and (phi < 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 10. destinations, profiling
# ---------------------------------------------------------------------------------------------------------------------
def test_pageable_and_page_locked_destinations_receive_the_same_bits():
    pos, m, _ = gold("ic_plummer_4096")
    lib = nb.load()
    ptr = lib.nb_host_alloc(4096 * 8)
    assert ptr
    try:
        pinned = np.frombuffer((C.c_uint8 * (4096 * 8)).from_address(ptr), dtype=np.float64)
        pinned[:] = SENTINEL
        with direct(bodies_of(pos, m)) as sim:
            pageable = sim.potentials()
            assert sim.potentials(out=pinned) is pinned
            assert np.array_equal(bits(pageable), bits(pinned)) and (pinned < 0).all()
            inside = np.full(5000, SENTINEL)                   # an unaligned pageable slice: the elements round it stay
            sim.potentials(out=inside[3:4099])
            assert np.array_equal(bits(inside[3:4099]), bits(pageable)) and (inside[:3] == SENTINEL).all() and (inside[4099:] == SENTINEL).all()
        del pinned
    finally:
        assert lib.nb_host_free(ptr) == 0


def test_the_sweep_counts_as_one_profiled_launch():
    pos, m, _ = gold("ic_plummer_1024")
    for make in (lambda b: direct(b), lambda b: tree_sim(b, 0.05, 0.5)):
        with make(bodies_of(pos, m)) as sim:
            sim.profile(True)
            sim.potentials()
            ms, launches = sim.profile_read()
            assert launches == 1 and ms > 0.0
