"""CPU: the composed integrators NB_INTEGRATOR_DKD and NB_INTEGRATOR_FR4 — the numpy model alone (tests/integrators_model.py:
convergence order, reversal, the coefficient sums) and what the library decides before it looks for a device."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import integrators_model as im  # noqa: E402

EPS, T = 0.05, 0.25
NEW = (("dkd", L.NB_INTEGRATOR_DKD if hasattr(L, "NB_INTEGRATOR_DKD") else 2), ("fr4", L.NB_INTEGRATOR_FR4 if hasattr(L, "NB_INTEGRATOR_FR4") else 3))


@pytest.fixture(scope="module")
def ring():
    """64 bodies of mass 1/64 on near-circular orbits."""
    rng = np.random.default_rng(1)
    r = np.sqrt(rng.uniform(0.2, 1.0, 64))
    phi = rng.uniform(0.0, 2.0 * np.pi, 64)
    x = np.stack([r * np.cos(phi), r * np.sin(phi)], 1)
    s = 0.7 * np.sqrt(r)
    v = np.stack([-s * np.sin(phi), s * np.cos(phi)], 1)
    return x, v, np.full(64, 1.0 / 64)


def run(ring, name, steps, t=T):
    x, v, m = ring
    h = np.float32(t / steps)                    # the model takes h as the library does: a C float
    for _ in range(steps):
        x, v, _a = im.step(x, v, lambda q: im.accel_plain(q, m, EPS), h, name)
    return x, v, float(h) * steps


def test_sums_of_the_coefficients_are_one():
    for name in ("dkd", "fr4"):
        kicks = sum(k for k, _ in im.STAGES[name])
        drifts = im.LEAD[name] + sum(d for _, d in im.STAGES[name])
        print(f"{name}: sum of kicks - 1 = {kicks - 1.0:.1e}, sum of drifts - 1 = {drifts - 1.0:.1e}")
        assert abs(kicks - 1.0) <= 2.0 ** -51 and abs(drifts - 1.0) <= 2.0 ** -51          # 1 to the rounding of three doubles near 1.35
    assert im.STAGES["dkd"] == ((1.0, 0.5),) and im.LEAD["dkd"] == 0.5
    assert abs(im.THETA - 1.0 / (2.0 - 2.0 ** (1.0 / 3.0))) < 1e-15 and im.STAGES["fr4"][1][0] < 0     # the middle kick runs backwards


@pytest.mark.parametrize("name,ideal", [("dkd", 4.0), ("fr4", 16.0)])
def test_convergence_order_of_the_model(ring, name, ideal):
    """max |x - x_ref| at T = 0.25 against FR4 at 2048 steps: halving the step divides it by 2^p, p = 2 (DKD) and 4 (FR4), within 10 %.
    The float h = T / steps is exact for these counts (T and the counts are powers of two), so every run ends at the same time."""
    ref, _, t_ref = run(ring, "fr4", 2048)
    err = {}
    for steps in (32, 64):
        x, _, t = run(ring, name, steps)
        assert t == t_ref == T
        err[steps] = np.max(np.abs(x - ref))
    ratio = err[32] / err[64]
    print(f"{name}: error {err[32]:.3e} at 32 steps, {err[64]:.3e} at 64: ratio {ratio:.3f} (ideal {ideal:g})")
    assert 0.9 * ideal <= ratio <= 1.1 * ideal, ratio


@pytest.mark.parametrize("name", ["dkd", "fr4"])
def test_the_model_reverses_to_rounding(ring, name):
    x0, v0, m = ring
    x, v, _ = run((x0, v0, m), name, 16)
    x, v, _ = run((x, -v, m), name, 16)
    back = np.max(np.abs(x - x0))
    print(f"{name}: 16 steps, v -> -v, 16 steps: max |x - x0| = {back:.1e}")
    assert back <= 1e-14 and np.max(np.abs(-v - v0)) <= 1e-13


# ------------------------------------------------------------------------------------------------------ the library ---
def direct_params():
    return L.default_params()


def tree_params():
    p = L.default_params()
    p.force, p.theta = L.NB_FORCE_TREE, 0.5
    p.flags = L.NB_FLAG_TREE_LEAVES | L.NB_FLAG_TREE_QUADRUPOLE | L.NB_FLAG_TREE_RELATIVE | L.NB_FLAG_TREE_ENERGY
    return p


def small_bodies(n=16):
    b = nb.bodies_array(n)
    b["mass"] = 1.0
    b["pos"][:, 0] = np.arange(n)
    return b


def test_abi_additions():
    header = (Path(__file__).resolve().parents[1] / "include" / "nbody.h").read_text()
    assert "NB_INTEGRATOR_DKD = 2" in header and "NB_INTEGRATOR_FR4 = 3" in header and "#define NB_ABI_VERSION 8" in header
    assert (L.NB_INTEGRATOR_DKD, L.NB_INTEGRATOR_FR4) == (2, 3) and nb.load().nb_abi_version() == 8


@pytest.mark.parametrize("name,value", NEW)
@pytest.mark.parametrize("params", [direct_params, tree_params], ids=["direct", "tree"])
def test_create_takes_the_new_integrators_as_far_as_the_device(name, value, params):
    """Without a device nb_create gets as far as NB_ENODEVICE: the parameters were accepted.  With one it returns a handle."""
    lib = nb.load()
    b = small_bodies()
    p = params()
    p.integrator = value
    h = lib.nb_create(b.ctypes.data, b.shape[0], C.byref(p))
    if h:
        lib.nb_destroy(h)
    else:
        assert lib.nb_last_error_code() == L.NB_ENODEVICE, lib.nb_last_error()


REFUSED = [
    (dict(shard_world=2, shard_rank=0), b"shard_world > 1"),
    (dict(i_begin=0, i_count=8), b"i_count < n"),
    (dict(flags=L.NB_FLAG_SHARD_SINGLE), b"NB_FLAG_SHARD_SINGLE"),
    (dict(flags=L.NB_FLAG_SHARD_ALLREDUCE), b"NB_FLAG_SHARD_ALLREDUCE"),
    (dict(extras=L.NB_EXTRA_COLLIDE), b"NB_EXTRA_COLLIDE"),
    (dict(extras=L.NB_EXTRA_COLLIDE | L.NB_EXTRA_VCLAMP), b"NB_EXTRA_COLLIDE"),
]


@pytest.mark.parametrize("name,value", NEW)
@pytest.mark.parametrize("params", [direct_params, tree_params], ids=["direct", "tree"])
def test_create_refuses_the_partners_by_name_before_looking_for_a_device(name, value, params):
    lib = nb.load()
    b = small_bodies()
    cases = list(REFUSED)
    if name == "fr4":
        cases += [(dict(extras=L.NB_EXTRA_VCLAMP), b"extras"), (dict(extras=L.NB_EXTRA_BOUNDARY), b"extras"), (dict(extras=3), b"extras")]
    for change, partner in cases:
        p = params()
        p.integrator = value
        for k, v in change.items():
            setattr(p, k, getattr(p, k) | v if k == "flags" else v)
        assert not lib.nb_create(b.ctypes.data, b.shape[0], C.byref(p)), change
        text = lib.nb_last_error()
        assert lib.nb_last_error_code() == L.NB_EINVAL and name.upper().encode() in text and partner in text, (change, text)


def test_dkd_takes_the_clamp_and_the_boundary():
    lib = nb.load()
    b = small_bodies()
    for extras in (1, 2, 3):
        p = direct_params()
        p.integrator, p.extras = L.NB_INTEGRATOR_DKD, extras
        h = lib.nb_create(b.ctypes.data, b.shape[0], C.byref(p))
        if h:
            lib.nb_destroy(h)
        else:
            assert lib.nb_last_error_code() == L.NB_ENODEVICE, lib.nb_last_error()


def test_integrators_outside_the_enum_are_still_refused():
    lib = nb.load()
    b = small_bodies()
    for value in (-1, 4):
        p = direct_params()
        p.integrator = value
        assert not lib.nb_create(b.ctypes.data, b.shape[0], C.byref(p))
        assert lib.nb_last_error_code() == L.NB_EINVAL and b"bad integrator" in lib.nb_last_error()


@pytest.mark.parametrize("name,value", NEW)
def test_the_dump_header_round_trips_the_new_integrators(tmp_path, name, value):
    lib = nb.load()
    b = small_bodies(5)
    p = L.default_params()
    p.integrator, p.eps, p.dt = value, 0.25, 2.0 ** -7
    path = str(tmp_path / f"{name}.nbd").encode()
    L.check("nb_write_bodies", lib.nb_write_bodies(path, b.ctypes.data, 5, 7, C.byref(p)))
    n, frame, q = C.c_size_t(), C.c_uint64(), L.nb_params()
    L.check("nb_read_header", lib.nb_read_header(path, C.byref(n), C.byref(frame), C.byref(q)))
    assert (n.value, frame.value, q.integrator, q.eps, q.dt) == (5, 7, value, 0.25, 2.0 ** -7)
    raw = bytearray(Path(path.decode()).read_bytes())
    raw[56:60] = (4).to_bytes(4, "little")                       # the integrator word of the 64-byte header: 4 is outside the enum
    Path(path.decode()).write_bytes(bytes(raw))
    assert lib.nb_read_header(path, None, None, None) == L.NB_EFORMAT


class _Spy:
    """The library with nb_create watched: what Simulation put into nb_params.integrator."""

    def __init__(self, lib):
        self._lib, self.seen = lib, []

    def __getattr__(self, k):
        return getattr(self._lib, k)

    def nb_create(self, bodies, n, params):
        self.seen.append(int(params._obj.integrator))
        return self._lib.nb_create(bodies, n, params)


@pytest.mark.parametrize("name,value", NEW)
def test_the_simulation_keyword_maps_the_two_strings(name, value):
    spy = _Spy(nb.load())
    try:
        nb.Simulation(small_bodies(), eps=0.1, integrator=name, library=spy).close()
    except L.NBodyError as e:
        assert e.code == L.NB_ENODEVICE, e                       # accepted; there is no device here
    assert spy.seen == [value]
