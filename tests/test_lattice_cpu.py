"""CPU: the integer-lattice model (tests/lattice_model.py) against a brute-force integer sum and against the project's own
oracle, and the conditions every case of the shared table must meet before tests/test_lattice_gpu.py may rely on it:
the magnitude bound  n (K - 1) m_max < 2^24  and at most 1e-4 of the pairs blind (on one site in every layout)."""
import numpy as np
import pytest

import lattice_model as lm

import nbodysim_amd as nb


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def brute_units(k, m):
    """sum_j m_j (k_j - k_i) by the O(n^2) definition, int64."""
    d = k[None, :, :] - k[:, None, :]                          # [i, j] = k_j - k_i
    return (m[None, :, None] * d).sum(1)


def test_pick_K_is_the_largest_power_of_two_under_the_bound():
    assert lm.pick_K(20000, 3) == 256 and lm.pick_K(262144, 2) == 32 and lm.pick_K(262144, 4) == 16 and lm.pick_K(1 << 20, 1) == 16
    assert lm.pick_K(1, 1) == lm.pick_K(3001, 3) == 512       # capped: |d|^2 must stay below 2^-25
    for n, m in ((20000, 3), (262144, 2), (262144, 4), (1 << 20, 1), (70001, 16)):
        K = lm.pick_K(n, m)
        assert n * (K - 1) * m < 2**24 <= n * (2 * K - 1) * m


def test_lattice_bodies_are_at_rest_on_exact_sites():
    for dims, unit in ((2, -22), (3, -22), (2, -40), (3, -40)):
        b, k, m = lm.lattice_bodies(777, 512, (1, 2, 3), 5, dims, unit)
        assert b.dtype == (nb.BODY3_DTYPE if dims == 3 else nb.BODY_DTYPE) and k.shape == (777, dims)
        assert k.min() >= 0 and k.max() < 512 and set(np.unique(m)) == {1, 2, 3}
        assert np.array_equal(b["pos"].astype(np.float64) * 2.0 ** -unit, k)
        assert not b["vel"].any() and not b["acc"].any() and not b["radius"].any() and np.array_equal(b["mass"], m)
        # the squared distance of any pair vanishes against eps^2 = 1 in the arithmetic of the handle it is meant for
        d2 = dims * (511 * 2.0 ** unit) ** 2
        assert (np.float32(1) + np.float32(d2) == np.float32(1)) if unit == -22 else (1.0 + d2 == 1.0)
    b1, k1, _ = lm.lattice_bodies(100, 64, (1,), 1)
    b2, k2, _ = lm.lattice_bodies(100, 64, (1,), 2)
    assert not np.array_equal(k1, k2)                          # seeds give different layouts


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("masses", [(1,), (3,), (1, 2, 3), (1, 4, 16), (0, 1)])
@pytest.mark.parametrize("n", [1, 2, 257, 2000])
def test_closed_form_equals_brute_force_integer_sum(n, masses, dims):
    _, k, m = lm.lattice_bodies(n, lm.pick_K(n, max(masses)), masses, 3, dims)
    want = brute_units(k, m)
    assert np.array_equal(lm.exact_units(k, m), want)
    for unit in (-22, -40):
        assert np.array_equal(lm.exact_acc(k, m, unit).astype(np.float64), want * 2.0 ** unit)


@pytest.mark.parametrize("masses", [(1,), (1, 2, 3), (1, 4, 16)])
@pytest.mark.parametrize("n", [1, 2, 63, 257, 1000, 3001])
def test_closed_form_equals_the_fp32_oracle_bit_for_bit(nbo, n, masses):
    """nbo.accel_f32 (reference arithmetic with the exact inverse square root, sequential fp32 running sum) on lattice bodies
    gives the closed form's bits: the model and the project's existing oracle agree."""
    b, k, m = lm.lattice_bodies(n, lm.pick_K(n, max(masses)), masses, 7)
    if n > 8:
        b["pos"][5], k[5] = b["pos"][6], k[6]                  # a coincident pair
    ax, ay = nbo.accel_f32(nbo.state_from_bodies(b), 1.0, nbo.RSQRT_EXACT)
    assert np.array_equal(bits(np.stack([ax, ay], 1)), bits(lm.exact_acc(k, m)))


@pytest.mark.parametrize("masses", [(1,), (1, 2, 3)])
@pytest.mark.parametrize("n", [2, 257, 3001])
def test_closed_form_equals_the_fp64_oracles_after_rounding_to_float(nbo, n, masses):
    b, k, m = lm.lattice_bodies(n, lm.pick_K(n, max(masses)), masses, 9, 2, lm.UNIT_F64)
    ax, ay = nbo.accel_f64(nbo.state_from_bodies(b, np.float64), 1.0)
    assert np.array_equal(bits(np.stack([ax, ay], 1).astype(np.float32)), bits(lm.exact_acc(k, m, lm.UNIT_F64)))
    b, k, m = lm.lattice_bodies(n, lm.pick_K(n, max(masses)), masses, 9, 3, lm.UNIT_F64)
    a3 = np.stack(nbo.accel3_f64(nbo.state3_from_bodies(b), 1.0), 1)
    assert np.array_equal(bits(a3.astype(np.float32)), bits(lm.exact_acc(k, m, lm.UNIT_F64)))


def test_blind_fraction_counts_pairs_on_one_site_in_every_layout():
    k = np.array([[0, 0], [0, 0], [1, 0], [0, 0]])            # 3 of 6 pairs on one site
    assert lm.blind_fraction([k]) == 0.5
    k2 = np.array([[5, 5], [5, 5], [5, 5], [7, 7]])           # ... of which only (0, 1) stays together in the second layout
    assert lm.blind_fraction([k, k2]) == pytest.approx(1 / 6)
    assert lm.blind_fraction([k[:1]]) == 0.0 and lm.blind_fraction([np.arange(8).reshape(4, 2)]) == 0.0
    _, ka, _ = lm.lattice_bodies(20000, 8, (1,), 1)
    assert abs(lm.blind_fraction([ka]) - 1 / 64) < 1e-3       # one layout: K^-dims


TUPLES = sorted({(c.n, c.K, c.masses, c.seeds, c.dims, c.unit_log2) for c in lm.CASES})


def test_the_case_table_covers_what_the_gpu_module_runs():
    assert {c.group for c in lm.CASES} == {"one_sided", "sym_f32", "fp64", "3d", "full", "sharded"}
    assert all(len(c.seeds) >= 2 for c in lm.CASES)
    assert all((c.unit_log2 == lm.UNIT_F64) == (c.precision == "fp64") for c in lm.CASES)
    assert all(set(c.masses) <= {1, 4, 16} for c in lm.CASES if c.kw.get("mass_scaling"))


@pytest.mark.parametrize("n,K,masses,seeds,dims,unit", TUPLES, ids=[f"n{t[0]}-K{t[1]}-m{'_'.join(map(str, t[2]))}-d{t[4]}-u{t[5]}" for t in TUPLES])
def test_every_case_meets_the_magnitude_bound_and_the_blind_cap(n, K, masses, seeds, dims, unit):
    assert K <= lm.K_MAX and K & (K - 1) == 0 and n * (K - 1) * max(masses) < 2**24
    assert dims * ((K - 1) * 2.0 ** unit) ** 2 < 2.0 ** -24   # |d|^2 below half an ulp of eps^2 = 1 (fp32; far below in fp64)
    ks = []
    for seed in seeds:
        _, k, m = lm.lattice_bodies(n, K, masses, seed, dims, unit)
        assert np.abs(lm.exact_units(k, m)).max() < 2**24
        ks.append(k)
    assert lm.blind_fraction(ks) <= lm.BLIND_CAP
