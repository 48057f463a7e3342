"""Integer-lattice bodies for which the softened direct sum is EXACT in the kernels' own arithmetic, and their closed form.

Positions are x = k u with integer k in [0, K) per axis and u a power of two, masses are small integers, eps = 1:

* fp32 handles, u = 2^-22, K <= 512: |d|^2 <= 2^-25 in 2-D (3 x 2^-26 in 3-D), below half an ulp of 1, so every
  fma(d, d, 1.0f) rounds to exactly 1.0f, the inverse cube is 1 (given rsq(1) = 1, which the first GPU tests pin), every term
  m_j (k_j - k_i) u is an integer multiple of u, and so is every partial sum — in ANY order, with or without fma contraction,
  over any split into tiles, chunks, slabs or ranks — as long as  n (K - 1) m_max < 2^24.  Padding lanes (1e18 away) still
  underflow to exactly 0.
* fp64 handles, u = 2^-40: still exact in the float Body record; 1 + d^2 rounds to 1 in double; the result comes back through
  the float record, where an integer below 2^24 survives a last-ulp wobble of the fp64 inverse cube.
* folded masses (NB_FLAG_MASS_SCALING): masses in {1, 4, 16}; sigma = m^(-1/2), sigma x, fma(-sigma, x_i, X_j) and
  sigma^2 eps^2 are all exact (given rsq(4^k) = 2^-k), the scaled term is m_j d again and the diagonal self-term exactly 0.

The exact answer is  a_i = u (sum_j m_j k_j - k_i sum_j m_j),  computed in int64 in O(n).

What the construction cannot see: a pair on the SAME site contributes 0 on every axis, so a slip on it is invisible —
``blind_fraction`` measures the share of pairs that are blind in every layout (seed) of a case; and the Quake inverse square
root, which is not 1 at 1.0 (the Quake kernels share the pair enumeration through a template parameter).

``CASES`` is the one table of (n, K, masses, seeds, ...) both lattice test modules read: tests/test_lattice_cpu.py proves the
magnitude bound and the blind cap for every entry, tests/test_lattice_gpu.py runs them.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import nbodysim_amd as nb

LIMIT = 1 << 24          # integers below 2^24 are exact in a float
K_MAX = 512              # |d|^2 <= 2 (K - 1)^2 u^2 < 2^-25 with u = 2^-22
UNIT_F32, UNIT_F64 = -22, -40
BLIND_CAP = 1e-4         # largest share of pairs allowed to be blind in every layout of a case


def pick_K(n: int, m_max: int) -> int:
    """Largest power of two K <= 512 with n (K - 1) m_max < 2^24."""
    K = K_MAX
    while K > 1 and n * (K - 1) * m_max >= LIMIT:
        K //= 2
    assert n * (K - 1) * m_max < LIMIT, (n, K, m_max)
    return K


def lattice_bodies(n: int, K: int, masses, seed: int, dims: int = 2, unit_log2: int = UNIT_F32):
    """(bodies, k, m): n Body records (BODY_DTYPE, or BODY3_DTYPE for dims = 3) at rest with radius 0 on random sites k
    (int64, (n, dims), uniform in [0, K)) scaled by 2^unit_log2, masses m (int64) drawn uniformly from ``masses``."""
    rng = np.random.default_rng([seed, n, K, dims])
    k = rng.integers(0, K, size=(n, dims), dtype=np.int64)
    masses = np.asarray(masses, np.int64)
    m = masses[rng.integers(0, masses.size, size=n)] if masses.size > 1 else np.full(n, masses[0], np.int64)
    b = nb.bodies_array(n)
    if dims == 3:
        b = b.view(nb.BODY3_DTYPE)
    pos = np.ldexp(k.astype(np.float64), unit_log2)
    b["pos"] = pos.astype(np.float32)
    assert np.array_equal(b["pos"].astype(np.float64), pos)          # the sites are exact floats
    b["mass"] = m.astype(np.float32)
    return b, k, m


def exact_units(k: np.ndarray, m: np.ndarray) -> np.ndarray:
    """sum_j m_j (k_j - k_i) per body and axis, int64, in O(n)."""
    k, m = np.asarray(k, np.int64), np.asarray(m, np.int64)
    units = (m[:, None] * k).sum(0)[None, :] - k * m.sum()
    assert np.abs(units).max(initial=0) < LIMIT
    return units


def exact_acc(k: np.ndarray, m: np.ndarray, unit_log2: int = UNIT_F32) -> np.ndarray:
    """The exact accelerations of lattice bodies (eps = 1), float32 (n, dims)."""
    units = exact_units(k, m)
    acc = np.ldexp(units.astype(np.float64), unit_log2)
    out = acc.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), acc)
    return out


def blind_fraction(ks) -> float:
    """Share of the unordered pairs (i, j) that sit on one site in EVERY layout of the list ``ks`` (each (n, dims))."""
    n = ks[0].shape[0]
    if n < 2:
        return 0.0
    key = np.concatenate([np.asarray(k, np.int64) for k in ks], axis=1)
    _, counts = np.unique(key, axis=0, return_counts=True)
    counts = counts.astype(np.int64)
    return float((counts * (counts - 1) // 2).sum()) / (n * (n - 1) / 2)


def seeds_for(K: int, dims: int) -> tuple:
    """Two layouts by default, more where K is small: a pair is blind in one layout with probability K^-dims."""
    s = 2
    while float(K) ** (-dims * s) > 0.25 * BLIND_CAP:
        s += 1
    return tuple(range(1, s + 1))


# ---------------------------------------------------------------------------------------------------------------------
# the shared case table
# ---------------------------------------------------------------------------------------------------------------------
UNIFORM, UNIFORM3, MIXED, MIXED2, POW4, POW4_2, TRACERS = (1,), (3,), (1, 2, 3), (1, 2), (1, 4, 16), (1, 4), (0, 1)

#: group: which GPU test drives the case; kw: Simulation arguments; step: also run one step and check the kick;
#: shard: (protocol, parts) for the in-process sharded drivers
Case = namedtuple("Case", "id group n K masses seeds dims precision unit_log2 kw step shard")


def _case(group, n, masses, dims=2, precision="fp32", step=False, shard=None, tag="", **kw):
    K = pick_K(n, max(max(masses), 1))
    parts = [group, f"n{n}", f"d{dims}", precision, "m" + "_".join(map(str, masses))]
    parts += [f"{a}={v}" for a, v in sorted(kw.items())]
    if shard:
        parts.append(f"{shard[0]}{shard[1]}")
    if step:
        parts.append("step")
    if tag:
        parts.append(tag)
    return Case("-".join(parts), group, n, K, tuple(masses), seeds_for(K, dims), dims, precision,
                UNIT_F64 if precision == "fp64" else UNIT_F32, kw, step, shard)


def _one_sided():
    out = []
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 2049, 5000, 20000, 70001):
        out.append(_case("one_sided", n, UNIFORM, symmetry=False))
        out.append(_case("one_sided", n, MIXED, symmetry=False))
    for n in (5000, 70001):                                   # lane blocking x forced j-slices
        for P in (1, 2, 4):
            for js in (1, 3, 8, 32):
                out.append(_case("one_sided", n, MIXED if (P + js) % 2 else UNIFORM, symmetry=False, lanes_p=P, j_slices=js))
    for n in (513, 20000):                                    # equal masses through the general variant
        out.append(_case("one_sided", n, UNIFORM3, symmetry=False, uniform_mass=False))
    for n in (257, 5000, 20000):                              # folded masses in the LDS-tiled kernel
        out.append(_case("one_sided", n, POW4, symmetry=False, mass_scaling=True))
    out.append(_case("one_sided", 5000, MIXED, symmetry=False, step=True))
    return out


def _sym_f32():
    out = []
    mass_kw = {"uniform": (UNIFORM, {}), "mixed": (MIXED, {}), "pow4": (POW4, {"mass_scaling": True})}

    def pick(n, mode):
        masses, kw = mass_kw[mode]
        if n >= 262144:                                       # keep K at 32 / 16 there: {1, 2} and {1, 4}
            masses = {"mixed": MIXED2, "pow4": POW4_2}.get(mode, masses)
        return masses, dict(kw)
    # every size with the library's own plan, all three mass modes
    for n in (5631, 5632, 5633, 9300, 12288, 16383, 16384, 20000, 49151, 49152, 65536, 70001, 262144):
        for mode in ("uniform", "mixed", "pow4"):
            masses, kw = pick(n, mode)
            out.append(_case("sym_f32", n, masses, **kw))
    # the full cross of the plan axes at two sizes (tile 512 below / above its automatic range, tile 2048 likewise)
    for n in (20000, 70001):
        i = 0
        for tile in (0, 512, 2048):
            for pairs in (-1, 1):
                for chunks in (0, 1, 3, 5, 8):
                    for tail in (True, False):
                        for static in (False, True):
                            masses, kw = pick(n, ("uniform", "mixed", "pow4")[i % 3])
                            i += 1
                            out.append(_case("sym_f32", n, masses, sym_tile=tile, sym_chunk_pairs=pairs, sym_chunks_per_item=chunks,
                                             guided_tail=tail, static_items=static, **kw))
    # the other sizes: every axis value again, one at a time and in a few combinations
    for n, kws in (
        (5632, [dict(sym_chunk_pairs=1), dict(sym_chunks_per_item=3, sym_chunk_pairs=1), dict(guided_tail=False), dict(static_items=True)]),
        (9300, [dict(sym_chunk_pairs=1, sym_chunks_per_item=5), dict(sym_tail=(0.3, 0.5, 0.7)), dict(sym_chunks_per_item=1)]),
        (16384, [dict(sym_tile=2048), dict(sym_tile=2048, sym_chunk_pairs=1, sym_chunks_per_item=3), dict(sym_tile=512, sym_chunks_per_item=8)]),
        (49151, [dict(sym_tile=2048, guided_tail=False), dict(sym_chunk_pairs=1, sym_chunks_per_item=5)]),
        (49152, [dict(sym_tile=512), dict(sym_tile=512, sym_chunk_pairs=1, static_items=True), dict(sym_chunk_pairs=-1)]),
        (65536, [dict(sym_chunk_pairs=-1, sym_chunks_per_item=3), dict(sym_tail=(0.5, 0.7, 0.9), sym_chunks_per_item=8), dict(guided_tail=False)]),
        (262144, [dict(sym_tile=512), dict(sym_chunk_pairs=-1), dict(guided_tail=False, static_items=True), dict(sym_chunks_per_item=5)]),
    ):
        for j, kw in enumerate(kws):
            for mode in (("uniform", "mixed", "pow4")[j % 3], ("mixed", "pow4", "uniform")[j % 3]):
                masses, mkw = pick(n, mode)
                out.append(_case("sym_f32", n, masses, **kw, **mkw))
    for n in (20000, 70001):                                  # mass 0 on (about) every other body: tracers feel, do not exert
        out.append(_case("sym_f32", n, TRACERS))
    for n in (20000, 70001):                                  # equal masses through the general variant
        out.append(_case("sym_f32", n, UNIFORM3, uniform_mass=False))
    out.append(_case("sym_f32", 20000, UNIFORM, step=True))
    out.append(_case("sym_f32", 20000, POW4, mass_scaling=True, step=True))
    out.append(_case("sym_f32", 70001, MIXED, step=True, sym_chunk_pairs=-1))
    out.append(_case("sym_f32", 262144, MIXED2, step=True))
    return out


def _fp64():
    out = []
    for n in (1000, 20000, 70001, 262144):
        for masses in (UNIFORM, MIXED if n < 262144 else MIXED2):
            for symm in (True, False):
                out.append(_case("fp64", n, masses, precision="fp64", symmetry=symm))
    out.append(_case("fp64", 20000, MIXED, precision="fp64", step=True))
    return out


def _three_d():
    out = []
    for precision in ("fp32", "fp64"):
        for n in (1000, 5000, 20000, 70001, 262144):
            for masses in (UNIFORM, MIXED if n < 262144 else MIXED2):
                out.append(_case("3d", n, masses, dims=3, precision=precision, symmetry=False))
                if precision == "fp64":
                    out.append(_case("3d", n, masses, dims=3, precision=precision))
                else:
                    for pairs in (-1, 1):
                        out.append(_case("3d", n, masses, dims=3, precision=precision, sym_chunk_pairs=pairs))
    out.append(_case("3d", 20000, MIXED, dims=3, step=True))
    return out


def _full_size():
    return [_case("full", 1 << 20, UNIFORM)]


def _sharded():
    out = []
    for parts in (2, 3, 8):
        out.append(_case("sharded", 6000, MIXED, shard=("allgather", parts)))
    out.append(_case("sharded", 70001, MIXED, shard=("allgather", 3)))
    out.append(_case("sharded", 6000, UNIFORM, shard=("allgather", 3)))
    for parts in (2, 4):
        for late in (-1.0, 40.0):
            for aux in (-1, 1):
                out.append(_case("sharded", 131072, MIXED if aux > 0 else UNIFORM, shard=("symmetric", parts), sym_late_us=late, sym_aux_stream=aux))
    out.append(_case("sharded", 262144, MIXED2, shard=("symmetric", 8)))
    out.append(_case("sharded", 262144, UNIFORM, shard=("symmetric", 8)))
    for precision in ("fp32", "fp64"):
        for masses in (UNIFORM, MIXED):
            out.append(_case("sharded", 131072, masses, precision=precision, shard=("allreduce", 4)))
    out.append(_case("sharded", 131072, MIXED, dims=3, shard=("allreduce", 4)))
    for allreduce in (False, True):
        out.append(_case("sharded", 70001, MIXED, shard=("single", 1), shard_allreduce=allreduce))
        out.append(_case("sharded", 131072, UNIFORM, shard=("single", 1), shard_allreduce=allreduce, sym_late_us=40.0, sym_aux_stream=1))
    return out


CASES = _one_sided() + _sym_f32() + _fp64() + _three_d() + _full_size() + _sharded()
assert len({c.id for c in CASES}) == len(CASES), "case ids must be unique"


def cases(group: str):
    return [c for c in CASES if c.group == group]


def layouts(c: Case):
    """(seed, bodies, k, m) for every layout of a case."""
    for seed in c.seeds:
        b, k, m = lattice_bodies(c.n, c.K, c.masses, seed, c.dims, c.unit_log2)
        yield seed, b, k, m
