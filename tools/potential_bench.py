"""Cost of the per-body potential: nb_potentials beside the one-sided force launch and nb_energy, on one GPU, from one process.

    python tools/potential_bench.py [--out FILE] [--limit SECONDS] [case ...]
        cases: d262144, d1048576 (Plummer spheres, fp32 2-D direct sum, NB_FLAG_NO_SYMMETRY so that the step's force launch is the
        one-sided force_tiled_f32; eps 0.01, dt 1e-3) and t1048576, t8388608 (the same bodies on NB_FLAG_TREE_LEAVES |
        NB_FLAG_TREE_ENERGY handles at theta 0.5); all four by default

Protocol (that of tools/raster_bench.py and tools/tree_bench.py): every handle first steps for at least 2 s (settled clocks); then,
per row, one untimed call (the first call allocates) and FIVE timed stretches of back-to-back calls under the host clock; a row
reports the five per-call figures, their median and their spread (max - min).  Rows per direct case: nb_potentials into a pageable
numpy array and into an nb_host_alloc block, beside the first the device time of the sweep alone (nb_profile_read: events around
potential_tiled_f32); the one-sided force launch alone (nb_profile_read around nb_accelerations); nb_energy; the sweep alone on
handles whose nb_params.lanes_p forces 1, 2 and 4 particle pairs per lane (the library's own choice is in the first row's handle).
Rows per tree case:
nb_potentials into a pageable array with the device time of its two walk kernels, and nb_energy.  One JSON line per row, appended
to FILE (default profiles/potential_bench.log) and printed; then per direct case the expectation of DESIGN.md: the sweep takes no
longer than the force launch (medians and the larger spread).  The process ends itself after --limit seconds (default 900).
"""
from __future__ import annotations

import ctypes as C
import json
import signal
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import nbodysim_amd as nb  # noqa: E402
import numpy as np  # noqa: E402
from nbodysim_amd import _lib as L  # noqa: E402

from raster_bench import timed_row  # noqa: E402
from tree_bench import settle, stats_of  # noqa: E402

DT = 1e-3


def open_case(case: str):
    n = int(case[1:])
    kw = dict(force="tree", theta=0.5, tree_leaves=True, tree_energy=True) if case[0] == "t" else dict(symmetry=False)
    return nb.Simulation(nb.plummer_2d(n, 42), rsqrt="exact", eps=0.01, device=0, **kw), n


def profiled(sim, call, row: dict, name: str) -> None:
    """The device time per bracketed launch of `call`, five stretches of row['calls_per_stretch'] calls."""
    sim.profile(True)
    sim.profile_read()
    v = []
    for _ in range(5):
        for _ in range(row["calls_per_stretch"]):
            call()
        sim.wait()
        ms, launches = sim.profile_read()
        v.append(ms / launches)
    sim.profile(False)
    stats_of(name, v, row)


def run(case: str, emit) -> None:
    lib = nb.load()
    sim, n = open_case(case)
    with sim:
        settle(sim, DT)
        describe = sim.describe()
        phi = np.zeros(n, np.float64)

        def potentials(dst=phi):
            L.check("nb_potentials", lib.nb_potentials(sim._h, dst.ctypes.data), lib)
        row = {"case": case, "n": n, "call": "nb_potentials", "destination": "pageable", "bytes": n * 8, "handle": describe}
        timed_row(potentials, row)
        profiled(sim, potentials, row, "sweep_ms" if case[0] == "d" else "walk_ms")
        row["phi_min"], row["phi_median"] = float(phi.min()), float(np.median(phi))
        emit(row)
        sweep = row
        if case[0] == "d":
            ptr = lib.nb_host_alloc(n * 8)
            if not ptr:
                raise L.NBodyError("nb_host_alloc", L.last_error_code(lib), L.last_error(lib))
            try:
                pinned = np.frombuffer((C.c_uint8 * (n * 8)).from_address(ptr), dtype=np.float64)
                row = {"case": case, "n": n, "call": "nb_potentials", "destination": "nb_host_alloc", "bytes": n * 8}
                timed_row(lambda: potentials(pinned), row)
                row["same_bits_as_pageable"] = bool(np.array_equal(pinned.view(np.uint64), phi.view(np.uint64)))
                emit(row)
                del pinned
            finally:
                L.check("nb_host_free", lib.nb_host_free(ptr), lib)

            def force():
                L.check("nb_accelerations", lib.nb_accelerations(sim._h), lib)
            row = {"case": case, "n": n, "call": "nb_accelerations", "what": "the one-sided force launch (force_tiled_f32) alone"}
            force()
            sim.wait()
            row["calls_per_stretch"] = sweep["calls_per_stretch"]
            profiled(sim, force, row, "force_ms")
            emit(row)
            margin = max(sweep["sweep_ms_spread"], row["force_ms_spread"])
            bar = {"case": case, "n": n, "expectation": "the potential sweep takes no longer than the one-sided force launch",
                   "sweep_ms": sweep["sweep_ms_median"], "force_ms": row["force_ms_median"], "larger_spread_ms": margin,
                   "met": bool(sweep["sweep_ms_median"] <= row["force_ms_median"] + margin)}
        k, u = C.c_double(), C.c_double()
        row = {"case": case, "n": n, "call": "nb_energy"}
        timed_row(lambda: L.check("nb_energy", lib.nb_energy(sim._h, C.byref(k), C.byref(u)), lib), row)
        row["potential"] = u.value
        mass = sim.bodies["mass"].astype(np.float64)
        row["half_sum_m_phi"] = float(0.5 * np.sum(mass * phi))
        emit(row)
        if case[0] == "d":
            emit(bar)
    if case[0] == "d":                                       # the sweep alone with the particles per lane forced (same bits, other geometry)
        for lanes in (1, 2, 4):
            with nb.Simulation(nb.plummer_2d(n, 42), rsqrt="exact", eps=0.01, device=0, symmetry=False, lanes_p=lanes) as forced:
                forced.potentials(out=phi)
                row = {"case": case, "n": n, "call": "nb_potentials", "lanes_p": lanes, "calls_per_stretch": sweep["calls_per_stretch"]}
                profiled(forced, lambda: L.check("nb_potentials", lib.nb_potentials(forced._h, phi.ctypes.data), lib), row, "sweep_ms")
                emit(row)


def main(argv) -> int:
    args = list(argv)
    out, limit = ROOT / "profiles" / "potential_bench.log", 900
    if "--out" in args:
        out = Path(args.pop(args.index("--out") + 1))
        args.remove("--out")
    if "--limit" in args:
        limit = int(args.pop(args.index("--limit") + 1))
        args.remove("--limit")
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"potential_bench: the time limit of {limit} s ran out"))
    signal.alarm(limit)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a") as log:
        def emit(row: dict) -> None:
            line = json.dumps(row)
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
        lib_path = Path(nb.load()._name).resolve()
        emit({"tool": "potential_bench", "library": str(lib_path.relative_to(ROOT) if ROOT in lib_path.parents else lib_path.name)})
        for case in args or ["d262144", "d1048576", "t1048576", "t8388608"]:
            run(case, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
