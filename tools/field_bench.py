"""Cost of the field at arbitrary points: nb_field beside nb_potentials' sweep and the one-sided force launch, on one GPU, from one
process.

    python tools/field_bench.py [--out FILE] [--limit SECONDS] [case ...]
        cases: d262144, d1048576 (Plummer spheres, fp32 2-D direct sum, NB_FLAG_NO_SYMMETRY so that the step's force launch is the
        one-sided force_tiled_f32; eps 0.01, dt 1e-3; npoints = n, the points uniform in the half-mass square) and t1048576,
        t8388608 (the same bodies on NB_FLAG_TREE_LEAVES | NB_FLAG_TREE_ENERGY handles at theta 0.5; a 1024 x 1024 row-major grid over
        the half-mass square, and the same points shuffled); all four by default

Protocol (that of tools/potential_bench.py): every handle first steps for at least 2 s (settled clocks); then, per row, one untimed
call (the first call allocates) and FIVE timed stretches of back-to-back calls under the host clock; a row reports the five per-call
figures, their median and their spread (max - min).  Rows per direct case: nb_field for phi only, acc only and both into pageable
numpy arrays, beside each the device time of the sweep alone (nb_profile_read: events around field_tiled_f32), and both into an
nb_host_alloc block; then the yardsticks on the same handle, nb_potentials' sweep and the one-sided force launch, device time.  Rows
per tree case: both planes for the grid and for the shuffled grid, with the device time of the walk kernel; the shuffled row shows
what incoherence costs the per-lane walk.  One JSON line per row, appended to FILE (default profiles/field_bench.log) and printed;
then per direct case the one condition of DESIGN.md: the joint sweep takes no longer than nb_potentials' sweep plus the one-sided
force launch for the same number of pairs (medians, with a margin of the larger of the two spreads).  The process ends itself after
--limit seconds (default 900).
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

from potential_bench import open_case, profiled  # noqa: E402
from raster_bench import timed_row  # noqa: E402
from tree_bench import settle  # noqa: E402

DT = 1e-3
GRID = 1024


def half_mass_square(sim) -> float:
    """Half the side of the origin-centred square that holds half the bodies' mass."""
    b = sim.sync()
    r = np.abs(b["pos"]).max(1)
    order = np.argsort(r)
    cum = np.cumsum(b["mass"][order].astype(np.float64))
    return float(r[order][np.searchsorted(cum, 0.5 * cum[-1])])


def run(case: str, emit) -> None:
    lib = nb.load()
    sim, n = open_case(case)
    rng = np.random.default_rng(7)
    with sim:
        settle(sim, DT)
        describe = sim.describe()
        half = half_mass_square(sim)
        if case[0] == "d":
            layouts = {"uniform": rng.uniform(-half, half, (n, 2)).astype(np.float32)}
        else:
            c = ((np.arange(GRID) + 0.5) / GRID * 2.0 - 1.0) * half
            grid = np.stack(np.meshgrid(c, c, indexing="xy"), -1).reshape(-1, 2).astype(np.float32)
            layouts = {"grid_row_major": grid, "grid_shuffled": grid[rng.permutation(grid.shape[0])]}
        rows = {}
        for layout, pts in layouts.items():
            k = pts.shape[0]
            phi, acc = np.zeros(k, np.float64), np.zeros((k, 2), np.float64)
            for planes in (("phi", "acc", "both") if case[0] == "d" else ("both",)):
                f = phi.ctypes.data if planes != "acc" else None
                a = acc.ctypes.data if planes != "phi" else None

                def call(f=f, a=a):
                    L.check("nb_field", lib.nb_field(sim._h, pts.ctypes.data, k, f, a), lib)
                row = {"case": case, "n": n, "call": "nb_field", "points": layout, "npoints": k, "planes": planes, "destination": "pageable",
                       "bytes": k * 8 * ((planes != "acc") + 2 * (planes != "phi")), "handle": describe}
                timed_row(call, row)
                profiled(sim, call, row, "sweep_ms" if case[0] == "d" else "walk_ms")
                emit(row)
                rows[planes] = row
            emit({"case": case, "points": layout, "phi_median": float(np.median(phi)), "acc_rms": float(np.sqrt((acc * acc).sum(1).mean())),
                  "finite": bool(np.isfinite(phi).all() and np.isfinite(acc).all())})
        if case[0] != "d":
            return
        pts = layouts["uniform"]
        ptr = lib.nb_host_alloc(n * 24)
        if not ptr:
            raise L.NBodyError("nb_host_alloc", L.last_error_code(lib), L.last_error(lib))
        try:
            pinned = np.frombuffer((C.c_uint8 * (n * 24)).from_address(ptr), dtype=np.float64)
            row = {"case": case, "n": n, "call": "nb_field", "points": "uniform", "npoints": n, "planes": "both", "destination": "nb_host_alloc",
                   "bytes": n * 24}
            timed_row(lambda: L.check("nb_field", lib.nb_field(sim._h, pts.ctypes.data, n, pinned[:n].ctypes.data, pinned[n:].ctypes.data), lib), row)
            row["same_bits_as_pageable"] = bool(np.array_equal(pinned[:n].view(np.uint64), phi.view(np.uint64))
                                                and np.array_equal(pinned[n:].view(np.uint64), acc.reshape(-1).view(np.uint64)))
            emit(row)
            del pinned
        finally:
            L.check("nb_host_free", lib.nb_host_free(ptr), lib)
        # the yardsticks: the fallback a caller already has, on the same handle, for the same n x n pairs
        both = rows["both"]
        own = np.zeros(n, np.float64)
        pot = {"case": case, "n": n, "call": "nb_potentials", "what": "the potential sweep (potential_tiled_f32) alone",
               "calls_per_stretch": both["calls_per_stretch"]}
        sim.potentials(out=own)
        profiled(sim, lambda: L.check("nb_potentials", lib.nb_potentials(sim._h, own.ctypes.data), lib), pot, "sweep_ms")
        emit(pot)
        force = {"case": case, "n": n, "call": "nb_accelerations", "what": "the one-sided force launch (force_tiled_f32) alone",
                 "calls_per_stretch": both["calls_per_stretch"]}
        L.check("nb_accelerations", lib.nb_accelerations(sim._h), lib)
        sim.wait()
        profiled(sim, lambda: L.check("nb_accelerations", lib.nb_accelerations(sim._h), lib), force, "force_ms")
        emit(force)
        fallback = pot["sweep_ms_median"] + force["force_ms_median"]
        margin = max(both["sweep_ms_spread"], pot["sweep_ms_spread"], force["force_ms_spread"])
        emit({"case": case, "n": n, "condition": "the joint field sweep takes no longer than the potential sweep plus the one-sided force launch",
              "field_both_ms": both["sweep_ms_median"], "potentials_plus_force_ms": round(fallback, 4), "larger_spread_ms": round(margin, 4),
              "met": bool(both["sweep_ms_median"] <= fallback + margin)})


def main(argv) -> int:
    args = list(argv)
    out, limit = ROOT / "profiles" / "field_bench.log", 900
    if "--out" in args:
        out = Path(args.pop(args.index("--out") + 1))
        args.remove("--out")
    if "--limit" in args:
        limit = int(args.pop(args.index("--limit") + 1))
        args.remove("--limit")
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"field_bench: the time limit of {limit} s ran out"))
    signal.alarm(limit)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a") as log:
        def emit(row: dict) -> None:
            line = json.dumps(row)
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
        lib_path = Path(nb.load()._name).resolve()
        emit({"tool": "field_bench", "library": str(lib_path.relative_to(ROOT) if ROOT in lib_path.parents else lib_path.name)})
        for case in args or ["d262144", "d1048576", "t1048576", "t8388608"]:
            run(case, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
