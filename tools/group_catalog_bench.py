"""Cost of the group catalogue: nb_group_catalog beside the two things it replaces, on one GPU, from one process.

    python tools/group_catalog_bench.py [--out FILE] [--limit SECONDS] [case ...]
        cases: d262144, d1048576 (Plummer spheres on direct-sum handles, eps 0.01, dt 1e-3), t8388608 (the same on a convergent tree
        handle: leaves, theta 0.5), and the two extremes of the reduction at min_members 1: single1048576 (a 1024 x 1024 unit lattice
        at radius 0.5: every body a group of its own) and one1048576 (the same lattice at radius 1.1: ALL bodies in ONE group);
        all five by default

Protocol (that of tools/groups_bench.py, whose radius search it uses): every handle first steps for at least 2 s (settled clocks); per
Plummer handle three radii for a mean of 1, 5 and 30 links per body, min_members 2; per row one untimed call (the first call allocates)
and FIVE timed stretches of back-to-back calls under the host clock; a row reports the five per-call figures, their median and their
spread (max - min).  Per handle and radius, in the same run:
    nb_group_catalog, both calls of the binding's route apart: the count query (grouping, sort by label, heads, scan: no reduction)
        and the filling call into nb_host_alloc memory and into a pageable array, beside it the device time of pass A + pass B with
        their carry launches (nb_profile_read: events around them)
    (a) nb_groups(label, size) into nb_host_alloc memory: what the grouping alone costs; and nb_groups(ngroups) alone, so that
        count query - nb_groups(ngroups) is what the sort by label, the heads and the scan cost
    (b) the host route: nb_groups(label) + nb_sync into pageable arrays + numpy bincount with weights (count, m, m x, m y, m vx, m vy;
        one thread)
One JSON line per row, appended to FILE (default profiles/group_catalog_bench.log) and printed.  The process ends itself after --limit
seconds (default 900).
"""
from __future__ import annotations

import ctypes as C
import json
import signal
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import nbodysim_amd as nb  # noqa: E402
import numpy as np  # noqa: E402
from nbodysim_amd import _lib as L  # noqa: E402

from groups_bench import find_radius, kernel_ms  # noqa: E402
from neighbors_bench import Pinned  # noqa: E402
from raster_bench import timed_row  # noqa: E402
from tree_bench import settle, stats_of  # noqa: E402

DT = 1e-3
TARGETS = (1.0, 5.0, 30.0)


def open_case(case: str):
    for prefix, radius in (("single", 0.5), ("one", 1.1)):
        if case.startswith(prefix):
            n = int(case[len(prefix):])
            side = int(round(n ** 0.5))
            assert side * side == n
            b = nb.bodies_array(n)
            gx, gy = np.meshgrid(np.arange(side, dtype=np.float32) - side / 2, np.arange(side, dtype=np.float32) - side / 2)
            order = np.random.default_rng(1).permutation(n)
            b["pos"][:, 0], b["pos"][:, 1] = gx.ravel()[order], gy.ravel()[order]
            b["mass"] = 1.0 / n
            return nb.Simulation(b, eps=0.01, device=0), n, radius
    n = int(case[1:])
    kw = dict(force="tree", theta=0.5, tree_leaves=True) if case[0] == "t" else {}
    return nb.Simulation(nb.plummer_2d(n, 42), rsqrt="exact", eps=0.01, device=0, **kw), n, None


def host_route(sim, lib, n: int, radius: float, row: dict) -> None:
    label, bodies = np.zeros(n, np.uint32), nb.bodies_array(n)

    def once():
        t0 = time.perf_counter()
        L.check("nb_groups", lib.nb_groups(sim._h, radius, label.ctypes.data, None, None), lib)
        t1 = time.perf_counter()
        L.check("nb_sync", lib.nb_sync(sim._h, bodies.ctypes.data), lib)
        t2 = time.perf_counter()
        m = bodies["mass"].astype(np.float64)
        sums = [np.bincount(label, minlength=n), np.bincount(label, weights=m, minlength=n)]
        for f in ("pos", "vel"):
            for d in range(2):
                sums.append(np.bincount(label, weights=m * bodies[f][:, d], minlength=n))
        t3 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3
    once()
    v = [once() for _ in range(5)]
    for k, name in enumerate(("groups_label_ms", "sync_ms", "bincount_ms", "total_ms")):
        stats_of(name, [a[k] for a in v], row)
    row["threads"] = 1


def run(case: str, emit) -> None:
    lib = nb.load()
    sim, n, fixed = open_case(case)
    with sim:
        settle(sim, DT)
        radii = [(fixed, None)] if fixed else [find_radius(sim, lib, n, t) for t in TARGETS]
        min_members = 1 if fixed else 2
        count, ngroups = C.c_size_t(0), C.c_uint64(0)
        pins = [Pinned(lib, n), Pinned(lib, n)]
        rec_pin, rec_cap = None, 0
        try:
            for radius, mean_count in radii:
                base = {"case": case, "n": n, "radius": radius, "mean_count": None if mean_count is None else round(mean_count, 2),
                        "min_members": min_members}
                got = sim.group_catalog(radius, min_members)
                groups = int(got.shape[0])
                emit(dict(base, groups=groups, largest=int(got["members"].max()) if groups else 0,
                          bodies_in_catalogue=int(got["members"].sum(dtype=np.uint64))))
                if groups > rec_cap:
                    if rec_pin:
                        rec_pin.close()
                    rec_pin, rec_cap = Pinned(lib, groups * 20), groups
                pageable = np.zeros(max(groups, 1), L.GROUP_DTYPE)
                rows = (("count query", "none", (None, 0)), ("records", "nb_host_alloc", (rec_pin.ptr, groups)),
                        ("records", "pageable", (pageable.ctypes.data, groups)))
                for what, dest, args in rows:
                    def call():
                        L.check("nb_group_catalog", lib.nb_group_catalog(sim._h, radius, min_members, *args, C.byref(count)), lib)
                    row = dict(base, call="nb_group_catalog", outputs=what, dest=dest)
                    sim.profile(False)
                    timed_row(call, row)
                    if what == "records" and groups:
                        kernel_ms(sim, call, row["calls_per_stretch"], row, "passes_ms")
                    emit(row)
                for what, args in (("label size", (pins[0].ptr, pins[1].ptr, None)), ("ngroups", (None, None, C.byref(ngroups)))):
                    def grouping():
                        L.check("nb_groups", lib.nb_groups(sim._h, radius, *args), lib)
                    row = dict(base, call="nb_groups", outputs=what, dest="nb_host_alloc" if what != "ngroups" else "none")
                    timed_row(grouping, row)
                    emit(row)
                row = dict(base, call="host route: nb_groups(label) + nb_sync + numpy bincount with weights", runs=5)
                host_route(sim, lib, n, radius, row)
                emit(row)
        finally:
            for p in pins + ([rec_pin] if rec_pin else []):
                p.close()


def main(argv) -> int:
    args = list(argv)
    out, limit = ROOT / "profiles" / "group_catalog_bench.log", 900
    if "--out" in args:
        out = Path(args.pop(args.index("--out") + 1))
        args.remove("--out")
    if "--limit" in args:
        limit = int(args.pop(args.index("--limit") + 1))
        args.remove("--limit")
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"group_catalog_bench: the time limit of {limit} s ran out"))
    signal.alarm(limit)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a") as log:
        def emit(row: dict) -> None:
            line = json.dumps(row)
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
        lib_path = Path(nb.load()._name).resolve()
        emit({"tool": "group_catalog_bench", "library": str(lib_path.relative_to(ROOT) if ROOT in lib_path.parents else lib_path.name)})
        for case in args or ["d262144", "d1048576", "t8388608", "single1048576", "one1048576"]:
            run(case, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
