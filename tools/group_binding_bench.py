"""Cost of unbinding on the device: nb_group_binding beside its yardsticks, on one GPU, from one process.

    python tools/group_binding_bench.py [--out FILE] [--limit SECONDS] [case ...]
        cases: d262144, d1048576 (Plummer spheres on direct-sum handles, eps 0.01, dt 1e-3), t8388608 (the same on a convergent tree
        handle: leaves, theta 0.5); the yardsticks of the sweep, handles whose bodies are ALL one group: cell16384 (16 384 bodies
        inside one cell) and one262144 (a 512 x 512 unit lattice at radius 1.1); and the opposite extreme, pairs1048576 (a 1024 x 1024
        lattice whose columns stand 0.6 and 1.4 apart in turn: radius 0.5 makes every body a singleton, radius 0.7 makes 524 288
        pairs; min_members 1); all six by default

Protocol (that of tools/group_catalog_bench.py, whose radius search it uses): every handle first steps for at least 2 s (settled
clocks); per Plummer handle three radii for a mean of 1, 5 and 31 links per body, min_members 2; per row one untimed call (the first
call allocates) and FIVE timed stretches of back-to-back calls under the host clock; a row reports the five per-call figures, their
median and their spread (max - min).  Per handle and radius, in the same run:
    the catalogue's members, from which sum n_g^2 over the kept groups: the lane-pairs the sweep owes.  A row whose sum exceeds 2e12
        is SKIPPED and says so (at nb_potentials' 6.7e12 pairs/s that is 0.3 s a call);
    nb_group_binding(e, out) into nb_host_alloc memory and into pageable arrays, and the count query; beside the first the device
        time of the sweep alone (nb_profile_read: events around it) and sum n_g^2 / that time, pairs per second;
    nb_group_catalog's filling call into nb_host_alloc memory, for scale;
    on the one-group handles nb_potentials' direct sweep from device events on the same handle: the same pairs, the same pair body;
        the ratio binding sweep / potentials sweep is what the segment bookkeeping and the two boundary tiles cost;
    at d262144 and the radius of a mean of 1 link only (where no group is large), the host route it replaces, once: nb_groups' labels,
        nb_sync, and numpy per group (a k x k distance matrix in float64, one thread).
One JSON line per row, appended to FILE (default profiles/group_binding_bench.log) and printed.  The process ends itself after --limit
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
TARGETS = (1.0, 5.0, 31.0)
PAIR_LIMIT = 2e12


def lattice(side: int, pitch=None):
    gx, gy = np.meshgrid(np.arange(side, dtype=np.float32), np.arange(side, dtype=np.float32))
    if pitch:                                                     # columns 0.6 and 1.4 apart in turn
        gx = 2.0 * (gx // 2) + np.float32(pitch) * (gx % 2)
    n = side * side
    b = nb.bodies_array(n)
    order = np.random.default_rng(1).permutation(n)
    b["pos"][:, 0], b["pos"][:, 1] = gx.ravel()[order] - side / 2, gy.ravel()[order] - side / 2
    b["mass"] = 1.0 / n
    return b


def open_case(case: str):
    """(handle, n, [(radius, min_members)] or None)"""
    if case.startswith("cell"):
        n = int(case[4:])
        b = nb.bodies_array(n)
        b["pos"] = np.random.default_rng(1).uniform(-0.3, 0.3, (n, 2)).astype(np.float32)
        b["mass"] = 1.0 / n
        return nb.Simulation(b, eps=0.01, device=0), n, [(1.0, 1)]
    if case.startswith("one"):
        n = int(case[3:])
        return nb.Simulation(lattice(int(round(n ** 0.5))), eps=0.01, device=0), n, [(1.1, 1)]
    if case.startswith("pairs"):
        n = int(case[5:])
        return nb.Simulation(lattice(int(round(n ** 0.5)), 0.6), eps=0.01, device=0), n, [(0.5, 1), (0.7, 1)]
    n = int(case[1:])
    kw = dict(force="tree", theta=0.5, tree_leaves=True) if case[0] == "t" else {}
    return nb.Simulation(nb.plummer_2d(n, 42), rsqrt="exact", eps=0.01, device=0, **kw), n, None


def host_route(sim, lib, n: int, radius: float, eps: float, row: dict) -> None:
    label, bodies = np.zeros(n, np.uint32), nb.bodies_array(n)
    t0 = time.perf_counter()
    L.check("nb_groups", lib.nb_groups(sim._h, radius, label.ctypes.data, None, None), lib)
    t1 = time.perf_counter()
    L.check("nb_sync", lib.nb_sync(sim._h, bodies.ctypes.data), lib)
    t2 = time.perf_counter()
    order = np.argsort(label, kind="stable")
    heads = np.flatnonzero(np.r_[True, label[order][1:] != label[order][:-1]])
    ends = np.r_[heads[1:], n]
    x, v, m = bodies["pos"].astype(np.float64), bodies["vel"].astype(np.float64), bodies["mass"].astype(np.float64)
    e = np.full(n, np.nan)
    for h, t in zip(heads, ends):
        if t - h < 2:
            continue
        idx = order[h:t]
        d = x[idx][:, None, :] - x[idx][None, :, :]
        inv = 1.0 / np.sqrt((d * d).sum(axis=2) + eps * eps)
        np.fill_diagonal(inv, 0.0)
        dv = v[idx] - (m[idx, None] * v[idx]).sum(axis=0) / m[idx].sum()
        e[idx] = 0.5 * (dv * dv).sum(axis=1) - inv @ m[idx]
    t3 = time.perf_counter()
    row.update(groups_label_ms=round((t1 - t0) * 1e3, 3), sync_ms=round((t2 - t1) * 1e3, 3), numpy_ms=round((t3 - t2) * 1e3, 3),
               total_ms=round((t3 - t0) * 1e3, 3), threads=1, runs=1)


def run(case: str, emit) -> None:
    lib = nb.load()
    sim, n, fixed = open_case(case)
    with sim:
        settle(sim, DT)
        rows = [(r, None, mm) for r, mm in fixed] if fixed else [find_radius(sim, lib, n, t) + (2,) for t in TARGETS]
        count = C.c_size_t(0)
        e_pin, phi_pin = Pinned(lib, 2 * n), Pinned(lib, 2 * n)
        rec_pin, rec_cap = None, 0
        try:
            for k, (radius, mean_count, min_members) in enumerate(rows):
                base = {"case": case, "n": n, "radius": radius, "mean_count": None if mean_count is None else round(mean_count, 2),
                        "min_members": min_members}
                cat = sim.group_catalog(radius, min_members)
                groups = int(cat.shape[0])
                members = cat["members"].astype(np.float64)
                pairs = float((members * members).sum())
                emit(dict(base, groups=groups, largest=int(cat["members"].max()) if groups else 0, sum_ng2=pairs))
                if pairs > PAIR_LIMIT:
                    emit(dict(base, skipped=f"sum n_g^2 = {pairs:.3g} exceeds {PAIR_LIMIT:.0e}: the sweep would take more than 0.3 s a call"))
                    continue
                if not groups:
                    continue
                if groups > rec_cap:
                    if rec_pin:
                        rec_pin.close()
                    rec_pin, rec_cap = Pinned(lib, groups * 20), groups
                pe, prec = np.zeros(n), np.zeros(max(groups, 1), L.GROUP_ENERGY_DTYPE)
                for what, dest, args in (("count query", "none", (None, None, None, 0)),
                                         ("e records", "nb_host_alloc", (None, e_pin.ptr, rec_pin.ptr, groups)),
                                         ("e records", "pageable", (None, pe.ctypes.data, prec.ctypes.data, groups))):
                    def call():
                        L.check("nb_group_binding", lib.nb_group_binding(sim._h, radius, min_members, *args, C.byref(count)), lib)
                    row = dict(base, call="nb_group_binding", outputs=what, dest=dest)
                    sim.profile(False)
                    timed_row(call, row)
                    if dest == "nb_host_alloc" and groups:
                        kernel_ms(sim, call, row["calls_per_stretch"], row, "sweep_ms")
                        row["pairs_per_s"] = float(f"{pairs / (row['sweep_ms_median'] * 1e-3):.4g}")
                    emit(row)

                def catalogue():
                    L.check("nb_group_catalog", lib.nb_group_catalog(sim._h, radius, min_members, rec_pin.ptr, groups, C.byref(count)), lib)
                row = dict(base, call="nb_group_catalog", outputs="records", dest="nb_host_alloc")
                timed_row(catalogue, row)
                emit(row)
                if fixed and not case.startswith("pairs"):                # all bodies one group: nb_potentials' sweep, the same pairs
                    def potentials():
                        L.check("nb_potentials", lib.nb_potentials(sim._h, phi_pin.ptr), lib)
                    row = dict(base, call="nb_potentials", dest="nb_host_alloc", pairs=float(n) * n)
                    timed_row(potentials, row)
                    kernel_ms(sim, potentials, row["calls_per_stretch"], row, "sweep_ms")
                    row["pairs_per_s"] = float(f"{float(n) * n / (row['sweep_ms_median'] * 1e-3):.4g}")
                    emit(row)
                if case == "d262144" and k == 0:
                    row = dict(base, call="host route: nb_groups(label) + nb_sync + numpy per group (k x k, float64)")
                    host_route(sim, lib, n, radius, 0.01, row)
                    emit(row)
        finally:
            for p in (e_pin, phi_pin) + ((rec_pin,) if rec_pin else ()):
                p.close()


def main(argv) -> int:
    args = list(argv)
    out, limit = ROOT / "profiles" / "group_binding_bench.log", 900
    if "--out" in args:
        out = Path(args.pop(args.index("--out") + 1))
        args.remove("--out")
    if "--limit" in args:
        limit = int(args.pop(args.index("--limit") + 1))
        args.remove("--limit")
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"group_binding_bench: the time limit of {limit} s ran out"))
    signal.alarm(limit)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a") as log:
        def emit(row: dict) -> None:
            line = json.dumps(row)
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
        lib_path = Path(nb.load()._name).resolve()
        emit({"tool": "group_binding_bench", "library": str(lib_path.relative_to(ROOT) if ROOT in lib_path.parents else lib_path.name)})
        for case in args or ["d262144", "d1048576", "t8388608", "cell16384", "one262144", "pairs1048576"]:
            run(case, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
