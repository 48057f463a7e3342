"""Cost of a step with the Barnes-Hut force (NB_FORCE_TREE) beside the direct sum, on one GPU, from one process.

    python tools/tree_bench.py [case ...]      cases: default (the reference's 25 000 bodies, eps 1, dt 0.01, clamp + boundary),
                                               262144, 1048576, 8388608 (Plummer spheres, eps 0.01, dt 1e-3); all by default

Per case: the tree with the reference's arithmetic (quake) and with the hardware rsqrt (exact) and, up to 1 048 576 bodies, the
direct default beside it.  Every handle first steps for at least 2 s (settled clocks), then a stretch of steps is timed between
two waits.  Prints one JSON line per case: milliseconds per step, the walk's share (nb_profile_read), nodes and depth of the
last build, and direct / tree.

    rocprofv3 --kernel-trace --stats -- python tools/tree_bench.py --trace CASE      50 tree steps alone: microseconds per kernel

    python tools/tree_bench.py --theta T [--leaves] [case ...]      the walk alone, hardware rsqrt, opening parameter T, with
                                               --leaves the convergent force (NB_FLAG_TREE_LEAVES); cases 262144 and 1048576 by default

    python tools/tree_bench.py --theta T --leaves --quad [case ...]  the same with the quadrupole term (NB_FLAG_TREE_QUADRUPOLE)
    python tools/tree_bench.py --sweep [case ...]                   the convergent force at theta 1.0, 0.7, 0.5, 0.3, each without and
                                               with the quadrupole term: one line per (case, theta, quad), then per case the
                                               equal-accuracy pairs (for each monopole theta the largest quadrupole theta whose
                                               median error is no worse)

    python tools/tree_bench.py --theta T --leaves [--quad] --alpha A [case ...]   the same with the acceleration-relative opening test
                                               (NB_FLAG_TREE_RELATIVE, nb_tree_alpha): theta is the cap, A is alpha
    python tools/tree_bench.py --sweep --alpha [case ...]           the theta rows of --sweep and, under theta = 1, alpha 0.02, 0.005, 0.0025,
                                               0.001, each without and with the quadrupole term; then per (case, quad) and theta the
                                               largest alpha whose 99th-percentile error is no worse than that theta's, with both
                                               walk and step times and their spreads side by side

    python tools/tree_bench.py --energy [case ...]                  nb_energy on a convergent tree handle (theta 0.5, without and with the
                                               quadrupole term): with NB_FLAG_TREE_ENERGY (the tree walk; cases 262144, 1048576 and
                                               8388608 by default) and, up to 1 048 576 bodies, without it (the direct fp64 pair
                                               sweep).  Every handle first steps for at least 2 s, then FIVE calls are timed (host
                                               clock around the call, which waits for its result): one JSON line per (case, quad,
                                               form) with the five figures, their median and spread (max - min), then per case the
                                               ratio direct / tree.  Up to 1 048 576 bodies also |U_tree - U_direct| / |U_direct| of
                                               the initial bodies at theta 1.0, 0.7, 0.5, 0.3, without and with the quadrupole term.

    python tools/tree_bench.py --nodes [case ...]                   nb_tree_nodes on the reference's arithmetic (quake, theta 1; cases default and
                                               262144 by default).  The handle first steps for at least 2 s; five stretches give the
                                               step and the walk (build = step - walk: the tree build, the integration and the launch
                                               gaps).  Then, into a page-locked (nb_host_alloc) and into a pageable (numpy) destination,
                                               FIVE times: one step, a wait, then the call under the host clock; its kernels come from
                                               nb_profile_read (device events around the export kernels), copy = call - kernels (the
                                               synchronisation, the DMA and, for a pageable destination, the host copy out of the
                                               staging buffer).  nb_sync into a pageable array is timed the same way for the bytes it
                                               moves, and a frame of the drop-in's step() (nb_step, nb_sync) without and with the two
                                               nb_tree_nodes calls of its NBODY_TREE_NODES build (count query, then the records into a
                                               vector that is reused).  One JSON line per case: five figures each, median and spread.

With --theta the handle steps for at least 2 s, then FIVE stretches are timed; per stretch the milliseconds per step (host clock
between two waits) and the milliseconds per walk (nb_profile_read, device events around the walk).  One JSON line per case: the
five figures of each, their median and spread (max - min), and the walk nb_describe names.  With --leaves the line also carries
the median, the 99th percentile and the maximum of the per-body error of the INITIAL accelerations, |a - a_direct| / |a_direct|,
against a direct-sum handle (hardware rsqrt) on the same bodies; with --alpha it is the error of the SECOND evaluation there
(fresh bodies have no previous acceleration: the first evaluation is the plain theta walk and the second one uses its result).  A library built from another commit is measured through NBODY_HIP_LIB
(the cases without --leaves need nothing this tool adds).
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import nbodysim_amd as nb  # noqa: E402
import numpy as np  # noqa: E402


def settle(sim, dt: float, warm_s: float = 2.0) -> float:
    """Step for at least warm_s seconds; returns the seconds one step takes."""
    sim.advance(2, dt)
    sim.wait()
    t0 = time.perf_counter()
    sim.advance(3, dt)
    sim.wait()
    est = max((time.perf_counter() - t0) / 3, 1e-5)
    left = warm_s
    while left > 0:                                          # in pieces: the queue stays short
        k = max(1, min(int(0.25 / est), 2000))
        sim.advance(k, dt)
        sim.wait()
        left -= k * est
    return est


def settled_ms(sim, dt: float, warm_s: float = 2.0, timed_s: float = 1.0) -> float:
    est = settle(sim, dt, warm_s)
    k = max(3, min(int(timed_s / est), 5000))
    t0 = time.perf_counter()
    sim.advance(k, dt)
    sim.wait()
    return (time.perf_counter() - t0) / k * 1e3


def direct_accelerations(case: str):
    """The initial accelerations of the case's bodies from a direct-sum handle (hardware rsqrt), as float64."""
    with nb.Simulation(nb.plummer_2d(int(case), 42), rsqrt="exact", eps=0.01, device=0) as sim:
        return sim.accelerations().astype("float64")


def run_walk(case: str, theta: float, leaves: bool, stretches: int = 5, timed_s: float = 1.0, quad: bool = False, direct=None,
             alpha=None) -> dict:
    bodies, dt = nb.plummer_2d(int(case), 42), 1e-3
    kw = dict(tree_leaves=True) if leaves else {}
    if quad:
        kw["tree_quadrupole"] = True
    if alpha is not None:
        kw["tree_alpha"] = alpha
    with nb.Simulation(bodies, force="tree", rsqrt="exact", theta=theta, eps=0.01, device=0, **kw) as sim:
        d = sim.describe()
        out = {"case": case, "n": int(bodies.shape[0]), "theta": theta, "leaves": int(leaves), "quad": int(quad),
               "walk": d.split(" walk=")[1].split()[0] if " walk=" in d else "lane"}
        if alpha is not None:
            out["alpha"] = alpha
        if direct is not None:
            if alpha is not None:
                sim.accelerations()                          # (the criterion is active from the second evaluation on)
            a = sim.accelerations().astype("float64")
            mag = (direct[:, 0] ** 2 + direct[:, 1] ** 2) ** 0.5
            err = sorted(((a[:, 0] - direct[:, 0]) ** 2 + (a[:, 1] - direct[:, 1]) ** 2) ** 0.5 / mag)
            out["err_median"], out["err_p99"] = float(f"{err[len(err) // 2]:.3e}"), float(f"{err[len(err) * 99 // 100]:.3e}")
            out["err_max"] = float(f"{err[-1]:.3e}")
        est = settle(sim, dt)
        k = max(3, min(int(timed_s / est), 5000))
        step_ms, walk_ms = [], []
        sim.profile(True)
        sim.profile_read()
        for _ in range(stretches):
            t0 = time.perf_counter()
            sim.advance(k, dt)
            sim.wait()
            step_ms.append((time.perf_counter() - t0) / k * 1e3)
            ms, launches = sim.profile_read()
            walk_ms.append(ms / launches)
        out["steps_per_stretch"] = k
        for name, v in (("walk_ms", walk_ms), ("step_ms", step_ms)):
            out[name] = [round(a, 4) for a in v]
            out[name + "_median"] = round(sorted(v)[len(v) // 2], 4)
            out[name + "_spread"] = round(max(v) - min(v), 4)
        out.update(sim.tree_stats())
    return out


def run(case: str) -> dict:
    if case == "default":
        bodies, kw, dt = nb.default_ics(25000), dict(eps=1.0, extras=3), 0.01
        bodies["radius"] = 0.0
    else:
        bodies, kw, dt = nb.plummer_2d(int(case), 42), dict(eps=0.01), 1e-3
    out = {"case": case, "n": int(bodies.shape[0])}
    for mode in ("quake", "exact"):
        with nb.Simulation(bodies, force="tree", rsqrt=mode, device=0, **kw) as sim:
            out[f"tree_{mode}_ms"] = round(settled_ms(sim, dt), 4)
            sim.profile(True)
            sim.advance(20, dt)
            ms, launches = sim.profile_read()
            out[f"tree_{mode}_walk_ms"] = round(ms / launches, 4)
            out.update(sim.tree_stats())
    if out["n"] <= 1 << 20:
        with nb.Simulation(bodies, device=0, **kw) as sim:
            out["direct_ms"] = round(settled_ms(sim, dt), 4)
        out["direct_over_tree_quake"] = round(out["direct_ms"] / out["tree_quake_ms"], 2)
        out["direct_over_tree_exact"] = round(out["direct_ms"] / out["tree_exact_ms"], 2)
    return out


def trace(case: str, steps: int = 50) -> None:
    """A short run of the tree step alone (the reference's arithmetic), for `rocprofv3 --kernel-trace --stats -- python
    tools/tree_bench.py --trace CASE`: the stats file then holds the time of every tree_* kernel and of rocPRIM's."""
    if case == "default":
        bodies, kw, dt = nb.default_ics(25000), dict(eps=1.0, extras=3), 0.01
        bodies["radius"] = 0.0
    else:
        bodies, kw, dt = nb.plummer_2d(int(case), 42), dict(eps=0.01), 1e-3
    with nb.Simulation(bodies, force="tree", rsqrt="quake", device=0, **kw) as sim:
        sim.advance(steps, dt)
        sim.wait()
    print(json.dumps({"case": case, "traced_steps": steps}))


def sweep(cases, thetas=(1.0, 0.7, 0.5, 0.3), alphas=()) -> None:
    for c in cases:
        direct = direct_accelerations(c)
        rows = {}
        for theta in thetas:
            for quad in (False, True):
                rows[theta, quad] = run_walk(c, theta, True, quad=quad, direct=direct)
                print(json.dumps(rows[theta, quad]), flush=True)
        rel = {}
        for alpha in alphas:                                 # the relative criterion under the theta = 1 cap
            for quad in (False, True):
                rel[alpha, quad] = run_walk(c, 1.0, True, quad=quad, direct=direct, alpha=alpha)
                print(json.dumps(rel[alpha, quad]), flush=True)
        for quad in (False, True) if alphas else ():         # equal tail: the largest alpha whose 99th percentile is no worse
            for theta in thetas:
                base = rows[theta, quad]
                ok = [a for a in alphas if rel[a, quad]["err_p99"] <= base["err_p99"]]
                if not ok:
                    print(json.dumps({"case": c, "quad": int(quad), "equal_tail": {"theta": theta, "alpha": None}}), flush=True)
                    continue
                r = rel[max(ok), quad]
                print(json.dumps({"case": c, "quad": int(quad), "equal_tail": {"theta": theta, "alpha": max(ok)},
                                  "err_p99": [base["err_p99"], r["err_p99"]], "err_max": [base["err_max"], r["err_max"]],
                                  "walk_ms": [base["walk_ms_median"], r["walk_ms_median"]], "step_ms": [base["step_ms_median"], r["step_ms_median"]],
                                  "walk_ms_spread": [base["walk_ms_spread"], r["walk_ms_spread"]],
                                  "step_ms_spread": [base["step_ms_spread"], r["step_ms_spread"]]}), flush=True)
        for theta in thetas:                                 # equal accuracy: the largest quadrupole theta that is no worse
            mono = rows[theta, False]
            ok = [t for t in thetas if rows[t, True]["err_median"] <= mono["err_median"]]
            if not ok:
                continue
            q = rows[max(ok), True]
            print(json.dumps({"case": c, "equal_accuracy": {"monopole_theta": theta, "quadrupole_theta": max(ok)},
                              "err_median": [mono["err_median"], q["err_median"]],
                              "walk_ms": [mono["walk_ms_median"], q["walk_ms_median"]], "step_ms": [mono["step_ms_median"], q["step_ms_median"]],
                              "walk_ms_spread": [mono["walk_ms_spread"], q["walk_ms_spread"]],
                              "step_ms_spread": [mono["step_ms_spread"], q["step_ms_spread"]]}), flush=True)


def energy_calls(sim, dt: float, calls: int = 5) -> dict:
    settle(sim, dt)
    ms = []
    for _ in range(calls):
        sim.wait()
        t0 = time.perf_counter()
        k, u = sim.energy()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"energy_ms": [round(a, 4) for a in ms], "energy_ms_median": round(sorted(ms)[len(ms) // 2], 4),
            "energy_ms_spread": round(max(ms) - min(ms), 4), "K": k, "U": u}


def energy(cases, theta: float = 0.5, thetas=(1.0, 0.7, 0.5, 0.3)) -> None:
    dt = 1e-3
    for c in cases:
        bodies = nb.plummer_2d(int(c), 42)
        n = int(bodies.shape[0])
        kw = dict(force="tree", rsqrt="exact", eps=0.01, device=0, tree_leaves=True)
        if n <= 1 << 20:                                     # accuracy at the initial positions, before anything steps
            with nb.Simulation(bodies, theta=theta, **kw) as sim:
                u_direct = sim.energy()[1]
            for t in thetas:
                for quad in (False, True):
                    with nb.Simulation(bodies, theta=t, tree_quadrupole=quad, tree_energy=True, **kw) as sim:
                        u = sim.energy()[1]
                    print(json.dumps({"case": c, "n": n, "theta": t, "quad": int(quad), "U_tree": u, "U_direct": u_direct,
                                      "rel_err": float(f"{abs(u - u_direct) / abs(u_direct):.3e}")}), flush=True)
        rows = {}
        for quad in (False, True):
            for flag in (True, False):
                if not flag and n > 1 << 20:
                    continue
                with nb.Simulation(bodies, theta=theta, tree_quadrupole=quad, tree_energy=flag, **kw) as sim:
                    row = {"case": c, "n": n, "theta": theta, "quad": int(quad), "energy": "tree" if flag else "direct"}
                    row.update(energy_calls(sim, dt))
                    if flag:
                        row.update(sim.tree_stats())
                rows[quad, flag] = row
                print(json.dumps(row), flush=True)
        for quad in (False, True):
            if (quad, False) in rows:
                t, d = rows[quad, True], rows[quad, False]
                print(json.dumps({"case": c, "quad": int(quad), "direct_over_tree": round(d["energy_ms_median"] / t["energy_ms_median"], 2),
                                  "energy_ms": [d["energy_ms_median"], t["energy_ms_median"]],
                                  "energy_ms_spread": [d["energy_ms_spread"], t["energy_ms_spread"]]}), flush=True)


def five(f, calls: int = 5):
    return [f() for _ in range(calls)]


def stats_of(name: str, v, out: dict) -> None:
    out[name] = [round(a, 4) for a in v]
    out[name + "_median"] = round(sorted(v)[len(v) // 2], 4)
    out[name + "_spread"] = round(max(v) - min(v), 4)


def nodes(case: str, timed_s: float = 1.0) -> dict:
    import ctypes as C
    from nbodysim_amd import _lib as L
    if case == "default":
        bodies, kw, dt = nb.default_ics(25000), dict(eps=1.0, extras=3), 0.01
        bodies["radius"] = 0.0
    else:
        bodies, kw, dt = nb.plummer_2d(int(case), 42), dict(eps=0.01), 1e-3
    lib = nb.load()
    out = {"case": case, "n": int(bodies.shape[0])}
    with nb.Simulation(bodies, force="tree", rsqrt="quake", device=0, **kw) as sim:
        est = settle(sim, dt)
        k = max(3, min(int(timed_s / est), 5000))
        step_ms, walk_ms = [], []
        sim.profile(True)
        sim.profile_read()
        for _ in range(5):
            t0 = time.perf_counter()
            sim.advance(k, dt)
            sim.wait()
            step_ms.append((time.perf_counter() - t0) / k * 1e3)
            ms, launches = sim.profile_read()
            walk_ms.append(ms / launches)
        stats_of("step_ms", step_ms, out)
        stats_of("walk_ms", walk_ms, out)
        out["build_ms_median"] = round(out["step_ms_median"] - out["walk_ms_median"], 4)
        out.update(sim.tree_stats())
        count = out["nodes"]
        room = count + count // 4 + 4096                    # the tree grows a little while the bodies move
        out["node_bytes"] = count * L.NODE_DTYPE.itemsize
        ptr = lib.nb_host_alloc(room * L.NODE_DTYPE.itemsize)
        assert ptr, L.last_error(lib)
        pinned = np.frombuffer((C.c_uint8 * (room * L.NODE_DTYPE.itemsize)).from_address(ptr), dtype=L.NODE_DTYPE)
        pageable = L.nodes_array(room)
        try:
            for name, dst in (("pinned", pinned), ("pageable", pageable)):
                sim.tree_nodes(out=dst)                     # the first call allocates the scratch (and, pageable, the staging)
                call, kern = [], []
                for _ in range(5):
                    sim.advance(1, dt)
                    sim.wait()
                    sim.profile_read()
                    t0 = time.perf_counter()
                    sim.tree_nodes(out=dst)
                    call.append((time.perf_counter() - t0) * 1e3)
                    kern.append(sim.profile_read()[0])
                stats_of(f"nodes_{name}_call_ms", call, out)
                stats_of(f"nodes_{name}_kernels_ms", kern, out)
                stats_of(f"nodes_{name}_copy_ms", [a - b for a, b in zip(call, kern)], out)
        finally:
            del pinned
            lib.nb_host_free(ptr)
        sim.profile(False)

        def timed(f):
            def one():
                sim.advance(1, dt)
                sim.wait()
                t0 = time.perf_counter()
                f()
                return (time.perf_counter() - t0) * 1e3
            return one
        sim.sync()
        stats_of("sync_pageable_ms", five(timed(sim.sync)), out)
        out["sync_bytes"] = int(bodies.shape[0]) * 64

        def frame(with_nodes: bool):
            def one():
                t0 = time.perf_counter()
                sim.step(dt)
                if with_nodes:
                    sim.tree_nodes(out=pageable)
                return (time.perf_counter() - t0) * 1e3
            return one
        for with_nodes, name in ((False, "frame_ms"), (True, "frame_with_nodes_ms")):
            five(frame(with_nodes))
            v = [sum(five(frame(with_nodes), 20)) / 20 for _ in range(5)]
            stats_of(name, v, out)
    return out


if __name__ == "__main__":
    if sys.argv[1:2] == ["--nodes"]:
        for c in sys.argv[2:] or ["default", "262144"]:
            print(json.dumps(nodes(c)), flush=True)
        sys.exit(0)
    if sys.argv[1:2] == ["--energy"]:
        energy(sys.argv[2:] or ["262144", "1048576", "8388608"])
        sys.exit(0)
    if sys.argv[1:2] == ["--trace"]:
        trace(sys.argv[2])
        sys.exit(0)
    if sys.argv[1:2] == ["--sweep"]:
        args = sys.argv[2:]
        relative = "--alpha" in args
        if relative:
            args.remove("--alpha")
        sweep(args or ["262144", "1048576"], alphas=(0.02, 0.005, 0.0025, 0.001) if relative else ())
        sys.exit(0)
    if "--theta" in sys.argv:
        args = sys.argv[1:]
        theta = float(args.pop(args.index("--theta") + 1))
        args.remove("--theta")
        alpha = None
        if "--alpha" in args:
            alpha = float(args.pop(args.index("--alpha") + 1))
            args.remove("--alpha")
        leaves, quad = "--leaves" in args, "--quad" in args
        for flag in ("--leaves", "--quad"):
            if flag in args:
                args.remove(flag)
        for c in args or ["262144", "1048576"]:
            print(json.dumps(run_walk(c, theta, leaves, quad=quad, direct=direct_accelerations(c) if leaves else None, alpha=alpha)), flush=True)
        sys.exit(0)
    for c in sys.argv[1:] or ["default", "262144", "1048576", "8388608"]:
        print(json.dumps(run(c)), flush=True)
