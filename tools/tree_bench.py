"""Cost of a step with the Barnes-Hut force (NB_FORCE_TREE) beside the direct sum, on one GPU, from one process.

    python tools/tree_bench.py [case ...]      cases: default (the reference's 25 000 bodies, eps 1, dt 0.01, clamp + boundary),
                                               262144, 1048576, 8388608 (Plummer spheres, eps 0.01, dt 1e-3); all by default

Per case: the tree with the reference's arithmetic (quake) and with the hardware rsqrt (exact) and, up to 1 048 576 bodies, the
direct default beside it.  Every handle first steps for at least 2 s (settled clocks), then a stretch of steps is timed between
two waits.  Prints one JSON line per case: milliseconds per step, the walk's share (nb_profile_read), nodes and depth of the
last build, and direct / tree.

    rocprofv3 --kernel-trace --stats -- python tools/tree_bench.py --trace CASE      50 tree steps alone: microseconds per kernel
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import nbodysim_amd as nb  # noqa: E402


def settled_ms(sim, dt: float, warm_s: float = 2.0, timed_s: float = 1.0) -> float:
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
    k = max(3, min(int(timed_s / est), 5000))
    t0 = time.perf_counter()
    sim.advance(k, dt)
    sim.wait()
    return (time.perf_counter() - t0) / k * 1e3


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


if __name__ == "__main__":
    if sys.argv[1:2] == ["--trace"]:
        trace(sys.argv[2])
        sys.exit(0)
    for c in sys.argv[1:] or ["default", "262144", "1048576", "8388608"]:
        print(json.dumps(run(c)), flush=True)
