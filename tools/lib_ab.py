#!/usr/bin/env python3
"""A previous build of the library against the current one, alternating, on one box: the same workloads stepped through both,
final bodies compared bit for bit (sha256 of pos | vel | acc) and timed.  For changes that must not alter a single sum.

    git worktree add /tmp/old <commit> && make -C /tmp/old/nbodysim_amd/csrc && cp /tmp/old/nbodysim_amd/libnbody_hip.so build/old_lib/
    python tools/lib_ab.py --old build/old_lib/libnbody_hip.so [--cases p9216,p16384,ref25000,...]

A case is [MODS-]BASE<n>.  BASE: p 2-D fp32, d 2-D fp64, q 3-D fp32, qd 3-D fp64, ref the reference start.  MODS, letters
in any order: o one-sided (symmetry=False), g eps = 0 (the guarded body, one-sided), k rsqrt="quake", s mass scaling in the
individual-masses run (uniform_mass=False, mass_scaling=True), c collisions (extras |= NB_EXTRA_COLLIDE, on the ref base: its bodies
have radii); the Barnes-Hut force: t force="tree" at theta = 0.5, l tree_leaves=True,
u tree_quadrupole=True, r tree_alpha=0.02, e tree_energy=True (the hash then also covers the two doubles of energy() read after the
steps); the symmetric sweep: x sym_chunk_pairs=1 (the chunk-pair sweep, below the size that switches it on), y sym_chunks_per_item=3
(an odd chunk count: with x, the last pair of an item is half empty).  Example: og-qd4096, os-p65536, c-ref25000, tlur-p4096,
kxy-q16421.  A combination Simulation rejects ends the run with its message.

(the Python binding loads $NBODY_HIP_LIB when set — the LIBRARY reads no environment variables; each side runs in a child process)

When the current binding declares an entry point the old library does not have yet (it refuses to bind a library that lacks a
declared symbol), give the old side its own binding too: --old-pkg DIR, a directory holding the old commit's `nbodysim_amd` package
with its library inside (cp -r /tmp/old/nbodysim_amd build/old_pkg/); --old is then not used.
"""
import argparse
import hashlib
import json
import os
import struct
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def child(cases, steps, pkg=None):
    if pkg:
        sys.path.insert(0, str(Path(pkg).resolve()))
    import nbodysim_amd as nb
    out = {}
    for name in cases:
        mods, _, base = name.rpartition("-")
        if base.startswith("ref"):
            ic, kw, dt = nb.default_ics(int(base[3:])), dict(eps=1.0, extras=3), 0.01
        elif base.startswith("qd"):                  # 3-D fp64
            ic, kw, dt = nb.plummer_3d(int(base[2:]), 42), dict(eps=0.01, dims=3, precision="fp64"), 1e-3
        elif base.startswith("q"):                   # 3-D
            ic, kw, dt = nb.plummer_3d(int(base[1:]), 42), dict(eps=0.01, dims=3), 1e-3
        elif base.startswith("d"):                   # fp64
            ic, kw, dt = nb.plummer_2d(int(base[1:]), 42), dict(eps=0.01, precision="fp64"), 1e-3
        else:
            ic, kw, dt = nb.plummer_2d(int(base[1:]), 42), dict(eps=0.01), 1e-3
        if "o" in mods:
            kw["symmetry"] = False
        if "g" in mods:
            kw["eps"] = 0.0
        if "k" in mods:
            kw["rsqrt"] = "quake"
        if "c" in mods:
            kw["extras"] = kw.get("extras", 0) | 4   # NB_EXTRA_COLLIDE
        if "t" in mods:
            kw.update(force="tree", theta=0.5)
        if "l" in mods:
            kw["tree_leaves"] = True
        if "u" in mods:
            kw["tree_quadrupole"] = True
        if "r" in mods:
            kw["tree_alpha"] = 0.02
        if "e" in mods:
            kw["tree_energy"] = True
        if "x" in mods:
            kw["sym_chunk_pairs"] = 1
        if "y" in mods:
            kw["sym_chunks_per_item"] = 3
        for general in (False, True):
            k = dict(kw)
            if general:
                k["uniform_mass"] = False
                if "s" in mods:
                    k["mass_scaling"] = True
            try:
                sim = nb.Simulation(ic, **k)
            except ValueError as err:                # a combination of letters it rejects
                sys.exit(f"{name}: {err}")
            with sim as s:
                s.advance(30, dt)
                s.wait()
                t0 = time.perf_counter()
                s.advance(steps, dt)
                s.wait()
                el = (time.perf_counter() - t0) / steps
                b = s.sync()
                data = b"".join(np.ascontiguousarray(b[f]).tobytes() for f in ("pos", "vel", "acc"))
                if "e" in mods:
                    data += struct.pack("dd", *s.energy())
                h = hashlib.sha256(data).hexdigest()
            out[f"{name}/{'individual' if general else 'equal'} masses"] = (h, el * 1e6)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=str(ROOT / "build" / "old_lib" / "libnbody_hip.so"))
    ap.add_argument("--cases", default="p9216,p16384,ref25000,p32768,p65536,p131072")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--old-pkg", default=None)
    ap.add_argument("--pkg", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    cases = args.cases.split(",")
    if args.child:
        child(cases, args.steps, args.pkg)
        return
    res = {}
    for tag, lib in (("old", args.old), ("new", None), ("old2", args.old), ("new2", None)):
        env = dict(os.environ)
        env.pop("NBODY_HIP_LIB", None)
        extra = []
        if lib and args.old_pkg:
            extra = ["--pkg", args.old_pkg]
        elif lib:
            env["NBODY_HIP_LIB"] = str(Path(lib).resolve())
        r = subprocess.run([sys.executable, __file__, "--child", "--cases", args.cases, "--steps", str(args.steps), *extra], env=env, capture_output=True, text=True, timeout=600)
        if r.returncode:
            print(tag, r.stderr[-2000:])
            sys.exit(1)
        res[tag] = json.loads(r.stdout.strip().splitlines()[-1])
    for k in res["old"]:
        o, n = res["old"][k][1] + res["old2"][k][1], res["new"][k][1] + res["new2"][k][1]
        print(f"{k:28s} same bits {res['old'][k][0] == res['new'][k][0]} | old {res['old'][k][1]:8.1f} {res['old2'][k][1]:8.1f} us/step | "
              f"new {res['new'][k][1]:8.1f} {res['new2'][k][1]:8.1f} us/step ({(n / o - 1) * 100:+.1f} %)")


if __name__ == "__main__":
    main()
