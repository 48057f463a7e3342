#!/usr/bin/env python3
"""Does the ORDER in which the symmetric force kernel sees the bodies move its launch time?  (not part of the product)

One process, one device.  Three handles of the same system (fp32, exact rsqrt, eps = 0.01):

  --mode ceiling (what the order can be worth; every handle sweeps in the caller's order, NB_FLAG_NO_BODY_ORDER)
    A   plummer_2d(n, 42) as generated (i.i.d. draws in index order)
    B   the same bodies permuted on the host into Morton order (16 bits per axis of (pos - lo) / (hi - lo), ties by index)
    A'  a second handle of A's bodies: the A/A' difference is what two handles of the SAME bodies differ by
  --mode ab (what the library's own order is worth; the bodies as generated on every handle, dt = 1e-3 as in bench.py)
    A   NB_FLAG_NO_BODY_ORDER          B   the library's default          A'  NB_FLAG_NO_BODY_ORDER again
    P   (--old-lib FILE) a handle of another build of the library, e.g. the parent commit's: the off-path must cost nothing

in interleaved rounds (the clock a part holds drifts within a call): after `--warm` seconds of steps, `--rounds` rounds of
`--steps` steps per handle, the order of the handles rotating from round to round.  Per round and handle the mean duration of
the force launch from nb_profile_read (the kernel alone: the sort and the copy of the positions are outside it; --wall adds
the wall time per step of every stretch, which holds them).  In ceiling mode dt is small (1e-5) so that B's bodies stay in
their order over the whole run.

    python tools/body_order_ab.py [--mode ceiling|ab] [--n 262144] [--rounds 8] [--steps 200] [--warm 2.0] [--general] [--dump DIR]
                                  [--old-lib FILE] [--wall]

`--dump DIR` also writes DIR/pos_A_<n>.f32x2 and DIR/pos_B_<n>.f32x2 (raw float2 records) for tools/sym_timeline.hip, whose
last argument reads them: the in-kernel shader clock of the two orders.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import nbodysim_amd as nb  # noqa: E402

EPS = 0.01


def spread_bits(v):
    """16 bits -> every other bit of 32."""
    v = v.astype(np.uint32)
    v = (v | (v << 8)) & np.uint32(0x00FF00FF)
    v = (v | (v << 4)) & np.uint32(0x0F0F0F0F)
    v = (v | (v << 2)) & np.uint32(0x33333333)
    v = (v | (v << 1)) & np.uint32(0x55555555)
    return v


def morton_order(pos):
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    ext = np.where(hi > lo, hi - lo, np.float32(1.0))
    q = np.minimum(((pos - lo) / ext * np.float32(65536.0)).astype(np.int64), 65535)
    key = spread_bits(q[:, 0]) | (spread_bits(q[:, 1]) << 1)
    return np.argsort(key, kind="stable")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warm", type=float, default=2.0)
    ap.add_argument("--general", action="store_true", help="individual masses (uniform_mass=False)")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--mode", default="ceiling", choices=["ceiling", "ab"])
    ap.add_argument("--old-lib", default=None, help="ab mode: a fourth handle P on this build of the library")
    ap.add_argument("--wall", action="store_true", help="also the wall time per step of every stretch")
    args = ap.parse_args()
    DT = 1e-5 if args.mode == "ceiling" else 1e-3

    a = nb.plummer_2d(args.n, 42)
    b = a[morton_order(a["pos"])].copy()
    if args.dump:
        Path(args.dump).mkdir(parents=True, exist_ok=True)
        np.ascontiguousarray(a["pos"], dtype=np.float32).tofile(Path(args.dump) / f"pos_A_{args.n}.f32x2")
        np.ascontiguousarray(b["pos"], dtype=np.float32).tofile(Path(args.dump) / f"pos_B_{args.n}.f32x2")
    kw = dict(eps=EPS, device=0, uniform_mass=not args.general)
    names = ["A", "B", "A'"]
    if args.mode == "ceiling":
        sims = [nb.Simulation(x, body_order=False, **kw) for x in (a, b, a)]
    else:
        sims = [nb.Simulation(a, body_order=o, **kw) for o in (False, None, False)]
        if args.old_lib:
            from nbodysim_amd import _lib as L
            old = L.bind(args.old_lib, {k: v for k, v in L.PROTOTYPES.items() if k != "nb_body_order"})
            names.append("P")
            sims.append(nb.Simulation(a, library=old, **kw))
    print("  ".join(f"{k}: {s.describe().split('CUs=')[1].split('|')[0].strip()}" for k, s in zip(names, sims)))
    print(f"n={args.n} general={int(args.general)} rounds={args.rounds} steps={args.steps} | {sims[0].describe()}", flush=True)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.warm:
        for s in sims:
            s.advance(20, DT)
        for s in sims:
            s.wait()
    per = {k: [] for k in names}
    wall = {k: [] for k in names}
    for r in range(args.rounds):
        for j in range(len(sims)):
            k = (j + r) % len(sims)
            s = sims[k]
            s.profile(True)
            t1 = time.perf_counter()
            s.advance(args.steps, DT)
            s.wait()
            wall[names[k]].append((time.perf_counter() - t1) / args.steps * 1e6)
            ms, cnt = s.profile_read()
            s.profile(False)
            per[names[k]].append(ms / cnt * 1e3)
        print(f"round {r + 1:2d}: " + "  ".join(f"{k} {per[k][-1]:9.2f} us" for k in names), flush=True)
    med = {k: float(np.median(per[k])) for k in names}
    mn = {k: float(np.min(per[k])) for k in names}
    aa = abs(med["A'"] - med["A"]) / med["A"]
    aa_rounds = max(abs(x - y) / x for x, y in zip(per["A"], per["A'"]))
    gain = (med["A"] - med["B"]) / med["A"]
    print("median us: " + "  ".join(f"{k} {med[k]:.2f}" for k in names) + " | min us: " + "  ".join(f"{k} {mn[k]:.2f}" for k in names))
    print(f"A/A' spread of the round medians {aa * 100:.3f} % (largest A/A' difference within one round {aa_rounds * 100:.3f} %) | "
          f"B below A by {gain * 100:+.3f} % of A's median")
    ok = gain > 2.0 * aa and gain >= 0.014
    print(f"gate (gain > 2 x spread and gain >= 1.4 %): {'PASS' if ok else 'FAIL'}", flush=True)
    if "P" in per:
        print(f"A against P (the other build): {(med['A'] - med['P']) / med['P'] * 100:+.3f} % of P's median launch time")
    if args.wall:                         # with profiling on, every launch is bracketed by events: a little above an unprofiled step
        wm = {k: float(np.median(wall[k])) for k in names}
        print("wall us per step, median of the stretches: " + "  ".join(f"{k} {wm[k]:.2f}" for k in names) +
              f" | B below A by {(wm['A'] - wm['B']) / wm['A'] * 100:+.3f} %")
    for s in sims:
        s.close()


if __name__ == "__main__":
    main()
