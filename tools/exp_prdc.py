"""Timing of prdc_device (csrc/prdc.hip) next to the blocked torch fp64 route, in one process on one GPU.

    python tools/exp_prdc.py --out profiles/prdc_mi355x.json

Per shape (n = m rows of width d, k = 5; reals randn, fakes randn shifted by 0.5 / sqrt(d)): prdc_device(route="hip") and
prdc_device(route="torch") on the same tensors.  One warm-up each, then five alternating repeats, every call bracketed by
device synchronisation; median and spread (max - min) in milliseconds.  The rule for slow shapes: where the torch warm-up
took more than SLOW_MS, the shape gets --slow_repeats alternating repeats (each entry records its own count and the warm-up
time that decided it), so one run of the tool reproduces the committed file.  `faster_by_more_than_the_spread` is the bar of
DESIGN.md: torch median - hip median > torch spread + hip spread.  The four figures of the two routes are recorded too
(they agree wherever no key is within rounding of a threshold)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(10000, 16), (10000, 256), (10000, 512), (50000, 16), (50000, 256), (50000, 512)]
K = 5
REPEATS = 5
SLOW_MS = 10000.0          # a torch call slower than this: --slow_repeats for the shape
FIGURES = ("precision", "recall", "density", "coverage")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    return {"median_ms": float(np.median(ms)), "spread_ms": float(max(ms) - min(ms)), "runs_ms": [float(x) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/prdc_mi355x.json")
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--slow_repeats", type=int, default=REPEATS, help=f"repeats of a shape whose torch warm-up took over {SLOW_MS:.0f} ms")
    ap.add_argument("--shapes", default=None, help="n:d,n:d,... instead of the built-in list")
    args = ap.parse_args()
    from vqvae_amd._device import device
    from vqvae_amd.eval.prdc import prdc_device
    dev = device()
    shapes = SHAPES if args.shapes is None else [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
    results = {"device": torch.cuda.get_device_name(dev), "k": K, "repeats": args.repeats, "slow_repeats": args.slow_repeats,
               "slow_ms": SLOW_MS, "shapes": []}
    for n, d in shapes:
        g = torch.Generator(device="cpu").manual_seed(n + d)
        real = torch.randn(n, d, generator=g).to(dev)
        fake = (torch.randn(n, d, generator=g) + 0.5 / d ** 0.5).to(dev)
        runs = {"hip": lambda: prdc_device(real, fake, K, route="hip"), "torch": lambda: prdc_device(real, fake, K, route="torch")}
        figures, warm = {}, {}
        for name, fn in runs.items():                              # warm-up: workspace allocation, code object load
            warm[name], res = timed(fn)
            figures[name] = {f: res[f] for f in FIGURES}
        repeats = args.slow_repeats if warm["torch"] > SLOW_MS else args.repeats
        ms = {name: [] for name in runs}
        for _ in range(repeats):                                   # alternating
            for name, fn in runs.items():
                ms[name].append(timed(fn)[0])
        entry = {"n": n, "m": n, "d": d, "repeats": repeats, "torch_warmup_ms": float(warm["torch"]), "hip": stats(ms["hip"]), "torch_fp64_blocked": stats(ms["torch"]), "figures": figures,
                 "figures_equal": figures["hip"] == figures["torch"]}
        gain = entry["torch_fp64_blocked"]["median_ms"] - entry["hip"]["median_ms"]
        entry["torch_over_hip"] = entry["torch_fp64_blocked"]["median_ms"] / entry["hip"]["median_ms"]
        entry["faster_by_more_than_the_spread"] = bool(gain > entry["hip"]["spread_ms"] + entry["torch_fp64_blocked"]["spread_ms"])
        print(json.dumps(entry), flush=True)
        results["shapes"].append(entry)
        del real, fake
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
