"""Curve relaxation under the vanilla decoder on one MI355X: the native route (geo_vanilla_curve_relax through
vqvae_amd.geo.relaxation) next to the torch route of the same module (relaxation._torch_relax: full Jacobians by
torch.autograd.functional.jacobian, one curve at a time) on the same GPU.

    shapes   64 and 1 024 curves x 9 frames x `--iters` iterations (default 20), the step left to the call, under the
             wide-bn-28 (d = 128, 784 outputs) and wide-bn-32x3 (d = 128, 3 072 outputs) decoders of tests/vanilla_jvp_cases.py
    native   seconds per relax_curves_device call (decoder export, the trace for the initial step and the `--iters` trials
             included), and per geo_vanilla_vjp call over the same frames
    torch    seconds per _torch_relax call.  The two routes alternate within a repetition.  The torch route stops repeating once
             its calls have used `--torch_budget` seconds per decoder and shape, and a shape whose first call would not fit is
             "not measured": nothing is extrapolated

Times are host clocks around calls that end in a device synchronise, after a warm-up of every timed shape (the torch route
warms up on two curves and one iteration: the same per-curve shapes); every repetition is listed.  No number is a target.
Writes profiles/vanilla_relax_mi355x.json (or --out).  `--trace` runs one native call of the 1 024-curve wide-bn-28 shape and
nothing else: the run to put under a kernel trace.

    python tools/exp_vanilla_relax.py [--reps 5] [--iters 20] [--torch_budget 120] [--out FILE] [--trace]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vqvae_amd import _lib  # noqa: E402
from vqvae_amd.geo import relaxation as rx  # noqa: E402
from vqvae_amd.geo.riemannian_metric import vanilla_vjp_device  # noqa: E402
from vqvae_amd.vae import Decoder  # noqa: E402
from vqvae_amd.vanilla_decoder import VanillaDecoderExport  # noqa: E402

SHAPES = {"wide-bn-28": (1, 28), "wide-bn-32x3": (3, 32)}
CHANNELS, D, F = (256, 128, 64), 128, 9
CURVES = (64, 1024)


def make_decoder(cout, px, dev):
    """vqvae_amd.vae.Decoder with seeded weights and non-trivial BatchNorm statistics, in eval mode."""
    torch.manual_seed(0)
    dec = Decoder(cout, CHANNELS, D, px, "batch")
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.normal_(1.0, 0.2)
                m.bias.normal_(0.0, 0.1)
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    return dec.to(dev).eval()


def curves(C, dev):
    """Zig-zags about random chords, as in tests/relax_cases.py but drawn in one go."""
    rs = np.random.RandomState(1)
    a, b, zig = rs.randn(C, 1, D), rs.randn(C, 1, D), rs.randn(C, 1, D)
    zig /= np.linalg.norm(zig, axis=2, keepdims=True)
    t = (np.arange(F) / (F - 1))[None, :, None]
    sign = np.where(np.arange(F) % 2 == 1, 0.5, -0.5)[None, :, None]
    sign[:, 0], sign[:, -1] = 0.0, 0.0
    return torch.from_numpy((a + t * (b - a) + sign * zig).astype(np.float32)).to(dev)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(ts):
    return {"reps": ts, "best": min(ts), "median": float(np.median(ts)), "worst": max(ts)} if ts else "not measured"


def main():
    cli = argparse.ArgumentParser()
    cli.add_argument("--reps", type=int, default=5)
    cli.add_argument("--iters", type=int, default=20)
    cli.add_argument("--torch_budget", type=float, default=120.0, help="seconds of torch-route calls per decoder and shape")
    cli.add_argument("--trace", action="store_true")
    cli.add_argument("--out", default=os.path.join(ROOT, "profiles", "vanilla_relax_mi355x.json"))
    args = cli.parse_args()
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    if args.trace:
        dec = make_decoder(*SHAPES["wide-bn-28"], dev)
        rx.relax_curves_device(dec, curves(CURVES[-1], dev), args.iters)
        torch.cuda.synchronize()
        return
    result = {"device": torch.cuda.get_device_name(0), "dec_channels": CHANNELS, "norm": "batch (eval)", "latent_dim": D,
              "frames": F, "iters": args.iters, "reps": args.reps, "torch_budget_s": args.torch_budget, "decoders": {}}
    for name, (cout, px) in SHAPES.items():
        dec = make_decoder(cout, px, dev)
        assert rx.native_vanilla_relax_covers(dec)
        ex = VanillaDecoderExport(dec, dev)
        warm = curves(2, dev)
        rx._torch_relax(dec, warm, 1, torch.full((2,), -1.0, dtype=torch.float64, device=dev))
        torch_per_curve = None                                   # seconds per curve of the last torch call: decides, is not reported
        shapes = {}
        for C in CURVES:
            x = curves(C, dev)
            u = torch.randn(C * F, ex.n_out, device=dev, generator=torch.Generator(dev).manual_seed(2))

            def native():
                return rx.relax_curves_device(dec, x, args.iters)

            def vjp():
                return vanilla_vjp_device(ex, x.reshape(C * F, D), u)

            def torch_route():
                return rx._torch_relax(dec, x, args.iters, torch.full((C,), -1.0, dtype=torch.float64, device=dev))

            native()
            vjp()
            t_native, t_vjp, t_torch, spent, why = [], [], [], 0.0, None
            if torch_per_curve is not None and torch_per_curve * C > args.torch_budget:
                why = f"not measured: one call would not fit {args.torch_budget:.0f} s"
            for _ in range(args.reps):                            # alternating
                t, got = timed(native)
                t_native.append(t)
                t_vjp.append(timed(vjp)[0])
                if why is None:
                    t, ref = timed(torch_route)
                    t_torch.append(t)
                    spent += t
                    torch_per_curve = t / C
                    if spent + t > args.torch_budget and len(t_torch) < args.reps:
                        why = f"{len(t_torch)} of {args.reps} repetitions: the next would pass {args.torch_budget:.0f} s"
            assert got.route == "native" and bool((got.energy <= got.energy0).all())
            ratio = (got.energy / got.energy0).cpu().numpy()
            entry = {"curves": C, "frames_total": C * F,
                     "workspace_bytes": int(lib.geo_vanilla_curve_workspace_bytes(ex.desc, C, F)),
                     "native_relax_s_per_call": spread(t_native), "native_vjp_s_per_call": spread(t_vjp),
                     "torch_relax_s_per_call": spread(t_torch), "torch_note": why,
                     "native_energy_ratio": {"min": float(ratio.min()), "median": float(np.median(ratio)), "max": float(ratio.max())},
                     "native_accepted_mean": float(got.accepted.double().mean())}
            if t_torch:
                t_ratio = (ref[2] / ref[1]).cpu().numpy()
                entry["torch_energy_ratio"] = {"min": float(t_ratio.min()), "median": float(np.median(t_ratio)),
                                               "max": float(t_ratio.max())}
                entry["torch_accepted_mean"] = float(ref[5].double().mean())
                entry["torch_over_native_best"] = min(t_torch) / min(t_native)
                entry["native_slower_than_torch"] = bool(min(t_native) > min(t_torch))
            shapes[str(C)] = entry
            print(name, C, json.dumps(entry), flush=True)
        result["decoders"][name] = {"out_channels": cout, "px": px, "outputs": ex.n_out, "shapes": shapes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
