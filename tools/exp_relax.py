"""Curve energy and relaxation on one MI355X (geo_curve_energy / geo_curve_relax through vqvae_amd.geo.relaxation):

    large   16 384 curves x 9 frames x 16 dims on the fm (28 px, 1 channel, 16 outputs) and cf (32 px, 3 channels, 192 outputs)
            decoders (dec_channels 256-128-64, eval-mode BatchNorm): seconds per geo_curve_energy call, per geo_curve_relax call
            of 0 and of `--iters` iterations (per iteration: their difference / iters), next to geo_decoder_metric_tensor
            (no spectrum) over the same 147 456 latents -- the cost of the new reductions over the column pass they ride on --
            and next to the torch route on the same GPU at 64 curves only (nothing is extrapolated from it)
    cli     48 curves x 9 frames, 100 iterations: with the weights packed once per call, and with option curve_repack = 1,
            which packs them before every evaluation as a run_jvp call per iteration would (same bits); the ratio is stated

Times are host clocks around `--inner` consecutive calls that end in a device synchronise, after a warm-up call of the same
shape; every repetition is listed.  The native times include the decoder export.  No number is a target.
Writes profiles/relax_mi355x.json (or --out).  `--trace` runs the large fm shape once (one energy call, one relax call of
`--iters` iterations) and nothing else: the run to put under a kernel trace.

    python tools/exp_relax.py [--reps 5] [--inner 3] [--iters 5] [--out FILE] [--trace]
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
from vqvae_amd.geo import riemannian_metric as rm  # noqa: E402
from vqvae_amd.spatial_decoder import DecoderExport, SpatialDecoder  # noqa: E402

SHAPES = {"fm": (1, 28), "cf": (3, 32)}
CHANNELS = (256, 128, 64)
C_LARGE, C_TORCH, C_CLI, F, D, CLI_ITERS = 16384, 64, 48, 9, 16, 100


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner, out


def make_decoder(cout, px, dev):
    torch.manual_seed(0)
    dec = SpatialDecoder(cout, CHANNELS, D, px, "batch")
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
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


def main():
    cli = argparse.ArgumentParser()
    cli.add_argument("--reps", type=int, default=5)
    cli.add_argument("--inner", type=int, default=3)
    cli.add_argument("--iters", type=int, default=5)
    cli.add_argument("--trace", action="store_true")
    cli.add_argument("--out", default=os.path.join(ROOT, "profiles", "relax_mi355x.json"))
    args = cli.parse_args()
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    x_large, x_torch, x_cli = curves(C_LARGE, dev), curves(C_TORCH, dev), curves(C_CLI, dev)
    if args.trace:
        ex = DecoderExport(make_decoder(*SHAPES["fm"], dev), dev)
        rx.curve_energy_device(ex, x_large)
        rx.relax_curves_device(ex, x_large, args.iters)
        torch.cuda.synchronize()
        return
    result = {"device": torch.cuda.get_device_name(0), "dec_channels": CHANNELS, "norm": "batch (eval)", "reps": args.reps,
              "calls_per_rep": args.inner, "frames": F, "latent_dim": D, "relax_iters_large": args.iters, "shapes": {}}
    for name, (cout, px) in SHAPES.items():
        dec = make_decoder(cout, px, dev)
        assert rx.native_relax_covers(dec)
        z_large = x_large.reshape(-1, D)

        def energy():
            return rx.curve_energy_device(dec, x_large)

        def relax0():
            return rx.relax_curves_device(dec, x_large, 0)

        def relaxn():
            return rx.relax_curves_device(dec, x_large, args.iters)

        def metric():
            return rm.pullback_metric_device(dec, z_large, spectrum=False)

        def energy_64():
            return rx.curve_energy_device(dec, x_torch)

        def torch_energy_64():
            return rx._torch_evaluate(dec, x_torch)

        def torch_relax1_64():
            return rx._torch_relax(dec, x_torch, 1, torch.full((C_TORCH,), -1.0, dtype=torch.float64, device=dev))

        def relax1_64():
            return rx.relax_curves_device(dec, x_torch, 1)

        def cli_relax():
            return rx.relax_curves_device(dec, x_cli, CLI_ITERS)

        for fn in (energy, relax0, relaxn, metric, energy_64, relax1_64, torch_energy_64, torch_relax1_64, cli_relax):
            fn()                                                           # warm-up of every timed shape
        times = {k: [] for k in ("energy", "relax0", "relaxn", "metric", "energy_64", "relax1_64", "torch_energy_64",
                                 "torch_relax1_64", "cli_once", "cli_repack")}
        for _ in range(args.reps):                                         # alternating
            for key, fn, inner in (("energy", energy, args.inner), ("relax0", relax0, args.inner), ("relaxn", relaxn, args.inner),
                                   ("metric", metric, args.inner), ("energy_64", energy_64, args.inner),
                                   ("relax1_64", relax1_64, args.inner), ("torch_energy_64", torch_energy_64, 1),
                                   ("torch_relax1_64", torch_relax1_64, 1), ("cli_once", cli_relax, args.inner)):
                t, out = timed(fn, inner)
                times[key].append(t)
                if key == "relaxn":
                    got = out
                if key == "cli_once":
                    once = out
            _lib.check(lib.geo_set_option(b"curve_repack", 1), "geo_set_option")
            try:
                t, repack = timed(cli_relax, args.inner)
            finally:
                lib.geo_set_option(b"curve_repack", 0)
            times["cli_repack"].append(t)
        assert got.route == "native" and torch.equal(once.frames, repack.frames) and torch.equal(once.step, repack.step)
        per_iter = [(a - b) / args.iters for a, b in zip(times["relaxn"], times["relax0"])]
        ws = lib.geo_curve_workspace_bytes(DecoderExport(dec, dev).desc, C_LARGE, F)
        ratio = (got.energy / got.energy0).cpu().numpy()
        result["shapes"][name] = {
            "out_channels": cout, "px": px, "outputs": cout * (16 if px == 28 else 64), "curves": C_LARGE,
            "latents": C_LARGE * F, "workspace_bytes": int(ws),
            "energy_s_per_call": times["energy"], "relax_0_iters_s_per_call": times["relax0"],
            f"relax_{args.iters}_iters_s_per_call": times["relaxn"], "relax_s_per_iteration": per_iter,
            "metric_tensor_s_per_call": times["metric"],
            "energy_over_metric_tensor_best": min(times["energy"]) / min(times["metric"]),
            "iteration_over_metric_tensor_best": min(per_iter) / min(times["metric"]),
            f"energy_ratio_after_{args.iters}_iters": {"min": float(ratio.min()), "median": float(np.median(ratio)),
                                                        "max": float(ratio.max())},
            "accepted_mean": float(got.accepted.double().mean()),
            "curves_64": {"native_energy_s_per_call": times["energy_64"], "native_relax_1_iter_s_per_call": times["relax1_64"],
                          "torch_energy_s_per_call": times["torch_energy_64"],
                          "torch_relax_1_iter_s_per_call": times["torch_relax1_64"]},
            "cli_sized": {"curves": C_CLI, "iters": CLI_ITERS, "packed_once_s_per_call": times["cli_once"],
                          "packed_every_evaluation_s_per_call": times["cli_repack"],
                          "repack_over_once_best": min(times["cli_repack"]) / min(times["cli_once"])}}
        print(name, json.dumps(result["shapes"][name]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
