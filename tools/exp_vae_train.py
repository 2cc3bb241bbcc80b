"""Timing of the vanilla-VAE training step and of the ELBO alone, native HIP loss against the torch loss.

    python tools/exp_vae_train.py --out profiles/vae_train_fm.json

FashionMNIST vanilla configuration (batch 256, 1 x 28 x 28, latent 128, channels 64 / 128 / 256, mse + sigmoid, batch norm,
AdamW, clip 1.0) on synthetic uint8 images: the step does not depend on pixel values.  Times are host clocks around windows
that end in a device synchronise; the two variants alternate, `--repeats` windows each, and the median and the spread are
reported.  The loss-alone figure times forward + backward of the loss on fixed (x_logits, mu, logvar); the kernel times
come from device events around each call, and the HBM rate is the bytes the kernel must move (forward 8 B P + 8 B d, backward
12 B P + 16 B d) over that time.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vqvae_amd.training.data import ResidentLoader, resident_images
from vqvae_amd.training.engine import TrainingEngine
from vqvae_amd.vae import VAE, elbo_hip

MODEL = dict(in_channels=1, output_image_size=28, latent_dim=128, enc_channels=[64, 128, 256], dec_channels=[256, 128, 64],
             recon_loss="mse", norm_type="batch", mse_use_sigmoid=True, free_bits_default=0.25, capacity_max_default=25.0,
             capacity_anneal_steps_default=100000, capacity_mode_default="abs")


def sync_time(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def event_time(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(n):
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--images", type=int, default=60000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda")
    B, P, d = args.batch, 784, MODEL["latent_dim"]
    result = {"device": torch.cuda.get_device_name(0), "batch": B, "model": MODEL, "images": args.images}

    # ---- the loss alone
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = torch.randn(B, 1, 28, 28, device=dev, generator=g)
    x = torch.rand(B, 1, 28, 28, device=dev, generator=g)
    mu = torch.randn(B, d, device=dev, generator=g)
    logvar = torch.randn(B, d, device=dev, generator=g)
    model = VAE(**MODEL)

    def loss_step(native, item_reads=False):
        leaves = [t.clone().requires_grad_(True) for t in (logits, mu, logvar)]

        def fn():
            model.native_loss = native
            total, recon, kl = model.loss(x, leaves[0], leaves[1], leaves[2], beta=1.0, step=1000)
            total.backward()
            if item_reads:
                total.item(), recon.item(), kl.item()                 # the reference's three reads per step
            for t in leaves:
                t.grad = None
        return fn

    variants = {"hip": loss_step(True), "torch": loss_step(False), "torch_with_item_reads": loss_step(False, True)}
    for fn in variants.values():
        sync_time(fn, 20)
    loss_ms = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            loss_ms[k].append(sync_time(fn, 500))
    result["loss_fwd_bwd_ms_per_call"] = {k: summary(v) for k, v in loss_ms.items()}

    out = elbo_hip(logits, x, mu, logvar, 1, 0.25, 1.0, 0.25, 1)
    leaf = [t.clone().requires_grad_(True) for t in (logits, mu, logvar)]
    fwd = event_time(lambda: elbo_hip(logits, x, mu, logvar, 1, 0.25, 1.0, 0.25, 1), 200)
    o = elbo_hip(leaf[0], x, leaf[1], leaf[2], 1, 0.25, 1.0, 0.25, 1)
    bwd = event_time(lambda: torch.autograd.grad(o[0], leaf, retain_graph=True), 200)
    fwd_bytes, bwd_bytes = 8 * B * P + 8 * B * d, 12 * B * P + 16 * B * d
    result["elbo_calls_event_ms"] = {
        "forward_ms": fwd, "backward_ms": bwd, "forward_bytes": fwd_bytes, "backward_bytes": bwd_bytes,
        "forward_GBps": fwd_bytes / fwd / 1e6, "backward_GBps": bwd_bytes / bwd / 1e6,
        "note": "event windows around the whole Python call (workspace allocation, two launches forward; autograd "
                "dispatch and three output allocations backward): a lower bound on the kernels' own rate"}
    del out

    # ---- the training step and epoch
    r = np.random.RandomState(0)
    data = resident_images(r.randint(0, 256, (args.images, 28, 28)).astype(np.uint8), r.randint(0, 10, args.images), dev)
    step_ms = {"hip": [], "torch": []}
    epoch_ms = {"hip": [], "torch": []}
    engines = {}
    for name in step_ms:
        torch.manual_seed(0)
        m = VAE(**MODEL).to(dev)
        m.native_loss = name == "hip"
        engines[name] = TrainingEngine(m, torch.optim.AdamW(m.parameters(), lr=3e-4, weight_decay=1e-4), dev)
    small = ResidentLoader(resident_images(data.u8[:B * args.steps].cpu().numpy()[..., 0], np.zeros(B * args.steps), dev), B, True)
    full = ResidentLoader(data, B, True)
    quiet = contextlib.redirect_stdout(io.StringIO())
    with quiet:
        for e in engines.values():
            e.run_epoch(small, True, 0, 0, 1.0, 1.0, 0)
        for _ in range(args.repeats):
            for name, e in engines.items():
                step_ms[name].append(sync_time(lambda: e.run_epoch(small, True, 0, 0, 1.0, 1.0, 0), 1) / len(small))
        for _ in range(2):
            for name, e in engines.items():
                epoch_ms[name].append(sync_time(lambda: e.run_epoch(full, True, 0, 0, 1.0, 1.0, 0), 1))
    result["train_step_ms"] = {k: summary(v) for k, v in step_ms.items()}
    result["train_epoch_ms"] = {k: summary(v) for k, v in epoch_ms.items()}
    result["steps_per_epoch"] = len(full)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: result[k] for k in ("loss_fwd_bwd_ms_per_call", "elbo_calls_event_ms", "train_step_ms", "train_epoch_ms")}))


if __name__ == "__main__":
    main()
