"""Native LPIPS against the torch module on one MI355X.  Writes profiles/lpips_mi355x.json (or --out).

Per size (1 000 and 10 000 pairs of 3 x 64 x 64 images), four routes, all warmed up three times and then alternating in one
process:
  - native_one_batch / native_batch32: vqvae_amd.eval.lpips.lpips_pairs on a prepared export (the HIP kernels of
    csrc/lpips.hip), all pairs in one call, and in calls of 32 pairs (the batch of the reference's baseline evaluation);
  - torch_one_batch / torch_batch32: LPIPSAlex on the same GPU under no_grad, float32, the same two batchings.
A repetition is the host clock around `inner` consecutive evaluations ending in a device synchronise, divided by `inner`; every
repetition is listed, with the median, and the spread as (max - min) / median.  Inputs are on the device before the clock starts.
Recorded with the times: the multiply-adds of one image (39 523 008), the whole call's share of the f32 matrix peak -- an
end-to-end rate over a peak, not a kernel's share -- and the maximum absolute difference between the two routes' values.

    python tools/exp_lpips.py [--out profiles/lpips_mi355x.json] [--reps 7]
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

from vqvae_amd.eval.lpips import CONVS, LPIPSAlex, LPIPSExport, last_lpips_path, lpips_pairs  # noqa: E402

MFMA_F32_FLOPS = 157.3e12        # f32 matrix peak (MI355X_MICROARCH.md)
SIZES = ((1_000, 20), (10_000, 5))                   # (pairs, evaluations per timed window)
OUT_PIXELS = (225, 49, 9, 9, 9)
MACS_PER_IMAGE = sum(p * o * i * k * k for p, (i, o, k, _, _) in zip(OUT_PIXELS, CONVS))


def seeded_model(dev):
    model = LPIPSAlex()
    torch.manual_seed(0)
    with torch.no_grad():
        for conv in model.convs:
            torch.nn.init.kaiming_normal_(conv.weight)
            conv.bias.normal_(0.0, 0.1)
        for lin in model.lins:
            lin.uniform_(0.0, 2.0 / lin.numel())
    return model.to(dev).eval()


def sync_time(f, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def measure(n, inner, model, export, dev, reps):
    g = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.rand(n, 3, 64, 64, device=dev, generator=g) * 2 - 1
    x1 = (x0 + 0.2 * torch.randn(n, 3, 64, 64, device=dev, generator=g)).clamp(-1, 1)
    x1[n // 2:] = torch.rand(n - n // 2, 3, 64, 64, device=dev, generator=g) * 2 - 1

    def native(batch):
        return torch.cat([lpips_pairs(export, x0[i:i + batch], x1[i:i + batch]) for i in range(0, n, batch)])

    @torch.no_grad()
    def module(batch):
        return torch.cat([model(x0[i:i + batch], x1[i:i + batch]).view(-1) for i in range(0, n, batch)])

    contestants = {"native_one_batch": lambda: native(n), "torch_one_batch": lambda: module(n),
                   "native_batch32": lambda: native(32), "torch_batch32": lambda: module(32)}
    for _ in range(3):                                       # warm-up: code objects, convolution set-up, the workspace
        outs = {k: f() for k, f in contestants.items()}
    assert last_lpips_path() == "hip"
    diff = float((outs["native_one_batch"] - outs["torch_one_batch"].double()).abs().max())
    assert torch.equal(outs["native_one_batch"], outs["native_batch32"])
    mean = float(outs["native_one_batch"].mean())
    del outs
    times = {k: [] for k in contestants}
    for _ in range(reps):                                    # alternating, one process
        for k, f in contestants.items():
            times[k].append(sync_time(f, inner))
    row = {"pairs": n, "evaluations_per_timed_window": inner, "model_multiply_adds_per_image": MACS_PER_IMAGE,
           "mean_value": mean, "max_abs_diff_native_vs_torch": diff}
    for k, ts in times.items():
        med = float(np.median(ts))
        row[f"{k}_s"] = ts
        row[f"{k}_s_median"] = med
        row[f"{k}_spread"] = (max(ts) - min(ts)) / med
        row[f"{k}_us_per_pair_median"] = med / n * 1e6
    for batch in ("one_batch", "batch32"):
        row[f"torch_over_native_{batch}_median"] = row[f"torch_{batch}_s_median"] / row[f"native_{batch}_s_median"]
    row["fraction_of_f32_matrix_peak_whole_call"] = 2 * MACS_PER_IMAGE * 2 * n / row["native_one_batch_s_median"] / MFMA_F32_FLOPS
    print(json.dumps({k: v for k, v in row.items() if not isinstance(v, list)}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_mi355x.json"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_lpips.py measures on the MI355X; no GPU here")
    dev = torch.device("cuda", 0)
    model = seeded_model(dev)
    export = LPIPSExport(model, dev)
    rows = [measure(n, inner, model, export, dev, args.reps) for n, inner in SIZES]
    rep = {"device": torch.cuda.get_device_name(0), "f32_matrix_peak_flops": MFMA_F32_FLOPS, "reps": args.reps,
           "timing": "host clock around evaluations_per_timed_window consecutive evaluations ending in a device synchronise, per "
                     "evaluation; three warm-ups; routes alternating in one process; median of the repetitions, spread = "
                     "(max - min) / median",
           "sizes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=2)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
