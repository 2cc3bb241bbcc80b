"""python -m vqvae_amd.scripts.evaluate_baseline --checkpoint ckpt_best.pt --out_dir DIR [--max_samples 1000 --gen_samples 100
--config config.yaml --lpips_weights alex.pt]: the reference's scripts/evaluate_baseline_simple.py.

Reconstruction of the first max_samples test images (batches of 128, in order) with PSNR and the global SSIM of the whole set
in [0, 1], codebook health of the first max_samples codes (the reference cuts the flattened codes, not the images); generation from uniformly random 8 x 8 code grids (torch.randint on the device,
gen_samples // 10 per class) against the first test images of each class.  Metrics come from vqvae_amd.eval.metrics, the grids
from the PNG writer of scripts/generate_samples.py.  Writes evaluation_results.json, codebook_health.json, metrics.yaml,
generated_samples.png and comparison_grid.png with the reference's keys and rounding.  LPIPS is computed when --lpips_weights
names the state dict of lpips.LPIPS(net='alex') (vqvae_amd.eval.lpips): generated and real images are
resized to 64 (bilinear), mapped to [-1, 1] and compared pair by pair, as the reference does; generation_quality gains "lpips",
metrics.yaml "LPIPS".  Without the flag no LPIPS key is written (the weights are not part of this project).  The config is
the checkpoint's "cfg" unless --config is given.
Exit code 0 on success, 1 on a missing checkpoint or an error.
"""
import argparse
import json
import traceback
from pathlib import Path

import torch
import torch.nn.functional as F
import yaml

from ..baseline.data import load_split
from ..baseline.model import model_from_config
from ..baseline.train import load_config, set_seed
from ..eval.data import cifar10_test
from ..eval.lpips import load_lpips_weights, lpips_mean
from ..eval.metrics import codebook_stats, psnr, ssim_simple
from .generate_samples import save_image


def _scale_each(images: torch.Tensor) -> torch.Tensor:
    """save_image(normalize=True, scale_each=True): each image min-max scaled to [0, 1] (torchvision's norm_range)."""
    out = images.clone()
    for t in out:
        lo, hi = float(t.min()), float(t.max())
        t.clamp_(min=lo, max=hi).sub_(lo).div_(max(hi - lo, 1e-5))
    return out


def results_dict(psnr_recon, ssim_recon, n_eval, gen_psnr, gen_ssim, n_gen, per_class, cb, K, *, gen_lpips=None) -> dict:
    """evaluation_results.json: the reference's keys and rounding (what compare_all_approaches.extract_metrics reads).
    generation_quality has "lpips" only when gen_lpips is given."""
    results = {
        "model_type": "baseline_vqvae",
        "dataset": "cifar10",
        "reconstruction_quality": {"psnr": float(f"{psnr_recon:.6f}"), "ssim": float(f"{ssim_recon:.6f}"),
                                   "samples_evaluated": n_eval},
        "generation_quality": {"psnr": float(f"{gen_psnr:.6f}"), "ssim": float(f"{gen_ssim:.6f}"), "samples_generated": n_gen,
                               "samples_per_class": per_class},
        "codebook_health": {"entropy": float(f"{cb['entropy']:.6f}"), "used_codes": int(cb["used"]),
                            "dead_codes": int(cb["dead_codes"]), "usage_percent": float(f"{100 * cb['used'] / K:.2f}"),
                            "codebook_size": K},
    }
    if gen_lpips is not None:
        results["generation_quality"]["lpips"] = float(f"{gen_lpips:.6f}")
    return results


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Simple Baseline VQ-VAE Evaluation")
    ap.add_argument("--checkpoint", default="outputs/checkpoints/ckpt_best.pt")
    ap.add_argument("--out_dir", default="evaluation")
    ap.add_argument("--max_samples", type=int, default=1000)
    ap.add_argument("--gen_samples", type=int, default=100)
    ap.add_argument("--config", default=None)
    ap.add_argument("--lpips_weights", default=None,
                    help="State dict of lpips.LPIPS(net='alex'); without it LPIPS is not computed")
    args = ap.parse_args(argv)
    try:
        if not torch.cuda.is_available():
            print("ERROR: evaluate_baseline needs a GPU: the quantizer runs as HIP kernels")
            return 1
        device = torch.device("cuda")
        print(f"Device: {device}")
        if not Path(args.checkpoint).exists():
            print(f"ERROR: Checkpoint not found: {args.checkpoint}")
            return 1
        print(f"Loading checkpoint: {args.checkpoint}")
        ckpt = torch.load(args.checkpoint, map_location=device, weights_only=False)
        config = load_config(args.config) if args.config else ckpt["cfg"]
        set_seed(config["seed"])
        model = model_from_config(config).to(device)
        model.load_state_dict(ckpt["model"])
        model.eval()
        K = model.quant.n_codes
        print("Model loaded successfully")
        print(f"   Epoch: {ckpt.get('epoch', 'Unknown')}")
        print(f"   Codebook size: {config['model']['n_codes']}")

        print("Loading test data...")
        test = load_split(config, "test", device)
        print(f"Evaluating reconstruction on {args.max_samples} samples...")
        origs, recs, codes = [], [], []
        done = 0
        with torch.no_grad():
            for x in test.ordered_batches(128):
                if done >= args.max_samples:
                    break
                x_rec, _, idx, _, _ = model(x)
                origs.append((x + 1.0) / 2.0)
                recs.append((x_rec + 1.0) / 2.0)
                codes.append(idx.view(-1))
                done += x.size(0)
                if done % 500 == 0:
                    print(f"   Processed {done}/{args.max_samples} samples")
        originals = torch.cat(origs, 0)[:args.max_samples].cpu()
        reconstructions = torch.cat(recs, 0)[:args.max_samples].cpu()
        codes = torch.cat(codes, 0)[:args.max_samples]

        print("Computing reconstruction metrics...")
        psnr_recon = psnr(originals, reconstructions)
        ssim_recon = ssim_simple(originals.reshape(-1), reconstructions.reshape(-1))
        cb = codebook_stats(codes, K)
        print("Reconstruction Results:")
        print(f"   PSNR: {psnr_recon:.4f} dB")
        print(f"   SSIM: {ssim_recon:.4f}")
        print(f"   Entropy: {cb['entropy']:.4f}")
        print(f"   Usage: {cb['used']}/{K} ({100 * cb['used'] / K:.1f}%)")

        print(f"Generating {args.gen_samples} samples...")
        per_class = args.gen_samples // 10
        gen = []
        with torch.no_grad():
            for _ in range(10):
                for _ in range(per_class):
                    rc = torch.randint(0, K, (1, 8, 8), device=device)
                    z_q = model.quant.embed[rc].view(1, 8, 8, -1).permute(0, 3, 1, 2).contiguous()
                    gen.append(((model.dec(z_q) + 1.0) / 2.0).cpu())
        generated = torch.cat(gen, 0) if gen else torch.zeros(0, 3, 32, 32)

        print("Loading real samples for comparison...")
        images, labels = cifar10_test(config["data"]["root"])
        by_class = {c: [] for c in range(10)}
        for img, lab in zip(images, labels.tolist()):
            if len(by_class[lab]) < per_class:
                by_class[lab].append(torch.from_numpy(img).permute(2, 0, 1).contiguous().to(torch.float32).div(255))
            if all(len(v) >= per_class for v in by_class.values()):
                break
        real = torch.stack([im for c in range(10) for im in by_class[c][:per_class]])

        print("Computing generation metrics...")
        gen_psnr = psnr(real, generated)
        gen_ssim = ssim_simple(real.reshape(-1), generated.reshape(-1))
        lpips_score = None
        if args.lpips_weights is not None:
            gen_lpips = (F.interpolate(generated, size=(64, 64), mode="bilinear", align_corners=False) * 2 - 1).to(device)
            real_lpips = (F.interpolate(real, size=(64, 64), mode="bilinear", align_corners=False) * 2 - 1).to(device)
            lpips_score = lpips_mean(load_lpips_weights(args.lpips_weights), gen_lpips, real_lpips)
            print(f"LPIPS: {lpips_score:.4f}")
        else:
            print("WARNING: LPIPS not available (not computed by this port)")    # (unchanged output; --lpips_weights computes it)
        print("Generation Results:")
        print(f"   PSNR (vs Real): {gen_psnr:.4f} dB")
        print(f"   SSIM (vs Real): {gen_ssim:.4f}")
        if lpips_score is not None:
            print(f"   LPIPS (vs Real): {lpips_score:.4f}")

        print("Saving results...")
        out_dir = Path(args.out_dir)
        out_dir.mkdir(parents=True, exist_ok=True)
        save_image(_scale_each(generated), str(out_dir / "generated_samples.png"), nrow=per_class)
        pairs = []
        for c in range(10):
            s = c * per_class
            if s + 1 < len(real) and s + 1 < len(generated):
                for i in range(2):
                    pairs += [real[s + i], generated[s + i]]
        if pairs:
            save_image(_scale_each(torch.stack(pairs)), str(out_dir / "comparison_grid.png"), nrow=4)

        results = results_dict(psnr_recon, ssim_recon, len(originals), gen_psnr, gen_ssim, len(generated), per_class, cb, K,
                               gen_lpips=lpips_score)
        metrics_yaml = {"PSNR": f"{gen_psnr:.4f}", "SSIM": f"{gen_ssim:.4f}"}
        if lpips_score is not None:
            metrics_yaml["LPIPS"] = f"{lpips_score:.4f}"
        with open(out_dir / "metrics.yaml", "w") as f:
            yaml.dump(metrics_yaml, f)
        with open(out_dir / "evaluation_results.json", "w") as f:
            json.dump(results, f, indent=2)
        with open(out_dir / "codebook_health.json", "w") as f:
            json.dump(results["codebook_health"], f, indent=2)
        print(f"Results saved to: {out_dir}")
        print("   Generated samples: generated_samples.png")
        print("   Comparison grid: comparison_grid.png")
        print("   Metrics: metrics.yaml, evaluation_results.json")
        return 0
    except Exception as e:  # the reference reports every failure and exits 1
        print(f"ERROR: Error during evaluation: {e}")
        traceback.print_exc()
        return 1


if __name__ == "__main__":
    raise SystemExit(main())
