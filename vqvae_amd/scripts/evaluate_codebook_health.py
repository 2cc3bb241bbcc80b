"""Codebook health on the MI355X: drop-in for the reference's src/eval/evaluate_codebook_health.py (same flags, same
evaluation/codebook_health.json: keys, rounding, health thresholds, exit codes).

    python -m vqvae_amd.scripts.evaluate_codebook_health --experiment experiments/fashionmnist/vanilla/geodesic \
        --dataset fashionmnist

Every validation latent is assigned to its nearest medoid (geo_kmeans_assign, exact fp64 key; vqvae_amd.eval.reconstruction),
decoded continuous and quantized in eval mode, post-processed as the reference's unnormalize_images, and reduced per image by
geo_image_pair_moments; images never leave the device.  Spatial experiments, on which the reference raises, are quantized
position by position (an extension; vqvae_amd.eval.experiment describes both layouts and the override flags).
"""
import argparse
import json
from pathlib import Path

import torch

from .._device import device
from ..eval.experiment import add_experiment_args, detect_layout, load_decoder
from ..eval.metrics import codebook_stats
from ..eval.reconstruction import decode_pair_moments, last_assign_path, metrics_from_moments, quantize


def health_of(entropy: float, usage_percent: float) -> str:
    if entropy > 4.5 and usage_percent > 80:
        return "EXCELLENT"
    if entropy > 3.5 and usage_percent > 60:
        return "GOOD"
    if entropy > 2.5 and usage_percent > 40:
        return "MODERATE"
    return "POOR"


def main(argv=None) -> int:
    args = make_parser().parse_args(argv)
    dev = device()
    try:
        paths = detect_layout(args.experiment, args.vae_ckpt_path, args.latents_path, args.codebook_path)
        codebook = torch.load(paths.codebook, map_location="cpu", weights_only=False) if paths.codebook.exists() else None
        vae, vae_config = load_decoder(paths, args, dev, codebook)
    except (OSError, ValueError, RuntimeError, KeyError) as e:
        print(f"Error: Failed to load VAE model ({e})")
        return 1

    try:
        z_val = torch.load(paths.latents, map_location="cpu", weights_only=False).float()
        if codebook is None:
            raise FileNotFoundError(f"{paths.codebook} does not exist")
        z_medoid = codebook["z_medoid"].float()
    except (OSError, ValueError, RuntimeError, KeyError) as e:
        print(f"Error loading data: {e}")
        return 1

    z_dev = z_val.to(dev)
    codes, zq_val = quantize(z_dev, z_medoid)
    print(f"Assigned {codes.numel()} latents to {z_medoid.shape[0]} medoids ({paths.layout}, assignment: {last_assign_path()})")

    recon_loss = vae_config.get("recon_loss", "mse").lower()
    mse_use_sigmoid = vae_config.get("mse_use_sigmoid", True)
    apply_sigmoid = (recon_loss == "bce") or mse_use_sigmoid

    mom = decode_pair_moments(vae, z_dev, zq_val, dataset=args.dataset, apply_sigmoid=apply_sigmoid,
                              batch_size=args.batch_size)
    cont_quant_psnr, cont_quant_ssim = metrics_from_moments(mom["a_b"], mom["n_pix"])
    cb_stats = codebook_stats(codes, K=z_medoid.shape[0])

    usage_percent = 100 * cb_stats["used"] / z_medoid.shape[0]
    print(f"PSNR: {cont_quant_psnr:.2f} dB, SSIM: {cont_quant_ssim:.4f}")
    print(f"Entropy: {cb_stats['entropy']:.3f}, Usage: {usage_percent:.1f}%")
    health = health_of(cb_stats["entropy"], usage_percent)
    print(f"Health: {health}")

    output_dir = Path(args.experiment) / "evaluation"
    output_dir.mkdir(parents=True, exist_ok=True)
    results = {
        "dataset": args.dataset,
        "samples_evaluated": len(z_val),
        "codebook_size": int(z_medoid.shape[0]),
        "psnr_continuous_vs_quantized": float(f"{cont_quant_psnr:.6f}"),
        "ssim_continuous_vs_quantized": float(f"{cont_quant_ssim:.6f}"),
        "entropy": float(f"{cb_stats['entropy']:.6f}"),
        "used_codes": int(cb_stats["used"]),
        "dead_codes": int(cb_stats["dead_codes"]),
        "usage_percent": float(f"{usage_percent:.2f}"),
        "health_assessment": health,
    }
    with open(output_dir / "codebook_health.json", "w") as f:
        json.dump(results, f, indent=2)
    print(f"Results saved to {output_dir}/codebook_health.json")
    return 0


def make_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Evaluate codebook health")
    parser.add_argument("--experiment", required=True, help="Experiment directory")
    parser.add_argument("--dataset", default="fashionmnist", help="Dataset name")
    parser.add_argument("--batch_size", type=int, default=512, help="Batch size for inference")
    parser.add_argument("--n_vis", type=int, default=32, help="Number of samples for visualization (unused, as in the reference)")
    add_experiment_args(parser)
    return parser


if __name__ == "__main__":
    raise SystemExit(main())
