"""Quantization loss on the MI355X: drop-in for the reference's src/eval/evaluate_quantization_loss.py (same flags, same
evaluation/quantization_analysis.json: keys, rounding, assessment thresholds, exit codes).

    python -m vqvae_amd.scripts.evaluate_quantization_loss --experiment experiments/fashionmnist/vanilla/geodesic \
        --dataset fashionmnist [--data_root data] [--seed S]

Real test images come from the files torchvision leaves under --data_root (vqvae_amd.eval.data); nothing is downloaded.
Decode, post-processing and the per-image reductions run on the device (vqvae_amd.eval.reconstruction).

Reference quirks kept on purpose (this is a drop-in):
  - unnormalize_images is applied to the real images too, so they go through a sigmoid when apply_sigmoid;
  - codebook/codes.npy is reused when it exists, although those are the codes of the training latents; only without it are
    the validation latents assigned (then by geo_kmeans_assign, exact fp64 key);
  - the real samples are an unseeded torch.randperm of the test split.  --seed S draws the permutation from a generator
    seeded with S instead; without it the behaviour is the reference's.
"""
import argparse
import json
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from .._device import device
from ..eval.data import load_test_split, to_tensor
from ..eval.experiment import add_experiment_args, detect_layout, load_decoder
from ..eval.reconstruction import decode_pair_moments, last_assign_path, metrics_from_moments, quantize, unnormalize_images


def load_dataset_samples(dataset_name: str, num_samples: int = 1000, root: str = "data",
                         seed: Optional[int] = None) -> torch.Tensor:
    """num_samples test images (N, 3, H, W) in [0, 1] in the order of torch.randperm (seeded when seed is given)."""
    images, _ = load_test_split(dataset_name, root)
    gen = torch.Generator().manual_seed(seed) if seed is not None else None
    indices = torch.randperm(len(images), generator=gen)[:num_samples]
    return torch.stack([to_tensor(images[int(i)]) for i in indices])


def assessment_of(cont_quant_psnr: float) -> str:
    if cont_quant_psnr > 25:
        return "EXCELLENT"
    if cont_quant_psnr > 20:
        return "GOOD"
    if cont_quant_psnr > 15:
        return "MODERATE"
    return "HIGH"


def main(argv=None) -> int:
    args = make_parser().parse_args(argv)
    dev = device()
    experiment_dir = Path(args.experiment)
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
        print(f"Error loading latents/codebook: {e}")
        return 1

    z_dev, zm_dev = z_val.to(dev), z_medoid.to(dev)
    if paths.codes.exists():                                   # the reference's quirk: training codes, reused as they are
        codes = torch.from_numpy(np.load(paths.codes).reshape(-1)).long().to(dev)
        zq_val = zm_dev[codes]
        if z_dev.dim() == 4:
            _, C, h, w = z_dev.shape
            zq_val = zq_val.view(-1, h, w, C).permute(0, 3, 1, 2).contiguous()
        print(f"Codes from {paths.codes}")
    else:
        codes, zq_val = quantize(z_dev, zm_dev)
        print(f"Assigned {codes.numel()} latents ({paths.layout}, assignment: {last_assign_path()})")

    try:
        x_real = load_dataset_samples(args.dataset, args.max_samples, args.data_root, args.seed)
        if vae_config["in_channels"] == 1 and x_real.size(1) == 3:
            x_real = x_real.mean(dim=1, keepdim=True)
        elif vae_config["in_channels"] == 3 and x_real.size(1) == 1:
            x_real = x_real.repeat(1, 3, 1, 1)
    except (OSError, ValueError) as e:
        print(f"Error loading dataset: {e}")
        return 1

    recon_loss = vae_config.get("recon_loss", "mse").lower()
    mse_use_sigmoid = vae_config.get("mse_use_sigmoid", True)
    apply_sigmoid = (recon_loss == "bce") or mse_use_sigmoid

    n_samples = min(len(z_val), args.max_samples)
    x_real = unnormalize_images(x_real[:n_samples].to(dev), args.dataset, apply_sigmoid)
    mom = decode_pair_moments(vae, z_dev, zq_val, dataset=args.dataset, apply_sigmoid=apply_sigmoid,
                              batch_size=args.batch_size, n_samples=n_samples, x_real=x_real)
    P = mom["n_pix"]
    (p_rc, s_rc), (p_rq, s_rq), (p_cq, s_cq) = (metrics_from_moments(mom[k], P) for k in ("real_a", "real_b", "a_b"))

    metrics = {
        "dataset": args.dataset,
        "samples_evaluated": n_samples,
        "codebook_size": int(z_medoid.shape[0]),
        "psnr_real_vs_continuous": float(f"{p_rc:.6f}"),
        "psnr_real_vs_quantized": float(f"{p_rq:.6f}"),
        "psnr_continuous_vs_quantized": float(f"{p_cq:.6f}"),
        "ssim_real_vs_continuous": float(f"{s_rc:.6f}"),
        "ssim_real_vs_quantized": float(f"{s_rq:.6f}"),
        "ssim_continuous_vs_quantized": float(f"{s_cq:.6f}"),
    }
    print(f"Real vs Continuous: PSNR {metrics['psnr_real_vs_continuous']:.2f} dB, SSIM {metrics['ssim_real_vs_continuous']:.4f}")
    print(f"Real vs Quantized: PSNR {metrics['psnr_real_vs_quantized']:.2f} dB, SSIM {metrics['ssim_real_vs_quantized']:.4f}")
    print(f"Continuous vs Quantized: PSNR {metrics['psnr_continuous_vs_quantized']:.2f} dB, "
          f"SSIM {metrics['ssim_continuous_vs_quantized']:.4f}")
    assessment = assessment_of(metrics["psnr_continuous_vs_quantized"])
    print(f"Quantization loss: {assessment}")

    output_dir = experiment_dir / "evaluation"
    output_dir.mkdir(parents=True, exist_ok=True)
    with open(output_dir / "quantization_analysis.json", "w") as f:
        json.dump(metrics, f, indent=2)
    print(f"Results saved to {output_dir}/quantization_analysis.json")
    return 0


def make_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Evaluate quantization loss")
    parser.add_argument("--experiment", required=True, help="Experiment directory")
    parser.add_argument("--dataset", default="fashionmnist", help="Dataset name")
    parser.add_argument("--batch_size", type=int, default=512, help="Batch size for inference")
    parser.add_argument("--max_samples", type=int, default=1000, help="Maximum samples to evaluate")
    parser.add_argument("--data_root", default="data", help="Where torchvision left the test split (nothing is downloaded)")
    parser.add_argument("--seed", type=int, default=None, help="Seed of the real-sample permutation (default: unseeded)")
    add_experiment_args(parser)
    return parser


if __name__ == "__main__":
    raise SystemExit(main())
