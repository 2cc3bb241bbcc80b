"""VAE reconstruction quality on the MI355X: drop-in for the reference's src/eval/evaluate_vae_quality.py (same flags, same
vae/vae_quality_assessment.json: keys, quality thresholds, exit code 0 = proceed, 1 = retrain or error).

    python -m vqvae_amd.scripts.evaluate_vae_quality --experiment experiments/fashionmnist/vanilla/geodesic \
        [--config configs/.../vae.yaml]

Decodes the validation latents z and mu (the first --max_samples), post-processes both as the reference does and compares
them per image with geo_image_pair_moments on the device.  The decoder's architecture comes from the config's `model`
section, as in the reference; whether the checkpoint holds a vanilla or a spatial decoder is read from its state dict
(vqvae_amd.eval.experiment; --vae_ckpt_path / --latents_path override the files).
"""
import argparse
import json
from pathlib import Path

import torch
import yaml

from .._device import device
from ..eval.experiment import detect_layout, latents_file
from ..eval.reconstruction import decode_pair_moments, metrics_from_moments
from ..spatial_decoder import SpatialDecoder
from ..vae import decoder_from_vae_checkpoint


def load_config(config_path: str) -> dict:
    with open(config_path, "r") as f:
        return yaml.safe_load(f) or {}


def load_decoder_from_config(checkpoint_path, vae_config: dict, layout: str, dev):
    """(decoder in eval mode, epoch) with the architecture of the config's model section (the reference's defaults)."""
    ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    state = ckpt["model_state_dict"]
    arch = dict(in_channels=int(vae_config.get("in_channels", 1)),
                dec_channels=tuple(vae_config.get("dec_channels", [256, 128, 64])),
                latent_dim=int(vae_config.get("latent_dim", 128)),
                output_image_size=int(vae_config.get("output_image_size", 28)),
                norm_type=str(vae_config.get("norm_type", "batch")))
    if layout == "spatial":
        dec = SpatialDecoder(arch["in_channels"], arch["dec_channels"], arch["latent_dim"], arch["output_image_size"],
                             arch["norm_type"])
        dec.load_state_dict({k[len("decoder."):]: v for k, v in state.items() if k.startswith("decoder.")})
    else:
        dec = decoder_from_vae_checkpoint(state, **arch)
    return dec.to(dev).eval(), ckpt.get("epoch", "unknown")


def assess_quality(psnr_value: float, ssim_value: float):
    if psnr_value > 20:
        return "excellent", True
    if psnr_value > 15:
        return "good", True
    if psnr_value > 10:
        return "acceptable", True
    return "poor", False


def main(argv=None) -> int:
    args = make_parser().parse_args(argv)
    dev = device()
    if args.config:
        config_path = args.config
    else:
        config_path = f"{args.experiment}/../../configs/sandbox-fashion/euclidean/vae.yaml"
        if not Path(config_path).exists():
            config_path = "configs/sandbox-fashion/euclidean/vae.yaml"
    try:
        config = load_config(config_path)
        vae_cfg = config.get("model", {})
        data_cfg = config.get("data", {})
    except Exception as e:  # noqa: BLE001 -- the reference reports any failure to read the config the same way
        print(f"Error loading config from {config_path}: {e}")
        return 1
    dataset_name = data_cfg.get("name", "Unknown")

    try:
        paths = detect_layout(args.experiment, args.vae_ckpt_path, args.latents_path, codebook_path=None)
        decoder, epoch = load_decoder_from_config(paths.vae_ckpt, vae_cfg, paths.layout, dev)
    except Exception as e:  # noqa: BLE001
        print(f"Error loading checkpoint: {e}")
        return 1

    try:
        mu_val = torch.load(latents_file(paths, "mu"), map_location="cpu").float()
        z_val = torch.load(latents_file(paths, "z"), map_location="cpu").float()
    except Exception as e:  # noqa: BLE001
        print(f"Error loading latents: {e}")
        return 1

    apply_sigmoid = str(vae_cfg.get("recon_loss", "mse")).lower() == "bce" or bool(vae_cfg.get("mse_use_sigmoid", True))
    n = min(len(z_val), len(mu_val), args.max_samples)
    mom = decode_pair_moments(decoder, z_val, mu_val, dataset=str(dataset_name), apply_sigmoid=apply_sigmoid,
                              batch_size=args.batch_size, n_samples=n)
    z_mu_psnr, z_mu_ssim = metrics_from_moments(mom["a_b"], mom["n_pix"])
    print(f"PSNR: {z_mu_psnr:.2f} dB, SSIM: {z_mu_ssim:.4f}")
    quality, proceed = assess_quality(z_mu_psnr, z_mu_ssim)
    print(f"Quality: {quality.upper()}")
    print(f'Recommendation: {"PROCEED" if proceed else "RETRAIN"}')

    results = {
        "dataset": dataset_name,
        "checkpoint_epoch": epoch,
        "psnr_db": float(z_mu_psnr),
        "ssim": float(z_mu_ssim),
        "quality_rating": quality,
        "recommendation": "proceed" if proceed else "retrain",
        "samples_evaluated": min(len(mu_val), args.max_samples),
    }
    output_file = Path(args.experiment) / "vae" / "vae_quality_assessment.json"
    output_file.parent.mkdir(parents=True, exist_ok=True)
    with open(output_file, "w") as f:
        json.dump(results, f, indent=2)
    print(f"Results saved to {output_file}")
    return 0 if proceed else 1


def make_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Evaluate VAE reconstruction quality")
    parser.add_argument("--experiment", required=True, help="Experiment directory")
    parser.add_argument("--config", help="Config file path (auto-detected if not provided)")
    parser.add_argument("--max_samples", type=int, default=1000, help="Max samples to evaluate")
    parser.add_argument("--batch_size", type=int, default=512, help="Batch size for inference")
    parser.add_argument("--vae_ckpt_path", type=str, default=None, help="Checkpoint (default: detected under --experiment)")
    parser.add_argument("--latents_path", type=str, default=None, help="z.pt, with mu.pt next to it (default: detected)")
    return parser


if __name__ == "__main__":
    raise SystemExit(main())
