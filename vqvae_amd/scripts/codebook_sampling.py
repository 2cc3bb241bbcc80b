"""Reconstruction grid of a built codebook: drop-in for the reference's demos/codebook_sampling.py.

    python -m vqvae_amd.scripts.codebook_sampling <experiment_dir> [--num_samples 16] [--seed 42]
        [--out reconstruction_grid_quantized.png] [--out_dir DIR] [--atlas FILE]

Top row: the decoder's reconstructions of `num_samples` validation latents; bottom row: the same samples quantized to the
codebook's medoids.  As the reference: the samples are np.sort(RandomState(seed).choice(N, min(num, N), replace=False));
codebook/codes.npy is used when its shape matches the latents ((N,) for vector latents, (N, h, w) for grids), else the
Euclidean nearest medoid; the sigmoid is applied when recon_loss == "bce" or mse_use_sigmoid, RGB without a sigmoid gets the
CIFAR-10 un-normalisation and a clamp; the grid has nrow = number of samples; a missing directory or a dimension mismatch
prints the reference's message and returns.

Both rows are decoded on the GPU by vqvae_amd.decode.decode_images: the top row from z, the bottom row from
table = z_medoid and the codes, so no quantized latent is materialised.  The experiment's files are found by
eval.experiment.detect_layout (the path and spatial-architecture overrides of add_experiment_args apply).

Which activation the images get is decided as the reference decides it: from the checkpoint's "config" (or "model_config")
entry, recon_loss defaulting to "mse" and mse_use_sigmoid to True; a checkpoint without one is treated as the reference's
inferred config, mse with mse_use_sigmoid = (in_channels == 1) -- so an RGB checkpoint without a config gets the CIFAR-10
un-normalisation, not a sigmoid.

Differences, deliberate:
  - between the checkpoint's config and that inference, the config build_codebook recorded in codebook.pt is consulted (the
    reference knows no such record), and --recon_loss / --mse_use_sigmoid override everything;
  - latents whose kind (vector or grid) does not match the checkpoint's decoder print a message and return; the reference
    fails inside the decoder;
  - with fewer than --num_samples latents the reference's reshape of the nearest-medoid indices raises; here the count is
    len(idx) everywhere;
  - the nearest-medoid fallback is the exact fp64 assignment (eval.reconstruction.nearest_medoid_assign), not the float32
    a^2 + b^2 - 2ab argmin: the two differ only on near-ties;
  - --atlas FILE (added) also writes every codebook entry decoded: for a vector codebook the K medoid images, for a spatial
    codebook the 4x4 grid filled with one code, decoded through the codes path.
"""
import argparse
import math
from pathlib import Path

import numpy as np
import torch

from ..eval.experiment import add_experiment_args, detect_layout, load_decoder
from .generate_samples import save_image


def select_indices(N: int, num: int, seed: int) -> np.ndarray:
    rng = np.random.RandomState(seed)
    return np.sort(rng.choice(N, size=min(num, N), replace=False))


def activation_config(ckpt_cfg, recorded, in_channels: int, recon_loss=None, mse_use_sigmoid=None):
    """(apply_sigmoid, is_rgb) as the reference's demo decides them (module docstring).  ckpt_cfg: the checkpoint's "config" /
    "model_config" dict or None; recorded: codebook.pt's "config" dict or None; recon_loss / mse_use_sigmoid: the flags."""
    if ckpt_cfg is None:
        recorded = recorded or {}
        ckpt_cfg = {"in_channels": in_channels, "recon_loss": recorded.get("recon_loss", "mse"),
                    "mse_use_sigmoid": recorded.get("mse_use_sigmoid", in_channels == 1)}
    loss = str(recon_loss if recon_loss is not None else ckpt_cfg.get("recon_loss", "mse")).lower()
    use = bool(mse_use_sigmoid if mse_use_sigmoid is not None else ckpt_cfg.get("mse_use_sigmoid", True))
    return loss == "bce" or use, ckpt_cfg.get("in_channels", 1) == 3


def save_grid(x_top: torch.Tensor, x_bottom: torch.Tensor, path: str) -> None:
    """The reference's grid: (B, C, H, W) images in [0, 1], x_top in the first row and x_bottom below (nrow = B), padding 2:
    for S-px images and m samples a PNG of (m (S + 2) + 2) x (2 (S + 2) + 2)."""
    save_image(torch.cat([x_top, x_bottom], dim=0).cpu(), path, nrow=x_top.size(0))


def _parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Reconstruction grid from codebook")
    p.add_argument("experiment_dir", type=str,
                   help="Path to experiment directory (e.g., experiments/fashionmnist/vanilla/euclidean)")
    p.add_argument("--num_samples", type=int, default=16, help="Number of samples to visualize")
    p.add_argument("--seed", type=int, default=42, help="Random seed for sample selection")
    p.add_argument("--out", type=str, default="reconstruction_grid_quantized.png", help="Output filename")
    p.add_argument("--out_dir", type=str, default="", help="Optional output directory (default: codebook_dir)")
    p.add_argument("--atlas", type=str, default=None, help="Also write every codebook entry decoded to this file")
    add_experiment_args(p)
    return p


def _find_paths(args):
    """The reference's auto_detect_paths messages, the package's layout detection."""
    exp = Path(args.experiment_dir)
    codebook_dir = Path(args.codebook_path).parent if args.codebook_path else exp / "codebook"
    if not codebook_dir.exists():
        raise FileNotFoundError(f"Codebook directory not found: {codebook_dir}")
    if args.vae_ckpt_path is None and not (exp / "vae").exists():
        raise FileNotFoundError(f"VAE directory not found: {exp / 'vae'}")
    paths = detect_layout(str(exp), args.vae_ckpt_path, args.latents_path, args.codebook_path)
    if not paths.latents.exists():
        raise FileNotFoundError(f"Validation latents not found in: {exp / 'vae'}")
    return codebook_dir, paths


def main(argv=None) -> None:
    args = _parser().parse_args(argv)
    try:
        codebook_dir, paths = _find_paths(args)
        print("Auto-detected paths:")
        print(f"  Codebook: {codebook_dir}")
        print(f"  Checkpoint: {paths.vae_ckpt}")
        print(f"  Latents: {paths.latents}")
    except FileNotFoundError as e:
        print(f"Error: {e}")
        return

    codebook = torch.load(paths.codebook, map_location="cpu", weights_only=False)
    z_medoid = codebook["z_medoid"].float()                      # (K, D)
    z = torch.load(paths.latents, map_location="cpu")
    if isinstance(z, dict) and "z" in z:
        z = z["z"]
    z = z.float()                                                # (N, D) or (N, C, H, W)

    spatial = z.dim() == 4
    print(f"Detected {'spatial' if spatial else 'vanilla'} latents: {tuple(z.shape)}")
    if z.shape[1] != z_medoid.shape[-1]:
        print("ERROR: Dimensional mismatch!")
        print(f"  Latents dimension: {z.shape[1]} ({'spatial shape' if spatial else 'shape'}: {tuple(z.shape)})")
        print(f"  Codebook dimension: {z_medoid.shape[-1]} (shape: {tuple(z_medoid.shape)})")
        print("\nEnsure latents and codebook come from compatible experiments.")
        return

    if spatial != (paths.layout == "spatial"):
        print(f"ERROR: {'grid' if spatial else 'vector'} latents {tuple(z.shape)} with the {paths.layout} decoder of {paths.vae_ckpt}")
        print("\nEnsure latents and checkpoint come from the same experiment.")
        return

    idx = select_indices(N=z.shape[0], num=args.num_samples, seed=args.seed)
    z_sel = z[torch.from_numpy(idx)]
    medoid_idx = None
    if paths.codes.exists():
        codes = np.load(paths.codes)
        if spatial and codes.shape == (z.shape[0], z.shape[2], z.shape[3]):
            print("Using precomputed spatial geodesic assignments from codes.npy")
            medoid_idx = torch.from_numpy(codes[idx].astype(np.int64))
        elif not spatial and codes.shape == (z.shape[0],):
            print("Using precomputed geodesic assignments from codes.npy")
            medoid_idx = torch.from_numpy(codes[idx].astype(np.int64))

    from .._device import device as gpu
    from ..decode import decode_images, native_decode_covers
    from ..eval.reconstruction import nearest_medoid_assign
    from ..spatial_decoder import SpatialImageDecoderExport
    from ..vanilla_decoder import VanillaDecoderExport
    dev = gpu()
    if medoid_idx is None:
        print("Computing nearest medoids using Euclidean distance for visualization")
        z_dev = z_sel.to(dev)
        if spatial:
            rows = z_dev.permute(0, 2, 3, 1).reshape(-1, z.shape[1])
            medoid_idx = nearest_medoid_assign(rows, z_medoid.to(dev)).view(len(idx), z.shape[2], z.shape[3])
        else:
            medoid_idx = nearest_medoid_assign(z_dev, z_medoid.to(dev))

    recorded = codebook.get("config") if isinstance(codebook, dict) else None
    decoder, vae_cfg = load_decoder(paths, args, dev, codebook if isinstance(codebook, dict) else None)
    ckpt = torch.load(paths.vae_ckpt, map_location="cpu", weights_only=False)
    ckpt_cfg = (ckpt.get("config") or ckpt.get("model_config")) if isinstance(ckpt, dict) else None
    apply_sigmoid, is_rgb = activation_config(ckpt_cfg, recorded, int(vae_cfg.get("in_channels") or 1), args.recon_loss,
                                              args.mse_use_sigmoid)
    if is_rgb and not apply_sigmoid:
        print("Applying CIFAR-10 denormalization (RGB + no sigmoid activation)")
    dataset = "CIFAR10" if is_rgb else "other"      # unnormalize_images: CIFAR-10 statistics exactly for RGB without sigmoid

    # one snapshot of the decoder for every decode below; a module outside the kernels' coverage decodes itself
    model = decoder
    if native_decode_covers(decoder):
        model = (SpatialImageDecoderExport if paths.layout == "spatial" else VanillaDecoderExport)(decoder, dev)
    table = z_medoid.to(dev)
    x_orig = decode_images(model, z_sel.to(dev), dataset=dataset, apply_sigmoid=apply_sigmoid)
    x_quant = decode_images(model, table=table, codes=medoid_idx.to(dev), dataset=dataset, apply_sigmoid=apply_sigmoid)

    base_out_dir = Path(args.out_dir) if args.out_dir else codebook_dir
    base_out_dir.mkdir(parents=True, exist_ok=True)
    out_path = base_out_dir / args.out
    save_grid(x_orig, x_quant, str(out_path))
    print(f"Saved reconstruction grid to: {out_path}")

    if args.atlas:
        K = table.shape[0]
        every = torch.arange(K, device=dev)
        if spatial:
            every = every.view(K, 1, 1).expand(K, z.shape[2], z.shape[3]).contiguous()
        atlas = decode_images(model, table=table, codes=every, dataset=dataset, apply_sigmoid=apply_sigmoid)
        atlas_path = Path(args.atlas) if Path(args.atlas).is_absolute() else base_out_dir / args.atlas
        save_image(atlas.cpu(), str(atlas_path), nrow=int(math.ceil(math.sqrt(K))))
        print(f"Saved the decoded codebook ({K} entries) to: {atlas_path}")


if __name__ == "__main__":
    main()
