"""Sanity check: Riemannian vs Euclidean lengths on kNN entries (the reference's experiments/geo/riemann_sanity_check.py).

    python -m vqvae_amd.scripts.riemann_sanity_check [--dataset mnist|cifar10|fashionmnist]
        [--latents_path z.pt] [--checkpoint_path best.pt] [--out_dir DIR]

Reads the dataset's latents and VAE checkpoint (the reference's paths, relative to the working directory), draws 2 000
stored entries of the k=10 mutual kNN graph and writes sanity_stats_<dataset>.npz (corr, ratio, de, dr, dataset,
decoder_type) and riemann_analysis_<dataset>.png under experiments/geo/riemann_sanity/<dataset> (or --out_dir).
The work is vqvae_amd.geo.experiments.riemann_sanity.
"""
import argparse
import os
from pathlib import Path

import numpy as np
import torch

DATASET_CONFIGS = {
    "mnist": {
        "latents_path": "experiments/vae_mnist/latents_val/z.pt",
        "checkpoint_path": "experiments/vae_mnist/checkpoints/best.pt",
    },
    "cifar10": {
        "latents_path": "experiments/cifar10/vanilla/euclidean/vae/latents_val/z.pt",
        "checkpoint_path": "experiments/cifar10/vanilla/euclidean/vae/checkpoints/best.pt",
    },
    "fashionmnist": {
        "latents_path": "experiments/fashionmnist/vanilla/euclidean/vae/latents_val/z.pt",
        "checkpoint_path": "experiments/fashionmnist/vanilla/euclidean/vae/checkpoints/best.pt",
    },
}
K_NEIGHBORS = 10
MAX_EDGES = 2000
SEED = 0
BATCH_SIZE = 256


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Riemannian vs Euclidean distance sanity check")
    p.add_argument("--dataset", choices=["mnist", "cifar10", "fashionmnist"], default="mnist",
                   help="Dataset to use for analysis")
    p.add_argument("--latents_path", type=str, default=None, help="Latents file (default: the dataset's path)")
    p.add_argument("--checkpoint_path", type=str, default=None, help="VAE checkpoint (default: the dataset's path)")
    p.add_argument("--out_dir", type=str, default=None,
                   help="Output directory (default: experiments/geo/riemann_sanity/<dataset>)")
    return p.parse_args(argv)


def load_latents(latent_path) -> torch.Tensor:
    """A tensor, or a dict with a 'z' entry (riemann_sanity_check.py:39-48)."""
    pth = Path(latent_path)
    if pth.exists():
        obj = torch.load(pth, map_location="cpu")
        if isinstance(obj, dict) and "z" in obj:
            return obj["z"].float()
        if torch.is_tensor(obj):
            return obj.float()
    raise FileNotFoundError(f"Latents not found at: {latent_path}")


def resolve_paths(args, experiment: str):
    cfg = DATASET_CONFIGS[args.dataset]
    out_dir = Path(args.out_dir) if args.out_dir else Path("experiments") / "geo" / experiment / args.dataset
    return args.latents_path or cfg["latents_path"], args.checkpoint_path or cfg["checkpoint_path"], out_dir


def run_experiment(args):
    from .._device import device
    from ..geo.experiments import riemann_sanity, sample_knn_entries
    from ..utils.checkpoint_utils import get_vae_decoder
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    latents_path, checkpoint_path, out_dir = resolve_paths(args, "riemann_sanity")
    out_dir.mkdir(parents=True, exist_ok=True)
    print(f"Loading latents from: {latents_path}")
    z = load_latents(latents_path).cpu()
    N, D = z.shape[0], z.shape[1]
    print(f"Loaded {N} latent vectors of dimension {D}")
    print(f"Building k-NN graph with k={K_NEIGHBORS}")
    sample = sample_knn_entries(z, k=K_NEIGHBORS, max_edges=MAX_EDGES, seed=SEED)
    print(f"Sampled {len(sample['indices'])} edges from k-NN graph")
    decoder = get_vae_decoder(checkpoint_path, latent_dim=D, device=device())
    if decoder is None:
        print("Cannot load decoder. Exiting.")
        return None
    res = riemann_sanity(z, decoder, batch_size=BATCH_SIZE, sample=sample)
    de, dr = res["de"], res["dr"]
    corr, mean_ratio = res["corr"], res["ratio"]
    np.savez(os.path.join(out_dir, f"sanity_stats_{args.dataset}.npz"), corr=corr, ratio=mean_ratio, de=de, dr=dr,
             dataset=args.dataset, decoder_type=f"real_VAE_{args.dataset.upper()}")
    print(f"Results: correlation={corr:.3f}, mean_ratio={mean_ratio:.3f}")

    ratios = dr / (de + 1e-8)
    fig, (ax1, ax2) = plt.subplots(1, 2, figsize=(10, 5))
    ax1.scatter(de, dr, s=6, alpha=0.6)
    ax1.set_xlabel("Euclidean edge length")
    ax1.set_ylabel("Riemannian edge length")
    ax1.set_title(f"{args.dataset.upper()} - Riemannian vs Euclidean (k={K_NEIGHBORS})")
    ax2.hist(ratios, bins=50)
    ax2.set_xlabel("Ratio Riemannian / Euclidean")
    ax2.set_ylabel("Count")
    ax2.set_title("Distribution of length ratios")
    plt.tight_layout()
    plot_path = os.path.join(out_dir, f"riemann_analysis_{args.dataset}.png")
    plt.savefig(plot_path, dpi=150)
    plt.close(fig)
    print(f"Analysis complete! Plots saved to: {plot_path}")
    return res


def main(argv=None):
    args = parse_args(argv)
    print(f"Running Riemann sanity check on {args.dataset.upper()} dataset")
    return run_experiment(args)


if __name__ == "__main__":
    main()
