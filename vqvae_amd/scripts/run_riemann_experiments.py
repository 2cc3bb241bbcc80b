"""Effect of replacing Euclidean edge weights with Riemannian lengths in the kNN graph (the reference's
experiments/geo/run_riemann_experiments.py).

    python -m vqvae_amd.scripts.run_riemann_experiments [--dataset mnist|cifar10|fashionmnist]
        [--latents_path z.pt] [--checkpoint_path best.pt] [--out_dir DIR]
        [--k 10] [--mode subset|full] [--sample_edges 5000] [--num_bins 5] [--num_sources 8] [--seed 0]

The defaults are the reference's hard-coded values.  Writes graph_effects_<dataset>.npz (the reference's keys) and
graph_effects_<dataset>.png under experiments/geo/riemann_graph_effects/<dataset> (or --out_dir).  The work is
vqvae_amd.geo.experiments.riemann_graph_effects.
"""
import argparse
import os

import numpy as np

from .riemann_sanity_check import BATCH_SIZE, DATASET_CONFIGS, load_latents, resolve_paths  # noqa: F401

K_NEIGHBORS = 10
REWEIGHT_MODE = "subset"
SAMPLE_EDGES = 5000
NUM_BINS = 5
NUM_SOURCES = 8
SEED = 0
SAVED_KEYS = ("ncomp_euc", "lcc_size_euc", "mean_sp_euc", "ncomp_riem", "lcc_size_riem", "mean_sp_riem", "ratio_sp",
              "reweight_mode", "sample_edges", "k", "num_sources")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Riemannian graph effects analysis")
    p.add_argument("--dataset", choices=["mnist", "cifar10", "fashionmnist"], default="mnist",
                   help="Dataset to use for analysis")
    p.add_argument("--latents_path", type=str, default=None, help="Latents file (default: the dataset's path)")
    p.add_argument("--checkpoint_path", type=str, default=None, help="VAE checkpoint (default: the dataset's path)")
    p.add_argument("--out_dir", type=str, default=None,
                   help="Output directory (default: experiments/geo/riemann_graph_effects/<dataset>)")
    p.add_argument("--k", type=int, default=K_NEIGHBORS, help="Neighbours of the mutual kNN graph")
    p.add_argument("--mode", choices=["subset", "full"], default=REWEIGHT_MODE, help="Re-weight a stratified sample or every edge")
    p.add_argument("--sample_edges", type=int, default=SAMPLE_EDGES, help="Edges re-weighted in subset mode")
    p.add_argument("--num_bins", type=int, default=NUM_BINS, help="Quantile bins of the stratified sample")
    p.add_argument("--num_sources", type=int, default=NUM_SOURCES, help="Shortest-path sources drawn from the LCC")
    p.add_argument("--seed", type=int, default=SEED, help="Seed of the source pick and the edge sample")
    return p.parse_args(argv)


def run_experiment(args):
    from .._device import device
    from ..geo.experiments import riemann_graph_effects
    from ..utils.checkpoint_utils import get_vae_decoder
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    latents_path, checkpoint_path, out_dir = resolve_paths(args, "riemann_graph_effects")
    out_dir.mkdir(parents=True, exist_ok=True)
    print(f"Loading latents from: {latents_path}")
    z = load_latents(latents_path).cpu()
    N, D = z.shape[0], z.shape[1]
    print(f"Loaded {N} latent vectors of dimension {D}")
    decoder = get_vae_decoder(checkpoint_path, latent_dim=D, device=device())
    if decoder is None:
        print("Cannot load decoder. Exiting.")
        return None
    print(f"Building k-NN graph with k={args.k}")
    res = riemann_graph_effects(z, decoder, k=args.k, mode=args.mode, sample_edges=args.sample_edges, num_bins=args.num_bins,
                                num_sources=args.num_sources, seed=args.seed, batch_size=BATCH_SIZE)
    print(f"[Euclidean] components={res['ncomp_euc']}, LCC size={res['lcc_size_euc']}, mean_sp={res['mean_sp_euc']:.4f}")
    if args.mode == "full":
        print(f"Re-weighting ALL {res['sample_edges']} edges")
    else:
        print(f"Re-weighting {res['sample_edges']} edges (stratified sampling)")
    print(f"[Riemann]  components={res['ncomp_riem']}, LCC size={res['lcc_size_riem']}, mean_sp={res['mean_sp_riem']:.4f}")
    print(f"[Effect]   mean shortest-path ratio (Riem/Eucl) = {res['ratio_sp']:.3f}")

    out_npz = os.path.join(out_dir, f"graph_effects_{args.dataset}.npz")
    np.savez(out_npz, **{key: res[key] for key in SAVED_KEYS}, dataset=args.dataset)
    print(f"Saved metrics to: {out_npz}")

    plt.figure(figsize=(5, 4))
    plt.bar(["Euclidean", "Riemann"], [res["mean_sp_euc"], res["mean_sp_riem"]])
    plt.ylabel("Mean shortest-path distance")
    plt.title(f"{args.dataset.upper()} - k={args.k}, mode={args.mode}, edges={res['sample_edges']}")
    plt.tight_layout()
    out_png = os.path.join(out_dir, f"graph_effects_{args.dataset}.png")
    plt.savefig(out_png, dpi=150)
    plt.close()
    print(f"Saved plot to: {out_png}")
    return res


def main(argv=None):
    args = parse_args(argv)
    print(f"Running Riemann graph effects analysis on {args.dataset.upper()} dataset")
    return run_experiment(args)


if __name__ == "__main__":
    main()
