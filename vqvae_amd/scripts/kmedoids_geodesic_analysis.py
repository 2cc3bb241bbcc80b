"""Geodesic k-medoids analysis on the GPU: choosing K (the reference's demos/kmedoids_geodesic_analysis.py).

    python -m vqvae_amd.scripts.kmedoids_geodesic_analysis <experiment_dir> [--k_graph 10] [--graph_sym mutual]
        [--K_values 32,64,128] [--inits kpp,random] [--seed 42] [--out_dir DIR]

Reads `vae/**/latents_val/z.pt` (and `y.pt` when present) under experiment_dir and writes metrics.csv, metrics.json,
elbow.png, pca_clusters_*.png and code_usage_*.png into demo_outputs/kmedoids_geodesic_<timestamp> (or --out_dir), with the
reference's columns and keys.  One kNN graph; per init ONE fit_kmedoids_path over all K (a single seeding chain for "kpp");
purity / NMI / ARI / perplexity from geo_cluster_label_scores; the finite fraction from the chain's d_min; one K x N solve
and its PCA (geo_feature_*) for the plotted configuration, the first (K, init), only.
"""
import argparse
import csv
import json
from datetime import datetime
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import torch

KEYS = ("graph", "K", "init", "seed", "qe_geo_finite", "finite_fraction", "purity", "nmi", "ari", "perplexity")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Geodesic K-medoids clustering analysis")
    p.add_argument("experiment_dir", type=str,
                   help="Path to experiment directory (e.g., experiments/fashionmnist/vanilla/euclidean)")
    p.add_argument("--k_graph", type=int, default=10, help="k-NN graph connectivity (default: 10)")
    p.add_argument("--graph_sym", type=str, choices=["mutual", "union"], default="mutual",
                   help="Graph symmetrization (default: mutual)")
    p.add_argument("--K_values", type=str, default="32,64,128", help="Comma-separated codebook sizes (default: 32,64,128)")
    p.add_argument("--inits", type=str, default="kpp,random", help="Comma-separated initialization methods (default: kpp,random)")
    p.add_argument("--seed", type=int, default=42, help="Random seed (default: 42)")
    p.add_argument("--out_dir", type=str, default=None,
                   help="Output directory (default: demo_outputs/kmedoids_geodesic_<timestamp>)")
    return p.parse_args(argv)


def auto_detect_paths(experiment_dir) -> dict:
    vae_dir = Path(experiment_dir) / "vae"
    if not vae_dir.exists():
        raise FileNotFoundError(f"VAE directory not found: {vae_dir}")
    latents = list(vae_dir.rglob("latents_val/z.pt"))
    if not latents:
        raise FileNotFoundError(f"Validation latents not found in: {vae_dir}")
    labels = list(vae_dir.rglob("latents_val/y.pt"))
    return {"latents_path": latents[0], "labels_path": labels[0] if labels else None}


def load_latents(path: Path) -> np.ndarray:
    obj = torch.load(path, map_location="cpu")
    if isinstance(obj, dict) and "z" in obj:
        z = obj["z"].float().numpy()
    elif torch.is_tensor(obj):
        z = obj.float().numpy()
    else:
        raise ValueError("Unsupported latent file format")
    if z.ndim != 2:
        raise ValueError(f"z must be 2D (N,D). Got shape={z.shape}")
    return z


def load_labels(path: Path) -> Optional[np.ndarray]:
    if not path.exists():
        return None
    obj = torch.load(path, map_location="cpu")
    return obj.numpy() if torch.is_tensor(obj) else None


def _pyplot():
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        return plt
    except ImportError:
        return None


def evaluate_setup(W, K_values: List[int], inits: List[str], seed: int, labels: Optional[np.ndarray], out_dir: Path,
                   tag: str, plt=None) -> List[Dict]:
    """The demo's evaluate_setup: one row per (K, init), K outermost; plots for the first (K, init)."""
    from .._device import DeviceCSR, device
    from ..geo.analysis import clustering_scores, distance_feature_pca, perplexity_from_counts
    from ..geo.geo_shortest_paths import _pull_structure, ensure_valid_graph, sssp_multi_device
    from ..geo.kmeans_optimized import fit_kmedoids_path
    dev = device()
    G = DeviceCSR.from_scipy(_pull_structure(ensure_valid_graph(W), directed=False), dev)
    y_dev = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels).astype(np.int32)).to(dev)
    rows = {}
    for init in inits:
        info = {}
        fits = fit_kmedoids_path(G, K_values, init=init, seed=seed, info=info)
        print(f"[demo] init={init}: {len(K_values)} codebook sizes from {info['solves']} solves")
        for K, (medoids, assign, qe), frac in zip(K_values, fits, info["finite_fraction"]):
            purity = nmi = ari = float("nan")
            if y_dev is not None:
                s = clustering_scores(torch.from_numpy(assign.astype(np.int32)).to(dev), y_dev, K)
                purity, nmi, ari, ppl = s["purity"], s["nmi"], s["ari"], s["perplexity"]
            else:
                ppl = perplexity_from_counts(np.bincount(assign, minlength=K))
            rows[(K, init)] = dict(zip(KEYS, (tag, int(K), init, int(seed), qe if np.isfinite(qe) else float("inf"),
                                              float(frac), purity, nmi, ari, ppl)))
            if K == K_values[0] and init == inits[0] and plt is not None:
                src = torch.from_numpy(np.asarray(medoids, dtype=np.int32)).to(dev)
                D, _, _, _, _ = sssp_multi_device(G, src, want_D=True)
                Z2, _, _ = distance_feature_pca(D, 2)
                plot_pca_with_clusters(plt, Z2, assign, medoids, out_dir / f"pca_clusters_{tag}_K{K}_{init}.png")
                plot_code_usage(plt, assign, K, out_dir / f"code_usage_{tag}_K{K}_{init}.png")
    return [rows[(K, init)] for K in K_values for init in inits]


def plot_pca_with_clusters(plt, Z2, assign, medoids, out_path: Path) -> None:
    plt.figure(figsize=(7, 6))
    plt.scatter(Z2[:, 0], Z2[:, 1], c=assign, cmap="tab20", s=8, alpha=0.8, linewidths=0)
    plt.scatter(Z2[medoids, 0], Z2[medoids, 1], c="black", s=60, marker="*", label="Medoids")
    plt.legend(loc="best")
    plt.title("PCA of distance-to-medoids representation")
    plt.tight_layout()
    plt.savefig(out_path, dpi=150)
    plt.close()


def plot_code_usage(plt, assign, K: int, out_path: Path) -> None:
    from ..geo.analysis import perplexity_from_counts
    counts = np.bincount(assign, minlength=K)
    plt.figure(figsize=(8, 3))
    plt.bar(np.arange(K), counts, width=0.9)
    plt.xlabel("Code index")
    plt.ylabel("Count")
    plt.title(f"Code usage (perplexity={perplexity_from_counts(counts):.2f})")
    plt.tight_layout()
    plt.savefig(out_path, dpi=150)
    plt.close()


def plot_elbow(plt, metrics: List[Dict], out_path: Path, tag: str) -> None:
    inits = sorted(set(m["init"] for m in metrics if m["graph"] == tag))
    K_values = sorted(set(int(m["K"]) for m in metrics if m["graph"] == tag))
    plt.figure(figsize=(6, 4))
    for init in inits:
        series = [np.mean([m["qe_geo_finite"] for m in metrics if m["graph"] == tag and m["init"] == init and m["K"] == K])
                  for K in K_values]
        plt.plot(K_values, series, marker="o", label=f"{init}")
    plt.xlabel("K (number of codes)")
    plt.ylabel("Geodesic QE (finite nodes)")
    plt.title(f"Elbow ({tag})")
    plt.legend(title="init")
    plt.tight_layout()
    plt.savefig(out_path, dpi=150)
    plt.close()


def main(argv=None) -> Path:
    args = parse_args(argv)
    try:
        paths = auto_detect_paths(args.experiment_dir)
    except FileNotFoundError as e:
        print(f"Error: {e}")
        return Path(".")
    print(f"Auto-detected paths:\n  Latents: {paths['latents_path']}")
    print(f"  Labels: {paths['labels_path'] or 'Not found (will skip label-based metrics)'}")
    K_values = [int(x.strip()) for x in args.K_values.split(",")]
    inits = [x.strip() for x in args.inits.split(",")]
    out_dir = Path(args.out_dir or f"demo_outputs/kmedoids_geodesic_{datetime.now().strftime('%Y%m%d_%H%M%S')}")
    out_dir.mkdir(parents=True, exist_ok=True)
    print("[demo] K-medoids Geodesic Demo\n[demo] Loading latents...")
    z = load_latents(paths["latents_path"])
    y = load_labels(paths["labels_path"]) if paths["labels_path"] else None
    print(f"[demo] Loaded {z.shape[0]} vectors (dim={z.shape[1]}), labels={'yes' if y is not None else 'no'}")
    plt = _pyplot()
    if plt is None:
        print("[demo] matplotlib is not installed: no plots")
    from ..geo import build_knn_graph
    print(f"[demo] Building k-NN graph: k={args.k_graph}, sym={args.graph_sym}")
    W, _ = build_knn_graph(z, k=args.k_graph, metric="euclidean", mode="distance", sym=args.graph_sym)
    print("[demo] Evaluating geodesic k-medoids on Euclidean-weight graph...")
    metrics = evaluate_setup(W, K_values, inits, seed=args.seed, labels=y, out_dir=out_dir, tag="euclidean", plt=plt)
    if metrics:
        with open(out_dir / "metrics.csv", "w", newline="") as f:
            writer = csv.DictWriter(f, fieldnames=list(metrics[0].keys()))
            writer.writeheader()
            for row in metrics:
                writer.writerow(row)
    with open(out_dir / "metrics.json", "w") as f:
        json.dump(metrics, f, indent=2)
    if plt is not None:
        plot_elbow(plt, metrics, out_dir / "elbow.png", tag="euclidean")
    print(f"[demo] Done. Outputs saved to: {out_dir}")
    return out_dir


if __name__ == "__main__":
    main()
