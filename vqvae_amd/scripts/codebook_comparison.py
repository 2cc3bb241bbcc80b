"""Geodesic vs Euclidean codebook comparison with both sides on the GPU (the reference's demos/codebook_comparison.py).

    python -m vqvae_amd.scripts.codebook_comparison <experiment_dir> [--K 64] [--k_graph 10] [--seed 42]

Reads `vae/**/checkpoints/best.pt` and `vae/**/latents_val/z.pt` under experiment_dir and writes
demo_outputs/codebook_comparison_<name>_<timestamp>/{metrics.json, config.yaml, codebook_comparison.png} under the working
directory, as the reference does.
  Euclidean side  vqvae_amd.cluster.KMeans(K, random_state=seed, n_init=10)   (the reference: sklearn's, on the CPU)
  Geodesic side   build_knn_graph (euclidean, distance, mutual) -> largest connected component -> fit_kmedoids_optimized
                  -> dijkstra_multi_source for the geodesic quantization error
  Metrics         the reference's compute_metrics: reconstruction MSE through the vanilla VAE's decoder (eval mode, sigmoid),
                  perplexity of the code histogram, quantization error.
"""
import argparse
import json
from datetime import datetime
from pathlib import Path
from typing import Dict, Tuple

import numpy as np
import torch
import yaml

VAE_DEFAULTS = {"in_channels": 1, "latent_dim": 128, "enc_channels": [64, 128, 256], "dec_channels": [256, 128, 64],
                "recon_loss": "mse", "output_image_size": 28, "norm_type": "batch", "mse_use_sigmoid": True}


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Geodesic vs Euclidean codebook comparison")
    p.add_argument("experiment_dir", type=str, help="Path to experiment directory")
    p.add_argument("--K", type=int, default=64, help="Codebook size (default: 64)")
    p.add_argument("--k_graph", type=int, default=10, help="k-NN connectivity (default: 10)")
    p.add_argument("--seed", type=int, default=42, help="Random seed (default: 42)")
    return p.parse_args(argv)


def auto_detect_paths(experiment_dir: str) -> dict:
    vae_dir = Path(experiment_dir) / "vae"
    if not vae_dir.exists():
        raise FileNotFoundError(f"VAE directory not found: {vae_dir}")
    ckpts = list(vae_dir.rglob("checkpoints/best.pt"))
    lats = list(vae_dir.rglob("latents_val/z.pt"))
    if not ckpts:
        raise FileNotFoundError(f"VAE checkpoint not found in: {vae_dir}")
    if not lats:
        raise FileNotFoundError(f"Validation latents not found in: {vae_dir}")
    return {"checkpoint_path": ckpts[0], "latents_path": lats[0]}


def load_decoder(checkpoint_path: Path, device: torch.device):
    """The vanilla VAE's decoder with the reference's config handling (checkpoint "config" / "model_config", else defaults)."""
    from ..vae import decoder_from_vae_checkpoint
    ckpt = torch.load(checkpoint_path, map_location="cpu")
    cfg = ckpt.get("config") or ckpt.get("model_config") or {}
    p = {k: cfg.get(k, VAE_DEFAULTS[k]) for k in VAE_DEFAULTS}
    dec = decoder_from_vae_checkpoint(ckpt["model_state_dict"], in_channels=p["in_channels"], dec_channels=p["dec_channels"],
                                      latent_dim=p["latent_dim"], output_image_size=p["output_image_size"],
                                      norm_type=p["norm_type"])
    return dec.to(device).eval()


def build_euclidean_codebook(z: np.ndarray, K: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    from ..cluster import KMeans
    km = KMeans(n_clusters=K, random_state=seed, n_init=10)
    assign = km.fit_predict(z)
    return km.cluster_centers_, assign


def build_geodesic_codebook(z: np.ndarray, K: int, k_graph: int, seed: int):
    from ..geo import build_knn_graph
    from ..geo.kmeans_optimized import fit_kmedoids_optimized
    from ..geo.knn_graph_optimized import largest_connected_component
    W, _ = build_knn_graph(z, k=k_graph, metric="euclidean", mode="distance", sym="mutual")
    mask = largest_connected_component(W)
    if mask.sum() < W.shape[0]:
        W_lcc, z_lcc = W[mask][:, mask], z[mask]
    else:
        W_lcc, z_lcc, mask = W, z, np.ones(len(z), dtype=bool)
    medoids, assign_lcc, _ = fit_kmedoids_optimized(W_lcc, K=K, init="kpp", seed=seed)
    assign = np.full(len(z), -1, dtype=np.int32)
    assign[mask] = assign_lcc
    return z_lcc[medoids], assign, W_lcc, mask, medoids


def reconstruction_mse(decoder, z_orig: torch.Tensor, z_quant: torch.Tensor, device) -> float:
    with torch.no_grad():
        a = torch.sigmoid(decoder(z_orig.to(device)))
        b = torch.sigmoid(decoder(z_quant.to(device)))
        return torch.nn.functional.mse_loss(b, a).item()


def compute_metrics(decoder, z, centroids, assign, W_lcc, mask_lcc, medoids, K, device, is_geodesic=False) -> Dict[str, float]:
    """The reference's compute_metrics (demos/codebook_comparison.py)."""
    zt = torch.from_numpy(z).float()
    if is_geodesic:
        valid = assign >= 0
        zq = zt.clone()
        if valid.any():
            zq[valid] = torch.from_numpy(centroids[assign[valid]]).float()
        mse = reconstruction_mse(decoder, zt[valid], zq[valid], device)
        n_valid = int(valid.sum())
    else:
        zq = torch.from_numpy(centroids[assign]).float()
        mse = reconstruction_mse(decoder, zt, zq, device)
        n_valid = len(z)
    va = assign[assign >= 0] if is_geodesic else assign
    counts = np.bincount(va, minlength=K)
    probs = counts / max(1, counts.sum())
    nz = probs[probs > 0]
    perplexity = float(np.exp(-np.sum(nz * np.log(nz + 1e-12))))
    if is_geodesic and mask_lcc.any():
        from ..geo import dijkstra_multi_source
        D = dijkstra_multi_source(W_lcc, medoids)
        a_lcc = assign[mask_lcc]
        dmin = D[a_lcc, np.arange(len(a_lcc))]
        fin = np.isfinite(dmin)
        qe = float(np.mean(dmin[fin] ** 2)) if fin.any() else float("inf")
    else:
        qe = float(np.mean(np.linalg.norm(z - zq.numpy(), axis=1) ** 2))
    return {"reconstruction_mse": float(mse), "perplexity": perplexity, "quantization_error": qe, "valid_samples": n_valid}


def save_comparison_plot(metrics, out_dir: Path) -> bool:
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        print("[demo] matplotlib is not installed: no plot")
        return False
    fig, axes = plt.subplots(1, 3, figsize=(15, 5))
    methods, colors = ["Euclidean", "Geodesic"], ["#1f77b4", "#ff7f0e"]
    for i, (key, ylabel, title) in enumerate([
            ("reconstruction_mse", "Reconstruction MSE", "Reconstruction Quality\n(Lower is Better)"),
            ("perplexity", "Perplexity", "Code Usage Diversity\n(Higher is Better)"),
            ("quantization_error", "Quantization Error", "Clustering Quality\n(Lower is Better)")]):
        axes[i].bar(methods, [metrics["euclidean"][key], metrics["geodesic"][key]], color=colors)
        axes[i].set_ylabel(ylabel)
        axes[i].set_title(title)
    plt.tight_layout()
    plt.savefig(out_dir / "codebook_comparison.png", dpi=150, bbox_inches="tight")
    plt.close()
    return True


def main(argv=None):
    args = parse_args(argv)
    try:
        paths = auto_detect_paths(args.experiment_dir)
    except FileNotFoundError as e:
        print(f"Error: {e}")
        return None
    print(f"Auto-detected paths:\n  Checkpoint: {paths['checkpoint_path']}\n  Latents: {paths['latents_path']}")
    timestamp = datetime.now().strftime("%Y%m%d_%H%M%S")
    out_dir = Path(f"demo_outputs/codebook_comparison_{Path(args.experiment_dir).name}_{timestamp}")
    out_dir.mkdir(parents=True, exist_ok=True)
    from .._device import device as gpu
    device = gpu()
    lat = torch.load(paths["latents_path"], map_location="cpu")
    z = np.ascontiguousarray((lat["z"] if isinstance(lat, dict) else lat).float().numpy())
    decoder = load_decoder(paths["checkpoint_path"], device)
    print(f"[demo] Loaded {len(z)} latents (dim={z.shape[1]})")
    print(f"[demo] Building Euclidean codebook (K={args.K})...")
    c_euc, a_euc = build_euclidean_codebook(z, args.K, args.seed)
    print(f"[demo] Building geodesic codebook (K={args.K}, k_graph={args.k_graph})...")
    c_geo, a_geo, W_lcc, mask, medoids = build_geodesic_codebook(z, args.K, args.k_graph, args.seed)
    m_euc = compute_metrics(decoder, z, c_euc, a_euc, None, None, None, args.K, device, False)
    m_geo = compute_metrics(decoder, z, c_geo, a_geo, W_lcc, mask, medoids, args.K, device, True)
    metrics = {"euclidean": m_euc, "geodesic": m_geo}
    save_comparison_plot(metrics, out_dir)
    with open(out_dir / "metrics.json", "w") as f:
        json.dump(metrics, f, indent=2)
    cfg = {"experiment_dir": args.experiment_dir, "K": args.K, "k_graph": args.k_graph, "seed": args.seed,
           "latents_path": str(paths["latents_path"]), "checkpoint_path": str(paths["checkpoint_path"])}
    with open(out_dir / "config.yaml", "w") as f:
        yaml.dump(cfg, f, default_flow_style=False, indent=2)
    print(f"\n[demo] Comparison (K={args.K}):")
    for name, m in (("Euclidean", m_euc), ("Geodesic ", m_geo)):
        print(f"[demo] {name}  MSE={m['reconstruction_mse']:.6f}  PPL={m['perplexity']:.2f}  QE={m['quantization_error']:.2f}")
    print(f"[demo] Results saved to: {out_dir}")
    return out_dir


if __name__ == "__main__":
    main()
