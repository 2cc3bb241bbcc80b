"""Map of the vanilla (vector-latent) VAE decoder's pull-back metric over a set of latents: riemann_metric_map for the decoders
of the legacy builders.  Per latent the volume element (logvol = 0.5 log det G), the trace, the extreme eigenvalues and the
numerical rank of G(z) = J(z)^T J(z), J = d sigmoid(decoder(z)) / dz (vqvae_amd.geo.pullback_metric_device).

    python -m vqvae_amd.scripts.vanilla_metric_map --codebook_dir out/riemannian_codebook --out_dir m
    python -m vqvae_amd.scripts.vanilla_metric_map --config configs/quantize.yaml --out_dir m \
        [--latents_path z.pt] [--max_latents 10000 --seed 0] [--chunk 8192] [--save_tensors]

The input is a legacy builder's YAML (--config: latents, checkpoint and VAE configuration read as
build_riemannian_codebook_legacy reads them) or the output directory of such a build (--codebook_dir: the configuration stored in
codebook.pt; its codes.npy, -1 outside the largest component, gives per-code statistics).  A covered decoder
(native_vanilla_metric_covers) on a GPU runs geo_vanilla_metric_tensor; anything else, and a machine without a GPU, takes the
autograd route.  The map is made --chunk latents at a time: the trace, the extreme eigenvalues, logvol and the rank are kept per
chunk, the tensors G (131 KB per latent at 128 dimensions) only with --save_tensors.

Writes metric_map.npz, metric_map.json and metric_map.png with riemann_metric_map's keys, plus "decoder": "vanilla".
"""
import argparse
import json
from pathlib import Path

import numpy as np
import torch

from .riemann_metric_map import plot_map, summarise


def make_parser():
    parser = argparse.ArgumentParser(description="Pull-back metric tensor per latent of a vanilla VAE decoder (eval mode): volume "
                                                 "element, trace, extreme eigenvalues, rank.")
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument("--config", type=str, default=None, help="YAML of build_riemannian_codebook_legacy")
    src.add_argument("--codebook_dir", type=str, default=None, help="output directory of build_riemannian_codebook_legacy")
    parser.add_argument("--out_dir", type=str, required=True)
    parser.add_argument("--latents_path", type=str, default=None, help="latents to map instead of the configuration's")
    parser.add_argument("--max_latents", type=int, default=None, help="seeded subsample of this many latents (default: all)")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--save_tensors", action="store_true", help="also store G [n, d, d] in metric_map.npz")
    parser.add_argument("--chunk", type=int, default=8192, help="latents per pullback_metric_device call")
    return parser


def main(args) -> dict:
    from ..geo.riemannian_metric import native_vanilla_metric_covers, pullback_metric_device
    from ..training.build_riemannian_codebook_legacy import LegacyJob, read_decoder, read_latents

    if args.chunk < 1:
        raise ValueError(f"--chunk {args.chunk} < 1")
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    codes_all = None
    if args.codebook_dir:
        cb_dir = Path(args.codebook_dir)
        config = torch.load(cb_dir / "codebook.pt", map_location="cpu", weights_only=False)["config"]
        if (cb_dir / "codes.npy").exists():
            codes_all = np.load(cb_dir / "codes.npy").reshape(-1)
    else:
        import yaml
        with open(args.config) as fh:
            config = yaml.safe_load(fh)
    job = LegacyJob.from_config(config)
    decoder = read_decoder(job.checkpoint, job.vae_config, dev)
    z = read_latents(Path(args.latents_path) if args.latents_path else job.latents)
    if z.dim() != 2:
        raise ValueError(f"expected latents [N, d], got {tuple(z.shape)}")
    n_all, d = z.shape
    if codes_all is not None and codes_all.shape[0] != n_all:
        if not args.latents_path:
            raise ValueError(f"codes.npy has {codes_all.shape[0]} entries, the latents {n_all}")
        codes_all = None                                   # other latents than the build's: no per-code statistics
    index = np.arange(n_all, dtype=np.int64)
    if args.max_latents is not None and args.max_latents < n_all:
        index = np.sort(np.random.RandomState(args.seed).choice(n_all, args.max_latents, replace=False)).astype(np.int64)
    print(f"Metric tensor of {len(index)} of {n_all} latents (d={d}), eval-mode vanilla decoder, {args.chunk} per call")

    keep = {k: [] for k in ("logvol", "trace", "eig_min", "eig_max", "rank")}
    # (the route of an empty map: what a call would take)
    tensors, route = [], "native" if native_vanilla_metric_covers(decoder) and dev.type == "cuda" else "autograd"
    for lo in range(0, len(index), args.chunk):
        res = pullback_metric_device(decoder, z[torch.from_numpy(index[lo:lo + args.chunk])].to(dev))
        route = res.route
        G, eig = res.G.cpu().numpy(), res.eig.cpu().numpy()
        keep["logvol"].append(res.logvol.cpu().numpy())
        keep["trace"].append(np.einsum("naa->n", G))
        keep["eig_min"].append(eig[:, 0])
        keep["eig_max"].append(eig[:, -1])
        keep["rank"].append(res.rank.cpu().numpy())
        if args.save_tensors:
            tensors.append(G)
    arrays = {k: np.concatenate(v) if v else np.zeros(0) for k, v in keep.items()}
    arrays["index"] = index
    if args.save_tensors:
        arrays["G"] = np.concatenate(tensors) if tensors else np.zeros((0, d, d))
    np.savez(out_dir / "metric_map.npz", **arrays)

    summary = summarise(arrays["logvol"], arrays["eig_min"], arrays["eig_max"], arrays["rank"], d, n_all, route,
                        None if codes_all is None else codes_all[index])
    summary["decoder"] = "vanilla"
    with open(out_dir / "metric_map.json", "w") as f:
        json.dump(summary, f, indent=1)
    plot_map(arrays["logvol"], arrays["eig_min"], arrays["eig_max"], out_dir / "metric_map.png")
    print(f"route {route}: {summary['n_rank_deficient']} of {summary['n']} latents rank deficient; saved to {out_dir}")
    return summary


if __name__ == "__main__":
    main(make_parser().parse_args())
