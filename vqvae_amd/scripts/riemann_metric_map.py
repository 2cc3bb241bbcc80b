"""Map of the decoder's pull-back metric over a set of latents: per latent the volume element sqrt(det G) (as
logvol = 0.5 log det G, the "magnification factor"), the trace, the extreme eigenvalues and the numerical rank of
G(z) = J(z)^T J(z), J = d sigmoid(decoder(z)) / dz (vqvae_amd.geo.pullback_metric_device).

    python -m vqvae_amd.scripts.riemann_metric_map --latents_path z.pt --out_dir out --vae_ckpt_path best.pt \
        --in_channels 1 --output_image_size 28 --latent_dim 16 --enc_channels 64 128 256 \
        --dec_channels 256 128 64 --recon_loss mse --norm_type batch --mse_use_sigmoid \
        [--codes out/codes.npy] [--max_latents 100000 --seed 0] [--save_tensors]

It takes build_codebook's command line (the graph and clustering flags are accepted and ignored), so the map is made from
the arguments the codebook was built with.  The decoder is put in eval(), as riemann_sanity_check does: build_codebook's default
re-weighting runs the decoder in train mode (batch statistics), where a latent has no metric tensor of its own, so this map
describes the eval-mode decoder, not the lengths of that build.

Writes metric_map.npz (logvol, trace, eig_min, eig_max, rank, index = the flat latent rows used, in build_codebook's (n, h, w)
order; G with --save_tensors), metric_map.json (counts, quantiles, the route taken, per-code statistics with --codes) and
metric_map.png.  Float32 Jacobian columns determine G's entries, its trace and its large eigenvalues; where G is nearly singular
-- 16 outputs from 16 latent dimensions: cond(G) up to 1e9 -- they do not determine eig_min or logvol, and the JSON says so
(`note`) whenever the largest condition number of the map is above 1e6.
"""
import json
from pathlib import Path

import numpy as np
import torch

from .build_codebook import make_parser as _codebook_parser

QUANTILES = (0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0)
ILL_CONDITIONED = 1e6
NOTE = ("cond(G) reaches {cond:.1e}: float32 Jacobian columns do not determine the smallest eigenvalues or logvol of such a "
        "latent (G's entries, trace and eig_max are unaffected)")


def make_parser():
    parser = _codebook_parser()
    parser.description = ("Pull-back metric tensor per latent of the EVAL-mode decoder: volume element, trace, extreme eigenvalues, "
                          "rank.  build_codebook's default re-weighting is train-mode (batch statistics); this map describes "
                          "the eval-mode decoder.  build_codebook's graph and clustering flags are accepted and ignored.")
    parser.add_argument("--codes", type=str, default=None, help="codes.npy of a build over the same latents: per-code statistics")
    parser.add_argument("--max_latents", type=int, default=None, help="seeded subsample of this many latents (default: all)")
    parser.add_argument("--save_tensors", action="store_true", help="also store G [n, d, d] in metric_map.npz")
    return parser


def per_code_stats(codes: np.ndarray, logvol: np.ndarray) -> dict:
    """{code: {count, count_finite, logvol_mean, logvol_std}} over the latents given; code -1 (no code) is skipped.  Mean and
    (population) std over the members with a finite logvol, the sums in fp64 in ascending latent order."""
    codes = np.asarray(codes).astype(np.int64).ravel()
    logvol = np.asarray(logvol, dtype=np.float64).ravel()
    keep = codes >= 0
    K = int(codes[keep].max()) + 1 if keep.any() else 0
    count = np.bincount(codes[keep], minlength=K)
    fin = keep & np.isfinite(logvol)
    n_fin = np.bincount(codes[fin], minlength=K)
    total = np.bincount(codes[fin], weights=logvol[fin], minlength=K)             # (bincount adds in array order)
    mean = np.divide(total, n_fin, out=np.full(K, np.nan), where=n_fin > 0)
    dev2 = np.bincount(codes[fin], weights=(logvol[fin] - mean[codes[fin]]) ** 2, minlength=K)
    std = np.sqrt(np.divide(dev2, n_fin, out=np.full(K, np.nan), where=n_fin > 0))
    return {str(c): {"count": int(count[c]), "count_finite": int(n_fin[c]),
                     "logvol_mean": float(mean[c]) if n_fin[c] else None, "logvol_std": float(std[c]) if n_fin[c] else None}
            for c in range(K) if count[c]}


def _quantiles(x: np.ndarray):
    return {f"{q:g}": float(np.quantile(x, q)) for q in QUANTILES} if x.size else None


def summarise(logvol, eig_min, eig_max, rank, d: int, n_total: int, route: str, codes=None) -> dict:
    """metric_map.json of a map (shared with vanilla_metric_map): counts, the quantiles of logvol over the full-rank latents and
    of eig_max / eig_min, the `note` for an ill-conditioned map, and per-code statistics where `codes` (one per latent of the
    map) is given."""
    full = rank == d
    finite = np.isfinite(logvol)
    cond = eig_max[eig_min > 0] / eig_min[eig_min > 0]
    summary = {"n": int(len(logvol)), "n_total": int(n_total), "latent_dim": int(d), "n_rank_deficient": int((~full).sum()),
               "route": route, "decoder_mode": "eval",
               "logvol_quantiles_full_rank": _quantiles(logvol[full & finite]),
               "eig_ratio_quantiles": _quantiles(cond)}
    if cond.size and cond.max() > ILL_CONDITIONED:
        summary["note"] = NOTE.format(cond=float(cond.max()))
        print("Note: " + summary["note"])
    if codes is not None:
        summary["per_code"] = per_code_stats(codes, logvol)
    return summary


def plot_map(logvol, eig_min, eig_max, path):
    """metric_map.png (shared with vanilla_metric_map): the histogram of logvol and logvol against the anisotropy."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    finite = np.isfinite(logvol)
    fig, (ax1, ax2) = plt.subplots(1, 2, figsize=(10, 5))
    ax1.hist(logvol[finite], bins=50)
    ax1.set_xlabel("logvol = 0.5 log det G")
    ax1.set_ylabel("Count")
    ax1.set_title("Volume element of the pull-back metric (eval-mode decoder)")
    both = finite & (eig_min > 0)
    ax2.scatter(np.log10(eig_max[both] / eig_min[both]), logvol[both], s=6, alpha=0.6)
    ax2.set_xlabel("log10(eig_max / eig_min)")
    ax2.set_ylabel("logvol")
    ax2.set_title("Volume element against anisotropy")
    plt.tight_layout()
    plt.savefig(path, dpi=150)
    plt.close(fig)


def main(args):
    from ..geo.riemannian_metric import pullback_metric_device
    from ..spatial_decoder import load_decoder_from_checkpoint

    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    decoder = load_decoder_from_checkpoint(
        args.vae_ckpt_path, in_channels=args.in_channels, dec_channels=args.dec_channels, latent_dim=args.latent_dim,
        output_image_size=args.output_image_size, norm_type=args.norm_type, device=dev).eval()

    z = torch.load(Path(args.latents_path), map_location="cpu").float()
    N, C, H, W = z.shape
    z_flat = z.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    n_all = z_flat.shape[0]
    index = np.arange(n_all, dtype=np.int64)
    if args.max_latents is not None and args.max_latents < n_all:
        index = np.sort(np.random.RandomState(args.seed).choice(n_all, args.max_latents, replace=False)).astype(np.int64)
    print(f"Metric tensor of {len(index)} of {n_all} latents (N={N}, C={C}, H={H}, W={W}), eval-mode decoder")

    res = pullback_metric_device(decoder, z_flat[torch.from_numpy(index)].to(dev))
    G, eig, logvol, rank = (t.cpu().numpy() for t in (res.G, res.eig, res.logvol, res.rank))
    d = eig.shape[1]
    trace = np.einsum("naa->n", G)
    eig_min, eig_max = eig[:, 0], eig[:, -1]
    arrays = {"logvol": logvol, "trace": trace, "eig_min": eig_min, "eig_max": eig_max, "rank": rank, "index": index}
    if args.save_tensors:
        arrays["G"] = G
    np.savez(out_dir / "metric_map.npz", **arrays)

    codes = None
    if args.codes:
        codes = np.load(args.codes).reshape(-1)
        if codes.shape[0] != n_all:
            raise ValueError(f"--codes has {codes.shape[0]} entries, the latents {n_all}")
        codes = codes[index]
    summary = summarise(logvol, eig_min, eig_max, rank, d, n_all, res.route, codes)
    with open(out_dir / "metric_map.json", "w") as f:
        json.dump(summary, f, indent=1)
    plot_map(logvol, eig_min, eig_max, out_dir / "metric_map.png")
    print(f"route {res.route}: {summary['n_rank_deficient']} of {summary['n']} latents rank deficient; saved to {out_dir}")
    return summary


if __name__ == "__main__":
    main(make_parser().parse_args())
