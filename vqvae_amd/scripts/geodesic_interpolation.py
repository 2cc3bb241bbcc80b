"""Interpolate between training images along the geodesics of a built codebook's graph, next to the straight line.

    python -m vqvae_amd.scripts.geodesic_interpolation --codebook_dir DIR --out_dir OUT
        (--pairs i:j [i:j ...] | --num_pairs N [--seed S]) [--frames 9] [--dataset other] [--batch_size 512]
        [--train_latents_path PATH] [--relax_iters N] [--relax_metric position|image]

DIR is an output of vqvae_amd.scripts.build_codebook (spatial pipeline): codebook.pt's "config" names the checkpoint, the
training latents and the decoder's arguments, exactly as vqvae_amd.training.assign_codes_val_geodesic reads them.  A pair i:j
is two images of the training latents; each of their grid positions is one node pair of knn_graph_geodesic.npz
(geo.interpolation.interpolate_images_spatial).  The decoder runs in eval() mode.  An extension: the reference's demos
(visualizations/interactive_knn_viz.py, demos/interactive_exploration.py) colour nodes by geodesic distance and stop there.

DIR may also be an output of vqvae_amd.training.build_riemannian_codebook_legacy (the vanilla/geodesic pipeline), recognised
by knn_graph_riemannian.npz beside a codebook.pt whose z_medoid is 2-D: its "config" is read as the builder read it
(LegacyJob.from_config, read_latents, read_decoder), an image is one latent and a pair one node pair
(geo.interpolation.interpolate_images_vanilla), and the artefacts below have h w = 1.

Writes to OUT:
  interpolation.png   two rows of `frames` images per pair: the chord on top, the geodesic below (the grid of codebook_sampling)
  interpolation.npz   pairs i64 [M, 2]; frames_lin, frames_geo f32 [M, F, d, h, w]; images_lin, images_geo f32 [M, F, C, S, S];
                      graph_dist f32, hops, status i32 [M, h w]; curve_len_lin, curve_len_geo f32 [M]; image_len_lin,
                      image_len_geo f64 [M]; fallback_pair, fallback_position i32 [n_fallback] (the positions that took the chord)
  interpolation.json  per pair: graph_dist (summed over the positions with a path), the four lengths, ratio_curve and
                      ratio_image (geodesic / chord), fallback_positions; and the totals over the pairs

--relax_iters N (default 0: none of the following) relaxes, per grid position, the geodesic's frames and the chord under the
decoder's metric with the ends fixed for N iterations each (geo.relaxation) and keeps the result with the lower curve energy:
  interpolation.png   a third row per pair, the relaxed curve
  interpolation.npz   also frames_relaxed, images_relaxed, curve_len_relaxed, image_len_relaxed; relax_from, accepted_geo,
                      accepted_lin i32 [M, h w]; energy_geo, energy_lin, energy_relaxed f64 [M, h w]
  interpolation.json  per pair also curve_len_relaxed, image_len_relaxed, energy_geo, energy_lin, energy_relaxed (summed over
                      the positions), relax_from and the accepted counts per position; the totals of the lengths and energies
The relaxed curve is never worse in energy than either start, by construction.
--relax_metric image (spatial builds with 4x4 grids, with --relax_iters N) relaxes each pair's two sequences of whole grids under
the whole decoder instead (geo.grid_relaxation): the third row is that result, relax_from, accepted_geo, accepted_lin are i32 [M]
and energy_geo, energy_lin, energy_relaxed f64 [M] (one curve per pair), and the JSON names "relax_metric": "image".  Without
the flag the three artefacts are what they were.

Whether the geodesic is the shorter curve under the decoder's metric is a property of the trained model; the JSON reports
the ratio and the script asserts nothing about it.
"""
import argparse
import json
from pathlib import Path

import numpy as np
import torch


def parse_pairs(tokens, n_images: int) -> np.ndarray:
    """["3:17", ...] -> i64 [M, 2]; ValueError for a token that is not i:j or an image outside [0, n_images)."""
    pairs = []
    for tok in tokens:
        parts = tok.split(":")
        if len(parts) != 2 or not all(p.strip().lstrip("-").isdigit() for p in parts):
            raise ValueError(f"--pairs: '{tok}' is not of the form i:j")
        i, j = int(parts[0]), int(parts[1])
        if not (0 <= i < n_images and 0 <= j < n_images):
            raise ValueError(f"--pairs: '{tok}' names an image outside 0...{n_images}")
        pairs.append((i, j))
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2)


def draw_pairs(n_images: int, num_pairs: int, seed: int) -> np.ndarray:
    """num_pairs pairs of distinct images, RandomState(seed).choice without replacement per pair."""
    if n_images < 2 or num_pairs < 1:
        raise ValueError(f"--num_pairs {num_pairs} of {n_images} images: at least one pair of two images is needed")
    rng = np.random.RandomState(seed)
    return np.stack([rng.choice(n_images, size=2, replace=False) for _ in range(num_pairs)]).astype(np.int64)


def _ratio(a: float, b: float):
    return a / b if b > 0 else None


def is_legacy_build(cb_dir: Path) -> bool:
    """A directory written by build_riemannian_codebook_legacy: knn_graph_riemannian.npz plus codebook.pt with 2-D z_medoid."""
    if not ((cb_dir / "knn_graph_riemannian.npz").is_file() and (cb_dir / "codebook.pt").is_file()):
        return False
    z_medoid = torch.load(cb_dir / "codebook.pt", map_location="cpu", weights_only=False).get("z_medoid")
    return torch.is_tensor(z_medoid) and z_medoid.dim() == 2


def load_legacy_build(cb_dir: Path, train_latents_path=None):
    """(job, apply_sigmoid, W scipy CSR, z f32 [N, d], lcc rows) of a legacy build; ValueError when codes.npy, the graph, the
    latents and z_medoid do not belong together."""
    from scipy import sparse
    from ..training.assign_codes_val_geodesic import lcc_rows
    from ..training.build_riemannian_codebook_legacy import LegacyJob, read_latents
    codebook = torch.load(cb_dir / "codebook.pt", map_location="cpu", weights_only=False)
    job = LegacyJob.from_config(codebook["config"])
    W = sparse.load_npz(cb_dir / "knn_graph_riemannian.npz").tocsr()
    z = read_latents(Path(train_latents_path) if train_latents_path else job.latents)
    rows = lcc_rows(np.load(cb_dir / "codes.npy"))
    med = np.asarray(codebook["medoid_indices"], dtype=np.int64)
    if z.dim() != 2 or np.load(cb_dir / "codes.npy").size != z.shape[0] or rows.size != W.shape[0] or (
            med.size and not torch.equal(z[torch.from_numpy(rows[med])], codebook["z_medoid"].float())):
        raise ValueError(f"{cb_dir}: codes.npy, knn_graph_riemannian.npz, codebook.pt and the latents {tuple(z.shape)} do not "
                         "belong together")
    vae = job.vae_config
    apply_sigmoid = str(vae.get("recon_loss", "mse")).lower() == "bce" or bool(vae.get("mse_use_sigmoid", False))
    return job, apply_sigmoid, W, z, rows


def main(args) -> dict:
    from .._device import DeviceCSR, device
    from ..geo.interpolation import interpolate_images_spatial, interpolate_images_vanilla
    from ..spatial_decoder import load_decoder_from_checkpoint
    from ..training.assign_codes_val_geodesic import lcc_rows, load_build
    cb_dir = Path(args.codebook_dir)
    if (args.pairs is None) == (args.num_pairs is None):
        raise ValueError("give either --pairs i:j ... or --num_pairs N")
    if is_legacy_build(cb_dir):
        if args.relax_metric != "position":
            raise ValueError("--relax_metric image relaxes the latent grids of a spatial build; this is a vanilla build")
        from ..training.build_riemannian_codebook_legacy import read_decoder
        job, apply_sigmoid, W, z, rows = load_legacy_build(cb_dir, args.train_latents_path)
        pairs = parse_pairs(args.pairs, z.shape[0]) if args.pairs is not None else draw_pairs(z.shape[0], args.num_pairs, args.seed)
        dev = device()
        out = interpolate_images_vanilla(z, rows, DeviceCSR.from_scipy(W, dev), read_decoder(job.checkpoint, job.vae_config, dev),
                                         pairs, args.frames, args.dataset, apply_sigmoid, batch_size=args.batch_size,
                                         relax_iters=args.relax_iters)
        # the same artefacts with h w = 1: a position axis of one, frames as 1 x 1 grids
        for k, v in out.items():
            if k.startswith("frames_"):
                out[k] = v.view(*v.shape, 1, 1)
            elif torch.is_tensor(v) and v.dim() == 1 and not k.startswith(("curve_len_", "image_len_")):
                out[k] = v.view(-1, 1)
        return write_artefacts(args, out, pairs, apply_sigmoid)
    codebook, W, _ = load_build(cb_dir, args.train_latents_path)       # checks that the artefacts belong together
    cfg = codebook["config"]
    z = torch.load(args.train_latents_path or cfg["latents_path"], map_location="cpu").float()
    if z.dim() != 4:
        raise ValueError(f"the build's latents are {tuple(z.shape)}: this script interpolates latent grids [N, d, h, w]")
    pairs = parse_pairs(args.pairs, z.shape[0]) if args.pairs is not None else draw_pairs(z.shape[0], args.num_pairs, args.seed)
    dev = device()
    decoder = load_decoder_from_checkpoint(
        cfg["vae_ckpt_path"], in_channels=cfg["in_channels"], dec_channels=cfg["dec_channels"], latent_dim=cfg["latent_dim"],
        output_image_size=cfg["output_image_size"], norm_type=cfg["norm_type"], device=dev).eval()
    apply_sigmoid = str(cfg.get("recon_loss", "mse")).lower() == "bce" or bool(cfg.get("mse_use_sigmoid", False))
    out = interpolate_images_spatial(z, lcc_rows(np.load(cb_dir / "codes.npy")), DeviceCSR.from_scipy(W, dev), decoder,
                                     pairs, args.frames, args.dataset, apply_sigmoid, batch_size=args.batch_size,
                                     relax_iters=args.relax_iters, relax_metric=args.relax_metric)
    return write_artefacts(args, out, pairs, apply_sigmoid)


def write_artefacts(args, out: dict, pairs: np.ndarray, apply_sigmoid: bool) -> dict:
    """interpolation.png / .npz / .json of the module docstring from an interpolate_images_* result with a position axis."""
    from .generate_samples import save_image
    cb_dir, out_dir = Path(args.codebook_dir), Path(args.out_dir)
    M, F = pairs.shape[0], int(args.frames)
    host = {k: out[k].cpu().numpy() for k in ("frames_lin", "frames_geo", "images_lin", "images_geo", "graph_dist", "hops",
                                               "status", "curve_len_lin", "curve_len_geo", "image_len_lin", "image_len_geo")}
    relaxed = args.relax_iters > 0
    relax_sums = ("curve_len_relaxed", "image_len_relaxed", "energy_geo", "energy_lin", "energy_relaxed")
    relax_lists = ("relax_from", "accepted_geo", "accepted_lin")
    if relaxed:
        host.update({k: out[k].cpu().numpy() for k in ("frames_relaxed", "images_relaxed") + relax_sums + relax_lists})
    fallback = out["fallback_positions"]
    per_pair = []
    for m in range(M):
        d = host["graph_dist"][m]
        with_path = host["status"][m] == 0
        rec = {"pair": [int(pairs[m, 0]), int(pairs[m, 1])],
               "graph_dist": float(d[with_path].astype(np.float64).sum()),
               "fallback_positions": [int(p) for p in fallback[m]]}
        for k in ("curve_len_lin", "curve_len_geo", "image_len_lin", "image_len_geo"):
            rec[k] = float(host[k][m])
        rec["ratio_curve"] = _ratio(rec["curve_len_geo"], rec["curve_len_lin"])
        rec["ratio_image"] = _ratio(rec["image_len_geo"], rec["image_len_lin"])
        if relaxed:
            for k in relax_sums:
                rec[k] = float(np.asarray(host[k][m], dtype=np.float64).sum())
            for k in relax_lists:
                rec[k] = [int(v) for v in np.atleast_1d(host[k][m])]
        per_pair.append(rec)
    totals = {k: float(sum(r[k] for r in per_pair))
              for k in ("graph_dist", "curve_len_lin", "curve_len_geo", "image_len_lin", "image_len_geo")}
    totals["ratio_curve"] = _ratio(totals["curve_len_geo"], totals["curve_len_lin"])
    totals["ratio_image"] = _ratio(totals["image_len_geo"], totals["image_len_lin"])
    totals["fallback_positions"] = int(sum(len(p) for p in fallback))
    if relaxed:
        totals.update({k: float(sum(r[k] for r in per_pair)) for k in relax_sums})
    summary = {"codebook_dir": str(cb_dir), "frames": F, "dataset": args.dataset, "apply_sigmoid": apply_sigmoid,
               "pairs": per_pair, "totals": totals}
    if relaxed:
        summary["relax_iters"] = int(args.relax_iters)
        if args.relax_metric != "position":
            summary["relax_metric"] = args.relax_metric

    out_dir.mkdir(parents=True, exist_ok=True)
    # [M, 2 or 3, F, C, S, S]: chord above geodesic (above the relaxed curve), per pair
    rows = torch.stack([out["images_lin"], out["images_geo"]] + ([out["images_relaxed"]] if relaxed else []), dim=1)
    save_image(rows.reshape(M * rows.shape[1] * F, *rows.shape[3:]).cpu(), str(out_dir / "interpolation.png"), nrow=F)
    np.savez(out_dir / "interpolation.npz", pairs=pairs,
             fallback_pair=np.concatenate([np.full(len(p), m, dtype=np.int32) for m, p in enumerate(fallback)]),
             fallback_position=np.concatenate([np.asarray(p, dtype=np.int32) for p in fallback]), **host)
    with open(out_dir / "interpolation.json", "w") as f:
        json.dump(summary, f, indent=2)
    t = totals
    print(f"{M} pair(s), {F} frames: pull-back length geodesic {t['curve_len_geo']:.4f} / chord {t['curve_len_lin']:.4f}; "
          f"image-space length geodesic {t['image_len_geo']:.4f} / chord {t['image_len_lin']:.4f}; "
          f"{t['fallback_positions']} position(s) took the chord")
    if relaxed:
        print(f"relaxed for {args.relax_iters} iteration(s): pull-back length {t['curve_len_relaxed']:.4f}, image-space length "
              f"{t['image_len_relaxed']:.4f}; curve energy {t['energy_relaxed']:.6g} from geodesic {t['energy_geo']:.6g} / chord "
              f"{t['energy_lin']:.6g}; {int(sum(sum(r['relax_from']) for r in per_pair))} "
              f"{'pair' if args.relax_metric == 'image' else 'position'}(s) kept the geodesic's result")
    print(f"Saved artifacts to: {out_dir}")
    return out


def make_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Geodesic and straight-line interpolation between training images of a built codebook.")
    p.add_argument("--codebook_dir", type=str, required=True)
    p.add_argument("--out_dir", type=str, required=True)
    p.add_argument("--pairs", type=str, nargs="+", default=None, help="image pairs i:j")
    p.add_argument("--num_pairs", type=int, default=None, help="draw this many random pairs instead of --pairs")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--frames", type=int, default=9)
    p.add_argument("--dataset", type=str, default="other", help="CIFAR10: un-normalise RGB images decoded without a sigmoid")
    p.add_argument("--batch_size", type=int, default=512)
    p.add_argument("--train_latents_path", type=str, default=None)
    p.add_argument("--relax_iters", type=int, default=0,
                   help="relax geodesic and chord under the decoder's metric for this many iterations and add the better result")
    p.add_argument("--relax_metric", choices=("position", "image"), default="position",
                   help="image: relax each pair's sequences of whole 4x4 grids under the whole decoder (spatial builds)")
    return p


if __name__ == "__main__":
    main(make_parser().parse_args())
