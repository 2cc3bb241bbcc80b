"""Build a geodesic spatial codebook on the MI355X -- drop-in for the reference CLI
src/scripts/build_codebook.py (main :14-106, flags :108-134; same flags, same three artefacts;
--connect_components, an extension, bridges the graph's components and adds bridges.json).

    python -m vqvae_amd.scripts.build_codebook --latents_path z.pt --out_dir out --vae_ckpt_path best.pt \
        --in_channels 1 --output_image_size 28 --latent_dim 16 --enc_channels 64 128 256 \
        --dec_channels 256 128 64 --recon_loss mse --norm_type batch --mse_use_sigmoid \
        --k 20 --sym union --K 512 --init kpp --seed 42 --batch_size 512

Everything between loading the latents and writing the artefacts stays resident in HBM:
kNN (csrc/knn.hip) -> symmetric CSR + upper edge list (csrc/graph.hip) -> pull-back edge lengths
(csrc/jvp.hip) -> largest component + compaction (csrc/graph.hip) -> k-means++ / assignment over
geodesic distances (csrc/sssp.hip).
"""
import argparse
import time
from pathlib import Path
from typing import Dict, Optional

import numpy as np
import torch
from scipy import sparse

from .._device import DeviceCSR, device
from ..geo.kmeans_optimized import fit_kmedoids_optimized, fit_kmedoids_voronoi_graph
from ..geo.knn_graph_optimized import (bridge_components_device, compact_device, knn_graph_device, lcc_mask_device,
                                       reweight_device, upper_edges_device)
from ..geo.riemannian_metric import edge_lengths_graph_device, edge_lengths_riemannian
from ..parallel import RunningStatFold, sharded_edge_lengths, world_info
from ..spatial_decoder import DecoderExport, hip_kernels_cover, load_decoder_from_checkpoint


def build_codebook_device(z_flat: torch.Tensor, decoder, *, k: int = 20, sym: str = "union", K: int = 512,
                          init: str = "kpp", seed: int = 42, batch_size: int = 512,
                          timers: Optional[Dict[str, float]] = None, group=None, refine_iters: int = 0,
                          refine_power: int = 2, connect_components: bool = False) -> dict:
    """The hot path on resident data.  z_flat: f32 [n_nodes, d] on the GPU, rows in (n, h, w) order.
    Returns device/host results; `timers` (if given) receives per-stage seconds (synchronised).
    Under an initialised torch.distributed group the kNN rows and the JVP chunks are sharded over the
    ranks (vqvae_amd/parallel.py); every rank ends with the full result.
    refine_iters > 0 (extension): the seeded codebook is refined by up to that many cell-restricted medoid updates
    (fit_kmedoids_voronoi_graph, objective sum of distance^refine_power) and the result gains the key "refine" = {history,
    iterations, info}.  Every rank refines its full copy: the refinement is deterministic, so the ranks agree.
    connect_components (extension, off by default): the components of the kNN graph are bridged (bridge_components_device:
    the C - 1 minimum-spanning-tree edges of the component graph) right after the search, so the bridges get pull-back
    lengths through the JVP like every other edge and every latent gets a code; the result gains the key "bridges" =
    {edges, keys, components, rounds}.  Everything downstream is untouched, the zero-length drop and the largest-component
    rule included: a bridge between exact duplicates that gets pull-back length 0 is removed by the zero rule and the
    largest-component rule then applies as before.  Every rank bridges its full copy (deterministic: the ranks agree).
    With train-mode BatchNorm the extra edges move the chunk boundaries, so the other lengths change as with any change of
    the edge list."""
    dev = z_flat.device

    def tick(name, t0):
        if timers is not None:
            torch.cuda.synchronize(dev)
            timers[name] = timers.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    t0 = time.perf_counter()
    G, _, _ = knn_graph_device(z_flat, k, mode="connectivity", sym=sym, group=group, need_dist=False)
    bridges = None
    if connect_components:
        G, b_edges, b_keys, b_info = bridge_components_device(G, z_flat, mode="connectivity")
        bridges = {"edges": b_edges, "keys": b_keys, "components": b_info["components"], "rounds": b_info["rounds"]}
    src, dst, entry_edge = upper_edges_device(G)
    t0 = tick("knn", t0)

    print(f"Re-weighting {src.numel()} edges using Riemannian metric...")
    world = world_info(group)[1]
    sharded = {"knn": world > 1, "jvp": world > 1 and hip_kernels_cover(decoder)}   # what the ranks really split
    if hip_kernels_cover(decoder):
        export = DecoderExport(decoder, dev)
        fold = RunningStatFold(export, group)           # multi-rank: BatchNorm running statistics as one process leaves them
        fold.start()
        # whole chunks of `batch_size` edges per rank: every BatchNorm batch stays intact; every rank is told the build's edge
        # count, so a decoder with fixed statistics takes the route one process takes
        lengths = sharded_edge_lengths(
            int(src.numel()), batch_size,
            lambda e0, e1: edge_lengths_graph_device(export, z_flat, src[e0:e1], dst[e0:e1], batch_size,
                                                     build_edges=int(src.numel())), group)
        fold.finish(int(src.numel()), batch_size)
    else:       # e.g. GroupNorm: no kernel, autograd on the GPU (the reference's own method)
        lengths = edge_lengths_riemannian(decoder, z_flat[src.long()], z_flat[dst.long()], batch_size).contiguous()
    t0 = tick("jvp", t0)

    W_geo = reweight_device(G, entry_edge, lengths)
    has_zero = bool((lengths == 0).any())               # U + U^T drops entries that sum to exactly 0
    if has_zero:
        W_geo, _ = compact_device(W_geo, None, drop_zero=True)
    mask = lcc_mask_device(W_geo)
    n_lcc = int(mask.sum())
    if n_lcc < W_geo.n:
        print(f"Using LCC: {n_lcc}/{W_geo.n} nodes")
        W_lcc, _ = compact_device(W_geo, mask, drop_zero=False)
        z_lcc = z_flat[mask]
    else:
        W_lcc, z_lcc = W_geo, z_flat
    t0 = tick("lcc", t0)

    refine = None
    if refine_iters > 0:
        refine_info = {}
        medoids, assign_lcc, qe, history = fit_kmedoids_voronoi_graph(W_lcc, K=K, init=init, seed=seed, max_iter=refine_iters,
                                                                      power=refine_power, info=refine_info)
        refine = {"history": history, "iterations": len(history) - 1, "info": refine_info}
    else:
        medoids, assign_lcc, qe = fit_kmedoids_optimized(W_lcc, K=K, init=init, seed=seed)
    t0 = tick("kmedoids", t0)

    mask_h = mask.cpu().numpy()
    assign_flat = np.full(z_flat.shape[0], -1, dtype=np.int32)
    assign_flat[mask_h] = assign_lcc
    z_medoid = z_lcc[torch.from_numpy(medoids).to(dev)].cpu()
    res = {"W_lcc": W_lcc, "mask_lcc": mask_h, "medoids": medoids, "assign_flat": assign_flat, "qe": qe,
           "z_medoid": z_medoid, "n_edges": int(src.numel()), "edge_lengths": lengths, "edges": (src, dst),
           "sharded": sharded}
    if refine is not None:
        res["refine"] = refine
    if bridges is not None:
        res["bridges"] = bridges
    return res


def build_codebooks_pipelined(latent_sets, decoder, *, depth: int = 3, **kwargs) -> list:
    """build_codebook_device for several independent latent sets (f32 [n_i, d] on the GPU) with `depth` builds in flight
    (vqvae_amd/pipeline.py): same results as one after the other, 30-45 % more builds per second at the 60 000-latent size.
    Every slot works on its own copy of the decoder (train-mode BatchNorm updates running statistics in place).
    Under an initialised process group every build is sharded over the ranks as usual and the builds in flight issue their
    collectives in ticket order (parallel.CollectiveOrder: every rank must call this with the same sets in the same order)."""
    import copy
    from ..parallel import CollectiveOrder, OrderedGroup
    from ..pipeline import run_pipelined
    depth = max(1, min(depth, len(latent_sets)))
    decoders = [decoder] + [copy.deepcopy(decoder) for _ in range(depth - 1)]
    dev = latent_sets[0].device if len(latent_sets) else None
    pg = kwargs.pop("group", None)
    if world_info(pg)[1] <= 1 or depth == 1:
        return run_pipelined(lambda i, slot: build_codebook_device(latent_sets[i], decoders[slot], group=pg, **kwargs),
                             len(latent_sets), depth, dev)
    order = CollectiveOrder(len(latent_sets), depth)

    def one(i, slot):
        try:
            return build_codebook_device(latent_sets[i], decoders[slot], group=OrderedGroup(order, i, pg), **kwargs)
        except BaseException as e:                  # noqa: BLE001 -- the other builds must not wait for this one's tickets
            order.abort(e)
            raise
        finally:
            order.finish(i)

    return run_pipelined(one, len(latent_sets), depth, dev)


def main(args):
    """Builds a spatial codebook using a geodesic metric and saves artifacts."""
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    dev = device()

    decoder = load_decoder_from_checkpoint(
        args.vae_ckpt_path, in_channels=args.in_channels, dec_channels=args.dec_channels,
        latent_dim=args.latent_dim, output_image_size=args.output_image_size, norm_type=args.norm_type, device=dev)

    z = torch.load(Path(args.latents_path), map_location="cpu").float()
    N, C, H, W = z.shape
    print(f"Loaded spatial latents: N={N}, C={C}, H={H}, W={W}")
    z_flat = z.permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(dev)
    print(f"Reshaped to: {tuple(z_flat.shape)}")

    print(f"Building k-NN graph: N={z_flat.shape[0]}, k={args.k}, method=hip")
    res = build_codebook_device(z_flat, decoder, k=args.k, sym=args.sym, K=args.K, init=args.init, seed=args.seed,
                                batch_size=args.batch_size, refine_iters=getattr(args, "refine_iters", 0),
                                refine_power=getattr(args, "refine_power", 2),
                                connect_components=getattr(args, "connect_components", False))

    sparse.save_npz(out_dir / "knn_graph_geodesic.npz", res["W_lcc"].to_scipy())
    codes = res["assign_flat"].reshape(N, H, W)
    codebook = {
        "medoid_indices": res["medoids"].astype(np.int32),
        "z_medoid": res["z_medoid"].float(),
        "config": {key: getattr(args, key) for key in (
            "latents_path", "out_dir", "vae_ckpt_path", "in_channels", "output_image_size", "latent_dim",
            "enc_channels", "dec_channels", "recon_loss", "norm_type", "mse_use_sigmoid", "k", "sym", "K", "init",
            "seed", "batch_size")},
    }
    torch.save(codebook, out_dir / "codebook.pt")
    np.save(out_dir / "codes.npy", codes)
    if "refine" in res:                                 # --refine_iters N: a fourth artefact, the other three keep their format
        import json
        with open(out_dir / "refine.json", "w") as f:
            json.dump({"refine_iters": args.refine_iters, "refine_power": args.refine_power, "qe": res["qe"], **res["refine"]}, f, indent=1)
    if "bridges" in res:                                # --connect_components: bridges.json, the other three keep their format
        import json
        b = res["bridges"]
        src, dst = res["edges"]
        n_nodes = int(z_flat.shape[0])
        edge_key = src.long() * n_nodes + dst.long()    # ascending: the upper edges are in row-major order
        at = torch.searchsorted(edge_key, b["edges"][:, 0].long() * n_nodes + b["edges"][:, 1].long())
        with open(out_dir / "bridges.json", "w") as f:
            json.dump({"connect_components": True, "components": b["components"], "rounds": b["rounds"],
                       "edges": b["edges"].cpu().tolist(), "keys": b["keys"].cpu().tolist(),
                       "lengths": res["edge_lengths"][at].cpu().tolist()}, f, indent=1)
    print(f"Quantization error: {res['qe']:.3f}")
    print(f"Saved artifacts to: {out_dir}")
    return res


def make_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Build a geodesic spatial codebook.")
    for name in ("latents_path", "out_dir", "vae_ckpt_path"):
        parser.add_argument(f"--{name}", type=str, required=True)
    for name in ("in_channels", "output_image_size", "latent_dim"):
        parser.add_argument(f"--{name}", type=int, required=True)
    parser.add_argument("--enc_channels", type=int, nargs='+', required=True)
    parser.add_argument("--dec_channels", type=int, nargs='+', required=True)
    parser.add_argument("--recon_loss", type=str, required=True)
    parser.add_argument("--norm_type", type=str, required=True)
    parser.add_argument("--mse_use_sigmoid", action='store_true')
    parser.add_argument("--k", type=int, default=20)
    parser.add_argument("--sym", type=str, default="union")
    parser.add_argument("--K", type=int, default=512)
    parser.add_argument("--init", type=str, default="kpp")
    parser.add_argument("--seed", type=int, default=42)
    parser.add_argument("--batch_size", type=int, default=512)
    # extension: cell-restricted medoid updates after the seeding (0: the reference's codebook, artefacts unchanged)
    parser.add_argument("--refine_iters", type=int, default=0)
    parser.add_argument("--refine_power", type=int, default=2, choices=(1, 2))
    # extension: bridge the kNN graph's components so that every latent gets a code (writes bridges.json as well)
    parser.add_argument("--connect_components", action='store_true')
    return parser


if __name__ == "__main__":
    main(make_parser().parse_args())
