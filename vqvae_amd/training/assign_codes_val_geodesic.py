"""Geodesic code assignment of latents that are NOT nodes of the training graph (validation / test sets).

The reference's result notes name `src/training/assign_codes_val_geodesic.py` ("robust geodesic assignment with
connectivity safeguards", docs/results/cifar10_quantization_analysis.md:147: it replaced a Euclidean nearest-medoid
assignment of the validation set) but the file is not in its repository.  This is a definition of that step in terms of
the pieces the training path already has, not a restatement (no oracle in the reference):

  1. every new latent v is attached to its k nearest graph nodes (exact fp64 squared Euclidean distances, ties by index);
     only nodes of the graph handed in take part -- with the LCC graph of build_codebook_device that is the
     connectivity safeguard: a neighbour outside the connected component can never carry the path;
  2. an attachment edge is as long as the training edges are: the decoder pull-back length
     (geo/riemannian_metric.py, same kernels, chunks of `batch_size` edges) when a decoder is given, else Euclidean;
  3. dist(v, medoid m) = min over the k attachments u of  len(v, u) + D[m][u]  with D the medoids' geodesic rows on the
     training graph (geo_sssp_multi); the code of v is the first medoid with the smallest distance
     (geo_attach_argmin).  A latent that coincides with a graph node and is attached along graph edges only (k not larger
     than the graph's own k) gets exactly that node's assignment and distance.

numpy restatement: oracle/pipeline.py (assign_new_latents); tests: tests/test_gpu_voronoi.py.

Command line (main below): python -m vqvae_amd.training.assign_codes_val_geodesic --codebook_dir DIR --latents_path VAL/z.pt
--out_dir OUT, against the artefacts of vqvae_amd.scripts.build_codebook; its step 1 is the kernel search
geo.knn_graph_optimized.knn_query_device(form=0), handed to assign_codes_geodesic through `neighbors`
(tests: tests/test_gpu_assign_val_cli.py, tests/test_knn_query_host.py).
"""
from typing import Dict, Optional

import numpy as np
import torch

from .. import _lib
from .._device import DeviceCSR, ptr, stream_ptr
from ..geo.geo_shortest_paths import sssp_multi_device


def attach_neighbors_device(z_new: torch.Tensor, z_graph: torch.Tensor, k: int, rows_per_block: int = 0):
    """(idx int32 [V, k'], d2 f64 [V, k']) with k' = min(k, n): the k' nearest graph nodes of every new latent, ranked by
    the fp64 squared distance accumulated dimension by dimension (sum_k (a_k - b_k)^2, ascending k), ties by node index."""
    V, n, d = int(z_new.shape[0]), int(z_graph.shape[0]), int(z_graph.shape[1])
    kk = min(int(k), n)
    dev = z_graph.device
    idx = torch.empty((V, kk), dtype=torch.int32, device=dev)
    d2 = torch.empty((V, kk), dtype=torch.float64, device=dev)
    if V == 0 or kk == 0:
        return idx, d2
    b64 = z_graph.to(torch.float64)
    step = rows_per_block or max(1, (1 << 26) // max(1, n))            # <= 512 MiB of fp64 distances per block
    for r0 in range(0, V, step):
        a64 = z_new[r0:r0 + step].to(device=dev, dtype=torch.float64)
        acc = torch.zeros((a64.shape[0], n), dtype=torch.float64, device=dev)
        for c in range(d):                                              # one rounding per dimension, the oracle's order
            diff = a64[:, c:c + 1] - b64[:, c].unsqueeze(0)
            acc += diff * diff
        vals, order = torch.sort(acc, dim=1, stable=True)              # stable: equal distances keep ascending index
        idx[r0:r0 + step] = order[:, :kk].to(torch.int32)
        d2[r0:r0 + step] = vals[:, :kk]
    return idx, d2


def assign_codes_geodesic(z_new: torch.Tensor, z_graph: torch.Tensor, G: DeviceCSR, medoids, *, k: int = 20,
                          decoder=None, batch_size: int = 512, D_rows: Optional[torch.Tensor] = None, neighbors=None) -> Dict:
    """z_new f32 [V, d] (any device), z_graph f32 [n, d] = the latents of G's nodes on the GPU, G = the geodesic training
    graph (e.g. W_lcc of build_codebook_device), medoids = node indices of G.  Returns a dict: codes int64 [V] (position
    in `medoids`), dist f32 [V], neighbors int32 [V, k], lengths f32 [V, k].
    neighbors: a precomputed attachment (idx int32 [V, k'], d2 f64 [V, k']) on the GPU, e.g. of
    geo.knn_graph_optimized.knn_query_device(z_graph, z_new, k', form=0), used in place of the torch search below; `k` is
    then not consulted.  Its d2 are fma chains where attach_neighbors_device rounds product and sum separately: keys a few
    ulps apart, which can swap near-ties and move a Euclidean length by a float32 ulp -- hence a keyword, not a new default."""
    lib = _lib.load()
    dev = z_graph.device
    z_new = z_new.to(device=dev, dtype=torch.float32).contiguous()
    V, n = int(z_new.shape[0]), G.n
    assert int(z_graph.shape[0]) == n, "z_graph must hold one latent per node of G"
    med = torch.from_numpy(np.asarray(medoids, dtype=np.int32)).to(dev)
    K = int(med.numel())
    if neighbors is None:
        idx, d2 = attach_neighbors_device(z_new, z_graph, k)
    else:
        idx, d2 = neighbors
        if idx.dtype != torch.int32 or d2.dtype != torch.float64 or idx.shape != d2.shape or idx.dim() != 2 \
                or int(idx.shape[0]) != V:
            raise ValueError(f"neighbors must be (int32 [V, k'], float64 [V, k']) with V = {V}, got {idx.dtype} "
                             f"{tuple(idx.shape)} and {d2.dtype} {tuple(d2.shape)}")
        idx, d2 = idx.to(dev).contiguous(), d2.to(dev).contiguous()
    kk = int(idx.shape[1])
    if decoder is not None and V > 0:
        from ..geo.riemannian_metric import edge_lengths_graph_device, edge_lengths_riemannian
        from ..spatial_decoder import DecoderExport, hip_kernels_cover
        z_cat = torch.cat([z_graph, z_new], dim=0).contiguous()
        src = (n + torch.arange(V, dtype=torch.int32, device=dev)).repeat_interleave(kk)
        dst = idx.reshape(-1).contiguous()
        if hip_kernels_cover(decoder):
            lengths = edge_lengths_graph_device(DecoderExport(decoder, dev), z_cat, src, dst, batch_size)
        else:
            lengths = edge_lengths_riemannian(decoder, z_cat[src.long()], z_cat[dst.long()], batch_size)
        lengths = lengths.reshape(V, kk).contiguous()
    else:
        lengths = torch.sqrt(d2).to(torch.float32).contiguous()
    if D_rows is None:
        D_rows, _, _, _, _ = sssp_multi_device(G, med, want_D=True)      # [K, n]
    Dt = D_rows.t().contiguous()                                         # [n, K]: a node's K distances are contiguous
    dist = torch.empty(V, dtype=torch.float32, device=dev)
    arg = torch.empty(V, dtype=torch.int32, device=dev)
    if V > 0:
        with torch.cuda.device(dev):
            _lib.check(lib.geo_attach_argmin(ptr(Dt), Dt.stride(0), K, ptr(idx), ptr(lengths), kk, V, ptr(dist), ptr(arg),
                                             stream_ptr()), "geo_attach_argmin")
    return {"codes": arg.to(torch.int64), "dist": dist, "neighbors": idx, "lengths": lengths}


# --------------------------------------------------------------------------------- command line
def lcc_rows(codes: np.ndarray) -> np.ndarray:
    """Rows of the flattened training latents that are nodes of the LCC graph, in node order: build_codebook writes -1 into
    codes.npy for every position outside the largest component and compacts the others in row order."""
    return np.flatnonzero(np.asarray(codes).reshape(-1) >= 0)


def flatten_latents(z: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] -> [N H W, C] in (n, h, w) order, as build_codebook flattens its latents; [N, d] as it is."""
    if z.dim() == 4:
        return z.permute(0, 2, 3, 1).reshape(-1, z.shape[1]).contiguous()
    if z.dim() == 2:
        return z.contiguous()
    raise ValueError(f"latents must be [N, C, H, W] or [N, d], got shape {tuple(z.shape)}")


def load_build(codebook_dir, train_latents_path=None):
    """What build_codebook left in `codebook_dir`, put back together: (codebook dict, W_lcc scipy CSR, z_lcc f32 [n, d] on the
    host).  Raises ValueError when the pieces do not belong together: z_lcc[medoid_indices] must equal z_medoid bit for bit."""
    from pathlib import Path
    from scipy import sparse
    cb_dir = Path(codebook_dir)
    codebook = torch.load(cb_dir / "codebook.pt", map_location="cpu", weights_only=False)
    W = sparse.load_npz(cb_dir / "knn_graph_geodesic.npz").tocsr()
    codes = np.load(cb_dir / "codes.npy")
    path = train_latents_path or codebook["config"]["latents_path"]
    z_train = flatten_latents(torch.load(path, map_location="cpu").float())
    rows = lcc_rows(codes)
    if codes.size != z_train.shape[0] or rows.size != W.shape[0]:
        raise ValueError(f"{cb_dir}: codes.npy has {codes.size} positions ({rows.size} in the graph), the training latents "
                         f"{path} {z_train.shape[0]} rows and knn_graph_geodesic.npz {W.shape[0]} nodes: "
                         "the artefacts do not belong together")
    z_lcc = z_train[torch.from_numpy(rows)].contiguous()
    med = torch.from_numpy(np.asarray(codebook["medoid_indices"], dtype=np.int64))
    if int(med.numel()) and (int(med.min()) < 0 or int(med.max()) >= z_lcc.shape[0]):
        raise ValueError(f"{cb_dir}: codebook.pt names medoid {int(med.max())} of a graph of {z_lcc.shape[0]} nodes: "
                         "the artefacts do not belong together")
    z_med = codebook["z_medoid"].float()
    if z_med.shape != z_lcc[med].shape or not torch.equal(z_lcc[med].view(torch.int32), z_med.contiguous().view(torch.int32)):
        raise ValueError(f"{cb_dir}: the training latents at the rows codebook.pt names as medoids are not its z_medoid: "
                         "codebook.pt, codes.npy, knn_graph_geodesic.npz and the training latents do not belong together")
    return codebook, W, z_lcc


def main(args):
    """Geodesic codes of held-out latents against a codebook built by vqvae_amd.scripts.build_codebook.

        python -m vqvae_amd.training.assign_codes_val_geodesic --codebook_dir DIR --latents_path VAL/z.pt --out_dir OUT
               [--k 20] [--metric riemannian|euclidean] [--batch_size 512] [--train_latents_path PATH]

    Reads codebook.pt, knn_graph_geodesic.npz and codes.npy from DIR and the training latents named in codebook.pt's config
    (or --train_latents_path), attaches every held-out latent to its k nearest graph nodes with knn_query_device(form=0) --
    step 1 of the module docstring: direct squared differences -- and assigns it as assign_codes_geodesic does; the medoid
    rows are solved once.  --metric riemannian (default) measures the attachment edges through the decoder of the build's
    checkpoint IN eval() MODE: the build measures its edges with train-mode BatchNorm and leaves the running statistics it
    found in the checkpoint untouched, and attachment batches of held-out latents must not move BatchNorm statistics nor
    depend on how they fall into batches.  --metric euclidean takes the Euclidean length of the attachment edges.
    Writes codes_val.npy (int32, the latents' leading shape), dist_val.npy (f32) and assign_val.json."""
    import json
    from pathlib import Path
    from .._device import device
    from ..geo.knn_graph_optimized import knn_query_device
    if args.metric not in ("riemannian", "euclidean"):
        raise ValueError(f"metric must be 'riemannian' or 'euclidean', got '{args.metric}'")
    out_dir = Path(args.out_dir)
    codebook, W, z_lcc = load_build(args.codebook_dir, args.train_latents_path)
    z_val = torch.load(Path(args.latents_path), map_location="cpu").float()
    lead = (z_val.shape[0], z_val.shape[2], z_val.shape[3]) if z_val.dim() == 4 else (z_val.shape[0],)
    z_new = flatten_latents(z_val)
    if z_new.shape[1] != z_lcc.shape[1]:
        raise ValueError(f"held-out latents have {z_new.shape[1]} channels, the codebook's graph {z_lcc.shape[1]}")
    dev = device()
    decoder = None
    if args.metric == "riemannian":
        from ..spatial_decoder import load_decoder_from_checkpoint
        cfg = codebook["config"]
        decoder = load_decoder_from_checkpoint(
            cfg["vae_ckpt_path"], in_channels=cfg["in_channels"], dec_channels=cfg["dec_channels"], latent_dim=cfg["latent_dim"],
            output_image_size=cfg["output_image_size"], norm_type=cfg["norm_type"], device=dev)
        decoder.eval()
    G = DeviceCSR.from_scipy(W, dev)
    z_graph, z_new = z_lcc.to(dev), z_new.to(dev)
    kk = min(int(args.k), int(z_graph.shape[0]))
    if kk < 1:
        raise ValueError(f"k = {args.k}: at least one attachment per latent is needed")
    neighbors = knn_query_device(z_graph, z_new, kk, form=0)
    knn_path = int(_lib.load().geo_knn_last_path())
    out = assign_codes_geodesic(z_new, z_graph, G, codebook["medoid_indices"], k=kk, decoder=decoder,
                                batch_size=args.batch_size, neighbors=neighbors)
    codes = out["codes"].to(torch.int32).cpu().numpy().reshape(lead)
    dist = out["dist"].cpu().numpy().astype(np.float32).reshape(lead)
    finite = np.isfinite(dist)
    summary = {"n_latents": int(z_new.shape[0]), "k": kk, "metric": args.metric, "knn_path": knn_path,
               "unreachable": int((~finite).sum()),
               "quantization_error": float(np.sum(dist[finite].astype(np.float32) ** 2)) if finite.any() else float("inf")}
    out_dir.mkdir(parents=True, exist_ok=True)
    np.save(out_dir / "codes_val.npy", codes)
    np.save(out_dir / "dist_val.npy", dist)
    with open(out_dir / "assign_val.json", "w") as f:
        json.dump(summary, f, indent=2)
    print(f"Assigned {summary['n_latents']} latents (k={kk}, {args.metric}); unreachable: {summary['unreachable']}; "
          f"quantization error: {summary['quantization_error']:.3f}")
    print(f"Saved artifacts to: {out_dir}")
    return out


def make_parser():
    import argparse
    parser = argparse.ArgumentParser(description="Geodesic codes of held-out latents against a built codebook.")
    for name in ("codebook_dir", "latents_path", "out_dir"):
        parser.add_argument(f"--{name}", type=str, required=True)
    parser.add_argument("--k", type=int, default=20)
    parser.add_argument("--metric", type=str, default="riemannian", choices=("riemannian", "euclidean"))
    parser.add_argument("--batch_size", type=int, default=512)
    parser.add_argument("--train_latents_path", type=str, default=None)
    return parser


if __name__ == "__main__":
    main(make_parser().parse_args())
