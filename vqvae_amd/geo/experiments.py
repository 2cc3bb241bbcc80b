"""The Riemannian graph experiments (the reference's experiments/geo/riemann_sanity_check.py and
run_riemann_experiments.py) on the MI355X: does the decoder's pull-back metric change the kNN graph?

    riemann_sanity(z, decoder)             Euclidean vs Riemannian length on sampled kNN entries: correlation, mean ratio
    riemann_graph_effects(z, decoder)      components, LCC size and mean shortest-path distance before / after re-weighting
    mean_shortest_path_device(G, sources)  the mean of the finite, positive entries of the S x N distance matrix
    reweight_edges_symmetric_device(...)   W[i, j] = W[j, i] = v on a resident CSR
    mean_shortest_path, pick_sources_from_lcc, stratified_edge_sample      the reference's helpers, same rules

Latents, graph, lengths and distance blocks stay on the device: the S x N blocks are reduced there by geo_path_stats and
the sampled entries are written by geo_csr_set_symmetric (csrc/graph_effects.hip).  The host sees the component labels'
counts, the stored distances of the upper-triangle edges (the stratified draw is the reference's seeded numpy chain), the
sampled index lists and scalars.  DESIGN.md section 16.
"""
import math
from typing import Dict, Optional

import numpy as np
import torch
from scipy import sparse

from .. import _lib
from .._device import DeviceCSR, device, ptr, stream_ptr
from ..vanilla_decoder import VanillaDecoderExport, vanilla_kernels_cover
from .geo_shortest_paths import _normalise_sources, _pull_structure, ensure_valid_graph, sssp_multi_device
from .knn_graph_optimized import (connected_components_device, knn_graph_device, largest_connected_component, lcc_mask_device,
                                  reweight_device, upper_edges_device)
from .riemannian_metric import edge_lengths_riemannian, edge_lengths_vanilla_graph_device

DEFAULT_BLOCK_BYTES = 1 << 30          # distance block solved and reduced at a time (4 473 sources at 60 000 nodes)
MAX_CORR_EDGES = 16384                 # geo_image_pair_moments' row length: longer vectors are reduced in pieces


# ---- device steps -------------------------------------------------------------------------------------------------------------
def path_stats_device(D: torch.Tensor, n: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """geo_path_stats on the rows of D (f32 [S][>= n] on the GPU, unit column stride): per row the fp64 sum and the count
    of the finite entries > 0, the count of +inf entries and the largest finite entry (0 without one).  Device tensors."""
    if not (torch.is_tensor(D) and D.is_cuda and D.dtype == torch.float32 and D.dim() == 2 and D.stride(1) == 1):
        raise ValueError("D must be a float32 [S][n] tensor on the GPU with contiguous rows")
    S = int(D.shape[0])
    n = int(D.shape[1]) if n is None else int(n)
    if S < 1 or not 1 <= n <= D.shape[1]:
        raise ValueError(f"path_stats_device: S={S}, n={n} for a block of shape {tuple(D.shape)}")
    dev = D.device
    out = {"sum": torch.empty(S, dtype=torch.float64, device=dev), "n_pos": torch.empty(S, dtype=torch.int64, device=dev),
           "n_unreached": torch.empty(S, dtype=torch.int64, device=dev), "max": torch.empty(S, dtype=torch.float32, device=dev)}
    ld = int(D.stride(0)) if S > 1 else max(int(D.stride(0)), n)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().geo_path_stats(ptr(D), ld, S, n, ptr(out["sum"]), ptr(out["n_pos"]), ptr(out["n_unreached"]),
                                              ptr(out["max"]), stream_ptr()), "geo_path_stats")
    return out


def _i32_device(a, dev) -> torch.Tensor:
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.int64))
    return a.to(dev).to(torch.int32).contiguous()


def reweight_edges_symmetric_device(G: DeviceCSR, src, dst, lengths, *, assume_unique: bool = False) -> DeviceCSR:
    """A copy of G (shared structure, new data) with W[src[t], dst[t]] = W[dst[t], src[t]] = lengths[t]: the reference's
    `W.tolil(); W[i, j] = W[j, i] = v; W.tocsr()` on existing entries, by geo_csr_set_symmetric.  The pairs must be
    unique as unordered pairs (checked here, on the host copy of the list, unless the caller vouches for it with
    assume_unique) and every pair must be a stored entry in both directions: otherwise ValueError, and G is left as it was.  A zero length stays a stored entry (scipy drops it)."""
    dev = G.indptr.device
    if G.data is None:
        raise ValueError("reweight_edges_symmetric_device needs a weighted graph")
    s, d = _i32_device(src, dev), _i32_device(dst, dev)
    v = lengths if torch.is_tensor(lengths) else torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.float32))
    v = v.to(dev, torch.float32).contiguous()
    m = int(s.numel())
    if d.numel() != m or v.numel() != m:
        raise ValueError(f"src, dst and lengths must have one length, got {m}, {d.numel()}, {v.numel()}")
    if m and not assume_unique:
        sh, dh = s.cpu().numpy().astype(np.int64), d.cpu().numpy().astype(np.int64)
        key = np.minimum(sh, dh) * (int(G.n) + 1) + np.maximum(sh, dh)
        if np.unique(key).size != m:
            raise ValueError("reweight_edges_symmetric_device: the pair list repeats an edge")
    data = G.data.clone()
    n_missing = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().geo_csr_set_symmetric(ptr(G.indptr), ptr(G.indices), ptr(data), G.n, ptr(s), ptr(d), ptr(v), m,
                                                     ptr(n_missing), stream_ptr()), "geo_csr_set_symmetric")
    missing = int(n_missing.item())
    if missing:
        raise ValueError(f"reweight_edges_symmetric_device: {missing} of {m} pairs are not stored in both directions")
    return DeviceCSR(G.n, G.indptr, G.indices, data)


def mean_shortest_path_device(G: DeviceCSR, sources, *, max_block_bytes: int = DEFAULT_BLOCK_BYTES) -> dict:
    """Mean of the finite, positive shortest-path distances from `sources` (the reference's mean_shortest_path) on a resident
    symmetric graph.  The sources are solved in blocks of max_block_bytes / (4 n) rows (geo_sssp_multi), every block is
    reduced on the device (geo_path_stats), and the per-source sums and counts are added on the host in source order, in
    fp64.  A source's row does not depend on its block and a row's reduction does not depend on the other rows, so the
    block size changes no returned value.  Returns mean (inf when no entry qualifies), sum f64 [S], count i64 [S],
    unreached i64 [S], n_unreached, max (the largest finite distance seen: a lower bound of the eccentricities'
    maximum), n_sources."""
    dev = G.indptr.device
    src = _normalise_sources(sources.cpu().numpy() if torch.is_tensor(sources) else sources, G.n)
    S, n = int(src.size), int(G.n)
    if S == 0 or n == 0:
        raise ValueError("mean_shortest_path_device needs at least one source and one node")
    src_dev = torch.from_numpy(src.astype(np.int32)).to(dev)
    block = max(1, min(S, int(max_block_bytes) // (4 * n)))
    parts = []
    for s0 in range(0, S, block):
        D, _, _, _, _ = sssp_multi_device(G, src_dev[s0:s0 + block].contiguous(), want_D=True)
        parts.append(path_stats_device(D))
        del D
    sums = torch.cat([p["sum"] for p in parts]).cpu().numpy()
    counts = torch.cat([p["n_pos"] for p in parts]).cpu().numpy()
    unreached = torch.cat([p["n_unreached"] for p in parts]).cpu().numpy()
    maxima = torch.cat([p["max"] for p in parts]).cpu().numpy()
    total, count = 0.0, 0
    for s_, c_ in zip(sums.tolist(), counts.tolist()):              # source order, fp64
        total += s_
        count += c_
    return {"mean": total / count if count > 0 else float("inf"), "sum": sums, "count": counts, "unreached": unreached,
            "n_unreached": int(unreached.sum()), "max": float(maxima.max()), "n_sources": S}


# ---- the reference's helpers -----------------------------------------------------------------------------------------------
def _device_graph(W) -> DeviceCSR:
    if isinstance(W, DeviceCSR):
        return W
    return DeviceCSR.from_scipy(_pull_structure(ensure_valid_graph(W), directed=False), device())


def mean_shortest_path(W: sparse.spmatrix, sources_idx) -> float:
    """run_riemann_experiments.py:54-58: a scipy matrix in, a Python float out (inf when no distance is finite and > 0)."""
    return float(mean_shortest_path_device(_device_graph(W), sources_idx)["mean"])


def pick_sources_from_lcc(W, num_sources: int, rng: np.random.RandomState) -> np.ndarray:
    """run_riemann_experiments.py:60-63: np.where(largest_connected_component(W))[0], then rng.choice(..., replace=False).
    W: scipy matrix or DeviceCSR."""
    mask = lcc_mask_device(W).cpu().numpy() if isinstance(W, DeviceCSR) else largest_connected_component(W)
    lcc_nodes = np.where(mask)[0]
    return rng.choice(lcc_nodes, size=min(num_sources, len(lcc_nodes)), replace=False)


def stratified_edge_sample(lengths: np.ndarray, sample_edges: int, num_bins: int, rng: np.random.RandomState) -> np.ndarray:
    """run_riemann_experiments.py:121-136: positions into `lengths` (the Euclidean lengths of the upper-triangle edges, in
    edge order), sample_edges // num_bins from every quantile bin, bins in order, by the seeded legacy chain `rng`."""
    distances = np.asarray(lengths)
    quantiles = np.quantile(distances, np.linspace(0, 1, num_bins + 1)[1:-1])
    bins = np.digitize(distances, quantiles)
    n_per_bin = max(1, sample_edges // num_bins)
    selected = []
    for b in range(num_bins):
        candidates = np.where(bins == b)[0]
        if len(candidates) > 0:
            n_take = min(n_per_bin, len(candidates))
            selected.extend(rng.choice(candidates, n_take, replace=False))
    return np.asarray(selected, dtype=np.int64)


# ---- the experiments -------------------------------------------------------------------------------------------------------
def _resident_latents(z) -> torch.Tensor:
    if not torch.is_tensor(z):
        z = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32))
    if z.dim() != 2:
        raise ValueError(f"z must be (N, D), got {tuple(z.shape)}")
    return z.detach().to(device(), torch.float32).contiguous()


def _entry_rows(G: DeviceCSR) -> torch.Tensor:
    """Row index of every stored entry (int64 on the device): with G.indices, scipy's W.nonzero() in row-major order."""
    deg = (G.indptr[1:] - G.indptr[:-1]).long()
    return torch.repeat_interleave(torch.arange(G.n, device=G.indptr.device), deg, output_size=G.nnz)


def _edge_lengths(decoder, z_dev: torch.Tensor, src: torch.Tensor, dst: torch.Tensor, batch_size: int) -> torch.Tensor:
    """Pull-back lengths of the edges (src[e], dst[e]) over the resident latents, f32 on z_dev's device: the graph entry
    point of the vanilla kernels where they cover the decoder, edge_lengths_riemannian on gathered endpoints otherwise."""
    if vanilla_kernels_cover(decoder):
        export = VanillaDecoderExport(decoder, z_dev.device)
        return edge_lengths_vanilla_graph_device(export, z_dev, src, dst)
    return edge_lengths_riemannian(decoder, z_dev[src.long()], z_dev[dst.long()], batch_size=batch_size).to(z_dev.device)


def _components(G: DeviceCSR):
    ncomp, labels = connected_components_device(G)
    return ncomp, int(torch.bincount(labels.long(), minlength=max(ncomp, 1)).max())


def sample_knn_entries(z, *, k: int = 10, max_edges: int = 2000, seed: int = 0) -> dict:
    """The sanity check's draw (riemann_sanity_check.py:74-88): min(max_edges, nnz) stored entries of the k-mutual kNN graph by
    RandomState(seed).choice(nnz, n_edges, replace=False) from W.nonzero()'s row-major order.  Device tensors z, i, j (int64),
    de (the stored distances, f32) and the host array `indices`."""
    z_dev = _resident_latents(z)
    G, _, _ = knn_graph_device(z_dev, k, mode="distance", sym="mutual", need_dist=False)
    n_edges = min(int(max_edges), G.nnz)
    if n_edges < 2:
        raise ValueError(f"riemann_sanity: the graph has {G.nnz} stored entries, at least 2 are needed")
    indices = np.random.RandomState(seed).choice(G.nnz, n_edges, replace=False)
    pick = torch.from_numpy(np.asarray(indices, dtype=np.int64)).to(z_dev.device)
    return {"z": z_dev, "i": _entry_rows(G)[pick], "j": G.indices[pick].long(), "de": G.data[pick].contiguous(),
            "indices": np.asarray(indices)}


def pearson_device(x: torch.Tensor, y: torch.Tensor) -> float:
    """Pearson correlation of two f32 device vectors in fp64 from geo_image_pair_moments (centred variance and covariance of
    one "image pair" of E pixels).  Longer vectors than the kernel's 16 384 pixels are cut into pieces of that length, one
    call per piece length, and the pieces' fp64 moments are pooled on the host in piece order:
    var = sum n_p (var_p + (mean_p - mean)^2) / n, likewise the covariance."""
    from ..eval.metrics import image_pair_moments
    E = int(x.numel())
    moms, sizes = [], []
    full = E // MAX_CORR_EDGES
    if full:
        cut = full * MAX_CORR_EDGES
        moms.append(image_pair_moments(x[:cut].view(full, MAX_CORR_EDGES), y[:cut].view(full, MAX_CORR_EDGES)).cpu().numpy())
        sizes += [MAX_CORR_EDGES] * full
    if E % MAX_CORR_EDGES:
        cut = full * MAX_CORR_EDGES
        moms.append(image_pair_moments(x[None, cut:], y[None, cut:]).cpu().numpy())
        sizes.append(E - cut)
    mom, w = np.concatenate(moms), np.asarray(sizes, dtype=np.float64)
    mx, my = float((w * mom[:, 0]).sum() / E), float((w * mom[:, 1]).sum() / E)
    vx = float((w * (mom[:, 2] + (mom[:, 0] - mx) ** 2)).sum() / E)
    vy = float((w * (mom[:, 3] + (mom[:, 1] - my) ** 2)).sum() / E)
    cov = float((w * (mom[:, 4] + (mom[:, 0] - mx) * (mom[:, 1] - my))).sum() / E)
    denom = math.sqrt(vx * vy)
    return cov / denom if denom > 0 else float("nan")


def riemann_sanity(z, decoder, *, k: int = 10, max_edges: int = 2000, seed: int = 0, batch_size: int = 256,
                   sample: Optional[dict] = None) -> dict:
    """riemann_sanity_check.py:74-104.  The entries of sample_knn_entries (`sample`: an earlier draw on the same z, as the CLI
    makes before it loads the decoder); de = the stored distances, dr = edge_lengths_riemannian; ratio = float32 mean of
    dr / (de + 1e-8); corr = pearson_device(de, dr).  Returns corr, ratio, de, dr (float32 arrays), i, j, indices."""
    if sample is None:
        sample = sample_knn_entries(z, k=k, max_edges=max_edges, seed=seed)
    z_dev, i, j, de = sample["z"], sample["i"], sample["j"], sample["de"]
    dec_dev = next(decoder.parameters()).device
    with torch.no_grad():
        dr = edge_lengths_riemannian(decoder, z_dev[i].to(dec_dev), z_dev[j].to(dec_dev), batch_size=batch_size)
    dr = dr.to(z_dev.device, torch.float32).contiguous()
    corr = pearson_device(de, dr)
    de_h, dr_h = de.cpu().numpy(), dr.cpu().numpy()
    ratio = np.mean(dr_h / (de_h + 1e-8))                                        # float32, as the reference computes it
    return {"corr": corr, "ratio": ratio, "de": de_h, "dr": dr_h, "i": i.cpu().numpy(), "j": j.cpu().numpy(),
            "indices": sample["indices"]}


def riemann_graph_effects(z, decoder, *, k: int = 10, mode: str = "subset", sample_edges: int = 5000, num_bins: int = 5,
                          num_sources: int = 8, seed: int = 0, batch_size: int = 256) -> dict:
    """run_riemann_experiments.py:84-166.  k-mutual kNN graph with Euclidean weights; components, LCC size and the mean
    shortest-path distance from num_sources LCC nodes; then the same on the graph whose selected edges carry the decoder's
    pull-back lengths (both directions).  mode "subset": sample_edges edges stratified over num_bins quantile bins of the
    stored Euclidean lengths; "full": every upper-triangle edge.  One RandomState(seed), consumed by the source pick and
    then by the bins; the same sources serve both graphs.  Returns the keys the reference saves plus sources, i_sel, j_sel,
    riem_lengths, euc_lengths (of the selected edges), n_zero_lengths and the two mean_shortest_path_device results."""
    if mode not in ("subset", "full"):
        raise ValueError(f"mode must be 'subset' or 'full', got {mode!r}")
    rng = np.random.RandomState(seed)
    z_dev = _resident_latents(z)
    G, _, _ = knn_graph_device(z_dev, k, mode="distance", sym="mutual", need_dist=False)
    ncomp_euc, lcc_size_euc = _components(G)
    src = pick_sources_from_lcc(G, num_sources, rng)
    sp_euc = mean_shortest_path_device(G, src)

    e_src, e_dst, entry_edge = upper_edges_device(G)
    euc_upper = G.data[_entry_rows(G) < G.indices.long()]                        # edge order: row-major, row < col
    if mode == "full":
        i_sel, j_sel, euc_sel = e_src, e_dst, euc_upper
        riem = _edge_lengths(decoder, z_dev, i_sel, j_sel, batch_size)
        G_riem = reweight_device(G, entry_edge, riem)
    else:
        selected = stratified_edge_sample(euc_upper.cpu().numpy(), sample_edges, num_bins, rng)
        sel = torch.from_numpy(selected).to(z_dev.device)
        i_sel, j_sel, euc_sel = e_src[sel].contiguous(), e_dst[sel].contiguous(), euc_upper[sel]
        riem = _edge_lengths(decoder, z_dev, i_sel, j_sel, batch_size)
        G_riem = reweight_edges_symmetric_device(G, i_sel, j_sel, riem, assume_unique=True)   # distinct positions of the edge list
    n_zero = int((riem == 0).sum())
    if n_zero:
        print(f"Warning: {n_zero} re-weighted edges have zero Riemannian length (duplicate latents); they stay in the graph")

    ncomp_r, lcc_size_r = _components(G_riem)
    sp_riem = mean_shortest_path_device(G_riem, src)
    mean_sp_euc, mean_sp_r = sp_euc["mean"], sp_riem["mean"]
    ratio_sp = mean_sp_r / mean_sp_euc if np.isfinite(mean_sp_euc) else np.inf
    return {"ncomp_euc": ncomp_euc, "lcc_size_euc": lcc_size_euc, "mean_sp_euc": mean_sp_euc,
            "ncomp_riem": ncomp_r, "lcc_size_riem": lcc_size_r, "mean_sp_riem": mean_sp_r, "ratio_sp": ratio_sp,
            "reweight_mode": mode, "sample_edges": int(i_sel.numel()), "k": int(k), "num_sources": int(len(src)),
            "sources": np.asarray(src), "i_sel": i_sel.cpu().numpy().copy(), "j_sel": j_sel.cpu().numpy().copy(),   # (owning arrays: scipy's fancy indexing refuses views of tensor memory)
            "riem_lengths": riem.cpu().numpy(), "euc_lengths": euc_sel.cpu().numpy(), "n_zero_lengths": n_zero,
            "paths_euc": sp_euc, "paths_riem": sp_riem, "graph_euc": G, "graph_riem": G_riem}
