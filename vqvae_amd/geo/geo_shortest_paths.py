"""Geodesic shortest paths on the MI355X -- same API as the reference's
src/geo/geo_shortest_paths.py (ensure_valid_graph :13, dijkstra_multi_source :24,
dijkstra_single_source :53, distances_between :66), with scipy's Dijkstra replaced by the fp64
label-correcting kernels of csrc/sssp.hip (geo_sssp_multi).  Host objects in, host objects out.
An extension below: the paths themselves (geodesic_paths, geodesic_paths_device, csrc/paths.hip)."""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
from scipy import sparse

from .. import _lib
from .._device import DeviceCSR, device, ptr, ptr_or_stand_in, stream_ptr, workspace


def ensure_valid_graph(W: sparse.spmatrix) -> sparse.spmatrix:
    """Same checks and exception classes as geo_shortest_paths.py:13-21."""
    if not sparse.isspmatrix(W):
        raise TypeError("W must be a scipy sparse matrix")
    if W.shape[0] != W.shape[1]:
        raise ValueError("W must be square")
    if W.nnz > 0 and (W.data < 0).any():
        raise ValueError("Negative weights")
    return W.tocsr()


def _pull_structure(W: sparse.csr_matrix, directed: bool) -> sparse.csr_matrix:
    """CSR whose row v lists the edges INTO v.  Undirected solves use every stored entry in both
    directions (scipy relaxes along csr and csr^T); duplicates are kept as parallel edges, the
    kernel takes the minimum over them."""
    WT = W.T.tocsr()
    if directed:
        return WT
    W = W.copy() if not W.has_sorted_indices else W
    W.sort_indices()
    WT.sort_indices()
    if (np.array_equal(W.indptr, WT.indptr) and np.array_equal(W.indices, WT.indices)
            and np.array_equal(W.data, WT.data)):
        return W
    n = W.shape[0]
    rows = np.concatenate([np.repeat(np.arange(n), np.diff(W.indptr)), np.repeat(np.arange(n), np.diff(WT.indptr))])
    cols = np.concatenate([W.indices, WT.indices])
    data = np.concatenate([W.data, WT.data])
    order = np.argsort(rows, kind="stable")
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    G = sparse.csr_matrix((n, n), dtype=W.dtype)
    G.indptr, G.indices, G.data = indptr.astype(np.int32), cols[order].astype(np.int32), data[order]
    return G


def sssp_multi_device(G: DeviceCSR, sources: torch.Tensor, *, unweighted: bool = False, want_D: bool = True,
                      want_P: bool = False, want_min: bool = False, out: Optional[torch.Tensor] = None):
    """Device-resident multi-source solve.  `sources` int32 on G's device.  Returns
    (D f32 [S,n] | None, P i32 [S,n] | None, dmin f32 [n] | None, argmin i32 [n] | None, sweeps).
    `out`: a contiguous f32 [S,n] block (e.g. rows of a resident all-pairs matrix) to receive D."""
    lib = _lib.load()
    dev = G.indptr.device
    S, n = int(sources.numel()), G.n
    if out is not None:
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (S, n) and out.device == dev
    D = out if out is not None else (torch.empty((S, n), dtype=torch.float32, device=dev) if want_D else None)
    P = torch.empty((S, n), dtype=torch.int32, device=dev) if want_P else None
    dmin = torch.empty(n, dtype=torch.float32, device=dev) if want_min else None
    amin = torch.empty(n, dtype=torch.int32, device=dev) if want_min else None
    ws = workspace(lib.geo_sssp_workspace_bytes(n, G.nnz, S), dev)
    sweeps = np.zeros(1, dtype=np.int32)
    weights = None if unweighted else G.data
    with torch.cuda.device(dev):
        _lib.check(lib.geo_sssp_multi(ptr(G.indptr), ptr(G.indices), ptr(weights), n, G.nnz, ptr(sources), S,
                                      ptr(D), ptr(P), ptr(dmin), ptr(amin), ptr(ws), ws.numel(),
                                      sweeps.ctypes.data, stream_ptr()), "geo_sssp_multi")
    return D, P, dmin, amin, int(sweeps[0])


def nearest_source_device(G: DeviceCSR, sources: torch.Tensor, *, unweighted: bool = False, info: Optional[dict] = None):
    """(dmin f32 [n], argmin i32 [n], sweeps): D.min(axis=0) / D.argmin(axis=0) of dijkstra_multi_source's FLOAT32 matrix
    (geo_shortest_paths.py:50, kmeans_optimized.py:100: the lowest row whose distance rounds to the column minimum) from ONE
    label-carrying solve (csrc/sssp.hip, geo_sssp_nearest_source) -- K times less work than the matrix.  G must be symmetric.
    When the call declines (weights outside the exact units, too many float32 collisions) the K-source solve answers instead.
    `info`, if given, receives declined / reason / suspects / sweeps of the one-solve attempt."""
    lib = _lib.load()
    dev = G.indptr.device
    S, n = int(sources.numel()), G.n
    dmin = torch.empty(n, dtype=torch.float32, device=dev)
    amin = torch.empty(n, dtype=torch.int32, device=dev)
    ws = workspace(lib.geo_sssp_nearest_workspace_bytes(n, G.nnz), dev)
    status = np.zeros(4, dtype=np.int32)
    weights = None if unweighted else G.data
    with torch.cuda.device(dev):
        _lib.check(lib.geo_sssp_nearest_source(ptr(G.indptr), ptr(G.indices), ptr(weights), n, G.nnz, ptr(sources), S,
                                               ptr(dmin), ptr(amin), ptr(ws), ws.numel(), status.ctypes.data, stream_ptr()),
                   "geo_sssp_nearest_source")
    if info is not None:
        info.update(declined=bool(status[0]), reason=int(status[3]), suspects=int(status[2]), sweeps=int(status[1]))
    if status[0] == 0:
        return dmin, amin, int(status[1])
    _, _, dmin, amin, sweeps = sssp_multi_device(G, sources, unweighted=unweighted, want_D=False, want_min=True)
    return dmin, amin, sweeps


def _normalise_sources(sources, n: int) -> np.ndarray:
    src = np.asarray(sources, dtype=int).copy()
    src[src < 0] += n
    if src.size and (src.min() < 0 or src.max() >= n):
        raise ValueError(f"indices out of range 0...{n}")
    return src


def dijkstra_multi_source(W: sparse.spmatrix, sources, directed: bool = False, unweighted: bool = False,
                          return_predecessors: bool = False, dtype=np.float32) -> Tuple:
    """Multi-source geodesic distances: D[i, v] = dist(sources[i], v) (geo_shortest_paths.py:24-50)."""
    if len(sources) == 0:
        raise ValueError("sources must be a non-empty sequence of node indices")
    W = ensure_valid_graph(W)
    n = W.shape[0]
    src = _normalise_sources(sources, n)
    if n == 0:
        raise ValueError("graph has no nodes")
    dev = device()
    G = DeviceCSR.from_scipy(_pull_structure(W, directed), dev, with_data=not unweighted)
    src_t = torch.from_numpy(src.astype(np.int32)).to(dev)
    D, P, _, _, _ = sssp_multi_device(G, src_t, unweighted=unweighted, want_D=True, want_P=return_predecessors)
    D_host = D.cpu().numpy().astype(dtype, copy=False)
    if return_predecessors:
        return D_host, P.cpu().numpy().astype(np.int32, copy=False)
    return D_host


def dijkstra_single_source(W: sparse.spmatrix, source: int, directed: bool = False, unweighted: bool = False,
                           return_predecessors: bool = False, dtype=np.float32) -> Tuple:
    """Single-source wrapper returning 1-D arrays (geo_shortest_paths.py:53-63)."""
    out = dijkstra_multi_source(W, [int(source)], directed=directed, unweighted=unweighted,
                                return_predecessors=return_predecessors, dtype=dtype)
    if return_predecessors:
        return out[0][0], out[1][0]
    return out[0]


def distances_between(W: sparse.spmatrix, sources, targets, directed: bool = False, unweighted: bool = False,
                      dtype=np.float32) -> np.ndarray:
    """Compact (S x T) distance matrix (geo_shortest_paths.py:66-76)."""
    if len(sources) == 0 or len(targets) == 0:
        raise ValueError("sources and targets must be non-empty.")
    sources = np.asarray(sources, dtype=int)
    targets = np.asarray(targets, dtype=int)
    D = dijkstra_multi_source(W, sources, directed=directed, unweighted=unweighted,
                              return_predecessors=False, dtype=dtype)
    return D[:, targets]


# ------------------------------------------------------------------------------------- geodesic paths
@dataclass
class GeodesicPaths:
    """M paths, device-resident, as csrc/paths.hip leaves them: pair m owns the slice [offsets[m], offsets[m + 1]) of `nodes`
    (source -> target) and `cum` (the running fp64 length, the solver's accumulation order); the slice is empty unless
    status[m] == 0.  status: 0 source reached, 1 target unreachable, 2 malformed predecessors (hops = -1 for both)."""
    nodes: torch.Tensor        # i32 [T]
    offsets: torch.Tensor      # i64 [M + 1]
    cum: torch.Tensor          # f64 [T]
    hops: torch.Tensor         # i32 [M]
    status: torch.Tensor       # i32 [M]

    def __len__(self) -> int:
        return int(self.hops.numel())

    def path(self, m: int):
        """(nodes np.int32, cum np.float64) of pair m on the host; empty arrays unless status[m] == 0."""
        lo, hi = (int(x) for x in self.offsets[m:m + 2].tolist())
        return self.nodes[lo:hi].cpu().numpy(), self.cum[lo:hi].cpu().numpy()

    def to_lists(self):
        """(list of M np.int32 node arrays, list of M np.float64 cum arrays): one copy of each array to the host."""
        nodes, cum, off = self.nodes.cpu().numpy(), self.cum.cpu().numpy(), self.offsets.cpu().numpy()
        return ([nodes[off[m]:off[m + 1]] for m in range(len(self))], [cum[off[m]:off[m + 1]] for m in range(len(self))])


def _i32(x, dev) -> torch.Tensor:
    return torch.as_tensor(x, device=dev).to(torch.int32).contiguous().view(-1)


def paths_from_predecessors_device(G: DeviceCSR, P: torch.Tensor, sources: torch.Tensor, rows: torch.Tensor,
                                   targets: torch.Tensor, *, unweighted: bool = False,
                                   max_hops: Optional[int] = None) -> GeodesicPaths:
    """The paths the predecessor rows `P` (i32 [S, n], sssp_multi_device(want_P=True) on `G`; a view with a row stride >= n
    is taken as it is) hold for the M pairs (rows[m], targets[m]): row rows[m] of P was solved from sources[rows[m]].
    count -> cumsum -> fill on the current stream; one synchronisation (the total number of path nodes sizes the outputs)."""
    lib = _lib.load()
    dev = G.indptr.device
    n = G.n
    if P.dtype != torch.int32 or P.dim() != 2 or P.shape[1] != n or P.stride(1) != 1 or (P.shape[0] > 1 and P.stride(0) < n):
        raise ValueError(f"P must be int32 [S, {n}] with unit column stride and a row stride >= n, got {P.dtype} "
                         f"{tuple(P.shape)} strides {tuple(P.stride())}")
    S, ld = int(P.shape[0]), int(P.stride(0)) if P.shape[0] > 1 else n
    sources, rows, targets = _i32(sources, dev), _i32(rows, dev), _i32(targets, dev)
    M = int(rows.numel())
    if int(sources.numel()) != S or int(targets.numel()) != M:
        raise ValueError(f"{int(sources.numel())} sources for {S} rows of P, {int(targets.numel())} targets for {M} rows")
    max_hops = n - 1 if max_hops is None else int(max_hops)
    if not 0 <= max_hops <= n - 1:
        raise ValueError(f"max_hops = {max_hops} outside [0, n - 1 = {n - 1}]")
    hops = torch.empty(M, dtype=torch.int32, device=dev)
    status = torch.empty(M, dtype=torch.int32, device=dev)
    offsets = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    if M == 0:
        return GeodesicPaths(torch.empty(0, dtype=torch.int32, device=dev), offsets,
                             torch.empty(0, dtype=torch.float64, device=dev), hops, status)
    weights = None if unweighted else G.data
    with torch.cuda.device(dev):
        _lib.check(lib.geo_sssp_paths_count(ptr(P), ld, S, ptr(sources), ptr(rows), ptr(targets), M, n, max_hops, ptr(hops),
                                            ptr(status), stream_ptr()), "geo_sssp_paths_count")
        torch.cumsum((hops + 1).to(torch.int64), 0, out=offsets[1:])          # hops = -1 wherever status != 0: no slot
        T = int(offsets[-1].item())
        nodes = torch.empty(T, dtype=torch.int32, device=dev)
        cum = torch.empty(T, dtype=torch.float64, device=dev)
        _lib.check(lib.geo_sssp_paths_fill(ptr(P), ld, S, ptr(sources), ptr(rows), ptr(targets), M, n, ptr(G.indptr),
                                           ptr_or_stand_in(G.indices), ptr(weights), ptr(offsets), T, ptr_or_stand_in(nodes),
                                           ptr_or_stand_in(cum), stream_ptr()), "geo_sssp_paths_fill")
    return GeodesicPaths(nodes, offsets, cum, hops, status)


def geodesic_paths_device(G: DeviceCSR, src_nodes, dst_nodes, *, unweighted: bool = False,
                          max_block_bytes: int = 4 << 30) -> Tuple[GeodesicPaths, torch.Tensor]:
    """Geodesics between the M node pairs (src_nodes[m], dst_nodes[m]) of G: (GeodesicPaths, dist f32 [M]) in the caller's
    pair order, dist[m] = D[row of src][dst] of sssp_multi_device.  The pairs are grouped by unique source; the sources are
    solved in blocks whose D and P rows (8 n bytes per source) fit `max_block_bytes` -- at least one source per block."""
    dev = G.indptr.device
    n = G.n
    src, dst = _i32(src_nodes, dev), _i32(dst_nodes, dev)
    M = int(src.numel())
    if int(dst.numel()) != M:
        raise ValueError(f"{M} sources for {int(dst.numel())} targets")
    if M and (int(torch.minimum(src.min(), dst.min())) < 0 or int(torch.maximum(src.max(), dst.max())) >= n):
        raise ValueError(f"indices out of range 0...{n}")
    dist = torch.empty(M, dtype=torch.float32, device=dev)
    hops = torch.empty(M, dtype=torch.int32, device=dev)
    status = torch.empty(M, dtype=torch.int32, device=dev)
    offsets = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    if M == 0:
        return GeodesicPaths(torch.empty(0, dtype=torch.int32, device=dev), offsets,
                             torch.empty(0, dtype=torch.float64, device=dev), hops, status), dist
    uniq, row_of = torch.unique(src, return_inverse=True)                     # sorted sources; row_of[m] = its row
    per_block = max(1, int(max_block_bytes) // (8 * n))
    order = torch.argsort(row_of, stable=True)                                # pairs by source row, the caller's order within
    row_sorted = row_of[order]
    parts = []
    for s0 in range(0, int(uniq.numel()), per_block):
        s1 = min(int(uniq.numel()), s0 + per_block)
        sel = order[(row_sorted >= s0) & (row_sorted < s1)]
        D, P, _, _, _ = sssp_multi_device(G, uniq[s0:s1].contiguous(), unweighted=unweighted, want_D=True, want_P=True)
        rows = (row_of[sel] - s0).to(torch.int32)
        part = paths_from_predecessors_device(G, P, uniq[s0:s1], rows, dst[sel], unweighted=unweighted)
        dist[sel] = D[rows.long(), dst[sel].long()]
        hops[sel], status[sel] = part.hops, part.status
        parts.append((sel, part))
    torch.cumsum((hops + 1).to(torch.int64), 0, out=offsets[1:])
    T = int(offsets[-1].item())
    nodes = torch.empty(T, dtype=torch.int32, device=dev)
    cum = torch.empty(T, dtype=torch.float64, device=dev)
    for sel, part in parts:                                                   # each block's slices to their place in pair order
        length = part.offsets[1:] - part.offsets[:-1]
        if int(part.nodes.numel()) == 0:
            continue
        pair = torch.repeat_interleave(torch.arange(sel.numel(), device=dev), length)
        at = offsets[sel][pair] + (torch.arange(part.nodes.numel(), device=dev) - part.offsets[:-1][pair])
        nodes[at], cum[at] = part.nodes, part.cum
    return GeodesicPaths(nodes, offsets, cum, hops, status), dist


def _check_frames(n_frames: int) -> int:
    if int(n_frames) < 2:
        raise ValueError(f"n_frames = {n_frames}: a curve needs its two ends (n_frames >= 2)")
    return int(n_frames)


def _resample(z: torch.Tensor, nodes, offsets, cum, M: int, F: int) -> torch.Tensor:
    lib = _lib.load()
    if z.dtype != torch.float32 or z.dim() != 2 or not z.is_contiguous():
        raise ValueError(f"z must be a contiguous float32 [n, d] tensor, got {z.dtype} {tuple(z.shape)}")
    frames = torch.full((M, F, z.shape[1]), float("nan"), dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        _lib.check(lib.geo_polyline_resample(ptr(z), z.shape[0], z.shape[1], ptr_or_stand_in(nodes), ptr(offsets),
                                             ptr_or_stand_in(cum), M, F, ptr_or_stand_in(frames), stream_ptr()),
                   "geo_polyline_resample")
    return frames


def resample_paths_device(z: torch.Tensor, paths: GeodesicPaths, n_frames: int) -> torch.Tensor:
    """n_frames points at equal arc length along each path's polyline through the latents z f32 [n, d]: f32 [M, F, d], the
    first the source's latent and the last the target's, bit for bit.  NaN for a pair without a path (status != 0)."""
    F = _check_frames(n_frames)
    return _resample(z, paths.nodes, paths.offsets, paths.cum, len(paths), F)


def chord_frames_device(z: torch.Tensor, src_nodes, dst_nodes, n_frames: int) -> torch.Tensor:
    """n_frames equally spaced points on the straight line from z[src_nodes[m]] to z[dst_nodes[m]]: f32 [M, F, d], through the
    kernel of resample_paths_device as the two-node polyline nodes = [a, b], cum = [0, 1]."""
    F = _check_frames(n_frames)
    src, dst = _i32(src_nodes, z.device), _i32(dst_nodes, z.device)
    M = int(src.numel())
    if int(dst.numel()) != M:
        raise ValueError(f"{M} sources for {int(dst.numel())} targets")
    if M and (int(torch.minimum(src.min(), dst.min())) < 0 or int(torch.maximum(src.max(), dst.max())) >= z.shape[0]):
        raise ValueError(f"indices out of range 0...{z.shape[0]}")
    nodes = torch.stack([src, dst], dim=1).contiguous().view(-1)
    offsets = torch.arange(M + 1, dtype=torch.int64, device=z.device) * 2
    cum = torch.tensor([0.0, 1.0], dtype=torch.float64, device=z.device).repeat(M)
    return _resample(z, nodes, offsets, cum, M, F)


def geodesic_paths(W: sparse.spmatrix, sources, targets, directed: bool = False, unweighted: bool = False):
    """Geodesics between the pairs (sources[m], targets[m]) of W: (list of np.int32 node arrays source -> target, np.float32
    distances).  Validation, index normalisation and exception classes of dijkstra_multi_source.  An unreachable pair gives
    an empty array and inf.  Raises ValueError when the solve's predecessors do not lead back to a source: on a graph with
    zero-weight edges (or weights below one ulp of the distances) two nodes at the same distance can name each other."""
    if len(sources) == 0 or len(targets) == 0:
        raise ValueError("sources and targets must be non-empty.")
    if len(sources) != len(targets):
        raise ValueError(f"{len(sources)} sources for {len(targets)} targets: one target per source")
    W = ensure_valid_graph(W)
    n = W.shape[0]
    src, dst = _normalise_sources(sources, n), _normalise_sources(targets, n)
    if n == 0:
        raise ValueError("graph has no nodes")
    dev = device()
    G = DeviceCSR.from_scipy(_pull_structure(W, directed), dev, with_data=not unweighted)
    paths, dist = geodesic_paths_device(G, src.astype(np.int32), dst.astype(np.int32), unweighted=unweighted)
    status = paths.status.cpu().numpy()
    bad = np.flatnonzero(status == 2)
    if bad.size:
        m = int(bad[0])
        raise ValueError(f"pair {m} ({int(src[m])} -> {int(dst[m])}): the predecessors of the solve do not lead back to the "
                         f"source ({bad.size} such pair(s)).  With zero-weight edges, or weights below one ulp of the "
                         "distances, two nodes at equal distance can name each other as predecessor; drop or merge such "
                         "edges (build_codebook does)")
    return paths.to_lists()[0], dist.cpu().numpy().astype(np.float32, copy=False)


def all_pairs_geodesic_device(G: DeviceCSR, block: int = 512, max_bytes: int = 200 << 30) -> torch.Tensor:
    """All-pairs geodesic distances as a resident f32 [n, n] matrix (row s = scipy Dijkstra from s rounded to f32, the
    rows geo_sssp_multi returns), filled `block` sources at a time.  Extension: the reference never
    forms the full matrix; 288 GB of HBM hold it up to n = 230 000 (14.4 GB at the 60 000-latent configuration)."""
    n = G.n
    if n * n * 4 > max_bytes:
        raise ValueError(f"all-pairs matrix of {n} nodes needs {n * n * 4 / 2**30:.1f} GiB (limit {max_bytes / 2**30:.0f} GiB)")
    dev = G.indptr.device
    D = torch.empty((n, n), dtype=torch.float32, device=dev)
    for s0 in range(0, n, block):
        s1 = min(n, s0 + block)
        sssp_multi_device(G, torch.arange(s0, s1, dtype=torch.int32, device=dev), out=D[s0:s1])
    return D

