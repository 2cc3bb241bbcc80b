"""Interpolation along geodesics of a pull-back weighted latent graph, next to the straight line (an extension: the reference's
demos stop at colouring nodes by geodesic distance).

geodesic_interpolation: node pairs -> the geodesic's polyline resampled at equal arc length (csrc/paths.hip), the chord, and
the pull-back length of both curves (edge_lengths_riemannian over consecutive frames).
interpolate_images_spatial: image pairs of the spatial pipeline -> 16 node pairs each, one per grid position, assembled into
latent grids, decoded (decode_images), with the image-space length of both routes (geo_image_pair_moments).
interpolate_images_vanilla: the same for a vanilla pipeline's vector latents, one node pair per image pair.
relax_iters > 0 (both): the geodesic's frames and the chord are each relaxed under the decoder's metric with the ends fixed
(relax_curves_device) and the result with the lower energy is kept per pair: never worse than either start.
interpolate_images_spatial(relax_metric="image") relaxes the two sequences of whole 4x4 grids under the whole decoder instead
(relax_grid_curves_device): the energy is the image sequence's own.
"""
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from .._device import DeviceCSR
from .geo_shortest_paths import _check_frames, chord_frames_device, geodesic_paths_device, resample_paths_device
from .grid_relaxation import relax_grid_curves_device
from .relaxation import relax_curves_device
from .riemannian_metric import edge_lengths_riemannian


def curve_lengths(decoder, frames: torch.Tensor, batch_size: int = 512) -> torch.Tensor:
    """Pull-back length of M polylines frames f32 [M, F, d]: f32 [M], the sum over the F - 1 segments, in segment order, of
    edge_lengths_riemannian(decoder, frames[:, f], frames[:, f + 1])."""
    total = torch.zeros(frames.shape[0], dtype=torch.float32, device=frames.device)
    for f in range(frames.shape[1] - 1):
        seg = edge_lengths_riemannian(decoder, frames[:, f].contiguous(), frames[:, f + 1].contiguous(), batch_size)
        total = total + seg.to(frames.device)
    return total


def relax_best(decoder, frames_geo: torch.Tensor, frames_lin: torch.Tensor, relax_iters: int,
               relax=relax_curves_device) -> Dict[str, torch.Tensor]:
    """Relax both starts of M curves [M, F, d] for relax_iters iterations and keep, per curve, the result with the lower final
    energy (a tie goes to the geodesic).  Returns frames_relaxed f32 [M, F, d]; relax_from i32 [M] (0 the chord, 1 the
    geodesic); energy_geo, energy_lin f64 [M] (of the starts), energy_relaxed f64 [M] (<= both); accepted_geo, accepted_lin
    i32 [M].  relax=relax_grid_curves_device: the same over curves of grids [M, F, d, 4, 4]."""
    geo = relax(decoder, frames_geo, relax_iters)
    lin = relax(decoder, frames_lin, relax_iters)
    from_geo = geo.energy <= lin.energy
    return {"frames_relaxed": torch.where(from_geo.view(-1, *([1] * (frames_geo.dim() - 1))), geo.frames, lin.frames),
            "relax_from": from_geo.to(torch.int32), "energy_geo": geo.energy0, "energy_lin": lin.energy0,
            "energy_relaxed": torch.where(from_geo, geo.energy, lin.energy), "accepted_geo": geo.accepted,
            "accepted_lin": lin.accepted}


def geodesic_interpolation(z: torch.Tensor, G: DeviceCSR, decoder, src_nodes, dst_nodes, n_frames: int, *,
                           batch_size: int = 512, relax_iters: int = 0) -> Dict[str, torch.Tensor]:
    """Curves between the M node pairs of the graph G over the latents z f32 [n, d] (device).  Returns frames_geo, frames_lin
    f32 [M, F, d]; graph_dist f32 [M] (the solver's distance); hops, status i32 [M] (GeodesicPaths); curve_len_geo,
    curve_len_lin f32 [M] (curve_lengths).  A pair without a path (status != 0) gets the chord as frames_geo.  Call with the
    decoder in eval mode: a train-mode BatchNorm would move its statistics and make a segment depend on its batch.
    relax_iters > 0 adds relax_best's fields and curve_len_relaxed f32 [M]; with 0 the result is what it always was."""
    F = _check_frames(n_frames)
    paths, dist = geodesic_paths_device(G, src_nodes, dst_nodes)
    frames_lin = chord_frames_device(z, src_nodes, dst_nodes, F)
    frames_geo = resample_paths_device(z, paths, F)
    frames_geo = torch.where((paths.status != 0).view(-1, 1, 1), frames_lin, frames_geo)
    out = {"frames_geo": frames_geo, "frames_lin": frames_lin, "graph_dist": dist, "hops": paths.hops, "status": paths.status,
           "curve_len_geo": curve_lengths(decoder, frames_geo, batch_size),
           "curve_len_lin": curve_lengths(decoder, frames_lin, batch_size)}
    if relax_iters > 0:
        out.update(relax_best(decoder, frames_geo, frames_lin, int(relax_iters)))
        out["curve_len_relaxed"] = curve_lengths(decoder, out["frames_relaxed"], batch_size)
    return out


def image_curve_lengths(images: torch.Tensor) -> torch.Tensor:
    """images f32 [M, F, C, S, S] -> f64 [M]: the sum over f, in order, of sqrt(squared error) between frames f and f + 1, the
    squared error being geo_image_pair_moments' sixth moment."""
    from ..eval.metrics import image_pair_moments
    M, F = images.shape[:2]
    flat = images.reshape(M, F, -1)
    total = torch.zeros(M, dtype=torch.float64, device=images.device)
    for f in range(F - 1):
        total = total + torch.sqrt(image_pair_moments(flat[:, f].contiguous(), flat[:, f + 1].contiguous())[:, 5])
    return total


def _row_pair_curves(flat: torch.Tensor, lcc_index: np.ndarray, G: DeviceCSR, a: np.ndarray, b: np.ndarray, F: int):
    """Curves between rows a[i] and b[i] of flat f32 [n, d] (device), of which the rows lcc_index (ascending) are the nodes of G:
    (frames_geo, frames_lin f32 [P, F, d], graph_dist f32 [P], hops, status i32 [P]).  A pair with an end outside the graph
    (graph_dist NaN, hops -1, status 3) or without a path takes the chord as frames_geo."""
    dev = G.indptr.device
    P = a.shape[0]
    node_of = np.full(flat.shape[0], -1, dtype=np.int64)
    node_of[lcc_index] = np.arange(lcc_index.size)
    frames_lin = chord_frames_device(flat, a, b, F)                           # over all pairs: a chord needs no graph
    in_graph = (node_of[a] >= 0) & (node_of[b] >= 0)
    sel = np.flatnonzero(in_graph)
    frames_geo = frames_lin.clone()
    graph_dist = torch.full((P,), float("nan"), dtype=torch.float32, device=dev)
    hops = torch.full((P,), -1, dtype=torch.int32, device=dev)
    status = torch.full((P,), 3, dtype=torch.int32, device=dev)
    if sel.size:
        sel_t = torch.from_numpy(sel).to(dev)
        z_lcc = flat[torch.from_numpy(lcc_index).to(dev)].contiguous()
        paths, dist = geodesic_paths_device(G, node_of[a[sel]], node_of[b[sel]])
        geo = resample_paths_device(z_lcc, paths, F)
        frames_geo[sel_t] = torch.where((paths.status != 0).view(-1, 1, 1), frames_lin[sel_t], geo)
        graph_dist[sel_t], hops[sel_t], status[sel_t] = dist, paths.hops, paths.status
    return frames_geo, frames_lin, graph_dist, hops, status


def _check_pairs(image_pairs, lcc_index, n_images: int, n_rows: int, G: DeviceCSR):
    """(pairs i64 [M, 2], lcc_index i64) checked as both image interpolations document them."""
    pairs = np.asarray(image_pairs, dtype=np.int64).reshape(-1, 2)
    if pairs.shape[0] == 0:
        raise ValueError("image_pairs must be a non-empty sequence of (i, j)")
    if pairs.min() < 0 or pairs.max() >= n_images:
        raise ValueError(f"image indices out of range 0...{n_images}")
    lcc_index = np.asarray(lcc_index, dtype=np.int64).reshape(-1)
    if lcc_index.size != G.n or (lcc_index.size and (lcc_index.min() < 0 or lcc_index.max() >= n_rows
                                                      or (np.diff(lcc_index) <= 0).any())):
        raise ValueError(f"lcc_index must list the {G.n} nodes of the graph as ascending flat positions below {n_rows}")
    return pairs, lcc_index


def interpolate_images_vanilla(z: torch.Tensor, lcc_index, G: DeviceCSR, decoder, image_pairs: Sequence[Tuple[int, int]],
                               n_frames: int, dataset: str, apply_sigmoid: bool, *, batch_size: int = 512,
                               relax_iters: int = 0) -> Dict:
    """Image pairs of a vanilla (vector-latent) pipeline: z f32 [N, d], one latent and so one node pair per image pair.
    lcc_index: the rows of z that are nodes of G, ascending -- np.flatnonzero(codes >= 0) of a build_riemannian_codebook_legacy
    output.  The fields of interpolate_images_spatial without the position axis: frames_geo, frames_lin f32 [M, F, d];
    images_geo, images_lin f32 [M, F, C, S, S] (decode_images); graph_dist f32 [M] (NaN outside the graph, inf without a path),
    hops, status i32 [M] (-1 and 3 outside the graph); curve_len_*, f32 [M]; image_len_* f64 [M]; fallback_positions per pair
    ([0] where the pair took the chord, else empty).  relax_iters > 0 adds frames_relaxed, images_relaxed, image_len_relaxed,
    curve_len_relaxed, relax_from, accepted_geo, accepted_lin i32 [M], energy_geo, energy_lin, energy_relaxed f64 [M]
    (relax_best: natively for a decoder native_vanilla_relax_covers admits)."""
    from ..decode import decode_images
    F = _check_frames(n_frames)
    dev = G.indptr.device
    if z.dim() != 2:
        raise ValueError(f"z must be [N, d], got {tuple(z.shape)}")
    N, d = z.shape
    pairs, lcc_index = _check_pairs(image_pairs, lcc_index, N, N, G)
    M = pairs.shape[0]
    flat = z.to(dev, torch.float32).contiguous()
    frames_geo, frames_lin, graph_dist, hops, status = _row_pair_curves(flat, lcc_index, G, pairs[:, 0], pairs[:, 1], F)
    st = status.cpu().numpy()
    out = {"graph_dist": graph_dist, "hops": hops, "status": status,
           "fallback_positions": [np.flatnonzero(st[m:m + 1] != 0).astype(np.int32) for m in range(M)]}
    routes = [("geo", frames_geo), ("lin", frames_lin)]
    if relax_iters > 0:
        best = relax_best(decoder, frames_geo, frames_lin, int(relax_iters))
        routes.append(("relaxed", best.pop("frames_relaxed")))
        out.update(best)
    for name, fr in routes:
        out[f"frames_{name}"] = fr
        out[f"curve_len_{name}"] = curve_lengths(decoder, fr, batch_size)
        images = decode_images(decoder, fr.reshape(M * F, d), dataset=dataset, apply_sigmoid=apply_sigmoid)
        out[f"images_{name}"] = images.view(M, F, *images.shape[1:])
        out[f"image_len_{name}"] = image_curve_lengths(out[f"images_{name}"])
    return out


def interpolate_images_spatial(z_grids: torch.Tensor, lcc_index, G: DeviceCSR, decoder, image_pairs: Sequence[Tuple[int, int]],
                               n_frames: int, dataset: str, apply_sigmoid: bool, *, batch_size: int = 512,
                               relax_iters: int = 0, relax_metric: str = "position") -> Dict:
    """Image pairs of the spatial pipeline.  z_grids f32 [N, d, 4, 4] (any h x w grid); lcc_index: the flat positions
    img * h * w + y * w + x that are nodes of G, ascending -- np.flatnonzero(codes.reshape(-1) >= 0) of a build_codebook
    output: a position's node is its rank in that list.  Pair (i, j) is h * w node pairs, position p of image i to position p
    of image j; a position with an end outside the graph, or without a path, takes the chord and is listed in
    fallback_positions (per pair, the sorted positions p).  Returns frames_geo, frames_lin f32 [M, F, d, h, w]; images_geo,
    images_lin f32 [M, F, C, S, S] (decode_images of those grids); graph_dist f32 [M, h w] (NaN outside the graph, inf
    without a path), hops, status i32 [M, h w] (-1 and 3 for a position outside the graph); curve_len_geo, curve_len_lin f32
    [M] (pull-back lengths summed over the positions in position order); image_len_geo, image_len_lin f64 [M].
    relax_iters > 0 relaxes every position's two curves (relax_best) and adds frames_relaxed, images_relaxed, image_len_relaxed
    and curve_len_relaxed like the other two routes', and relax_from, accepted_geo, accepted_lin i32 [M, h w], energy_geo,
    energy_lin, energy_relaxed f64 [M, h w]; with 0 the result is what it always was.
    relax_metric="image" (needs h = w = 4; the default "position" is the above) relaxes, per pair, the two sequences of whole
    grids frames_geo and frames_lin under the whole decoder instead (relax_grid_curves_device): the energy is the image
    sequence's own and sees the overlap of neighbouring positions.  The relaxed fields are then per pair: frames_relaxed
    [M, F, d, 4, 4], images_relaxed, image_len_relaxed, curve_len_relaxed as before; energy_geo, energy_lin, energy_relaxed
    f64 [M]; accepted_geo, accepted_lin, relax_from i32 [M]."""
    from ..decode import decode_images
    F = _check_frames(n_frames)
    dev = G.indptr.device
    N, d, h, w = z_grids.shape
    hw = h * w
    if relax_metric not in ("position", "image"):
        raise ValueError(f"relax_metric must be 'position' or 'image', got {relax_metric!r}")
    by_image = relax_metric == "image" and relax_iters > 0
    if by_image and (h, w) != (4, 4):
        raise ValueError(f"relax_metric='image' relaxes 4x4 grids, the latents are {h}x{w}")
    pairs, lcc_index = _check_pairs(image_pairs, lcc_index, N, N * hw, G)
    M = pairs.shape[0]
    flat = z_grids.to(dev, torch.float32).permute(0, 2, 3, 1).reshape(N * hw, d).contiguous()
    pos = np.arange(hw)
    a = (pairs[:, :1] * hw + pos).reshape(-1)                                # flat positions of the M hw node pairs
    b = (pairs[:, 1:] * hw + pos).reshape(-1)
    frames_geo, frames_lin, graph_dist, hops, status = _row_pair_curves(flat, lcc_index, G, a, b, F)
    st = status.view(M, hw).cpu().numpy()
    out = {"frames_geo": None, "frames_lin": None, "graph_dist": graph_dist.view(M, hw), "hops": hops.view(M, hw),
           "status": status.view(M, hw), "fallback_positions": [np.flatnonzero(st[m] != 0).astype(np.int32) for m in range(M)]}
    routes = [("geo", frames_geo), ("lin", frames_lin)]

    def as_grids(fr):                                                        # [M hw, F, d] -> [M, F, d, h, w]
        return fr.view(M, h, w, F, d).permute(0, 3, 4, 1, 2).contiguous()

    if by_image:
        best = relax_best(decoder, as_grids(frames_geo), as_grids(frames_lin), int(relax_iters), relax_grid_curves_device)
        routes.append(("relaxed", best.pop("frames_relaxed").permute(0, 3, 4, 1, 2).reshape(M * hw, F, d).contiguous()))
        out.update(best)
    elif relax_iters > 0:
        best = relax_best(decoder, frames_geo, frames_lin, int(relax_iters))
        routes.append(("relaxed", best.pop("frames_relaxed")))
        out.update({k: v.view(M, hw) for k, v in best.items()})
    for name, fr in routes:
        out[f"curve_len_{name}"] = curve_lengths(decoder, fr, batch_size).view(M, hw).sum(dim=1)
        grids = as_grids(fr)
        images = decode_images(decoder, grids.view(M * F, d, h, w), dataset=dataset, apply_sigmoid=apply_sigmoid)
        out[f"frames_{name}"] = grids
        out[f"images_{name}"] = images.view(M, F, *images.shape[1:])
        out[f"image_len_{name}"] = image_curve_lengths(out[f"images_{name}"])
    return out
