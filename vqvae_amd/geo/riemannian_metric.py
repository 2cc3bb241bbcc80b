"""Riemannian (decoder pull-back) edge lengths on the MI355X -- same API as the reference's
src/geo/riemannian_metric.py (decoder_logits_to_img :7, edge_lengths_riemannian :37).

For decoders with the SpatialDecoder layer layout the Jacobian-vector products run in the HIP
kernels of csrc/jvp.hip (forward-mode tangent propagation, MFMA for the dominant ConvT layer),
chunked by `batch_size` exactly like riemannian_metric.py:50-58 so that train-mode BatchNorm sees
the same batches; BatchNorm (train and eval), GroupNorm and no normalisation are all in those kernels.  The vanilla
(vector-latent) VAE decoder with fixed statistics -- eval-mode BatchNorm with running statistics, or no norm: every call site
of the reference -- runs in the kernels of csrc/vanilla_jvp.hip (composed affine front, ReLU masks as bits, ConvT2 on the
float32 matrix cores; vanilla_decoder.vanilla_kernels_cover states the coverage); `batch_size` does not
enter there.  Any other nn.Module (e.g. the Linear test decoder of the reference's tests/test_riemannian_metric.py, a
vanilla decoder with GroupNorm or train-mode BatchNorm, or a SpatialDecoder variant outside spatial_decoder.hip_kernels_cover)
has no kernel: it is differentiated by autograd on the decoder's own device.
"""
import torch

from .. import _lib
from .._device import device, ptr, stream_ptr, workspace
from .._export import capped_workspace
from ..spatial_decoder import DecoderExport, hip_kernels_cover, looks_like_spatial_decoder
from ..vanilla_decoder import VanillaDecoderExport, vanilla_kernels_cover


@torch.no_grad()
def decoder_logits_to_img(logits: torch.Tensor) -> torch.Tensor:
    """Decoder logits -> image space [0,1] (riemannian_metric.py:7-10)."""
    return torch.sigmoid(logits)


def edge_lengths_device(export: DecoderExport, z_start: torch.Tensor, z_end: torch.Tensor,
                        batch_size: int = 512) -> torch.Tensor:
    """HIP path on explicit endpoint arrays (f32, contiguous, on the export's device)."""
    lib = _lib.load()
    dev = z_start.device
    E = z_start.shape[0]
    out = torch.empty(E, dtype=torch.float32, device=dev)
    if E == 0:
        return out
    nbytes = lib.geo_jvp_workspace_bytes(export.desc, E, int(batch_size))
    if nbytes == 0:
        raise _lib.GeoHipError("geo_jvp_workspace_bytes: decoder configuration not supported by the HIP path")
    ws = workspace(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.geo_decoder_jvp_pairs(export.desc, ptr(z_start), ptr(z_end), E, int(batch_size), ptr(out),
                                             ptr(ws), ws.numel(), stream_ptr()), "geo_decoder_jvp_pairs")
    export.commit_running_stats(2 * ((E + int(batch_size) - 1) // int(batch_size)))
    return out


def edge_lengths_graph_device(export: DecoderExport, z: torch.Tensor, src: torch.Tensor, dst: torch.Tensor,
                              batch_size: int = 512, build_edges=None) -> torch.Tensor:
    """HIP path on an edge list over resident latents: len[e] for (src[e], dst[e]) without gathers in HBM.
    `build_edges`: the edge count of the whole graph when (src, dst) is a part of it -- a rank's share, or one slice of several
    in one process (None: the call's own count).  Decoders with fixed statistics pick the per-latent Jacobian route from the
    edges per latent, and the two routes differ in their last bits: told the build's count, every part takes the route the
    whole graph takes, so the lengths do not depend on how the edges are divided."""
    lib = _lib.load()
    dev = z.device
    E = int(src.numel())
    build_edges = E if build_edges is None else int(build_edges)
    if build_edges < E:
        raise ValueError(f"build_edges {build_edges} < {E} edges of the call")
    out = torch.empty(E, dtype=torch.float32, device=dev)
    if E == 0:
        return out
    # (with the per-latent buffers: decoders with fixed statistics run their primal pass once per latent, not per edge end)
    nbytes = lib.geo_jvp_edges_part_workspace_bytes(export.desc, int(z.shape[0]), E, build_edges, int(batch_size))
    if nbytes == 0:
        raise _lib.GeoHipError("geo_jvp_edges_part_workspace_bytes: decoder configuration not supported by the HIP path")
    ws = workspace(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.geo_decoder_jvp_edges_part(export.desc, ptr(z), z.shape[0], ptr(src), ptr(dst), E, build_edges,
                                                  int(batch_size), ptr(out), ptr(ws), ws.numel(), stream_ptr()),
                   "geo_decoder_jvp_edges_part")
    export.commit_running_stats(2 * ((E + int(batch_size) - 1) // int(batch_size)))
    return out


def edge_lengths_vanilla_device(export: VanillaDecoderExport, z_start: torch.Tensor, z_end: torch.Tensor,
                                max_workspace_bytes=None) -> torch.Tensor:
    """Vanilla-decoder HIP path on explicit endpoint arrays (f32, contiguous, on the export's device).  The edges are cut
    into passes that fit the workspace; `max_workspace_bytes` caps it (not below geo_vanilla_jvp_workspace_bytes(desc, 1))
    and changes no length."""
    lib = _lib.load()
    dev = z_start.device
    E = z_start.shape[0]
    assert z_start.shape == z_end.shape and z_start.shape[1] == export.latent_dim, (z_start.shape, z_end.shape)
    out = torch.empty(E, dtype=torch.float32, device=dev)
    if E == 0:
        return out
    with torch.cuda.device(dev):
        ws = capped_workspace(lib.geo_vanilla_jvp_workspace_bytes(export.desc, E), max_workspace_bytes, dev,
                              "geo_vanilla_jvp_workspace_bytes: decoder")
        _lib.check(lib.geo_vanilla_jvp_pairs(export.desc, ptr(z_start), ptr(z_end), E, 0, ptr(out), ptr(ws), ws.numel(),
                                             stream_ptr()), "geo_vanilla_jvp_pairs")
    return out


def edge_lengths_vanilla_graph_device(export: VanillaDecoderExport, z: torch.Tensor, src: torch.Tensor, dst: torch.Tensor,
                                      max_workspace_bytes=None) -> torch.Tensor:
    """Vanilla-decoder HIP path on an edge list (int32 src / dst) over resident latents, no gathered copies: with the
    queried workspace and at least half as many edges as latents the per-point work runs once per latent.  Bit for bit the
    lengths of edge_lengths_vanilla_device on z[src], z[dst]."""
    lib = _lib.load()
    dev = z.device
    E, N = int(src.numel()), int(z.shape[0])
    assert z.shape[1] == export.latent_dim and src.dtype == torch.int32 and dst.dtype == torch.int32 and dst.numel() == E
    out = torch.empty(E, dtype=torch.float32, device=dev)
    if E == 0:
        return out
    lo, hi = torch.aminmax(torch.stack((src, dst)))
    if int(lo) < 0 or int(hi) >= N:
        raise ValueError(f"edge endpoints outside [0, {N})")
    with torch.cuda.device(dev):
        ws = capped_workspace(lib.geo_vanilla_jvp_edges_workspace_bytes(export.desc, N, E), max_workspace_bytes, dev,
                              "geo_vanilla_jvp_edges_workspace_bytes: decoder")
        _lib.check(lib.geo_vanilla_jvp_edges(export.desc, ptr(z), N, ptr(src), ptr(dst), E, 0, ptr(out), ptr(ws), ws.numel(),
                                             stream_ptr()), "geo_vanilla_jvp_edges")
    return out


def _generic_jvp_norms(decoder, z: torch.Tensor, direction: torch.Tensor) -> torch.Tensor:
    """|J(z) v| for a decoder the kernels cannot represent, by autograd on the decoder's own device
    (works for any module, including train-mode BatchNorm with its running-statistic updates).
    Linear-first decoders take 2-D input, conv-first ones a 1x1 latent image (riemannian_metric.py:18-27)."""
    first = next(decoder.children())
    flat_input = hasattr(first, "in_features")

    def image(latent):
        if not flat_input and latent.ndim == 2:
            latent = latent[:, :, None, None]
        return torch.sigmoid(decoder(latent)).flatten(1)

    _, tangent = torch.autograd.functional.jvp(image, (z,), (direction,))
    return torch.linalg.vector_norm(tangent, dim=1)


@torch.no_grad()
def edge_lengths_riemannian(decoder, z_start: torch.Tensor, z_end: torch.Tensor, batch_size: int = 512) -> torch.Tensor:
    """0.5 * (|J(z_i) dz| + |J(z_j) dz|) per edge, float32, on the decoder's device (riemannian_metric.py:37-66)."""
    assert z_start.shape == z_end.shape, "Start and end points must have same shape"
    dec_dev = next(decoder.parameters()).device
    if looks_like_spatial_decoder(decoder) and z_start.ndim == 2 and hip_kernels_cover(decoder):
        dev = dec_dev if dec_dev.type == "cuda" else device()
        export = DecoderExport(decoder, dev)
        zs = z_start.detach().to(dev, torch.float32).contiguous()
        ze = z_end.detach().to(dev, torch.float32).contiguous()
        return edge_lengths_device(export, zs, ze, batch_size).to(dec_dev)
    if z_start.ndim == 2 and vanilla_kernels_cover(decoder):           # fixed statistics: batch_size does not enter
        dev = dec_dev if dec_dev.type == "cuda" else device()
        export = VanillaDecoderExport(decoder, dev)
        zs = z_start.detach().to(dev, torch.float32).contiguous()
        ze = z_end.detach().to(dev, torch.float32).contiguous()
        return edge_lengths_vanilla_device(export, zs, ze).to(dec_dev)
    z_start, z_end = z_start.to(dec_dev), z_end.to(dec_dev)
    delta = z_end - z_start
    pieces = []
    for lo in range(0, z_start.size(0), batch_size):
        sl = slice(lo, min(lo + batch_size, z_start.size(0)))
        pieces.append(0.5 * (_generic_jvp_norms(decoder, z_start[sl], delta[sl])
                             + _generic_jvp_norms(decoder, z_end[sl], delta[sl])))
    if not pieces:
        return torch.empty(0, dtype=torch.float32, device=dec_dev)
    return torch.cat(pieces).to(torch.float32)
