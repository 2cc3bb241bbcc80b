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
from dataclasses import dataclass

import numpy as np
import torch

from .. import _lib
from .._device import device, ptr, stream_ptr, workspace
from .._export import _fixed_statistics, capped_workspace
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


def vanilla_vjp_device(export_or_decoder, z: torch.Tensor, u: torch.Tensor, *, index=None, max_workspace_bytes=None) -> torch.Tensor:
    """out[i] = J(z_i)^T u_i in fp64 for a covered vanilla decoder (vanilla_kernels_cover) or its VanillaDecoderExport, with
    g = sigmoid(decoder(.)) flattened to [C S S] and J = dg/dz: z f32 [., d] on a GPU, u f32 [n, C S S] (any trailing shape of
    that many values), `index` None or int32 [n] choosing row i's latent z[index[i]].  Native only (geo_vanilla_vjp): an
    uncovered decoder raises ValueError.  `max_workspace_bytes` caps the workspace (not below
    geo_vanilla_vjp_min_workspace_bytes) and changes no bit."""
    lib = _lib.load()
    dev = z.device
    export = export_or_decoder if isinstance(export_or_decoder, VanillaDecoderExport) else VanillaDecoderExport(export_or_decoder, dev)
    n = int(z.shape[0] if index is None else index.numel())
    if z.ndim != 2 or z.shape[1] != export.latent_dim:
        raise ValueError(f"z must be [., {export.latent_dim}], got {tuple(z.shape)}")
    if u.shape[0] != n or u.numel() != n * export.n_out:
        raise ValueError(f"u must hold {n} rows of {export.n_out} values, got {tuple(u.shape)}")
    if index is not None:
        if index.dtype != torch.int32:
            raise ValueError("index must be int32")
        if n and not (0 <= int(index.min()) and int(index.max()) < z.shape[0]):
            raise ValueError("index out of range")
        index = index.to(dev).contiguous()
    z = z.detach().to(torch.float32).contiguous()
    u = u.detach().to(dev, torch.float32).contiguous()
    out = torch.empty(n, export.latent_dim, dtype=torch.float64, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        ws = capped_workspace(lib.geo_vanilla_vjp_workspace_bytes(export.desc, n), max_workspace_bytes, dev,
                              "geo_vanilla_vjp_workspace_bytes: decoder")
        _lib.check(lib.geo_vanilla_vjp(export.desc, ptr(z), ptr(index), n, ptr(u), ptr(out), ptr(ws), ws.numel(), stream_ptr()),
                   "geo_vanilla_vjp")
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


# ---------------------------------------------------------------------------------------------- the metric tensor itself
# G(z) = J(z)^T J(z) per latent, its eigenvalues, the volume element sqrt(det G) (as logvol = 0.5 log det G) and the numerical
# rank.  Covered decoders run geo_decoder_metric_tensor (csrc/jvp.hip: the column pass of the per-latent
# Jacobian route, jacobian_gram_kernel, metric_spectrum_kernel); every other decoder, and the CPU, takes the generic route:
# torch.func.jacfwd of sigmoid(decoder(.)) in float32, the Gram matrix and torch.linalg.eigvalsh in fp64.  Both routes apply
# the same rank and logvol rules.  Float32 columns determine G's entries and its large eigenvalues; where G is nearly singular
# (16 outputs from 16 latent dimensions: cond(G) up to 1e9) they do not determine the smallest eigenvalues or logvol.
_GENERIC_BATCH = 256            # latents per jacfwd call on the generic route
_GRAM_LOOP_MAX_OUTPUTS = 256    # up to this many outputs the generic Gram is accumulated output by output, ascending


@dataclass
class PullbackMetric:
    """G fp64 [n, d, d] (or [N, H, W, d, d] for a latent grid); eig fp64 [..., d] ascending, logvol fp64 [...] = 0.5 log det G
    (-inf unless every eigenvalue is > 0), rank int32 [...] -- None with spectrum=False; route "native" or "autograd"; J the
    columns themselves, f32 [..., d, nout] (J[k] = d sigmoid(decoder(z)) / dz_k, flattened), only with jacobian=True."""
    G: object
    eig: object
    logvol: object
    rank: object
    route: str
    J: object = None


def native_metric_covers(decoder) -> bool:
    """Whether geo_decoder_metric_tensor computes this decoder's metric tensor (else: the generic autograd route).  Exactly:
    looks_like_spatial_decoder(decoder) and hip_kernels_cover(decoder), and
      - fixed statistics: both norm layers nn.Identity, or nn.BatchNorm2d in eval mode with running statistics, or
        nn.GroupNorm (32 groups per layer);
      - latent_dim <= 16;
      - dec_channels[1] in {32, 64, 128} and dec_channels[2] == 64, any dec_channels[0];
      - 16, 32 or 192 outputs on the decoder's 1x1 latent: (out_channels, size) = (1, 28), (2, 28) or (3, 32).
    Not covered: train-mode BatchNorm (a sample's Jacobian depends on its batch; pullback_metric* raise ValueError for it on
    either route), latent_dim > 16, other widths or output sizes, the vanilla decoder and any other module."""
    if not (isinstance(decoder, torch.nn.Module) and looks_like_spatial_decoder(decoder) and hip_kernels_cover(decoder)):
        return False
    seq = decoder.deconv_layers
    fixed = all(isinstance(l, torch.nn.GroupNorm) or _fixed_statistics(l) for l in (seq[1], seq[4]))
    s_out = 8 if seq[6].padding[0] == 1 else 4
    tiles = (seq[6].out_channels * s_out * s_out + 31) // 32
    return (fixed and decoder.conv_in.in_channels <= 16 and seq[0].out_channels in (32, 64, 128) and seq[3].out_channels == 64
            and tiles in (1, 6))


def native_vanilla_metric_covers(decoder) -> bool:
    """Whether geo_vanilla_metric_tensor computes this decoder's metric tensor: exactly
    vanilla_kernels_cover(decoder) -- the vanilla decoder with eval-mode BatchNorm or no norm, 1 <= latent_dim <= 128,
    dec_channels[1:] (128, 64) or (64, 32), 1 or 3 channels of 28 or 32 px.  native_metric_covers stays False for it."""
    return vanilla_kernels_cover(decoder)


def _has_train_batchnorm(decoder) -> bool:
    return any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and (m.training or m.running_mean is None)
               for m in decoder.modules())


def metric_spectrum_fields(G: torch.Tensor, eig: torch.Tensor, p_out: int):
    """(logvol, rank) of ascending eigenvalues `eig` [n, d] of G [n, d, d], by the rules of metric_spectrum_kernel:
    rank = #{i: sqrt(eig_i) > max(p_out, d) * FLT_EPSILON * sqrt(eig_max)}; logvol = 0.5 * sum log eig_i if all > 0, else -inf."""
    d = eig.shape[-1]
    pos = eig.clamp_min(0.0)
    tol = float(max(p_out, d)) * float(torch.finfo(torch.float32).eps) * pos[:, -1:].sqrt()
    rank = ((eig > 0) & (pos.sqrt() > tol)).sum(1).to(torch.int32)
    all_pos = (eig > 0).all(1)
    logs = torch.log(torch.where(eig > 0, eig, torch.ones_like(eig)))
    logvol = torch.zeros(eig.shape[0], dtype=torch.float64, device=eig.device)
    for i in range(d):                                   # ascending, like the kernel
        logvol = logvol + logs[:, i]
    logvol = torch.where(all_pos, 0.5 * logvol, torch.full_like(logvol, float("-inf")))
    return logvol, rank


def _generic_metric(decoder, z: torch.Tensor, spectrum: bool, jacobian: bool = False):
    """The generic route on the decoder's own device: (G, eig, logvol, rank, J) for z [n, d]; J f32 [n, d, p_out] is jacfwd's,
    transposed, with `jacobian`, else None."""
    dec_dev = next(decoder.parameters()).device
    first = next(decoder.children())
    flat_input = hasattr(first, "in_features")

    def image(latent):                                   # one latent [d] -> its image, flattened
        x = latent.view(1, -1) if flat_input else latent.view(1, -1, 1, 1)
        return torch.sigmoid(decoder(x)).reshape(-1)

    z = z.detach().to(dec_dev, torch.float32)
    n, d = z.shape
    G = torch.empty(n, d, d, dtype=torch.float64, device=dec_dev)
    p_out = 0
    cols = []
    for lo in range(0, n, _GENERIC_BATCH):
        with torch.no_grad():
            J = torch.func.vmap(torch.func.jacfwd(image))(z[lo:lo + _GENERIC_BATCH])               # [b, p_out, d]
        if jacobian:
            cols.append(J.transpose(1, 2).contiguous())
        J = J.double()
        p_out = J.shape[1]
        if p_out <= _GRAM_LOOP_MAX_OUTPUTS:
            g = torch.zeros(J.shape[0], d, d, dtype=torch.float64, device=dec_dev)
            for o in range(p_out):
                g += J[:, o, :, None] * J[:, o, None, :]
        else:                                            # (many outputs: one matrix product, the upper triangle mirrored)
            g = torch.bmm(J.transpose(1, 2), J)
            g = torch.triu(g) + torch.triu(g, 1).transpose(1, 2)
        G[lo:lo + _GENERIC_BATCH] = g
    Jt = None
    if jacobian:
        Jt = torch.cat(cols) if cols else torch.empty(0, d, 0, dtype=torch.float32, device=dec_dev)
    if not spectrum:
        return G, None, None, None, Jt
    eig = torch.linalg.eigvalsh(G) if n else torch.empty(0, d, dtype=torch.float64, device=dec_dev)
    logvol, rank = metric_spectrum_fields(G, eig, p_out)
    return G, eig, logvol, rank, Jt


def _native_metric(export: DecoderExport, z: torch.Tensor, spectrum: bool, max_workspace_bytes):
    lib = _lib.load()
    dev = z.device
    n, d = z.shape
    G = torch.empty(n, d, d, dtype=torch.float64, device=dev)
    eig = torch.empty(n, d, dtype=torch.float64, device=dev) if spectrum else None
    logvol = torch.empty(n, dtype=torch.float64, device=dev) if spectrum else None
    rank = torch.empty(n, dtype=torch.int32, device=dev) if spectrum else None
    if n == 0:
        return G, eig, logvol, rank
    with torch.cuda.device(dev):
        ws = capped_workspace(lib.geo_metric_tensor_workspace_bytes(export.desc, n), max_workspace_bytes, dev,
                              "geo_metric_tensor_workspace_bytes: decoder")
        _lib.check(lib.geo_decoder_metric_tensor(export.desc, ptr(z), n, ptr(G), ptr(eig), ptr(logvol), ptr(rank), ptr(ws),
                                                 ws.numel(), stream_ptr()), "geo_decoder_metric_tensor")
    return G, eig, logvol, rank, None


def _native_vanilla_metric(export: VanillaDecoderExport, z: torch.Tensor, spectrum: bool, jacobian: bool, max_workspace_bytes):
    lib = _lib.load()
    dev = z.device
    n, d = z.shape
    G = torch.empty(n, d, d, dtype=torch.float64, device=dev)
    J = torch.empty(n, d, export.n_out, dtype=torch.float32, device=dev) if jacobian else None
    eig = torch.empty(n, d, dtype=torch.float64, device=dev) if spectrum else None
    logvol = torch.empty(n, dtype=torch.float64, device=dev) if spectrum else None
    rank = torch.empty(n, dtype=torch.int32, device=dev) if spectrum else None
    if n == 0:
        return G, eig, logvol, rank, J
    with torch.cuda.device(dev):
        ws = capped_workspace(lib.geo_vanilla_metric_workspace_bytes(export.desc, n), max_workspace_bytes, dev,
                              "geo_vanilla_metric_workspace_bytes: decoder")
        _lib.check(lib.geo_vanilla_metric_tensor(export.desc, ptr(z), None, n, ptr(G), ptr(J), ptr(eig), ptr(logvol), ptr(rank),
                                                 ptr(ws), ws.numel(), stream_ptr()), "geo_vanilla_metric_tensor")
    return G, eig, logvol, rank, J


def sym_spectrum_device(G: torch.Tensor, p_out: int):
    """(eig f64 [n, d] ascending, logvol f64 [n], rank int32 [n]) of symmetric matrices G, a CUDA fp64 tensor [n, d, d] with
    1 <= d <= 128, by geo_sym_spectrum (csrc/sym_spectrum.hip): only the upper triangles are read; the rank and logvol rules of
    metric_spectrum_fields with `p_out` outputs.  A matrix with a NaN or an inf gives eig NaN, logvol NaN, rank 0."""
    if G.ndim != 3 or G.shape[1] != G.shape[2] or G.dtype != torch.float64 or G.device.type != "cuda":
        raise ValueError(f"G must be a CUDA float64 tensor [n, d, d], got {G.dtype} {tuple(G.shape)} on {G.device}")
    lib = _lib.load()
    G = G.contiguous()
    n, d = int(G.shape[0]), int(G.shape[1])
    eig = torch.empty(n, d, dtype=torch.float64, device=G.device)
    logvol = torch.empty(n, dtype=torch.float64, device=G.device)
    rank = torch.empty(n, dtype=torch.int32, device=G.device)
    with torch.cuda.device(G.device):
        _lib.check(lib.geo_sym_spectrum(ptr(G), n, d, int(p_out), ptr(eig), ptr(logvol), ptr(rank), stream_ptr()),
                   "geo_sym_spectrum")
    return eig, logvol, rank


def pullback_metric_device(decoder_or_export, z: torch.Tensor, *, spectrum: bool = True, max_workspace_bytes=None,
                           jacobian: bool = False) -> PullbackMetric:
    """The pull-back metric tensor G = J^T J of every latent, J = d sigmoid(decoder(z)) / dz on a 1x1 latent, with (spectrum)
    its eigenvalues, logvol = 0.5 log det G and numerical rank.  z: [n, d], or a latent grid [N, d, H, W], which is flattened
    in build_codebook's (n, h, w) row order and gives fields shaped [N, H, W, ...].  The tensors live on z's device.
    A decoder with native_metric_covers and z on a GPU run geo_decoder_metric_tensor (a DecoderExport always does;
    `max_workspace_bytes` caps its workspace, not below geo_metric_tensor_min_workspace_bytes, and changes no bit); anything
    else takes the generic autograd route on the decoder's device.  Train-mode BatchNorm raises ValueError on both routes: a
    sample's Jacobian there depends on the batch it is in.
    A vanilla decoder with native_vanilla_metric_covers and z [n, d] on a GPU run geo_vanilla_metric_tensor (a
    VanillaDecoderExport always does), d up to 128; its workspace is capped the same way.  `jacobian`: the result also carries
    the columns J f32 [n, d, nout] (the spatial decoder's native route has none to give: ValueError for a DecoderExport and for a
    module that would take that route)."""
    grid = None
    if z.ndim == 4:
        N, d, H, W = z.shape
        grid = (N, H, W)
        z = z.permute(0, 2, 3, 1).reshape(-1, d)
    if z.ndim != 2:
        raise ValueError(f"z must be [n, d] or [N, d, H, W], got {tuple(z.shape)}")
    out_dev = z.device
    if isinstance(decoder_or_export, VanillaDecoderExport):
        if z.shape[1] != decoder_or_export.latent_dim:
            raise ValueError(f"z has {z.shape[1]} latent dimensions, the decoder {decoder_or_export.latent_dim}")
        fields = _native_vanilla_metric(decoder_or_export, z.detach().to(torch.float32).contiguous(), spectrum, jacobian,
                                        max_workspace_bytes)
        route = "native"
    elif isinstance(decoder_or_export, DecoderExport):
        if jacobian:
            raise ValueError("jacobian=True: geo_decoder_metric_tensor does not return its columns")
        if decoder_or_export.desc.norm == 1 and decoder_or_export.desc.bn_train:
            raise ValueError("pull-back metric tensor of a train-mode BatchNorm decoder: a sample's Jacobian depends on its "
                             "batch; put the decoder in eval()")
        fields = _native_metric(decoder_or_export, z.detach().to(torch.float32).contiguous(), spectrum, max_workspace_bytes)
        route = "native"
    else:
        decoder = decoder_or_export
        if _has_train_batchnorm(decoder):
            raise ValueError("pull-back metric tensor of a train-mode BatchNorm decoder: a sample's Jacobian depends on its "
                             "batch; put the decoder in eval()")
        if native_vanilla_metric_covers(decoder) and out_dev.type == "cuda" and grid is None:
            export = VanillaDecoderExport(decoder, out_dev)
            if z.shape[1] != export.latent_dim:
                raise ValueError(f"z has {z.shape[1]} latent dimensions, the decoder {export.latent_dim}")
            fields = _native_vanilla_metric(export, z.detach().to(torch.float32).contiguous(), spectrum, jacobian,
                                            max_workspace_bytes)
            route = "native"
        elif native_metric_covers(decoder) and out_dev.type == "cuda":
            if jacobian:
                raise ValueError("jacobian=True: geo_decoder_metric_tensor does not return its columns")
            if z.shape[1] != decoder.conv_in.in_channels:
                raise ValueError(f"z has {z.shape[1]} latent dimensions, the decoder {decoder.conv_in.in_channels}")
            fields = _native_metric(DecoderExport(decoder, out_dev), z.detach().to(torch.float32).contiguous(), spectrum,
                                    max_workspace_bytes)
            route = "native"
        else:
            fields = tuple(None if t is None else t.to(out_dev) for t in _generic_metric(decoder, z, spectrum, jacobian))
            route = "autograd"
    if grid is not None:
        fields = tuple(None if t is None else t.reshape(*grid, *t.shape[1:]) for t in fields)
    return PullbackMetric(*fields[:4], route=route, J=fields[4])


def pullback_metric(decoder, z, *, jacobian: bool = False) -> PullbackMetric:
    """pullback_metric_device on host arrays: z a numpy array ([n, d] or [N, d, H, W]), the fields numpy arrays.  A covered decoder
    runs natively (on its own GPU, or on this process's when it lives on the CPU and there is one); any other on its own device."""
    dec_dev = next(decoder.parameters()).device
    dev = dec_dev
    covered = native_metric_covers(decoder) or (native_vanilla_metric_covers(decoder) and np.ndim(z) == 2)
    if covered and dec_dev.type != "cuda" and torch.cuda.is_available():
        dev = device()
    res = pullback_metric_device(decoder, torch.as_tensor(z, dtype=torch.float32).to(dev), jacobian=jacobian)
    return PullbackMetric(*(None if t is None else t.cpu().numpy() for t in (res.G, res.eig, res.logvol, res.rank)),
                          route=res.route, J=None if res.J is None else res.J.cpu().numpy())
