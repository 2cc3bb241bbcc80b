"""Latents or codes -> images on the MI355X: the native decode of both VAE decoders.

  - decode_logits: the decoder's raw output, f32 [n, C, S, S] on the device.  A vanilla decoder (vqvae_amd.vae.Decoder) takes
    vector latents z (n, d), or table (K, d) and codes (n,): row i decodes table[codes[i]] straight from the table, no gathered
    copy.  A spatial decoder (SpatialDecoder) takes latent grids z (n, d, 4, 4), or table (K, d) and codes (n, 4, 4): position
    (y, x) of image i is table[codes[i, y, x]], which is how build_codebook's codes quantize a grid.  Decoders with fixed
    statistics that `native_decode_covers` accepts run in geo_vanilla_decode / geo_spatial_decode (csrc/vanilla_jvp.hip); any
    other module (GroupNorm, train-mode BatchNorm, other widths) is decoded with the module itself, in eval() under no_grad.
    last_decode_path() says which ran.  A row's logits depend on nothing but its latent: not on the batch, the workspace, the
    stream, nor on whether the latent came directly or through the codes.
  - decode_images: decode_logits, then the reference's post-processing (eval.reconstruction.unnormalize_images) as float32
    torch ops: for the same logits the pixels are the reference's.

Passing a module composes its export on every call; a caller that decodes repeatedly builds `VanillaDecoderExport` /
`SpatialImageDecoderExport` once and passes that.  The evaluation CLIs and the training loops do not use this path yet.
"""
from typing import Optional

import torch
import torch.nn as nn

from . import _lib
from ._device import device, ptr, stream_ptr
from ._export import capped_workspace, eval_mode
from .spatial_decoder import SpatialImageDecoderExport, looks_like_spatial_decoder, spatial_image_kernels_cover
from .vanilla_decoder import VanillaDecoderExport, looks_like_vanilla_decoder, vanilla_kernels_cover

_last_decode_path = None
_TORCH_BATCH = 512


def last_decode_path() -> Optional[str]:
    """"hip" or "torch": the route the last decode_logits / decode_images call took."""
    return _last_decode_path


def native_decode_covers(decoder: nn.Module) -> bool:
    """Whether decode_logits runs this module in the HIP kernels: vanilla_decoder.vanilla_kernels_cover for the vanilla
    layout, spatial_decoder.spatial_image_kernels_cover for the spatial one, False for anything else."""
    if looks_like_vanilla_decoder(decoder):
        return vanilla_kernels_cover(decoder)
    if looks_like_spatial_decoder(decoder):
        return spatial_image_kernels_cover(decoder)
    return False


def _check_inputs(spatial: bool, d: Optional[int], z, table, codes):
    """Checks shapes and code ranges; returns n.  Exactly one of z and (table, codes)."""
    if (z is None) == (table is None and codes is None) or (table is None) != (codes is None):
        raise ValueError("give either z or (table, codes)")
    if z is not None:
        want = "(n, d, 4, 4)" if spatial else "(n, d)"
        ok = (z.dim() == 4 and tuple(z.shape[2:]) == (4, 4)) if spatial else z.dim() == 2
        if not ok or (d is not None and z.shape[1] != d):
            raise ValueError(f"latents must be {want} with d = {d}, got {tuple(z.shape)}")
        return int(z.shape[0])
    if table.dim() != 2 or (d is not None and table.shape[1] != d):
        raise ValueError(f"table must be (K, d) with d = {d}, got {tuple(table.shape)}")
    if codes.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError(f"codes must be integers, got {codes.dtype}")
    ok = (codes.dim() == 3 and tuple(codes.shape[1:]) == (4, 4)) if spatial else codes.dim() == 1
    if not ok:
        raise ValueError(f"codes must be {'(n, 4, 4)' if spatial else '(n,)'}, got {tuple(codes.shape)}")
    K = int(table.shape[0])
    if codes.numel():
        lo, hi = torch.aminmax(codes)
        if int(lo) < 0 or int(hi) >= K:
            raise ValueError(f"code {int(hi) if int(hi) >= K else int(lo)} is outside the table's {K} rows")
    return int(codes.shape[0])


def _native(export, spatial: bool, z, table, codes, n: int, max_workspace_bytes) -> torch.Tensor:
    lib = _lib.load()
    dev = export.tensors["w2p"].device
    C, S = int(export.desc.out_channels), int(export.desc.out_size)
    out = torch.empty(n, C, S, S, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    if n >= 2 ** 31:
        raise ValueError(f"{n} rows: the decode takes fewer than 2^31")

    def f32(t):
        return None if t is None else t.detach().to(dev, torch.float32).contiguous()

    z, table = f32(z), f32(table)
    codes = None if codes is None else codes.to(dev, torch.int32).contiguous()
    query = lib.geo_spatial_decode_workspace_bytes if spatial else lib.geo_vanilla_decode_workspace_bytes
    with torch.cuda.device(dev):
        ws = capped_workspace(query(export.desc, n), max_workspace_bytes, dev, "decode: decoder")
        if spatial:
            _lib.check(lib.geo_spatial_decode(export.desc, ptr(z), ptr(table), ptr(codes), n, ptr(out), ptr(ws), ws.numel(),
                                              stream_ptr()), "geo_spatial_decode")
        else:
            _lib.check(lib.geo_vanilla_decode(export.desc, ptr(z if table is None else table), ptr(codes), n, ptr(out), ptr(ws),
                                              ws.numel(), stream_ptr()), "geo_vanilla_decode")
    return out


@torch.no_grad()
def _torch_route(decoder: nn.Module, spatial: bool, z, table, codes, n: int) -> torch.Tensor:
    """The module itself in eval() (its layers' own modes are put back afterwards), in batches of 512; codes become the
    quantized latents first, grids as contiguous NCHW tensors (a convolution library may sum a channels-last view of the same
    values in another order)."""
    dev = next(decoder.parameters()).device
    with eval_mode(decoder):
        out = []
        for i in range(0, n, _TORCH_BATCH):
            if z is not None:
                zi = z[i:i + _TORCH_BATCH].to(dev, torch.float32)
            else:
                zi = table.to(dev, torch.float32)[codes[i:i + _TORCH_BATCH].to(dev).long()]
                if spatial:
                    zi = zi.permute(0, 3, 1, 2).contiguous()
            out.append(decoder(zi).float())
        if not out:
            probe = z[:0] if z is not None else table.new_zeros((0, table.shape[1]) + ((4, 4) if spatial else ()))
            out.append(decoder(probe.to(dev, torch.float32)).float())
        return torch.cat(out)


def decode_logits(decoder_or_export, z: Optional[torch.Tensor] = None, *, table: Optional[torch.Tensor] = None,
                  codes: Optional[torch.Tensor] = None, max_workspace_bytes: Optional[int] = None) -> torch.Tensor:
    """The decoder's raw output f32 [n, C, S, S] on the device for z, or for table[codes] (module docstring).  Codes are
    checked against the table (ValueError).  The kernels run on the caller's current stream with the cached workspace;
    `max_workspace_bytes` caps it (not below *_decode_workspace_bytes(desc, 1)) and changes no value."""
    global _last_decode_path
    obj = decoder_or_export
    if isinstance(obj, (VanillaDecoderExport, SpatialImageDecoderExport)):
        export, spatial = obj, isinstance(obj, SpatialImageDecoderExport)
        n = _check_inputs(spatial, export.latent_dim, z, table, codes)
    else:
        spatial = looks_like_spatial_decoder(obj)
        d = obj.conv_in.in_channels if spatial else (obj.fc.in_features if looks_like_vanilla_decoder(obj) else None)
        if not spatial and d is None and z is not None and z.dim() == 4:
            spatial = True                                       # an unknown module fed latent grids
        n = _check_inputs(spatial, d, z, table, codes)
        if not native_decode_covers(obj):
            _last_decode_path = "torch"
            return _torch_route(obj, spatial, z, table, codes, n)
        own = next(obj.parameters()).device
        dev = own if own.type == "cuda" else device()
        export = (SpatialImageDecoderExport if spatial else VanillaDecoderExport)(obj, dev)
    out = _native(export, spatial, z, table, codes, n, max_workspace_bytes)
    _last_decode_path = "hip"
    return out


def decode_images(decoder_or_export, z: Optional[torch.Tensor] = None, *, table: Optional[torch.Tensor] = None,
                  codes: Optional[torch.Tensor] = None, dataset: str, apply_sigmoid: bool,
                  max_workspace_bytes: Optional[int] = None) -> torch.Tensor:
    """decode_logits, then eval.reconstruction.unnormalize_images(logits, dataset, apply_sigmoid): images in [0, 1], f32
    [n, C, S, S] on the device."""
    from .eval.reconstruction import unnormalize_images
    logits = decode_logits(decoder_or_export, z, table=table, codes=codes, max_workspace_bytes=max_workspace_bytes)
    return unnormalize_images(logits, dataset, apply_sigmoid)
