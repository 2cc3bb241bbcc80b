"""Images -> (mu, logvar) on the MI355X: the native encode of both VAE encoders, the counterpart of
vqvae_amd.decode.

  - encode_latents: the encoder's two outputs, f32 on the device: (n, d) each for a vanilla encoder (vqvae_amd.vae.Encoder),
    (n, d, 4, 4) each for a spatial one (SpatialEncoder).  `x` is the batch the module would be given, (n, C, S, S), already
    normalised.  Encoders with fixed statistics that `native_encode_covers` accepts, on images of the size that goes with
    their channel count, run in geo_image_encode (csrc/encode.hip); any other module (GroupNorm, train-mode BatchNorm, other
    widths or sizes) encodes with the module itself, in eval() under no_grad, in batches of 512.  last_encode_path() says
    which ran.  The route follows from the module and the images, never from an option.  A row's (mu, logvar) on the native
    route depends on nothing but its image: not on the batch, the workspace, the stream.

Passing a module composes its export on every call; a caller that encodes repeatedly builds `ImageEncoderExport` once and
passes that.  The latent writers (utils/latents.py, utils/spatial_latents.py), the training loops and the evaluation CLIs do
not use this path yet: they run the whole model; scripts/encode_latents.py is the command that does.
"""
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._device import device, ptr, stream_ptr
from ._export import capped_workspace, eval_mode
from .image_encoder import ImageEncoderExport, encoder_kernels_cover

_last_encode_path = None
_TORCH_BATCH = 512


def last_encode_path() -> Optional[str]:
    """"hip" or "torch": the route the last encode_latents call took."""
    return _last_encode_path


def native_encode_covers(encoder: nn.Module, in_size: Optional[int] = None) -> bool:
    """Whether encode_latents runs this module in the HIP kernels (image_encoder.encoder_kernels_cover: the exact list) for
    images of `in_size` px; None: the size that goes with the module's channel count (28 for 1 channel, 32 for 3)."""
    return encoder_kernels_cover(encoder, in_size)


def _native(export: ImageEncoderExport, x: torch.Tensor, max_workspace_bytes) -> Tuple[torch.Tensor, torch.Tensor]:
    lib = _lib.load()
    dev = export.tensors["w1p"].device
    n, d = int(x.shape[0]), export.latent_dim
    shape = (n, d, 4, 4) if export.spatial else (n, d)
    mu = torch.empty(shape, dtype=torch.float32, device=dev)
    logvar = torch.empty(shape, dtype=torch.float32, device=dev)
    if n == 0:
        return mu, logvar
    if n >= 2 ** 31:
        raise ValueError(f"{n} images: the encode takes fewer than 2^31")
    x = x.detach().to(dev, torch.float32).contiguous()
    with torch.cuda.device(dev):
        ws = capped_workspace(lib.geo_image_encode_workspace_bytes(export.desc, n), max_workspace_bytes, dev, "encode: encoder")
        _lib.check(lib.geo_image_encode(export.desc, ptr(x), n, ptr(mu), ptr(logvar), ptr(ws), ws.numel(), stream_ptr()),
                   "geo_image_encode")
    return mu, logvar


@torch.no_grad()
def _torch_route(encoder: nn.Module, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The module itself in eval() (its layers' own modes are put back afterwards), in batches of 512."""
    dev = next(encoder.parameters()).device
    with eval_mode(encoder):
        mus, logvars = [], []
        for i in range(0, int(x.shape[0]), _TORCH_BATCH):
            mu, logvar = encoder(x[i:i + _TORCH_BATCH].to(dev, torch.float32))
            mus.append(mu.float()), logvars.append(logvar.float())
        if not mus:                  # an empty batch: the output shapes from one blank image (the vanilla flatten refuses n = 0)
            mu, logvar = encoder(x.new_zeros((1,) + tuple(x.shape[1:])).to(dev, torch.float32))
            mus.append(mu.float()[:0]), logvars.append(logvar.float()[:0])
        return torch.cat(mus), torch.cat(logvars)


def encode_latents(encoder_or_export, x: torch.Tensor, *, max_workspace_bytes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mu, logvar) of the images x (n, C, S, S) on the device (module docstring).  The kernels run on the caller's current
    stream with the cached workspace; `max_workspace_bytes` caps it (not below geo_image_encode_workspace_bytes(desc, 1)) and
    changes no value."""
    global _last_encode_path
    obj = encoder_or_export
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise ValueError(f"images must be (n, C, S, S), got {tuple(x.shape)}")
    if isinstance(obj, ImageEncoderExport):
        export = obj
        if tuple(x.shape[1:]) != (export.in_channels, export.in_size, export.in_size):
            raise ValueError(f"this export encodes (n, {export.in_channels}, {export.in_size}, {export.in_size}) images, "
                             f"got {tuple(x.shape)}")
    else:
        if not native_encode_covers(obj, int(x.shape[2])) or x.shape[1] != obj.conv_layers[0].in_channels:
            _last_encode_path = "torch"
            return _torch_route(obj, x)
        own = next(obj.parameters()).device
        export = ImageEncoderExport(obj, own if own.type == "cuda" else device())
    out = _native(export, x, max_workspace_bytes)
    _last_encode_path = "hip"
    return out
