"""Host-side description of the encoders the image-encode kernels of csrc/encode.hip run:
vqvae_amd.vae.Encoder and vqvae_amd.spatial_vae.SpatialEncoder (reference src/models/vae.py:22-50, spatial_vae.py:22-44) with
FIXED statistics -- eval-mode BatchNorm with running statistics, or no normalisation.

    conv_layers: [Conv2d(k3, s2, p1) -> norm -> ReLU] x 3,  28 -> 14 -> 7 -> 4 px | 32 -> 16 -> 8 -> 4 px
    vanilla head: fc_mu, fc_logvar = Linear(16 e3, d) on the NCHW flatten;   spatial head: Conv2d(e3, d, 1)

`ImageEncoderExport` folds each norm and its convolution's bias into one scale and one shift per channel in fp64, lays the
weights out as the kernels read them (the vanilla head permuted from the module's channel-major flatten to the activations'
pixel-major order), rounds once to f32 and holds the `geo_image_encoder_desc` of include/geo_hip.h over those tensors."""
from typing import Optional

import torch
import torch.nn as nn

from . import _lib
from ._export import _fixed_statistics, _fold, conv_taps, f64, fill_desc, pack_k_quads

COVERED_ENC_WIDTHS = ((64, 128, 256), (32, 64, 128))          # enc_channels the kernels are compiled for
COVERED_INPUTS = {1: 28, 3: 32}                               # in_channels -> image size
MAX_VANILLA_LATENT_DIM = 128
MAX_SPATIAL_LATENT_DIM = 64


def _stack(m: nn.Module):
    """((conv, norm) x 3) of an encoder's `conv_layers`, or None when the layout is another one."""
    seq = getattr(m, "conv_layers", None)
    if not isinstance(seq, nn.Sequential) or len(seq) != 9:
        return None
    stages = []
    for i in (0, 3, 6):
        conv, norm, act = seq[i], seq[i + 1], seq[i + 2]
        if not isinstance(conv, nn.Conv2d) or not isinstance(act, nn.ReLU):
            return None
        if (conv.kernel_size != (3, 3) or conv.stride != (2, 2) or conv.padding != (1, 1) or conv.dilation != (1, 1)
                or conv.groups != 1 or conv.padding_mode != "zeros"):
            return None
        stages.append((conv, norm))
    if stages[0][0].out_channels != stages[1][0].in_channels or stages[1][0].out_channels != stages[2][0].in_channels:
        return None
    kinds = {type(norm) for _, norm in stages}
    if len(kinds) != 1 or not kinds <= {nn.BatchNorm2d, nn.GroupNorm, nn.Identity}:
        return None
    return stages


def looks_like_vanilla_encoder(m: nn.Module) -> bool:
    """True for vqvae_amd.vae.Encoder and any module with the reference Encoder's layout (duck typing on `conv_layers`,
    `fc_mu`, `fc_logvar`): three Conv2d k3 s2 p1, each followed by one norm layer (BatchNorm2d, GroupNorm or Identity, the same
    kind three times) and a ReLU, then two Linear heads of equal shape on the flattened 4 x 4 grid."""
    stages, mu, lv = _stack(m), getattr(m, "fc_mu", None), getattr(m, "fc_logvar", None)
    if stages is None or not isinstance(mu, nn.Linear) or not isinstance(lv, nn.Linear):
        return False
    return mu.in_features == lv.in_features == 16 * stages[2][0].out_channels and mu.out_features == lv.out_features


def looks_like_spatial_encoder(m: nn.Module) -> bool:
    """True for vqvae_amd.spatial_vae.SpatialEncoder and any module with the reference SpatialEncoder's layout: the same
    convolution stack, then two 1 x 1 Conv2d heads of equal shape."""
    stages, mu, lv = _stack(m), getattr(m, "fc_mu", None), getattr(m, "fc_logvar", None)
    if stages is None or not isinstance(mu, nn.Conv2d) or not isinstance(lv, nn.Conv2d):
        return False
    for head in (mu, lv):
        if (head.kernel_size != (1, 1) or head.stride != (1, 1) or head.padding != (0, 0) or head.dilation != (1, 1)
                or head.groups != 1 or head.in_channels != stages[2][0].out_channels):
            return False
    return mu.out_channels == lv.out_channels


def encoder_kernels_cover(m: nn.Module, in_size: Optional[int] = None) -> bool:
    """Whether geo_image_encode (csrc/encode.hip) runs this module on images of `in_size` px (None: the size that goes with its
    channel count; else vqvae_amd.encode runs the module itself).  Exactly: looks_like_vanilla_encoder(m) or
    looks_like_spatial_encoder(m), and
      - the three norm layers are nn.Identity, or nn.BatchNorm2d in eval mode with running statistics (affine or not);
      - the three convolutions and both heads have a bias;
      - enc_channels is (64, 128, 256) or (32, 64, 128);
      - 1 input channel with 28 px, or 3 input channels with 32 px;
      - 1 <= latent_dim <= 128 (vanilla head) or <= 64 (spatial head).
    Anything else -- GroupNorm, train-mode BatchNorm, BatchNorm without running statistics, a layer without bias, other widths,
    another pairing of channels and size -- is not covered."""
    vanilla = looks_like_vanilla_encoder(m)
    if not vanilla and not looks_like_spatial_encoder(m):
        return False
    stages = _stack(m)
    if not all(_fixed_statistics(norm) for _, norm in stages):
        return False
    if any(layer.bias is None for layer in [conv for conv, _ in stages] + [m.fc_mu, m.fc_logvar]):
        return False
    C = stages[0][0].in_channels
    if C not in COVERED_INPUTS or (in_size is not None and int(in_size) != COVERED_INPUTS[C]):
        return False
    if tuple(conv.out_channels for conv, _ in stages) not in COVERED_ENC_WIDTHS:
        return False
    d = m.fc_mu.out_features if vanilla else m.fc_mu.out_channels
    return 1 <= d <= (MAX_VANILLA_LATENT_DIM if vanilla else MAX_SPATIAL_LATENT_DIM)


class ImageEncoderExport:
    """A covered encoder as geo_image_encode reads it: f32 tensors on `dev` plus the ctypes descriptor over them.  `host` keeps
    the same arrays in fp64, before the one rounding: "w1p" [9 C][e1], "w2p" [9][e1 / 4][e2][4], "w3p" [9][e2 / 4][e3][4],
    "scale_i", "shift_i" (the convolution's bias inside the shift), "whp" [segments][e3 / 4][npad][4] and "bh" [npad] with
    npad = 2 d rounded up to 32, columns mu then logvar (geo_hip.h has the element formulas).  `spatial` says which head,
    `in_channels` / `in_size` which images.  A snapshot: later changes of the module (weights, statistics, mode) are not seen."""

    def __init__(self, enc: nn.Module, dev: torch.device):
        if not encoder_kernels_cover(enc):
            raise ValueError("encoder not covered by the image-encode kernels (see encoder_kernels_cover)")
        stages = _stack(enc)
        self.spatial = looks_like_spatial_encoder(enc)
        (conv1, _), (conv2, _), (conv3, _) = stages
        C, e1, e2, e3 = conv1.in_channels, conv1.out_channels, conv2.out_channels, conv3.out_channels
        d = enc.fc_mu.out_channels if self.spatial else enc.fc_mu.out_features
        npad = (2 * d + 31) // 32 * 32
        host = {}
        with torch.no_grad():
            for tag, (conv, norm) in zip("123", stages):
                scale, shift = _fold(norm, conv.out_channels)
                host["scale" + tag], host["shift" + tag] = scale, shift + scale * f64(conv.bias)
            host["w1p"] = f64(conv1.weight).permute(1, 2, 3, 0).reshape(9 * C, e1)
            host["w2p"], host["w3p"] = conv_taps(f64(conv2.weight)), conv_taps(f64(conv3.weight))
            wh = torch.cat([f64(enc.fc_mu.weight).reshape(d, -1), f64(enc.fc_logvar.weight).reshape(d, -1)])    # [2 d][K]
            nseg = 1 if self.spatial else 16
            wh = wh.view(2 * d, e3, nseg).permute(2, 1, 0)                 # [segment = pixel][channel][column]
            whp = torch.zeros(nseg, e3, npad, dtype=torch.float64)
            whp[:, :, :2 * d] = wh
            host["whp"] = pack_k_quads(whp)
            bh = torch.zeros(npad, dtype=torch.float64)
            bh[:2 * d] = torch.cat([f64(enc.fc_mu.bias), f64(enc.fc_logvar.bias)])
            host["bh"] = bh
        self.host = {k: v.contiguous() for k, v in host.items()}
        self.tensors = {k: v.to(torch.float32).to(dev) for k, v in self.host.items()}
        self.latent_dim, self.in_channels, self.in_size = d, C, COVERED_INPUTS[C]
        desc = _lib.ImageEncoderDesc()
        desc.in_channels, desc.in_size, desc.e1, desc.e2, desc.e3 = C, self.in_size, e1, e2, e3
        desc.latent_dim, desc.spatial_head = d, int(self.spatial)
        self.desc = fill_desc(desc, self.tensors)
