"""Host-side description of the decoder the JVP kernels differentiate, and of the same decoder as the image decode of
csrc/vanilla_jvp.hip runs it (`spatial_image_kernels_cover`, `SpatialImageDecoderExport`).

The function being differentiated is the reference's SpatialDecoder
(src/models/spatial_vae.py:47-81; norm factory :8-19).  Only what the geodesic-codebook path needs
is kept here: a module with the SAME parameter names (so `best.pt` state dicts load and the
reference's own SpatialDecoder instances are accepted by duck typing) and the export of its
weights into the `geo_decoder_desc` of include/geo_hip.h.  Encoder, losses and training are out
of scope.
"""
from typing import Mapping, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._export import _fixed_statistics, _fold, _parity_taps, f32, f64, fill_desc, pack_k_quads
from .vanilla_decoder import COVERED_WIDTHS

MAX_IMAGE_LATENT_DIM = 64

_NORM_CODE = {"none": 0, "batch": 1, "group": 2}


def make_norm(norm_type: Optional[str], channels: int) -> nn.Module:
    """batch -> BatchNorm2d, group -> GroupNorm with the largest divisor of `channels` <= 32, else identity."""
    kind = (norm_type or "none").lower()
    if kind == "batch":
        return nn.BatchNorm2d(channels)
    if kind == "group":
        groups = next(g for g in range(max(1, min(32, channels)), 0, -1) if channels % g == 0)
        return nn.GroupNorm(groups, channels)
    return nn.Identity()


class SpatialDecoder(nn.Module):
    """1x1 conv to channels[0], two stride-2 transposed convs with norm + ReLU, one output transposed conv."""

    LAST_PADDING = {32: 1, 28: 3}

    def __init__(self, out_channels: int, channels: Sequence[int], latent_dim: int, output_image_size: int,
                 norm_type: Optional[str]):
        super().__init__()
        if output_image_size not in self.LAST_PADDING:
            raise ValueError(f"Unsupported output size: {output_image_size}")
        c0, c1, c2 = channels
        self.conv_in = nn.Conv2d(latent_dim, c0, 1)
        self.deconv_layers = nn.Sequential(
            nn.ConvTranspose2d(c0, c1, 4, stride=2, padding=1), make_norm(norm_type, c1), nn.ReLU(inplace=True),
            nn.ConvTranspose2d(c1, c2, 4, stride=2, padding=1), make_norm(norm_type, c2), nn.ReLU(inplace=True),
            nn.ConvTranspose2d(c2, out_channels, 4, stride=2, padding=self.LAST_PADDING[output_image_size]),
        )

    def forward(self, z: torch.Tensor) -> torch.Tensor:
        return self.deconv_layers(self.conv_in(z))


def load_decoder_from_checkpoint(ckpt_path: str, *, in_channels: int, dec_channels: Sequence[int], latent_dim: int,
                                 output_image_size: int, norm_type: str, device) -> SpatialDecoder:
    """Decoder half of a SpatialVAE checkpoint ({'model_state_dict', 'epoch'}, spatial_engine.py:142).
    The module is left in training mode, as src/scripts/build_codebook.py:27-29 leaves it."""
    state = torch.load(ckpt_path, map_location="cpu")["model_state_dict"]
    dec_state = {k[len("decoder."):]: v for k, v in state.items() if k.startswith("decoder.")}
    dec = SpatialDecoder(in_channels, tuple(dec_channels), latent_dim, output_image_size, norm_type)
    dec.load_state_dict(dec_state)
    return dec.to(device)


def looks_like_spatial_decoder(m: nn.Module) -> bool:
    """True for this class and for any module with the reference SpatialDecoder's layer layout."""
    conv_in, seq = getattr(m, "conv_in", None), getattr(m, "deconv_layers", None)
    if not isinstance(conv_in, nn.Conv2d) or not isinstance(seq, nn.Sequential) or len(seq) != 7:
        return False
    if conv_in.kernel_size != (1, 1) or conv_in.stride != (1, 1) or conv_in.padding != (0, 0):
        return False
    if not all(isinstance(seq[i], nn.ConvTranspose2d) for i in (0, 3, 6)):
        return False
    if not all(isinstance(seq[i], nn.ReLU) for i in (2, 5)):
        return False
    for i, pads in ((0, (1,)), (3, (1,)), (6, (1, 3))):
        c = seq[i]
        if (c.kernel_size != (4, 4) or c.stride != (2, 2) or c.padding[0] not in pads or c.padding[0] != c.padding[1]
                or c.output_padding != (0, 0) or c.dilation != (1, 1) or c.groups != 1):
            return False
    kinds = {type(seq[1]), type(seq[4])}
    return len(kinds) == 1 and kinds <= {nn.BatchNorm2d, nn.GroupNorm, nn.Identity}


def hip_kernels_cover(m: nn.Module) -> bool:
    """Whether csrc/jvp.hip implements this SpatialDecoder-shaped module (else the caller differentiates it
    with autograd): dec_channels[1] in {32,64,128}, dec_channels[2] a multiple of 16 dividing 128,
    latent_dim <= 64, LDS budget of the output stage; GroupNorm with 32 groups per layer,
    dec_channels[2] == 64 (the reference's default decoder 256-128-64) and a head of 16, 32 or 192 outputs on the
    1x1 latent -- (out_channels * s_out * s_out + 31) // 32 in {1, 6}, s_out = 4 at 28 px and 8 at 32 px: GroupNorm has
    no VALU ConvT3.  The library's make_route (csrc/jvp.hip) decides the same way: for every module this function
    answers what geo_jvp_plan >= 0 answers (tests/test_jvp_envelope_host.py sweeps both)."""
    seq = m.deconv_layers
    d, c1, c2, co = m.conv_in.in_channels, seq[0].out_channels, seq[3].out_channels, seq[6].out_channels
    s_out = 8 if seq[6].padding[0] == 1 else 4
    if isinstance(seq[1], nn.GroupNorm):
        if seq[1].num_groups != 32 or seq[4].num_groups != 32 or c2 != 64 or c1 % 16 != 0:
            return False
        if (co * s_out * s_out + 31) // 32 not in (1, 6):
            return False
    back_lds = (2 * 8 * 16 * (c2 + 4) + 16 * co * (c2 + 4) + 8 * co * s_out * s_out) * 4
    return (d <= 64 and c1 in (32, 64, 128) and c2 % 16 == 0 and 128 % c2 == 0 and back_lds <= 160 * 1024
            and all(getattr(l, "bias", None) is not None for l in (m.conv_in, seq[0], seq[3], seq[6])))


class DecoderExport:
    """f32 contiguous copies of a decoder's parameters on `dev` plus the ctypes descriptor over them."""

    def __init__(self, dec: nn.Module, dev: torch.device):
        seq = dec.deconv_layers
        norm = seq[1]

        def f(t):
            return None if t is None else t.detach().to(dev, torch.float32).contiguous()

        self.tensors = {
            "w_in": f(dec.conv_in.weight.view(dec.conv_in.out_channels, -1)), "b_in": f(dec.conv_in.bias),
            "w1": f(seq[0].weight), "b1": f(seq[0].bias), "w2": f(seq[3].weight), "b2": f(seq[3].bias),
            "w3": f(seq[6].weight), "b3": f(seq[6].bias),
        }
        for tag, layer in (("1", seq[1]), ("2", seq[4])):
            affine = getattr(layer, "weight", None) is not None
            self.tensors["g" + tag] = f(layer.weight) if affine else None
            self.tensors["be" + tag] = f(layer.bias) if affine else None
            self.tensors["rm" + tag] = f(getattr(layer, "running_mean", None))
            self.tensors["rv" + tag] = f(getattr(layer, "running_var", None))
        for name in ("b_in", "b1", "b2", "b3"):
            if self.tensors[name] is None:
                raise ValueError("decoder convolutions without bias are not supported")
        d = _lib.DecoderDesc()
        d.latent_dim = dec.conv_in.in_channels
        d.c0, d.c1, d.c2 = dec.conv_in.out_channels, seq[0].out_channels, seq[3].out_channels
        d.out_channels = seq[6].out_channels
        d.out_size = {1: 32, 3: 28}[seq[6].padding[0]]
        if isinstance(norm, nn.BatchNorm2d):
            d.norm, d.eps = 1, norm.eps
            # batch statistics are used when the NORM layer is in training mode (torch looks at the layer's own flag, not
            # at its parent's), or when no running statistics are tracked
            d.bn_train = 1 if norm.training or norm.running_mean is None else 0
            if norm.weight is None:
                ones = {t: torch.ones(c, device=dev) for t, c in (("1", d.c1), ("2", d.c2))}
                for t in ("1", "2"):
                    self.tensors["g" + t], self.tensors["be" + t] = ones[t], torch.zeros_like(ones[t])
        elif isinstance(norm, nn.GroupNorm):
            d.norm, d.eps, d.bn_train = 2, norm.eps, 0
            d.groups1, d.groups2 = seq[1].num_groups, seq[4].num_groups
            if norm.weight is None:                      # affine=False
                for t, c in (("1", d.c1), ("2", d.c2)):
                    self.tensors["g" + t] = torch.ones(c, device=dev)
                    self.tensors["be" + t] = torch.zeros(c, device=dev)
        else:
            d.norm, d.eps, d.bn_train = 0, 1e-5, 0
        # train-mode BatchNorm with tracked statistics: the kernels fold every batch into running_mean / running_var
        # as torch does (riemannian_metric.py:57-58 runs the decoder in whatever mode it is in); a cumulative average
        # (momentum=None) is not reproduced
        self._bn_layers = [seq[1], seq[4]] if isinstance(norm, nn.BatchNorm2d) else []
        self.tracks_running = bool(d.bn_train and self._bn_layers and norm.running_mean is not None
                                   and norm.momentum is not None)
        d.update_running = 1 if self.tracks_running else 0
        d.momentum = float(norm.momentum) if self.tracks_running else 0.0
        self.desc = fill_desc(d, self.tensors)

    def commit_running_stats(self, n_calls: int) -> None:
        """After a JVP run over `n_calls` decoder calls (2 per chunk): write the updated statistics back when the export
        holds copies (decoder on another device / dtype) and advance num_batches_tracked."""
        if not self.tracks_running:
            return
        with torch.no_grad():
            for tag, layer in zip(("1", "2"), self._bn_layers):
                for attr, key in (("running_mean", "rm" + tag), ("running_var", "rv" + tag)):
                    buf, mine = getattr(layer, attr), self.tensors[key]
                    if buf.data_ptr() != mine.data_ptr():
                        buf.copy_(mine.to(buf.device, buf.dtype))
                if layer.num_batches_tracked is not None:
                    layer.num_batches_tracked += n_calls


def spatial_image_kernels_cover(m: nn.Module) -> bool:
    """Whether geo_spatial_decode (csrc/vanilla_jvp.hip) decodes whole 4x4 latent grids of this module to images (else
    vqvae_amd.decode runs the module itself).  Exactly: looks_like_spatial_decoder(m), and
      - both norm layers are nn.Identity, or both are nn.BatchNorm2d in eval mode with running statistics (affine or not);
      - conv_in and the three transposed convolutions have a bias;
      - 1 <= latent_dim <= 64; (dec_channels[1], dec_channels[2]) is (128, 64) or (64, 32), any dec_channels[0];
      - 1 or 3 output channels; output 32 px (last padding 1) or 28 px (last padding 3).
    Anything else -- GroupNorm, train-mode BatchNorm, BatchNorm without running statistics, a layer without bias, other
    widths -- is not covered."""
    if not looks_like_spatial_decoder(m):
        return False
    seq = m.deconv_layers
    if not (_fixed_statistics(seq[1]) and _fixed_statistics(seq[4])):
        return False
    if any(layer.bias is None for layer in (m.conv_in, seq[0], seq[3], seq[6])):
        return False
    return (1 <= m.conv_in.in_channels <= MAX_IMAGE_LATENT_DIM and m.conv_in.out_channels == seq[0].in_channels
            and seq[0].out_channels == seq[3].in_channels and seq[3].out_channels == seq[6].in_channels
            and (seq[0].out_channels, seq[3].out_channels) in COVERED_WIDTHS and seq[6].out_channels in (1, 3))


class SpatialImageDecoderExport:
    """A covered decoder as geo_spatial_decode reads it: conv_in composed into ConvT1 in fp64 and rounded to f32 once, both
    norms folded into a scale and a shift, the three transposed convolutions laid out by output-pixel parity and tap
    (`_parity_taps`), as f32 tensors on `dev` plus the ctypes descriptor over them.

    conv_in's bias reaches an 8x8 pixel only through the taps that lie inside the 4x4 grid, so it is not a per-channel
    constant.  It is carried as input channel d, which the kernel holds at 1 inside the grid; outside the grid every channel,
    that one included, is 0.  `host` keeps the fp64 originals: "W" [parity][tap][d + 1][c1] (row d is the bias row),
    "scale1", "shift1" [c1] with pre1 = scale1 * sum(taps, channels) + shift1 (ConvT1's bias inside shift1).
    `tensors` are what geo_spatial_decode reads; `adjoint` holds the transposed packs that geo_spatial_vjp and the grid curves read
    besides: "w2t", "w3t" as in VanillaDecoderExport, "w1t" [16][c1 / 4][dn][4] the composed first stage by
    kernel tap 4 ky + kx with scale1 folded in, latent channels only (the bias channel has no gradient), dn = d rounded up to 32.
    A snapshot: later changes of the module (weights, statistics, mode) are not seen."""

    def __init__(self, dec: nn.Module, dev: torch.device):
        if not spatial_image_kernels_cover(dec):
            raise ValueError("decoder not covered by the spatial image decode (see spatial_image_kernels_cover)")
        seq = dec.deconv_layers
        conv1, norm1, conv2, norm2, out = seq[0], seq[1], seq[3], seq[4], seq[6]
        d, c0, c1, c2, C = dec.conv_in.in_channels, dec.conv_in.out_channels, conv1.out_channels, conv2.out_channels, out.out_channels

        with torch.no_grad():
            aug = torch.cat([f64(dec.conv_in.weight).view(c0, d), f64(dec.conv_in.bias)[:, None]], 1)      # [c0][d + 1]
            W = torch.einsum("ck,ptco->ptko", aug, _parity_taps(f64(conv1.weight)))                        # [4][4][d + 1][c1]
            scale1, shift1 = _fold(norm1, c1)
            shift1 = shift1 + scale1 * f64(conv1.bias)
            dp = (d + 1 + 7) // 8 * 8
            w1p = torch.zeros(4, 4, dp, c1, dtype=torch.float64)
            w1p[:, :, :d + 1] = W
            w1p = pack_k_quads(w1p)                                                                        # [4][4][dp / 4][c1][4]
            scale2, shift2 = _fold(norm2, c2)
            shift2 = shift2 + scale2 * f64(conv2.bias)
            w2p = pack_k_quads(_parity_taps(f64(conv2.weight)))                                            # [4][4][c1 / 4][c2][4]
            w3p = _parity_taps(f64(out.weight)).permute(0, 1, 3, 2)                                        # [4][4][C][c2]
            # the transposed packs: every layer by kernel tap 4 ky + kx, the first as a K-quad B operand [c1][dn]
            w1n = torch.zeros(16, c1, (d + 31) // 32 * 32, dtype=torch.float64)
            w1n[:, :, :d] = torch.einsum("ck,coyx,o->yxok", aug[:, :d], f64(conv1.weight), scale1).reshape(16, c1, d)
            w1t = pack_k_quads(w1n)                                                                        # [16][c1 / 4][dn][4]
            w2t = pack_k_quads(f64(conv2.weight).permute(2, 3, 1, 0).reshape(16, c2, c1))                  # [16][c2 / 4][c1][4]
            w3t = f64(out.weight).permute(2, 3, 1, 0).reshape(16, C, c2)                                   # [16][C][c2]
        self.host = {"W": W, "scale1": scale1, "shift1": shift1}
        packed = {"w1p": w1p, "scale1": scale1, "shift1": shift1, "w2p": w2p, "scale2": scale2, "shift2": shift2, "w3p": w3p,
                  "b3": f64(out.bias)}
        self.tensors = {k: f32(v, dev) for k, v in packed.items()}
        self.adjoint = {k: f32(v, dev) for k, v in {"w1t": w1t, "w2t": w2t, "w3t": w3t}.items()}
        self.latent_dim, self.out_channels, self.out_size = d, C, {1: 32, 3: 28}[out.padding[0]]
        self.n_out = C * self.out_size ** 2
        desc = _lib.SpatialImageDecoderDesc()
        desc.latent_dim, desc.c1, desc.c2, desc.out_channels, desc.out_size = d, c1, c2, C, self.out_size
        self.desc = fill_desc(fill_desc(desc, self.tensors), self.adjoint)
