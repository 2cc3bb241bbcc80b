"""Shared by test_encode_host.py and test_gpu_encode.py: seeded encoders with non-trivial BatchNorm parameters and statistics,
the images of the accuracy test, and the fp64 / float32 CPU references of the image encode (computed once per case,
read-only)."""
import copy
import functools

import torch
import torch.nn as nn

from vanilla_jvp_cases import plain_batchnorm

# (kind, name) -> (enc_channels, latent_dim, in_channels, image size, norm_type)
CASES = {
    ("vanilla", "wide-bn-28"): ((64, 128, 256), 128, 1, 28, "batch"),
    ("vanilla", "wide-bn-32x3"): ((64, 128, 256), 128, 3, 32, "batch"),
    ("vanilla", "narrow-none-28"): ((32, 64, 128), 16, 1, 28, "none"),
    ("vanilla", "narrow-none-32x3-d5"): ((32, 64, 128), 5, 3, 32, "none"),
    ("spatial", "wide-bn-28-d16"): ((64, 128, 256), 16, 1, 28, "batch"),
    ("spatial", "wide-bn-32x3-d32"): ((64, 128, 256), 32, 3, 32, "batch"),
    ("spatial", "narrow-none-28-d5"): ((32, 64, 128), 5, 1, 28, "none"),
}
ALL_CASES = list(CASES)
# Points of the admitted envelope (encoder_kernels_cover) chosen for the branches of enc_head_kernel they reach: ntiles =
# ceil(2 d / 32) column tiles, of which wave w takes w and w + 4.  "batch-plain" is BatchNorm2d(affine=False).
ENVELOPE_CASES = {
    ("vanilla", "narrow-bn-28-d1"): ((32, 64, 128), 1, 1, 28, "batch"),               # d = 1: two live columns
    ("vanilla", "wide-none-32x3-d33"): ((64, 128, 256), 33, 3, 32, "none"),           # 3 tiles: one idle wave
    ("vanilla", "narrow-bn-32x3-d65"): ((32, 64, 128), 65, 3, 32, "batch"),           # 5 tiles: only wave 0 takes a second one
    ("vanilla", "wide-none-28-d96"): ((64, 128, 256), 96, 1, 28, "none"),             # 6 tiles, mu / logvar boundary on a tile edge
    ("vanilla", "narrow-none-28-d100"): ((32, 64, 128), 100, 1, 28, "none"),          # 7 tiles
    ("vanilla", "wide-bn-28-d127"): ((64, 128, 256), 127, 1, 28, "batch"),            # 8 tiles, two dead columns in the last
    ("spatial", "narrow-bn-32x3-d1"): ((32, 64, 128), 1, 3, 32, "batch"),
    ("spatial", "wide-none-28-d33"): ((64, 128, 256), 33, 1, 28, "none"),             # 3 tiles
    ("spatial", "narrow-none-32x3-d64"): ((32, 64, 128), 64, 3, 32, "none"),          # 4 tiles, the maximum
    ("spatial", "wide-bn-28-d63"): ((64, 128, 256), 63, 1, 28, "batch"),              # odd d just under the maximum
    ("vanilla", "wide-plainbn-32x3-d40"): ((64, 128, 256), 40, 3, 32, "batch-plain"),
    ("spatial", "narrow-plainbn-28-d20"): ((32, 64, 128), 20, 1, 28, "batch-plain"),
}
ALL_ENVELOPE_CASES = list(ENVELOPE_CASES)
N_VANILLA, N_SPATIAL = 77, 37           # no multiple of the 1, 2 or 4 items of a convolution workgroup, nor of the 32 head rows


def make_encoder(kind, channels, latent_dim, in_channels, norm_type, seed=0, eval_mode=True) -> nn.Module:
    """Encoder / SpatialEncoder with torch's seeded default weights and, for BatchNorm / GroupNorm, seeded non-trivial affine
    parameters and running statistics."""
    from vqvae_amd.spatial_vae import SpatialEncoder
    from vqvae_amd.vae import Encoder
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        if kind == "vanilla":
            enc = Encoder(in_channels, tuple(channels), latent_dim, norm_type)
        else:
            enc = SpatialEncoder(in_channels, tuple(channels), latent_dim, norm_type)
        with torch.no_grad():
            for m in enc.modules():
                if isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                    m.weight.copy_(1.0 + 0.2 * torch.randn_like(m.weight))
                    m.bias.copy_(0.1 * torch.randn_like(m.bias))
                if isinstance(m, nn.BatchNorm2d):
                    m.running_mean.copy_(0.1 * torch.randn_like(m.running_mean))
                    m.running_var.copy_(0.5 + torch.rand_like(m.running_var))
    return enc.eval() if eval_mode else enc.train()


def build(kind, channels, latent_dim, in_channels, norm_type, seed=0) -> nn.Module:
    """make_encoder in eval mode, with "batch-plain" meaning plain_batchnorm of the "batch" encoder."""
    if norm_type == "batch-plain":
        return plain_batchnorm(make_encoder(kind, channels, latent_dim, in_channels, "batch", seed=seed), seed)
    return make_encoder(kind, channels, latent_dim, in_channels, norm_type, seed=seed)


def images(n, in_channels, size, seed=1) -> torch.Tensor:
    """Uniform [0, 1) images for one channel, normal ones for three; image 0 is all zeros and image 1 all ones (the border
    outputs of a constant image differ from the interior only through the padding taps)."""
    g = torch.Generator().manual_seed(seed)
    shape = (n, in_channels, size, size)
    x = torch.rand(shape, generator=g) if in_channels == 1 else torch.randn(shape, generator=g)
    if n > 0:
        x[0] = 0.0
    if n > 1:
        x[1] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def case(kind, name):
    """(encoder on the CPU in eval mode, x, fp64 mu, fp64 logvar, float32-torch maximum error of mu, of logvar)."""
    return _case(CASES, kind, name)


@functools.lru_cache(maxsize=None)
def envelope_case(kind, name):
    """`case` for ENVELOPE_CASES."""
    return _case(ENVELOPE_CASES, kind, name)


def _case(table, kind, name):
    channels, d, C, size, norm = table[(kind, name)]
    enc = build(kind, channels, d, C, norm, seed=len(name))
    x = images(N_VANILLA if kind == "vanilla" else N_SPATIAL, C, size)
    with torch.no_grad():
        mu64, lv64 = copy.deepcopy(enc).double()(x.double())
        mu32, lv32 = copy.deepcopy(enc).float()(x.float())
    return (enc, x, mu64, lv64, float((mu32.double() - mu64).abs().max()), float((lv32.double() - lv64).abs().max()))
