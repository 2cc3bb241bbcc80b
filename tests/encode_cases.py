"""Shared by test_encode_host.py and test_gpu_encode.py: seeded encoders with non-trivial BatchNorm parameters and statistics,
the images of the accuracy test, and the fp64 / float32 CPU references of the image encode (computed once per case,
read-only)."""
import copy
import functools

import torch
import torch.nn as nn

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
    channels, d, C, size, norm = CASES[(kind, name)]
    enc = make_encoder(kind, channels, d, C, norm, seed=len(name))
    x = images(N_VANILLA if kind == "vanilla" else N_SPATIAL, C, size)
    with torch.no_grad():
        mu64, lv64 = copy.deepcopy(enc).double()(x.double())
        mu32, lv32 = copy.deepcopy(enc).float()(x.float())
    return (enc, x, mu64, lv64, float((mu32.double() - mu64).abs().max()), float((lv32.double() - lv64).abs().max()))
