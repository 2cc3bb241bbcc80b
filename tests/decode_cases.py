"""Shared by test_decode_host.py and test_gpu_decode.py: seeded spatial decoders with non-trivial statistics, the latents of
the accuracy test, and the fp64 / float32 CPU references of the image decode (computed once per case, read-only)."""
import copy
import functools

import torch
import torch.nn as nn

import vanilla_jvp_cases as V

# name -> (dec_channels, latent_dim, out_channels, output_image_size, norm_type)
SPATIAL_CASES = {
    "wide-bn-28-d16": ((256, 128, 64), 16, 1, 28, "batch"),
    "wide-bn-32x3-d32": ((256, 128, 64), 32, 3, 32, "batch"),
    "narrow-none-28-d5": ((128, 64, 32), 5, 1, 28, "none"),
}
# Points of the admitted envelope (spatial_image_kernels_cover) chosen for sd_front_kernel's K blocks, dp = (d + 8) & ~7 with
# the constant-one channel at index d: the last lane of a block (d = 7, 63), the first of a fresh one (d = 8, 64 -- the LDS
# maximum), d = 1; 3 channels at 32 and at 28 px (crop 2) on both widths.  "batch-plain" is BatchNorm2d(affine=False).
SPATIAL_ENVELOPE_CASES = {
    "narrow-bn-32x3-d7": ((128, 64, 32), 7, 3, 32, "batch"),
    "wide-none-28x3-d8": ((256, 128, 64), 8, 3, 28, "none"),
    "wide-bn-32x1-d64": ((256, 128, 64), 64, 1, 32, "batch"),
    "narrow-none-32x1-d1": ((128, 64, 32), 1, 1, 32, "none"),
    "narrow-bn-28x3-d63": ((128, 64, 32), 63, 3, 28, "batch"),
    "c0-96-plainbn-28x1-d24": ((96, 128, 64), 24, 1, 28, "batch-plain"),
}
N_VANILLA, N_SPATIAL = 77, 37           # no multiple of the 4, 5 or 16 items of a mid workgroup, nor of the 64 front rows


def make_spatial_decoder(channels, latent_dim, out_channels, size, norm_type, seed=0, eval_mode=True) -> nn.Module:
    """SpatialDecoder with torch's seeded default weights and, for BatchNorm / GroupNorm, seeded non-trivial affine parameters
    and running statistics (as vanilla_jvp_cases.make_decoder)."""
    from vqvae_amd.spatial_decoder import SpatialDecoder
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        dec = SpatialDecoder(out_channels, tuple(channels), latent_dim, size, norm_type)
        with torch.no_grad():
            for m in dec.modules():
                if isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                    m.weight.copy_(1.0 + 0.2 * torch.randn_like(m.weight))
                    m.bias.copy_(0.1 * torch.randn_like(m.bias))
                if isinstance(m, nn.BatchNorm2d):
                    m.running_mean.copy_(0.1 * torch.randn_like(m.running_mean))
                    m.running_var.copy_(0.5 + torch.rand_like(m.running_var))
    return dec.eval() if eval_mode else dec.train()


def build_spatial(channels, latent_dim, out_channels, size, norm_type, seed=0) -> nn.Module:
    """make_spatial_decoder in eval mode, with "batch-plain" meaning vanilla_jvp_cases.plain_batchnorm of the "batch" decoder."""
    if norm_type == "batch-plain":
        return V.plain_batchnorm(make_spatial_decoder(channels, latent_dim, out_channels, size, "batch", seed=seed), seed)
    return make_spatial_decoder(channels, latent_dim, out_channels, size, norm_type, seed=seed)


def grids(n, latent_dim, seed=1) -> torch.Tensor:
    return torch.randn(n, latent_dim, 4, 4, generator=torch.Generator().manual_seed(seed))


def vectors(n, latent_dim, seed=1) -> torch.Tensor:
    return torch.randn(n, latent_dim, generator=torch.Generator().manual_seed(seed))


def _references(dec, z):
    """(fp64 logits of the module on the CPU, maximum absolute error of the same module in float32 on the CPU)."""
    with torch.no_grad():
        truth = copy.deepcopy(dec).double()(z.double())
        f32 = copy.deepcopy(dec).float()(z.float())
    return truth, float((f32.double() - truth).abs().max())


@functools.lru_cache(maxsize=None)
def vanilla_case(name):
    """(decoder on the CPU in eval mode, z [77, d], fp64 logits, float32-torch maximum error)."""
    return _vanilla(V.CASES, name)


@functools.lru_cache(maxsize=None)
def vanilla_envelope_case(name):
    """`vanilla_case` for vanilla_jvp_cases.ENVELOPE_CASES."""
    return _vanilla(V.ENVELOPE_CASES, name)


def _vanilla(table, name):
    channels, d, C, size, norm = table[name]
    dec = V.build(channels, d, C, size, norm, seed=len(name))
    z = vectors(N_VANILLA, d)
    return (dec, z) + _references(dec, z)


@functools.lru_cache(maxsize=None)
def spatial_case(name):
    """(decoder on the CPU in eval mode, z [37, d, 4, 4], fp64 logits, float32-torch maximum error)."""
    return _spatial(SPATIAL_CASES, name)


@functools.lru_cache(maxsize=None)
def spatial_envelope_case(name):
    """`spatial_case` for SPATIAL_ENVELOPE_CASES."""
    return _spatial(SPATIAL_ENVELOPE_CASES, name)


def _spatial(table, name):
    channels, d, C, size, norm = table[name]
    dec = build_spatial(channels, d, C, size, norm, seed=len(name))
    z = grids(N_SPATIAL, d)
    return (dec, z) + _references(dec, z)
