"""Shared by test_vanilla_jvp_host.py and test_gpu_vanilla_jvp.py: seeded vanilla decoders with non-trivial statistics, the
edge sets, the fp64 / float32 autograd references (computed once per case) and the accuracy criteria."""
import functools

import numpy as np
import torch
import torch.nn as nn

from vqvae_amd.geo.riemannian_metric import _generic_jvp_norms as _AUTOGRAD      # bound here, before any monkeypatching

# name -> (dec_channels, latent_dim, out_channels, output_image_size, norm_type)
CASES = {
    "wide-bn-28": ((256, 128, 64), 128, 1, 28, "batch"),
    "wide-bn-32x3": ((256, 128, 64), 128, 3, 32, "batch"),
    "narrow-none-28": ((128, 64, 32), 16, 1, 28, "none"),
    "narrow-none-32x3-d5": ((128, 64, 32), 5, 3, 32, "none"),
}
# Points of the admitted envelope (vanilla_kernels_cover) for the decode and the pull-back: d = 1 and 2, odd d above 5 (dp = d
# rounded to even), 3 channels at 28 px and 1 channel at 32 px, a dec_channels[0] other than 256 / 128, and "batch-plain" =
# BatchNorm2d(affine=False).  Name, width and seed fix the decoder and with it how many of the 2085 edges float32 autograd
# itself leaves outside 1e-5 (check_against_fp64's cap is 10).  The count is noted per case; a case is admitted with at most
# 6, the most any of CASES has.  On the wide BatchNorm 32-px decoder d = 1 has 9 (every edge lies along one line and crosses
# many ReLU boundaries), hence d = 2 there.  After changing a name, a width or a seed, count again (envelope_case on the CPU).
ENVELOPE_CASES = {
    "wide-none-28x3-d127": ((256, 128, 64), 127, 3, 28, "none"),                  # 6
    "wide-bn-32x1-d2": ((256, 128, 64), 2, 1, 32, "batch"),                       # 5
    "narrow-bn-28x3-d33": ((128, 64, 32), 33, 3, 28, "batch"),                    # 0
    "narrow-none-32x1-d1": ((128, 64, 32), 1, 1, 32, "none"),                     # 2
    "c0-192-bn-28-d65": ((192, 128, 64), 65, 1, 28, "batch"),                     # 5
    "c0-48-none-32x3-d7": ((48, 64, 32), 7, 3, 32, "none"),                       # 3
    "narrow-plainbn-28x1-d12": ((128, 64, 32), 12, 1, 28, "batch-plain"),         # 2
}
N_EDGES = 2085                          # no multiple of 32, 64, the items of a workgroup or the edges of a pass


def make_decoder(channels, latent_dim, out_channels, size, norm_type, seed=0, eval_mode=True) -> nn.Module:
    """vqvae_amd.vae.Decoder with torch's seeded default weights and, for BatchNorm / GroupNorm, seeded non-trivial affine
    parameters and running statistics."""
    from vqvae_amd.vae import Decoder
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        dec = Decoder(out_channels, tuple(channels), latent_dim, size, norm_type)
        with torch.no_grad():
            for m in dec.modules():
                if isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                    m.weight.copy_(1.0 + 0.2 * torch.randn_like(m.weight))
                    m.bias.copy_(0.1 * torch.randn_like(m.bias))
                if isinstance(m, nn.BatchNorm2d):
                    m.running_mean.copy_(0.1 * torch.randn_like(m.running_mean))
                    m.running_var.copy_(0.5 + torch.rand_like(m.running_var))
    return dec.eval() if eval_mode else dec.train()


def plain_batchnorm(module: nn.Module, seed=0) -> nn.Module:
    """Every BatchNorm2d of `module` replaced by BatchNorm2d(affine=False) in eval mode with seeded non-trivial running
    statistics; the other layers keep their weights."""
    g = torch.Generator().manual_seed(seed)
    for parent in list(module.modules()):
        for key, child in list(parent.named_children()):
            if isinstance(child, nn.BatchNorm2d):
                bn = nn.BatchNorm2d(child.num_features, affine=False)
                bn.running_mean.copy_(0.1 * torch.randn(child.num_features, generator=g))
                bn.running_var.copy_(0.5 + torch.rand(child.num_features, generator=g))
                setattr(parent, key, bn.eval())
    return module


def build(channels, latent_dim, out_channels, size, norm_type, seed=0) -> nn.Module:
    """make_decoder in eval mode, with "batch-plain" meaning plain_batchnorm of the "batch" decoder."""
    if norm_type == "batch-plain":
        return plain_batchnorm(make_decoder(channels, latent_dim, out_channels, size, "batch", seed=seed), seed)
    return make_decoder(channels, latent_dim, out_channels, size, norm_type, seed=seed)


def make_edges(latent_dim, n_edges=N_EDGES, seed=1):
    g = torch.Generator().manual_seed(seed)
    zs = torch.randn(n_edges, latent_dim, generator=g)
    return zs, zs + 0.3 * torch.randn(n_edges, latent_dim, generator=g)


def small_graph(latent_dim, n_nodes=300, n_edges=1500, seed=9):
    """(z [n_nodes, d], src, dst int32 [n_edges]) on the CPU: random endpoints, every 50th edge a self loop."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n_nodes, latent_dim, generator=g)
    src = torch.randint(0, n_nodes, (n_edges,), generator=g, dtype=torch.int32)
    dst = torch.randint(0, n_nodes, (n_edges,), generator=g, dtype=torch.int32)
    dst[::50] = src[::50]
    return z, src, dst


def autograd_lengths(decoder, zs, ze, dtype) -> np.ndarray:
    """The package's autograd route (riemannian_metric._generic_jvp_norms as imported here, before any monkeypatching) on a
    CPU copy of the decoder in `dtype`."""
    import copy
    dec = copy.deepcopy(decoder).cpu().to(dtype)
    zs, ze = zs.cpu().to(dtype), ze.cpu().to(dtype)
    delta = ze - zs
    out = [0.5 * (_AUTOGRAD(dec, zs[lo:lo + 512], delta[lo:lo + 512]) + _AUTOGRAD(dec, ze[lo:lo + 512], delta[lo:lo + 512]))
           for lo in range(0, zs.shape[0], 512)]
    return torch.cat(out).detach().numpy()


@functools.lru_cache(maxsize=None)
def case(name):
    """(decoder on the CPU in eval mode, z_start, z_end, fp64 autograd lengths, float32 autograd lengths); read-only."""
    return _case(CASES, name)


@functools.lru_cache(maxsize=None)
def envelope_case(name):
    """`case` for ENVELOPE_CASES."""
    return _case(ENVELOPE_CASES, name)


def _case(table, name):
    channels, d, C, size, norm = table[name]
    dec = build(channels, d, C, size, norm, seed=len(name))
    zs, ze = make_edges(d)
    return dec, zs, ze, autograd_lengths(dec, zs, ze, torch.float64), autograd_lengths(dec, zs, ze, torch.float32)


def rel_error(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.abs(want.astype(np.float64))


def check_against_fp64(got: np.ndarray, want: np.ndarray, what: str) -> None:
    """At least 99.5 % of the edges within 1e-5, maximum below 1e-3, 0.99-quantile below 2e-6 (relative).  The 0.5 % are a cap
    for edges with a ReLU pre-activation within float32 rounding of zero at an endpoint: any float32 evaluation moves those
    by 1e-5 .. 4e-4."""
    rel = rel_error(got, want)
    within, worst, q99 = float(np.mean(rel <= 1e-5)), float(rel.max()), float(np.quantile(rel, 0.99))
    print(f"{what}: {within:.4%} within 1e-5, max {worst:.3e}, q99 {q99:.3e}")
    assert within >= 0.995 and worst < 1e-3 and q99 < 2e-6, (what, within, worst, q99)
