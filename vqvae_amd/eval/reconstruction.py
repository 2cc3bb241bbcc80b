"""Streamed quantize -> decode -> compare on the device: the work every evaluation CLI does.

  - nearest_medoid_assign: Euclidean nearest medoid by geo_kmeans_assign (exact fp64 key, ties to the lowest index) in place
    of the reference's float32 a^2 + b^2 - 2ab argmin; the two can differ only on near-ties.  Inputs outside that ABI's
    envelope (d > 128, K > 4096, K > n) take a chunked fp64 torch argmin.  last_assign_path() records which ran ("hip" or
    "torch_fp64").
  - quantize: vector latents (N, d) row by row; spatial latents (N, C, h, w) -- an extension, the reference's scripts raise on
    them -- position by position, rows in the (n, h, w) order build_codebook uses, codes mapped back to (N, h, w) and the
    gathered medoids permuted back to (N, C, h, w).
  - decode_pair_moments: decoder batches in eval() mode under no_grad, each post-processed exactly as the reference's
    unnormalize_images (float32 torch ops, so the images are the reference's for the same decoder output), then the moments
    kernel into one device f64 [N][6] per image pair.  Images stay on the device unless the caller asks for them.
The decoder itself stays torch: the JVP kernels of csrc/jvp.hip decode a 1x1 latent patch, not a whole image.
A native decode of whole images now exists (vqvae_amd.decode); the evaluation CLIs built on this module
do not use it yet.
"""
from typing import Dict, Optional

import torch

from .. import cluster
from .metrics import MAX_PIX, image_pair_moments, psnr_from_moments, ssim_from_moments

_last_assign_path = None

_CIFAR_MEAN = (0.4914, 0.4822, 0.4465)
_CIFAR_STD = (0.2470, 0.2430, 0.2610)


def last_assign_path() -> Optional[str]:
    """"hip" or "torch_fp64": the assignment the last nearest_medoid_assign / quantize call ran."""
    return _last_assign_path


def unnormalize_images(x: torch.Tensor, dataset_name: str, apply_sigmoid: bool) -> torch.Tensor:
    """The reference's post-processing: CIFAR-10 without sigmoid is un-normalised with its statistics and clamped; anything
    else gets a sigmoid when apply_sigmoid, else a clamp to [0, 1]."""
    if dataset_name.upper() == "CIFAR10" and not apply_sigmoid:
        mean = torch.tensor(list(_CIFAR_MEAN), device=x.device).view(1, 3, 1, 1)
        std = torch.tensor(list(_CIFAR_STD), device=x.device).view(1, 3, 1, 1)
        return (x * std + mean).clamp(0, 1)
    return torch.sigmoid(x) if apply_sigmoid else x.clamp(0, 1)


@torch.no_grad()
def nearest_medoid_assign(z: torch.Tensor, z_medoid: torch.Tensor, batch_size: int = 8192) -> torch.Tensor:
    """Codes int64 [n] (on z's device, a GPU) of the rows of z f32 [n, d] against z_medoid f32 [K, d] (module docstring)."""
    global _last_assign_path
    n, d = z.shape
    K = z_medoid.shape[0]
    z = z.float().contiguous()
    C = z_medoid.to(z.device).float().contiguous()
    if 1 <= d <= cluster.MAX_D and 1 <= K <= min(n, cluster.MAX_K):
        labels, _, _ = cluster.assign(z, C)
        _last_assign_path = "hip"
        return labels.long()
    C64 = C.double()
    chunk = max(1, min(batch_size, (1 << 28) // max(1, K * d * 8)))
    out = torch.empty(n, dtype=torch.int64, device=z.device)
    for i in range(0, n, chunk):
        zi = z[i:i + chunk].double()
        out[i:i + chunk] = ((zi[:, None, :] - C64[None]) ** 2).sum(-1).argmin(dim=1)
    _last_assign_path = "torch_fp64"
    return out


@torch.no_grad()
def quantize(z: torch.Tensor, z_medoid: torch.Tensor):
    """(codes, zq): vector latents (N, d) -> codes [N], zq [N, d]; spatial latents (N, C, h, w) -> codes [N, h, w] and zq
    (N, C, h, w) built from z_medoid[codes] (the spatial case is an extension of the reference)."""
    z_medoid = z_medoid.to(z.device).float()
    if z.dim() == 2:
        codes = nearest_medoid_assign(z, z_medoid)
        return codes, z_medoid[codes]
    if z.dim() != 4:
        raise ValueError(f"latents must be (N, d) or (N, C, h, w), got {tuple(z.shape)}")
    N, C, h, w = z.shape
    rows = z.permute(0, 2, 3, 1).reshape(-1, C)
    codes = nearest_medoid_assign(rows, z_medoid).view(N, h, w)
    zq = z_medoid[codes].permute(0, 3, 1, 2).contiguous()
    return codes, zq


@torch.no_grad()
def decode_pair_moments(decoder, za: torch.Tensor, zb: torch.Tensor, *, dataset: str, apply_sigmoid: bool,
                        batch_size: int = 512, n_samples: Optional[int] = None, x_real: Optional[torch.Tensor] = None,
                        return_images: bool = False) -> Dict:
    """Decode za and zb (the first n_samples rows, default all) in batches, post-process both like unnormalize_images and
    reduce every image pair with geo_image_pair_moments.  Returns {"a_b": f64 [n][6]} on the device, plus "real_a" and
    "real_b" when x_real (n or more post-processed images, any device) is given, "n_pix", and "a" / "b" (f32 images on the
    device) when return_images."""
    dev = next(decoder.parameters()).device
    decoder.eval()
    n = len(za) if n_samples is None else min(len(za), n_samples)
    out: Dict = {}
    keep = {"a": [], "b": []}
    for i in range(0, n, batch_size):
        j = min(i + batch_size, n)
        xa = unnormalize_images(decoder(za[i:j].to(dev)), dataset, apply_sigmoid)
        xb = unnormalize_images(decoder(zb[i:j].to(dev)), dataset, apply_sigmoid)
        b, P = xa.shape[0], xa[0].numel()
        if P > MAX_PIX:
            raise ValueError(f"images of {P} values: the moments kernel takes at most {MAX_PIX}")
        if not out:
            out = {"a_b": torch.empty(n, 6, dtype=torch.float64, device=dev), "n_pix": P}
            if x_real is not None:
                out["real_a"] = torch.empty_like(out["a_b"])
                out["real_b"] = torch.empty_like(out["a_b"])
        fa, fb = xa.reshape(b, P), xb.reshape(b, P)
        out["a_b"][i:j] = image_pair_moments(fa, fb)
        if x_real is not None:
            fr = x_real[i:j].to(dev).reshape(b, P)
            out["real_a"][i:j] = image_pair_moments(fr, fa)
            out["real_b"][i:j] = image_pair_moments(fr, fb)
        if return_images:
            keep["a"].append(xa)
            keep["b"].append(xb)
    if return_images:
        out["a"], out["b"] = torch.cat(keep["a"]), torch.cat(keep["b"])
    return out


def metrics_from_moments(mom: torch.Tensor, n_pix: int):
    """(psnr, ssim_simple) of 4-D image batches from their per-image moments: the formulas of vqvae_amd.eval.metrics."""
    m = mom.cpu().numpy()
    return psnr_from_moments(m, n_pix), ssim_from_moments(m)
