"""Drop-in for the reference's src/eval/metrics.py: psnr, ssim_simple and codebook_stats with the same signatures and return
types.  Every metric reduces to per-image pair moments (mean_x, mean_y, var_x, var_y, cov_xy, sse), accumulated in fp64:
tensors on the GPU go through the HIP kernel geo_image_pair_moments (csrc/evalstats.hip), CPU tensors through the same
formulas in numpy.  The reference reduces in float32 torch; the formulas are unchanged.

  psnr          mse = (sum over images b, ascending, of sse_b) / (B P), clamp_min(1e-12), 10 log10(max_val^2 / mse).
  ssim_simple   4-D input (B, C, H, W): per image, with the SUM form of the denominator,
                    (2 mx my + C1)(2 cov + C2) / ((mx^2 + my^2 + C1) + (vx + vy + C2)),
                clamped to [0, 1] and averaged in ascending order.  The reference's batched branch adds the two factors of
                the denominator instead of multiplying them; this port is a drop-in and keeps that.  Any other rank: the
                whole tensor is one image and the denominator is the product (mx^2 + my^2 + C1)(vx + vy + C2).
  codebook_stats  codes < 0 ignored; counts by an integer bincount (exact); p = counts / max(sum, 1e-12) clamped to >= 1e-12,
                so a dead code contributes what the reference's does; entropy = -sum p log p in fp64.

On the GPU an image is at most MAX_PIX values (the kernel's cap); psnr splits longer images into rows, which changes nothing
(sse adds up), while ssim_simple needs whole images and rejects longer ones.
"""
import ctypes

import numpy as np
import torch
from torch import Tensor

from .. import _lib

MAX_PIX = 16384


def image_pair_moments(x: Tensor, y: Tensor) -> Tensor:
    """geo_image_pair_moments on rows: x, y device (B, P) -> f64 [B][6] (mean_x, mean_y, var_x, var_y, cov_xy, sse) on the
    same device.  1 <= P <= MAX_PIX.  Asynchronous on the current stream."""
    if x.shape != y.shape or x.dim() != 2:
        raise ValueError(f"image_pair_moments: x {tuple(x.shape)} and y {tuple(y.shape)} must be the same (B, P)")
    if not x.is_cuda or x.device != y.device:
        raise ValueError("image_pair_moments: x and y must be on the same GPU")
    B, P = x.shape
    x = x.detach().float().contiguous()
    y = y.detach().float().contiguous()
    out = torch.empty(B, 6, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(_lib.load().geo_image_pair_moments(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), B, P,
                                                      ctypes.c_void_p(out.data_ptr()), stream), "geo_image_pair_moments")
    return out


def image_pair_moments_numpy(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """The same moments on the host: x, y (B, P) -> f64 [B][6], centred two-pass in fp64."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = x.shape[1]
    mx, my = x.sum(axis=1) / n, y.sum(axis=1) / n
    dx, dy = x - mx[:, None], y - my[:, None]
    d = x - y
    return np.stack([mx, my, (dx * dx).sum(axis=1) / n, (dy * dy).sum(axis=1) / n, (dx * dy).sum(axis=1) / n,
                     (d * d).sum(axis=1)], axis=1)


def _moments(x: Tensor, y: Tensor, rows: int) -> np.ndarray:
    """Moments of x and y viewed as `rows` rows, on x's device; returned on the host."""
    if x.shape != y.shape:
        raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} differ in shape")
    if x.is_cuda or y.is_cuda:
        return image_pair_moments(x.reshape(rows, -1), y.reshape(rows, -1).to(x.device)).cpu().numpy()
    return image_pair_moments_numpy(x.detach().reshape(rows, -1).double().numpy(), y.detach().reshape(rows, -1).double().numpy())


def _psnr_rows(x: Tensor) -> int:
    """Rows for psnr: one per image when an image fits the kernel, else the fewest rows of at most MAX_PIX values."""
    n = x.numel()
    per = n // x.shape[0] if x.dim() >= 2 and x.shape[0] > 0 else n
    if not x.is_cuda or per <= MAX_PIX:
        return n // per
    r = max(p for p in range(1, MAX_PIX + 1) if per % p == 0)
    return n // r


def psnr_from_moments(mom: np.ndarray, n_pix: int, max_val: float = 1.0) -> float:
    """PSNR from per-row moments f64 [B][6] of rows of n_pix values: sse summed in ascending row order."""
    total = float(np.cumsum(np.asarray(mom)[:, 5])[-1])
    mse = max(total / (len(mom) * n_pix), 1e-12)
    return float(10.0 * np.log10(max_val ** 2 / mse))


def ssim_from_moments(mom: np.ndarray, C1: float = 0.01 ** 2, C2: float = 0.03 ** 2) -> float:
    """Mean of the per-image SSIM values (sum-form denominator, each clamped to [0, 1]) in ascending order: the 4-D branch."""
    mx, my, vx, vy, cxy = (np.asarray(mom)[:, k] for k in range(5))
    num = (2 * mx * my + C1) * (2 * cxy + C2)
    den = (mx ** 2 + my ** 2 + C1) + (vx + vy + C2)
    vals = np.clip(num / den, 0.0, 1.0).tolist()
    return sum(vals) / len(vals)


@torch.no_grad()
def psnr(x: Tensor, y: Tensor, max_val: float = 1.0) -> float:
    # x,y in [0,1], shape (N,C,H,W)
    rows = _psnr_rows(x)
    return psnr_from_moments(_moments(x, y, rows), x.numel() // rows, max_val)


@torch.no_grad()
def ssim_simple(x: Tensor, y: Tensor, C1=0.01 ** 2, C2=0.03 ** 2) -> float:
    """Per-image SSIM averaged for 4-D input (sum-form denominator, as the reference); global SSIM with the product-form
    denominator for any other rank (module docstring)."""
    if x.dim() == 4:
        if x.is_cuda and x[0].numel() > MAX_PIX:
            raise ValueError(f"ssim_simple on the GPU: {x[0].numel()} values per image, the kernel takes at most {MAX_PIX}")
        return ssim_from_moments(_moments(x, y, x.shape[0]), C1, C2)
    if x.is_cuda and x.numel() > MAX_PIX:
        raise ValueError(f"ssim_simple on the GPU: {x.numel()} values in one image, the kernel takes at most {MAX_PIX}")
    mx, my, vx, vy, cxy, _ = _moments(x, y, 1)[0]
    num = (2 * mx * my + C1) * (2 * cxy + C2)
    den = (mx ** 2 + my ** 2 + C1) * (vx + vy + C2)
    return float(min(max(num / den, 0.0), 1.0))


@torch.no_grad()
def codebook_stats(codes: torch.Tensor, K: int) -> dict:
    # codes: (N,) int64, may contain -1 for invalid/unassigned
    codes = torch.as_tensor(codes).reshape(-1).long()
    hist = torch.bincount(codes[codes >= 0], minlength=K)            # on the codes' device; integer counts are exact
    counts = hist.cpu().numpy().astype(np.float64)
    p = np.maximum(counts / max(float(counts.sum()), 1e-12), 1e-12)
    entropy = float(-(p * np.log(p)).sum())
    return {"entropy": entropy, "dead_codes": int((counts == 0).sum()), "used": int((counts > 0).sum())}
