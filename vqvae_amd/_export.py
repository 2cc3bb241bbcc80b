"""What the native exports (VanillaDecoderExport, SpatialImageDecoderExport, ImageEncoderExport, LPIPSExport) and their call
wrappers (decode, encode, eval.lpips, the vanilla pull-back) share: the weight layouts of csrc/mfma_conv.h (DESIGN.md section
20), the fixed-statistics norm fold, the casts, the descriptor fill, the capped workspace and the eval-mode guard."""
import contextlib
import ctypes

import torch
import torch.nn as nn

from . import _lib


def f64(t: torch.Tensor) -> torch.Tensor:
    """fp64 on the CPU: what the exports compose in."""
    return t.detach().double().cpu()


def f32(t: torch.Tensor, dev) -> torch.Tensor:
    """The one rounding to f32, contiguous on `dev`."""
    return t.to(torch.float32).contiguous().to(dev)


def pack_k_quads(w: torch.Tensor) -> torch.Tensor:
    """[..., K, N] -> [..., K / 4, N, 4]: element (q, n, r) = w[4 q + r][n], the B operand of mfma_conv.h (a view)."""
    *lead, K, N = w.shape
    return w.reshape(*lead, K // 4, 4, N).transpose(-1, -2)


def conv_taps(w: torch.Tensor) -> torch.Tensor:
    """Conv2d weight [cout][cin][k][k] -> [tap k ky + kx][cin / 4][cout][4]: element (tap, q, co, r) = w[co][4 q + r][ky][kx]."""
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    return pack_k_quads(w.permute(2, 3, 1, 0).reshape(k * k, cin, cout))


def _parity_taps(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d(k4, s2, p1) weight [cin][cout][4][4] -> [parity 2 py + px][tap 2 a + b][cin][cout]: output pixel
    (2 y + py, 2 x + px) reads input pixel (y + py - a, x + px - b) through kernel element (2 a + 1 - py, 2 b + 1 - px)."""
    rows = []
    for py in (0, 1):
        for px in (0, 1):
            rows.append(torch.stack([w[:, :, 2 * a + 1 - py, 2 * b + 1 - px] for a in (0, 1) for b in (0, 1)]))
    return torch.stack(rows)


def _fixed_statistics(norm: nn.Module) -> bool:
    if isinstance(norm, nn.Identity):
        return True
    # torch normalises with the running statistics exactly when the LAYER is in eval mode and tracks them
    return (isinstance(norm, nn.BatchNorm2d) and not norm.training and norm.running_mean is not None
            and norm.running_var is not None)


def _fold(norm: nn.Module, channels: int):
    """(scale, shift) in fp64 on the CPU of a fixed-statistics norm layer: y = scale x + shift."""
    if isinstance(norm, nn.Identity):
        return torch.ones(channels, dtype=torch.float64), torch.zeros(channels, dtype=torch.float64)
    rm, rv = f64(norm.running_mean), f64(norm.running_var)
    scale = 1.0 / torch.sqrt(rv + norm.eps)
    if norm.weight is not None:
        scale = scale * f64(norm.weight)
    shift = -rm * scale
    if norm.bias is not None:
        shift = shift + f64(norm.bias)
    return scale, shift


def fill_desc(desc, tensors):
    """Points the descriptor's fields at the tensors of the same names (None stays a null pointer); returns it."""
    for name, t in tensors.items():
        setattr(desc, name, None if t is None else ctypes.c_void_p(t.data_ptr()))
    return desc


def capped_workspace(query_bytes: int, max_workspace_bytes, dev, what: str) -> torch.Tensor:
    """The cached workspace cut to a *_workspace_bytes answer, or to `max_workspace_bytes` when that is less.  An answer of 0
    means the library does not take the configuration: GeoHipError "`what` configuration not supported by the HIP path"."""
    from ._device import workspace
    if query_bytes == 0:
        raise _lib.GeoHipError(f"{what} configuration not supported by the HIP path")
    nbytes = query_bytes if max_workspace_bytes is None else min(query_bytes, int(max_workspace_bytes))
    return workspace(nbytes, dev)[:nbytes]


@contextlib.contextmanager
def eval_mode(module: nn.Module):
    """The module in eval(); every layer's own mode is put back afterwards."""
    modes = [(m, m.training) for m in module.modules()]
    module.eval()
    try:
        yield module
    finally:
        for m, mode in modes:
            m.training = mode
