"""LPIPS v0.1 with the AlexNet backbone, what the reference's `lpips.LPIPS(net='alex')` computes (src/eval/evaluate_model.py,
scripts/evaluate_baseline_simple.py), with the weights read from a file instead of fetched.

The function (normalize=False, spatial=False), for x0, x1 f32 [n, 3, H, W] in [-1, 1]:

    scaled = (x - shift) / scale per channel, shift = (-.030, -.088, -.188), scale = (.458, .448, .450)
    Conv(3,64,k11,s4,p2) ReLU -> f1;  MaxPool(3,s2) Conv(64,192,k5,p2) ReLU -> f2;  MaxPool(3,s2) Conv(192,384,k3,p1) ReLU -> f3;
    Conv(384,256,k3,p1) ReLU -> f4;  Conv(256,256,k3,p1) ReLU -> f5          (the convolutions zero-pad the SCALED image)
    u = f / (sqrt(sum_c f^2) + 1e-10);  d_l = mean over pixels of sum_c lin_l[c] (u0 - u1)^2;  value = d_1 + ... + d_5

  - LPIPSAlex: that function in plain torch -- the definition, the CPU route and the route for sizes the kernels do not cover.
  - load_lpips_weights: an LPIPSAlex from the file `torch.save(lpips.LPIPS(net='alex').state_dict(), path)` writes on a
    machine that has the package (or from torchvision's AlexNet keys for the backbone plus the lin layers).
  - preprocess_for_lpips: the reference's three lines (repeat to three channels, bilinear resize to 64, * 2 - 1), torch ops.
  - lpips_pairs / lpips_mean: per-pair values in f64 on the device and their mean (fp64 sum in ascending pair order / n).  Pairs
    of 3 x 64 x 64 f32 GPU images (`native_lpips_covers`) run in geo_lpips_alex (csrc/lpips.hip); anything else runs the
    module.  last_lpips_path() says which ran; the route follows from the images, never from an option.  On the native route
    a pair's value depends on nothing but its two images: not on the batch, the workspace, the stream, nor on which is x0.

Passing a module packs its weights on every call; a caller that evaluates repeatedly builds `LPIPSExport` once.
"""
from typing import Optional, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from .._export import capped_workspace, fill_desc
from .._export import conv_taps as _taps

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
CHANNELS = (64, 192, 384, 256, 256)                       # f1 .. f5
# (in, out, kernel, stride, padding) of the five convolutions
CONVS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
NATIVE_SIZE = 64
_TORCH_BATCH = 256

# Where the lpips package keeps each convolution (net.slice<k>.<i>) and torchvision's AlexNet does (features.<i>).  The lpips
# names are written from memory of lpips 0.1.4 and were not checked against the package.
_LPIPS_CONV_KEYS = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
_TORCHVISION_CONV_KEYS = ("features.0", "features.3", "features.6", "features.8", "features.10")
_LPIPS_LIN_KEYS = tuple(f"lin{l}.model.1.weight" for l in range(5))

_last_lpips_path = None


def last_lpips_path() -> Optional[str]:
    """"hip" or "torch": the route the last lpips_pairs call took."""
    return _last_lpips_path


class LPIPSAlex(nn.Module):
    """The function of the module docstring in plain torch, in the dtype of its parameters (float32, or float64 after
    .double(); the inputs are cast to it).  `convs[k]` are the five convolutions, `lins[k]` the lin weights as [C_k]
    vectors; shift and scale are float32 constants (a .double() module uses those rounded values, as the kernels do)."""

    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT, dtype=torch.float32).view(1, 3, 1, 1), persistent=False)
        self.register_buffer("scale", torch.tensor(SCALE, dtype=torch.float32).view(1, 3, 1, 1), persistent=False)
        self.convs = nn.ModuleList(nn.Conv2d(i, o, k, stride=s, padding=p) for i, o, k, s, p in CONVS)
        self.lins = nn.ParameterList(nn.Parameter(torch.zeros(c)) for c in CHANNELS)
        for p in self.parameters():
            p.requires_grad_(False)

    def features(self, x: torch.Tensor):
        h = (x.to(self.shift.dtype) - self.shift) / self.scale
        f1 = F.relu(self.convs[0](h))
        f2 = F.relu(self.convs[1](F.max_pool2d(f1, 3, 2)))
        f3 = F.relu(self.convs[2](F.max_pool2d(f2, 3, 2)))
        f4 = F.relu(self.convs[3](f3))
        f5 = F.relu(self.convs[4](f4))
        return f1, f2, f3, f4, f5

    def forward(self, x0: torch.Tensor, x1: torch.Tensor, per_layer: bool = False) -> torch.Tensor:
        """[n, 1, 1, 1] like the package, or the five layer values [n, 5]."""
        cols = []
        for f0, f1, lin in zip(self.features(x0), self.features(x1), self.lins):
            u0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
            u1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
            cols.append((lin.view(1, -1, 1, 1) * (u0 - u1) ** 2).sum(dim=1).mean(dim=(1, 2)))
        layers = torch.stack(cols, dim=1)
        if per_layer:
            return layers
        total = layers[:, 0]
        for k in range(1, 5):
            total = total + layers[:, k]
        return total.view(-1, 1, 1, 1)


def _layout() -> str:
    rows = [f"  {a}.weight {[o, i, k, k]} and {a}.bias [{o}]   (or {b}.weight / {b}.bias)"
            for a, b, (i, o, k, _, _) in zip(_LPIPS_CONV_KEYS, _TORCHVISION_CONV_KEYS, CONVS)]
    rows += [f"  {a} [1, {c}, 1, 1]" for a, c in zip(_LPIPS_LIN_KEYS, CHANNELS)]
    return "expected layout:\n" + "\n".join(rows)


def load_lpips_weights(path) -> LPIPSAlex:
    """An LPIPSAlex (float32, on the CPU, eval mode) from a state-dict file.  The file is what

        torch.save(lpips.LPIPS(net='alex').state_dict(), path)

    writes on a machine that has the `lpips` package.  The key names below are from memory of lpips 0.1.4 and could not be
    checked against the package here:
      - the backbone as `net.slice1.0`, `net.slice2.3`, `net.slice3.6`, `net.slice4.8`, `net.slice5.10` (`.weight`, `.bias`),
        or under torchvision's AlexNet names `features.{0,3,6,8,10}`;
      - the lin layers as `lin0.model.1.weight` .. `lin4.model.1.weight`, shape [1, C, 1, 1];
      - `lins.*` (duplicates of the lin layers) are ignored;
      - `scaling_layer.shift` / `scaling_layer.scale`, if present, must equal the constants of LPIPS v0.1.
    A missing key or a wrong shape raises a ValueError that names the key and lists the expected layout."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: not a state dict\n{_layout()}")
    model = LPIPSAlex()

    def take(key, shape):
        if key not in sd:
            raise ValueError(f"{path}: key '{key}' is missing\n{_layout()}")
        t = torch.as_tensor(sd[key])
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{path}: key '{key}' has shape {list(t.shape)}, expected {list(shape)}\n{_layout()}")
        return t.detach().to(torch.float32)

    names = _LPIPS_CONV_KEYS if any(k.startswith("net.") for k in sd) else _TORCHVISION_CONV_KEYS
    with torch.no_grad():
        for conv, name, (i, o, k, _, _) in zip(model.convs, names, CONVS):
            conv.weight.copy_(take(name + ".weight", (o, i, k, k)))
            conv.bias.copy_(take(name + ".bias", (o,)))
        for lin, key, c in zip(model.lins, _LPIPS_LIN_KEYS, CHANNELS):
            lin.copy_(take(key, (1, c, 1, 1)).view(c))
    for key, const in (("scaling_layer.shift", SHIFT), ("scaling_layer.scale", SCALE)):
        if key in sd:
            got = torch.as_tensor(sd[key]).detach().to(torch.float32).reshape(-1)
            if got.numel() != 3 or not torch.equal(got, torch.tensor(const, dtype=torch.float32)):
                raise ValueError(f"{path}: key '{key}' is {got.tolist()}, LPIPS v0.1 has {list(const)}")
    return model.eval()


def preprocess_for_lpips(images: torch.Tensor, target_size: int = 64) -> torch.Tensor:
    """Prepares a batch of images in [0, 1] for LPIPS: the reference's function (src/eval/evaluate_model.py:92-102)."""
    if images.size(1) == 1:
        images = images.repeat(1, 3, 1, 1)
    images = F.interpolate(images, size=(target_size, target_size), mode="bilinear", align_corners=False)
    return images * 2 - 1


def native_lpips_covers(x: torch.Tensor) -> bool:
    """Whether geo_lpips_alex (csrc/lpips.hip) takes these images: a float32 GPU tensor [n, 3, 64, 64]."""
    return (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and tuple(x.shape[1:]) == (3, NATIVE_SIZE, NATIVE_SIZE))


def _first(w: torch.Tensor) -> torch.Tensor:
    """conv1.weight [64][3][11][11] -> [c 11 + ky][h][co][8]: element s < 6 = w[co][c][ky][2 s + h], 0 where kx = 11, s = 6, 7."""
    wk = torch.zeros(64, 3, 11, 16, dtype=w.dtype)
    wk[..., :11] = w
    return wk.view(64, 3, 11, 8, 2).permute(1, 2, 4, 0, 3).reshape(33, 2, 64, 8)


class LPIPSExport:
    """An LPIPSAlex as geo_lpips_alex reads it: f32 tensors on `dev` (geo_hip.h has the element formulas) plus the ctypes
    descriptor over them.  A snapshot: later changes of the module are not seen."""

    def __init__(self, model: LPIPSAlex, dev: torch.device):
        if not isinstance(model, LPIPSAlex):
            raise ValueError("LPIPSExport takes an LPIPSAlex")
        host = {}
        with torch.no_grad():
            for k, conv in enumerate(model.convs, start=1):
                w = conv.weight.detach().to("cpu", torch.float32)
                host[f"w{k}p"] = _first(w) if k == 1 else _taps(w)
                host[f"b{k}"] = conv.bias.detach().to("cpu", torch.float32)
            for k, lin in enumerate(model.lins, start=1):
                host[f"lin{k}"] = lin.detach().to("cpu", torch.float32)
        self.tensors = {k: v.contiguous().to(dev) for k, v in host.items()}
        self.device = torch.device(dev)
        self.desc = fill_desc(_lib.LPIPSAlexDesc(), self.tensors)


def _native(export: LPIPSExport, x0: torch.Tensor, x1: torch.Tensor, per_layer: bool, max_workspace_bytes) -> torch.Tensor:
    from .._device import ptr, stream_ptr
    lib = _lib.load()
    dev = export.device
    n = int(x0.shape[0])
    total = torch.empty(n, dtype=torch.float64, device=dev)
    layers = torch.empty((n, 5), dtype=torch.float64, device=dev) if per_layer else None
    if n == 0:
        return layers if per_layer else total
    if n >= 2 ** 31:
        raise ValueError(f"{n} pairs: the kernels take fewer than 2^31")
    x0 = x0.detach().to(dev).contiguous()
    x1 = x1.detach().to(dev).contiguous()
    with torch.cuda.device(dev):
        ws = capped_workspace(lib.geo_lpips_alex_workspace_bytes(n), max_workspace_bytes, dev, "lpips: network")
        _lib.check(lib.geo_lpips_alex(export.desc, ptr(x0), ptr(x1), n, ptr(total), ptr(layers), ptr(ws), ws.numel(), stream_ptr()),
                   "geo_lpips_alex")
    return layers if per_layer else total


@torch.no_grad()
def _torch_route(model: LPIPSAlex, x0: torch.Tensor, x1: torch.Tensor, per_layer: bool) -> torch.Tensor:
    """The module itself on its own device, in batches of 256; f64 like the native route."""
    dev = model.shift.device
    n = int(x0.shape[0])
    parts = [model(x0[i:i + _TORCH_BATCH].to(dev), x1[i:i + _TORCH_BATCH].to(dev), per_layer=per_layer).double()
             for i in range(0, n, _TORCH_BATCH)]
    if not parts:
        return torch.empty((0, 5) if per_layer else (0,), dtype=torch.float64, device=dev)
    out = torch.cat(parts)
    return out if per_layer else out.view(n)


def lpips_pairs(model_or_export: Union[LPIPSAlex, LPIPSExport], x0: torch.Tensor, x1: torch.Tensor, *, per_layer: bool = False,
                max_workspace_bytes: Optional[int] = None) -> torch.Tensor:
    """The LPIPS value of every pair (x0[i], x1[i]): f64 [n], or the five layer values f64 [n, 5], on the device.  The kernels run
    on the caller's current stream with the cached workspace; `max_workspace_bytes` caps it (not below
    geo_lpips_alex_workspace_bytes(1)) and changes no value."""
    global _last_lpips_path
    if x0.dim() != 4 or x0.shape != x1.shape or x0.shape[1] != 3:
        raise ValueError(f"images must be two (n, 3, H, W) batches of one shape, got {tuple(x0.shape)} and {tuple(x1.shape)}")
    obj = model_or_export
    native = native_lpips_covers(x0) and native_lpips_covers(x1) and x0.device == x1.device
    if isinstance(obj, LPIPSExport):
        if not native:
            raise ValueError("a prepared export takes float32 GPU images of 3 x 64 x 64 (native_lpips_covers); pass the module")
        export = obj
    elif not native:
        _last_lpips_path = "torch"
        return _torch_route(obj, x0, x1, per_layer)
    else:
        export = LPIPSExport(obj, x0.device)
    out = _native(export, x0, x1, per_layer, max_workspace_bytes)
    _last_lpips_path = "hip"
    return out


def lpips_mean(model_or_export, x0: torch.Tensor, x1: torch.Tensor, *, max_workspace_bytes: Optional[int] = None) -> float:
    """The mean over the pairs: the fp64 sum in ascending pair order divided by n (DESIGN.md section 10's rule)."""
    vals = lpips_pairs(model_or_export, x0, x1, max_workspace_bytes=max_workspace_bytes).cpu().tolist()
    if not vals:
        raise ValueError("lpips_mean of no pairs")
    total = 0.0
    for v in vals:
        total += v
    return total / len(vals)
