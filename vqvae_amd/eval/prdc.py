"""Precision, recall, density and coverage of a generated sample set against a real one, in a feature space.

Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020; the `prdc` package's
compute_prdc) are pairwise-distance tests against per-sample k-nearest-neighbour radii.  With n real features R, m generated
features F and k neighbours, four passes over all pairs:

    r2_R = kth_radius(R, k)                  the squared distance from each real to its k-th nearest OTHER real
    r2_F = kth_radius(F, k)
    cF   = ball_count(z=R, r2_R, q=F).count  how many real balls hold each fake
    cR, near = ball_count(z=F, r2_F, q=R)    how many fake balls hold each real; each real's nearest fake

    precision = #{cF > 0} / m                density  = sum(cF) / (k m)
    recall    = #{cR > 0} / n                coverage = #{near_key_i <= r2_R[i]} / n

These are the package's definitions on squared distances (a comparison of squares of non-negatives is the comparison of
their roots).  The key of a pair is the fp64 fma chain of include/geo_hip.h; the counts are integers and the ratios are formed
from them on the host, so the four figures are bit-identical across runs, streams and workspace sizes.

CUDA float32 features of width <= 1024 run on csrc/prdc.hip (geo_kth_radius, geo_ball_count).  CPU tensors, and shapes
outside that envelope, take a blocked torch fp64 route with the same rules: it never forms more than a bounded slab of the
difference tensor and gives the same results wherever no key is within rounding of its threshold.
"""
from typing import Dict, Optional

import numpy as np
import torch

MAX_K = 64                  # GEO_PRDC_MAX_K of include/geo_hip.h
MAX_WIDTH = 1024
_SLAB_ELEMENTS = 1 << 24    # fp64 elements of the torch route's difference slab (128 MiB)


# ------------------------------------------------------------------------------------------- checks (no library, no GPU)
def _check_features(name: str, t) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError(f"{name} must be a 2-D tensor, got {getattr(t, 'shape', type(t))}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if t.shape[1] < 1:
        raise ValueError(f"{name} has no columns")


def _check_k(k: int, rows: int, name: str) -> None:
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k = {k} outside [1, {MAX_K}]")
    if k >= rows:
        raise ValueError(f"k = {k} needs at least k + 1 rows of {name}, got {rows}")


def _check_width(d: int) -> None:
    if not 1 <= d <= MAX_WIDTH:
        raise ValueError(f"feature width {d} outside the supported range [1, {MAX_WIDTH}]")


def _check_finite(name: str, t: torch.Tensor) -> None:
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name} holds non-finite values")


def _check_ball_shapes(z, r2, q) -> None:
    _check_features("z", z)
    _check_features("q", q)
    if q.shape[1] != z.shape[1]:
        raise ValueError(f"queries have {q.shape[1]} columns, the corpus {z.shape[1]}")
    if z.shape[0] < 1:
        raise ValueError("the corpus has no rows")
    if not isinstance(r2, torch.Tensor) or r2.dtype != torch.float64 or tuple(r2.shape) != (z.shape[0],):
        raise ValueError(f"r2 must be float64 of shape ({z.shape[0]},), got {getattr(r2, 'dtype', None)} "
                         f"{tuple(getattr(r2, 'shape', ()))}")
    if z.device != q.device or r2.device != z.device:
        raise ValueError(f"corpus on {z.device}, radii on {r2.device}, queries on {q.device}")


def _need_cuda(name: str, t: torch.Tensor) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA tensor for the HIP path (prdc_device takes CPU tensors on its torch route)")


# --------------------------------------------------------------------------------------------------------- HIP callers
def _workspace(lib, n: int, m: int, d: int, max_workspace_bytes, dev, what: str):
    from .._export import capped_workspace
    cap = None if max_workspace_bytes is None else max(int(max_workspace_bytes), lib.geo_prdc_min_workspace_bytes(d))
    return capped_workspace(lib.geo_prdc_workspace_bytes(n, m, d), cap, dev, what)


def kth_radius_device(a: torch.Tensor, k: int, max_workspace_bytes: Optional[int] = None) -> torch.Tensor:
    """r2 float64 [n]: for every row of the resident features a (f32 [n, d], d <= 1024) the k-th smallest key to the OTHER rows
    (self left out by index; a duplicate row is a neighbour at key 0), by geo_kth_radius on the caller's stream.
    max_workspace_bytes caps the workspace (never below the library's minimum); the result does not depend on it."""
    _check_features("a", a)
    _check_k(k, a.shape[0], "a")
    _check_width(a.shape[1])
    _need_cuda("a", a)
    _check_finite("a", a)
    return _kth_radius(a, k, max_workspace_bytes)


def _kth_radius(a: torch.Tensor, k: int, max_workspace_bytes: Optional[int] = None) -> torch.Tensor:
    """kth_radius_device behind its checks (prdc_device has made them once for all four passes)."""
    from .. import _lib
    from .._device import ptr, stream_ptr
    lib = _lib.load()
    a = a.contiguous()
    n, d = a.shape
    r2 = torch.empty(n, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        ws = _workspace(lib, n, n, d, max_workspace_bytes, a.device, "kth_radius_device:")
        _lib.check(lib.geo_kth_radius(ptr(a), n, d, int(k), ptr(r2), ptr(ws), ws.numel(), stream_ptr()), "geo_kth_radius")
    return r2


def ball_count_device(z: torch.Tensor, r2: torch.Tensor, q: torch.Tensor, max_workspace_bytes: Optional[int] = None):
    """(count int32 [m], near_key float64 [m], near_idx int32 [m]) for the resident queries q (f32 [m, d]) against the corpus z
    (f32 [n, d]) with squared radii r2 (f64 [n]): count[j] = #{i : key(q_j, z_i) <= r2[i]}, near_key[j] the smallest key of
    query j and near_idx[j] the lowest corpus row attaining it, by geo_ball_count on the caller's stream."""
    _check_ball_shapes(z, r2, q)
    _check_width(z.shape[1])
    _need_cuda("z", z)
    _check_finite("z", z)
    _check_finite("q", q)
    return _ball_count(z, r2, q, max_workspace_bytes)


def _ball_count(z: torch.Tensor, r2: torch.Tensor, q: torch.Tensor, max_workspace_bytes: Optional[int] = None):
    """ball_count_device behind its checks."""
    from .. import _lib
    from .._device import ptr, stream_ptr
    lib = _lib.load()
    z, q, r2 = z.contiguous(), q.contiguous(), r2.contiguous()
    (n, d), m = z.shape, int(q.shape[0])
    count = torch.empty(m, dtype=torch.int32, device=z.device)
    near_key = torch.empty(m, dtype=torch.float64, device=z.device)
    near_idx = torch.empty(m, dtype=torch.int32, device=z.device)
    if m == 0:
        return count, near_key, near_idx
    with torch.cuda.device(z.device):
        ws = _workspace(lib, n, m, d, max_workspace_bytes, z.device, "ball_count_device:")
        _lib.check(lib.geo_ball_count(ptr(z), ptr(r2), n, ptr(q), m, d, ptr(count), ptr(near_key), ptr(near_idx), ptr(ws),
                                      ws.numel(), stream_ptr()), "geo_ball_count")
    return count, near_key, near_idx


# --------------------------------------------------------------------------------------------- torch fp64 blocked route
def _blocks(d: int):
    bq = 256
    bz = max(1, _SLAB_ELEMENTS // (bq * d))
    return bq, bz


def _keys(qb: torch.Tensor, zb: torch.Tensor) -> torch.Tensor:
    """fp64 keys [len(qb), len(zb)] by differences (never the norm expansion: no cancellation)."""
    t = qb.double()[:, None, :] - zb.double()[None, :, :]
    return (t * t).sum(-1)


def kth_radius_torch(a: torch.Tensor, k: int) -> torch.Tensor:
    n, d = a.shape
    bq, bz = _blocks(d)
    out = torch.empty(n, dtype=torch.float64, device=a.device)
    for i0 in range(0, n, bq):
        qb = a[i0:i0 + bq]
        rows = torch.arange(i0, i0 + len(qb), device=a.device)
        best = torch.full((len(qb), k), float("inf"), dtype=torch.float64, device=a.device)
        for j0 in range(0, n, bz):
            keys = _keys(qb, a[j0:j0 + bz])
            cols = torch.arange(j0, j0 + keys.shape[1], device=a.device)
            keys = keys.masked_fill(rows[:, None] == cols[None, :], float("inf"))       # self, by index
            best = torch.topk(torch.cat([best, keys], 1), k, dim=1, largest=False).values
        out[i0:i0 + len(qb)] = best.max(1).values
    return out


def ball_count_torch(z: torch.Tensor, r2: torch.Tensor, q: torch.Tensor):
    (n, d), m = z.shape, q.shape[0]
    bq, bz = _blocks(d)
    count = torch.zeros(m, dtype=torch.int32, device=z.device)
    near_key = torch.full((m,), float("inf"), dtype=torch.float64, device=z.device)
    near_idx = torch.full((m,), -1, dtype=torch.int32, device=z.device)
    for i0 in range(0, m, bq):
        qb = q[i0:i0 + bq]
        c = torch.zeros(len(qb), dtype=torch.int64, device=z.device)
        bk = torch.full((len(qb),), float("inf"), dtype=torch.float64, device=z.device)
        bi = torch.full((len(qb),), -1, dtype=torch.int64, device=z.device)
        for j0 in range(0, n, bz):
            keys = _keys(qb, z[j0:j0 + bz])
            c += (keys <= r2[None, j0:j0 + bz]).sum(1)
            kmin = keys.min(1).values
            cols = torch.arange(j0, j0 + keys.shape[1], device=z.device)
            first = torch.where(keys == kmin[:, None], cols[None, :], n).min(1).values      # the lowest index of the block
            better = kmin < bk                                                                # blocks ascend: ties keep theirs
            bk = torch.where(better, kmin, bk)
            bi = torch.where(better, first, bi)
        count[i0:i0 + len(qb)] = c.to(torch.int32)
        near_key[i0:i0 + len(qb)] = bk
        near_idx[i0:i0 + len(qb)] = bi.to(torch.int32)
    return count, near_key, near_idx


# -------------------------------------------------------------------------------------------------------- the figures
def _hip_route(real: torch.Tensor, fake: torch.Tensor) -> bool:
    return real.is_cuda and fake.is_cuda and real.shape[1] <= MAX_WIDTH


def prdc_device(real: torch.Tensor, fake: torch.Tensor, k: int = 5, route: Optional[str] = None) -> Dict[str, object]:
    """Precision, recall, density, coverage (Python floats) of the fake features (f32 [m, d]) against the real ones
    (f32 [n, d]) with k neighbours, and the per-sample tensors behind them: real_radius2, fake_radius2 (f64), fake_count
    (how many real balls hold each fake), real_count (how many fake balls hold each real), real_near_key, real_near_idx
    (each real's nearest fake).  `route`: "hip", "torch" or None = HIP for CUDA features of width <= 1024, else torch."""
    _check_features("real", real)
    _check_features("fake", fake)
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"real features have {real.shape[1]} columns, fake ones {fake.shape[1]}")
    _check_k(k, real.shape[0], "real")
    _check_k(k, fake.shape[0], "fake")
    if real.device != fake.device:
        raise ValueError(f"real features on {real.device}, fake ones on {fake.device}")
    _check_finite("real", real)
    _check_finite("fake", fake)
    if route is None:
        route = "hip" if _hip_route(real, fake) else "torch"
    if route == "hip":
        _check_width(real.shape[1])
        _need_cuda("real", real)
        r2_R, r2_F = _kth_radius(real, k), _kth_radius(fake, k)          # checked above, once: no second pass over the features
        cF = _ball_count(real, r2_R, fake)[0]
        cR, near_key, near_idx = _ball_count(fake, r2_F, real)
    elif route == "torch":
        real, fake = real.contiguous(), fake.contiguous()
        r2_R, r2_F = kth_radius_torch(real, k), kth_radius_torch(fake, k)
        cF = ball_count_torch(real, r2_R, fake)[0]
        cR, near_key, near_idx = ball_count_torch(fake, r2_F, real)
    else:
        raise ValueError(f"route = {route!r}: expected 'hip', 'torch' or None")
    n, m = int(real.shape[0]), int(fake.shape[0])
    ints = torch.stack([(cF > 0).sum(), cF.to(torch.int64).sum(), (cR > 0).sum(), (near_key <= r2_R).sum()]).cpu().tolist()
    return {"precision": ints[0] / m, "recall": ints[2] / n, "density": ints[1] / (k * m), "coverage": ints[3] / n,
            "route": route, "real_radius2": r2_R, "fake_radius2": r2_F, "fake_count": cF, "real_count": cR,
            "real_near_key": near_key, "real_near_idx": near_idx}


FIGURES = ("precision", "recall", "density", "coverage")


def compute_prdc(real_features, fake_features, nearest_k: int) -> Dict[str, float]:
    """The `prdc` package's compute_prdc signature: numpy features in, {"precision", "recall", "density", "coverage"} out.  On
    the MI355X when one is present, on the torch route otherwise.  Two differences from the package, both deliberate: the
    features are rounded to float32 first (the package works in the caller's dtype; the keys here are fp64 sums over float32
    coordinates), and nearest_k is limited to [1, 64] (ValueError beyond).  The figures are the package's by definition for
    float32-representable features and k <= 64; float64 features may differ where the rounding moves a key across a radius."""
    real = torch.from_numpy(np.ascontiguousarray(real_features, dtype=np.float32))
    fake = torch.from_numpy(np.ascontiguousarray(fake_features, dtype=np.float32))
    if torch.cuda.is_available():
        from .._device import device
        real, fake = real.to(device()), fake.to(device())
    res = prdc_device(real, fake, int(nearest_k))
    return {name: float(res[name]) for name in FIGURES}
