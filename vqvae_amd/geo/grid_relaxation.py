"""Image curves under the whole spatial decoder: the vector-Jacobian product of a 4x4 latent grid, the energy of a curve of
grids and its monotone relaxation with fixed ends (an extension: the reference has no counterpart).

A point is a grid z [d, 4, 4] (16 d coordinates, NCHW), g(z) = sigmoid(decoder(z)) the whole image flattened [C S S], J its
Jacobian.  relaxation.py's definitions hold with these coordinates:
    seg_sq[f] = |g(x[f+1]) - g(x[f])|^2,   E = sum_f seg_sq[f],   grad[f] = 2 J(x[f])^T ((g[f] - g[f-1]) - (g[f+1] - g[f])),
seg_sq by `strided_fold_sum` (256 strided fp64 partial sums, then folded), E ascending, the residual in fp64 rounded once to
float32, and the accept / reject loop unchanged.  The first step differs: the trace would cost 16 d tangents per frame, so
    probe[f] = sum over the 16 d coordinates, ascending, in fp64, of (J(x[f])^T s)[k]^2,   s = `sign_probe`,
a one-sample estimate of tr J J^T (not a bound), takes its place: step = 1 / (8 max over interior f of probe[f]).

Decoders native_grid_relax_covers admits, with the tensors on a GPU, run geo_spatial_vjp / geo_spatial_curve_energy /
geo_spatial_curve_relax (csrc/vanilla_jvp.hip); every other decoder (GroupNorm, other widths), and the CPU, takes the torch
route with the same rules: the float32 eval module, torch.autograd.grad for both vector-Jacobian products, the reductions in
fp64 in the orders above.  Unlike the per-position relaxation this metric sees the overlap of neighbouring positions'
receptive fields, and it has no limit at latent_dim 16.
"""
import math

import torch

from .. import _lib
from .._device import ptr, stream_ptr
from .._export import capped_workspace, eval_mode
from ..spatial_decoder import SpatialImageDecoderExport, spatial_image_kernels_cover
from .relaxation import _BN_ERROR, MAX_FRAMES, CurveEnergy, RelaxedCurves, initial_step, trial_frames
from .riemannian_metric import _has_train_batchnorm


def native_grid_relax_covers(decoder) -> bool:
    """Whether geo_spatial_vjp and the grid curve calls take this decoder: exactly spatial_image_kernels_cover."""
    return spatial_image_kernels_cover(decoder)


def sign_probe(channels: int, size: int, device=None) -> torch.Tensor:
    """s f32 [C, S, S]: +1 where c + y + x is even, else -1."""
    c = torch.arange(channels, device=device).view(-1, 1, 1)
    y = torch.arange(size, device=device).view(1, -1, 1)
    x = torch.arange(size, device=device).view(1, 1, -1)
    return 1.0 - 2.0 * ((c + y + x) % 2).to(torch.float32)


def strided_fold_sum(v: torch.Tensor) -> torch.Tensor:
    """Sum over the last axis of v f64 [..., p] in the order of vc_residual_kernel: partial sum t of 256 adds entries t, t + 256,
    ... ascending from 0, then p[t] += p[t + s] for s = 128, 64, ..., 1."""
    p = v.shape[-1]
    rows = (p + 255) // 256
    padded = torch.zeros(*v.shape[:-1], rows * 256, dtype=torch.float64, device=v.device)
    padded[..., :p] = v
    padded = padded.view(*v.shape[:-1], rows, 256)
    part = torch.zeros(*v.shape[:-1], 256, dtype=torch.float64, device=v.device)
    for i in range(rows):
        part = part + padded[..., i, :]
    s = 128
    while s >= 1:
        part = part[..., :s] + part[..., s:2 * s]
        s //= 2
    return part[..., 0]


def _route(decoder_or_export, dev: torch.device, d: int):
    """(export or None, decoder or None): the native route's export, or the module of the torch route."""
    if isinstance(decoder_or_export, SpatialImageDecoderExport):
        if dev.type != "cuda":
            raise ValueError("a SpatialImageDecoderExport runs the native route only: the tensors must be on its GPU")
        export, decoder = decoder_or_export, None
        have = export.latent_dim
    else:
        decoder = decoder_or_export
        if _has_train_batchnorm(decoder):
            raise ValueError(_BN_ERROR)
        export = SpatialImageDecoderExport(decoder, dev) if native_grid_relax_covers(decoder) and dev.type == "cuda" else None
        if export is not None:
            decoder = None
        have = decoder_or_export.conv_in.in_channels
    if d != have:
        raise ValueError(f"the grids have {d} latent channels, the decoder {have}")
    return export, decoder


def _check_grids(z: torch.Tensor, lead: int, what: str) -> torch.Tensor:
    if z.ndim != lead + 3 or tuple(z.shape[-2:]) != (4, 4):
        raise ValueError(f"{what} must be [{'C, F, ' if lead == 2 else '., '}d, 4, 4], got {tuple(z.shape)}")
    if lead == 2 and not 2 <= z.shape[1] <= MAX_FRAMES:
        raise ValueError(f"F = {z.shape[1]} frames, must be in [2, {MAX_FRAMES}]")
    return z.detach().to(torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------------------ torch route
def _torch_vjps(decoder, z: torch.Tensor, us):
    """g f32 [n, p] of the grids z [n, d, 4, 4] and, for every u [n, p] of `us`, J(z_i)^T u_i f32 [n, d, 4, 4], by the float32
    eval module (on its device).  With fixed statistics an image depends on its own grid alone, so one backward pass over the
    batch gives every row's own product."""
    with eval_mode(decoder):
        x = z.clone().requires_grad_(True)
        g = torch.sigmoid(decoder(x)).reshape(z.shape[0], -1)
        outs = [torch.autograd.grad(g, x, u.reshape(g.shape), retain_graph=True)[0] for u in us]
    return g.detach().to(torch.float32), outs


def _torch_evaluate(decoder, x: torch.Tensor, probe: bool):
    """Evaluate(x) on the torch route, x [C, F, d, 4, 4] on the decoder's device: (energy, seg_sq, grad, probe or None, g)."""
    C, F = x.shape[:2]
    with torch.no_grad(), eval_mode(decoder):
        g = torch.sigmoid(decoder(x.reshape(C * F, *x.shape[2:]))).reshape(C, F, -1).to(torch.float32)
    gd = g.double()
    dseg = gd[:, 1:] - gd[:, :-1]
    seg = strided_fold_sum(dseg * dseg)
    energy = torch.zeros(C, dtype=torch.float64, device=x.device)
    for f in range(F - 1):
        energy = energy + seg[:, f]
    finite = torch.isfinite(x).reshape(C, -1).all(dim=1)
    energy = torch.where(finite, energy, torch.full_like(energy, float("nan")))
    r = torch.zeros_like(g)
    if F > 2:
        r[:, 1:-1] = ((gd[:, 1:-1] - gd[:, :-2]) - (gd[:, 2:] - gd[:, 1:-1])).to(torch.float32)
    us = [r.reshape(C * F, -1)]
    if probe:
        channels = decoder.deconv_layers[6].out_channels
        size = math.isqrt(g.shape[2] // channels)
        us.append(sign_probe(channels, size, x.device).reshape(1, -1).expand(C * F, -1))
    _, outs = _torch_vjps(decoder, x.reshape(C * F, *x.shape[2:]), us)
    grad = 2.0 * outs[0].double().reshape(x.shape)
    grad[:, 0] = 0.0
    grad[:, -1] = 0.0
    pr = None
    if probe:
        v = outs[1].double().reshape(C, F, -1)
        pr = torch.zeros(C, F, dtype=torch.float64, device=x.device)
        for k in range(v.shape[2]):
            pr = pr + v[:, :, k] * v[:, :, k]
    return energy, seg, grad, pr, g


def _torch_relax(decoder, x: torch.Tensor, n_iters: int, step: torch.Tensor):
    C, F = x.shape[:2]
    flat = lambda t: t.reshape(C, F, -1)
    E, seg, grad, pr, _ = _torch_evaluate(decoder, x, bool((step < 0).any()))
    energy0 = E.clone()
    if pr is not None:
        step = torch.where(step < 0, initial_step(pr), step)
    accepted = torch.zeros(C, dtype=torch.int32, device=x.device)
    for _ in range(n_iters if F > 2 else 0):
        y = trial_frames(flat(x), step, flat(grad)).reshape(x.shape)
        Ey, segy, grady, _, _ = _torch_evaluate(decoder, y, False)
        take = Ey < E                                   # (False for a NaN on either side)
        x = torch.where(take.view(-1, 1, 1, 1, 1), y, x)
        grad = torch.where(take.view(-1, 1, 1, 1, 1), grady, grad)
        seg = torch.where(take[:, None], segy, seg)
        E = torch.where(take, Ey, E)
        step = torch.where(take, 2.0 * step, step / 4.0)
        accepted = accepted + take.to(torch.int32)
    return x, energy0, E, seg, step, accepted


# ------------------------------------------------------------------------------------------------------------ public
def spatial_grid_vjp_device(decoder_or_export, z: torch.Tensor, u: torch.Tensor, index=None,
                            max_workspace_bytes=None) -> torch.Tensor:
    """out f64 [n, d, 4, 4], out[i] = J(z_i)^T u_i with z_i = z[index[i]] (index None: z[i]): z f32 [., d, 4, 4], u f32
    [n, C, S, S] (or flattened), `index` None or int32 [n].  A row's value does not depend on the batch; u_i = 0 gives exactly 0.
    `max_workspace_bytes` caps the native workspace (not below geo_spatial_vjp_min_workspace_bytes) and changes no bit.
    Train-mode BatchNorm raises ValueError."""
    z = _check_grids(z, 1, "z")
    dev = z.device
    export, decoder = _route(decoder_or_export, dev, z.shape[1])
    n = int(z.shape[0] if index is None else index.numel())
    u = u.detach().to(dev, torch.float32).reshape(u.shape[0], -1).contiguous()
    if index is not None:
        index = index.detach().to(dev, torch.int32).reshape(-1).contiguous()
        if n and (int(index.min()) < 0 or int(index.max()) >= z.shape[0]):
            raise ValueError(f"index out of range 0...{z.shape[0]}")
    if u.shape[0] != n:
        raise ValueError(f"u has {u.shape[0]} rows for {n} grids")
    if export is None:
        dec_dev = next(decoder.parameters()).device
        rows = (z if index is None else z[index.long()]).to(dec_dev)
        _, outs = _torch_vjps(decoder, rows, [u.to(dec_dev)]) if n else (None, [torch.zeros_like(rows)])
        return outs[0].double().to(dev)
    if u.shape[1] != export.n_out:
        raise ValueError(f"u must have {export.n_out} values per row, got {u.shape[1]}")
    out = torch.empty(n, export.latent_dim, 4, 4, dtype=torch.float64, device=dev)
    if n:
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws = capped_workspace(lib.geo_spatial_vjp_workspace_bytes(export.desc, n), max_workspace_bytes, dev,
                                  "geo_spatial_vjp_workspace_bytes: decoder")
            _lib.check(lib.geo_spatial_vjp(export.desc, ptr(z), ptr(index), n, ptr(u), ptr(out), ptr(ws), ws.numel(), stream_ptr()),
                       "geo_spatial_vjp")
    return out


def grid_curve_energy_device(decoder_or_export, frames: torch.Tensor, *, probe: bool = False,
                             max_workspace_bytes=None) -> CurveEnergy:
    """Evaluate C curves of grids: frames f32 [C, F, d, 4, 4], 2 <= F <= 64.  energy f64 [C]; seg_sq f64 [C, F-1]; grad f64
    [C, F, d, 4, 4] (0 at the ends); outputs f32 [C, F, C_out S S]; jac None; `trace` carries the probe f64 [C, F] where `probe`
    asks for it, else None.  `max_workspace_bytes` caps the native workspace (not below geo_spatial_curve_min_workspace_bytes) and
    changes no bit.  Train-mode BatchNorm raises ValueError on both routes."""
    x = _check_grids(frames, 2, "frames")
    dev = x.device
    export, decoder = _route(decoder_or_export, dev, x.shape[2])
    C, F = x.shape[:2]
    if export is None:
        dec_dev = next(decoder.parameters()).device
        energy, seg, grad, pr, g = _torch_evaluate(decoder, x.to(dec_dev), probe)
        return CurveEnergy(energy.to(dev), seg.to(dev), grad.to(dev), g.to(dev), None, "torch", None if pr is None else pr.to(dev))
    energy = torch.empty(C, dtype=torch.float64, device=dev)
    seg = torch.empty(C, F - 1, dtype=torch.float64, device=dev)
    grad = torch.empty(x.shape, dtype=torch.float64, device=dev)
    g = torch.empty(C, F, export.n_out, dtype=torch.float32, device=dev)
    pr = torch.empty(C, F, dtype=torch.float64, device=dev) if probe else None
    if C:
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws = capped_workspace(lib.geo_spatial_curve_workspace_bytes(export.desc, C, F), max_workspace_bytes, dev,
                                  "geo_spatial_curve_workspace_bytes: decoder")
            _lib.check(lib.geo_spatial_curve_energy(export.desc, ptr(x), C, F, ptr(energy), ptr(seg), ptr(grad), ptr(g), ptr(pr),
                                                    ptr(ws), ws.numel(), stream_ptr()), "geo_spatial_curve_energy")
    return CurveEnergy(energy, seg, grad, g, None, "native", pr)


def relax_grid_curves_device(decoder_or_export, frames: torch.Tensor, n_iters: int, *, step=None,
                             max_workspace_bytes=None) -> RelaxedCurves:
    """Relax C curves of grids for n_iters trial steps each: frames f32 [C, F, d, 4, 4] (not modified), the end grids fixed.
    `step`: None (the probe rule above), a number, or f64 [C] -- pass a result's `step` to continue where it stopped: n
    iterations in one call are the bits of n calls of one iteration.  energy <= energy0 for every curve; a curve with a NaN or
    an inf comes back unchanged with accepted == 0.  The fields are RelaxedCurves' with frames [C, F, d, 4, 4].  Train-mode
    BatchNorm raises ValueError on both routes."""
    x = _check_grids(frames, 2, "frames")
    n_iters = int(n_iters)
    if n_iters < 0:
        raise ValueError(f"n_iters = {n_iters} < 0")
    dev = x.device
    export, decoder = _route(decoder_or_export, dev, x.shape[2])
    C, F = x.shape[:2]
    if step is None:
        step_t = torch.full((C,), -1.0, dtype=torch.float64, device=dev)
    elif torch.is_tensor(step):
        step_t = step.detach().to(dev, torch.float64).reshape(-1).clone()
        if step_t.numel() != C:
            raise ValueError(f"step has {step_t.numel()} entries for {C} curves")
    else:
        step_t = torch.full((C,), float(step), dtype=torch.float64, device=dev)
    if export is None:
        dec_dev = next(decoder.parameters()).device
        res = _torch_relax(decoder, x.to(dec_dev), n_iters, step_t.to(dec_dev))
        return RelaxedCurves(*(t.to(dev) for t in res), route="torch")
    x = x.clone()
    energy0 = torch.empty(C, dtype=torch.float64, device=dev)
    energy = torch.empty(C, dtype=torch.float64, device=dev)
    seg = torch.empty(C, F - 1, dtype=torch.float64, device=dev)
    accepted = torch.zeros(C, dtype=torch.int32, device=dev)
    if C:
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws = capped_workspace(lib.geo_spatial_curve_workspace_bytes(export.desc, C, F), max_workspace_bytes, dev,
                                  "geo_spatial_curve_workspace_bytes: decoder")
            _lib.check(lib.geo_spatial_curve_relax(export.desc, ptr(x), C, F, n_iters, ptr(step_t), ptr(energy0), ptr(energy),
                                                   ptr(seg), ptr(accepted), ptr(ws), ws.numel(), stream_ptr()),
                       "geo_spatial_curve_relax")
    return RelaxedCurves(x, energy0, energy, seg, step_t, accepted, "native")
