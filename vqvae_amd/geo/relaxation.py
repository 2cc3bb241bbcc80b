"""Curves under the pull-back metric: their discrete energy and its monotone relaxation with fixed ends (an extension: the
reference has no counterpart).

A curve is F frames x[0..F-1] in latent space.  With g(z) = sigmoid(decoder(z)) on a 1x1 latent and J its Jacobian,
    seg_sq[f] = |g(x[f+1]) - g(x[f])|^2,   E = sum_f seg_sq[f],   grad[f] = 2 J(x[f])^T ((g[f] - g[f-1]) - (g[f+1] - g[f])),
every sum one fp64 accumulator over ascending indices; a curve with a NaN or an inf among its coordinates has E = NaN.
relax_curves_device takes n_iters trial steps y = x - step * grad per curve, keeps a trial only where its energy is lower
(step *= 2, else step /= 4) and never moves the ends: E can only fall.

Covered decoders (native_relax_covers) with frames on a GPU run geo_curve_energy / geo_curve_relax (csrc/jvp.hip); covered
vanilla decoders (native_vanilla_relax_covers; g the flattened image) run geo_vanilla_curve_energy / geo_vanilla_curve_relax
(csrc/vanilla_jvp.hip), whose gradient is one vector-Jacobian product per frame and whose sums over the
outputs follow the fixed order written down there; every other decoder, and the CPU, takes the torch route with the same rules:
g from the float32 eval module, J by torch.autograd.functional.jacobian in float32, the reductions in fp64 by explicit ascending
loops.
"""
from dataclasses import dataclass

import torch

from .. import _lib
from .._device import ptr, stream_ptr
from .._export import capped_workspace, eval_mode
from ..spatial_decoder import DecoderExport
from ..vanilla_decoder import VanillaDecoderExport, vanilla_kernels_cover
from .riemannian_metric import _has_train_batchnorm, native_metric_covers

MAX_FRAMES = 64
_BN_ERROR = ("curve energy under a train-mode BatchNorm decoder: a sample's Jacobian depends on its batch; put the decoder "
             "in eval()")


@dataclass
class CurveEnergy:
    """energy f64 [C]; seg_sq f64 [C, F-1]; grad f64 [C, F, d] (0 at the ends); outputs f32 [C, F, p_out] (the sigmoids g);
    jac f32 [C, F, d, p_out] or None; route "native" or "torch"; trace f64 [C, F] (tr J^T J per frame) where the call was asked
    for it on the native vanilla route, else None.  grid_relaxation's calls return it with frames of grids ([C, F, d, 4, 4] for
    grad) and their sign probe in `trace`."""
    energy: object
    seg_sq: object
    grad: object
    outputs: object
    jac: object
    route: str
    trace: object = None


@dataclass
class RelaxedCurves:
    """frames f32 [C, F, d]; energy0, energy f64 [C] (before, after); seg_sq f64 [C, F-1] of the result; step f64 [C] (the state to
    continue from); accepted i32 [C]; route "native" or "torch"."""
    frames: object
    energy0: object
    energy: object
    seg_sq: object
    step: object
    accepted: object
    route: str


def native_relax_covers(decoder) -> bool:
    """Whether geo_curve_energy / geo_curve_relax take this decoder: exactly native_metric_covers (same passes)."""
    return native_metric_covers(decoder)


def native_vanilla_relax_covers(decoder) -> bool:
    """Whether geo_vanilla_curve_energy / geo_vanilla_curve_relax take this decoder: exactly vanilla_kernels_cover."""
    return vanilla_kernels_cover(decoder)


def _check_frames(frames: torch.Tensor) -> torch.Tensor:
    if frames.ndim != 3:
        raise ValueError(f"frames must be [C, F, d], got {tuple(frames.shape)}")
    if not 2 <= frames.shape[1] <= MAX_FRAMES:
        raise ValueError(f"F = {frames.shape[1]} frames, must be in [2, {MAX_FRAMES}]")
    return frames.detach().to(torch.float32).contiguous()


def _route(decoder_or_export, frames: torch.Tensor, jacobian: bool = False):
    """(export or None, decoder or None): the native route's export (a DecoderExport, or a VanillaDecoderExport, whose route
    computes no Jacobian), or the module of the torch route."""
    if isinstance(decoder_or_export, VanillaDecoderExport):
        if jacobian:
            raise ValueError("jacobian=True with a VanillaDecoderExport: the native vanilla route computes vector-Jacobian "
                             "products, not the d x p_out Jacobian of a frame; pass the module for the torch route")
        if frames.shape[2] != decoder_or_export.latent_dim:
            raise ValueError(f"frames have {frames.shape[2]} latent dimensions, the decoder {decoder_or_export.latent_dim}")
        if frames.device.type != "cuda":
            raise ValueError("a VanillaDecoderExport runs the native route only: the frames must be on its GPU")
        return decoder_or_export, None
    if isinstance(decoder_or_export, DecoderExport):
        if decoder_or_export.desc.norm == 1 and decoder_or_export.desc.bn_train:
            raise ValueError(_BN_ERROR)
        return decoder_or_export, None
    decoder = decoder_or_export
    if _has_train_batchnorm(decoder):
        raise ValueError(_BN_ERROR)
    if native_relax_covers(decoder) and frames.device.type == "cuda":
        if frames.shape[2] != decoder.conv_in.in_channels:
            raise ValueError(f"frames have {frames.shape[2]} latent dimensions, the decoder {decoder.conv_in.in_channels}")
        return DecoderExport(decoder, frames.device), None
    if native_vanilla_relax_covers(decoder) and frames.device.type == "cuda" and not jacobian:
        if frames.shape[2] != decoder.fc.in_features:
            raise ValueError(f"frames have {frames.shape[2]} latent dimensions, the decoder {decoder.fc.in_features}")
        return VanillaDecoderExport(decoder, frames.device), None
    return None, decoder


# ------------------------------------------------------------------------------------------------------------ torch route
def _torch_outputs_jac(decoder, x: torch.Tensor):
    """g f32 [C, F, p_out] and J f32 [C, F, d, p_out] of frames x [C, F, d] (on the decoder's device)."""
    C, F, d = x.shape
    flat_input = hasattr(next(decoder.children()), "in_features")

    def images(latents):                                 # [n, d] -> [n, p_out]
        z = latents if flat_input else latents.view(latents.shape[0], -1, 1, 1)
        return torch.sigmoid(decoder(z)).reshape(latents.shape[0], -1)

    # With fixed statistics a latent's image depends on its own row alone, so the Jacobian of the images summed over the
    # batch, with respect to the whole batch, holds every latent's own Jacobian: [p_out, n, d] from one call.
    J = []
    with eval_mode(decoder):
        with torch.no_grad():
            g = images(x.reshape(C * F, d)).reshape(C, F, -1).to(torch.float32)
        strategy = "forward-mode" if F * d < g.shape[2] else "reverse-mode"      # the fewer passes
        for c in range(C):                               # a curve at a time: a curve's J does not depend on its neighbours
            J.append(torch.autograd.functional.jacobian(lambda rows: images(rows).sum(0), x[c], vectorize=True,
                                                        strategy=strategy))
    J = torch.stack(J).detach().to(torch.float32)                                  # [C, p_out, F, d]
    return g, J.permute(0, 2, 3, 1).contiguous()


def curve_reductions(g: torch.Tensor, jac: torch.Tensor):
    """(energy [C], seg_sq [C, F-1], grad [C, F, d], tr [C, F]) in fp64 from g f32 [C, F, p] and jac f32 [C, F, d, p], by the
    rules of curve_reduce_kernel: one accumulator per sum, ascending, product and sum separate operations."""
    C, F, p = g.shape
    d = jac.shape[2]
    gd, Jd = g.double(), jac.double()
    dseg = gd[:, 1:] - gd[:, :-1]
    seg = torch.zeros(C, F - 1, dtype=torch.float64, device=g.device)
    for o in range(p):
        seg = seg + dseg[:, :, o] * dseg[:, :, o]
    energy = torch.zeros(C, dtype=torch.float64, device=g.device)
    for f in range(F - 1):
        energy = energy + seg[:, f]
    grad = torch.zeros(C, F, d, dtype=torch.float64, device=g.device)
    if F > 2:
        r = (gd[:, 1:-1] - gd[:, :-2]) - (gd[:, 2:] - gd[:, 1:-1])
        s = torch.zeros(C, F - 2, d, dtype=torch.float64, device=g.device)
        for o in range(p):
            s = s + Jd[:, 1:-1, :, o] * r[:, :, None, o]
        grad[:, 1:-1] = 2.0 * s
    row = torch.zeros(C, F, d, dtype=torch.float64, device=g.device)
    for o in range(p):
        row = row + Jd[:, :, :, o] * Jd[:, :, :, o]
    tr = torch.zeros(C, F, dtype=torch.float64, device=g.device)
    for k in range(d):
        tr = tr + row[:, :, k]
    return energy, seg, grad, tr


def _torch_evaluate(decoder, x: torch.Tensor):
    """Evaluate(x) on the torch route: (energy, seg_sq, grad, tr, g, jac); energy = NaN for a curve with a NaN or an inf among
    its coordinates, as on the native route."""
    g, jac = _torch_outputs_jac(decoder, x)
    energy, seg, grad, tr = curve_reductions(g, jac)
    finite = torch.isfinite(x).all(dim=2).all(dim=1)
    return torch.where(finite, energy, torch.full_like(energy, float("nan"))), seg, grad, tr, g, jac


def initial_step(tr: torch.Tensor) -> torch.Tensor:
    """1 / (8 * max over interior f of tr[f]) per curve, 0 where that maximum is 0; the maximum ignores a NaN."""
    m = torch.zeros(tr.shape[0], dtype=torch.float64, device=tr.device)
    for f in range(1, tr.shape[1] - 1):
        m = torch.where(tr[:, f] > m, tr[:, f], m)
    return torch.where(m > 0, 1.0 / (8.0 * m), torch.zeros_like(m))


def trial_frames(x: torch.Tensor, step: torch.Tensor, grad: torch.Tensor) -> torch.Tensor:
    """y[f] = (float)((double)x[f] - step * grad[f]) for interior f; the ends are copied."""
    y = x.clone()
    if x.shape[1] > 2:
        y[:, 1:-1] = (x[:, 1:-1].double() - step[:, None, None] * grad[:, 1:-1]).to(torch.float32)
    return y


def _torch_relax(decoder, x: torch.Tensor, n_iters: int, step: torch.Tensor):
    E, seg, grad, tr, _, _ = _torch_evaluate(decoder, x)
    energy0 = E.clone()
    step = torch.where(step < 0, initial_step(tr), step)
    accepted = torch.zeros(x.shape[0], dtype=torch.int32, device=x.device)
    for _ in range(n_iters if x.shape[1] > 2 else 0):
        y = trial_frames(x, step, grad)
        Ey, segy, grady, _, _, _ = _torch_evaluate(decoder, y)
        take = Ey < E                                   # (False for a NaN on either side)
        x = torch.where(take[:, None, None], y, x)
        grad = torch.where(take[:, None, None], grady, grad)
        seg = torch.where(take[:, None], segy, seg)
        E = torch.where(take, Ey, E)
        step = torch.where(take, 2.0 * step, step / 4.0)
        accepted = accepted + take.to(torch.int32)
    return x, energy0, E, seg, step, accepted


# ------------------------------------------------------------------------------------------------------------ public
def _vanilla_energy(export, x, trace, max_workspace_bytes) -> CurveEnergy:
    lib = _lib.load()
    C, F, d = x.shape
    dev = x.device
    energy = torch.empty(C, dtype=torch.float64, device=dev)
    seg = torch.empty(C, F - 1, dtype=torch.float64, device=dev)
    grad = torch.empty(C, F, d, dtype=torch.float64, device=dev)
    g = torch.empty(C, F, export.n_out, dtype=torch.float32, device=dev)
    tr = torch.empty(C, F, dtype=torch.float64, device=dev) if trace else None
    if C:
        with torch.cuda.device(dev):
            ws = capped_workspace(lib.geo_vanilla_curve_workspace_bytes(export.desc, C, F), max_workspace_bytes, dev,
                                  "geo_vanilla_curve_workspace_bytes: decoder")
            _lib.check(lib.geo_vanilla_curve_energy(export.desc, ptr(x), C, F, ptr(energy), ptr(seg), ptr(grad), ptr(g), ptr(tr),
                                                    ptr(ws), ws.numel(), stream_ptr()), "geo_vanilla_curve_energy")
    return CurveEnergy(energy, seg, grad, g, None, "native", tr)


def curve_energy_device(decoder_or_export, frames: torch.Tensor, *, jacobian: bool = False, trace: bool = False,
                        max_workspace_bytes=None) -> CurveEnergy:
    """Evaluate C curves: frames f32 [C, F, d], 2 <= F <= 64.  The tensors live on frames' device.  `jacobian` also returns the
    float32 Jacobians the sums were taken over (a covered vanilla module then takes the torch route, a VanillaDecoderExport
    raises ValueError: that route computes no Jacobian); `trace` asks the native vanilla route for tr J^T J per frame (other
    routes leave it None); `max_workspace_bytes` caps the native route's workspace (not below geo_curve_min_workspace_bytes /
    geo_vanilla_curve_min_workspace_bytes) and changes no bit.  Train-mode BatchNorm raises ValueError on both routes."""
    x = _check_frames(frames)
    export, decoder = _route(decoder_or_export, x, jacobian)
    C, F, d = x.shape
    dev = x.device
    if isinstance(export, VanillaDecoderExport):
        return _vanilla_energy(export, x, trace, max_workspace_bytes)
    if export is None:
        dec_dev = next(decoder.parameters()).device
        energy, seg, grad, _, g, jac = _torch_evaluate(decoder, x.to(dec_dev))
        return CurveEnergy(energy.to(dev), seg.to(dev), grad.to(dev), g.to(dev), jac.to(dev) if jacobian else None, "torch")
    lib = _lib.load()
    s_out = 4 if export.desc.out_size == 28 else 8
    p_out = export.desc.out_channels * s_out * s_out
    energy = torch.empty(C, dtype=torch.float64, device=dev)
    seg = torch.empty(C, F - 1, dtype=torch.float64, device=dev)
    grad = torch.empty(C, F, d, dtype=torch.float64, device=dev)
    g = torch.empty(C, F, p_out, dtype=torch.float32, device=dev)
    jac = torch.empty(C, F, d, p_out, dtype=torch.float32, device=dev) if jacobian else None
    if C:
        with torch.cuda.device(dev):
            ws = capped_workspace(lib.geo_curve_workspace_bytes(export.desc, C, F), max_workspace_bytes, dev,
                                  "geo_curve_workspace_bytes: decoder")
            _lib.check(lib.geo_curve_energy(export.desc, ptr(x), C, F, ptr(energy), ptr(seg), ptr(grad), ptr(g), ptr(jac), ptr(ws),
                                            ws.numel(), stream_ptr()), "geo_curve_energy")
    return CurveEnergy(energy, seg, grad, g, jac, "native")


def relax_curves_device(decoder_or_export, frames: torch.Tensor, n_iters: int, *, step=None,
                        max_workspace_bytes=None) -> RelaxedCurves:
    """Relax C curves for n_iters trial steps each: frames f32 [C, F, d] (not modified), the ends fixed.  `step`: None (the rule
    1 / (8 * max tr J^T J over the interior frames)), a number, or f64 [C] -- pass a result's `step` to continue where it stopped:
    n iterations in one call are the bits of n calls of one iteration.  energy <= energy0 for every curve; a curve with a NaN
    comes back unchanged with accepted == 0.  Train-mode BatchNorm raises ValueError on both routes."""
    x = _check_frames(frames)
    n_iters = int(n_iters)
    if n_iters < 0:
        raise ValueError(f"n_iters = {n_iters} < 0")
    export, decoder = _route(decoder_or_export, x)
    C, F, d = x.shape
    dev = x.device
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
    lib = _lib.load()
    x = x.clone()
    energy0 = torch.empty(C, dtype=torch.float64, device=dev)
    energy = torch.empty(C, dtype=torch.float64, device=dev)
    seg = torch.empty(C, F - 1, dtype=torch.float64, device=dev)
    accepted = torch.zeros(C, dtype=torch.int32, device=dev)
    if C and isinstance(export, VanillaDecoderExport):
        with torch.cuda.device(dev):
            ws = capped_workspace(lib.geo_vanilla_curve_workspace_bytes(export.desc, C, F), max_workspace_bytes, dev,
                                  "geo_vanilla_curve_workspace_bytes: decoder")
            _lib.check(lib.geo_vanilla_curve_relax(export.desc, ptr(x), C, F, n_iters, ptr(step_t), ptr(energy0), ptr(energy),
                                                   ptr(seg), ptr(accepted), ptr(ws), ws.numel(), stream_ptr()),
                       "geo_vanilla_curve_relax")
    elif C:
        with torch.cuda.device(dev):
            ws = capped_workspace(lib.geo_curve_workspace_bytes(export.desc, C, F), max_workspace_bytes, dev,
                                  "geo_curve_workspace_bytes: decoder")
            _lib.check(lib.geo_curve_relax(export.desc, ptr(x), C, F, n_iters, ptr(step_t), ptr(energy0), ptr(energy), ptr(seg),
                                           ptr(accepted), ptr(ws), ws.numel(), stream_ptr()), "geo_curve_relax")
    return RelaxedCurves(x, energy0, energy, seg, step_t, accepted, "native")
