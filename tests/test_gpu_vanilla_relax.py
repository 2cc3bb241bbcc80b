"""Curve energy and relaxation under the vanilla decoder (geo_vanilla_curve_energy / geo_vanilla_curve_relax, DESIGN.md section
27) on the GPU: the evaluation against its numpy restatement and against geo_vanilla_vjp bit for bit, accuracy against the fp64
module with float32 torch as the yardstick, the relax rules on one iteration and on a whole call, a descent at least half as
deep as the same rules over the float32 torch module, invariance, and the Python routes."""
import copy
import functools

import numpy as np
import pytest
import torch

import relax_cases as rc
import vanilla_curve_cases as K
import vanilla_jvp_cases as V

pytestmark = pytest.mark.gpu

CASES = ("wide-bn-28", "wide-bn-32x3", "narrow-none-28", "narrow-none-32x3-d5")
SHAPES = ((3, 5), (3, 9), (1, 3), (7, 5), (2, 2), (1, 64))
ITERS = rc.RELAX_ITERS


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _export(name):
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    return VanillaDecoderExport(K.decoder(name), _dev())


def _lib():
    from vqvae_amd import _lib
    return _lib.load()


def _np(t):
    return None if t is None else t.cpu().numpy()


def _energy(ex, x, fill=None, **kw):
    """(energy, seg_sq, grad, g, trace) as numpy; `fill`: the cached workspace is filled with that byte first."""
    from vqvae_amd._device import workspace
    from vqvae_amd.geo import curve_energy_device
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(_dev())
    if fill is not None:
        workspace(_lib().geo_vanilla_curve_workspace_bytes(ex.desc, x.shape[0], x.shape[1]), _dev()).fill_(fill)
    r = curve_energy_device(ex, xt, **kw)
    assert r.route == "native" and r.jac is None
    return _np(r.energy), _np(r.seg_sq), _np(r.grad), _np(r.outputs), _np(r.trace)


def _relax(ex, x, n_iters, step=None, fill=None, **kw):
    """(frames, energy0, energy, seg_sq, step, accepted) as numpy."""
    from vqvae_amd._device import workspace
    from vqvae_amd.geo import relax_curves_device
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(_dev())
    if fill is not None:
        workspace(_lib().geo_vanilla_curve_workspace_bytes(ex.desc, x.shape[0], x.shape[1]), _dev()).fill_(fill)
    r = relax_curves_device(ex, xt, n_iters, step=None if step is None else torch.from_numpy(np.asarray(step, dtype=np.float64)), **kw)
    assert r.route == "native"
    return tuple(_np(t) for t in (r.frames, r.energy0, r.energy, r.seg_sq, r.step, r.accepted))


def _least(ex, F):
    return _lib().geo_vanilla_curve_min_workspace_bytes(ex.desc, F)


# ------------------------------------------------------------------------------------- the restatement (no code of the project)
def fold_256(sq):
    """The fixed order of a sum over the outputs, [..., nout] -> [...]: lane t of 256 adds entries t, t + 256, ... ascending (from
    the first entry: 0 + a is a), then p[t] += p[t + s] for s = 128, 64, ..., 1."""
    nout = sq.shape[-1]
    pad = (-nout) % 256
    rows = np.concatenate([sq, np.zeros(sq.shape[:-1] + (pad,))], axis=-1).reshape(sq.shape[:-1] + (-1, 256))
    p = rows[..., 0, :].copy()
    for j in range(1, rows.shape[-2]):
        p = p + rows[..., j, :]
    s = 128
    while s >= 1:
        p = p[..., :s] + p[..., s:2 * s]
        s //= 2
    return p[..., 0]


def restate(g, x):
    """(energy [C], seg_sq [C, F-1], r f32 [C, F, nout]) from the float32 outputs g [C, F, nout] and the frames x."""
    g64 = np.asarray(g, dtype=np.float32).astype(np.float64)
    C, F, nout = g64.shape
    with np.errstate(invalid="ignore", over="ignore"):
        ahead = g64[:, 1:] - g64[:, :-1]
        seg = fold_256(ahead * ahead)
        energy = np.zeros(C)
        for f in range(F - 1):
            energy = energy + seg[:, f]
        r = np.zeros((C, F, nout), dtype=np.float32)
        if F > 2:
            r[:, 1:-1] = ((g64[:, 1:-1] - g64[:, :-2]) - (g64[:, 2:] - g64[:, 1:-1])).astype(np.float32)
    energy = np.where(np.isfinite(np.asarray(x)).all(axis=(1, 2)), energy, np.nan)
    return energy, seg, r


def _curves(name, F, C):
    return rc.zigzags(K.spec(name)[1], F, C)


# ------------------------------------------------------------------------------------- 1. evaluate
@pytest.mark.parametrize("C,F", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_evaluate_is_the_restatement_and_the_vjp(name, C, F):
    """energy and seg_sq are the numpy restatement from g_out, grad is 0 at the ends and 2 geo_vanilla_vjp(x[f], (float) r[f])
    inside, all bit for bit; the same bits at the minimum workspace on 0xFF; F = 2: grad 0 and relax a no-op."""
    from vqvae_amd.geo import vanilla_vjp_device
    ex = _export(name)
    x = _curves(name, F, C)
    d = x.shape[2]
    E, seg, grad, g, tr = _energy(ex, x)
    assert tr is None and g.dtype == np.float32 and g.shape == (C, F, ex.n_out) and np.all((g > 0) & (g < 1))
    wE, wseg, r = restate(g, x)
    print(f"{name} C={C} F={F}: E = {E}")
    assert rc.bits(E) == rc.bits(wE) and rc.bits(seg) == rc.bits(wseg)
    assert np.all(grad[:, 0] == 0.0) and np.all(grad[:, -1] == 0.0)
    vjp = vanilla_vjp_device(ex, torch.from_numpy(x.reshape(C * F, d)).to(_dev()), torch.from_numpy(r.reshape(C * F, -1)).to(_dev()))
    want = 2.0 * vjp.cpu().numpy().reshape(C, F, d)
    want[:, 0] = want[:, -1] = 0.0
    assert rc.bits(grad) == rc.bits(want)
    low = _energy(ex, x, fill=0xFF, max_workspace_bytes=_least(ex, F))
    assert all(rc.bits(a) == rc.bits(b) for a, b in zip(low[:4], (E, seg, grad, g)))
    if F == 2:
        assert np.all(grad == 0.0)
        frames, e0, e1, seg1, step, acc = _relax(ex, x, 5)
        assert rc.bits(frames) == rc.bits(x) and np.all(acc == 0) and rc.bits(e0) == rc.bits(E) == rc.bits(e1)
        assert rc.bits(seg1) == rc.bits(seg)
    else:
        assert np.all(np.abs(grad[:, 1:-1]).sum(axis=2) > 0)


# ------------------------------------------------------------------------------------- 2. accuracy against the fp64 module
def _module_eval(dec, x, dtype, dev):
    """(g [C, F, nout], grad [C, F, d]) of the curves x by torch in `dtype` on `dev`: g from the module, r from that g in fp64
    (rounded to `dtype`), grad = 2 VJP by autograd.grad, 0 at the ends."""
    dd = copy.deepcopy(dec).to(dev).to(dtype).eval()
    C, F, d = x.shape
    z = torch.from_numpy(x.reshape(C * F, d)).to(dev).to(dtype).requires_grad_(True)
    g = torch.sigmoid(dd(z)).reshape(C, F, -1)
    g64 = g.detach().double()
    r = torch.zeros_like(g64)
    r[:, 1:-1] = (g64[:, 1:-1] - g64[:, :-2]) - (g64[:, 2:] - g64[:, 1:-1])
    grad = 2.0 * torch.autograd.grad((g * r.to(dtype)).sum(), z)[0].double().reshape(C, F, d)
    grad[:, 0] = 0
    grad[:, -1] = 0
    return g.detach().double().cpu().numpy(), grad.cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_accuracy_against_fp64(name):
    """6 zig-zags of 5 and of 9 frames.  g: largest absolute error at most 4 x float32 torch's.  grad: per interior frame the
    relative 2-norm error against the fp64 module; the median over the frames of the 6 curves at most 4 x float32 torch's median,
    and at most one frame per case above 1e-4 (a ReLU mask that flips in float32: among these curves of narrow-none-28 at F = 9
    float32 torch on a CPU has one such frame, 3.4e-4, and so has the native route on the MI355X)."""
    ex = _export(name)
    above_all = 0
    for F in rc.FRAMES:
        x = _curves(name, F, 6)
        g64, grad64 = _module_eval(K.decoder(name), x, torch.float64, torch.device("cpu"))
        g32, grad32 = _module_eval(K.decoder(name), x, torch.float32, _dev())
        _, _, grad, g, _ = _energy(ex, x)
        e_g, t_g = np.abs(g - g64).max(), np.abs(g32 - g64).max()

        def frame_error(a):
            return (np.linalg.norm(a - grad64, axis=2)[:, 1:-1] / np.linalg.norm(grad64, axis=2)[:, 1:-1]).ravel()
        e, t = frame_error(grad), frame_error(grad32)
        above_all += int((e > 1e-4).sum())
        print(f"{name} F={F}: g e = {e_g:.3e}, e_torch = {t_g:.3e}, ratio {e_g / t_g:.2f}; grad median e = {np.median(e):.3e}, "
              f"median e_torch = {np.median(t):.3e}, ratio {np.median(e) / np.median(t):.2f}; max e = {e.max():.3e}, "
              f"max e_torch = {t.max():.3e}; frames above 1e-4: {int((e > 1e-4).sum())} (torch {int((t > 1e-4).sum())})")
        assert e_g <= 4 * t_g
        assert np.median(e) <= 4 * np.median(t)
    assert above_all <= 1


# ------------------------------------------------------------------------------------- 3. the relaxation
@pytest.mark.parametrize("F", rc.FRAMES)
@pytest.mark.parametrize("name", CASES)
def test_one_iteration_follows_the_rules(name, F):
    """With the step left to the call: trial, decision and new step are relax_cases.trial / decide / step0 applied to the
    evaluation's own energy, grad and trace and to a second evaluation; at the queried workspace and at the minimum on 0xFF."""
    ex = _export(name)
    x = _curves(name, F, 3)
    E, seg, grad, g, tr = _energy(ex, x, trace=True)
    assert tr.shape == (3, F) and np.all(tr > 0)
    assert all(rc.bits(a) == rc.bits(b) for a, b in zip(_energy(ex, x), (E, seg, grad, g)))       # the trace changes nothing else
    low_tr = _energy(ex, x, trace=True, fill=0xFF, max_workspace_bytes=_least(ex, F))[4]
    assert rc.bits(low_tr) == rc.bits(tr)
    step = rc.step0(tr)
    y = rc.trial(x, step, grad)
    Ey, segy, _, _, _ = _energy(ex, y)
    take, new_step = rc.decide(E, Ey, step)
    print(f"{name} F={F}: E = {E}, E_y = {Ey}, step0 = {step}, take {take.astype(int)}")
    want = (np.where(take[:, None, None], y, x), E, np.where(take, Ey, E), np.where(take[:, None], segy, seg), new_step,
            take.astype(np.int32))
    for kw in ({}, {"fill": 0xFF, "max_workspace_bytes": _least(ex, F)}):
        got = _relax(ex, x, 1, **kw)
        assert all(rc.bits(a) == rc.bits(b) for a, b in zip(got, want)), kw
    given = _relax(ex, x, 1, step=step)                                                             # the same step, given
    assert all(rc.bits(a) == rc.bits(b) for a, b in zip(given, want))


def _torch_rules(dec, x, n_iters, step):
    """relax_cases' loop over the float32 torch module on the GPU, gradients by autograd.grad: (energy0, energy, accepted)."""
    dev = _dev()

    def evaluate(frames):
        g, grad = _module_eval(dec, frames, torch.float32, dev)
        E, seg, _ = restate(g.astype(np.float32), frames)
        return E, grad
    x = np.array(x, dtype=np.float32, copy=True)
    E, grad = evaluate(x)
    e0, step, accepted = E.copy(), np.array(step, dtype=np.float64), np.zeros(x.shape[0], dtype=np.int32)
    for _ in range(n_iters):
        y = rc.trial(x, step, grad)
        Ey, grady = evaluate(y)
        take, step = rc.decide(E, Ey, step)
        x[take], grad[take], E[take] = y[take], grady[take], Ey[take]
        accepted += take.astype(np.int32)
    return e0, E, accepted


@pytest.mark.parametrize("F", rc.FRAMES)
@pytest.mark.parametrize("name", CASES)
def test_a_whole_call(name, F):
    """20 iterations in one call are the bits of 20 calls of one; the result's energy and segments are those of Evaluate(result);
    the ends are untouched; energy <= energy0.  And the descent is real: from the common explicit step 1 / (8 max interior
    native trace), the native energy falls at least half as far as under the same rules over the float32 torch module."""
    ex = _export(name)
    x = _curves(name, F, 3)
    step = rc.step0(_energy(ex, x, trace=True)[4])
    frames, e0, e1, seg, st, acc = _relax(ex, x, ITERS, step=step)
    assert np.all(e1 <= e0)
    assert rc.bits(frames[:, 0]) == rc.bits(x[:, 0]) and rc.bits(frames[:, -1]) == rc.bits(x[:, -1])
    E, seg_r, _, _, _ = _energy(ex, frames)
    assert rc.bits(E) == rc.bits(e1) and rc.bits(seg_r) == rc.bits(seg)
    cur, s = x, step
    for _ in range(ITERS):
        cur, _, e_one, seg_one, s, _ = _relax(ex, cur, 1, step=s)
    assert rc.bits(cur) == rc.bits(frames) and rc.bits(s) == rc.bits(st)
    assert rc.bits(e_one) == rc.bits(e1) and rc.bits(seg_one) == rc.bits(seg)
    t0, t1, t_acc = _torch_rules(K.decoder(name), x, ITERS, step)
    print(f"{name} F={F}: native E / E0 = {e1 / e0}, accepted {acc}; float32 torch E / E0 = {t1 / t0}, accepted {t_acc}")
    assert np.all(t1 < t0)                                                                          # the yardstick descends
    assert np.all(e0 - e1 >= 0.5 * (t0 - t1))


@pytest.mark.parametrize("name", ["wide-bn-32x3", "narrow-none-28"])
def test_a_curve_does_not_depend_on_its_company(name):
    """5 curves of 5 frames, 6 iterations, the step left to the call: a curve alone, among the others, permuted, in slices of
    one and of two curves, on a side stream, and beside a NaN curve gives the same bits; the NaN curve comes back unchanged with
    E = NaN and accepted 0."""
    ex = _export(name)
    F, C, n = 5, 5, 6
    x = _curves(name, F, C)
    base = _relax(ex, x, n)
    assert np.all(base[5] >= 1)
    alone = _relax(ex, x[2:3], n)
    assert all(rc.bits(a) == rc.bits(b[2:3]) for a, b in zip(alone, base))
    perm = np.array([3, 0, 4, 2, 1])
    assert all(rc.bits(a) == rc.bits(b[perm]) for a, b in zip(_relax(ex, x[perm], n), base))
    lib = _lib()
    for per_slice in (1, 2):
        cap = lib.geo_vanilla_curve_workspace_bytes(ex.desc, per_slice, F)
        assert cap < lib.geo_vanilla_curve_workspace_bytes(ex.desc, C, F)
        assert all(rc.bits(a) == rc.bits(b) for a, b in zip(_relax(ex, x, n, fill=0xFF, max_workspace_bytes=cap), base)), per_slice
    from vqvae_amd._lib import GeoHipError
    with pytest.raises(GeoHipError):
        _relax(ex, x, n, max_workspace_bytes=_least(ex, F) - 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _relax(ex, x, n)
    side.synchronize()
    assert all(rc.bits(a) == rc.bits(b) for a, b in zip(other, base))
    sick = x.copy()
    sick[1, 2, 0] = np.nan
    got = _relax(ex, sick, n)
    healthy = [0, 2, 3, 4]
    assert all(rc.bits(a[healthy]) == rc.bits(b[healthy]) for a, b in zip(got, base))
    assert rc.bits(got[0][1]) == rc.bits(sick[1]) and np.isnan(got[1][1]) and np.isnan(got[2][1]) and got[5][1] == 0
    sick[1, 2, 0] = np.inf
    got = _relax(ex, sick, n)
    assert rc.bits(got[0][1]) == rc.bits(sick[1]) and np.isnan(got[2][1]) and got[5][1] == 0


# ------------------------------------------------------------------------------------- 4. the Python routes
def test_python_routes():
    """A covered module on the GPU takes the native route with the export's bits, which are those of the raw calls on the
    test's own buffers; jacobian=True keeps a module on the torch route
    and refuses an export; an uncovered decoder keeps the torch route; train-mode BatchNorm raises; the size queries refuse an
    uncovered descriptor and a bad F."""
    from vqvae_amd import _lib
    from vqvae_amd.geo import curve_energy_device, native_relax_covers, native_vanilla_relax_covers, relax_curves_device
    name, F = "narrow-none-28", 5
    ex = _export(name)
    dec = copy.deepcopy(K.decoder(name)).to(_dev())
    assert native_vanilla_relax_covers(dec) and not native_relax_covers(dec)
    x = torch.from_numpy(_curves(name, F, 2)).to(_dev())
    a, b = curve_energy_device(dec, x, trace=True), curve_energy_device(ex, x, trace=True)
    assert a.route == b.route == "native" and a.jac is None and a.trace.dtype == torch.float64
    for f in ("energy", "seg_sq", "grad", "outputs", "trace"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.energy.dtype == a.seg_sq.dtype == a.grad.dtype == torch.float64 and a.outputs.dtype == torch.float32
    # ... and with the raw calls on buffers of the test's own
    from vqvae_amd._device import ptr
    lib = _lib.load()
    raw = {"energy": torch.empty(2, dtype=torch.float64, device=_dev()), "seg_sq": torch.empty(2, F - 1, dtype=torch.float64, device=_dev()),
           "grad": torch.empty(2, F, 16, dtype=torch.float64, device=_dev()), "outputs": torch.empty(2, F, 784, device=_dev()),
           "trace": torch.empty(2, F, dtype=torch.float64, device=_dev())}
    ws = torch.empty(lib.geo_vanilla_curve_workspace_bytes(ex.desc, 2, F), dtype=torch.uint8, device=_dev())
    assert lib.geo_vanilla_curve_energy(ex.desc, ptr(x), 2, F, ptr(raw["energy"]), ptr(raw["seg_sq"]), ptr(raw["grad"]),
                                        ptr(raw["outputs"]), ptr(raw["trace"]), ptr(ws), ws.numel(), None) == 0
    torch.cuda.synchronize()
    for f, t in raw.items():
        assert torch.equal(getattr(a, f), t), f
    xr, step = x.clone(), torch.full((2,), -1.0, dtype=torch.float64, device=_dev())
    e0, e1, acc = torch.empty_like(raw["energy"]), torch.empty_like(raw["energy"]), torch.zeros(2, dtype=torch.int32, device=_dev())
    assert lib.geo_vanilla_curve_relax(ex.desc, ptr(xr), 2, F, 3, ptr(step), ptr(e0), ptr(e1), ptr(raw["seg_sq"]), ptr(acc), ptr(ws),
                                       ws.numel(), None) == 0
    torch.cuda.synchronize()
    ra, rb = relax_curves_device(dec, x, 3), relax_curves_device(ex, x, 3)
    for f, t in (("frames", xr), ("energy0", e0), ("energy", e1), ("seg_sq", raw["seg_sq"]), ("step", step), ("accepted", acc)):
        assert torch.equal(getattr(ra, f), t), f
    assert ra.route == rb.route == "native" and ra.accepted.dtype == torch.int32 and ra.frames.dtype == torch.float32
    for f in ("frames", "energy0", "energy", "seg_sq", "step", "accepted"):
        assert torch.equal(getattr(ra, f), getattr(rb, f)), f
    with_jac = curve_energy_device(dec, x, jacobian=True)
    assert with_jac.route == "torch" and with_jac.jac.shape == (2, F, 16, 784) and with_jac.trace is None
    with pytest.raises(ValueError, match="Jacobian"):
        curve_energy_device(ex, x, jacobian=True)
    group = V.make_decoder((128, 64, 32), 16, 1, 28, "group").to(_dev())
    assert not native_vanilla_relax_covers(group) and curve_energy_device(group, x[:1, :3]).route == "torch"
    train = V.make_decoder((128, 64, 32), 16, 1, 28, "batch", eval_mode=False).to(_dev())
    with pytest.raises(ValueError, match="train-mode BatchNorm"):
        relax_curves_device(train, x, 1)
    with pytest.raises(ValueError):
        curve_energy_device(ex, x[:, :, :7])
    lib = _lib.load()
    bad = _lib.VanillaDecoderDesc.from_buffer_copy(ex.desc)
    bad.c1, bad.c2 = 32, 16
    assert lib.geo_vanilla_curve_workspace_bytes(bad, 3, F) == 0 and lib.geo_vanilla_curve_min_workspace_bytes(bad, F) == 0
    assert lib.geo_vanilla_curve_workspace_bytes(ex.desc, 3, 1) == 0 and lib.geo_vanilla_curve_workspace_bytes(ex.desc, 3, 65) == 0
    from vqvae_amd._device import ptr
    energy = torch.full((2,), 7.0, dtype=torch.float64, device=_dev())
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=_dev())
    assert lib.geo_vanilla_curve_energy(bad, ptr(x), 2, F, ptr(energy), None, None, None, None, ptr(ws), ws.numel(), None) == -1
    torch.cuda.synchronize()
    assert bool((energy == 7.0).all())


# ------------------------------------------------------------------------------------- 5. interpolation on a legacy build
def test_interpolation_cli_on_a_legacy_riemannian_build(tmp_path):
    """300 latents under the narrow-none-28 decoder, built by build_riemannian_codebook_legacy in the test: the CLI's artefacts
    are interpolate_images_vanilla's fields (with h w = 1), --relax_iters 3 adds the relaxed fields, and the relaxed energy is
    at most that of either start."""
    import json
    import os
    from scipy import sparse
    from vqvae_amd._device import DeviceCSR
    from vqvae_amd.geo import interpolate_images_vanilla
    from vqvae_amd.scripts.geodesic_interpolation import main, make_parser
    from vqvae_amd.training.build_riemannian_codebook_legacy import build_and_save
    tmp = str(tmp_path)
    dec = K.decoder("narrow-none-28")
    torch.save({"model_state_dict": {"decoder." + k: v for k, v in dec.state_dict().items()}, "epoch": 0}, os.path.join(tmp, "best.pt"))
    z = torch.randn(300, 16, generator=torch.Generator().manual_seed(22))
    torch.save(z, os.path.join(tmp, "z.pt"))
    vae = dict(in_channels=1, enc_channels=[32, 64, 128], dec_channels=[128, 64, 32], latent_dim=16, recon_loss="bce",
               output_image_size=28, norm_type="none", mse_use_sigmoid=True)
    config = {"data": {"latents_path": os.path.join(tmp, "z.pt")}, "checkpoint_path": os.path.join(tmp, "best.pt"),
              "vae_config": vae, "graph": {"k": 10, "metric": "euclidean", "sym": "union", "mode": "distance"},
              "riemannian": {"mode": "full", "max_edges": 1000, "batch_size": 256},
              "quantize": {"K": 8, "init": "kpp", "seed": 42}, "out": {"dir": os.path.join(tmp, "build")}}
    cb_dir = build_and_save(config)
    codes = np.load(cb_dir / "codes.npy")
    rows = np.flatnonzero(codes >= 0)
    assert rows.size >= 250
    pairs = [(int(rows[0]), int(rows[40])), (int(rows[7]), int(rows[-1])), (int(rows[100]), int(rows[3]))]
    out_dir = os.path.join(tmp, "interp")
    got = main(make_parser().parse_args(["--codebook_dir", str(cb_dir), "--out_dir", out_dir, "--frames", "7", "--relax_iters", "3",
                                         "--pairs"] + [f"{i}:{j}" for i, j in pairs]))
    W = sparse.load_npz(cb_dir / "knn_graph_riemannian.npz").tocsr()
    want = interpolate_images_vanilla(z, rows, DeviceCSR.from_scipy(W, _dev()), copy.deepcopy(dec).to(_dev()), pairs, 7, "other", True,
                                      relax_iters=3)
    saved = np.load(os.path.join(out_dir, "interpolation.npz"))
    assert os.path.getsize(os.path.join(out_dir, "interpolation.png")) > 0
    relaxed = ("frames_relaxed", "images_relaxed", "curve_len_relaxed", "image_len_relaxed", "relax_from", "accepted_geo",
               "accepted_lin", "energy_geo", "energy_lin", "energy_relaxed")
    for k in ("frames_lin", "frames_geo", "images_lin", "images_geo", "graph_dist", "hops", "status", "curve_len_lin",
              "curve_len_geo", "image_len_lin", "image_len_geo") + relaxed:
        w = want[k].cpu().numpy()
        if k.startswith("frames_"):
            w = w.reshape(w.shape + (1, 1))
        elif w.ndim == 1 and not k.startswith(("curve_len_", "image_len_")):
            w = w.reshape(-1, 1)
        assert saved[k].dtype == w.dtype and np.array_equal(saved[k], w), k
        assert np.array_equal(got[k].cpu().numpy(), w), k
    assert saved["frames_geo"].shape == (3, 7, 16, 1, 1) and saved["images_geo"].shape == (3, 7, 1, 28, 28)
    assert np.array_equal(saved["pairs"], np.asarray(pairs)) and np.all(saved["status"] == 0)
    assert np.all(saved["energy_relaxed"] <= np.minimum(saved["energy_geo"], saved["energy_lin"]))
    summary = json.load(open(os.path.join(out_dir, "interpolation.json")))
    assert summary["relax_iters"] == 3 and len(summary["pairs"]) == 3 and summary["apply_sigmoid"] is True
    print(f"energy geo {saved['energy_geo'].ravel()}, chord {saved['energy_lin'].ravel()}, relaxed {saved['energy_relaxed'].ravel()}, "
          f"accepted {saved['accepted_geo'].ravel()} / {saved['accepted_lin'].ravel()}")
    plain = main(make_parser().parse_args(["--codebook_dir", str(cb_dir), "--out_dir", os.path.join(tmp, "plain"), "--frames", "7",
                                           "--pairs", "0:1"]))
    assert "frames_relaxed" not in plain and "frames_relaxed" not in np.load(os.path.join(tmp, "plain", "interpolation.npz")).files
