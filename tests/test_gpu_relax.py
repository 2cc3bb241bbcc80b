"""geo_curve_energy / geo_curve_relax (csrc/jvp.hip: the per-node primal pass, the column pass, curve_reduce_kernel,
curve_step_kernel) and vqvae_amd.geo.relaxation on the GPU, against the numpy restatement of tests/relax_cases.py computed from
the call's own g_out and jac_out (bit for bit), against the fp64 module (accuracy, float32 torch's own error as the yardstick,
gate 4 x), and against themselves (batch, position, workspace size and contents, stream: the same bits).  Every test prints the
figures it asserts on.

Measured on the MI355X (the accuracy ratios e / e_torch, worst over F in {5, 9}; the relaxation's worst energy / energy0 and
fewest accepts of 20): see DESIGN.md section 26."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

import relax_cases as rc
import ws_guard
from relax_cases import CASES, FRAMES, NATIVE, RELAX_ITERS

pytestmark = pytest.mark.gpu

GEO_E_ARG = -1
SHAPES = ((3, 5), (3, 9), (1, 3), (7, 5))        # (C, F); 7 x 5 = 35 latents: past the 32-sample tile


def _dev():
    from vqvae_amd._device import device
    return device()


@functools.lru_cache(maxsize=None)
def _export(name, training=False):
    from vqvae_amd.spatial_decoder import DecoderExport
    return DecoderExport(rc.make_decoder(name, training)[0].to(_dev()), _dev())


def _lib():
    from vqvae_amd import _lib
    return _lib.load()


def _ws(nbytes, fill):
    ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=_dev())
    if fill is not None:
        ws.fill_(fill)
    return ws


def _raw_energy(ex, x, *, ws_bytes=None, fill=None, jac=True):
    """geo_curve_energy on a workspace of the test's own: (status, energy, seg_sq, grad, g, jac) as numpy arrays."""
    from vqvae_amd._device import ptr, stream_ptr
    lib = _lib()
    x = torch.as_tensor(x).to(_dev()).contiguous()
    C, F, d = x.shape
    p = ex.desc.out_channels * (16 if ex.desc.out_size == 28 else 64)
    if ws_bytes is None:
        ws_bytes = lib.geo_curve_workspace_bytes(ex.desc, C, F)
    ws = _ws(ws_bytes, fill)
    nan = float("nan")
    E = torch.full((C,), nan, dtype=torch.float64, device=_dev())
    seg = torch.full((C, F - 1), nan, dtype=torch.float64, device=_dev())
    grad = torch.full((C, F, d), nan, dtype=torch.float64, device=_dev())
    g = torch.full((C, F, p), nan, dtype=torch.float32, device=_dev())
    J = torch.full((C, F, d, p), nan, dtype=torch.float32, device=_dev()) if jac else None
    with torch.cuda.device(_dev()):
        status = lib.geo_curve_energy(ex.desc, ptr(x), C, F, ptr(E), ptr(seg), ptr(grad), ptr(g), ptr(J), ptr(ws), int(ws_bytes),
                                      stream_ptr())
        torch.cuda.current_stream().synchronize()
    return (status,) + tuple(None if t is None else t.cpu().numpy() for t in (E, seg, grad, g, J))


def _raw_relax(ex, x, n_iters, *, step=None, ws_bytes=None, fill=None):
    """geo_curve_relax: (status, frames, energy0, energy, seg_sq, step, accepted) as numpy arrays."""
    from vqvae_amd._device import ptr, stream_ptr
    lib = _lib()
    x = torch.as_tensor(x).to(_dev()).contiguous().clone()
    C, F, d = x.shape
    if ws_bytes is None:
        ws_bytes = lib.geo_curve_workspace_bytes(ex.desc, C, F)
    ws = _ws(ws_bytes, fill)
    nan = float("nan")
    st = torch.full((C,), -1.0, dtype=torch.float64, device=_dev()) if step is None else torch.as_tensor(step).to(_dev()).clone()
    e0 = torch.full((C,), nan, dtype=torch.float64, device=_dev())
    e1 = torch.full((C,), nan, dtype=torch.float64, device=_dev())
    seg = torch.full((C, F - 1), nan, dtype=torch.float64, device=_dev())
    acc = torch.full((C,), -7, dtype=torch.int32, device=_dev())
    with torch.cuda.device(_dev()):
        status = lib.geo_curve_relax(ex.desc, ptr(x), C, F, n_iters, ptr(st), ptr(e0), ptr(e1), ptr(seg), ptr(acc), ptr(ws),
                                     int(ws_bytes), stream_ptr())
        torch.cuda.current_stream().synchronize()
    return (status,) + tuple(t.cpu().numpy() for t in (x, e0, e1, seg, st, acc))


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert rc.bits(x) == rc.bits(y)
        else:
            assert x == y


def _curves(name, C, F):
    return rc.zigzags(CASES[name][1], F, C)


# ------------------------------------------------------------------------------------- 1. batch shapes, bit for bit
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"C{s[0]}F{s[1]}")
@pytest.mark.parametrize("name", NATIVE)
def test_evaluate_and_step_rule_equal_restatement(name, shape):
    from vqvae_amd._device import ptr, stream_ptr
    lib = _lib()
    ex = _export(name)
    C, F = shape
    d = CASES[name][1]
    x = _curves(name, C, F)
    status, E, seg, grad, g, J = _raw_energy(ex, x)
    assert status == 0, lib.geo_last_error()
    assert g.shape == (C, F, rc.p_out_of(name)) and not np.isnan(g).any() and not np.isnan(J).any()
    wE, wseg, wgrad, wtr = rc.evaluate(g, J)
    assert rc.bits(E) == rc.bits(wE) and rc.bits(seg) == rc.bits(wseg) and rc.bits(grad) == rc.bits(wgrad)
    assert np.all(grad[:, 0] == 0) and np.all(grad[:, -1] == 0) and np.all(E > 0)
    # G restated from jac_out (exact products, ascending sum) is geo_decoder_metric_tensor at the same latents
    J64 = J.astype(np.float64).reshape(C * F, d, -1)
    G = np.zeros((C * F, d, d))
    for o in range(J64.shape[2]):
        G = G + J64[:, :, None, o] * J64[:, None, :, o]
    z = torch.from_numpy(x.reshape(C * F, d)).to(_dev())
    Gm = torch.full((C * F, d, d), float("nan"), dtype=torch.float64, device=_dev())
    nb = lib.geo_metric_tensor_workspace_bytes(ex.desc, C * F)
    ws = _ws(nb, None)
    with torch.cuda.device(_dev()):
        assert lib.geo_decoder_metric_tensor(ex.desc, ptr(z), C * F, ptr(Gm), None, None, None, ptr(ws), nb, stream_ptr()) == 0
    assert rc.bits(Gm.cpu().numpy()) == rc.bits(G)
    # one iteration: the trial, the decision and the step are the restated ones, at the queried and the minimum workspace
    y = rc.trial(x, rc.step0(wtr), wgrad)
    sy, Ey, segy, _, _, _ = _raw_energy(ex, y, jac=False)
    assert sy == 0
    take, step1 = rc.decide(wE, Ey, rc.step0(wtr))
    one = _raw_relax(ex, x, 1)
    assert one[0] == 0, lib.geo_last_error()
    want = (0, np.where(take[:, None, None], y, x), wE, np.where(take, Ey, wE), np.where(take[:, None], segy, wseg), step1,
            take.astype(np.int32))
    _same(one, want)
    ws_min = lib.geo_curve_min_workspace_bytes(ex.desc, F)
    assert 0 < ws_min <= lib.geo_curve_workspace_bytes(ex.desc, C, F)
    assert (ws_min < lib.geo_curve_workspace_bytes(ex.desc, C, F)) == (C > 1)
    _same(_raw_relax(ex, x, 1, ws_bytes=ws_min, fill=0xFF), want)
    _same(_raw_energy(ex, x, ws_bytes=ws_min, fill=0xFF), (0, E, seg, grad, g, J))
    print(f"{name} C={C} F={F}: E = {E}, step0 = {rc.step0(wtr)}, accepted {take.astype(int)}")


# ------------------------------------------------------------------------------------- 2. accuracy against the fp64 module
@functools.lru_cache(maxsize=None)
def _fp64(name, F):
    """(g64 [F, p], J64 [F, p, d], grad64 [F, d], scale [F, d]) of the zig-zag of (case, F), by autograd on the CPU in fp64."""
    dec64 = copy.deepcopy(rc.make_decoder(name)[0]).double().eval()
    x = torch.from_numpy(rc.zigzag(CASES[name][1], F)).double()

    def image(latent):
        return torch.sigmoid(dec64(latent.view(1, -1, 1, 1))).reshape(-1)

    g64 = torch.stack([image(r) for r in x]).detach().numpy()
    J64 = torch.stack([torch.autograd.functional.jacobian(image, r, vectorize=True) for r in x]).numpy()
    return (g64, J64) + _grad_of(g64, J64)


def _grad_of(g, J):
    """grad [F, d] = 2 J^T ((g[f] - g[f-1]) - (g[f+1] - g[f])) in fp64 and its scale sqrt(G_kk) |r| (interior rows)."""
    g, J = np.asarray(g, dtype=np.float64), np.asarray(J, dtype=np.float64)
    r = np.zeros_like(g)
    r[1:-1] = (g[1:-1] - g[:-2]) - (g[2:] - g[1:-1])
    grad = 2.0 * np.einsum("fok,fo->fk", J, r)
    scale = np.sqrt(np.einsum("fok,fok->fk", J, J)) * np.linalg.norm(r, axis=1)[:, None]
    return grad, scale


@pytest.mark.parametrize("name", NATIVE)
def test_accuracy_against_fp64(name):
    """Measured on the MI355X (ratio of the native error to float32 torch's, g / grad): DESIGN.md section 26."""
    dec = rc.make_decoder(name)[0].to(_dev())

    def image(latent):
        return torch.sigmoid(dec(latent.view(1, -1, 1, 1))).reshape(-1)

    for F in FRAMES:
        g64, J64, grad64, scale = _fp64(name, F)
        x = rc.zigzag(CASES[name][1], F)[None]
        status, _, _, grad, g, _ = _raw_energy(_export(name), x)
        assert status == 0
        xg = torch.from_numpy(x[0]).to(_dev())
        with torch.no_grad():
            g32 = torch.stack([image(r) for r in xg]).cpu().numpy()
            J32 = torch.func.vmap(torch.func.jacfwd(image))(xg).cpu().numpy()
        grad32, _ = _grad_of(g32, J32)
        inner = slice(1, F - 1)
        e_g, t_g = np.abs(g[0] - g64).max(), np.abs(g32 - g64).max()
        e_grad = (np.abs(grad[0] - grad64)[inner] / scale[inner]).max()
        t_grad = (np.abs(grad32 - grad64)[inner] / scale[inner]).max()
        print(f"{name} F={F}: g e = {e_g:.3e}, e_torch = {t_g:.3e}, ratio {e_g / t_g:.2f}; grad e = {e_grad:.3e}, "
              f"e_torch = {t_grad:.3e}, ratio {e_grad / t_grad:.2f}")
        assert e_g <= 4 * t_g
        assert e_grad <= 4 * t_grad


# ------------------------------------------------------------------------------------- 3. the relaxation
@functools.lru_cache(maxsize=None)
def _relaxed(name, F):
    return _raw_relax(_export(name), rc.zigzag(CASES[name][1], F)[None], RELAX_ITERS)


@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("name", NATIVE)
def test_relaxation_of_the_zigzags(name, F):
    ex = _export(name)
    x = rc.zigzag(CASES[name][1], F)[None]
    status, frames, e0, e1, seg, step, acc = _relaxed(name, F)
    assert status == 0, _lib().geo_last_error()
    print(f"{name} F={F}: energy / energy0 = {e1[0] / e0[0]:.4f}, accepted {acc[0]} of {RELAX_ITERS}, step {step[0]:.4g}")
    assert e1[0] <= e0[0]
    assert rc.bits(frames[:, 0]) == rc.bits(x[:, 0]) and rc.bits(frames[:, -1]) == rc.bits(x[:, -1])
    cur, st = x, None
    for _ in range(RELAX_ITERS):
        s, cur, _, e_one, seg_one, st, _ = _raw_relax(ex, cur, 1, step=st)
        assert s == 0
    assert rc.bits(cur) == rc.bits(frames) and rc.bits(st) == rc.bits(step)
    assert rc.bits(e_one) == rc.bits(e1) and rc.bits(seg_one) == rc.bits(seg)
    assert e1[0] <= 0.9 * e0[0] and acc[0] >= 10
    assert np.sqrt(seg[0]).sum() ** 2 <= (F - 1) * e1[0] * (1 + 1e-12)
    # the result's energy and segments are Evaluate of the result
    _, E, seg_e, _, _, _ = _raw_energy(ex, frames, jac=False)
    assert rc.bits(E) == rc.bits(e1) and rc.bits(seg_e) == rc.bits(seg)


def test_evaluate_only_and_python_api():
    from vqvae_amd.geo import curve_energy_device, native_relax_covers, relax_curves_device
    name = "fm_none5"
    ex = _export(name)
    dec = rc.make_decoder(name)[0].to(_dev())
    assert native_relax_covers(dec) and not native_relax_covers(rc.make_decoder("fm_small")[0])
    x = _curves(name, 3, 5)
    _, E, seg, grad, g, J = _raw_energy(ex, x)
    for frames, iters in ((x, 0), (x[:, :2].copy(), 4)):
        status, fr, e0, e1, sg, st, acc = _raw_relax(ex, frames, iters)
        assert status == 0 and rc.bits(fr) == rc.bits(frames) and np.all(acc == 0) and rc.bits(e0) == rc.bits(e1)
        assert np.all(st >= 0) and (frames.shape[1] > 2 or np.all(st == 0))
    xg = torch.from_numpy(x).to(_dev())
    res = curve_energy_device(dec, xg, jacobian=True)
    assert res.route == "native" and res.energy.is_cuda
    _same((res.energy.cpu().numpy(), res.seg_sq.cpu().numpy(), res.grad.cpu().numpy(), res.outputs.cpu().numpy(),
           res.jac.cpu().numpy()), (E, seg, grad, g, J))
    assert curve_energy_device(ex, xg).jac is None
    rel = relax_curves_device(dec, xg, 3)
    assert rel.route == "native" and rc.bits(xg.cpu().numpy()) == rc.bits(x)          # the input is not modified
    _same((0,) + tuple(t.cpu().numpy() for t in (rel.frames, rel.energy0, rel.energy, rel.seg_sq, rel.step, rel.accepted)),
          _raw_relax(ex, x, 3))
    small = rc.make_decoder("fm_small")[0].to(_dev())
    assert relax_curves_device(small, torch.from_numpy(_curves("fm_small", 2, 5)).to(_dev()), 1).route == "torch"
    with pytest.raises(ValueError, match="BatchNorm"):
        relax_curves_device(rc.make_decoder("fm_batch", training=True)[0].to(_dev()), torch.zeros(1, 5, 16, device=_dev()), 1)
    with pytest.raises(ValueError, match="BatchNorm"):
        curve_energy_device(_export("fm_batch", True), torch.zeros(1, 5, 16, device=_dev()))


# ------------------------------------------------------------------------------------- 4. invariance
@pytest.mark.parametrize("name", ["fm_batch", "cf_batch", "fm_group", "fm_none5"])
def test_a_curve_alone_among_others_and_on_a_side_stream(name):
    ex = _export(name)
    lib = _lib()
    F, n = 5, 3
    x = _curves(name, 7, F)
    full = _raw_relax(ex, x, n)
    full_e = _raw_energy(ex, x)
    assert full[0] == 0 and full_e[0] == 0, lib.geo_last_error()
    for c in (0, 3, 6):                                   # alone
        _same(_raw_relax(ex, x[c:c + 1], n), (0,) + tuple(t[c:c + 1] for t in full[1:]))
        _same(_raw_energy(ex, x[c:c + 1]), (0,) + tuple(t[c:c + 1] for t in full_e[1:]))
    perm = np.random.RandomState(3).permutation(7)        # at another position
    _same(_raw_relax(ex, x[perm], n), (0,) + tuple(t[perm] for t in full[1:]))
    ws_min = lib.geo_curve_min_workspace_bytes(ex.desc, F)
    ws_3 = lib.geo_curve_workspace_bytes(ex.desc, 3, F)   # slices of 3, 3 and 1 curves
    for nbytes in (ws_min, ws_3):
        _same(_raw_relax(ex, x, n, ws_bytes=nbytes, fill=0xFF), full)
        _same(_raw_energy(ex, x, ws_bytes=nbytes, fill=0xFF), full_e)
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        _same(_raw_relax(ex, x, n), full)
        _same(_raw_energy(ex, x), full_e)
    # a NaN or inf in one curve stays there
    for poison in (float("nan"), float("inf")):
        bad = x.copy()
        bad[2, 1, 0] = poison
        got = _raw_relax(ex, bad, n)
        assert got[0] == 0
        keep = np.array([0, 1, 3, 4, 5, 6])
        _same(tuple(t[keep] for t in got[1:]), tuple(t[keep] for t in full[1:]))
        assert got[6][2] == 0 and rc.bits(got[1][2]) == rc.bits(bad[2])
        assert not (got[3][2] < got[2][2])


@pytest.mark.parametrize("ws_kind", ["queried", "minimum"])
@pytest.mark.parametrize("name", ["fm_batch", "cf_batch"])
def test_guarded_workspaces(monkeypatch, name, ws_kind):
    """The Python calls on guarded, exact-size workspaces with zero, ones32 and stale payloads: the same bits, intact guards."""
    from vqvae_amd.geo import curve_energy_device, relax_curves_device
    ex = _export(name)
    F = 5
    cap = _lib().geo_curve_min_workspace_bytes(ex.desc, F) if ws_kind == "minimum" else None
    A = torch.from_numpy(rc.zigzags(CASES[name][1], F, 4)[1:]).to(_dev())
    B = torch.from_numpy(_curves(name, 3, F)).to(_dev())

    def call(x):
        ev = curve_energy_device(ex, x, jacobian=True, max_workspace_bytes=cap)
        rel = relax_curves_device(ex, x, 3, max_workspace_bytes=cap)
        out = {"energy": ev.energy, "seg_sq": ev.seg_sq, "grad": ev.grad, "outputs": ev.outputs, "jac": ev.jac,
               "frames": rel.frames, "energy0": rel.energy0, "energy1": rel.energy, "seg1": rel.seg_sq, "step": rel.step,
               "accepted": rel.accepted}
        return out, rel.route

    want = ws_guard.four_runs(monkeypatch, call, A, B, "native")
    _same((0,) + tuple(want[k].cpu().numpy() for k in ("frames", "energy0", "energy1", "seg1", "step", "accepted")),
          _raw_relax(ex, B.cpu().numpy(), 3))


# ------------------------------------------------------------------------------------- 5. refusals
def test_refusals_without_a_launch():
    from vqvae_amd.spatial_decoder import DecoderExport, SpatialDecoder
    lib = _lib()
    dev = _dev()
    train = _export("fm_batch", True)
    wide = DecoderExport(SpatialDecoder(1, (256, 128, 64), 32, 28, "none").eval().to(dev), dev)
    for ex, d, word in ((train, 16, "BatchNorm"), (wide, 32, "latent_dim")):
        assert lib.geo_curve_workspace_bytes(ex.desc, 10, 5) == 0 and lib.geo_curve_min_workspace_bytes(ex.desc, 5) == 0
        assert lib.geo_metric_tensor_workspace_bytes(ex.desc, 50) == 0
        x = np.zeros((2, 5, d), dtype=np.float32)
        got = _raw_energy(ex, x, ws_bytes=1 << 20)
        assert got[0] == GEO_E_ARG and word in lib.geo_last_error().decode()
        assert all(np.isnan(t).all() for t in got[1:])                           # nothing was written
        got = _raw_relax(ex, x, 2, ws_bytes=1 << 20)
        assert got[0] == GEO_E_ARG and word in lib.geo_last_error().decode()
        assert rc.bits(got[1]) == rc.bits(x) and np.isnan(got[3]).all() and np.all(got[6] == -7)
    ok = _export("fm_batch")
    x = _curves("fm_batch", 2, 5)
    big = 1 << 26
    for F in (1, 65):
        assert lib.geo_curve_workspace_bytes(ok.desc, 2, F) == 0 and lib.geo_curve_min_workspace_bytes(ok.desc, F) == 0
    from vqvae_amd._device import ptr
    xg, ws = torch.from_numpy(x).to(dev), _ws(big, None)
    e = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    st = torch.full((2,), -1.0, dtype=torch.float64, device=dev)
    acc = torch.full((2,), -7, dtype=torch.int32, device=dev)
    for F, word in ((1, "F 1"), (65, "F 65")):
        assert lib.geo_curve_energy(ok.desc, ptr(xg), 2, F, ptr(e), None, None, None, None, ptr(ws), big, None) == GEO_E_ARG
        assert word in lib.geo_last_error().decode()
        assert lib.geo_curve_relax(ok.desc, ptr(xg), 2, F, 1, ptr(st), None, ptr(e), None, ptr(acc), ptr(ws), big, None) == GEO_E_ARG
        assert word in lib.geo_last_error().decode()
    assert lib.geo_curve_relax(ok.desc, ptr(xg), 2, 5, -1, ptr(st), None, ptr(e), None, ptr(acc), ptr(ws), big, None) == GEO_E_ARG
    assert "n_iters" in lib.geo_last_error().decode()
    for args in ((None, ptr(e), ptr(ws)), (ptr(xg), None, ptr(ws)), (ptr(xg), ptr(e), None)):
        assert lib.geo_curve_energy(ok.desc, args[0], 2, 5, args[1], None, None, None, None, args[2], big, None) == GEO_E_ARG
        assert "null" in lib.geo_last_error().decode()
    for args in ((None, ptr(st), ptr(e), ptr(acc)), (ptr(xg), None, ptr(e), ptr(acc)), (ptr(xg), ptr(st), None, ptr(acc)),
                 (ptr(xg), ptr(st), ptr(e), None)):
        assert lib.geo_curve_relax(ok.desc, args[0], 2, 5, 1, args[1], None, args[2], None, args[3], ptr(ws), big,
                                   None) == GEO_E_ARG
        assert "null" in lib.geo_last_error().decode()
    ws_min = lib.geo_curve_min_workspace_bytes(ok.desc, 5)
    got = _raw_energy(ok, x, ws_bytes=ws_min - 256)
    assert got[0] == GEO_E_ARG and "workspace" in lib.geo_last_error().decode() and np.isnan(got[1]).all()
    got = _raw_relax(ok, x, 1, ws_bytes=ws_min - 256)
    assert got[0] == GEO_E_ARG and "workspace" in lib.geo_last_error().decode() and np.isnan(got[3]).all()
    torch.cuda.synchronize()
    assert np.isnan(e.cpu().numpy()).all() and np.all(acc.cpu().numpy() == -7) and np.all(st.cpu().numpy() == -1.0)
    assert lib.geo_curve_energy(ok.desc, None, 0, 5, None, None, None, None, None, None, 0, None) == 0           # C == 0
    assert lib.geo_curve_relax(ok.desc, None, 0, 5, 3, None, None, None, None, None, None, 0, None) == 0


# ------------------------------------------------------------------------------------- 6. the CLI
D, COUT, SIZE, N_IMG, F_CLI = 16, 1, 28, 128, 5
PAIRS = [(3, 100), (77, 4)]


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    """A seeded decoder checkpoint and one build_codebook run on 128 seeded 16 x 4 x 4 latents (tests/test_gpu_interpolation.py's)."""
    from oracle import metric as om
    from vqvae_amd.scripts.build_codebook import main, make_parser
    tmp = str(tmp_path_factory.mktemp("relax_cli"))
    sd = om.make_decoder_state(7, D, COUT, norm_type="batch")
    torch.save({"model_state_dict": {"decoder." + k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, "epoch": 0},
               os.path.join(tmp, "best.pt"))
    z4 = np.random.RandomState(7).randn(N_IMG * 16, D).astype(np.float32).reshape(N_IMG, 4, 4, D)
    z_path = os.path.join(tmp, "z.pt")
    torch.save(torch.from_numpy(np.ascontiguousarray(np.transpose(z4, (0, 3, 1, 2)))), z_path)
    out = os.path.join(tmp, "codebook")
    main(make_parser().parse_args([
        "--latents_path", z_path, "--out_dir", out, "--vae_ckpt_path", os.path.join(tmp, "best.pt"),
        "--in_channels", str(COUT), "--output_image_size", str(SIZE), "--latent_dim", str(D),
        "--enc_channels", "64", "128", "256", "--dec_channels", "256", "128", "64", "--recon_loss", "mse",
        "--norm_type", "batch", "--mse_use_sigmoid", "--k", "20", "--sym", "union", "--K", "64", "--init", "kpp",
        "--seed", "42", "--batch_size", "512"]))
    return {"tmp": tmp, "codebook": out, "z": z_path}


def _run_cli(build, out_name, extra=()):
    from vqvae_amd.scripts.geodesic_interpolation import main, make_parser
    out = os.path.join(build["tmp"], out_name)
    res = main(make_parser().parse_args(["--codebook_dir", build["codebook"], "--out_dir", out, "--frames", str(F_CLI),
                                         "--pairs", *[f"{i}:{j}" for i, j in PAIRS], *extra]))
    return out, res


def _parent_artefacts(build, out_name):
    """The three artefacts as the script wrote them before --relax_iters existed, from interpolate_images_spatial without
    relaxation: the same calls in the same order with the same keys."""
    from scipy import sparse
    from vqvae_amd._device import DeviceCSR, device
    from vqvae_amd.geo import interpolate_images_spatial
    from vqvae_amd.scripts.generate_samples import save_image
    from vqvae_amd.spatial_decoder import load_decoder_from_checkpoint
    dev = device()
    cb = build["codebook"]
    cfg = torch.load(os.path.join(cb, "codebook.pt"), weights_only=False)["config"]
    codes = np.load(os.path.join(cb, "codes.npy"))
    W = sparse.load_npz(os.path.join(cb, "knn_graph_geodesic.npz")).tocsr()
    z = torch.load(build["z"]).float()
    dec = load_decoder_from_checkpoint(cfg["vae_ckpt_path"], in_channels=COUT, dec_channels=cfg["dec_channels"], latent_dim=D,
                                       output_image_size=SIZE, norm_type="batch", device=dev).eval()
    pairs = np.asarray(PAIRS, dtype=np.int64)
    out = interpolate_images_spatial(z, np.flatnonzero(codes.reshape(-1) >= 0), DeviceCSR.from_scipy(W, dev), dec, pairs, F_CLI,
                                     "other", True, batch_size=512)
    M, F = 2, F_CLI
    host = {k: out[k].cpu().numpy() for k in ("frames_lin", "frames_geo", "images_lin", "images_geo", "graph_dist", "hops",
                                               "status", "curve_len_lin", "curve_len_geo", "image_len_lin", "image_len_geo")}
    fallback = out["fallback_positions"]
    ratio = lambda a, b: a / b if b > 0 else None      # noqa: E731
    per_pair = []
    for m in range(M):
        rec = {"pair": [int(pairs[m, 0]), int(pairs[m, 1])],
               "graph_dist": float(host["graph_dist"][m][host["status"][m] == 0].astype(np.float64).sum()),
               "fallback_positions": [int(p) for p in fallback[m]]}
        for k in ("curve_len_lin", "curve_len_geo", "image_len_lin", "image_len_geo"):
            rec[k] = float(host[k][m])
        rec["ratio_curve"] = ratio(rec["curve_len_geo"], rec["curve_len_lin"])
        rec["ratio_image"] = ratio(rec["image_len_geo"], rec["image_len_lin"])
        per_pair.append(rec)
    totals = {k: float(sum(r[k] for r in per_pair))
              for k in ("graph_dist", "curve_len_lin", "curve_len_geo", "image_len_lin", "image_len_geo")}
    totals["ratio_curve"] = ratio(totals["curve_len_geo"], totals["curve_len_lin"])
    totals["ratio_image"] = ratio(totals["image_len_geo"], totals["image_len_lin"])
    totals["fallback_positions"] = int(sum(len(p) for p in fallback))
    summary = {"codebook_dir": str(cb), "frames": F, "dataset": "other", "apply_sigmoid": True, "pairs": per_pair,
               "totals": totals}
    dst = os.path.join(build["tmp"], out_name)
    os.makedirs(dst, exist_ok=True)
    rows = torch.stack([out["images_lin"], out["images_geo"]], dim=1)
    save_image(rows.reshape(M * 2 * F, *rows.shape[3:]).cpu(), os.path.join(dst, "interpolation.png"), nrow=F)
    np.savez(os.path.join(dst, "interpolation.npz"), pairs=pairs,
             fallback_pair=np.concatenate([np.full(len(p), m, dtype=np.int32) for m, p in enumerate(fallback)]),
             fallback_position=np.concatenate([np.asarray(p, dtype=np.int32) for p in fallback]), **host)
    with open(os.path.join(dst, "interpolation.json"), "w") as f:
        json.dump(summary, f, indent=2)
    return dst


def test_cli_without_the_flag_writes_the_parents_bytes(build):
    plain, _ = _run_cli(build, "plain")
    parent = _parent_artefacts(build, "parent")
    npz_a, npz_b = np.load(os.path.join(plain, "interpolation.npz")), np.load(os.path.join(parent, "interpolation.npz"))
    assert npz_a.files == npz_b.files
    for k in npz_a.files:
        assert rc.bits(npz_a[k]) == rc.bits(npz_b[k]), k
    for name in ("interpolation.png", "interpolation.json"):
        assert open(os.path.join(plain, name), "rb").read() == open(os.path.join(parent, name), "rb").read(), name
    # (an .npz is a zip archive and carries its members' modification times: compared member by member above)


def test_cli_with_relax_iters(build):
    from PIL import Image
    plain, _ = _run_cli(build, "plain_again")
    out, res = _run_cli(build, "relaxed", ["--relax_iters", "5"])
    npz, base = np.load(os.path.join(out, "interpolation.npz")), np.load(os.path.join(plain, "interpolation.npz"))
    new = {"frames_relaxed": (2, F_CLI, D, 4, 4), "images_relaxed": (2, F_CLI, COUT, SIZE, SIZE), "curve_len_relaxed": (2,),
           "image_len_relaxed": (2,), "relax_from": (2, 16), "accepted_geo": (2, 16), "accepted_lin": (2, 16),
           "energy_geo": (2, 16), "energy_lin": (2, 16), "energy_relaxed": (2, 16)}
    assert sorted(npz.files) == sorted(base.files + list(new))
    for k in base.files:
        assert rc.bits(npz[k]) == rc.bits(base[k]), k
    for k, shape in new.items():
        assert npz[k].shape == shape, (k, npz[k].shape)
    with Image.open(os.path.join(out, "interpolation.png")) as im:
        assert im.size == (F_CLI * (SIZE + 2) + 2, 3 * len(PAIRS) * (SIZE + 2) + 2)           # the third row per pair
    assert np.all(npz["energy_relaxed"] <= np.minimum(npz["energy_geo"], npz["energy_lin"]))
    assert set(np.unique(npz["relax_from"])) <= {0, 1} and npz["accepted_geo"].max() <= 5 and npz["accepted_lin"].min() >= 0
    assert rc.bits(npz["frames_relaxed"][:, 0]) == rc.bits(npz["frames_lin"][:, 0])             # the ends did not move
    assert rc.bits(npz["frames_relaxed"][:, -1]) == rc.bits(npz["frames_lin"][:, -1])
    summary = json.load(open(os.path.join(out, "interpolation.json")))
    assert summary["relax_iters"] == 5
    for m, rec in enumerate(summary["pairs"]):
        for k in ("curve_len_relaxed", "image_len_relaxed"):
            assert rec[k] == float(npz[k][m])
        for k in ("energy_geo", "energy_lin", "energy_relaxed"):
            assert rec[k] == float(npz[k][m].astype(np.float64).sum())
        for k in ("relax_from", "accepted_geo", "accepted_lin"):
            assert rec[k] == npz[k][m].tolist()
    for k in ("curve_len_relaxed", "image_len_relaxed", "energy_geo", "energy_lin", "energy_relaxed"):
        assert summary["totals"][k] == float(sum(r[k] for r in summary["pairs"]))
    assert rc.bits(res["frames_relaxed"].cpu().numpy()) == rc.bits(npz["frames_relaxed"])
