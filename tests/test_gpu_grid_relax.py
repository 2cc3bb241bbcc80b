"""geo_spatial_curve_energy / geo_spatial_curve_relax (csrc/vanilla_jvp.hip) on the GPU: every output
restated in numpy from the call's own outputs, bit for bit; a curve's bits independent of its company, the slices and a NaN
neighbour; and descent on zig-zag curves of grids."""
import numpy as np
import pytest
import torch

import grid_vjp_cases as K

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _export(name):
    from vqvae_amd.spatial_decoder import SpatialImageDecoderExport
    return SpatialImageDecoderExport(K.decoder(name), _dev())


def _np(t):
    return t.cpu().numpy()


def _vjp(ex, z, u):
    from vqvae_amd.geo import spatial_grid_vjp_device
    return _np(spatial_grid_vjp_device(ex, z, u))


def _relax_fields(r):
    return [_np(t) for t in (r.frames, r.energy0, r.energy, r.seg_sq, r.step, r.accepted)]


@pytest.mark.parametrize("shape", K.CURVE_SHAPES, ids=lambda s: f"C{s[0]}-F{s[1]}")
@pytest.mark.parametrize("name", K.CURVE_CASES)
def test_energy_outputs_are_their_restatement(name, shape):
    """energy and seg_sq equal the numpy restatement from g_out (fold_256 included); grad equals 2 geo_spatial_vjp(x[f], (float) r[f])
    and is 0 at the ends; probe_out equals the restatement from geo_spatial_vjp(x[f], s): all bit for bit.  Then one iteration of the
    relaxation equals the restated first step, trial and decision from the calls' own outputs."""
    from vqvae_amd.geo import grid_curve_energy_device, relax_grid_curves_device
    C, F = shape
    _, d, Co, S, _ = K.spec(name)
    ex = _export(name)
    x = K.curves(name, C, F).to(_dev())
    ev = grid_curve_energy_device(ex, x, probe=True)
    assert ev.route == "native" and ev.jac is None
    g = _np(ev.outputs)
    energy, seg, r = K.restate_energy(g, _np(x))
    assert np.array_equal(_np(ev.energy), energy) and np.array_equal(_np(ev.seg_sq), seg)
    flat = x.view(C * F, d, 4, 4)
    vj = _vjp(ex, flat, torch.from_numpy(r).view(C * F, -1).to(_dev())).reshape(C, F, d, 4, 4)
    want = 2.0 * vj
    want[:, 0] = 0.0
    want[:, -1] = 0.0
    grad = _np(ev.grad)
    assert np.array_equal(grad, want) and not grad[:, 0].any() and not grad[:, -1].any()
    if F > 2:
        assert np.abs(grad[:, 1:-1]).reshape(C, -1).sum(1).min() > 0
    s = torch.from_numpy(K.sign_probe(Co, S)).view(1, -1).expand(C * F, -1).contiguous().to(_dev())
    probe = K.restate_probe(_vjp(ex, flat, s).reshape(C * F, -1)).reshape(C, F)
    assert np.array_equal(_np(ev.trace), probe) and probe.min() > 0
    # one iteration from the step left to the call
    one = relax_grid_curves_device(ex, x, 1)
    frames1, e0, e1, seg1, step1, acc1 = _relax_fields(one)
    assert np.array_equal(e0, energy)
    h = K.restate_first_step(probe)
    y = K.restate_trial(_np(x), h, grad)
    ev_y = grid_curve_energy_device(ex, torch.from_numpy(y).to(_dev()))
    ey = _np(ev_y.energy)
    take = (ey < energy) if F > 2 else np.zeros(C, bool)
    assert np.array_equal(acc1, take.astype(np.int32))
    assert np.array_equal(frames1, np.where(take.reshape(-1, 1, 1, 1, 1), y, _np(x)))
    assert np.array_equal(e1, np.where(take, ey, energy))
    assert np.array_equal(seg1, np.where(take[:, None], _np(ev_y.seg_sq), seg))
    assert np.array_equal(step1, np.where(take, 2.0 * h, h / 4.0) if F > 2 else h)


@pytest.mark.parametrize("name", K.CURVE_CASES)
def test_iterations_and_company_change_no_bit(name):
    """20 calls of one iteration equal one call of 20.  A curve's bits are the same alone, among others, permuted, in slices of
    one and two curves (workspace caps, on 0xFF-filled memory), and beside a NaN or an inf curve, which comes back unchanged with
    accepted == 0."""
    from vqvae_amd import _lib
    from vqvae_amd._device import workspace
    from vqvae_amd.geo import relax_grid_curves_device
    d = K.spec(name)[1]
    C, F, n = 5, 5, 20
    ex = _export(name)
    x = K.zigzag_grids(d, F, C).to(_dev())
    whole = relax_grid_curves_device(ex, x, n)
    base = _relax_fields(whole)
    assert base[5].min() >= 1 and np.all(base[2] < base[1])
    cur, step, total = x, None, torch.zeros(C, dtype=torch.int32, device=_dev())
    for _ in range(n):
        r = relax_grid_curves_device(ex, cur, 1, step=step)
        cur, step, total = r.frames, r.step, total + r.accepted
    assert np.array_equal(_np(cur), base[0]) and np.array_equal(_np(r.energy), base[2]) and np.array_equal(_np(step), base[4])
    assert np.array_equal(_np(total), base[5]) and np.array_equal(_np(r.seg_sq), base[3])
    alone = _relax_fields(relax_grid_curves_device(ex, x[3:4], n))
    assert all(np.array_equal(a, b[3:4]) for a, b in zip(alone, base))
    perm = torch.tensor([4, 2, 0, 3, 1], device=_dev())
    permuted = _relax_fields(relax_grid_curves_device(ex, x[perm], n))
    assert all(np.array_equal(a, b[_np(perm)]) for a, b in zip(permuted, base))
    lib = _lib.load()
    full = lib.geo_spatial_curve_workspace_bytes(ex.desc, C, F)
    least = lib.geo_spatial_curve_min_workspace_bytes(ex.desc, F)
    assert 0 < least == lib.geo_spatial_curve_workspace_bytes(ex.desc, 1, F) < full
    for cap in (least, lib.geo_spatial_curve_workspace_bytes(ex.desc, 2, F)):
        workspace(full, _dev()).fill_(0xFF)
        sliced = _relax_fields(relax_grid_curves_device(ex, x, n, max_workspace_bytes=cap))
        assert all(np.array_equal(a, b) for a, b in zip(sliced, base)), cap
    with pytest.raises(_lib.GeoHipError):
        relax_grid_curves_device(ex, x, n, max_workspace_bytes=least - 1)
    for bad in (float("nan"), float("inf")):
        xb = x.clone()
        xb[1, 2, 0, 1, 1] = bad
        got = _relax_fields(relax_grid_curves_device(ex, xb, n))
        keep = [0, 2, 3, 4]
        assert all(np.array_equal(a[keep], b[keep]) for a, b in zip(got, base))
        assert np.array_equal(got[0][1], _np(xb[1]), equal_nan=True) and got[5][1] == 0 and np.isnan(got[2][1])


@pytest.mark.parametrize("F", [5, 9])
@pytest.mark.parametrize("name", ["wide-bn-28-d16", "wide-bn-32x3-d32", "narrow-none-28-d5"])
def test_zigzags_descend(name, F):
    """Zig-zags of amplitude 4 over the 16 d coordinates, C = 3, 20 iterations with the step left to the call: energy / energy0
    <= 0.75, at least 12 accepted steps, energy <= energy0, the ends bitwise fixed.  (The same rules over the float32 torch module
    on the CPU give 0.04 .. 0.63 and 15 .. 17 accepts on these curves.)  From a common explicit step the native energy / energy0
    agrees with the torch route's on the CPU to 3 digits."""
    from vqvae_amd.geo import relax_grid_curves_device
    d = K.spec(name)[1]
    x = K.zigzag_grids(d, F, 3)
    r = relax_grid_curves_device(_export(name), x.to(_dev()), 20)
    frames, e0, e1, _, _, acc = _relax_fields(r)
    print(f"{name} F={F}: energy / energy0 {e1 / e0}, accepted {acc}, step {_np(r.step)}")
    assert r.route == "native"
    assert np.all(e1 <= e0) and np.all(e1 / e0 <= 0.75) and np.all(acc >= 12)
    assert np.array_equal(frames[:, 0], x[:, 0].numpy()) and np.array_equal(frames[:, -1], x[:, -1].numpy())
    step = 0.25 * _np(relax_grid_curves_device(_export(name), x.to(_dev()), 0).step)
    native = relax_grid_curves_device(_export(name), x.to(_dev()), 20, step=torch.from_numpy(step))
    torch_route = relax_grid_curves_device(K.decoder(name), x, 20, step=torch.from_numpy(step))
    assert torch_route.route == "torch"
    ratio_n, ratio_t = _np(native.energy) / _np(native.energy0), _np(torch_route.energy) / _np(torch_route.energy0)
    print(f"{name} F={F}: common step {step}: native {ratio_n}, torch {ratio_t}")
    assert np.allclose(ratio_n, ratio_t, rtol=1e-3, atol=0)
