"""Host side of the curve relaxation (vqvae_amd.geo.relaxation, geo_curve_energy / geo_curve_relax): the ABI names, the torch
route on the CPU against the numpy restatement of tests/relax_cases.py, and the relax_iters argument of geodesic_interpolation
on a small CPU graph.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import relax_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("geo_curve_workspace_bytes", "geo_curve_min_workspace_bytes", "geo_curve_energy", "geo_curve_relax")


def test_abi_names():
    from vqvae_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "geo_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (geo_[a-z0-9_]+)", out))
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and name in _lib._SIGNATURES, name
        assert name in exported, name
    from vqvae_amd import geo
    for name in ("curve_energy_device", "relax_curves_device", "native_relax_covers"):
        assert name in geo.__all__ and callable(getattr(geo, name))


def _vanilla():
    from vqvae_amd.vae import Decoder
    torch.manual_seed(3)
    return Decoder(1, (32, 16, 8), 4, 28, "batch").eval()


DECODERS = {"fm_small": lambda: rc.make_decoder("fm_small")[0], "vanilla": _vanilla}


def _curves(d, F):
    return torch.from_numpy(rc.zigzags(d, F, 3))


@pytest.mark.parametrize("kind", list(DECODERS))
def test_torch_route_evaluate_equals_restatement(kind):
    from vqvae_amd.geo import curve_energy_device, native_relax_covers
    dec = DECODERS[kind]()
    d = 16 if kind == "fm_small" else 4
    assert not native_relax_covers(dec)
    for F in (2, 3, 5):
        x = _curves(d, F)
        res = curve_energy_device(dec, x, jacobian=True)
        assert res.route == "torch" and res.jac.shape[:3] == (3, F, d) and res.outputs.shape[:2] == (3, F)
        assert res.energy.dtype == torch.float64 and res.outputs.dtype == torch.float32 and res.jac.dtype == torch.float32
        E, seg, grad, _ = rc.evaluate(res.outputs.numpy(), res.jac.numpy())
        assert rc.bits(res.energy.numpy()) == rc.bits(E)
        assert rc.bits(res.seg_sq.numpy()) == rc.bits(seg)
        assert rc.bits(res.grad.numpy()) == rc.bits(grad)
        assert np.all(res.grad.numpy()[:, 0] == 0) and np.all(res.grad.numpy()[:, -1] == 0)
        assert curve_energy_device(dec, x).jac is None
        # Cauchy-Schwarz, up to rounding
        assert np.all(np.sqrt(seg).sum(1) ** 2 <= (F - 1) * E * (1 + 1e-12))


@pytest.mark.parametrize("kind", list(DECODERS))
def test_torch_route_relax(kind):
    from vqvae_amd.geo import curve_energy_device, relax_curves_device
    dec = DECODERS[kind]()
    d = 16 if kind == "fm_small" else 4
    F, n = 5, 4
    x = _curves(d, F)

    def outputs_jac(frames):                              # the route's own g and J
        r = curve_energy_device(dec, torch.from_numpy(frames), jacobian=True)
        return r.outputs.numpy(), r.jac.numpy()

    res = relax_curves_device(dec, x, n)
    assert res.route == "torch" and res.frames.dtype == torch.float32 and res.accepted.dtype == torch.int32
    want = rc.relax(outputs_jac, x.numpy(), n)
    for got, ref in zip((res.frames, res.energy0, res.energy, res.seg_sq, res.step, res.accepted), want):
        assert rc.bits(got.numpy()) == rc.bits(ref)
    assert rc.bits(res.frames[:, 0].numpy()) == rc.bits(x[:, 0].numpy())          # the ends come back bitwise
    assert rc.bits(res.frames[:, -1].numpy()) == rc.bits(x[:, -1].numpy())
    assert np.all(res.energy.numpy() <= res.energy0.numpy()) and int(res.accepted.min()) >= 1
    # n iterations in one call = n calls of one iteration
    cur, step = x, None
    for _ in range(n):
        one = relax_curves_device(dec, cur, 1, step=step)
        cur, step = one.frames, one.step
    assert rc.bits(cur.numpy()) == rc.bits(res.frames.numpy()) and rc.bits(step.numpy()) == rc.bits(res.step.numpy())
    # the first trial is x - step0 * grad
    ev = curve_energy_device(dec, x, jacobian=True)
    _, _, grad, tr = rc.evaluate(ev.outputs.numpy(), ev.jac.numpy())
    first = relax_curves_device(dec, x, 1)
    y = rc.trial(x.numpy(), rc.step0(tr), grad)
    took = first.accepted.numpy() == 1
    assert took.any()
    assert rc.bits(first.frames.numpy()[took]) == rc.bits(y[took])
    assert rc.bits(first.frames.numpy()[~took]) == rc.bits(x.numpy()[~took])
    # evaluate only
    for frames, iters in ((x, 0), (_curves(d, 2), 3)):
        still = relax_curves_device(dec, frames, iters)
        assert rc.bits(still.frames.numpy()) == rc.bits(frames.numpy()) and int(still.accepted.max()) == 0
        assert rc.bits(still.energy.numpy()) == rc.bits(still.energy0.numpy())


def test_torch_route_refusals_and_nan_curve():
    from vqvae_amd.geo import curve_energy_device, relax_curves_device
    dec = DECODERS["fm_small"]()
    x = _curves(16, 5)
    with pytest.raises(ValueError, match="BatchNorm"):
        curve_energy_device(rc.make_decoder("fm_small", training=True)[0], x)
    with pytest.raises(ValueError, match="BatchNorm"):
        relax_curves_device(rc.make_decoder("fm_small", training=True)[0], x, 1)
    with pytest.raises(ValueError, match="F = 1"):
        curve_energy_device(dec, x[:, :1])
    with pytest.raises(ValueError, match="F = 65"):
        relax_curves_device(dec, torch.zeros(1, 65, 16), 1)
    with pytest.raises(ValueError, match="n_iters"):
        relax_curves_device(dec, x, -1)
    with pytest.raises(ValueError, match=r"\[C, F, d\]"):
        curve_energy_device(dec, x[0])
    bad = x.clone()
    bad[1, 2, 3] = float("nan")
    clean = relax_curves_device(dec, x, 3)
    res = relax_curves_device(dec, bad, 3)
    assert int(res.accepted[1]) == 0 and rc.bits(res.frames[1].numpy()) == rc.bits(bad[1].numpy())
    assert bool(torch.isnan(res.energy[1])) and bool(torch.isnan(res.energy0[1]))
    for k in (0, 2):
        assert int(res.accepted[k]) == int(clean.accepted[k])
        assert np.all(res.energy.numpy()[k] <= res.energy0.numpy()[k])


def _small_graph():
    """A kNN-like graph over 40 seeded latents on the CPU: (z, DeviceCSR, decoder)."""
    from scipy import sparse
    from vqvae_amd._device import DeviceCSR
    z = np.random.RandomState(31).randn(40, 16).astype(np.float32)
    dist = np.linalg.norm(z[:, None] - z[None], axis=2)
    rows, cols = [], []
    for i in range(40):
        for j in np.argsort(dist[i])[1:6]:
            rows += [i, j]
            cols += [j, i]
    W = sparse.csr_matrix((dist[rows, cols].astype(np.float32), (rows, cols)), shape=(40, 40))
    W.sum_duplicates()
    W.data = dist[W.nonzero()].astype(np.float32)
    return z, W, DeviceCSR.from_scipy(W, torch.device("cpu"))


def _interpolation(monkeypatch, relax_iters):
    """geodesic_interpolation on the CPU graph: the path walk and the resampling are HIP kernels, so the test stands in for them
    with scipy's predecessors and numpy's polyline resampling -- what is under test is the relax_iters argument."""
    from scipy.sparse.csgraph import dijkstra
    from vqvae_amd.geo import interpolation as ip
    z, W, G = _small_graph()
    src, dst = np.array([0, 3, 7]), np.array([25, 3, 30])
    dmat, pred = dijkstra(W, indices=src, return_predecessors=True)

    class Paths:
        status = torch.zeros(3, dtype=torch.int32)
        hops = torch.zeros(3, dtype=torch.int32)

    def frames_geo(F):
        out = np.zeros((3, F, 16), dtype=np.float32)
        for m in range(3):
            nodes = [int(dst[m])]
            while nodes[-1] != src[m]:
                nodes.append(int(pred[m, nodes[-1]]))
            pts = z[nodes[::-1]].astype(np.float64)
            if len(pts) == 1:
                out[m] = pts[0]
                continue
            cum = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(pts, axis=0), axis=1))])
            t = np.linspace(0.0, cum[-1], F)
            out[m] = np.stack([np.interp(t, cum, pts[:, k]) for k in range(16)], axis=1)
            out[m, 0], out[m, -1] = z[src[m]], z[dst[m]]
        return torch.from_numpy(out)

    def chord(zt, a, b, F):
        t = torch.linspace(0, 1, F).view(1, F, 1)
        fr = zt[a].unsqueeze(1) * (1 - t) + zt[b].unsqueeze(1) * t
        fr[:, 0], fr[:, -1] = zt[a], zt[b]
        return fr.float()

    monkeypatch.setattr(ip, "geodesic_paths_device", lambda G_, s, d_: (Paths, torch.from_numpy(dmat[np.arange(3), dst]).float()))
    monkeypatch.setattr(ip, "resample_paths_device", lambda zt, paths, F: frames_geo(F))
    monkeypatch.setattr(ip, "chord_frames_device", chord)
    dec = rc.make_decoder("fm_small")[0]

    def lengths(decoder, frames, batch_size=512):        # (curve_lengths runs the JVP kernels: sum of sqrt(seg_sq) stands in)
        from vqvae_amd.geo import curve_energy_device
        return curve_energy_device(decoder, frames).seg_sq.sqrt().sum(1).float()

    monkeypatch.setattr(ip, "curve_lengths", lengths)
    return ip.geodesic_interpolation(torch.from_numpy(z), G, dec, src, dst, 5, relax_iters=relax_iters)


def test_interpolation_without_relaxation_returns_todays_keys(monkeypatch):
    out = _interpolation(monkeypatch, 0)
    assert sorted(out) == ["curve_len_geo", "curve_len_lin", "frames_geo", "frames_lin", "graph_dist", "hops", "status"]


def test_interpolation_relaxed_is_never_worse_than_either_start(monkeypatch):
    from vqvae_amd.geo import relax_curves_device
    out = _interpolation(monkeypatch, 6)
    plain = _interpolation(monkeypatch, 0)
    for k in plain:
        assert rc.bits(out[k].numpy()) == rc.bits(plain[k].numpy()), k
    assert sorted(set(out) - set(plain)) == ["accepted_geo", "accepted_lin", "curve_len_relaxed", "energy_geo", "energy_lin",
                                            "energy_relaxed", "frames_relaxed", "relax_from"]
    e_geo, e_lin, e_rel = (out[k].numpy() for k in ("energy_geo", "energy_lin", "energy_relaxed"))
    assert np.all(e_rel <= np.minimum(e_geo, e_lin))
    dec = rc.make_decoder("fm_small")[0]
    geo, lin = relax_curves_device(dec, out["frames_geo"], 6), relax_curves_device(dec, out["frames_lin"], 6)
    want_from = (geo.energy.numpy() <= lin.energy.numpy()).astype(np.int32)       # a tie goes to the geodesic
    assert out["relax_from"].dtype == torch.int32 and np.array_equal(out["relax_from"].numpy(), want_from)
    assert int(out["relax_from"][1]) == 1                                        # the pair that is one node: 0 == 0, a tie
    want = np.where(want_from[:, None, None] == 1, geo.frames.numpy(), lin.frames.numpy())
    assert rc.bits(out["frames_relaxed"].numpy()) == rc.bits(want)
    assert rc.bits(e_rel) == rc.bits(np.where(want_from == 1, geo.energy.numpy(), lin.energy.numpy()))
    assert out["curve_len_relaxed"].shape == (3,) and bool(torch.isfinite(out["curve_len_relaxed"]).all())
