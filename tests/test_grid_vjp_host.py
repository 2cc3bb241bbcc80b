"""The grid VJP and the grid curves without a GPU: the coverage predicate, the export's transposed packs
against fp64 autograd, the torch route against a numpy restatement, the ABI's three listings and the refusals that come before
any launch."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import decode_cases as D
import grid_vjp_cases as K
import vanilla_jvp_cases as V

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("geo_spatial_vjp_workspace_bytes", "geo_spatial_vjp_min_workspace_bytes", "geo_spatial_vjp",
               "geo_spatial_curve_workspace_bytes", "geo_spatial_curve_min_workspace_bytes", "geo_spatial_curve_energy",
               "geo_spatial_curve_relax")


def test_predicate_table():
    from vqvae_amd.geo import native_grid_relax_covers
    from vqvae_amd.spatial_decoder import spatial_image_kernels_cover
    for name in K.ALL_CASES:
        assert native_grid_relax_covers(K.decoder(name)), name
    uncovered = {
        "group": D.make_spatial_decoder((256, 128, 64), 16, 1, 28, "group"),
        "train": D.make_spatial_decoder((256, 128, 64), 16, 1, 28, "batch", eval_mode=False),
        "widths": D.make_spatial_decoder((32, 32, 16), 8, 1, 28, "none"),
        "d65": D.make_spatial_decoder((128, 64, 32), 65, 1, 28, "none"),
        "vanilla": V.build((128, 64, 32), 16, 1, 28, "none"),
    }
    for what, dec in uncovered.items():
        assert not native_grid_relax_covers(dec), what
        assert native_grid_relax_covers(dec) == spatial_image_kernels_cover(dec)


@pytest.mark.parametrize("name", list(K.ALL_CASES))
def test_transposed_packs_reproduce_autograd(name):
    """The backward pass restated in fp64 torch from `adjoint` and the fp64 module's masks, against fp64 autograd through the
    module on 6 grids: per grid 1e-6 relative (everything but the packs' one float32 rounding, 6e-8 each, is fp64)."""
    from vqvae_amd.spatial_decoder import SpatialImageDecoderExport
    dec = K.decoder(name)
    ex = SpatialImageDecoderExport(dec, CPU)
    z, u = (t[:6] for t in K.rows(name))
    got = K.emulate_backward(ex, dec, z, u).numpy()
    want = K.reference(name)[0][:6]
    e = K.row_error(got, want)
    print(f"{name}: {e}")
    assert e.max() <= 1e-6


def test_export_keeps_its_tensors_and_adds_the_adjoint_packs():
    from vqvae_amd.spatial_decoder import SpatialImageDecoderExport
    ex = SpatialImageDecoderExport(K.decoder("narrow-bn-28x3-d63"), CPU)
    assert sorted(ex.tensors) == ["b3", "scale1", "scale2", "shift1", "shift2", "w1p", "w2p", "w3p"]      # what native_bits hashes
    assert {k: tuple(v.shape) for k, v in ex.adjoint.items()} == {"w1t": (16, 16, 64, 4), "w2t": (16, 8, 64, 4), "w3t": (16, 3, 32)}
    assert all(v.dtype == torch.float32 and v.is_contiguous() for v in ex.adjoint.values())
    assert not ex.adjoint["w1t"][:, :, 63:].any() and ex.n_out == 3 * 28 * 28
    for k, v in ex.adjoint.items():
        assert getattr(ex.desc, k) == v.data_ptr()


@pytest.mark.parametrize("name", ["wide-bn-28-d16", "narrow-bn-32x3-d7"])
def test_torch_route_is_its_restatement(name):
    """energy, seg_sq, grad and the probe of the torch route equal a numpy restatement that runs no project code: g and both
    vector-Jacobian products by the float32 module and torch.autograd.grad, the sums in numpy in the documented orders."""
    from vqvae_amd.geo import grid_curve_energy_device, relax_grid_curves_device
    _, d, Co, S, _ = K.spec(name)
    dec = K.decoder(name)
    C, F = 2, 5
    x = K.curves(name, C, F)
    ev = grid_curve_energy_device(dec, x, probe=True)
    assert ev.route == "torch" and ev.jac is None
    flat = x.view(C * F, d, 4, 4).clone().requires_grad_(True)
    g = torch.sigmoid(dec(flat)).reshape(C * F, -1)
    energy, seg, r = K.restate_energy(g.detach().numpy().reshape(C, F, -1), x.numpy())
    assert np.array_equal(ev.outputs.numpy().reshape(C * F, -1), g.detach().numpy())
    assert np.array_equal(ev.energy.numpy(), energy) and np.array_equal(ev.seg_sq.numpy(), seg)
    vr = torch.autograd.grad(g, flat, torch.from_numpy(r).view(C * F, -1), retain_graph=True)[0]
    grad = 2.0 * vr.double().numpy().reshape(C, F, d, 4, 4)
    grad[:, 0] = 0.0
    grad[:, -1] = 0.0
    assert np.allclose(ev.grad.numpy(), grad, rtol=1e-12, atol=0) and not ev.grad[:, 0].any() and not ev.grad[:, -1].any()
    s = torch.from_numpy(K.sign_probe(Co, S)).view(1, -1).expand(C * F, -1)
    vs = torch.autograd.grad(g, flat, s)[0].double().numpy().reshape(C * F, -1)
    probe = K.restate_probe(vs).reshape(C, F)
    assert np.allclose(ev.trace.numpy(), probe, rtol=1e-12, atol=0)
    zero = relax_grid_curves_device(dec, x, 0)
    assert np.allclose(zero.step.numpy(), K.restate_first_step(ev.trace.numpy()), rtol=1e-15, atol=0)
    assert torch.equal(zero.frames, x) and np.array_equal(zero.energy.numpy(), energy)
    bad = x.clone()
    bad[1, 2, 0, 0, 0] = float("inf")
    out = relax_grid_curves_device(dec, bad, 3)
    assert out.accepted[1] == 0 and torch.isnan(out.energy[1]) and torch.equal(out.frames[1], bad[1]) and out.accepted[0] >= 1


def test_torch_route_takes_uncovered_decoders_and_refuses_train_mode():
    from vqvae_amd.geo import grid_curve_energy_device, relax_grid_curves_device, spatial_grid_vjp_device
    dec = D.make_spatial_decoder((64, 32, 16), 3, 1, 28, "group")
    x = D.grids(8, 3, seed=2).view(2, 4, 3, 4, 4)
    r = relax_grid_curves_device(dec, x, 4)
    assert r.route == "torch" and bool((r.energy <= r.energy0).all()) and r.frames.shape == x.shape
    assert torch.equal(r.frames[:, 0], x[:, 0]) and torch.equal(r.frames[:, -1], x[:, -1])
    out = spatial_grid_vjp_device(dec, x.view(8, 3, 4, 4), torch.zeros(8, 1, 28, 28))
    assert out.dtype == torch.float64 and out.shape == (8, 3, 4, 4) and not out.any()
    train = D.make_spatial_decoder((256, 128, 64), 16, 1, 28, "batch", eval_mode=False)
    z = D.grids(4, 16).view(1, 4, 16, 4, 4)
    for call in (lambda: grid_curve_energy_device(train, z), lambda: relax_grid_curves_device(train, z, 1),
                 lambda: spatial_grid_vjp_device(train, z[0], torch.zeros(4, 1, 28, 28))):
        with pytest.raises(ValueError, match="train-mode BatchNorm"):
            call()
    with pytest.raises(ValueError):
        grid_curve_energy_device(K.decoder("wide-bn-28-d16"), D.grids(4, 16).view(4, 1, 16, 4, 4))      # F = 1


def test_abi_lists_the_new_symbols():
    from vqvae_amd import _lib
    header = open(os.path.join(ROOT, "include", "geo_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vqvae_amd", "libgeo_hip.so")], check=True,
                        capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", nm))
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % sym, header), sym
        assert sym in _lib._SIGNATURES and sym in exported, sym
    fields = [f[0] for f in _lib.SpatialImageDecoderDesc._fields_]
    assert fields[-3:] == ["w1t", "w2t", "w3t"] and fields[:13] == ["latent_dim", "c1", "c2", "out_channels", "out_size", "w1p",
                                                                     "scale1", "shift1", "w2p", "scale2", "shift2", "w3p", "b3"]
    assert re.search(r"b3;[^}]*w1t;[^}]*w2t;[^}]*w3t;[^}]*\} geo_spatial_image_decoder_desc;", header)


def test_refusals_come_before_any_launch():
    """An uncovered or null descriptor: size queries 0 and GEO_E_ARG; a covered one answers its queries on the host, 0 for F
    outside [2, 64], and refuses a short workspace with GEO_E_WORKSPACE."""
    from vqvae_amd import _lib
    from vqvae_amd.spatial_decoder import SpatialImageDecoderExport
    lib = _lib.load()
    ex = SpatialImageDecoderExport(K.decoder("narrow-none-28-d5"), CPU)
    assert 0 < lib.geo_spatial_vjp_min_workspace_bytes(ex.desc) == lib.geo_spatial_vjp_workspace_bytes(ex.desc, 1)
    assert lib.geo_spatial_vjp_workspace_bytes(ex.desc, 2000) == lib.geo_spatial_vjp_workspace_bytes(ex.desc, 1024)
    assert 0 < lib.geo_spatial_curve_min_workspace_bytes(ex.desc, 9) == lib.geo_spatial_curve_workspace_bytes(ex.desc, 1, 9)
    assert lib.geo_spatial_curve_workspace_bytes(ex.desc, 10 ** 6, 9) == lib.geo_spatial_curve_workspace_bytes(ex.desc, 4096 // 9, 9)
    for F in (1, 65):
        assert lib.geo_spatial_curve_workspace_bytes(ex.desc, 3, F) == 0 and lib.geo_spatial_curve_min_workspace_bytes(ex.desc, F) == 0
    wide = _lib.SpatialImageDecoderDesc.from_buffer_copy(ex.desc)
    wide.c1, wide.c2 = 32, 16
    deep = _lib.SpatialImageDecoderDesc.from_buffer_copy(ex.desc)
    deep.latent_dim = 65
    one = np.zeros(64, np.float64)                                 # never read: every call below returns before a launch
    p = one.ctypes.data
    for bad in (wide, deep, None):
        assert lib.geo_spatial_vjp_workspace_bytes(bad, 4) == 0 and lib.geo_spatial_vjp_min_workspace_bytes(bad) == 0
        assert lib.geo_spatial_curve_workspace_bytes(bad, 3, 5) == 0 and lib.geo_spatial_curve_min_workspace_bytes(bad, 5) == 0
        assert lib.geo_spatial_vjp(bad, p, None, 4, p, p, p, 1 << 30, None) == -1
        assert lib.geo_spatial_curve_energy(bad, p, 3, 5, p, None, None, None, None, p, 1 << 30, None) == -1
        assert lib.geo_spatial_curve_relax(bad, p, 3, 5, 2, p, None, p, None, p, p, 1 << 30, None) == -1
    assert lib.geo_spatial_curve_energy(ex.desc, p, 3, 65, p, None, None, None, None, p, 1 << 30, None) == -1
    assert lib.geo_spatial_vjp(ex.desc, p, None, 0, p, p, p, 0, None) == 0                       # n == 0: GEO_OK, no launch
    assert lib.geo_spatial_curve_energy(ex.desc, p, 0, 5, p, None, None, None, None, p, 0, None) == 0
    short = lib.geo_spatial_vjp_min_workspace_bytes(ex.desc) - 1
    assert lib.geo_spatial_vjp(ex.desc, p, None, 4, p, p, p, short, None) == -2
    short = lib.geo_spatial_curve_min_workspace_bytes(ex.desc, 5) - 1
    assert lib.geo_spatial_curve_energy(ex.desc, p, 3, 5, p, None, None, None, None, p, short, None) == -2
    assert not one.any()
