"""geo_vanilla_vjp (csrc/vanilla_jvp.hip) on the GPU: accuracy against fp64 autograd with float32 autograd as the yardstick,
bit equality under everything a row must not depend on, the refusal of uncovered decoders, and the adjoint identity against
the library's own tangent kernels."""
import numpy as np
import pytest
import torch

import vanilla_curve_cases as K
import vanilla_jvp_cases as V

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _export(name):
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    return VanillaDecoderExport(K.decoder(name), _dev())


def _vjp(ex, z, u, **kw):
    from vqvae_amd.geo import vanilla_vjp_device
    return vanilla_vjp_device(ex, z.to(_dev()), u.to(_dev()), **kw).cpu().numpy()


@pytest.mark.parametrize("name", list(K.VJP_CASES))
def test_accuracy_against_fp64_autograd(name):
    """2085 rows, u = randn: per row e = |out - ref|_2 / |ref|_2 against fp64 autograd on the CPU.  Gates: median and
    0.99-quantile at most 4 x float32 autograd's on the same rows, at most 10 rows (0.5 %, check_against_fp64's cap for rows
    at a ReLU boundary) above 1e-5.  float32 autograd's own count is printed beside the one noted in vanilla_curve_cases.VJP_CASES; it is no gate, since it
    moves with the CPU's float32 kernels (5 and 13 of wide-bn-32x1-d2's rows on two machines)."""
    z, u = K.rows(name)
    ref64, ref32 = K.reference(name)
    e_torch = K.row_error(ref32, ref64)
    got = _vjp(_export(name), z, u)
    assert got.dtype == np.float64 and got.shape == ref64.shape and np.all(np.isfinite(got))
    e = K.row_error(got, ref64)
    med, q99, above = np.median(e), np.quantile(e, 0.99), int((e > 1e-5).sum())
    med_t, q99_t, above_t = np.median(e_torch), np.quantile(e_torch, 0.99), int((e_torch > 1e-5).sum())
    print(f"{name}: native median {med:.3e} q99 {q99:.3e} max {e.max():.3e} above 1e-5: {above} | float32 autograd median "
          f"{med_t:.3e} q99 {q99_t:.3e} max {e_torch.max():.3e} above 1e-5: {above_t} (noted: {K.VJP_CASES[name]}) | ratios {med / med_t:.2f} {q99 / q99_t:.2f}")
    assert med <= 4 * med_t and q99 <= 4 * q99_t and above <= K.BOUNDARY_CAP


@pytest.mark.parametrize("name", K.EXACT_CASES)
def test_rows_do_not_depend_on_their_company(name):
    """Bit for bit: the rows permuted; through `index`; n in {1, 2, 3, 63, 64, 65}; the minimum workspace (one item per pass)
    and one in between, both filled with 0xFF first; a side stream; a second run.  u = 0 gives exactly 0."""
    from vqvae_amd import _lib
    from vqvae_amd._device import workspace
    dev = _dev()
    ex = _export(name)
    z, u = (t[:130].to(dev) for t in K.rows(name))
    base = _vjp(ex, z, u)
    assert np.all(np.isfinite(base)) and np.all(np.abs(base).sum(1) > 0)
    assert np.array_equal(_vjp(ex, z, u), base)
    perm = torch.randperm(130, generator=torch.Generator().manual_seed(3)).to(dev)
    assert np.array_equal(_vjp(ex, z[perm], u[perm]), base[perm.cpu().numpy()])
    assert np.array_equal(_vjp(ex, z, u[perm], index=perm.to(torch.int32)), base[perm.cpu().numpy()])
    for n in (1, 2, 3, 63, 64, 65):
        assert np.array_equal(_vjp(ex, z[7:7 + n], u[7:7 + n]), base[7:7 + n]), n
    lib = _lib.load()
    least = lib.geo_vanilla_vjp_min_workspace_bytes(ex.desc)
    assert 0 < least == lib.geo_vanilla_vjp_workspace_bytes(ex.desc, 1) < lib.geo_vanilla_vjp_workspace_bytes(ex.desc, 130)
    for cap in (least, lib.geo_vanilla_vjp_workspace_bytes(ex.desc, 37)):
        workspace(lib.geo_vanilla_vjp_workspace_bytes(ex.desc, 130), dev).fill_(0xFF)
        assert np.array_equal(_vjp(ex, z, u, max_workspace_bytes=cap), base), cap
    with pytest.raises(_lib.GeoHipError):
        _vjp(ex, z, u, max_workspace_bytes=least - 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _vjp(ex, z, u)
    side.synchronize()
    assert np.array_equal(other, base)
    zero = _vjp(ex, z, torch.zeros_like(u))
    assert zero.shape == base.shape and np.all(zero == 0.0)
    mixed = u.clone()
    mixed[::2] = 0
    got = _vjp(ex, z, mixed)
    assert np.all(got[::2] == 0.0) and np.array_equal(got[1::2], base[1::2])


@pytest.mark.parametrize("what", ["widths", "group"])
def test_uncovered_decoders_are_refused(what):
    """A (32, 32, 16)-wide decoder and a GroupNorm decoder: the Python entry raises, a descriptor with such widths gets size
    queries of 0 and GEO_E_ARG."""
    from vqvae_amd import _lib
    from vqvae_amd.geo import vanilla_vjp_device
    dev = _dev()
    dec = (V.make_decoder((32, 32, 16), 8, 1, 28, "none") if what == "widths" else V.make_decoder((128, 64, 32), 8, 1, 28, "group")).to(dev)
    z, u = torch.randn(4, 8, device=dev), torch.randn(4, 784, device=dev)
    with pytest.raises(ValueError, match="not covered"):
        vanilla_vjp_device(dec, z, u)
    lib = _lib.load()
    ex = _export("narrow-none-28")
    bad = _lib.VanillaDecoderDesc.from_buffer_copy(ex.desc)
    bad.c1, bad.c2 = 32, 16
    assert lib.geo_vanilla_vjp_workspace_bytes(bad, 4) == 0 and lib.geo_vanilla_vjp_min_workspace_bytes(bad) == 0
    out = torch.full((4, 16), 7.0, dtype=torch.float64, device=dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    from vqvae_amd._device import ptr
    zz, uu = torch.randn(4, 16, device=dev), torch.randn(4, 784, device=dev)
    assert lib.geo_vanilla_vjp(bad, ptr(zz), None, 4, ptr(uu), ptr(out), ptr(ws), ws.numel(), None) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                       # nothing was launched


@pytest.mark.parametrize("name", list(V.CASES))
def test_adjoint_identity_against_the_tangent_kernels(name):
    """dz . (J^T u) = u . (J dz): with u = J dz the left side is |J dz|^2, which the tangent kernels give through
    geo_vanilla_jvp_pairs as len = (|J(z_a) dz| + |J(z_b) dz|) / 2 (the unit-tangent pass stays internal).  300 edges, u_a and
    u_b = J dz by fp64 forward-mode autograd, rounded to float32 and given to the VJP as data:
        (sqrt(dz . vjp(z_a, u_a)) + sqrt(dz . vjp(z_b, u_b))) / 2   against   len,
    per-edge relative mismatch.  The yardstick is float32 torch's own mismatch on the same rows -- its autograd VJP in the
    same expression against its autograd lengths -- and the gate 4 x its median and 4 x its 0.99-quantile."""
    from vqvae_amd.geo.riemannian_metric import edge_lengths_vanilla_device
    dec, zs, ze, _, auto32 = V.case(name)
    n = 300
    za, zb = zs[:n], ze[:n]
    dz = (zb - za).double().numpy()
    ua = torch.from_numpy(K.autograd_jvp(dec, za, zb - za, torch.float64)).float()
    ub = torch.from_numpy(K.autograd_jvp(dec, zb, zb - za, torch.float64)).float()
    ex = _export(name)

    def through(vjp):
        return 0.5 * (np.sqrt((dz * vjp(za, ua)).sum(1)) + np.sqrt((dz * vjp(zb, ub)).sum(1)))
    native_len = edge_lengths_vanilla_device(ex, za.to(_dev()).contiguous(), zb.to(_dev()).contiguous()).cpu().numpy().astype(np.float64)
    e = np.abs(through(lambda z, u: _vjp(ex, z, u)) - native_len) / native_len
    t = np.abs(through(lambda z, u: K.autograd_vjp(dec, z, u, torch.float32)) - auto32[:n]) / auto32[:n]
    print(f"{name}: adjoint mismatch native median {np.median(e):.3e} q99 {np.quantile(e, 0.99):.3e} max {e.max():.3e} | "
          f"float32 torch median {np.median(t):.3e} q99 {np.quantile(t, 0.99):.3e} max {t.max():.3e}")
    assert np.median(e) <= 4 * np.median(t) and np.quantile(e, 0.99) <= 4 * np.quantile(t, 0.99)
