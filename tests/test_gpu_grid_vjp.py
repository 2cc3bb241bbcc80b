"""geo_spatial_vjp (csrc/vanilla_jvp.hip) on the GPU: accuracy against fp64 autograd of the module with
float32 autograd as the yardstick, bit equality under everything a row must not depend on, the 28-px crop against the padding-1
twin, and geo_spatial_decode untouched by the descriptor's new fields."""
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


def _vjp(ex, z, u, **kw):
    from vqvae_amd.geo import spatial_grid_vjp_device
    return spatial_grid_vjp_device(ex, z.to(_dev()), u.to(_dev()), **kw).cpu().numpy()


@pytest.mark.parametrize("name", list(K.ALL_CASES))
def test_accuracy_against_fp64_autograd(name):
    """260 grids, u = randn: per grid e = |out - ref|_2 / |ref|_2 against fp64 autograd of the module on the CPU.  Gates: median
    and 0.99-quantile at most 4 x float32 autograd's on the same rows; the maximum error of g (the native route's sigmoids, through
    grid_curve_energy_device) at most 4 x float32 torch's; at most 4 rows (ReLU-boundary mask flips) above 1e-5."""
    from vqvae_amd.geo import grid_curve_energy_device
    z, u = K.rows(name)
    ref64, g64, ref32, g32 = K.reference(name)
    ex = _export(name)
    got = _vjp(ex, z, u)
    assert got.dtype == np.float64 and got.shape == tuple(z.shape) and np.all(np.isfinite(got))
    e, e_torch = K.row_error(got, ref64), K.row_error(ref32, ref64)
    g = grid_curve_energy_device(ex, z.view(K.N_ROWS // 2, 2, *z.shape[1:]).to(_dev())).outputs.cpu().numpy().reshape(g64.shape)
    g_err, g_err_torch = np.abs(g - g64).max(), np.abs(g32 - g64).max()
    med, q99, above = np.median(e), np.quantile(e, 0.99), int((e > 1e-5).sum())
    med_t, q99_t, above_t = np.median(e_torch), np.quantile(e_torch, 0.99), int((e_torch > 1e-5).sum())
    print(f"{name}: native median {med:.3e} q99 {q99:.3e} max {e.max():.3e} above 1e-5: {above} g {g_err:.3e} | float32 autograd "
          f"median {med_t:.3e} q99 {q99_t:.3e} max {e_torch.max():.3e} above 1e-5: {above_t} g {g_err_torch:.3e}")
    assert med <= 4 * med_t and q99 <= 4 * q99_t
    assert g_err <= 4 * g_err_torch
    assert above <= K.BOUNDARY_CAP


@pytest.mark.parametrize("name", ["wide-bn-32x3-d32", "narrow-none-28-d5", "narrow-bn-28x3-d63", "wide-bn-32x1-d64"])
def test_rows_do_not_depend_on_their_company(name):
    """Bit for bit: the rows permuted; through `index`; n in {1, 2, 3, 15, 16, 17, 31, 33} (16 grids per front workgroup, 2 items
    per mid workgroup, 32 rows per final tile); the minimum workspace and one in between, both filled with 0xFF first; a side
    stream.  u = 0 gives exactly 0, also for single rows among others."""
    from vqvae_amd import _lib
    from vqvae_amd._device import workspace
    dev = _dev()
    ex = _export(name)
    z, u = (t[:70].to(dev) for t in K.rows(name))
    base = _vjp(ex, z, u)
    flat = base.reshape(70, -1)
    assert np.all(np.isfinite(base)) and np.all(np.abs(flat).sum(1) > 0)
    perm = torch.randperm(70, generator=torch.Generator().manual_seed(3)).to(dev)
    assert np.array_equal(_vjp(ex, z[perm], u[perm]), base[perm.cpu().numpy()])
    assert np.array_equal(_vjp(ex, z, u[perm], index=perm.to(torch.int32)), base[perm.cpu().numpy()])
    for n in (1, 2, 3, 15, 16, 17, 31, 33):
        assert np.array_equal(_vjp(ex, z[5:5 + n], u[5:5 + n]), base[5:5 + n]), n
    lib = _lib.load()
    least = lib.geo_spatial_vjp_min_workspace_bytes(ex.desc)
    full = lib.geo_spatial_vjp_workspace_bytes(ex.desc, 70)
    assert 0 < least == lib.geo_spatial_vjp_workspace_bytes(ex.desc, 1) < full
    for cap in (least, lib.geo_spatial_vjp_workspace_bytes(ex.desc, 19)):
        workspace(full, dev).fill_(0xFF)
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


@pytest.mark.parametrize("name", ["wide-bn-28-d16", "narrow-bn-28x3-d63"])
def test_28_px_is_the_window_of_the_padding_one_twin(name):
    """At 28 px the result equals, bit for bit, the call on the padding-1 twin module (same weights, 32 px) with u zero-padded
    by 2."""
    from vqvae_amd.spatial_decoder import SpatialImageDecoderExport
    z, u = (t[:37] for t in K.rows(name))
    twin = SpatialImageDecoderExport(K.padding_one_twin(K.decoder(name)), _dev())
    assert twin.out_size == 32
    got = _vjp(_export(name), z, u)
    assert np.array_equal(got, _vjp(twin, z, torch.nn.functional.pad(u, (2, 2, 2, 2))))
    assert np.all(np.abs(got.reshape(37, -1)).sum(1) > 0)


@pytest.mark.parametrize("name", ["wide-bn-28-d16", "wide-bn-32x3-d32", "narrow-none-28-d5"])
def test_decode_ignores_the_transposed_packs(name):
    """geo_spatial_decode on the export gives, bit for bit, the logits of a call whose descriptor has the new fields null."""
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr
    from vqvae_amd.decode import decode_logits
    dev = _dev()
    ex = _export(name)
    z = K.rows(name)[0][:37].to(dev).contiguous()
    want = decode_logits(ex, z)
    bare = _lib.SpatialImageDecoderDesc.from_buffer_copy(ex.desc)
    bare.w1t = bare.w2t = bare.w3t = None
    lib = _lib.load()
    out = torch.empty_like(want)
    ws = torch.empty(lib.geo_spatial_decode_workspace_bytes(bare, 37), dtype=torch.uint8, device=dev)
    assert lib.geo_spatial_decode(bare, ptr(z), None, None, 37, ptr(out), ptr(ws), ws.numel(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    grid = torch.empty(37, ex.latent_dim, 4, 4, dtype=torch.float64, device=dev)
    u = K.rows(name)[1][:37].to(dev).contiguous()
    assert lib.geo_spatial_vjp(bare, ptr(z), None, 37, ptr(u), ptr(grid), ptr(ws), ws.numel(), None) == -1     # GEO_E_ARG
