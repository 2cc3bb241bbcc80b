"""The native image encode, image decode and eval-mode vanilla pull-back across the envelope their predicates admit
(encoder_kernels_cover, vanilla_kernels_cover, spatial_image_kernels_cover): the points of encode_cases.ENVELOPE_CASES,
decode_cases.SPATIAL_ENVELOPE_CASES and vanilla_jvp_cases.ENVELOPE_CASES, chosen for the d-dependent branches and the
template / size pairings of csrc/encode.hip and csrc/vanilla_jvp.hip that the suites of DESIGN.md sections 15, 17 and 18 do not
reach.  Every bound is the one those suites apply: 8 x the same module's float32-torch error against fp64 for every element of
the encode and the decode, vanilla_jvp_cases.check_against_fp64 for the lengths.  The batches are the small ones of those
suites (77 | 37 items, 2085 edges, 300 latents with 1500 edges); the references are computed once per case on the CPU.

The tests print the error ratios and the pull-back shares; DESIGN.md sections 15, 17 and 18 record them."""
import copy

import numpy as np
import pytest
import torch

import decode_cases as D
import encode_cases as E
import vanilla_jvp_cases as V

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def same(a, b) -> bool:
    return all(torch.equal(p, q) for p, q in zip(a, b))


# ---------------------------------------------------------------- encode

@pytest.mark.parametrize("kind,name", E.ALL_ENVELOPE_CASES)
def test_encode(kind, name):
    """The module itself is routed to the kernels; every element of mu and of logvar within 8 x the float32-torch error of
    the same module against fp64; the first row alone, the last row alone and the whole batch at the minimum workspace are the
    bits of the plain call."""
    from vqvae_amd import _lib
    from vqvae_amd.encode import encode_latents, last_encode_path
    from vqvae_amd.image_encoder import ImageEncoderExport
    enc, x, mu64, lv64, err_mu, err_lv = E.envelope_case(kind, name)
    x, n, err32 = x.to(dev()), x.shape[0], max(err_mu, err_lv)
    plain = encode_latents(copy.deepcopy(enc).to(dev()), x)
    assert last_encode_path() == "hip"
    for tag, got, truth in (("mu", plain[0], mu64), ("logvar", plain[1], lv64)):
        assert got.dtype == torch.float32 and got.shape == truth.shape and got.is_cuda
        err = float((got.cpu().double() - truth).abs().max())
        print(f"{kind} {name} {tag}: n={n} max abs error {err:.3e}, float32 torch {err32:.3e}, ratio {err / err32:.2f}, "
              f"magnitude {float(truth.abs().max()):.2f}")
        assert torch.isfinite(got).all()
        assert err <= 8 * err32, (tag, err, err32)
    export = ImageEncoderExport(enc, dev())
    assert same(encode_latents(export, x), plain), "module and export differ"
    assert same(encode_latents(export, x[:1]), (plain[0][:1], plain[1][:1])), "row 0 alone differs"
    assert same(encode_latents(export, x[n - 1:]), (plain[0][n - 1:], plain[1][n - 1:])), "the last row alone differs"
    least = int(_lib.load().geo_image_encode_workspace_bytes(export.desc, 1))
    assert same(encode_latents(export, x, max_workspace_bytes=least), plain), "minimum workspace differs"


# ---------------------------------------------------------------- decode

def _check_decode(kind, name, dec, z, truth, err32):
    """The checks the two decoders share; returns (export, plain logits)."""
    from vqvae_amd import _lib
    from vqvae_amd.decode import decode_logits, last_decode_path
    from vqvae_amd.spatial_decoder import SpatialImageDecoderExport
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    n = z.shape[0]
    plain = decode_logits(copy.deepcopy(dec).to(dev()), z)
    assert last_decode_path() == "hip" and plain.dtype == torch.float32 and plain.shape == truth.shape and plain.is_cuda
    err = float((plain.cpu().double() - truth).abs().max())
    print(f"{kind} {name}: n={n} max abs error {err:.3e}, float32 torch {err32:.3e}, ratio {err / err32:.2f}, "
          f"logit magnitude {float(truth.abs().max()):.2f}")
    assert torch.isfinite(plain).all()
    assert err <= 8 * err32, (err, err32)
    lib = _lib.load()
    if kind == "vanilla":
        export, query = VanillaDecoderExport(dec, dev()), lib.geo_vanilla_decode_workspace_bytes
    else:
        export, query = SpatialImageDecoderExport(dec, dev()), lib.geo_spatial_decode_workspace_bytes
    assert torch.equal(decode_logits(export, z), plain), "module and export differ"
    assert torch.equal(decode_logits(export, z[:1]), plain[:1]), "row 0 alone differs"
    assert torch.equal(decode_logits(export, z[n - 1:]), plain[n - 1:]), "the last row alone differs"
    assert torch.equal(decode_logits(export, z, max_workspace_bytes=int(query(export.desc, 1))), plain), "minimum workspace differs"
    return export, plain


@pytest.mark.parametrize("name", list(V.ENVELOPE_CASES))
def test_vanilla_decode(name):
    """As test_encode, for the logits of the vanilla decoder."""
    dec, z, truth, err32 = D.vanilla_envelope_case(name)
    _check_decode("vanilla", name, dec, z.to(dev()), truth, err32)


@pytest.mark.parametrize("name", list(D.SPATIAL_ENVELOPE_CASES))
def test_spatial_decode(name):
    """As test_encode, for the logits of the spatial decoder; the (table, codes) route is the grid route bit for bit; a 28-px
    decoder, with 3 channels too, gives exactly the [2:30, 2:30] crop of the 32-px decoder with the same state dict."""
    from vqvae_amd.decode import decode_logits
    channels, d, C, size, norm = D.SPATIAL_ENVELOPE_CASES[name]
    dec, z, truth, err32 = D.spatial_envelope_case(name)
    z = z.to(dev())
    export, plain = _check_decode("spatial", name, dec, z, truth, err32)
    g = torch.Generator().manual_seed(7)
    table = torch.randn(11, d, generator=g).to(dev())
    codes = torch.randint(0, 11, (z.shape[0], 4, 4), generator=g).to(dev())
    grid = table[codes].permute(0, 3, 1, 2).contiguous()
    assert torch.equal(decode_logits(export, table=table, codes=codes), decode_logits(export, grid)), "(table, codes) route differs"
    if size == 28:
        dec32 = D.build_spatial(channels, d, C, 32, norm)
        dec32.load_state_dict(dec.state_dict())
        big = decode_logits(dec32.eval().to(dev()), z)
        assert plain.shape[-2:] == (28, 28) and big.shape == (z.shape[0], C, 32, 32)
        assert torch.equal(plain, big[:, :, 2:30, 2:30])


# ---------------------------------------------------------------- pull-back

def _forbid_autograd(monkeypatch):
    from vqvae_amd.geo import riemannian_metric

    def boom(*a, **k):
        raise AssertionError("autograd route taken")
    monkeypatch.setattr(riemannian_metric, "_generic_jvp_norms", boom)


@pytest.mark.parametrize("name", list(V.ENVELOPE_CASES))
def test_pull_back_pairs(name, monkeypatch):
    """The three criteria of vanilla_jvp_cases.check_against_fp64 for the kernels AND for float32 autograd on the CPU on the
    same inputs (which ties the inputs to the 0.5 % cap); with the autograd route made to raise, the public entry still
    answers; endpoints swapped give the same bits; dz = 0 gives exactly 0."""
    from vqvae_amd.geo.riemannian_metric import edge_lengths_riemannian, edge_lengths_vanilla_device
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    dec, zs, ze, want64, auto32 = V.envelope_case(name)
    print(f"{name}: float32 autograd (CPU) leaves {int((V.rel_error(auto32, want64) > 1e-5).sum())} of {V.N_EDGES} edges outside 1e-5")
    V.check_against_fp64(auto32, want64, f"{name}: float32 autograd (CPU)")
    _forbid_autograd(monkeypatch)
    got = edge_lengths_riemannian(dec, zs, ze, batch_size=512)
    assert got.dtype == torch.float32 and got.shape == (V.N_EDGES,)
    got = got.cpu().numpy()
    print(f"{name}: native leaves {int((V.rel_error(got, want64) > 1e-5).sum())} of {V.N_EDGES} edges outside 1e-5")
    V.check_against_fp64(got, want64, f"{name}: native")
    ex = VanillaDecoderExport(dec, dev())
    zs, ze = zs.to(dev()).contiguous(), ze.to(dev()).contiguous()
    assert np.array_equal(edge_lengths_vanilla_device(ex, zs, ze).cpu().numpy(), got), "export and module differ"
    assert np.array_equal(edge_lengths_vanilla_device(ex, ze, zs).cpu().numpy(), got), "swapped endpoints differ"
    still = edge_lengths_vanilla_device(ex, zs, zs.clone()).cpu().numpy()
    assert still.shape == got.shape and np.all(still == 0.0), "dz = 0 is not exactly 0"


@pytest.mark.parametrize("name", list(V.ENVELOPE_CASES))
def test_pull_back_graph_entry(name):
    """300 latents, 1500 random (src, dst) pairs with self loops: the graph entry is bit for bit the pairs entry on the
    gathered endpoints, at the default workspace and at the documented minimum; self loops are exactly 0."""
    from vqvae_amd import _lib
    from vqvae_amd.geo.riemannian_metric import edge_lengths_vanilla_device, edge_lengths_vanilla_graph_device
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    channels, d, C, size, norm = V.ENVELOPE_CASES[name]
    ex = VanillaDecoderExport(V.build(channels, d, C, size, norm, seed=len(name)), dev())
    g = torch.Generator().manual_seed(9)
    z = torch.randn(300, d, generator=g).to(dev())
    src = torch.randint(0, 300, (1500,), generator=g, dtype=torch.int32)
    dst = torch.randint(0, 300, (1500,), generator=g, dtype=torch.int32)
    dst[::50] = src[::50]
    src, dst = src.to(dev()), dst.to(dev())
    pairs = edge_lengths_vanilla_device(ex, z[src.long()].contiguous(), z[dst.long()].contiguous()).cpu().numpy()
    assert np.array_equal(edge_lengths_vanilla_graph_device(ex, z, src, dst).cpu().numpy(), pairs)
    loops = (src == dst).cpu().numpy()
    assert loops.sum() >= 30 and np.all(pairs[loops] == 0.0) and np.all(np.isfinite(pairs)) and np.all(pairs[~loops] > 0)
    least = _lib.load().geo_vanilla_jvp_workspace_bytes(ex.desc, 1)
    assert np.array_equal(edge_lengths_vanilla_graph_device(ex, z, src, dst, max_workspace_bytes=least).cpu().numpy(), pairs)
