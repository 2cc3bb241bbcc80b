"""The vector-Jacobian product of the vanilla decoder on the host: the export's transposed packs reproduce fp64 autograd when
the kernels' passes are restated in fp64 torch, the existing tensors and their hash inputs are untouched, the size queries
follow one layout, and the descriptor's coverage is make_shape's."""
import numpy as np
import pytest
import torch

import vanilla_curve_cases as K
import vanilla_jvp_cases as V

CPU = torch.device("cpu")
GEO_E_ARG = -1                          # include/geo_hip.h


@pytest.mark.parametrize("name", ["narrow-none-28", "narrow-none-32x3-d5", "narrow-bn-28x3-d33", "wide-bn-32x1-d2",
                                  "narrow-none-32x1-d1"])
def test_transposed_packs_reproduce_autograd(name):
    """Point pass + the adjoint convolutions by kernel tap + the K-quad At, evaluated in fp64 from the export's float32 tensors,
    against fp64 autograd through the module on 12 rows: everything but the tensors' one rounding (6e-8 relative each) is fp64,
    so rows agree to about 1e-7; 1e-5 leaves room for a row next to a ReLU boundary."""
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    dec = K.decoder(name)
    d = K.spec(name)[1]
    g = torch.Generator().manual_seed(4)
    z, u = torch.randn(12, d, generator=g), torch.randn(12, K.n_out(name), generator=g)
    want = K.autograd_vjp(dec, z, u, torch.float64)
    got = K.emulate_vjp(VanillaDecoderExport(dec, CPU), z, u).numpy()
    e = K.row_error(got, want)
    print(f"{name}: emulated VJP against fp64 autograd, worst row {e.max():.3e}")
    assert np.all(np.linalg.norm(want, axis=1) > 0) and e.max() < 1e-5


def test_export_keeps_its_tensors_and_adds_the_adjoint_packs():
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    ex = VanillaDecoderExport(V.build((128, 64, 32), 33, 3, 28, "batch"), CPU)
    assert sorted(ex.tensors) == ["At", "b3", "c", "scale2", "shift2", "w2p", "w3p"]      # what native_bits hashes
    assert ex.adjoint["w2t"].shape == (16, 8, 64, 4) and ex.adjoint["w3t"].shape == (16, 3, 32)
    assert ex.adjoint["Atq"].shape == (49 * 64 // 4, 64, 4) and not ex.adjoint["Atq"][:, 33:].any()
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in ex.adjoint.values())
    for name, t in ex.adjoint.items():
        assert getattr(ex.desc, name) == t.data_ptr()
    assert ex.n_out == 3 * 28 * 28


def test_size_queries_and_coverage():
    from vqvae_amd import _lib
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    lib = _lib.load()
    ex = VanillaDecoderExport(V.build((256, 128, 64), 128, 3, 32, "batch"), CPU)
    q, least = lib.geo_vanilla_vjp_workspace_bytes, lib.geo_vanilla_vjp_min_workspace_bytes(ex.desc)
    assert 0 < least == q(ex.desc, 1) == q(ex.desc, 0) < q(ex.desc, 65) < q(ex.desc, 1024) == q(ex.desc, 10 ** 7)
    assert q(ex.desc, -1) == 0 and q(None, 5) == 0 and lib.geo_vanilla_vjp_min_workspace_bytes(None) == 0
    for field, value in (("c1", 32), ("c2", 16), ("latent_dim", 129), ("latent_dim", 0), ("out_channels", 2), ("out_size", 64)):
        bad = _lib.VanillaDecoderDesc.from_buffer_copy(ex.desc)
        setattr(bad, field, value)
        assert q(bad, 100) == 0 and lib.geo_vanilla_vjp_min_workspace_bytes(bad) == 0, field
        # rejected before any launch: no GPU is needed to be refused
        assert lib.geo_vanilla_vjp(bad, None, None, 4, None, None, None, 0, None) == GEO_E_ARG, field
    # the existing entry points take a descriptor without the transposed packs; the VJP does not
    old = _lib.VanillaDecoderDesc.from_buffer_copy(ex.desc)
    old.w2t = old.w3t = old.Atq = None
    assert lib.geo_vanilla_jvp_workspace_bytes(old, 7) == lib.geo_vanilla_jvp_workspace_bytes(ex.desc, 7) > 0
    assert lib.geo_vanilla_vjp(old, None, None, 4, None, None, None, 0, None) == GEO_E_ARG


def test_python_entry_refuses_an_uncovered_decoder():
    from vqvae_amd.geo import vanilla_vjp_device
    dec = V.make_decoder((128, 64, 32), 16, 1, 28, "group")
    with pytest.raises(ValueError, match="not covered"):
        vanilla_vjp_device(dec, torch.zeros(2, 16), torch.zeros(2, 784))
