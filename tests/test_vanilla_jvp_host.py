"""Host side of the native vanilla-decoder pull-back metric (no GPU): which modules the kernels of csrc/vanilla_jvp.hip cover,
the export's fp64-composed front and re-laid-out convolutions against the module itself, and the workspace queries."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import vanilla_jvp_cases as V
from vanilla_jvp_cases import autograd_lengths, make_decoder, make_edges

CPU = torch.device("cpu")


class ReferenceStyleDecoder(nn.Module):
    """Not vqvae_amd.vae.Decoder: another class with the reference Decoder's attribute names and layers."""

    def __init__(self, out_channels, channels, latent_dim, size, batch_norm):
        super().__init__()
        self.fc = nn.Linear(latent_dim, channels[0] * 16)
        norm = (lambda c: nn.BatchNorm2d(c)) if batch_norm else (lambda c: nn.Identity())
        self.deconv1 = nn.Sequential(nn.ConvTranspose2d(channels[0], channels[1], 3, stride=2, padding=1,
                                                        output_padding=1 if size == 32 else 0), norm(channels[1]), nn.ReLU(inplace=True))
        self.deconv2 = nn.Sequential(nn.ConvTranspose2d(channels[1], channels[2], 4, stride=2, padding=1), norm(channels[2]),
                                     nn.ReLU(inplace=True))
        self.output_layer = nn.ConvTranspose2d(channels[2], out_channels, 4, stride=2, padding=1)

    def forward(self, z):
        return self.output_layer(self.deconv2(self.deconv1(self.fc(z).view(z.size(0), -1, 4, 4))))


def test_predicate_truth_table():
    from vqvae_amd.spatial_decoder import SpatialDecoder
    from vqvae_amd.vanilla_decoder import looks_like_vanilla_decoder, vanilla_kernels_cover
    wide, narrow = (256, 128, 64), (128, 64, 32)
    for channels in (wide, narrow):
        for d in (1, 5, 16, 127, 128):
            for C, size in ((1, 28), (3, 32), (3, 28), (1, 32)):
                assert vanilla_kernels_cover(make_decoder(channels, d, C, size, "none")), (channels, d, C, size)
        assert vanilla_kernels_cover(make_decoder(channels, 16, 1, 28, "batch"))                      # eval-mode BatchNorm
        train_bn = make_decoder(channels, 16, 1, 28, "batch", eval_mode=False)
        assert looks_like_vanilla_decoder(train_bn) and not vanilla_kernels_cover(train_bn)
        group = make_decoder(channels, 16, 1, 28, "group")
        assert looks_like_vanilla_decoder(group) and not vanilla_kernels_cover(group)
    assert vanilla_kernels_cover(make_decoder((64, 128, 64), 16, 1, 28, "none"))                       # any dec_channels[0]
    assert vanilla_kernels_cover(ReferenceStyleDecoder(1, narrow, 16, 28, True).eval())               # duck typing
    assert vanilla_kernels_cover(ReferenceStyleDecoder(3, wide, 128, 32, False).eval())
    assert not vanilla_kernels_cover(ReferenceStyleDecoder(1, narrow, 16, 28, True).train())
    # one norm layer left in training mode is enough: torch looks at the layer's own flag
    half = make_decoder(wide, 16, 1, 28, "batch")
    half.deconv2[1].train()
    assert not vanilla_kernels_cover(half)
    no_stats = make_decoder(narrow, 16, 1, 28, "none")
    no_stats.deconv1[1] = nn.BatchNorm2d(64, track_running_stats=False).eval()
    no_stats.deconv2[1] = nn.BatchNorm2d(32, track_running_stats=False).eval()
    assert looks_like_vanilla_decoder(no_stats) and not vanilla_kernels_cover(no_stats)
    for layer in ("fc", "output_layer"):
        no_bias = make_decoder(narrow, 16, 1, 28, "none")
        getattr(no_bias, layer).bias = None
        assert looks_like_vanilla_decoder(no_bias) and not vanilla_kernels_cover(no_bias)
    no_bias = make_decoder(narrow, 16, 1, 28, "none")
    no_bias.deconv2[0].bias = None
    assert not vanilla_kernels_cover(no_bias)
    assert not vanilla_kernels_cover(make_decoder((128, 96, 32), 16, 1, 28, "none"))                   # other widths
    assert not vanilla_kernels_cover(make_decoder((128, 128, 32), 16, 1, 28, "none"))
    assert not vanilla_kernels_cover(make_decoder(narrow, 129, 1, 28, "none"))
    assert not vanilla_kernels_cover(make_decoder(narrow, 16, 2, 28, "none"))
    assert not looks_like_vanilla_decoder(SpatialDecoder(1, wide, 16, 28, "none"))
    assert not looks_like_vanilla_decoder(nn.Sequential(nn.Linear(4, 4)))
    with pytest.raises(ValueError):
        from vqvae_amd.vanilla_decoder import VanillaDecoderExport
        VanillaDecoderExport(group, CPU)


@pytest.mark.parametrize("channels", [(256, 128, 64), (128, 64, 32)])
@pytest.mark.parametrize("size,C", [(28, 1), (32, 3), (28, 3), (32, 1)])
@pytest.mark.parametrize("norm", ["batch", "none"])
def test_composed_front_equals_the_module_in_fp64(channels, size, C, norm):
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    d = 37
    dec = make_decoder(channels, d, C, size, norm, seed=3)
    ex = VanillaDecoderExport(dec, CPU)
    s1 = size // 4
    assert ex.A.shape == (s1 * s1 * channels[1], d) and ex.c.shape == (s1 * s1 * channels[1],)
    assert ex.A.dtype == torch.float32 and ex.tensors["At"].shape[0] == d + 1 and not ex.tensors["At"][d].any()   # even rows
    z = torch.randn(9, d, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    dd = copy.deepcopy(dec).double()
    with torch.no_grad():
        want = dd.deconv1[1](dd.deconv1[0](dd.fc(z).view(9, -1, 4, 4)))              # norm1(ConvT1(fc(z))), before the ReLU
    want = want.permute(0, 2, 3, 1).reshape(9, -1)                                   # column = pixel * c1 + channel
    got = z @ ex.A.double().t() + ex.c.double()
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-6


def _emulate(ex, zs, ze):
    """The kernels' algorithm in fp64 torch from the export's tensors alone (composed front, masks, parity / tap layouts)."""
    T = {k: v.double() for k, v in ex.tensors.items()}
    d, c1, c2, C, S = ex.desc.latent_dim, ex.desc.c1, ex.desc.c2, ex.desc.out_channels, ex.desc.out_size
    w2 = T["w2p"].permute(0, 1, 2, 4, 3).reshape(4, 4, c1, c2)
    w3 = T["w3p"].permute(0, 1, 3, 2)

    def convt(x, w):                                                                 # x [B][s][s][cin] -> [B][2s][2s][cout]
        B, s = x.shape[0], x.shape[1]
        xp = F.pad(x, (0, 0, 1, 1, 1, 1))
        out = torch.zeros(B, 2 * s, 2 * s, w.shape[3], dtype=x.dtype)
        for py in (0, 1):
            for px in (0, 1):
                for a in (0, 1):
                    for b in (0, 1):
                        out[:, py::2, px::2] += xp[:, 1 + py - a:1 + py - a + s, 1 + px - b:1 + px - b + s] @ w[2 * py + px][2 * a + b]
        return out

    def point(z):
        pre1 = (z @ T["At"][:d] + T["c"]).view(-1, S // 4, S // 4, c1)
        pre2 = T["scale2"] * convt(pre1.clamp(min=0), w2) + T["shift2"]
        sig = torch.sigmoid(convt(pre2.clamp(min=0), w3) + T["b3"])
        return pre1 > 0, pre2 > 0, sig * (1 - sig)

    def end(z, delta):
        m1, m2, sp = point(z)
        t1 = (delta @ T["At"][:d]).view(-1, S // 4, S // 4, c1) * m1
        t2 = T["scale2"] * convt(t1, w2) * m2
        return (sp * convt(t2, w3)).flatten(1).norm(dim=1)

    zs, ze = zs.double(), ze.double()
    return (0.5 * (end(zs, ze - zs) + end(ze, ze - zs))).numpy()


@pytest.mark.parametrize("channels,d,C,size,norm", [((256, 128, 64), 21, 1, 28, "batch"), ((128, 64, 32), 6, 3, 32, "none"),
                                                    ((128, 64, 32), 16, 1, 32, "batch")])
def test_export_layouts_reproduce_the_jacobian(channels, d, C, size, norm):
    """Composed front + ReLU masks + parity / tap layouts + folded second norm, evaluated in fp64, against fp64 autograd
    through the module.  The export's tensors are float32 roundings (6e-8 relative each) of fp64 values and everything
    else is fp64, so the lengths agree to about 1e-7; 1e-5 leaves room for an edge next to a ReLU boundary."""
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    dec = make_decoder(channels, d, C, size, norm, seed=11)
    zs, ze = make_edges(d, n_edges=12, seed=4)
    want = autograd_lengths(dec, zs, ze, torch.float64)
    got = _emulate(VanillaDecoderExport(dec, CPU), zs, ze)
    assert np.all(want > 0) and float(np.max(np.abs(got - want) / want)) < 1e-5


@pytest.mark.parametrize("name", list(V.ENVELOPE_CASES))
def test_envelope_cases_export_and_coverage(name):
    """vanilla_jvp_cases.ENVELOPE_CASES on the host: the predicate covers each and not the same module at d = 129; the composed
    front against the module in fp64 (d = 1, 2, odd d with the zero row that makes dp even, a dec_channels[0] other than
    256 / 128, BatchNorm2d(affine=False)); the export's layouts against fp64 autograd as in
    test_export_layouts_reproduce_the_jacobian; both workspace queries non-zero, and zero one step outside make_shape."""
    from vqvae_amd import _lib
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport, vanilla_kernels_cover
    channels, d, C, size, norm = V.ENVELOPE_CASES[name]
    dec = V.build(channels, d, C, size, norm, seed=len(name))
    assert vanilla_kernels_cover(dec) and not vanilla_kernels_cover(V.build(channels, 129, C, size, norm))
    if norm == "batch-plain":
        norms = [m for m in dec.modules() if isinstance(m, nn.BatchNorm2d)]
        assert len(norms) == 2 and all(m.weight is None and m.bias is None and not m.training for m in norms)
    ex = VanillaDecoderExport(dec, CPU)
    s1, c1 = size // 4, channels[1]
    assert (ex.desc.latent_dim, ex.desc.c1, ex.desc.c2, ex.desc.out_channels, ex.desc.out_size) == (d, c1, channels[2], C, size)
    assert ex.A.shape == (s1 * s1 * c1, d) and ex.tensors["At"].shape[0] == d + (d & 1) and not ex.tensors["At"][d:].any()
    z = torch.randn(9, d, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    dd = copy.deepcopy(dec).double()
    with torch.no_grad():
        want = dd.deconv1[1](dd.deconv1[0](dd.fc(z).view(9, -1, 4, 4))).permute(0, 2, 3, 1).reshape(9, -1)
    got = z @ ex.A.double().t() + ex.c.double()
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-6
    zs, ze = make_edges(d, n_edges=12, seed=4)
    want_len = autograd_lengths(dec, zs, ze, torch.float64)
    assert np.all(want_len > 0) and float(np.max(np.abs(_emulate(ex, zs, ze) - want_len) / want_len)) < 1e-5
    lib = _lib.load()
    pairs, edges = lib.geo_vanilla_jvp_workspace_bytes, lib.geo_vanilla_jvp_edges_workspace_bytes
    assert 0 < pairs(ex.desc, 1) < pairs(ex.desc, V.N_EDGES) and 0 < edges(ex.desc, 300, 1500) < pairs(ex.desc, 1500)
    for field, value in (("latent_dim", 129), ("latent_dim", 0), ("out_size", 24 if size == 28 else 36), ("out_channels", 2), ("out_channels", 4)):
        bad = _lib.VanillaDecoderDesc.from_buffer_copy(ex.desc)
        setattr(bad, field, value)
        assert pairs(bad, 100) == 0 and edges(bad, 50, 100) == 0, (field, value)


def test_workspace_queries():
    from vqvae_amd import _lib
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    lib = _lib.load()
    assert lib.geo_version() >= 104
    ex = VanillaDecoderExport(make_decoder((256, 128, 64), 128, 3, 32, "batch"), CPU)
    pairs, edges = lib.geo_vanilla_jvp_workspace_bytes, lib.geo_vanilla_jvp_edges_workspace_bytes
    least = pairs(ex.desc, 1)
    assert 0 < least < pairs(ex.desc, 100) < pairs(ex.desc, 5000) == pairs(ex.desc, 10 ** 7)           # passes bound it
    assert pairs(ex.desc, 0) == least and pairs(ex.desc, -1) == 0
    assert edges(ex.desc, 600, 5000) > 0 and edges(ex.desc, 10 ** 6, 5000) == pairs(ex.desc, 5000)     # few edges: per edge end
    assert edges(ex.desc, 20000, 5000) == pairs(ex.desc, 5000) and edges(ex.desc, 10000, 5000) > pairs(ex.desc, 5000)
    for field, value in (("c1", 96), ("c2", 32), ("latent_dim", 129), ("latent_dim", 0), ("out_channels", 2), ("out_size", 64)):
        bad = _lib.VanillaDecoderDesc.from_buffer_copy(ex.desc)
        setattr(bad, field, value)
        assert pairs(bad, 100) == 0 and edges(bad, 50, 100) == 0, field
    assert pairs(None, 100) == 0
