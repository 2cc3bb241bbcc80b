"""Host checks of vqvae_amd.eval.lpips: the torch module against a functional restatement, the weights
loader, the preprocessing, the exact zeros, the weight packing, and the flags of the two evaluation CLIs."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

import lpips_cases as LC


def restated(model, x0, x1):
    """LPIPS v0.1 (AlexNet) written out with explicit arguments, in fp64: [n, 5]."""
    w = [(c.weight.detach().double(), c.bias.detach().double()) for c in model.convs]
    shift = torch.tensor([-.030, -.088, -.188], dtype=torch.float32).double().view(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], dtype=torch.float32).double().view(1, 3, 1, 1)

    def feats(x):
        h = (x.double() - shift) / scale
        f1 = F.relu(F.conv2d(h, w[0][0], w[0][1], stride=4, padding=2))
        f2 = F.relu(F.conv2d(F.max_pool2d(f1, kernel_size=3, stride=2, padding=0), w[1][0], w[1][1], stride=1, padding=2))
        f3 = F.relu(F.conv2d(F.max_pool2d(f2, kernel_size=3, stride=2, padding=0), w[2][0], w[2][1], stride=1, padding=1))
        f4 = F.relu(F.conv2d(f3, w[3][0], w[3][1], stride=1, padding=1))
        f5 = F.relu(F.conv2d(f4, w[4][0], w[4][1], stride=1, padding=1))
        return f1, f2, f3, f4, f5

    cols = []
    for a, b, lin in zip(feats(x0), feats(x1), model.lins):
        ua = a / (a.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        ub = b / (b.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        d = F.conv2d((ua - ub).pow(2), lin.detach().double().view(1, -1, 1, 1))          # the package's 1 x 1 lin layer
        cols.append(d.mean(dim=(2, 3)).view(-1))
    return torch.stack(cols, dim=1)


@pytest.mark.parametrize("name", LC.ALL_CASES)
def test_module_equals_functional_restatement(name):
    x0, x1, v64, err32 = LC.case(name)
    want = restated(LC.model(), x0[:16], x1[:16])
    assert v64.dtype == torch.float64 and v64.shape == (LC.N_PAIRS, 6)
    assert float((v64[:16, :5] - want).abs().max()) <= 1e-12
    assert float((v64[:16, 5] - want.sum(dim=1)).abs().max()) <= 1e-12
    assert bool((v64[:, :5] > 0).all()) and bool((err32 > 0).all())
    out = LC.model()(x0[:3], x1[:3])
    assert out.shape == (3, 1, 1, 1) and out.dtype == torch.float32
    assert LC.model()(x0[:3], x1[:3], per_layer=True).shape == (3, 5)


def test_feature_map_sizes():
    x0, _, _, _ = LC.case("c3-64")
    sizes = [tuple(f.shape[1:]) for f in LC.model().features(x0[:1])]
    assert sizes == [(64, 15, 15), (192, 7, 7), (384, 3, 3), (256, 3, 3), (256, 3, 3)]


@pytest.mark.parametrize("layout", ["lpips", "torchvision"])
def test_loader_round_trips_both_layouts(tmp_path, layout):
    from vqvae_amd.eval.lpips import load_lpips_weights
    m = LC.model()
    torch.save(LC.state_dict_for_file(m, layout), tmp_path / "w.pt")
    got = load_lpips_weights(tmp_path / "w.pt")
    assert not got.training
    for a, b in zip(m.state_dict().items(), got.state_dict().items()):
        assert a[0] == b[0] and torch.equal(a[1], b[1]), a[0]
    x0, x1, _, _ = LC.case("c3-64")
    assert torch.equal(got(x0[:4], x1[:4]), m(x0[:4], x1[:4]))


def test_loader_ignores_lins_duplicates(tmp_path):
    from vqvae_amd.eval.lpips import load_lpips_weights
    m = LC.model()
    sd = LC.state_dict_for_file(m)
    for l in range(5):
        sd[f"lins.{l}.model.1.weight"] = torch.full((7,), 9.0)               # wrong shape, wrong values: never looked at
    torch.save(sd, tmp_path / "w.pt")
    got = load_lpips_weights(tmp_path / "w.pt")
    assert all(torch.equal(a, b) for a, b in zip(m.lins, got.lins))
    torch.save(LC.state_dict_for_file(m, with_extras=False), tmp_path / "bare.pt")          # neither lins.* nor scaling_layer.*
    assert all(torch.equal(a, b) for a, b in zip(m.lins, load_lpips_weights(tmp_path / "bare.pt").lins))


def test_loader_names_the_missing_or_misshapen_key(tmp_path):
    from vqvae_amd.eval.lpips import load_lpips_weights
    m = LC.model()
    for layout, key in (("lpips", "net.slice3.6.bias"), ("torchvision", "features.8.weight"), ("lpips", "lin2.model.1.weight")):
        sd = LC.state_dict_for_file(m, layout)
        del sd[key]
        torch.save(sd, tmp_path / "w.pt")
        with pytest.raises(ValueError) as e:
            load_lpips_weights(tmp_path / "w.pt")
        assert f"'{key}' is missing" in str(e.value) and "expected layout" in str(e.value) and "lin4.model.1.weight" in str(e.value)
    sd = LC.state_dict_for_file(m)
    sd["net.slice2.3.weight"] = sd["net.slice2.3.weight"][:, :, :3, :3].clone()
    torch.save(sd, tmp_path / "w.pt")
    with pytest.raises(ValueError, match=r"'net\.slice2\.3\.weight' has shape \[192, 64, 3, 3\], expected \[192, 64, 5, 5\]"):
        load_lpips_weights(tmp_path / "w.pt")
    sd = LC.state_dict_for_file(m)
    sd["lin0.model.1.weight"] = sd["lin0.model.1.weight"].view(-1).clone()
    torch.save(sd, tmp_path / "w.pt")
    with pytest.raises(ValueError, match=r"'lin0\.model\.1\.weight' has shape \[64\], expected \[1, 64, 1, 1\]"):
        load_lpips_weights(tmp_path / "w.pt")
    sd = LC.state_dict_for_file(m)
    sd["scaling_layer.shift"] = torch.tensor([-.03, -.088, -.2]).view(1, 3, 1, 1)
    torch.save(sd, tmp_path / "w.pt")
    with pytest.raises(ValueError, match="scaling_layer.shift"):
        load_lpips_weights(tmp_path / "w.pt")


@pytest.mark.parametrize("channels,size", [(1, 28), (3, 32)])
def test_preprocess_is_the_references_three_lines(channels, size):
    from vqvae_amd.eval.lpips import preprocess_for_lpips
    images = torch.rand((6, channels, size, size), generator=torch.Generator().manual_seed(4))
    want = images.repeat(1, 3, 1, 1) if channels == 1 else images
    want = F.interpolate(want, size=(64, 64), mode="bilinear", align_corners=False)
    want = want * 2 - 1
    got = preprocess_for_lpips(images)
    assert got.shape == (6, 3, 64, 64) and torch.equal(got, want)
    assert preprocess_for_lpips(images, target_size=48).shape == (6, 3, 48, 48)


def test_identical_pairs_give_exactly_zero():
    from vqvae_amd.eval.lpips import last_lpips_path, lpips_mean, lpips_pairs
    x0, _, _, _ = LC.case("c1-28")
    m = LC.model()
    for mod in (m, copy.deepcopy(m).double()):
        out = mod(x0[:9], x0[:9].clone(), per_layer=True)
        assert out.shape == (9, 5) and bool((out == 0.0).all())
    vals = lpips_pairs(m, x0[:9], x0[:9].clone())                            # CPU images: the module's route, f64 out
    assert last_lpips_path() == "torch" and vals.dtype == torch.float64 and vals.shape == (9,) and bool((vals == 0.0).all())
    assert lpips_mean(m, x0[:9], x0[:9].clone()) == 0.0


def test_dead_layer5_column_is_exactly_zero():
    x0, x1, v64, _ = LC.case("c3-32")
    dead = LC.dead_layer5(LC.model())
    for mod in (dead, copy.deepcopy(dead).double()):
        assert all(bool((f == 0).all()) for f in (mod.features(x0[:8])[4], mod.features(x1[:8])[4]))
        layers = mod(x0[:8], x1[:8], per_layer=True)
        assert bool((layers[:, 4] == 0.0).all()) and bool(torch.isfinite(layers).all()) and bool((layers[:, :4] > 0).all())
        assert bool(torch.isfinite(mod(x0[:8], x1[:8])).all())
    assert float((copy.deepcopy(dead).double()(x0[:8], x1[:8], per_layer=True)[:, :4] - v64[:8, :4]).abs().max()) <= 1e-12


def test_lpips_mean_is_the_ascending_fp64_sum():
    from vqvae_amd.eval.lpips import lpips_mean, lpips_pairs
    x0, x1, _, _ = LC.case("c3-64")
    vals = lpips_pairs(LC.model(), x0[:11], x1[:11]).tolist()
    total = 0.0
    for v in vals:
        total += v
    assert lpips_mean(LC.model(), x0[:11], x1[:11]) == total / 11
    layers = lpips_pairs(LC.model(), x0[:11], x1[:11], per_layer=True)
    assert layers.shape == (11, 5) and layers.dtype == torch.float64
    empty = lpips_pairs(LC.model(), x0[:0], x1[:0])
    assert empty.shape == (0,) and empty.dtype == torch.float64
    with pytest.raises(ValueError):
        lpips_pairs(LC.model(), x0[:3], x1[:2])


def test_native_route_is_for_f32_gpu_images_of_64_px():
    from vqvae_amd.eval.lpips import native_lpips_covers
    assert not native_lpips_covers(torch.zeros(2, 3, 64, 64))                # a CPU tensor
    assert not native_lpips_covers(torch.zeros(3, 64, 64))


def test_weight_packing_matches_the_header():
    """The two layouts of geo_lpips_alex_desc, element by element on a few indices."""
    from vqvae_amd.eval import lpips as L
    w1 = LC.model().convs[0].weight.detach()
    p1 = L._first(w1)
    assert p1.shape == (33, 2, 64, 8)
    for c, ky, h, co, s in ((0, 0, 0, 0, 0), (2, 10, 1, 63, 4), (1, 5, 0, 17, 5), (1, 3, 1, 40, 2)):
        assert p1[c * 11 + ky, h, co, s] == w1[co, c, ky, 2 * s + h]
    assert bool((p1[:, 1, :, 5] == 0).all()) and bool((p1[..., 6:] == 0).all())
    assert float(p1.abs().sum()) == pytest.approx(float(w1.abs().sum()), rel=1e-6)
    w2 = LC.model().convs[1].weight.detach()
    p2 = L._taps(w2)
    assert p2.shape == (25, 16, 192, 4)
    for ky, kx, q, co, r in ((0, 0, 0, 0, 0), (4, 4, 15, 191, 3), (2, 3, 7, 100, 1)):
        assert p2[5 * ky + kx, q, co, r] == w2[co, 4 * q + r, ky, kx]
    assert L._taps(LC.model().convs[3].weight.detach()).shape == (9, 96, 256, 4)


def test_abi_declares_the_lpips_entry_points():
    from vqvae_amd import _lib
    lib = _lib.load()
    assert lib.geo_version() >= 109
    assert {"geo_lpips_alex", "geo_lpips_alex_workspace_bytes"} <= set(_lib.EXPORTS)
    assert ctypes.sizeof(_lib.LPIPSAlexDesc) == 15 * ctypes.sizeof(ctypes.c_void_p)
    per_pair = 2 * 31872 * 4
    assert lib.geo_lpips_alex_workspace_bytes(1) == per_pair and lib.geo_lpips_alex_workspace_bytes(0) == per_pair
    assert lib.geo_lpips_alex_workspace_bytes(100) == 100 * per_pair
    assert lib.geo_lpips_alex_workspace_bytes(10 ** 6) == 4096 * per_pair
    # argument checks come before anything touches the GPU
    assert lib.geo_lpips_alex(None, None, None, 3, None, None, None, 0, None) == -1
    assert b"null descriptor" in lib.geo_last_error()


def test_both_clis_list_the_flag(capsys):
    from vqvae_amd.scripts import evaluate_baseline, evaluate_model
    assert "--lpips_weights" in evaluate_model.make_parser().format_help()
    assert evaluate_model.make_parser().parse_args(["--config", "c.yaml"]).lpips_weights is None
    with pytest.raises(SystemExit):
        evaluate_baseline.main(["--help"])
    assert "--lpips_weights" in capsys.readouterr().out


def test_results_dict_writes_the_rounded_key():
    from vqvae_amd.scripts.evaluate_baseline import results_dict
    cb = {"entropy": 1.0, "used": 3, "dead_codes": 1}
    plain = results_dict(20.0, 0.5, 10, 11.0, 0.25, 10, 1, cb, 4)
    assert "lpips" not in plain["generation_quality"]
    with_lpips = results_dict(20.0, 0.5, 10, 11.0, 0.25, 10, 1, cb, 4, gen_lpips=0.12345678)
    assert with_lpips["generation_quality"]["lpips"] == 0.123457
    del with_lpips["generation_quality"]["lpips"]
    assert with_lpips == plain
    with pytest.raises(TypeError):
        results_dict(20.0, 0.5, 10, 11.0, 0.25, 10, 1, cb, 4, 0.1)            # keyword-only
