"""The native LPIPS on the MI355X: geo_lpips_alex through vqvae_amd.eval.lpips against the torch module
in fp64, the bit-equality rules of the ABI, the exact zeros, empty batches and the ABI's contract, the two routes, and
evaluate_model end to end.

test_accuracy_against_fp64 prints, per case and column (the five layers, then the total), the maximum absolute error over the
pairs and its ratio to the float32 module's error on the CPU in the same column (the bound is 8); DESIGN.md section 19 records
the figures."""
import copy
import ctypes
import gzip

import numpy as np
import pytest
import torch

import lpips_cases as LC

pytestmark = pytest.mark.gpu

GEO_OK, GEO_E_ARG, GEO_E_WORKSPACE = 0, -1, -2
COLUMNS = ("layer1", "layer2", "layer3", "layer4", "layer5", "total")


def dev():
    return torch.device("cuda", 0)


_exports = {}


def export():
    from vqvae_amd.eval.lpips import LPIPSExport
    if "e" not in _exports:
        _exports["e"] = LPIPSExport(LC.model(), dev())
    return _exports["e"]


def both(obj, x0, x1, **kw):
    """[n, 6]: the five layer values and the total, from two calls."""
    from vqvae_amd.eval.lpips import lpips_pairs
    layers = lpips_pairs(obj, x0, x1, per_layer=True, **kw)
    total = lpips_pairs(obj, x0, x1, **kw)
    assert layers.dtype == total.dtype == torch.float64 and layers.is_cuda and total.is_cuda
    assert layers.shape == (x0.shape[0], 5) and total.shape == (x0.shape[0],)
    return torch.cat([layers, total.view(-1, 1)], dim=1)


@pytest.mark.parametrize("name", LC.ALL_CASES)
def test_accuracy_against_fp64(name):
    """Every pair's total and every per-layer value within 8 x the float32 CPU module's own maximum error against the fp64
    module in the same column (no ReLU-boundary allowance: the map is continuous), for the whole batch and for n = 1."""
    from vqvae_amd.eval.lpips import last_lpips_path
    x0, x1, v64, err32 = LC.case(name)
    g0, g1 = x0.to(dev()), x1.to(dev())
    got = both(export(), g0, g1)
    assert last_lpips_path() == "hip"
    one = both(export(), g0[:1], g1[:1])
    assert bool(torch.isfinite(got).all())
    err = (got.cpu() - v64).abs().max(dim=0).values
    err_one = (one.cpu() - v64[:1]).abs().max(dim=0).values
    for k, tag in enumerate(COLUMNS):
        print(f"{name} {tag}: n={x0.shape[0]} max abs error {float(err[k]):.3e} (n=1: {float(err_one[k]):.3e}), float32 torch "
              f"{float(err32[k]):.3e}, ratio {float(err[k] / err32[k]):.2f}, magnitude {float(v64[:, k].min()):.2e} .. "
              f"{float(v64[:, k].max()):.2e}")
    for k, tag in enumerate(COLUMNS):
        assert float(err[k]) <= 8 * float(err32[k]) and float(err_one[k]) <= 8 * float(err32[k]), (tag, err[k], err_one[k], err32[k])
    assert torch.equal(one, got[:1])
    layer_sum = got[:, 0]
    for k in range(1, 5):
        layer_sum = layer_sum + got[:, k]
    assert torch.equal(layer_sum, got[:, 5]), "the total is the layer values added in layer order"


@pytest.mark.parametrize("name", LC.ALL_CASES)
def test_bit_equality(name):
    """A pair's values are the same bits alone and at any position of any batch, with the minimum workspace, twice the minimum
    and the default, on a side stream, in two runs, with x0 and x1 swapped, and whether a module or an export is passed."""
    from vqvae_amd import _lib
    from vqvae_amd.eval.lpips import last_lpips_path
    x0, x1, _, _ = LC.case(name)
    x0, x1 = x0.to(dev()), x1.to(dev())
    n = x0.shape[0]
    e = export()
    plain = both(e, x0, x1)
    assert torch.equal(both(e, x0, x1), plain), "second run differs"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = both(e, x0, x1)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(on_side, plain), "side stream differs"
    nmin = int(_lib.load().geo_lpips_alex_workspace_bytes(1))
    assert torch.equal(both(e, x0, x1, max_workspace_bytes=nmin), plain), "minimum workspace differs"
    assert torch.equal(both(e, x0, x1, max_workspace_bytes=2 * nmin), plain), "twice the minimum workspace differs"
    assert torch.equal(both(e, x0, x1, max_workspace_bytes=9 * nmin + 100), plain), "a workspace of nine pairs differs"
    for i in (0, 1, n // 2, n - 1):
        assert torch.equal(both(e, x0[i:i + 1], x1[i:i + 1]), plain[i:i + 1]), f"row {i} alone differs"
    for size in (5, 64):
        parts = [both(e, x0[i:i + size], x1[i:i + size]) for i in range(0, n, size)]
        assert torch.equal(torch.cat(parts), plain), f"sub-batches of {size} differ"
    got = both(e, torch.cat([x0[3:], x0[:3]]), torch.cat([x1[3:], x1[:3]]))                # every row at another position
    assert torch.equal(got[:n - 3], plain[3:]) and torch.equal(got[n - 3:], plain[:3]), "position matters"
    assert torch.equal(both(e, x1, x0), plain), "swapping x0 and x1 changes a value"
    from_module = both(copy.deepcopy(LC.model()).to(dev()), x0, x1)
    assert last_lpips_path() == "hip" and torch.equal(from_module, plain), "module and export differ"
    assert torch.equal(both(LC.model(), x0, x1), plain), "a CPU module with GPU images differs"


def test_large_batches_equal_small_ones():
    """520 and 910 pairs (grids of several hundred groups per layer instead of a few dozen) keep, pair by pair, the bits of the
    batch of 130, also when a capped workspace cuts the 910 into passes of 100."""
    from vqvae_amd import _lib
    x0, x1, _, _ = LC.case("c3-64")
    x0, x1 = x0.to(dev()), x1.to(dev())
    e = export()
    plain = both(e, x0, x1)
    for times in (4, 7):
        got = both(e, x0.repeat(times, 1, 1, 1), x1.repeat(times, 1, 1, 1))
        assert torch.equal(got, plain.repeat(times, 1)), f"{times * x0.shape[0]} pairs differ from {x0.shape[0]}"
    nmin = int(_lib.load().geo_lpips_alex_workspace_bytes(1))
    got = both(e, x0.repeat(7, 1, 1, 1), x1.repeat(7, 1, 1, 1), max_workspace_bytes=100 * nmin)
    assert torch.equal(got, plain.repeat(7, 1)), "passes of 100 pairs differ"


def test_exact_zeros():
    from vqvae_amd.eval.lpips import LPIPSExport, last_lpips_path
    x0, x1, v64, err32 = LC.case("c1-28")
    x0, x1 = x0.to(dev()), x1.to(dev())
    same = both(export(), x0, x0.clone())
    assert last_lpips_path() == "hip" and bool((same == 0.0).all()), "identical pairs must give exactly 0.0"
    dead = both(LPIPSExport(LC.dead_layer5(LC.model()), dev()), x0, x1)
    assert bool((dead[:, 4] == 0.0).all()) and bool(torch.isfinite(dead).all()) and bool((dead[:, :4] > 0).all())
    alive = both(export(), x0, x1)
    assert torch.equal(dead[:, :4], alive[:, :4]) and bool((alive[:, 4] > 0).all())


def test_empty_batch_and_abi_contract():
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr
    from vqvae_amd.eval.lpips import last_lpips_path, lpips_pairs
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    e = export()
    x0, x1, _, _ = LC.case("c3-64")
    n = 3
    x0, x1 = x0[:n].to(dev()).contiguous(), x1[:n].to(dev()).contiguous()
    empty = lpips_pairs(e, x0[:0], x1[:0])
    assert last_lpips_path() == "hip" and empty.shape == (0,) and empty.dtype == torch.float64 and empty.is_cuda
    assert lpips_pairs(e, x0[:0], x1[:0], per_layer=True).shape == (0, 5)
    # n = 0 through the ABI: GEO_OK, nothing is launched or written, null data pointers are not looked at
    assert lib.geo_lpips_alex(e.desc, None, None, 0, None, None, None, 0, null) == GEO_OK

    nmin = int(lib.geo_lpips_alex_workspace_bytes(1))
    total = torch.full((n,), 7.0, dtype=torch.float64, device=dev())
    layers = torch.full((n, 5), 7.0, dtype=torch.float64, device=dev())
    ws = torch.empty(4 * nmin, dtype=torch.uint8, device=dev())

    def call(desc, a, b, n_, t, l, w, nbytes):
        return lib.geo_lpips_alex(desc, a, b, n_, t, l, w, nbytes, null)

    assert call(e.desc, ptr(x0), ptr(x1), 0, ptr(total), ptr(layers), ptr(ws), ws.numel()) == GEO_OK
    assert call(None, ptr(x0), ptr(x1), n, ptr(total), ptr(layers), ptr(ws), ws.numel()) == GEO_E_ARG
    assert b"null descriptor" in lib.geo_last_error()
    for hole in ("w1p", "b3", "w5p", "lin4"):
        holed = type(e.desc)()
        ctypes.pointer(holed)[0] = e.desc
        setattr(holed, hole, None)
        assert call(holed, ptr(x0), ptr(x1), n, ptr(total), ptr(layers), ptr(ws), ws.numel()) == GEO_E_ARG, hole
    assert call(e.desc, None, ptr(x1), n, ptr(total), ptr(layers), ptr(ws), ws.numel()) == GEO_E_ARG
    assert call(e.desc, ptr(x0), None, n, ptr(total), ptr(layers), ptr(ws), ws.numel()) == GEO_E_ARG
    assert call(e.desc, ptr(x0), ptr(x1), n, None, ptr(layers), ptr(ws), ws.numel()) == GEO_E_ARG
    assert call(e.desc, ptr(x0), ptr(x1), n, ptr(total), ptr(layers), None, ws.numel()) == GEO_E_ARG
    assert call(e.desc, ptr(x0), ptr(x1), -1, ptr(total), ptr(layers), ptr(ws), ws.numel()) == GEO_E_ARG
    assert call(e.desc, ptr(x0), ptr(x1), 2 ** 31, ptr(total), ptr(layers), ptr(ws), ws.numel()) == GEO_E_ARG
    assert call(e.desc, ptr(x0), ptr(x1), n, ptr(total), ptr(layers), ptr(ws), nmin - 1) == GEO_E_WORKSPACE
    assert b"below the minimum" in lib.geo_last_error()
    torch.cuda.synchronize()
    assert bool((total == 7.0).all()) and bool((layers == 7.0).all()), "a rejected call wrote to the output"
    assert call(e.desc, ptr(x0), ptr(x1), n, ptr(total), None, ptr(ws), nmin) == GEO_OK          # the minimum is enough; no layer output
    torch.cuda.synchronize()
    assert torch.equal(total, lpips_pairs(e, x0, x1)) and bool((layers == 7.0).all())
    assert call(e.desc, ptr(x0), ptr(x1), n, ptr(total), ptr(layers), ptr(ws), nmin) == GEO_OK
    torch.cuda.synchronize()
    assert torch.equal(layers, lpips_pairs(e, x0, x1, per_layer=True))


def test_routes():
    from vqvae_amd.eval.lpips import last_lpips_path, lpips_mean, lpips_pairs, native_lpips_covers
    model = copy.deepcopy(LC.model()).to(dev())
    x0, x1, v64, _ = LC.case("c3-64")
    g0, g1 = x0[:6].to(dev()), x1[:6].to(dev())
    assert native_lpips_covers(g0) and not native_lpips_covers(g0.double()) and not native_lpips_covers(g0.cpu())
    vals = lpips_pairs(model, g0, g1)
    assert last_lpips_path() == "hip"
    total = 0.0
    for v in vals.cpu().tolist():
        total += v
    assert lpips_mean(model, g0, g1) == total / 6
    g = torch.Generator().manual_seed(8)
    b0, b1 = (torch.rand((4, 3, 96, 96), generator=g) * 2 - 1).to(dev()), (torch.rand((4, 3, 96, 96), generator=g) * 2 - 1).to(dev())
    assert not native_lpips_covers(b0)
    big = lpips_pairs(model, b0, b1)
    assert last_lpips_path() == "torch" and big.dtype == torch.float64 and big.shape == (4,) and big.is_cuda
    # equals the module: the float32 module on the GPU against the fp64 module on the CPU, 1e-5 relative (float32 rounding of
    # chains of at most 3456 terms; two runs of the library's convolutions need not agree to the bit)
    with torch.no_grad():
        again = model(b0, b1).view(-1).double()
        want = copy.deepcopy(LC.model()).double()(b0.cpu(), b1.cpu()).view(-1)
    assert float((big.cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    assert float((big - again).abs().max()) <= 1e-5 * float(want.abs().max())
    with pytest.raises(ValueError):
        lpips_pairs(export(), b0, b1)                                          # an export is for the native shape only


# ---------------------------------------------------------------- evaluate_model end to end

E2E_SEED = 2


def _write_idx_gz(path, array):
    with gzip.open(str(path) + ".gz", "wb") as f:
        f.write(bytes([0, 0, 0x08, array.ndim]) + b"".join(int(s).to_bytes(4, "big") for s in array.shape) + array.tobytes())


def e2e_inputs(root, seed):
    """A FashionMNIST-format test split of 40 images (four per class) as idx .gz files, a 10 x 2 grid PNG of 28-px cells, a seeded
    weights file and the config; returns the config's path."""
    import yaml
    from PIL import Image
    r = np.random.RandomState(100 + seed)
    raw = root / "data" / "FashionMNIST" / "raw"
    raw.mkdir(parents=True)
    _write_idx_gz(raw / "t10k-images-idx3-ubyte", r.randint(0, 256, (40, 28, 28)).astype(np.uint8))
    _write_idx_gz(raw / "t10k-labels-idx1-ubyte", (np.arange(40) % 10).astype(np.uint8))
    Image.fromarray(r.randint(0, 256, (280, 56, 3)).astype(np.uint8)).save(root / "grid.png")
    torch.save(LC.state_dict_for_file(LC.make_model(seed)), root / "alex.pt")
    config = {"generated_path": str(root / "grid.png"), "num_samples": 20, "samples_per_class": 2, "image_size": 28,
              "dataset_name": "fashionmnist", "out_dir": str(root / "out")}
    (root / "evaluate.yaml").write_text(yaml.safe_dump(config))
    return root / "evaluate.yaml", config


def e2e_truth(root, config, seed) -> float:
    """The fp64 module's mean on the CPU over the images as the CLI loads them."""
    from vqvae_amd.eval.lpips import preprocess_for_lpips
    from vqvae_amd.scripts.evaluate_model import load_images
    generated = load_images(config["generated_path"], 20, 28, "fashionmnist", is_real_data=False, samples_per_class=2)
    real = load_images("fashionmnist", 20, 28, "fashionmnist", is_real_data=True, samples_per_class=2, data_root=str(root / "data"))
    with torch.no_grad():
        vals = LC.make_model(seed).double()(preprocess_for_lpips(generated), preprocess_for_lpips(real)).view(-1).tolist()
    total = 0.0
    for v in vals:
        total += v
    return total / len(vals)


def test_evaluate_model_end_to_end(tmp_path, capsys):
    import yaml
    from vqvae_amd.scripts import evaluate_model
    config_path, config = e2e_inputs(tmp_path, E2E_SEED)
    v64 = e2e_truth(tmp_path, config, E2E_SEED)
    # admission: the value is not within 0.01 units of the fourth decimal of a rounding boundary, so the string is decided
    frac = (v64 * 1e4) % 1.0
    print(f"evaluate_model: fp64 LPIPS {v64:.10f}, {abs(frac - 0.5):.3f} of the fourth decimal from a rounding boundary")
    assert v64 > 0 and abs(frac - 0.5) > 0.01, "choose another E2E_SEED"
    capsys.readouterr()
    assert evaluate_model.main(str(config_path), str(tmp_path / "data"), str(tmp_path / "alex.pt")) == 0
    out = capsys.readouterr().out
    with open(tmp_path / "out" / "metrics.yaml") as f:
        with_lpips = yaml.safe_load(f)
    assert set(with_lpips) == {"PSNR", "SSIM", "LPIPS"}
    assert with_lpips["LPIPS"] == f"{v64:.4f}"
    assert f"PSNR: {with_lpips['PSNR']}, SSIM: {with_lpips['SSIM']}, LPIPS: {with_lpips['LPIPS']}\n" in out
    assert "LPIPS not computed" not in out

    # the config key works like the flag, and the flag wins over it
    (tmp_path / "keyed.yaml").write_text(yaml.safe_dump(dict(config, lpips_weights=str(tmp_path / "alex.pt"), out_dir=str(tmp_path / "keyed"))))
    assert evaluate_model.main(str(tmp_path / "keyed.yaml"), str(tmp_path / "data")) == 0
    with open(tmp_path / "keyed" / "metrics.yaml") as f:
        assert yaml.safe_load(f) == with_lpips
    (tmp_path / "wrong.yaml").write_text(yaml.safe_dump(dict(config, lpips_weights=str(tmp_path / "missing.pt"), out_dir=str(tmp_path / "won"))))
    assert evaluate_model.main(str(tmp_path / "wrong.yaml"), str(tmp_path / "data"), str(tmp_path / "alex.pt")) == 0
    with open(tmp_path / "won" / "metrics.yaml") as f:
        assert yaml.safe_load(f) == with_lpips

    # without weights: the two keys and the two lines of before
    capsys.readouterr()
    (tmp_path / "plain.yaml").write_text(yaml.safe_dump(dict(config, out_dir=str(tmp_path / "plain"))))
    assert evaluate_model.main(str(tmp_path / "plain.yaml"), str(tmp_path / "data")) == 0
    out = capsys.readouterr().out
    with open(tmp_path / "plain" / "metrics.yaml") as f:
        plain = yaml.safe_load(f)
    assert plain == {"PSNR": with_lpips["PSNR"], "SSIM": with_lpips["SSIM"]}
    assert out.startswith(f"PSNR: {plain['PSNR']}, SSIM: {plain['SSIM']}\nLPIPS not computed: it needs AlexNet weights, which are "
                          "not available here\n")


# ---------------------------------------------------------------- evaluate_baseline with the flag

def test_evaluate_baseline_writes_lpips(tmp_path, capsys):
    """An untrained baseline VQ-VAE on a synthetic CIFAR-10 directory: with --lpips_weights the reference's key, yaml entry and
    two printed lines appear and agree with each other; without it the files have the keys of before."""
    import json
    import pickle
    import yaml
    from vqvae_amd.baseline.model import model_from_config
    from vqvae_amd.scripts import evaluate_baseline
    r = np.random.RandomState(0)
    d = tmp_path / "data" / "cifar-10-batches-py"
    d.mkdir(parents=True)
    with open(d / "test_batch", "wb") as f:
        pickle.dump({"data": r.randint(0, 256, (20, 3072)).astype(np.uint8), "labels": (np.arange(20) % 10).tolist()}, f)
    cfg = {"seed": 42,
           "data": {"root": str(tmp_path / "data"), "num_workers": 0, "img_size": 32, "normalize_mean": [0.5] * 3,
                    "normalize_std": [0.5] * 3},
           "train": {"batch_size": 8, "epochs": 1, "lr": 2e-4, "weight_decay": 0.0, "grad_clip": 1.0, "amp": False},
           "model": {"in_channels": 3, "z_channels": 32, "hidden": 64, "n_res_blocks": 2, "n_codes": 64, "beta": 0.25,
                     "ema_decay": 0.99, "ema_eps": 1e-5},
           "log": {"samples_every": 1, "save_best": True}}
    torch.manual_seed(0)
    torch.save({"model": model_from_config(cfg).state_dict(), "cfg": cfg, "epoch": 0}, tmp_path / "ckpt.pt")
    torch.save(LC.state_dict_for_file(LC.model()), tmp_path / "alex.pt")
    common = ["--checkpoint", str(tmp_path / "ckpt.pt"), "--max_samples", "16", "--gen_samples", "20"]
    capsys.readouterr()
    assert evaluate_baseline.main(common + ["--out_dir", str(tmp_path / "with"), "--lpips_weights", str(tmp_path / "alex.pt")]) == 0
    out = capsys.readouterr().out
    res = json.load(open(tmp_path / "with" / "evaluation_results.json"))
    value = res["generation_quality"]["lpips"]
    assert isinstance(value, float) and 0.0 < value < 1.0 and value == float(f"{value:.6f}")
    with open(tmp_path / "with" / "metrics.yaml") as f:
        metrics = yaml.safe_load(f)
    assert set(metrics) == {"PSNR", "SSIM", "LPIPS"} and abs(float(metrics["LPIPS"]) - value) <= 5.1e-5
    assert f"LPIPS: {metrics['LPIPS']}\n" in out and f"   LPIPS (vs Real): {metrics['LPIPS']}\n" in out
    assert "LPIPS not available" not in out
    assert evaluate_baseline.main(common + ["--out_dir", str(tmp_path / "without")]) == 0
    out = capsys.readouterr().out
    plain = json.load(open(tmp_path / "without" / "evaluation_results.json"))
    assert "lpips" not in plain["generation_quality"] and "WARNING: LPIPS not available (not computed by this port)\n" in out
    del res["generation_quality"]["lpips"]
    assert plain == res
    with open(tmp_path / "without" / "metrics.yaml") as f:
        assert yaml.safe_load(f) == {"PSNR": metrics["PSNR"], "SSIM": metrics["SSIM"]}
