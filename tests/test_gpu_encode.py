"""The native image encode on the MI355X: geo_image_encode through vqvae_amd.encode against the module
in fp64, the bit-equality rules of the ABI, empty and single batches, the ABI's contract, the reference's encoder fixture, and
the encode_latents CLI end to end.

test_accuracy_against_fp64 prints, per case, the maximum absolute error of mu and of logvar and their ratio to the same
module's float32 error in torch on the CPU (the bound is 8); DESIGN.md section 18 records the figures."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import encode_cases as E

pytestmark = pytest.mark.gpu

GEO_OK, GEO_E_ARG, GEO_E_WORKSPACE = 0, -1, -2


def dev():
    return torch.device("cuda", 0)


def load_case(kind, name):
    """(export on the GPU, x on the GPU, fp64 mu, fp64 logvar, float32-torch error over both outputs, encoder on the CPU)."""
    from vqvae_amd.image_encoder import ImageEncoderExport
    enc, x, mu64, lv64, err_mu, err_lv = E.case(kind, name)
    return ImageEncoderExport(enc, dev()), x.to(dev()), mu64, lv64, max(err_mu, err_lv), enc


def min_workspace(export) -> int:
    from vqvae_amd import _lib
    return int(_lib.load().geo_image_encode_workspace_bytes(export.desc, 1))


def same(a, b) -> bool:
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def rows(pair, lo, hi):
    return pair[0][lo:hi], pair[1][lo:hi]


@pytest.mark.parametrize("kind,name", E.ALL_CASES)
def test_accuracy_against_fp64(kind, name):
    """Every element of mu and of logvar within 8 x the float32-torch error of the same module against fp64 (no ReLU-boundary
    allowance: the map is continuous), for the whole batch and for one image."""
    from vqvae_amd.encode import encode_latents, last_encode_path
    export, x, mu64, lv64, err32, _ = load_case(kind, name)
    mu, logvar = encode_latents(export, x)
    assert last_encode_path() == "hip"
    one = encode_latents(export, x[:1])
    for tag, got, got_one, truth in (("mu", mu, one[0], mu64), ("logvar", logvar, one[1], lv64)):
        assert got.dtype == torch.float32 and got.shape == truth.shape and got.is_cuda
        err = float((got.cpu().double() - truth).abs().max())
        err_one = float((got_one.cpu().double() - truth[:1]).abs().max())
        print(f"{kind} {name} {tag}: n={x.shape[0]} max abs error {err:.3e} (n=1: {err_one:.3e}), float32 torch {err32:.3e}, "
              f"ratio {err / err32:.2f}, magnitude {float(truth.abs().max()):.2f}")
        assert torch.isfinite(got).all()
        assert err <= 8 * err32 and err_one <= 8 * err32, (tag, err, err_one, err32)
        assert torch.equal(got_one, got[:1])


@pytest.mark.parametrize("kind,name", E.ALL_CASES)
def test_bit_equality(kind, name):
    """A row's (mu, logvar) is the same bits alone and at any position of any batch, with the minimum workspace, twice the
    minimum and the default, on a side stream, in two runs, and whether a module or a prepared export is passed."""
    from vqvae_amd.encode import encode_latents, last_encode_path
    export, x, _, _, _, enc = load_case(kind, name)
    n = x.shape[0]
    plain = encode_latents(export, x)
    assert same(encode_latents(export, x), plain), "second run differs"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = encode_latents(export, x)
    torch.cuda.current_stream().wait_stream(side)
    assert same(on_side, plain), "side stream differs"
    nmin = min_workspace(export)
    assert same(encode_latents(export, x, max_workspace_bytes=nmin), plain), "minimum workspace differs"
    assert same(encode_latents(export, x, max_workspace_bytes=2 * nmin), plain), "twice the minimum workspace differs"
    for i in (0, 1, n // 2, n - 1):
        assert same(encode_latents(export, x[i:i + 1]), rows(plain, i, i + 1)), f"row {i} alone differs"
    for size in (5, 64):
        parts = [encode_latents(export, x[i:i + size]) for i in range(0, n, size)]
        assert same((torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])), plain), f"sub-batches of {size} differ"
    moved = torch.cat([x[3:], x[:3]])                                         # every row at another position
    got = encode_latents(export, moved)
    assert same(rows(got, 0, n - 3), rows(plain, 3, n)) and same(rows(got, n - 3, n), rows(plain, 0, 3)), "position matters"
    from_module = encode_latents(copy.deepcopy(enc).to(dev()), x)
    assert last_encode_path() == "hip" and same(from_module, plain), "module and export differ"
    assert same(encode_latents(enc, x.cpu()), plain), "a CPU module with CPU images differs"


def test_empty_and_single_batches():
    from vqvae_amd import _lib
    from vqvae_amd.encode import encode_latents, last_encode_path
    for kind, name, shape in (("vanilla", "narrow-none-28", (16,)), ("spatial", "wide-bn-32x3-d32", (32, 4, 4))):
        export, x, mu64, _, err32, _ = load_case(kind, name)
        mu, logvar = encode_latents(export, x[:0])
        assert last_encode_path() == "hip" and mu.shape == logvar.shape == (0,) + shape and mu.is_cuda and mu.dtype == torch.float32
        mu, logvar = encode_latents(export, x[2:3])
        assert mu.shape == logvar.shape == (1,) + shape
        assert float((mu.cpu().double() - mu64[2:3]).abs().max()) <= 8 * err32
    # n = 0 through the ABI: GEO_OK, nothing is launched or written, null data pointers are not looked at
    lib = _lib.load()
    assert lib.geo_image_encode(export.desc, None, 0, None, None, None, 0, ctypes.c_void_p(0)) == GEO_OK


def test_abi_contract():
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr
    from vqvae_amd.encode import encode_latents
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    for kind, name in (("vanilla", "narrow-none-28"), ("spatial", "narrow-none-28-d5")):
        export, x, _, _, _, _ = load_case(kind, name)
        n, nmin, d = 3, min_workspace(export), export.latent_dim
        x = x[:n].contiguous()
        shape = (n, d, 4, 4) if kind == "spatial" else (n, d)
        mu, logvar = torch.full(shape, 7.0, device=dev()), torch.full(shape, 7.0, device=dev())
        ws = torch.empty(4 * nmin, dtype=torch.uint8, device=dev())

        def call(desc, xp, n_, mu_, lv_, ws_, nbytes):
            return lib.geo_image_encode(desc, xp, n_, mu_, lv_, ws_, nbytes, null)

        assert call(export.desc, ptr(x), 0, ptr(mu), ptr(logvar), ptr(ws), ws.numel()) == GEO_OK      # n = 0: nothing happens
        for change in (dict(latent_dim=129 if kind == "vanilla" else 65), dict(e1=48), dict(in_size=32), dict(in_channels=3)):
            bad = type(export.desc)()
            ctypes.pointer(bad)[0] = export.desc
            for k, v in change.items():
                setattr(bad, k, v)
            assert lib.geo_image_encode_workspace_bytes(bad, n) == 0, change
            assert call(bad, ptr(x), n, ptr(mu), ptr(logvar), ptr(ws), ws.numel()) == GEO_E_ARG, change
            assert b"not covered" in lib.geo_last_error()
        for hole in ("w1p", "shift2", "whp", "bh"):
            holed = type(export.desc)()
            ctypes.pointer(holed)[0] = export.desc
            setattr(holed, hole, None)
            assert call(holed, ptr(x), n, ptr(mu), ptr(logvar), ptr(ws), ws.numel()) == GEO_E_ARG, hole
        assert call(export.desc, None, n, ptr(mu), ptr(logvar), ptr(ws), ws.numel()) == GEO_E_ARG
        assert call(export.desc, ptr(x), n, None, ptr(logvar), ptr(ws), ws.numel()) == GEO_E_ARG
        assert call(export.desc, ptr(x), n, ptr(mu), None, ptr(ws), ws.numel()) == GEO_E_ARG
        assert call(export.desc, ptr(x), n, ptr(mu), ptr(logvar), None, ws.numel()) == GEO_E_ARG
        assert call(export.desc, ptr(x), -1, ptr(mu), ptr(logvar), ptr(ws), ws.numel()) == GEO_E_ARG
        assert call(export.desc, ptr(x), 2 ** 31, ptr(mu), ptr(logvar), ptr(ws), ws.numel()) == GEO_E_ARG
        assert call(export.desc, ptr(x), n, ptr(mu), ptr(logvar), ptr(ws), nmin - 1) == GEO_E_WORKSPACE
        torch.cuda.synchronize()
        assert bool((mu == 7.0).all()) and bool((logvar == 7.0).all()), "a rejected call wrote to the output"
        assert call(export.desc, ptr(x), n, ptr(mu), ptr(logvar), ptr(ws), nmin) == GEO_OK              # the minimum is enough
        torch.cuda.synchronize()
        assert same((mu, logvar), encode_latents(export, x))


def test_reference_fixture(golden):
    """tests/golden/encoder.npz: the batch-norm SpatialVAE encoder on the native route, the GroupNorm one on the torch route,
    both within test_encoder_outputs_equal_reference's tolerance of the reference's outputs."""
    from oracle import synthetic as syn
    from vqvae_amd.encode import encode_latents, last_encode_path
    from vqvae_amd.spatial_vae import SpatialVAE
    g = golden("encoder")
    for name, (cin, size, d, norm, route) in {"fm": (1, 28, 16, "batch", "hip"), "cf": (3, 32, 32, "group", "torch")}.items():
        vae = SpatialVAE(cin, [64, 128, 256], [256, 128, 64], d, "mse", size, norm, mse_use_sigmoid=True)
        vae.load_state_dict(syn.seeded_state_dict(vae.state_dict(), 5))
        x = torch.from_numpy(np.random.RandomState(6).rand(24, cin, size, size).astype(np.float32))
        mu, logvar = encode_latents(vae.eval().to(dev()).encoder, x.to(dev()))
        assert last_encode_path() == route
        np.testing.assert_allclose(mu.cpu().numpy(), g[f"{name}/mu"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(logvar.cpu().numpy(), g[f"{name}/logvar"], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- the CLI end to end

def _write_idx(path, array):
    with open(path, "wb") as f:
        f.write(bytes([0, 0, 0x08, array.ndim]) + b"".join(int(s).to_bytes(4, "big") for s in array.shape) + array.tobytes())


def _tiny_fashionmnist(root):
    """64 images per split in the layout vqvae_amd.eval.data reads."""
    r = np.random.RandomState(9)
    raw = root / "FashionMNIST" / "raw"
    raw.mkdir(parents=True)
    for prefix in ("train", "t10k"):
        _write_idx(raw / f"{prefix}-images-idx3-ubyte", r.randint(0, 256, (64, 28, 28)).astype(np.uint8))
        _write_idx(raw / f"{prefix}-labels-idx1-ubyte", r.randint(0, 10, 64).astype(np.uint8))


def _shake_batchnorm(model):
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))


def _check_cli(tmp_path, capsys, model, writer, config, latent_shape, route, tag, notes):
    """Runs the CLI on `model`'s checkpoint and compares its four files with `writer`'s on the same loader and seed; the
    figures go to `notes` (capsys is emptied before each run of the CLI)."""
    from vqvae_amd.scripts import encode_latents as cli
    from vqvae_amd.training.data import get_data_loaders
    ckpt = tmp_path / f"{tag}.pt"
    torch.save({"model_state_dict": model.state_dict(), "epoch": 1}, ckpt)
    args = ["--checkpoint", str(ckpt), "--dataset", "FashionMNIST", "--data_root", str(tmp_path / "data"), "--split", "val",
            "--out_dir", str(tmp_path / f"{tag}_cli"), "--batch_size", "24", "--seed", "3"]
    capsys.readouterr()
    cli.main(args + (["--config", str(config)] if config else []))
    assert f"encode route: {route}\n" in capsys.readouterr().out
    model = model.to(dev()).eval()
    _, val = get_data_loaders("FashionMNIST", str(tmp_path / "data"), 24, dev())
    torch.manual_seed(3)
    writer(model, val, dev(), tmp_path / f"{tag}_writer")
    for name in ("z", "mu", "logvar"):
        got, want = torch.load(tmp_path / f"{tag}_cli" / f"{name}.pt"), torch.load(tmp_path / f"{tag}_writer" / f"{name}.pt")
        assert got.shape == want.shape == (64,) + latent_shape and got.dtype == want.dtype == torch.float32 and not got.is_cuda
        notes.append(f"{tag} {name}: max abs difference from the writer {float((got - want).abs().max()):.3e} at magnitude "
                     f"{float(want.abs().max()):.2f}")
        assert torch.isfinite(got).all()
        if route == "hip":               # (the torch route is the library's convolutions twice: two runs need not agree to the bit)
            np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-6)
    got_y, want_y = torch.load(tmp_path / f"{tag}_cli" / "y.pt"), torch.load(tmp_path / f"{tag}_writer" / "y.pt")
    assert got_y.dtype == want_y.dtype == torch.int64 and torch.equal(got_y, want_y) and got_y.shape == (64,)


def test_cli_end_to_end(tmp_path, capsys):
    import yaml
    from vqvae_amd.spatial_vae import SpatialVAE
    from vqvae_amd.utils.latents import save_latents
    from vqvae_amd.utils.spatial_latents import save_spatial_latents
    from vqvae_amd.vae import VAE
    _tiny_fashionmnist(tmp_path / "data")
    notes = []
    torch.manual_seed(5)
    vanilla = VAE(in_channels=1, enc_channels=(64, 128, 256), dec_channels=(256, 128, 64), latent_dim=128, norm_type="batch")
    _shake_batchnorm(vanilla)
    _check_cli(tmp_path, capsys, vanilla, save_latents, None, (128,), "hip", "vanilla", notes)

    section = {"in_channels": 1, "enc_channels": [64, 128, 256], "dec_channels": [256, 128, 64], "latent_dim": 16,
               "recon_loss": "mse", "output_image_size": 28, "norm_type": "batch", "mse_use_sigmoid": True, "beta": 1.0}
    (tmp_path / "vae.yaml").write_text(yaml.safe_dump({"model": section, "data": {"name": "FashionMNIST"}}))
    spatial = SpatialVAE(**section)
    _shake_batchnorm(spatial)
    _check_cli(tmp_path, capsys, spatial, save_spatial_latents, tmp_path / "vae.yaml", (16, 4, 4), "hip", "spatial", notes)

    group = dict(section, norm_type="group")
    (tmp_path / "group.yaml").write_text(yaml.safe_dump({"model": group}))
    _check_cli(tmp_path, capsys, SpatialVAE(**group), save_spatial_latents, tmp_path / "group.yaml", (16, 4, 4), "torch", "group", notes)
    print("\n".join(notes))
