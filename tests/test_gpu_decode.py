"""The native image decode on the MI355X: geo_vanilla_decode / geo_spatial_decode through
vqvae_amd.decode against the module in fp64, the bit-equality rules of the ABI, the 28-px crop, the ABI's contract, and the
codebook_sampling CLI end to end.

test_accuracy_against_fp64 prints, per case, the maximum absolute logit error and its ratio to the same module's float32 error
in torch on the CPU (the bound is 8); DESIGN.md section 17 records the figures."""
import copy
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

import decode_cases as D
import vanilla_jvp_cases as V

pytestmark = pytest.mark.gpu

GEO_OK, GEO_E_ARG, GEO_E_WORKSPACE = 0, -1, -2
ALL_CASES = [("vanilla", n) for n in V.CASES] + [("spatial", n) for n in D.SPATIAL_CASES]


def dev():
    return torch.device("cuda", 0)


def load_case(kind, name):
    """(export on the GPU, z on the GPU, fp64 truth, float32-torch error, decoder on the CPU)."""
    from vqvae_amd.spatial_decoder import SpatialImageDecoderExport
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    dec, z, truth, err32 = D.vanilla_case(name) if kind == "vanilla" else D.spatial_case(name)
    export = (VanillaDecoderExport if kind == "vanilla" else SpatialImageDecoderExport)(dec, dev())
    return export, z.to(dev()), truth, err32, dec


def min_workspace(kind, export) -> int:
    from vqvae_amd import _lib
    lib = _lib.load()
    query = lib.geo_vanilla_decode_workspace_bytes if kind == "vanilla" else lib.geo_spatial_decode_workspace_bytes
    return int(query(export.desc, 1))


@pytest.mark.parametrize("kind,name", ALL_CASES)
def test_accuracy_against_fp64(kind, name):
    """Every logit within 8 x the float32-torch error of the same module (no ReLU-boundary allowance: the primal is
    continuous), for the whole batch and for one row."""
    from vqvae_amd.decode import decode_logits, last_decode_path
    export, z, truth, err32, _ = load_case(kind, name)
    got = decode_logits(export, z)
    assert last_decode_path() == "hip" and got.dtype == torch.float32 and got.shape == truth.shape and got.is_cuda
    err = float((got.cpu().double() - truth).abs().max())
    one = decode_logits(export, z[:1])
    err_one = float((one.cpu().double() - truth[:1]).abs().max())
    print(f"{kind} {name}: n={z.shape[0]} max abs error {err:.3e} (n=1: {err_one:.3e}), float32 torch {err32:.3e}, "
          f"ratio {err / err32:.2f}, logit magnitude {float(truth.abs().max()):.2f}")
    assert torch.isfinite(got).all()
    assert err <= 8 * err32 and err_one <= 8 * err32, (err, err_one, err32)
    assert torch.equal(one, got[:1])


@pytest.mark.parametrize("kind,name", ALL_CASES)
def test_bit_equality(kind, name):
    """The same call twice, a side stream, the minimum workspace, rows alone and in two sub-batches, and the latent arriving
    through index / (table, codes): all bit-equal to the plain call."""
    from vqvae_amd.decode import decode_logits
    export, z, _, _, _ = load_case(kind, name)
    n = z.shape[0]
    plain = decode_logits(export, z)
    assert torch.equal(decode_logits(export, z), plain), "second run differs"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = decode_logits(export, z)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(on_side, plain), "side stream differs"
    assert torch.equal(decode_logits(export, z, max_workspace_bytes=min_workspace(kind, export)), plain), "minimum workspace differs"
    for i in (0, n // 2, n - 1):
        assert torch.equal(decode_logits(export, z[i:i + 1]), plain[i:i + 1]), f"row {i} alone differs"
    cut = 13
    assert torch.equal(torch.cat([decode_logits(export, z[:cut]), decode_logits(export, z[cut:])]), plain), "sub-batches differ"
    g = torch.Generator().manual_seed(7)
    if kind == "vanilla":
        perm = torch.randperm(n, generator=g).to(z.device)
        codes = torch.argsort(perm)                                           # z[perm][codes[i]] = z[i]
        assert torch.equal(decode_logits(export, table=z[perm].contiguous(), codes=codes), plain), "index route differs"
        assert torch.equal(decode_logits(export, table=z[perm].contiguous(), codes=codes.int(),
                                         max_workspace_bytes=min_workspace(kind, export)), plain)
    else:
        K = 11
        table = torch.randn(K, z.shape[1], generator=g).to(z.device)
        codes = torch.randint(0, K, (n, 4, 4), generator=g).to(z.device)
        grid = table[codes].permute(0, 3, 1, 2).contiguous()
        want = decode_logits(export, grid)
        assert torch.equal(decode_logits(export, table=table, codes=codes), want), "(table, codes) route differs"
        assert torch.equal(decode_logits(export, table=table, codes=codes[5:6]), want[5:6])


@pytest.mark.parametrize("name", ["wide-bn-28-d16", "narrow-none-28-d5"])
def test_28px_is_the_crop_of_32px(name):
    from vqvae_amd.decode import decode_logits
    from vqvae_amd.spatial_decoder import SpatialDecoder
    channels, d, C, size, norm = D.SPATIAL_CASES[name]
    assert size == 28
    dec28, z, _, _ = D.spatial_case(name)
    dec32 = SpatialDecoder(C, channels, d, 32, norm)
    dec32.load_state_dict(dec28.state_dict())
    dec32.eval()
    small, big = decode_logits(copy.deepcopy(dec28).to(dev()), z.to(dev())), decode_logits(dec32.to(dev()), z.to(dev()))
    assert small.shape[-2:] == (28, 28) and big.shape[-2:] == (32, 32)
    assert torch.equal(small, big[:, :, 2:30, 2:30])


def test_abi_contract():
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    for kind, name in (("vanilla", "narrow-none-28"), ("spatial", "narrow-none-28-d5")):
        export, z, _, _, _ = load_case(kind, name)
        n, nmin = 3, min_workspace(kind, export)
        z = z[:n].contiguous()
        out = torch.full((n,) + ((1, 28, 28)), 7.0, device=dev())
        ws = torch.empty(4 * nmin, dtype=torch.uint8, device=dev())

        def call(desc, zp, n_, out_, ws_, nbytes):
            if kind == "vanilla":
                return lib.geo_vanilla_decode(desc, zp, None, n_, out_, ws_, nbytes, null)
            return lib.geo_spatial_decode(desc, zp, None, None, n_, out_, ws_, nbytes, null)

        assert call(export.desc, ptr(z), 0, ptr(out), ptr(ws), ws.numel()) == GEO_OK          # n = 0: nothing happens
        assert call(export.desc, None, 0, None, None, 0) == GEO_OK
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
        bad = type(export.desc)()
        ctypes.pointer(bad)[0] = export.desc
        bad.latent_dim = 200
        assert call(bad, ptr(z), n, ptr(out), ptr(ws), ws.numel()) == GEO_E_ARG
        assert b"not covered" in lib.geo_last_error()
        holed = type(export.desc)()
        ctypes.pointer(holed)[0] = export.desc
        holed.w2p = None
        assert call(holed, ptr(z), n, ptr(out), ptr(ws), ws.numel()) == GEO_E_ARG
        assert call(export.desc, None, n, ptr(out), ptr(ws), ws.numel()) == GEO_E_ARG
        assert call(export.desc, ptr(z), n, None, ptr(ws), ws.numel()) == GEO_E_ARG
        assert call(export.desc, ptr(z), n, ptr(out), None, ws.numel()) == GEO_E_ARG
        assert call(export.desc, ptr(z), -1, ptr(out), ptr(ws), ws.numel()) == GEO_E_ARG
        if kind == "spatial":                                                                  # both z and (table, codes)
            codes = torch.zeros(n, 16, dtype=torch.int32, device=dev())
            assert lib.geo_spatial_decode(export.desc, ptr(z), ptr(z), ptr(codes), n, ptr(out), ptr(ws), ws.numel(), null) == GEO_E_ARG
            assert lib.geo_spatial_decode(export.desc, None, ptr(z), None, n, ptr(out), ptr(ws), ws.numel(), null) == GEO_E_ARG
        assert call(export.desc, ptr(z), n, ptr(out), ptr(ws), nmin - 1) == GEO_E_WORKSPACE
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "a rejected call wrote to the output"
        assert call(export.desc, ptr(z), n, ptr(out), ptr(ws), nmin) == GEO_OK                  # the minimum is enough
        torch.cuda.synchronize()
        from vqvae_amd.decode import decode_logits
        assert torch.equal(out, decode_logits(export, z))


def test_decode_logits_checks_codes_and_keeps_the_torch_route():
    from vqvae_amd.decode import decode_images, decode_logits, last_decode_path
    export, z, _, _, _ = load_case("spatial", "wide-bn-28-d16")
    table = torch.randn(8, 16, device=dev())
    with pytest.raises(ValueError):
        decode_logits(export, table=table, codes=torch.full((2, 4, 4), 8, device=dev()))
    vexport, vz, _, _, _ = load_case("vanilla", "narrow-none-28")
    with pytest.raises(ValueError):
        decode_logits(vexport, table=vz, codes=torch.tensor([0, vz.shape[0]], device=dev()))
    assert decode_logits(export, z[:0]).shape == (0, 1, 28, 28)
    # GroupNorm: no kernel, the module itself in eval() under no_grad -- from a module left in train mode, which stays so.
    # "Equals the module's" is asserted bit for bit with the module and the latents on the CPU, where two runs of a module
    # agree.  On the GPU they need not: after a warm-up run of the shape, two runs of the SAME GroupNorm SpatialDecoder on
    # the SAME 37 grids differed by up to 1.9e-6 at logit magnitude 2 (the library's transposed convolutions; recorded on the
    # MI355X), so there the route and the result's soundness are asserted and the difference is printed.
    codes = torch.randint(0, 8, (5, 4, 4), device=dev())
    for dec, zz, cc in ((D.make_spatial_decoder((256, 128, 64), 16, 1, 28, "group", eval_mode=False), z, codes),
                        (V.make_decoder((128, 64, 32), 16, 1, 28, "group", eval_mode=False), vz, codes[:, 0, 0])):
        ref = copy.deepcopy(dec).eval()
        zq = table[cc].permute(0, 3, 1, 2).contiguous() if cc.dim() == 3 else table[cc]           # the quantized latents
        with torch.no_grad():
            want, want_q = ref(zz.cpu()), ref(zq.cpu())
        got = decode_logits(dec, zz.cpu())
        assert last_decode_path() == "torch" and dec.training and not got.requires_grad and torch.equal(got, want)
        assert torch.equal(decode_logits(dec, table=table.cpu(), codes=cc.cpu()), want_q) and last_decode_path() == "torch"
        dec = dec.to(dev())
        got, got_q = decode_logits(dec, zz), decode_logits(dec, table=table, codes=cc)
        assert last_decode_path() == "torch" and dec.training and got.is_cuda and got.shape == want.shape
        print(f"torch route on the GPU, {type(dec).__name__}: max abs difference from the module on the CPU "
              f"{float((got.cpu() - want).abs().max()):.3e} (z), {float((got_q.cpu() - want_q).abs().max()):.3e} (table, codes)")
        assert torch.isfinite(got).all() and torch.isfinite(got_q).all()
    # a covered module takes the kernels, and decode_images is the reference's post-processing of those logits
    cdec = copy.deepcopy(D.spatial_case("wide-bn-28-d16")[0]).to(dev())
    logits = decode_logits(cdec, z)
    assert last_decode_path() == "hip" and torch.equal(logits, decode_logits(export, z))
    assert torch.equal(decode_images(cdec, z, dataset="FashionMNIST", apply_sigmoid=True), torch.sigmoid(logits))


# ---------------------------------------------------------------- the CLI end to end

def _shake_batchnorm(model):
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))


def _pixels(path):
    return np.asarray(Image.open(path)).astype(np.int32)


def _close(got_png, want_png):
    """At most one 8-bit level apart, on at most 1 % of the pixels."""
    got, want = _pixels(got_png), _pixels(want_png)
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = np.abs(got - want)
    print(f"{got_png.name}: {int((diff > 0).sum())} of {diff.size} pixel values differ, max {int(diff.max())}")
    return diff.max() <= 1 and np.mean(diff > 0) <= 0.01


def _torch_grid(decoder, z_top, z_bottom, path):
    from vqvae_amd.scripts.codebook_sampling import save_grid
    with torch.no_grad():
        save_grid(torch.sigmoid(decoder(z_top.to(dev()))), torch.sigmoid(decoder(z_bottom.to(dev()))), str(path))


def test_cli_vanilla_experiment(tmp_path):
    from vqvae_amd.decode import last_decode_path
    from vqvae_amd.scripts import codebook_sampling
    from vqvae_amd.vae import VAE
    torch.manual_seed(3)
    vae = VAE(in_channels=1, latent_dim=16, norm_type="batch")
    _shake_batchnorm(vae)
    exp = tmp_path / "exp"
    for sub in ("vae/checkpoints", "vae/latents_val", "codebook"):
        (exp / sub).mkdir(parents=True)
    z = torch.randn(40, 16)
    K = 8
    z_medoid = z[torch.arange(K) * 5].clone()
    torch.save({"model_state_dict": vae.state_dict()}, exp / "vae" / "checkpoints" / "best.pt")
    torch.save(z, exp / "vae" / "latents_val" / "z.pt")
    torch.save({"z_medoid": z_medoid}, exp / "codebook" / "codebook.pt")
    decoder = vae.decoder.to(dev()).eval()
    idx = torch.from_numpy(np.sort(np.random.RandomState(42).choice(40, 16, replace=False)))
    nearest = ((z[idx].double()[:, None] - z_medoid.double()[None]) ** 2).sum(-1).argmin(1)

    codebook_sampling.main([str(exp), "--atlas", "atlas.png"])                       # no codes.npy: nearest medoids
    assert last_decode_path() == "hip"
    png = exp / "codebook" / "reconstruction_grid_quantized.png"
    assert Image.open(png).size == (16 * 30 + 2, 2 * 30 + 2)
    _torch_grid(decoder, z[idx], z_medoid[nearest], tmp_path / "want_nearest.png")
    assert _close(png, tmp_path / "want_nearest.png")
    # the atlas: K cells of a 3 x 3 grid, the ninth left empty
    atlas = exp / "codebook" / "atlas.png"
    assert Image.open(atlas).size == (3 * 30 + 2, 3 * 30 + 2)
    from vqvae_amd.scripts.generate_samples import save_image
    with torch.no_grad():
        save_image(torch.sigmoid(decoder(z_medoid.to(dev()))).cpu(), str(tmp_path / "want_atlas.png"), nrow=3)
    assert _close(atlas, tmp_path / "want_atlas.png")
    assert not _pixels(atlas)[62:, 62:].any()

    codes = (torch.arange(40) * 3) % K                                               # deliberately not the nearest medoid
    assert not torch.equal(codes[idx], nearest)
    np.save(exp / "codebook" / "codes.npy", codes.numpy())
    codebook_sampling.main([str(exp), "--out", "with_codes.png", "--out_dir", str(tmp_path / "out")])
    _torch_grid(decoder, z[idx], z_medoid[codes[idx]], tmp_path / "want_codes.png")
    assert _close(tmp_path / "out" / "with_codes.png", tmp_path / "want_codes.png")
    assert np.array_equal(_pixels(tmp_path / "out" / "with_codes.png")[:31], _pixels(png)[:31])       # same top row
    assert not np.array_equal(_pixels(tmp_path / "out" / "with_codes.png")[32:], _pixels(png)[32:])   # another bottom row


def test_cli_spatial_experiment(tmp_path):
    from vqvae_amd.decode import last_decode_path
    from vqvae_amd.scripts import codebook_sampling
    from vqvae_amd.scripts.generate_samples import save_image
    from vqvae_amd.spatial_vae import SpatialVAE
    torch.manual_seed(4)
    cfg = {"in_channels": 1, "output_image_size": 28, "latent_dim": 16, "dec_channels": [256, 128, 64], "norm_type": "batch",
           "recon_loss": "mse", "mse_use_sigmoid": True}
    vae = SpatialVAE(1, (64, 128, 256), (256, 128, 64), 16, "mse", 28, "batch")
    _shake_batchnorm(vae)
    exp = tmp_path / "exp"
    for sub in ("vae/run1/checkpoints", "vae/run1/latents_val", "codebook"):
        (exp / sub).mkdir(parents=True)
    z, K = torch.randn(12, 16, 4, 4), 8
    z_medoid = torch.randn(K, 16)
    codes = torch.randint(0, K, (12, 4, 4))
    torch.save({"model_state_dict": vae.state_dict(), "epoch": 1}, exp / "vae" / "run1" / "checkpoints" / "best.pt")
    torch.save(z, exp / "vae" / "run1" / "latents_val" / "z.pt")
    torch.save({"z_medoid": z_medoid, "config": cfg}, exp / "codebook" / "codebook.pt")
    np.save(exp / "codebook" / "codes.npy", codes.numpy())
    decoder = vae.decoder.to(dev()).eval()

    codebook_sampling.main([str(exp), "--atlas", "atlas.png"])                       # 16 asked for, 12 there
    assert last_decode_path() == "hip"
    png = exp / "codebook" / "reconstruction_grid_quantized.png"
    assert Image.open(png).size == (12 * 30 + 2, 2 * 30 + 2)
    _torch_grid(decoder, z, z_medoid[codes].permute(0, 3, 1, 2), tmp_path / "want.png")
    assert _close(png, tmp_path / "want.png")
    atlas = exp / "codebook" / "atlas.png"
    assert Image.open(atlas).size == (3 * 30 + 2, 3 * 30 + 2)
    with torch.no_grad():
        filled = z_medoid[:, :, None, None].expand(K, 16, 4, 4).contiguous().to(dev())
        save_image(torch.sigmoid(decoder(filled)).cpu(), str(tmp_path / "want_atlas.png"), nrow=3)
    assert _close(atlas, tmp_path / "want_atlas.png")

    (exp / "codebook" / "codes.npy").unlink()                                         # the fallback: nearest medoids per position
    codebook_sampling.main([str(exp), "--out", "nearest.png"])
    rows = z.permute(0, 2, 3, 1).reshape(-1, 16).double()
    nearest = ((rows[:, None] - z_medoid.double()[None]) ** 2).sum(-1).argmin(1).view(12, 4, 4)
    _torch_grid(decoder, z, z_medoid[nearest].permute(0, 3, 1, 2), tmp_path / "want_nearest.png")
    assert _close(exp / "codebook" / "nearest.png", tmp_path / "want_nearest.png")
