"""CPU-side checks of the native image decode: the spatial export's composed first stage against the
module in fp64, the coverage predicate, the workspace query's answer for an uncovered descriptor, and the host logic of the
codebook_sampling CLI."""
import numpy as np
import pytest
import torch
import torch.nn as nn
from PIL import Image

import decode_cases as D
import vanilla_jvp_cases as V


def composed_front(export, z: np.ndarray) -> np.ndarray:
    """The export's first stage in numpy fp64: z [n][d][4][4] -> the first ReLU's pre-activation [n][c1][8][8], from
    host["W"] [parity][tap][d + 1][c1] with the parity / tap meaning of _parity_taps and the constant-one channel d."""
    W, scale, shift = (export.host[k].numpy() for k in ("W", "scale1", "shift1"))
    n, d = z.shape[:2]
    grid = np.zeros((n, 6, 6, d + 1))                                  # one pixel of zeros around the 4 x 4 grid
    grid[:, 1:5, 1:5, :d] = z.transpose(0, 2, 3, 1)
    grid[:, 1:5, 1:5, d] = 1.0
    out = np.zeros((n, 8, 8, W.shape[-1]))
    for py in (0, 1):
        for px in (0, 1):
            acc = np.zeros((n, 4, 4, W.shape[-1]))
            for a in (0, 1):
                for b in (0, 1):
                    src = grid[:, 1 + py - a:5 + py - a, 1 + px - b:5 + px - b]          # input pixel (y + py - a, x + px - b)
                    acc += src @ W[2 * py + px, 2 * a + b]
            out[:, py::2, px::2] = acc
    return (out * scale + shift).transpose(0, 3, 1, 2)


@pytest.mark.parametrize("name", list(D.SPATIAL_CASES))
def test_composed_front_matches_the_module_in_fp64(name):
    _check_composed_front(name, D.SPATIAL_CASES[name])


@pytest.mark.parametrize("name", list(D.SPATIAL_ENVELOPE_CASES))
def test_composed_front_matches_the_envelope_modules_in_fp64(name):
    """The same check over decode_cases.SPATIAL_ENVELOPE_CASES: the constant-one channel on either side of a K block's edge,
    d = 1 and 64, BatchNorm2d(affine=False), a dec_channels[0] other than 256 / 128."""
    _check_composed_front(name, D.SPATIAL_ENVELOPE_CASES[name])


def _check_composed_front(name, config):
    from vqvae_amd.spatial_decoder import SpatialImageDecoderExport, spatial_image_kernels_cover
    channels, d, C, size, norm = config
    dec = D.build_spatial(channels, d, C, size, norm, seed=len(name))
    assert spatial_image_kernels_cover(dec)
    export = SpatialImageDecoderExport(dec, torch.device("cpu"))
    z = D.grids(9, d, seed=5).double()
    with torch.no_grad():
        dd = dec.double()
        want = dd.deconv_layers[1](dd.deconv_layers[0](dd.conv_in(z))).numpy()
    got = composed_front(export, z.numpy())
    err = float(np.abs(got - want).max())
    print(f"{name}: composed front vs module, fp64: max abs error {err:.3e} at magnitude {np.abs(want).max():.2f}")
    assert got.shape == want.shape and err <= 1e-12
    dp = (d + 1 + 7) // 8 * 8
    c1 = channels[1]
    assert export.tensors["w1p"].shape == (4, 4, dp // 4, c1, 4) and export.tensors["w1p"].dtype == torch.float32
    # the device layout is the fp64 composition rounded once: element (par, tap, q, co, r) = W[par][tap][4 q + r][co]
    back = export.tensors["w1p"].permute(0, 1, 2, 4, 3).reshape(4, 4, dp, c1)
    assert torch.equal(back[:, :, :d + 1], export.host["W"].float()) and not back[:, :, d + 1:].any()
    assert (export.desc.latent_dim, export.desc.c1, export.desc.c2, export.desc.out_channels, export.desc.out_size) == \
        (d, channels[1], channels[2], C, size)


def test_coverage_predicate_rejects_what_the_kernels_do_not_run():
    from vqvae_amd.decode import native_decode_covers
    from vqvae_amd.spatial_decoder import SpatialImageDecoderExport, spatial_image_kernels_cover
    wide = ((256, 128, 64), 16, 1, 28)
    assert not spatial_image_kernels_cover(D.make_spatial_decoder(*wide, "group"))
    assert not spatial_image_kernels_cover(D.make_spatial_decoder(*wide, "batch", eval_mode=False))
    assert not spatial_image_kernels_cover(D.make_spatial_decoder((256, 128, 64), 65, 1, 28, "batch"))
    assert spatial_image_kernels_cover(D.make_spatial_decoder((256, 128, 64), 64, 1, 28, "batch"))
    assert not spatial_image_kernels_cover(D.make_spatial_decoder((256, 96, 64), 16, 1, 28, "batch"))
    nobias = D.make_spatial_decoder(*wide, "none")
    nobias.deconv_layers[3].bias = None
    assert not spatial_image_kernels_cover(nobias)
    assert not spatial_image_kernels_cover(nn.Linear(4, 4))
    with pytest.raises(ValueError):
        SpatialImageDecoderExport(D.make_spatial_decoder(*wide, "group"), torch.device("cpu"))
    # decode's predicate: the spatial one for spatial decoders, vanilla_kernels_cover for vanilla ones
    import vanilla_jvp_cases as V
    assert native_decode_covers(D.make_spatial_decoder(*wide, "batch"))
    assert not native_decode_covers(D.make_spatial_decoder(*wide, "group"))
    assert native_decode_covers(V.make_decoder((256, 128, 64), 128, 1, 28, "batch"))
    assert not native_decode_covers(V.make_decoder((256, 128, 64), 128, 1, 28, "group"))
    assert not native_decode_covers(nn.Linear(4, 4))


@pytest.mark.parametrize("kind,name", [("spatial", n) for n in D.SPATIAL_ENVELOPE_CASES] + [("vanilla", n) for n in V.ENVELOPE_CASES])
def test_envelope_cases_are_covered_and_one_step_outside_is_not(kind, name):
    """Predicate and make_shape / make_spatial_shape agree on every envelope case: covered, with a workspace of the two
    activation buffers; the same module one latent dimension above the maximum (65 | 129) is not covered, and the descriptor
    with that dimension, with 0, or with a size or channel count next to the admitted ones answers 0."""
    from vqvae_amd import _lib
    from vqvae_amd.decode import native_decode_covers
    from vqvae_amd.spatial_decoder import SpatialImageDecoderExport
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    lib = _lib.load()
    if kind == "spatial":
        channels, d, C, size, norm = D.SPATIAL_ENVELOPE_CASES[name]
        build, d_max, Export, query = D.build_spatial, 64, SpatialImageDecoderExport, lib.geo_spatial_decode_workspace_bytes
        per_item = 4 * (64 * channels[1] + 256 * channels[2])
    else:
        channels, d, C, size, norm = V.ENVELOPE_CASES[name]
        build, d_max, Export, query = V.build, 128, VanillaDecoderExport, lib.geo_vanilla_decode_workspace_bytes
        per_item = 4 * ((size // 4) ** 2 * channels[1] + (size // 2) ** 2 * channels[2])
    dec = build(channels, d, C, size, norm, seed=len(name))
    assert native_decode_covers(dec)
    if norm == "batch-plain":
        norms = [m for m in dec.modules() if isinstance(m, nn.BatchNorm2d)]
        assert len(norms) == 2 and all(m.weight is None and m.bias is None and not m.training for m in norms)
    assert not native_decode_covers(build(channels, d_max + 1, C, size, norm))
    desc = Export(dec, torch.device("cpu")).desc
    assert per_item % 256 == 0 and query(desc, 1) == per_item and query(desc, D.N_SPATIAL) == D.N_SPATIAL * per_item
    for change in (dict(latent_dim=d_max + 1), dict(latent_dim=0), dict(out_size=24 if size == 28 else 36), dict(out_channels=2),
                   dict(out_channels=4)):
        bad = type(desc).from_buffer_copy(desc)
        for k, v in change.items():
            setattr(bad, k, v)
        assert query(bad, 8) == 0, change


def test_workspace_query_answers_zero_outside_the_coverage():
    from vqvae_amd import _lib
    lib = _lib.load()
    assert lib.geo_version() >= 107

    def spatial(**kw):
        d = _lib.SpatialImageDecoderDesc()
        d.latent_dim, d.c1, d.c2, d.out_channels, d.out_size = 16, 128, 64, 1, 28
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def vanilla(**kw):
        d = _lib.VanillaDecoderDesc()
        d.latent_dim, d.c1, d.c2, d.out_channels, d.out_size = 128, 128, 64, 1, 28
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    # the two activation buffers of a pass, each rounded up to 256 bytes
    assert lib.geo_spatial_decode_workspace_bytes(spatial(), 1) == (64 * 128 + 256 * 64) * 4
    assert lib.geo_spatial_decode_workspace_bytes(spatial(), 3) == 3 * (64 * 128 + 256 * 64) * 4
    assert lib.geo_vanilla_decode_workspace_bytes(vanilla(), 1) == (49 * 128 + 196 * 64) * 4
    assert lib.geo_spatial_decode_workspace_bytes(spatial(), 10 ** 6) == lib.geo_spatial_decode_workspace_bytes(spatial(), 10 ** 7)
    for bad in (dict(latent_dim=65), dict(latent_dim=0), dict(c1=96), dict(c1=128, c2=32), dict(out_channels=2), dict(out_size=30)):
        assert lib.geo_spatial_decode_workspace_bytes(spatial(**bad), 8) == 0, bad
    for bad in (dict(latent_dim=129), dict(c1=96), dict(out_channels=2), dict(out_size=30)):
        assert lib.geo_vanilla_decode_workspace_bytes(vanilla(**bad), 8) == 0, bad
    assert lib.geo_spatial_decode_workspace_bytes(None, 8) == 0 and lib.geo_vanilla_decode_workspace_bytes(None, 8) == 0
    assert lib.geo_spatial_decode_workspace_bytes(spatial(), -1) == 0


def test_decode_logits_checks_shapes_and_codes_before_any_device_work():
    from vqvae_amd.decode import decode_logits
    dec = D.make_spatial_decoder((256, 128, 64), 16, 1, 28, "group")
    table = torch.randn(8, 16)
    with pytest.raises(ValueError):
        decode_logits(dec, table=table, codes=torch.full((2, 4, 4), 8))
    with pytest.raises(ValueError):
        decode_logits(dec, table=table, codes=torch.full((2, 4, 4), -1))
    with pytest.raises(ValueError):
        decode_logits(dec, torch.randn(2, 16, 4, 4), table=table, codes=torch.zeros(2, 4, 4, dtype=torch.long))
    with pytest.raises(ValueError):
        decode_logits(dec, torch.randn(2, 15, 4, 4))
    with pytest.raises(ValueError):
        decode_logits(dec, table=table, codes=torch.zeros(2, 4, 4))


def test_uncovered_modules_decode_themselves_and_equal_the_module():
    """The torch route on the CPU, where it is deterministic: GroupNorm and train-mode BatchNorm decoders, from z and from
    (table, codes); the result is the module's own in eval(), bit for bit, and the layers' modes are put back."""
    import copy

    import vanilla_jvp_cases as V
    from vqvae_amd.decode import decode_logits, last_decode_path
    g = torch.Generator().manual_seed(2)
    table = torch.randn(8, 16, generator=g)
    for dec, z, codes in (
            (D.make_spatial_decoder((128, 64, 32), 16, 1, 28, "group", eval_mode=False), D.grids(5, 16),
             torch.randint(0, 8, (5, 4, 4), generator=g)),
            (D.make_spatial_decoder((128, 64, 32), 16, 3, 32, "batch", eval_mode=False), D.grids(5, 16),
             torch.randint(0, 8, (5, 4, 4), generator=g)),
            (V.make_decoder((128, 64, 32), 16, 1, 28, "group", eval_mode=False), D.vectors(5, 16),
             torch.randint(0, 8, (5,), generator=g))):
        ref = copy.deepcopy(dec).eval()
        with torch.no_grad():
            want_z = ref(z)
            zq = table[codes]
            want_q = ref(zq.permute(0, 3, 1, 2).contiguous() if zq.dim() == 4 else zq)       # the quantized grid, NCHW
        got = decode_logits(dec, z)
        assert last_decode_path() == "torch" and torch.equal(got, want_z) and not got.requires_grad
        assert torch.equal(decode_logits(dec, table=table, codes=codes), want_q)
        assert dec.training and all(m.training for m in dec.modules())


# ---------------------------------------------------------------- the CLI's host logic

def test_cli_selects_the_reference_indices():
    from vqvae_amd.scripts.codebook_sampling import select_indices
    for N, num, seed in ((40, 16, 42), (12, 16, 42), (1000, 7, 3)):
        want = np.sort(np.random.RandomState(seed).choice(N, min(num, N), replace=False))
        got = select_indices(N, num, seed)
        assert np.array_equal(got, want) and len(got) == min(num, N)


def test_cli_reports_a_missing_codebook_directory_and_returns(tmp_path, capsys):
    from vqvae_amd.scripts import codebook_sampling
    (tmp_path / "vae").mkdir()
    assert codebook_sampling.main([str(tmp_path)]) is None
    assert capsys.readouterr().out.strip() == f"Error: Codebook directory not found: {tmp_path / 'codebook'}"
    (tmp_path / "codebook").mkdir()
    (tmp_path / "vae").rmdir()
    codebook_sampling.main([str(tmp_path)])
    assert capsys.readouterr().out.strip() == f"Error: VAE directory not found: {tmp_path / 'vae'}"


def test_cli_reports_a_dimension_mismatch_and_returns(tmp_path, capsys):
    from vqvae_amd.scripts import codebook_sampling
    from vqvae_amd.vae import VAE
    torch.manual_seed(0)
    (tmp_path / "vae" / "checkpoints").mkdir(parents=True)
    (tmp_path / "vae" / "latents_val").mkdir()
    (tmp_path / "codebook").mkdir()
    torch.save({"model_state_dict": VAE(latent_dim=16).state_dict()}, tmp_path / "vae" / "checkpoints" / "best.pt")
    torch.save(torch.randn(40, 16), tmp_path / "vae" / "latents_val" / "z.pt")
    torch.save({"z_medoid": torch.randn(8, 12)}, tmp_path / "codebook" / "codebook.pt")
    codebook_sampling.main([str(tmp_path), "--out_dir", str(tmp_path / "out")])
    out = capsys.readouterr().out
    assert "ERROR: Dimensional mismatch!\n  Latents dimension: 16 (shape: (40, 16))\n  Codebook dimension: 12 (shape: (8, 12))\n" in out
    assert "Ensure latents and codebook come from compatible experiments." in out
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("S,C,m", [(28, 1, 16), (32, 3, 5)])
def test_cli_grid_size(tmp_path, S, C, m):
    from vqvae_amd.scripts.codebook_sampling import save_grid
    top, bottom = torch.rand(m, C, S, S), torch.rand(m, C, S, S)
    save_grid(top, bottom, str(tmp_path / "grid.png"))
    img = Image.open(tmp_path / "grid.png")
    assert img.size == (m * (S + 2) + 2, 2 * (S + 2) + 2) and img.mode == "RGB"
    px = np.asarray(img)
    want = (top[m - 1].expand(3, S, S) * 255 + 0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy()
    assert np.array_equal(px[2:2 + S, (m - 1) * (S + 2) + 2:(m - 1) * (S + 2) + 2 + S], want)        # top row, last sample


def test_cli_activation_follows_the_reference():
    from vqvae_amd.scripts.codebook_sampling import activation_config
    # a checkpoint config decides, with the reference's defaults for missing keys
    assert activation_config({"in_channels": 3, "recon_loss": "mse", "mse_use_sigmoid": False}, None, 3) == (False, True)
    assert activation_config({"in_channels": 3, "recon_loss": "bce", "mse_use_sigmoid": False}, None, 3) == (True, True)
    assert activation_config({"in_channels": 1}, None, 1) == (True, False)
    # no config: the reference infers mse with mse_use_sigmoid = (in_channels == 1)
    assert activation_config(None, None, 1) == (True, False)
    assert activation_config(None, None, 3) == (False, True)
    # ... unless build_codebook recorded one, and the flags override everything
    assert activation_config(None, {"recon_loss": "mse", "mse_use_sigmoid": True}, 3) == (True, True)
    assert activation_config(None, {"recon_loss": "bce"}, 3) == (True, True)
    assert activation_config({"in_channels": 3, "mse_use_sigmoid": False}, None, 3, mse_use_sigmoid=True) == (True, True)
    assert activation_config({"in_channels": 1, "mse_use_sigmoid": False}, None, 1, recon_loss="bce") == (True, False)


def test_cli_reports_latents_of_the_wrong_kind_and_returns(tmp_path, capsys):
    from vqvae_amd.scripts import codebook_sampling
    from vqvae_amd.vae import VAE
    torch.manual_seed(0)
    (tmp_path / "vae" / "checkpoints").mkdir(parents=True)
    (tmp_path / "vae" / "latents_val").mkdir()
    (tmp_path / "codebook").mkdir()
    torch.save({"model_state_dict": VAE(latent_dim=16).state_dict()}, tmp_path / "vae" / "checkpoints" / "best.pt")
    torch.save(torch.randn(6, 16, 4, 4), tmp_path / "vae" / "latents_val" / "z.pt")
    torch.save({"z_medoid": torch.randn(8, 16)}, tmp_path / "codebook" / "codebook.pt")
    assert codebook_sampling.main([str(tmp_path)]) is None
    out = capsys.readouterr().out
    assert "ERROR: grid latents (6, 16, 4, 4) with the vanilla decoder of" in out
    assert not list((tmp_path / "codebook").glob("*.png"))
