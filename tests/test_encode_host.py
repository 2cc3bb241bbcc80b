"""CPU-side checks of the native image encode: the export's packed arrays evaluated in numpy, in the
order the kernels read them, against the module in fp64; the coverage predicate; the torch route; the CLI's parser; the
ctypes table."""
import copy
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn as nn

import encode_cases as E


def packed_conv(a: np.ndarray, wp: np.ndarray, scale: np.ndarray, shift: np.ndarray) -> np.ndarray:
    """One stride-2 k3 p1 convolution as enc_conv_kernel reads it: a [n][s][s][cin] channels last, wp [tap][cin / 4][cout][4];
    output pixel (oy, ox) reads input pixel (2 oy - 1 + ky, 2 ox - 1 + kx) for tap 3 ky + kx, nothing outside the image; K
    runs over the taps, then the 8-channel blocks, within a block over the channels 0 4 1 5 2 6 3 7."""
    n, s, _, cin = a.shape
    so, cout = (s + 1) // 2, wp.shape[2]
    out = np.zeros((n, so, so, cout))
    for oy in range(so):
        for ox in range(so):
            acc = np.zeros((n, cout))
            for tap in range(9):
                iy, ix = 2 * oy - 1 + tap // 3, 2 * ox - 1 + tap % 3
                if not (0 <= iy < s and 0 <= ix < s):
                    continue                                              # the staged zero row
                for cb in range(cin // 8):
                    for r in range(4):
                        for h in (0, 1):
                            ch = 8 * cb + 4 * h + r
                            acc += a[:, iy, ix, ch, None] * wp[tap, 2 * cb + h, :, r][None]
            out[:, oy, ox] = acc
    return np.maximum(out * scale + shift, 0.0)


def packed_first(x: np.ndarray, w1p: np.ndarray, scale: np.ndarray, shift: np.ndarray) -> np.ndarray:
    """Layer 1 as enc_first_kernel reads it: x [n][C][S][S], w1p [(c, ky, kx)][e1], one row and column of zeros in front."""
    n, C, S, _ = x.shape
    pad = np.zeros((n, C, S + 1, S + 1))
    pad[:, :, 1:, 1:] = x
    so = S // 2
    acc = np.zeros((n, so, so, w1p.shape[1]))
    for c in range(C):
        for ky in range(3):
            for kx in range(3):
                acc += pad[:, c, ky:ky + 2 * so:2, kx:kx + 2 * so:2, None] * w1p[(c * 3 + ky) * 3 + kx]
    return np.maximum(acc * scale + shift, 0.0)


def packed_head(a3: np.ndarray, whp: np.ndarray, bh: np.ndarray, d: int, spatial: bool):
    """Both heads as enc_head_kernel reads them: the last activation [n][16][e3] as a matrix of rows (items: 16 segments of e3;
    or (item, pixel): one segment); per segment one sum over the channels in the conv kernels' block order, the segments added
    in order, then the bias; columns 0 .. d-1 are mu, d .. 2d-1 logvar."""
    n, _, e3 = a3.shape
    rows = a3.reshape(n * 16, 1, e3) if spatial else a3
    nseg, _, npad, _ = whp.shape
    assert rows.shape[1] == nseg
    total = np.zeros((rows.shape[0], npad))
    for s in range(nseg):
        part = np.zeros_like(total)
        for cb in range(e3 // 8):
            for r in range(4):
                for h in (0, 1):
                    part += rows[:, s, 8 * cb + 4 * h + r, None] * whp[s, 2 * cb + h, :, r][None]
        total += part
    total += bh
    assert not whp[:, :, 2 * d:].any() and not bh[2 * d:].any()
    mu, logvar = total[:, :d], total[:, d:2 * d]
    if spatial:                                                            # row (item, pixel) -> [item][col][pixel]
        mu, logvar = (t.reshape(n, 16, d).transpose(0, 2, 1).reshape(n, d, 4, 4) for t in (mu, logvar))
    return mu, logvar


@pytest.mark.parametrize("kind,name", E.ALL_CASES)
def test_packed_arrays_reproduce_the_module_in_fp64(kind, name):
    _check_packed_arrays(kind, name, E.CASES[(kind, name)], E.case(kind, name))


@pytest.mark.parametrize("kind,name", E.ALL_ENVELOPE_CASES)
def test_packed_arrays_reproduce_the_envelope_modules_in_fp64(kind, name):
    """The same check over encode_cases.ENVELOPE_CASES: every head tile count, d = 1, BatchNorm2d(affine=False)."""
    _check_packed_arrays(kind, name, E.ENVELOPE_CASES[(kind, name)], E.envelope_case(kind, name))


def _check_packed_arrays(kind, name, config, case):
    from vqvae_amd.image_encoder import ImageEncoderExport, encoder_kernels_cover
    channels, d, C, size, _ = config
    enc, x, mu64, lv64, _, _ = case
    assert encoder_kernels_cover(enc) and encoder_kernels_cover(enc, size)
    export = ImageEncoderExport(enc, torch.device("cpu"))
    h = {k: v.numpy() for k, v in export.host.items()}
    xs = x[:6].double().numpy()                                             # the zero image, the one image and four others
    a = packed_first(xs, h["w1p"], h["scale1"], h["shift1"])
    a = packed_conv(a, h["w2p"], h["scale2"], h["shift2"])
    a = packed_conv(a, h["w3p"], h["scale3"], h["shift3"])
    assert a.shape == (6, 4, 4, channels[2])
    mu, logvar = packed_head(a.reshape(6, 16, -1), h["whp"], h["bh"], d, kind == "spatial")
    err = max(float(np.abs(mu - mu64[:6].numpy()).max()), float(np.abs(logvar - lv64[:6].numpy()).max()))
    print(f"{kind} {name}: packed arrays vs module, fp64: max abs error {err:.3e} at magnitude {float(mu64.abs().max()):.2f}")
    assert mu.shape == tuple(mu64[:6].shape) and err <= 1e-12
    # the device tensors are the fp64 composition rounded once, in the documented shapes
    npad = (2 * d + 31) // 32 * 32
    shapes = {"w1p": (9 * C, channels[0]), "w2p": (9, channels[0] // 4, channels[1], 4), "w3p": (9, channels[1] // 4, channels[2], 4),
              "whp": (1 if kind == "spatial" else 16, channels[2] // 4, npad, 4), "bh": (npad,), "scale1": (channels[0],),
              "shift1": (channels[0],), "scale2": (channels[1],), "shift2": (channels[1],), "scale3": (channels[2],),
              "shift3": (channels[2],)}
    assert set(export.tensors) == set(shapes)
    for key, shape in shapes.items():
        t = export.tensors[key]
        assert tuple(t.shape) == shape and t.dtype == torch.float32 and t.is_contiguous(), key
        assert torch.equal(t, export.host[key].float()), key
    desc = export.desc
    assert (desc.in_channels, desc.in_size, desc.e1, desc.e2, desc.e3, desc.latent_dim, desc.spatial_head) == \
        (C, size, *channels, d, int(kind == "spatial"))
    assert export.latent_dim == d and export.spatial == (kind == "spatial")


def test_coverage_predicate_rejects_what_the_kernels_do_not_run():
    from vqvae_amd.encode import native_encode_covers
    from vqvae_amd.image_encoder import (ImageEncoderExport, encoder_kernels_cover, looks_like_spatial_encoder,
                                         looks_like_vanilla_encoder)
    wide = (64, 128, 256)
    for kind, d_max in (("vanilla", 128), ("spatial", 64)):
        good = E.make_encoder(kind, wide, d_max, 1, "batch")
        assert encoder_kernels_cover(good) and native_encode_covers(good) and encoder_kernels_cover(good, 28)
        assert looks_like_vanilla_encoder(good) == (kind == "vanilla") and looks_like_spatial_encoder(good) == (kind == "spatial")
        assert encoder_kernels_cover(E.make_encoder(kind, (32, 64, 128), 5, 3, "none"), 32)
        assert not encoder_kernels_cover(E.make_encoder(kind, wide, 16, 1, "group"))
        assert not encoder_kernels_cover(E.make_encoder(kind, wide, 16, 1, "batch", eval_mode=False))
        one_training = E.make_encoder(kind, wide, 16, 1, "batch")
        one_training.conv_layers[4].train()                                 # torch looks at the layer's own flag
        assert not encoder_kernels_cover(one_training)
        no_stats = E.make_encoder(kind, wide, 16, 1, "none")
        for i in (1, 4, 7):
            no_stats.conv_layers[i] = nn.BatchNorm2d(wide[i // 3], track_running_stats=False)
        assert not encoder_kernels_cover(no_stats.eval())
        for layer in ("conv", "head"):
            nobias = E.make_encoder(kind, wide, 16, 1, "none")
            if layer == "conv":
                nobias.conv_layers[3].bias = None
            else:
                nobias.fc_logvar.bias = None
            assert not encoder_kernels_cover(nobias)
        assert not encoder_kernels_cover(E.make_encoder(kind, (48, 96, 192), 16, 1, "batch"))
        assert not encoder_kernels_cover(good, 32)                          # C = 1 at 32 px
        assert not encoder_kernels_cover(E.make_encoder(kind, wide, 16, 3, "batch"), 28)
        assert not encoder_kernels_cover(E.make_encoder(kind, wide, 16, 2, "batch"))
        assert not encoder_kernels_cover(E.make_encoder(kind, wide, d_max + 1, 1, "batch"))       # d = 129 | 65
        with pytest.raises(ValueError):
            ImageEncoderExport(E.make_encoder(kind, wide, 16, 1, "group"), torch.device("cpu"))
    assert not encoder_kernels_cover(nn.Linear(4, 4)) and not native_encode_covers(nn.Linear(4, 4))


@pytest.mark.parametrize("kind,name", E.ALL_ENVELOPE_CASES)
def test_envelope_cases_are_covered_and_one_step_outside_is_not(kind, name):
    """Predicate and make_shape agree on every envelope case: covered, with a workspace of the three activation buffers; the
    same module one latent dimension above the maximum (129 | 65) is not covered, and the descriptor with that dimension, with
    0, or with the other image size answers 0."""
    from vqvae_amd import _lib
    from vqvae_amd.encode import native_encode_covers
    from vqvae_amd.image_encoder import ImageEncoderExport, encoder_kernels_cover
    lib = _lib.load()
    channels, d, C, size, norm = E.ENVELOPE_CASES[(kind, name)]
    enc = E.envelope_case(kind, name)[0]
    assert encoder_kernels_cover(enc) and encoder_kernels_cover(enc, size) and native_encode_covers(enc, size)
    assert not encoder_kernels_cover(enc, 60 - size)
    if norm == "batch-plain":
        norms = [m for m in enc.modules() if isinstance(m, nn.BatchNorm2d)]
        assert len(norms) == 3 and all(m.weight is None and m.bias is None and not m.training for m in norms)
    d_max = 128 if kind == "vanilla" else 64
    assert not encoder_kernels_cover(E.build(kind, channels, d_max + 1, C, norm))
    desc = ImageEncoderExport(enc, torch.device("cpu")).desc
    per_item = 4 * ((size // 2) ** 2 * channels[0] + (size // 4) ** 2 * channels[1] + 16 * channels[2])
    assert per_item % 256 == 0 and lib.geo_image_encode_workspace_bytes(desc, 1) == per_item
    assert lib.geo_image_encode_workspace_bytes(desc, E.N_VANILLA) == E.N_VANILLA * per_item
    for change in (dict(latent_dim=d_max + 1), dict(latent_dim=0), dict(in_size=60 - size), dict(in_channels=4 - C)):
        bad = type(desc).from_buffer_copy(desc)
        for k, v in change.items():
            setattr(bad, k, v)
        assert lib.geo_image_encode_workspace_bytes(bad, 8) == 0, change


def test_workspace_query_answers_zero_outside_the_coverage():
    from vqvae_amd import _lib
    lib = _lib.load()
    assert lib.geo_version() >= 108

    def desc(**kw):
        d = _lib.ImageEncoderDesc()
        d.in_channels, d.in_size, d.e1, d.e2, d.e3, d.latent_dim, d.spatial_head = 1, 28, 64, 128, 256, 128, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    per_item = (196 * 64 + 49 * 128 + 16 * 256) * 4                         # the three activation buffers, 256-byte multiples
    assert lib.geo_image_encode_workspace_bytes(desc(), 1) == per_item
    assert lib.geo_image_encode_workspace_bytes(desc(), 3) == 3 * per_item
    assert lib.geo_image_encode_workspace_bytes(desc(), 0) == per_item
    assert lib.geo_image_encode_workspace_bytes(desc(), 10 ** 6) == 4096 * per_item
    assert lib.geo_image_encode_workspace_bytes(desc(in_channels=3, in_size=32, spatial_head=1, latent_dim=64), 1) == \
        (256 * 64 + 64 * 128 + 16 * 256) * 4
    for bad in (dict(latent_dim=129), dict(latent_dim=0), dict(latent_dim=65, spatial_head=1), dict(e1=48, e2=96, e3=192),
                dict(e3=128), dict(in_size=32), dict(in_channels=3), dict(in_channels=2), dict(spatial_head=2)):
        assert lib.geo_image_encode_workspace_bytes(desc(**bad), 8) == 0, bad
    assert lib.geo_image_encode_workspace_bytes(None, 8) == 0
    assert lib.geo_image_encode_workspace_bytes(desc(), -1) == 0


def test_uncovered_modules_encode_themselves_and_equal_the_module():
    """The torch route on the CPU, where it is deterministic: GroupNorm and train-mode BatchNorm encoders, other widths and a
    size the kernels do not take; the result is the module's own in eval(), bit for bit, and the layers' modes are put back."""
    from vqvae_amd.encode import encode_latents, last_encode_path
    for enc, x in ((E.make_encoder("vanilla", (32, 64, 128), 16, 1, "group", eval_mode=False), E.images(5, 1, 28)),
                   (E.make_encoder("spatial", (32, 64, 128), 8, 3, "batch", eval_mode=False), E.images(5, 3, 32)),
                   (E.make_encoder("spatial", (48, 96, 192), 8, 1, "none", eval_mode=False), E.images(5, 1, 28)),
                   (E.make_encoder("vanilla", (32, 64, 128), 16, 1, "none", eval_mode=False), E.images(5, 1, 32))):
        ref = copy.deepcopy(enc).eval()
        with torch.no_grad():
            want_mu, want_lv = ref(x)
        enc.conv_layers[2].eval()                                           # a mixed state must come back as it was
        before = [m.training for m in enc.modules()]
        mu, logvar = encode_latents(enc, x)
        assert last_encode_path() == "torch"
        assert torch.equal(mu, want_mu) and torch.equal(logvar, want_lv) and not mu.requires_grad
        assert [m.training for m in enc.modules()] == before and enc.training
        empty_mu, empty_lv = encode_latents(enc, x[:0])
        assert empty_mu.shape == (0,) + tuple(want_mu.shape[1:]) and empty_lv.shape == empty_mu.shape
    with pytest.raises(ValueError):
        encode_latents(enc, torch.zeros(3, 28, 28))


def test_an_export_refuses_images_of_another_shape():
    from vqvae_amd.encode import encode_latents
    from vqvae_amd.image_encoder import ImageEncoderExport
    export = ImageEncoderExport(E.case("spatial", "narrow-none-28-d5")[0], torch.device("cpu"))
    with pytest.raises(ValueError):
        encode_latents(export, torch.zeros(2, 1, 32, 32))
    with pytest.raises(ValueError):
        encode_latents(export, torch.zeros(2, 3, 28, 28))


def test_cli_help_parses(capsys):
    from vqvae_amd.scripts.encode_latents import make_parser
    with pytest.raises(SystemExit) as stop:
        make_parser().parse_args(["--help"])
    assert stop.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--checkpoint", "--config", "--dataset", "--data_root", "--split", "--out_dir", "--batch_size", "--seed",
                 "--max_samples"):
        assert flag in text, flag
    args = make_parser().parse_args(["--checkpoint", "c.pt", "--dataset", "MNIST", "--out_dir", "o", "--split", "train"])
    assert args.split == "train" and args.seed is None and args.config is None and args.max_samples is None
    with pytest.raises(SystemExit):
        make_parser().parse_args(["--checkpoint", "c.pt", "--dataset", "MNIST", "--out_dir", "o", "--split", "test"])


def test_cli_names_a_missing_data_file(tmp_path):
    from vqvae_amd.scripts.encode_latents import split_loader
    with pytest.raises(FileNotFoundError) as err:
        split_loader("FashionMNIST", str(tmp_path), "val", 8, torch.device("cpu"))
    assert str(tmp_path / "FashionMNIST" / "raw") in str(err.value)


def test_cli_resolves_a_spatial_config(tmp_path):
    import yaml
    from vqvae_amd.scripts.encode_latents import spatial_model_config
    model = {"in_channels": 1, "enc_channels": [32, 64, 128], "dec_channels": [128, 64, 32], "latent_dim": 4, "recon_loss": "mse",
             "output_image_size": 28, "norm_type": "none"}
    ckpt = tmp_path / "run" / "checkpoints" / "best.pt"
    ckpt.parent.mkdir(parents=True)
    torch.save({"model_state_dict": {}}, ckpt)
    with pytest.raises(FileNotFoundError) as err:
        spatial_model_config(ckpt, None)
    assert "--config" in str(err.value) and str(ckpt.parent / "vae.yaml") in str(err.value)
    (tmp_path / "run" / "vae.yaml").write_text(yaml.safe_dump({"model": model, "seed": 1}))
    assert spatial_model_config(ckpt, None) == model
    other = dict(model, latent_dim=8)
    (tmp_path / "given.yaml").write_text(yaml.safe_dump({"model": other}))
    assert spatial_model_config(ckpt, str(tmp_path / "given.yaml")) == other
    torch.save({"model_state_dict": {}, "config": {"model": dict(model, latent_dim=6)}}, ckpt)
    assert spatial_model_config(ckpt, None)["latent_dim"] == 6


def test_header_symbols_are_in_the_ctypes_table():
    from vqvae_amd import _lib
    header = (Path(__file__).resolve().parents[1] / "include" / "geo_hip.h").read_text()
    declared = set(re.findall(r"\b(geo_image_encode\w*)\s*\(", header))
    assert declared == {"geo_image_encode_workspace_bytes", "geo_image_encode"}
    assert declared <= set(_lib.EXPORTS)
    fields = re.search(r"typedef struct geo_image_encoder_desc \{(.*?)\} geo_image_encoder_desc;", header, re.S).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", fields, flags=re.S).replace(",", ";"))
    assert names == [n for n, _ in _lib.ImageEncoderDesc._fields_]
