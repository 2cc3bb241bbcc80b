"""Host side of the pull-back metric tensor (vqvae_amd.geo.pullback_metric*, scripts.riemann_metric_map): the generic autograd
route against the fp64 reference of tests/metric_tensor_cases.py, the rank and logvol rules, input shapes, the coverage
predicate and the CLI.  No GPU is needed: latents on the CPU take the generic route (the CLI runs on a GPU where there is one)."""
import json

import numpy as np
import pytest
import torch

from metric_tensor_cases import CASES, gram64_of, make_decoder, normalised_error, rank_rule, reference

FLT_EPS = float(np.finfo(np.float32).eps)


def _check_against_fp64(res, G64, p_out):
    """float32 Jacobian columns against fp64: entries to a few float32 roundings of sqrt(G_aa G_bb) (64 eps: the tangent passes
    ~1 000-term float32 sums), eigenvalues to the same share of eig_max (Weyl), logvol by the first-order bound
    d * cond * (entry error)."""
    d = G64.shape[-1]
    e = normalised_error(res.G, G64)
    assert e <= 64 * FLT_EPS, e
    ref = np.linalg.eigvalsh(G64)
    assert np.all(np.abs(res.eig - ref) <= d * 64 * FLT_EPS * ref[:, -1:])
    np.testing.assert_array_equal(res.rank, rank_rule(ref, p_out))
    cond = ref[:, -1] / ref[:, 0]
    assert cond.max() <= 1e3
    assert np.all(np.abs(res.logvol - 0.5 * np.linalg.slogdet(G64)[1]) <= d * cond * 64 * FLT_EPS)


def test_generic_route_spatial_decoder_against_fp64():
    from vqvae_amd.geo import PullbackMetric, pullback_metric_device
    z, G64 = reference("fm_none5", 12)
    res = pullback_metric_device(make_decoder("fm_none5")[0], torch.tensor(z))       # latents on the CPU: the generic route
    assert res.route == "autograd" and res.G.device.type == "cpu"
    res = PullbackMetric(res.G.numpy(), res.eig.numpy(), res.logvol.numpy(), res.rank.numpy(), res.route)
    assert res.G.dtype == np.float64 and res.G.shape == (12, 5, 5)
    assert res.eig.shape == (12, 5) and res.logvol.shape == (12,) and res.rank.dtype == np.int32
    assert np.array_equal(res.G, res.G.transpose(0, 2, 1))
    _check_against_fp64(res, G64, 16)


def test_generic_route_vanilla_decoder_against_fp64():
    from vqvae_amd.geo import native_metric_covers, pullback_metric
    from vqvae_amd.vae import Decoder
    torch.manual_seed(3)
    dec = Decoder(1, (32, 16, 8), 4, 28, "batch").eval()
    assert not native_metric_covers(dec)
    z = np.random.RandomState(4).randn(6, 4).astype(np.float32)
    res = pullback_metric(dec, z)
    assert res.route == "autograd" and res.G.shape == (6, 4, 4)
    assert np.array_equal(res.G, res.G.transpose(0, 2, 1))
    _check_against_fp64(res, gram64_of(dec, z), 28 * 28)


def test_train_mode_batchnorm_raises():
    from vqvae_amd.geo import pullback_metric, pullback_metric_device
    from vqvae_amd.vae import Decoder
    z = np.zeros((3, 16), np.float32)
    with pytest.raises(ValueError, match="BatchNorm"):
        pullback_metric(make_decoder("fm_batch", training=True)[0], z)
    with pytest.raises(ValueError, match="BatchNorm"):
        pullback_metric_device(Decoder(1, (32, 16, 8), 16, 28, "batch").train(), torch.from_numpy(z))
    with pytest.raises(ValueError, match="n, d"):
        pullback_metric_device(make_decoder("fm_batch")[0], torch.zeros(3, 16, 2))


def test_grid_input_shapes_and_row_order():
    from vqvae_amd.geo import pullback_metric_device
    dec = make_decoder("fm_none5")[0]
    z4 = torch.from_numpy(np.random.RandomState(6).randn(2, 5, 3, 2).astype(np.float32))
    grid = pullback_metric_device(dec, z4)
    assert grid.G.shape == (2, 3, 2, 5, 5) and grid.eig.shape == (2, 3, 2, 5) and grid.logvol.shape == (2, 3, 2)
    assert grid.rank.shape == (2, 3, 2) and grid.G.device == z4.device
    flat = pullback_metric_device(dec, z4.permute(0, 2, 3, 1).reshape(-1, 5))          # build_codebook's (n, h, w) row order
    assert torch.equal(grid.G.reshape(-1, 5, 5), flat.G) and torch.equal(grid.logvol.reshape(-1), flat.logvol)
    one = pullback_metric_device(dec, z4[1, :, 2, 1][None])                             # latent (n, h, w) = (1, 2, 1)
    assert torch.equal(one.G[0], grid.G[1, 2, 1])
    bare = pullback_metric_device(dec, z4, spectrum=False)
    assert bare.eig is None and bare.logvol is None and bare.rank is None and torch.equal(bare.G, grid.G)
    empty = pullback_metric_device(dec, torch.zeros(0, 5))
    assert empty.G.shape == (0, 5, 5) and empty.eig.shape == (0, 5) and empty.rank.shape == (0,)


def test_rank_and_logvol_rules_on_hand_made_G():
    from vqvae_amd.geo.riemannian_metric import metric_spectrum_fields
    d = 4
    G = torch.zeros(4, d, d, dtype=torch.float64)
    G[1] = torch.eye(d, dtype=torch.float64)
    G[2] = torch.diag(torch.tensor([2.0, 0.0, 3.0, 5.0], dtype=torch.float64))           # one zero row and column
    G[3] = torch.diag(torch.tensor([1.0, 1e-20, 1.0, 1.0], dtype=torch.float64))         # positive, below the rank tolerance
    eig = torch.linalg.eigvalsh(G)
    logvol, rank = metric_spectrum_fields(G, eig, p_out=16)
    assert rank.dtype == torch.int32 and rank.tolist() == [0, 4, 3, 3]
    assert logvol[0] == float("-inf") and logvol[1] == 0.0 and logvol[2] == float("-inf")
    assert abs(float(logvol[3]) - 0.5 * np.log(1e-20)) < 1e-12
    assert not torch.isnan(logvol).any()
    np.testing.assert_array_equal(rank.numpy(), rank_rule(eig.numpy(), 16))
    # the tolerance is max(p_out, d) * FLT_EPSILON on the singular values sqrt(eig)
    edge = torch.tensor([[(0.5 * 192 * FLT_EPS) ** 2, 1.0], [(2.0 * 192 * FLT_EPS) ** 2, 1.0]], dtype=torch.float64)
    assert metric_spectrum_fields(torch.diag_embed(edge), edge, p_out=192)[1].tolist() == [1, 2]
    assert metric_spectrum_fields(torch.diag_embed(edge), edge, p_out=16)[1].tolist() == [2, 2]


def test_native_metric_covers_truth_table():
    from vqvae_amd.geo import native_metric_covers
    from vqvae_amd.spatial_decoder import SpatialDecoder
    from vqvae_amd.vae import Decoder
    assert native_metric_covers(make_decoder("fm_none5")[0])
    assert native_metric_covers(make_decoder("fm_batch")[0])                       # eval BatchNorm
    assert native_metric_covers(make_decoder("fm_group")[0])                       # GroupNorm(32)
    assert native_metric_covers(make_decoder("cf_batch")[0])
    assert native_metric_covers(make_decoder("fm_batch1")[0])
    assert not native_metric_covers(make_decoder("fm_batch", training=True)[0])
    assert not native_metric_covers(SpatialDecoder(1, (256, 128, 64), 17, 28, "none").eval())
    assert not native_metric_covers(Decoder(1, (128, 64, 32), 16, 28, "none").eval())
    assert not native_metric_covers(make_decoder("fm_small")[0])                   # dec_channels[2] = 16: no column pass
    assert not native_metric_covers(SpatialDecoder(1, (256, 128, 64), 16, 32, "none").eval())     # 64 outputs
    assert not native_metric_covers(torch.nn.Linear(4, 4))
    assert set(CASES) >= {"fm_batch", "fm_none5", "cf_batch", "fm_group", "fm_batch1", "fm_small"}


def test_cli_end_to_end(tmp_path):
    from vqvae_amd.scripts import riemann_metric_map as cli
    dec, _ = make_decoder("fm_none5")
    torch.save({"model_state_dict": {"decoder." + k: v for k, v in dec.state_dict().items()}, "epoch": 0}, tmp_path / "best.pt")
    z = torch.from_numpy(np.random.RandomState(8).randn(5, 5, 2, 4).astype(np.float32))      # 40 latents
    torch.save(z, tmp_path / "z.pt")
    codes = np.random.RandomState(9).randint(-1, 4, size=(5, 2, 4)).astype(np.int32)
    np.save(tmp_path / "codes.npy", codes)
    out = tmp_path / "out"
    argv = ["--latents_path", str(tmp_path / "z.pt"), "--out_dir", str(out), "--vae_ckpt_path", str(tmp_path / "best.pt"),
            "--in_channels", "1", "--output_image_size", "28", "--latent_dim", "5", "--enc_channels", "64", "128", "256",
            "--dec_channels", "256", "128", "64", "--recon_loss", "mse", "--norm_type", "none",
            "--codes", str(tmp_path / "codes.npy"), "--save_tensors"]
    summary = cli.main(cli.make_parser().parse_args(argv))
    for name in ("metric_map.npz", "metric_map.json", "metric_map.png"):
        assert (out / name).stat().st_size > 0
    stored = json.loads((out / "metric_map.json").read_text())
    assert stored == json.loads(json.dumps(summary))
    for key in ("n", "n_rank_deficient", "logvol_quantiles_full_rank", "eig_ratio_quantiles", "route", "per_code"):
        assert key in stored
    assert stored["n"] == 40 and stored["n_rank_deficient"] == 0
    assert stored["route"] == ("native" if torch.cuda.is_available() else "autograd")
    arrays = np.load(out / "metric_map.npz")
    assert set(arrays.files) == {"logvol", "trace", "eig_min", "eig_max", "rank", "index", "G"}
    assert arrays["G"].shape == (40, 5, 5) and np.array_equal(arrays["index"], np.arange(40))
    np.testing.assert_allclose(arrays["trace"], np.einsum("naa->n", arrays["G"]), rtol=1e-15)
    # rows in (n, h, w) order: latent 13 = image 1, h 1, w 1
    G64 = gram64_of(dec, z[1, :, 1, 1][None].numpy())
    assert normalised_error(arrays["G"][13:14], G64) <= 64 * FLT_EPS
    flat_codes, logvol = codes.reshape(-1), arrays["logvol"]
    assert "-1" not in stored["per_code"] and set(stored["per_code"]) == {str(c) for c in set(flat_codes.tolist()) - {-1}}
    for c, entry in stored["per_code"].items():
        members = [float(logvol[i]) for i in range(40) if flat_codes[i] == int(c)]
        total = 0.0
        for m in members:                                                          # fp64, ascending latent order
            total += m
        mean = total / len(members)
        assert entry["count"] == len(members) == entry["count_finite"]
        assert entry["logvol_mean"] == mean
        assert entry["logvol_std"] == pytest.approx(np.sqrt(sum((m - mean) ** 2 for m in members) / len(members)), rel=1e-12)
    # a seeded subsample: sorted rows of the full map
    sub = cli.main(cli.make_parser().parse_args(argv[:-1] + ["--max_latents", "7", "--seed", "3", "--out_dir", str(out / "sub")]))
    sub_arrays = np.load(out / "sub" / "metric_map.npz")
    idx = sub_arrays["index"]
    assert sub["n"] == 7 and sub["n_total"] == 40 and "G" not in sub_arrays.files
    assert np.array_equal(idx, np.sort(np.random.RandomState(3).choice(40, 7, replace=False)))
    np.testing.assert_allclose(sub_arrays["logvol"], logvol[idx], rtol=0, atol=5 * 18 * 64 * FLT_EPS)   # (another torch batch)
    assert "eval-mode" in cli.make_parser().format_help() and "train-mode" in cli.make_parser().format_help()
