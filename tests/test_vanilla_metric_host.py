"""Host side of the vanilla decoder's metric tensor, no GPU: the coverage predicate, the size queries and
refusals of geo_vanilla_metric_tensor and geo_sym_spectrum, the `jacobian` field on the autograd route, and
python -m vqvae_amd.scripts.vanilla_metric_map on the CPU through --config and --codebook_dir."""
import json
import os

import numpy as np
import pytest
import torch

import vanilla_jvp_cases as V
from metric_tensor_cases import gram64_of, normalised_error

CPU = torch.device("cpu")
GEO_E_ARG = -1
TINY_VAE = dict(in_channels=1, enc_channels=[8, 16, 32], dec_channels=[32, 16, 8], latent_dim=4, recon_loss="bce",
                output_image_size=28, norm_type="none", mse_use_sigmoid=True)


def test_the_predicate_is_the_vanilla_kernels_coverage():
    from vqvae_amd.geo import native_metric_covers, native_vanilla_metric_covers
    from vqvae_amd.geo.riemannian_metric import native_vanilla_metric_covers as from_module
    from vqvae_amd.vanilla_decoder import vanilla_kernels_cover
    assert from_module is native_vanilla_metric_covers
    table = {name: True for name in list(V.CASES) + list(V.ENVELOPE_CASES)}
    decoders = {name: V.build(*spec) for name, spec in {**V.CASES, **V.ENVELOPE_CASES}.items()}
    decoders["group"] = V.build((256, 128, 64), 16, 1, 28, "group")
    decoders["train-bn"] = V.make_decoder((256, 128, 64), 16, 1, 28, "batch", eval_mode=False)
    decoders["other-width"] = V.build((64, 32, 16), 16, 1, 28, "none")
    decoders["d129"] = V.build((256, 128, 64), 129, 1, 28, "none")
    decoders["linear"] = torch.nn.Sequential(torch.nn.Linear(4, 9))
    for name, dec in decoders.items():
        want = table.get(name, False)
        assert vanilla_kernels_cover(dec) == want, name
        assert native_vanilla_metric_covers(dec) == want, name
        assert not native_metric_covers(dec), name                # the spatial route's predicate keeps its meaning


def test_size_queries_and_argument_checks():
    from vqvae_amd import _lib
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    lib = _lib.load()
    ex = VanillaDecoderExport(V.build(*V.CASES["wide-bn-32x3"]), CPU)
    q, least = lib.geo_vanilla_metric_workspace_bytes, lib.geo_vanilla_metric_min_workspace_bytes
    # d = 128: a slice holds at most 32 pairs of latents
    assert 0 < least(ex.desc) == q(ex.desc, 0) == q(ex.desc, 1) == q(ex.desc, 2) < q(ex.desc, 3) < q(ex.desc, 63) == q(ex.desc, 64)
    assert q(ex.desc, 64) == q(ex.desc, 10 ** 6)
    assert q(ex.desc, -1) == 0 and q(None, 4) == 0 and least(None) == 0
    call = lib.geo_vanilla_metric_tensor
    for field, value in (("c1", 32), ("latent_dim", 129), ("latent_dim", 0), ("out_channels", 2), ("out_size", 64)):
        bad = _lib.VanillaDecoderDesc.from_buffer_copy(ex.desc)
        setattr(bad, field, value)
        assert q(bad, 4) == 0 and least(bad) == 0, field
        assert call(bad, None, None, 4, None, None, None, None, None, None, 0, None) == GEO_E_ARG, field
    assert call(ex.desc, None, None, 0, None, None, None, None, None, None, 0, None) == 0          # n == 0
    assert call(ex.desc, None, None, 4, None, None, None, None, None, None, 0, None) == GEO_E_ARG  # null pointers
    assert call(ex.desc, None, None, -1, None, None, None, None, None, None, 0, None) == GEO_E_ARG
    assert call(ex.desc, None, None, 1 << 31, None, None, None, None, None, None, 0, None) == GEO_E_ARG
    old = _lib.VanillaDecoderDesc.from_buffer_copy(ex.desc)                                        # the transposed packs are not needed
    old.w2t = old.w3t = old.Atq = None
    assert q(old, 4) == q(ex.desc, 4)
    spec = lib.geo_sym_spectrum
    assert spec(None, 0, 4, 16, None, None, None, None) == 0
    for n, d, p_out in ((2, 0, 16), (2, 129, 16), (-1, 4, 16), (2, 4, 0), (2, 4, 16)):            # the last: null pointers
        assert spec(None, n, d, p_out, None, None, None, None) == GEO_E_ARG
    assert 16 <= lib.geo_sym_spectrum_sweep_cap() <= 1024


def test_jacobian_field_on_the_autograd_route():
    from vqvae_amd.geo import PullbackMetric, pullback_metric, pullback_metric_device
    dec = V.build((64, 32, 16), 6, 1, 28, "none", seed=3)
    z = torch.randn(5, 6, generator=torch.Generator().manual_seed(1))
    plain = pullback_metric_device(dec, z)
    assert plain.route == "autograd" and plain.J is None
    res = pullback_metric_device(dec, z, jacobian=True)
    assert res.route == "autograd" and tuple(res.J.shape) == (5, 6, 784) and res.J.dtype == torch.float32
    for a, b in ((res.G, plain.G), (res.eig, plain.eig), (res.logvol, plain.logvol), (res.rank, plain.rank)):
        assert torch.equal(a, b)                                  # asking for the columns moves no bit
    J = res.J.double()
    assert torch.allclose(torch.bmm(J, J.transpose(1, 2)), res.G, rtol=1e-12, atol=0)
    host = pullback_metric(dec, z.numpy(), jacobian=True)
    assert isinstance(host, PullbackMetric) and isinstance(host.J, np.ndarray) and np.array_equal(host.J, res.J.numpy())
    assert PullbackMetric(1, 2, 3, 4, "native").J is None         # the new field is last and optional
    covered = V.build(*V.CASES["narrow-none-28"])                  # latents on the CPU: the autograd route, unchanged
    assert pullback_metric_device(covered, torch.zeros(2, 16), spectrum=False).route == "autograd"
    with pytest.raises(ValueError, match="train-mode"):
        pullback_metric_device(V.make_decoder((256, 128, 64), 16, 1, 28, "batch", eval_mode=False), torch.zeros(2, 16))


def _legacy_build(tmp, n=10, n_lcc=8):
    """A tiny uncovered vanilla decoder's checkpoint, seeded latents, the YAML and the output directory of a legacy build."""
    import yaml
    from vqvae_amd.vae import Decoder
    torch.manual_seed(11)
    dec = Decoder(1, (32, 16, 8), 4, 28, "none").eval()
    torch.save({"model_state_dict": {"decoder." + k: v for k, v in dec.state_dict().items()}}, os.path.join(tmp, "best.pt"))
    z = torch.randn(n, 4, generator=torch.Generator().manual_seed(3))
    torch.save({"z": z}, os.path.join(tmp, "z.pt"))
    out = os.path.join(tmp, "build")
    os.makedirs(out)
    codes = np.full(n, -1, dtype=np.int32)
    codes[:n_lcc] = np.arange(n_lcc) % 3
    np.save(os.path.join(out, "codes.npy"), codes)
    config = {"data": {"latents_path": os.path.join(tmp, "z.pt")}, "checkpoint_path": os.path.join(tmp, "best.pt"),
              "vae_config": dict(TINY_VAE), "graph": {"k": 3, "metric": "euclidean", "sym": "mutual", "mode": "distance"},
              "riemannian": {"mode": "full", "max_edges": 100, "batch_size": 16},
              "quantize": {"K": 3, "init": "kpp", "seed": 42}, "out": {"dir": out}}
    torch.save({"medoid_indices": np.array([0, 1, 2], dtype=np.int32), "z_medoid": z[:3], "config": config, "graph_stats": {},
                "method": "riemannian_geodesic"}, os.path.join(out, "codebook.pt"))
    with open(os.path.join(tmp, "quantize.yaml"), "w") as fh:
        yaml.safe_dump(config, fh)
    return dec, z, codes, out


def test_cli_on_the_cpu_through_both_inputs(tmp_path, monkeypatch):
    from vqvae_amd.scripts import riemann_metric_map, vanilla_metric_map as cli
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    tmp = str(tmp_path)
    dec, z, codes, build = _legacy_build(tmp)
    G64 = gram64_of(dec, z.numpy())
    by_dir = cli.main(cli.make_parser().parse_args(["--codebook_dir", build, "--out_dir", os.path.join(tmp, "a"), "--save_tensors"]))
    by_cfg = cli.main(cli.make_parser().parse_args(["--config", os.path.join(tmp, "quantize.yaml"), "--out_dir",
                                                    os.path.join(tmp, "b"), "--chunk", "4", "--save_tensors"]))
    a, b = np.load(os.path.join(tmp, "a", "metric_map.npz")), np.load(os.path.join(tmp, "b", "metric_map.npz"))
    assert set(a.files) == {"logvol", "trace", "eig_min", "eig_max", "rank", "index", "G"} == set(b.files)
    # three chunks of 4, 4, 2 latents give the arrays of one chunk.  On this route only up to float32 rounding of the columns:
    # torch's CPU convolutions block by batch size, so jacfwd's bits move with the latents per call: float32 rounding, about 1e-7
    # of a column, times cond(G), about 10 here, bounds the gates below (the native route is chunk-invariant bit for bit,
    # tests/test_gpu_vanilla_metric.py)
    assert a["index"].tobytes() == b["index"].tobytes() and a["rank"].tobytes() == b["rank"].tobytes()
    assert normalised_error(b["G"], a["G"]) <= 1e-6
    for key, rtol in (("trace", 1e-6), ("eig_max", 1e-6), ("eig_min", 1e-5)):
        np.testing.assert_allclose(b[key], a[key], rtol=rtol, err_msg=key)
    np.testing.assert_allclose(b["logvol"], a["logvol"], atol=1e-5)
    assert np.array_equal(a["index"], np.arange(10)) and a["G"].shape == (10, 4, 4) and a["rank"].dtype == np.int32
    assert normalised_error(a["G"], G64) <= 1e-5
    ev = np.linalg.eigvalsh(G64)
    np.testing.assert_allclose(a["trace"], np.einsum("naa->n", G64), rtol=1e-5)
    np.testing.assert_allclose(a["eig_max"], ev[:, -1], rtol=1e-5)
    np.testing.assert_allclose(a["eig_min"], ev[:, 0], rtol=1e-4)
    np.testing.assert_allclose(a["logvol"], 0.5 * np.linalg.slogdet(G64)[1], atol=1e-4)
    assert np.all(a["rank"] == 4)
    # the JSON: riemann_metric_map's keys plus the decoder kind; per-code statistics from codes.npy with --codebook_dir only
    with open(os.path.join(tmp, "a", "metric_map.json")) as fh:
        on_disk = json.load(fh)
    assert on_disk == json.loads(json.dumps(by_dir))
    assert by_dir["decoder"] == "vanilla" and by_dir["route"] == "autograd" and by_dir["decoder_mode"] == "eval"
    assert by_dir["n"] == by_dir["n_total"] == 10 and by_dir["latent_dim"] == 4 and by_dir["n_rank_deficient"] == 0
    assert "per_code" not in by_cfg and set(by_dir) - {"per_code"} == set(by_cfg)
    assert all(by_dir[k] == by_cfg[k] for k in ("n", "n_total", "latent_dim", "n_rank_deficient", "route", "decoder_mode", "decoder"))
    want = riemann_metric_map.per_code_stats(codes, a["logvol"])
    assert by_dir["per_code"] == want and set(want) == {"0", "1", "2"} and sum(v["count"] for v in want.values()) == 8
    for sub in ("a", "b"):
        assert os.path.getsize(os.path.join(tmp, sub, "metric_map.png")) > 0
    # a seeded subsample, without the tensors
    sub = cli.main(cli.make_parser().parse_args(["--codebook_dir", build, "--out_dir", os.path.join(tmp, "c"), "--max_latents", "6",
                                                 "--seed", "5", "--chunk", "4"]))
    c = np.load(os.path.join(tmp, "c", "metric_map.npz"))
    idx = np.sort(np.random.RandomState(5).choice(10, 6, replace=False))
    assert "G" not in c.files and np.array_equal(c["index"], idx) and np.allclose(c["logvol"], a["logvol"][idx], rtol=0, atol=1e-5)
    assert sub["n"] == 6 and sub["per_code"] == riemann_metric_map.per_code_stats(codes[idx], c["logvol"])
    with pytest.raises(SystemExit):
        cli.make_parser().parse_args(["--out_dir", "x"])          # one of --config / --codebook_dir is required
