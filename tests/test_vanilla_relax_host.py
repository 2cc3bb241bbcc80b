"""Curve relaxation under the vanilla decoder on the host: which decoders the native route admits, that the predicates of the
spatial route keep their meaning, that CPU frames keep the torch route, the size queries, and how the interpolation CLI reads a
directory written by build_riemannian_codebook_legacy."""
import dataclasses
import os

import numpy as np
import pytest
import torch
from scipy import sparse

import relax_cases as rc
import vanilla_jvp_cases as V

CPU = torch.device("cpu")
GEO_E_ARG = -1                          # include/geo_hip.h
LEGACY_VAE = dict(in_channels=1, enc_channels=[32, 64, 128], dec_channels=[128, 64, 32], latent_dim=16, recon_loss="bce",
                  output_image_size=28, norm_type="none", mse_use_sigmoid=True)


def test_the_native_route_admits_exactly_the_covered_decoders():
    from vqvae_amd.geo import native_metric_covers, native_relax_covers, native_vanilla_relax_covers
    from vqvae_amd.geo.relaxation import native_vanilla_relax_covers as from_module
    from vqvae_amd.vanilla_decoder import vanilla_kernels_cover
    assert from_module is native_vanilla_relax_covers
    covered = [V.build(*spec) for spec in list(V.CASES.values()) + list(V.ENVELOPE_CASES.values())]
    uncovered = [V.make_decoder((128, 64, 32), 16, 1, 28, "group"), V.make_decoder((128, 64, 32), 16, 1, 28, "batch", eval_mode=False),
                 V.make_decoder((32, 32, 16), 8, 1, 28, "none"), V.make_decoder((256, 128, 64), 129, 1, 28, "none")]
    for dec in covered:
        assert native_vanilla_relax_covers(dec) and vanilla_kernels_cover(dec)
        assert not native_relax_covers(dec) and not native_metric_covers(dec)       # the spatial route's predicates keep their meaning
    for dec in uncovered:
        assert not native_vanilla_relax_covers(dec) and not vanilla_kernels_cover(dec) and not native_relax_covers(dec)
    from metric_tensor_cases import NATIVE, make_decoder
    spatial = make_decoder(NATIVE[0])[0]
    assert native_relax_covers(spatial) and not native_vanilla_relax_covers(spatial)


def test_cpu_frames_keep_the_torch_route():
    from vqvae_amd.geo import CurveEnergy, curve_energy_device, relax_curves_device
    assert [f.name for f in dataclasses.fields(CurveEnergy)][-1] == "trace"
    assert CurveEnergy(1, 2, 3, 4, 5, "torch").trace is None
    dec = V.build(*V.CASES["narrow-none-32x3-d5"])
    x = torch.from_numpy(rc.zigzags(5, 3, 1))
    e = curve_energy_device(dec, x, trace=True)
    assert e.route == "torch" and e.trace is None and e.jac is None and e.outputs.shape == (1, 3, 3072)
    assert e.energy.dtype == torch.float64 and bool((e.grad[:, 0] == 0).all()) and bool(e.grad[:, 1].abs().sum() > 0)
    r = relax_curves_device(dec, x, 1)
    assert r.route == "torch" and bool((r.energy <= r.energy0).all())


def test_an_export_is_refused_a_jacobian_and_foreign_frames():
    from vqvae_amd.geo import curve_energy_device
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    ex = VanillaDecoderExport(V.build(*V.CASES["narrow-none-32x3-d5"]), CPU)
    x = torch.from_numpy(rc.zigzags(5, 3, 1))
    with pytest.raises(ValueError, match="Jacobian"):
        curve_energy_device(ex, x, jacobian=True)
    with pytest.raises(ValueError, match="latent dimensions"):
        curve_energy_device(ex, torch.zeros(1, 3, 4))


def test_size_queries_and_argument_checks():
    from vqvae_amd import _lib
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    lib = _lib.load()
    ex = VanillaDecoderExport(V.build(*V.CASES["wide-bn-32x3"]), CPU)
    q, least = lib.geo_vanilla_curve_workspace_bytes, lib.geo_vanilla_curve_min_workspace_bytes
    assert 0 < least(ex.desc, 9) == q(ex.desc, 1, 9) == q(ex.desc, 0, 9) < q(ex.desc, 7, 9) < q(ex.desc, 455, 9) == q(ex.desc, 10 ** 6, 9)
    assert least(ex.desc, 2) < least(ex.desc, 64)
    for F in (1, 65, 0, -3):
        assert q(ex.desc, 3, F) == 0 and least(ex.desc, F) == 0
        assert lib.geo_vanilla_curve_energy(ex.desc, None, 3, F, None, None, None, None, None, None, 0, None) == GEO_E_ARG
    assert q(ex.desc, -1, 9) == 0 and q(None, 3, 9) == 0 and least(None, 9) == 0
    assert lib.geo_vanilla_curve_relax(ex.desc, None, 3, 9, -1, None, None, None, None, None, None, 0, None) == GEO_E_ARG
    for field, value in (("c1", 32), ("latent_dim", 129), ("out_channels", 2), ("out_size", 64)):
        bad = _lib.VanillaDecoderDesc.from_buffer_copy(ex.desc)
        setattr(bad, field, value)
        assert q(bad, 3, 9) == 0 and least(bad, 9) == 0, field
        assert lib.geo_vanilla_curve_relax(bad, None, 3, 9, 1, None, None, None, None, None, None, 0, None) == GEO_E_ARG, field


def _legacy_dir(tmp, n=40, n_lcc=36):
    """A directory with the legacy builder's artefacts over seeded latents (a ring graph over the first n_lcc rows)."""
    z = torch.randn(n, 16, generator=torch.Generator().manual_seed(3))
    torch.save({"z": z}, os.path.join(tmp, "z.pt"))
    out = os.path.join(tmp, "out")
    os.makedirs(out)
    codes = np.full(n, -1, dtype=np.int32)
    codes[:n_lcc] = np.arange(n_lcc) % 4
    np.save(os.path.join(out, "codes.npy"), codes)
    ring = sparse.csr_matrix((np.ones(n_lcc, dtype=np.float32), (np.arange(n_lcc), (np.arange(n_lcc) + 1) % n_lcc)), shape=(n_lcc, n_lcc))
    sparse.save_npz(os.path.join(out, "knn_graph_riemannian.npz"), (ring + ring.T).tocsr())
    config = {"data": {"latents_path": os.path.join(tmp, "z.pt")}, "checkpoint_path": os.path.join(tmp, "best.pt"),
              "vae_config": dict(LEGACY_VAE), "graph": {"k": 10, "metric": "euclidean", "sym": "mutual", "mode": "distance"},
              "riemannian": {"mode": "full", "max_edges": 1000, "batch_size": 256},
              "quantize": {"K": 4, "init": "kpp", "seed": 42}, "out": {"dir": out}}
    medoids = np.array([0, 5, 11, 30], dtype=np.int32)
    torch.save({"medoid_indices": medoids, "z_medoid": z[:n_lcc][torch.from_numpy(medoids).long()], "config": config,
                "graph_stats": {}, "method": "riemannian_geodesic"}, os.path.join(out, "codebook.pt"))
    return out, z


def test_the_cli_reads_a_legacy_directory(tmp_path):
    from pathlib import Path
    from vqvae_amd.scripts.geodesic_interpolation import is_legacy_build, load_legacy_build, make_parser
    out, z = _legacy_dir(str(tmp_path))
    assert is_legacy_build(Path(out)) and not is_legacy_build(tmp_path)
    job, apply_sigmoid, W, z_read, rows = load_legacy_build(Path(out))
    assert apply_sigmoid and job.vae_config["latent_dim"] == 16 and str(job.checkpoint).endswith("best.pt")
    assert torch.equal(z_read, z) and np.array_equal(rows, np.arange(36)) and W.shape == (36, 36)
    other = os.path.join(str(tmp_path), "other.pt")
    torch.save(z.flip(0).contiguous(), other)
    with pytest.raises(ValueError, match="do not belong together"):
        load_legacy_build(Path(out), other)
    # a spatial build's codebook.pt (4-D latents, 2-D z_medoid) without knn_graph_riemannian.npz is not a legacy build
    spatial = tmp_path / "spatial"
    spatial.mkdir()
    torch.save({"z_medoid": torch.zeros(4, 16), "config": {}}, spatial / "codebook.pt")
    assert not is_legacy_build(spatial)
    args = make_parser().parse_args(["--codebook_dir", out, "--out_dir", "o", "--pairs", "0:5", "--relax_iters", "3"])
    assert args.relax_iters == 3 and args.frames == 9


def test_an_export_does_not_take_cpu_frames():
    from vqvae_amd.geo import relax_curves_device
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    ex = VanillaDecoderExport(V.build(*V.CASES["narrow-none-32x3-d5"]), CPU)
    with pytest.raises(ValueError, match="on its GPU"):
        relax_curves_device(ex, torch.from_numpy(rc.zigzags(5, 3, 1)), 1)
