"""Precision / recall / density / coverage without a GPU: the torch fp64 route of prdc_device / compute_prdc against the numpy
oracle on every case of prdc_cases.py, the ValueErrors (raised from shapes and dtypes alone, before the library is loaded),
the ABI rows, the CLI's argument set and its missing-encoder error."""
import os
import re

import numpy as np
import pytest
import torch

import prdc_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("geo_kth_radius", "geo_ball_count", "geo_prdc_workspace_bytes", "geo_prdc_min_workspace_bytes")


@pytest.mark.parametrize("case_id", pc.CASE_IDS)
def test_torch_route_equals_the_oracle(case_id):
    from vqvae_amd.eval.prdc import FIGURES, prdc_device
    pc.assert_margin(case_id)
    real, fake, k, exact = pc.inputs(case_id)
    o = pc.oracle(case_id)
    got = prdc_device(torch.from_numpy(real), torch.from_numpy(fake), k)
    assert got["route"] == "torch"
    for name in ("fake_count", "real_count", "real_near_idx"):
        np.testing.assert_array_equal(got[name].numpy(), o[name], err_msg=name)
    for name in ("real_radius2", "fake_radius2", "real_near_key"):
        if exact:
            np.testing.assert_array_equal(got[name].numpy(), o[name], err_msg=name)
        else:
            np.testing.assert_allclose(got[name].numpy(), o[name], rtol=1e-12, atol=0, err_msg=name)
    for name in FIGURES:
        assert got[name] == o[name], (name, got[name], o[name])


def test_narrow_fakes_score_full_precision_and_no_recall():
    """Fakes at half the reals' scale sit inside the real manifold and cover almost none of it: compute_prdc must say
    precision 1, recall near 0 (the oracle finds exactly 0 of 500 reals in a fake ball for this seed), density far above 1."""
    from vqvae_amd.eval.prdc import compute_prdc
    real, fake, k, _ = pc.inputs("narrow-500x400x32-k5")
    got = compute_prdc(real, fake, k)
    assert got["precision"] == 1.0 and got["recall"] < 0.02 and got["density"] > 10 and got["coverage"] == 1.0
    assert got == {name: pc.oracle("narrow-500x400x32-k5")[name] for name in got}


def test_compute_prdc_is_the_package_signature():
    from vqvae_amd.eval.prdc import compute_prdc
    real, fake, k, _ = pc.inputs("gauss-65x63x3-k5")
    got = compute_prdc(real_features=real.astype(np.float64), fake_features=fake, nearest_k=k)
    assert sorted(got) == ["coverage", "density", "precision", "recall"]
    o = pc.oracle("gauss-65x63x3-k5")
    assert all(isinstance(got[name], float) and got[name] == o[name] for name in got)


def test_the_torch_route_works_in_bounded_slabs(monkeypatch):
    """Blocks of a few rows: the blocked passes give what one slab gives."""
    from vqvae_amd.eval import prdc
    real, fake, k, _ = pc.inputs("grid-193x200x5-k3-hi3")
    R, F = torch.from_numpy(real), torch.from_numpy(fake)
    ref = prdc.prdc_device(R, F, k)
    monkeypatch.setattr(prdc, "_blocks", lambda d: (7, 13))
    got = prdc.prdc_device(R, F, k)
    for name, v in ref.items():
        assert torch.equal(v, got[name]) if isinstance(v, torch.Tensor) else v == got[name], name


def test_value_errors_come_from_shapes_and_dtypes_alone(monkeypatch):
    from vqvae_amd import _lib
    from vqvae_amd.eval.prdc import ball_count_device, compute_prdc, kth_radius_device, prdc_device

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    a = torch.zeros(10, 4)
    r2 = torch.ones(10, dtype=torch.float64)
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match="outside"):
            kth_radius_device(a, k)
        with pytest.raises(ValueError, match="outside"):
            prdc_device(a, a, k)
    with pytest.raises(ValueError, match="at least k"):
        kth_radius_device(a, 10)                                            # k >= n
    with pytest.raises(ValueError, match="at least k"):
        prdc_device(torch.zeros(30, 4), a, 10)                              # k >= m
    with pytest.raises(ValueError, match="at least k"):
        prdc_device(a, torch.zeros(30, 4), 10)                              # k >= n
    with pytest.raises(ValueError, match="columns"):
        prdc_device(a, torch.zeros(10, 5), 3)
    with pytest.raises(ValueError, match="columns"):
        ball_count_device(a, r2, torch.zeros(3, 5))
    with pytest.raises(ValueError, match="1024"):
        kth_radius_device(torch.zeros(4, 1025), 1)
    with pytest.raises(ValueError, match="1024"):
        ball_count_device(torch.zeros(4, 1025), r2[:4], torch.zeros(2, 1025))
    for bad in (a.double(), a.half(), a.long()):
        with pytest.raises(ValueError, match="float32"):
            kth_radius_device(bad, 3)
        with pytest.raises(ValueError, match="float32"):
            ball_count_device(a, r2, bad)
        with pytest.raises(ValueError, match="float32"):
            prdc_device(bad, a, 3)
    with pytest.raises(ValueError, match="float64"):
        ball_count_device(a, r2.float(), a)
    with pytest.raises(ValueError, match="2-D"):
        kth_radius_device(torch.zeros(10), 3)
    for poison in (float("nan"), float("inf")):
        b = a.clone()
        b[3, 2] = poison
        with pytest.raises(ValueError, match="non-finite"):
            prdc_device(a, b, 3)
        with pytest.raises(ValueError, match="non-finite"):
            prdc_device(b, a, 3)
        with pytest.raises(ValueError, match="non-finite"):
            compute_prdc(b.numpy(), a.numpy(), 3)
    # CPU tensors are not the device callers' business, and they say so before any library call
    with pytest.raises(ValueError, match="CUDA"):
        kth_radius_device(a, 3)
    with pytest.raises(ValueError, match="CUDA"):
        ball_count_device(a, r2, a)


def test_symbols_are_in_the_binding_and_the_header():
    from vqvae_amd import _lib
    header = open(os.path.join(ROOT, "include", "geo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and re.search(rf"\b{name}\s*\(", code) and hasattr(lib, name), name
    assert "#define GEO_PRDC_MAX_K 64" in header
    # host-only answers: the queries and the refusals need no GPU
    lo = lib.geo_prdc_min_workspace_bytes(16)
    assert lo > 0 and lib.geo_prdc_min_workspace_bytes(1024) == lo and lib.geo_prdc_min_workspace_bytes(1025) == 0
    assert lib.geo_prdc_workspace_bytes(50000, 50000, 512) >= lib.geo_prdc_workspace_bytes(64, 64, 512) >= lo
    assert lib.geo_prdc_workspace_bytes(1 << 31, 5, 8) == 0 and lib.geo_prdc_workspace_bytes(5, 5, 0) == 0
    assert lib.geo_kth_radius(None, 5, 3, 1, None, None, 0, None) == -1 and b"null" in lib.geo_last_error()


def test_cli_argument_set():
    from vqvae_amd.scripts.evaluate_generation import make_parser
    p = make_parser()
    options = {o for a in p._actions for o in a.option_strings} - {"-h", "--help"}
    assert options == {"--config", "--dataset", "--data_root", "--split", "--num_samples", "--k", "--max_real", "--out_dir", "--seed"}
    args = p.parse_args(["--config", "g.yaml", "--dataset", "FashionMNIST"])
    assert (args.split, args.k, args.data_root, args.max_real, args.out_dir, args.seed) == ("test", 5, "data", None, None, None)
    assert p.parse_args(["--config", "g.yaml", "--dataset", "CIFAR10", "--split", "train"]).split == "train"
    with pytest.raises(SystemExit):
        p.parse_args(["--config", "g.yaml", "--dataset", "x", "--split", "val"])
    with pytest.raises(SystemExit):
        p.parse_args(["--dataset", "FashionMNIST"])


def test_a_checkpoint_without_an_encoder_is_refused_by_name(tmp_path):
    from test_prior_sample_host import tiny_setup
    from vqvae_amd.scripts.evaluate_generation import load_model
    _, cfg = tiny_setup(str(tmp_path), vanilla=True)                        # its vae.pt holds decoder.* entries only
    with pytest.raises(ValueError) as err:
        load_model(cfg, torch.device("cpu"))
    text = str(err.value)
    assert "encoder.fc_mu.weight" in text and "encoder.conv_layers" in text and "decoder.*" in text and cfg["vae_ckpt_path"] in text
    spatial = tmp_path / "spatial"
    spatial.mkdir()
    _, cfg = tiny_setup(str(spatial), vanilla=False)                        # a whole SpatialVAE: loads, in eval mode
    model = load_model(cfg, torch.device("cpu"))
    assert not model.training and hasattr(model, "encoder") and hasattr(model, "decoder")
