"""The HIP EMA quantizer (csrc/kmeans.hip geo_vq_*, vqvae_amd.baseline) on the GPU: every row's label against fp64 brute force,
parity with the reference's fixture, the backward, determinism, eval mode, reseeding, and the three CLIs end to end on a
synthetic CIFAR-10 directory."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_rules as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _quant(K, C, seed=0, embed=None):
    from vqvae_amd.baseline import VectorQuantizerEMA
    torch.manual_seed(seed)
    q = VectorQuantizerEMA(n_codes=K, code_dim=C)
    if embed is not None:
        q.embed.copy_(torch.as_tensor(embed))
        q.embed_avg.copy_(q.embed)
    return q.cuda()


def _brute_labels(z: torch.Tensor, embed: torch.Tensor) -> torch.Tensor:
    """fp64 argmin (first minimum) on the device, 512 rows at a time."""
    x = z.double().permute(0, 2, 3, 1).reshape(-1, z.shape[1])
    e = embed.double()
    return torch.cat([((x[i:i + 512, None, :] - e[None]) ** 2).sum(-1).argmin(1) for i in range(0, x.shape[0], 512)])


def _check_labels(z, q):
    idx = q(z)[2].reshape(-1)
    want = _brute_labels(z, q.embed)
    assert torch.equal(idx, want), f"{int((idx != want).sum())} rows differ"


def test_labels_random_cifar_shape():
    q = _quant(512, 128).eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    z = torch.randn(128, 128, 8, 8, device="cuda", generator=g) * 1.5
    _check_labels(z, q)


def test_labels_planted_ties_and_duplicates():
    r = np.random.RandomState(2)
    K, C = 64, 16
    emb = r.randint(-3, 4, (K, C)).astype(np.float32)
    emb[40] = emb[7]                                   # duplicate codes: 7 must win
    emb[50] = emb[7]
    q = _quant(K, C, embed=emb).eval()
    a, b = r.randint(0, K, 200), r.randint(0, K, 200)
    rows = (emb[a] + emb[b]) / 2                       # exact midpoints: exact ties between a and b
    rows[:20] = emb[7]
    z = torch.from_numpy(rows.reshape(8, 25, C).transpose(0, 2, 1).reshape(8, C, 5, 5).copy()).cuda()
    _check_labels(z, q)


def test_labels_f16_and_more_codes_than_rows():
    q = _quant(512, 128, seed=3).eval()
    z = (torch.randn(16, 128, 8, 8, device="cuda") * 1.5).half()
    _check_labels(z, q)
    q2 = _quant(4096, 32, seed=4).eval()
    z2 = torch.randn(1, 32, 2, 3, device="cuda")     # n = 6 rows, K = 4096
    _check_labels(z2, q2)


def test_golden_parity(golden):
    fx = golden("vqvae_baseline")
    K, C, B, H, W, steps = (int(v) for v in fx["dims"])
    q = _quant(K, C, seed=int(fx["seed"]))
    assert np.array_equal(q.embed.cpu().numpy(), fx["embed0"])
    for s in range(steps + 1):
        q.train(s < steps)
        before = q.embed.cpu().numpy().copy()
        z = torch.from_numpy(fx["z_e"][s]).cuda()
        z_q_st, loss, idx, z_q, z_e = q(z)
        assert np.array_equal(idx.cpu().numpy(), fx[f"idx_{s}"])
        want = R.forward(fx["z_e"][s], before, None, None, training=False, idx=idx.cpu().numpy())
        assert np.array_equal(z_q.cpu().numpy(), want["z_q"]) and np.array_equal(z_q_st.cpu().numpy(), want["z_q_st"])
        np.testing.assert_allclose(loss.item(), fx[f"loss_{s}"], rtol=1e-6)
        st = q.last_stats.cpu().numpy()
        np.testing.assert_allclose(st, [want["q_mse"], want["perplex"], want["usage"], want["dead"]], rtol=1e-6)
        for b in ("cluster_size", "embed_avg", "embed"):
            np.testing.assert_allclose(getattr(q, b).cpu().numpy(), fx[f"{b}_{s}"], rtol=1e-6, atol=1e-6, err_msg=f"{b} {s}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_backward_matches_rules(dtype):
    q = _quant(64, 32, seed=5).eval()
    z = (torch.randn(4, 32, 8, 8, device="cuda") * 1.5).to(dtype).requires_grad_()
    z_q_st, loss, *_ = q(z)
    g = torch.randn_like(z_q_st)
    ((z_q_st * g).sum() + loss * 3.0).backward()
    assert z.grad.dtype == dtype
    want = R.backward(g.cpu().numpy(), 3.0, z.detach().float().cpu().numpy(), z_q_st.detach().cpu().numpy())
    tol = 1e-6 if dtype == torch.float32 else 1e-3
    np.testing.assert_allclose(z.grad.float().cpu().numpy(), want, rtol=tol, atol=tol * 1e-2)


def _run(q, z):
    out = q(z)
    torch.cuda.synchronize()
    return [out[0], out[1], out[2], out[3], q.last_stats.clone(), q.embed.clone(), q.cluster_size.clone(), q.embed_avg.clone()]


def test_runs_and_streams_bit_identical():
    z = torch.randn(128, 128, 8, 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6)) * 1.5
    outs = []
    for stream in (None, None, torch.cuda.Stream()):
        q = _quant(512, 128, seed=7).train()
        q.cluster_size.fill_(3.0)
        if stream is None:
            outs.append(_run(q, z))
        else:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                outs.append(_run(q, z))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)


def test_eval_mode_keeps_codebook_state():
    q = _quant(512, 128, seed=8).eval()
    before = [b.clone() for b in (q.embed, q.cluster_size, q.embed_avg)]
    q(torch.randn(8, 128, 8, 8, device="cuda"))
    for a, b in zip(before, (q.embed, q.cluster_size, q.embed_avg)):
        assert torch.equal(a, b)


def test_reseed_dead_codes():
    q = _quant(64, 16, seed=9)
    q.cluster_size.copy_(torch.arange(64, device="cuda").float())   # codes 0..4 are dead at min_count 5
    bank = torch.randn(3, 16, device="cuda")
    torch.cuda.manual_seed(11)
    assert q.reseed_dead_codes(min_count=5, sample_bank=bank) == 3
    torch.cuda.manual_seed(11)
    perm = torch.randperm(3, device="cuda")[:3]
    assert torch.equal(q.embed[:3], bank[perm]) and torch.equal(q.embed_avg[:3], bank[perm])
    assert q.cluster_size[:3].tolist() == [5.0] * 3 and q.cluster_size[3:5].tolist() == [3.0, 4.0]
    assert q.reseed_dead_codes(5, None) == 0


# ------------------------------------------------------------------------------------------------------------------ CLIs
def _synthetic_cifar(root, n_train_per=5, n_test=20, seed=0):
    r = np.random.RandomState(seed)
    d = os.path.join(root, "cifar-10-batches-py")
    os.makedirs(d, exist_ok=True)
    for name, n in [(f"data_batch_{i}", n_train_per) for i in range(1, 6)] + [("test_batch", n_test)]:
        img = r.randint(0, 256, (n, 3, 8, 8)).repeat(4, 2).repeat(4, 3)     # blocky images: something to reconstruct
        with open(os.path.join(d, name), "wb") as f:
            pickle.dump({"data": img.reshape(n, 3072).astype(np.uint8), "labels": (np.arange(n) % 10).tolist()}, f)


def _config(tmp, amp):
    cfg = {"seed": 42,
           "data": {"root": os.path.join(tmp, "data"), "num_workers": 0, "img_size": 32, "normalize_mean": [0.5] * 3,
                    "normalize_std": [0.5] * 3},
           "train": {"batch_size": 8, "epochs": 1, "lr": 2e-4, "weight_decay": 0.0, "grad_clip": 1.0, "amp": amp},
           "model": {"in_channels": 3, "z_channels": 32, "hidden": 64, "n_res_blocks": 2, "n_codes": 64, "beta": 0.25,
                     "ema_decay": 0.99, "ema_eps": 1e-5},
           "log": {"samples_every": 1, "save_best": True}}
    path = os.path.join(tmp, f"config_{int(amp)}.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path, cfg


def _cli(args, cwd, timeout=240):
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


@pytest.fixture(scope="module")
def trained(tmp_path_factory, golden):
    tmp = str(tmp_path_factory.mktemp("vqvae_cli"))
    _synthetic_cifar(os.path.join(tmp, "data"))
    runs = {}
    for amp in (True, False):
        cfg_path, cfg = _config(tmp, amp)
        out = os.path.join(tmp, f"out_{int(amp)}")
        log = _cli(["vqvae_amd.scripts.train_vqvae_baseline", "--config", cfg_path, "--out_dir", out], tmp)
        runs[amp] = (cfg_path, cfg, out, log)
    return tmp, runs, golden("vqvae_baseline")


@pytest.mark.parametrize("amp", [True, False])
def test_train_cli_writes_reference_files(trained, amp):
    from vqvae_amd.baseline.model import model_from_config
    from vqvae_amd.baseline.train import LOG_HEADER
    tmp, runs, fx = trained
    cfg_path, cfg, out, log = runs[amp]
    assert "Epoch 1/1 | train loss:" in log and "Training finished in" in log
    lines = open(os.path.join(out, "log.csv")).read().splitlines()
    assert lines[0] == ",".join(LOG_HEADER) and len(lines) == 3
    assert lines[1].startswith("1,train,") and lines[2].startswith("1,val,")
    assert all(np.isfinite(float(v)) for v in lines[1].split(",")[2:])
    assert os.path.exists(os.path.join(out, "recon_epoch0001.png"))
    for name in ("ckpt_last.pt", "ckpt_best.pt"):
        st = torch.load(os.path.join(out, "checkpoints", name), map_location="cpu", weights_only=False)
        assert sorted(st) == ["cfg", "epoch", "model", "opt"] and st["epoch"] == 1 and st["cfg"] == cfg
        assert list(st["model"].keys()) == [str(n) for n in fx["sd_names"]]
        m = model_from_config(cfg)
        m.load_state_dict(st["model"], strict=True)
        assert torch.equal(m.quant.embed, st["model"]["quant.embed"])


def _restated_metrics(cfg, ckpt):
    """eval_codebook_metrics restated: model convolutions in torch on the GPU, the quantizer by vq_rules."""
    from vqvae_amd.baseline.data import load_split
    from vqvae_amd.baseline.model import model_from_config
    model = model_from_config(cfg).cuda().eval()
    model.load_state_dict(torch.load(ckpt, map_location="cuda")["model"])
    emb = model.quant.embed.cpu().numpy()
    data = load_split(cfg, "test", "cuda")
    acc, n, codes = np.zeros(7), 0, []
    with torch.no_grad():
        for x in data.ordered_batches(cfg["train"]["batch_size"]):
            z = model.enc(x)
            o = R.forward(z.cpu().numpy(), emb, None, None, training=False)
            x_rec = model.dec(torch.from_numpy(o["z_q_st"]).cuda())
            rec = torch.nn.functional.l1_loss(x_rec, x).item()
            vals = [rec + float(o["loss"]), rec, o["loss"], o["q_mse"], o["perplex"], o["usage"], o["dead"]]
            acc += np.array(vals, np.float64) * x.size(0)
            n += x.size(0)
            codes.append(o["idx"].reshape(-1))
    return dict(zip(["loss", "rec", "vq", "q_mse", "perplex", "usage", "dead"], acc / n)), np.concatenate(codes)


def test_eval_codebook_cli(trained):
    tmp, runs, _ = trained
    cfg_path, cfg, out, _ = runs[False]
    ckpt = os.path.join(out, "checkpoints", "ckpt_last.pt")
    log = _cli(["vqvae_amd.scripts.eval_vqvae_codebook", "--config", cfg_path, "--ckpt", ckpt, "--split", "test"], tmp)
    assert "Split: test" in log
    rows = open(os.path.join(tmp, "outputs", "codebook_eval_test.csv")).read().splitlines()
    assert rows[0] == "split,loss,rec,vq,q_mse,perplex,usage,dead,embed_norm_mean,embed_norm_min,embed_norm_max"
    got = dict(zip(rows[0].split(",")[1:], map(float, rows[1].split(",")[1:])))
    want, _ = _restated_metrics(cfg, ckpt)
    for k in ("vq", "q_mse", "perplex", "usage", "dead"):
        assert got[k] == pytest.approx(want[k], rel=1e-6, abs=1e-9), k
    for k in ("loss", "rec"):
        assert got[k] == pytest.approx(want[k], rel=1e-5), k


def test_evaluate_baseline_cli(trained):
    import json
    tmp, runs, _ = trained
    cfg_path, cfg, out, _ = runs[True]
    ckpt = os.path.join(out, "checkpoints", "ckpt_best.pt")
    ev = os.path.join(tmp, "evaluation")
    log = _cli(["vqvae_amd.scripts.evaluate_baseline", "--checkpoint", ckpt, "--out_dir", ev, "--max_samples", "16",
                "--gen_samples", "20"], tmp)
    assert "Reconstruction Results:" in log and "Generation Results:" in log
    res = json.load(open(os.path.join(ev, "evaluation_results.json")))
    health = json.load(open(os.path.join(ev, "codebook_health.json")))
    assert health == res["codebook_health"] and health["codebook_size"] == 64
    assert res["reconstruction_quality"]["samples_evaluated"] == 16
    assert res["generation_quality"]["samples_generated"] == 20 and res["generation_quality"]["samples_per_class"] == 2
    m = yaml.safe_load(open(os.path.join(ev, "metrics.yaml")))
    assert set(m) == {"PSNR", "SSIM"} and float(m["PSNR"]) == pytest.approx(res["generation_quality"]["psnr"], abs=1e-4)
    _, codes = _restated_metrics(cfg, ckpt)
    counts = np.bincount(codes[:16], minlength=64)   # the reference keeps the first max_samples codes.astype(np.float64)
    p = np.maximum(counts / counts.sum(), 1e-12)
    assert health["entropy"] == pytest.approx(float(-(p * np.log(p)).sum()), abs=2e-6)
    assert health["used_codes"] == int((counts > 0).sum())
    for f in ("generated_samples.png", "comparison_grid.png"):
        assert os.path.exists(os.path.join(ev, f))


# ----------------------------------------------------------------------------------- non-finite rows, skew, K > n, arguments
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("training", [False, True])
def test_non_finite_rows_match_host(dtype, training):
    """A NaN row and an infinite row get a real code (0, as on the host and under torch.argmin) and the loss comes out NaN."""
    z = torch.randn(4, 32, 8, 8) * 1.5
    z[1, 5, 2, 3] = float("nan")
    z[2, 0, 7, 7] = float("inf")
    z[3, 9, 0, 0] = -float("inf")
    z = z.to(dtype)
    q_dev = _quant(64, 32, seed=12).train(training)
    q_cpu = _quant(64, 32, seed=12).cpu().train(training)
    z_q_st, loss, idx, z_q, _ = q_dev(z.cuda())
    h_st, h_loss, h_idx, h_zq, _ = q_cpu(z.float())
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu(), h_idx)
    assert idx[1, 2, 3] == 0 and idx[2, 7, 7] == 0 and idx[3, 0, 0] == 0
    assert torch.isnan(loss).item() and torch.isnan(h_loss).item()
    assert torch.equal(z_q.cpu(), h_zq)
    assert torch.equal(torch.isnan(z_q_st.cpu()), torch.isnan(h_st))
    fin = ~torch.isnan(h_st)
    assert torch.equal(z_q_st.cpu()[fin], h_st[fin])
    for b in ("cluster_size", "embed_avg", "embed"):
        np.testing.assert_allclose(getattr(q_dev, b).cpu().numpy(), getattr(q_cpu, b).numpy(), rtol=1e-6, atol=1e-6,
                                   equal_nan=True, err_msg=b)


def _check_training_step(q, z, K):
    """One training forward against vq_rules at the kernel's labels (themselves checked against fp64 brute force)."""
    emb, cs, ea = (b.cpu().numpy().copy() for b in (q.embed, q.cluster_size, q.embed_avg))
    z_q_st, loss, idx, z_q, _ = q(z)
    assert torch.equal(idx.reshape(-1), _brute_labels(z.float(), torch.from_numpy(emb).cuda()))
    want = R.forward(z.float().cpu().numpy(), emb, cs, ea, training=True, idx=idx.cpu().numpy())
    assert np.array_equal(z_q.cpu().numpy(), want["z_q"]) and np.array_equal(z_q_st.cpu().numpy(), want["z_q_st"])
    np.testing.assert_allclose(loss.item(), want["loss"], rtol=1e-6)
    np.testing.assert_allclose(q.last_stats.cpu().numpy(), [want["q_mse"], want["perplex"], want["usage"], want["dead"]],
                               rtol=1e-6)
    for b in ("cluster_size", "embed_avg", "embed"):
        np.testing.assert_allclose(getattr(q, b).cpu().numpy(), want[b], rtol=1e-6, atol=1e-6, err_msg=b)
    return want["counts"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_training_step_skewed_cifar_shape(dtype):
    """8192 rows x 128, K 512, most rows on one code: that code's run spans ~120 tiles of the per-code sums."""
    K, C = 512, 128
    g = torch.Generator(device="cuda").manual_seed(13)
    q = _quant(K, C, seed=13).train()
    q.embed[5] = 0.0
    q.cluster_size.copy_(torch.rand(K, device="cuda", generator=g) * 20)
    q.embed_avg.copy_(q.embed * q.cluster_size[:, None])
    z = torch.randn(128, C, 8, 8, device="cuda", generator=g) * 0.05                       # near code 5
    pick = torch.randint(0, K, (8,), device="cuda", generator=g)
    z[:8] = q.embed[pick][:, :, None, None] + 0.3 * torch.randn(8, C, 8, 8, device="cuda", generator=g)
    counts = _check_training_step(q, z.to(dtype), K)
    assert counts[5] > 7000 and (counts > 0).sum() >= 5


def test_training_step_more_codes_than_rows():
    q = _quant(4096, 32, seed=14).train()
    z = torch.randn(1, 32, 2, 3, device="cuda") * 1.5                                        # n = 6 rows
    counts = _check_training_step(q, z, 4096)
    assert counts.sum() == 6


def test_mismatched_codebook_is_rejected():
    q = _quant(64, 64, seed=15)
    with pytest.raises(ValueError, match="embed"):
        q(torch.randn(2, 128, 4, 4, device="cuda"))
    q2 = _quant(64, 32, seed=15)
    q2.cluster_size = q2.cluster_size.double()
    with pytest.raises(ValueError, match="cluster_size"):
        q2(torch.randn(2, 32, 4, 4, device="cuda"))
