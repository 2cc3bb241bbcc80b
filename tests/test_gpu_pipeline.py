"""End-to-end build_codebook CLI on the GPU against the reference CLI's artefacts (golden, config C1)."""
import os

import numpy as np
import pytest
import torch
from scipy import sparse

pytestmark = pytest.mark.gpu


def _write_inputs(tmp, d, cout, size, norm, seed, n_img):
    from oracle import metric as om
    sd = om.make_decoder_state(seed, d, cout, norm_type=norm)
    z4 = np.random.RandomState(seed).randn(n_img * 16, d).astype(np.float32).reshape(n_img, 4, 4, d)
    z4 = np.ascontiguousarray(np.transpose(z4, (0, 3, 1, 2)))
    state = {"decoder." + k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    state["encoder.fc_mu.weight"] = torch.zeros(d, 256, 1, 1)          # encoder keys are ignored by the CLI
    torch.save({"model_state_dict": state, "epoch": 0}, os.path.join(tmp, "best.pt"))
    torch.save(torch.from_numpy(z4), os.path.join(tmp, "z.pt"))
    return sd, z4


def test_cli_c1_matches_reference_artefacts(golden, tmp_path):
    from vqvae_amd.scripts.build_codebook import main, make_parser
    g = golden("cli")
    d, cout, size, seed, n_img = [int(x) for x in g["c1_fm/meta"]]
    tmp = str(tmp_path)
    _write_inputs(tmp, d, cout, size, "batch", seed, n_img)
    out = os.path.join(tmp, "out")
    args = make_parser().parse_args([
        "--latents_path", os.path.join(tmp, "z.pt"), "--out_dir", out, "--vae_ckpt_path", os.path.join(tmp, "best.pt"),
        "--in_channels", str(cout), "--output_image_size", str(size), "--latent_dim", str(d),
        "--enc_channels", "64", "128", "256", "--dec_channels", "256", "128", "64", "--recon_loss", "mse",
        "--norm_type", "batch", "--mse_use_sigmoid", "--k", "20", "--sym", "union", "--K", "64", "--init", "kpp",
        "--seed", "42", "--batch_size", "512"])
    main(args)
    codes = np.load(os.path.join(out, "codes.npy"))
    cb = torch.load(os.path.join(out, "codebook.pt"), weights_only=False)
    W = sparse.load_npz(os.path.join(out, "knn_graph_geodesic.npz"))
    assert codes.dtype == np.int32 and codes.shape == (n_img, 4, 4)
    np.testing.assert_array_equal(codes, g["c1_fm/codes"])
    assert cb["medoid_indices"].dtype == np.int32
    np.testing.assert_array_equal(cb["medoid_indices"], g["c1_fm/medoid_indices"])
    assert cb["z_medoid"].dtype == torch.float32
    np.testing.assert_array_equal(cb["z_medoid"].numpy(), g["c1_fm/z_medoid"])
    assert sorted(cb["config"].keys()) == list(g["c1_fm/config_keys"])
    assert W.dtype == np.float32 and W.format == "csr"
    W.sort_indices()
    np.testing.assert_array_equal(W.indptr, g["c1_fm/indptr"])
    np.testing.assert_array_equal(W.indices, g["c1_fm/indices"])
    rel = np.abs(W.data - g["c1_fm/data"]) / g["c1_fm/data"]
    # >= 99.9 % of the weights within 1e-5; the few outliers are ReLU pre-activations that sit
    # on their f32 rounding boundary (the reference itself moves by ~1e-3 there between f32 and fp64)
    assert np.mean(rel <= 1e-5) >= 0.999 and rel.max() < 1e-2, (np.mean(rel <= 1e-5), rel.max())


def test_pipeline_with_disconnected_graph_vs_oracle(tmp_path):
    """k=1 mutual graph: many components -> LCC compaction, codes = -1 outside, LCC-local medoid ids."""
    from oracle import pipeline as op
    from vqvae_amd._device import device
    from vqvae_amd.scripts.build_codebook import build_codebook_device
    from vqvae_amd.spatial_decoder import SpatialDecoder
    sd, z4 = _write_inputs(str(tmp_path), 16, 1, 28, "batch", 5, 40)
    dec = SpatialDecoder(1, (256, 128, 64), 16, 28, "batch")
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    dev = device()
    z_flat = torch.from_numpy(op.flatten_latents(z4)).to(dev)
    res = build_codebook_device(z_flat, dec.to(dev).train(), k=2, sym="mutual", K=8, init="kpp", seed=1, batch_size=64)
    ref = op.build_codebook(z4, sd, "batch", 28, k=2, sym="mutual", K=8, init="kpp", seed=1, batch_size=64, training=True)
    np.testing.assert_array_equal(res["mask_lcc"], ref["mask_lcc"])
    assert res["mask_lcc"].sum() < z_flat.shape[0]
    np.testing.assert_array_equal(res["assign_flat"].reshape(ref["codes"].shape), ref["codes"])
    np.testing.assert_array_equal(res["medoids"], ref["medoid_indices"])
    np.testing.assert_array_equal(res["z_medoid"].numpy(), ref["z_medoid"])


def test_bench_prints_one_contract_line(tmp_path):
    """bench.py --full on the small c1 workload (the reference's CPU-runnable configuration), CPU baseline included: ONE JSON
    line on stdout with the driver's fields, the roofline object of the sweep kernel and the cpu_baseline object; with
    --dump-outputs, the last timed build's arrays as float .npy files that agree with the line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GEO_BENCH_CPU_SAMPLE="1")
    dump = tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "c1", "--steps", "2", "--warmup", "1",
                          "--dump-outputs", str(dump), "--full"],
                         capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "latents/s" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert d["config"]["workload"].startswith("c1:") and "model" not in d["config"]
    assert abs(d["value"] - 2048 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and "traffic" in r and r["kernel"]
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]
    assert d["parity_selfcheck"]["batched_assign_equals_fused"] is True
    got = {f[:-4]: np.load(dump / f) for f in os.listdir(dump) if f.endswith(".npy")}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(os.path.getsize(dump / f) for f in os.listdir(dump)) <= 64 * 10 ** 6
    assert float(got["qe"]) == d["parity_selfcheck"]["qe"] and got["medoids"].shape == (64,)
    assert len(got["edge_lengths"]) == d["config"]["graph"]["edges_reweighted"] and got["edge_lengths"].dtype == np.float32
    np.testing.assert_array_equal(got["assign_batched"], got["assign_flat"][got["mask_lcc"] > 0])
    assert np.all(np.isfinite(got["dmin_batched"])) and got["dmin_batched"][got["medoids"].astype(np.int64)].max() == 0


def test_bench_plain_run_prints_the_headline_and_dumps_what_a_full_run_dumps(tmp_path):
    """bench.py without --full: the same ONE line with the headline fields and the timed builds' self-check, none of what
    --full measures after the timed steps (instrumented build, rooflines, CPU baseline), and with --dump-outputs exactly the
    arrays a --full run of the same arguments writes."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = {}
    for mode in ("plain", "full"):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "c1", "--steps", "3", "--warmup", "1",
                              "--dump-outputs", str(tmp_path / mode)] + (["--full", "--no-cpu-baseline"] if mode == "full" else []),
                             capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, out.stderr[-2000:]
        js = [ln for ln in out.stdout.splitlines() if ln.strip()]
        assert len(js) == 1, out.stdout[-2000:]
        lines[mode] = json.loads(js[0])
    plain, full = lines["plain"], lines["full"]
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "parity_selfcheck"):
        assert key in plain, key
    for key in ("roofline", "roofline_knn", "roofline_jvp", "stages_ms", "latency_ms_single_build", "serial_fraction", "cpu_baseline"):
        assert key not in plain, key
    assert "roofline" in full and "stages_ms" in full and "cpu_baseline" not in full
    assert "one_solve_assignment" not in plain["parity_selfcheck"] and full["parity_selfcheck"]["one_solve_assignment"]
    for key in ("metric", "unit", "n_gpus", "steps", "warmup", "higher_is_better", "scaling", "dtype", "data"):
        assert plain[key] == full[key], key
    assert plain["config"]["graph"] == full["config"]["graph"]
    assert plain["config"]["pipeline_depth"] == full["config"]["pipeline_depth"]
    assert abs(plain["value"] - 2048 / (plain["ms_per_step"] * 1e-3)) < 1e-6 * plain["value"]
    assert plain["parity_selfcheck"]["batched_assign_equals_fused"] is True
    assert plain["parity_selfcheck"]["qe"] == full["parity_selfcheck"]["qe"]
    names = sorted(f for f in os.listdir(tmp_path / "plain") if f.endswith(".npy"))
    assert names and names == sorted(f for f in os.listdir(tmp_path / "full") if f.endswith(".npy"))
    for f in names:
        np.testing.assert_array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f), err_msg=f)
    assert float(np.load(tmp_path / "plain" / "qe.npy")) == plain["parity_selfcheck"]["qe"]


def test_bench_two_ranks_with_sharded_builds_in_flight():
    """`bench.py --gpus 2` on the one-GPU box (two rank processes over gloo sharing the card; RCCL when the box has a GPU per
    rank): every build sharded over the ranks AND three builds in flight per rank, their collectives issued in ticket order
    on the one communicator (parallel.CollectiveOrder).  The run must end (no rank parked behind a ticket), every build must
    return the same QE as the one-rank run, and the line must say what it did."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = {}
    for gpus in (1, 2):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "c1", "--gpus", str(gpus), "--steps", "7",
                              "--warmup", "1", "--pipeline", "3", "--no-cpu-baseline"],
                             capture_output=True, text=True, timeout=900, cwd=root,
                             env=dict(os.environ, **({"GEO_BENCH_BACKEND": "gloo"} if torch.cuda.device_count() < gpus else {})))
        assert out.returncode == 0, out.stderr[-3000:]
        js = [ln for ln in out.stdout.splitlines() if ln.strip().startswith("{")]
        assert len(js) == 1, out.stdout[-2000:]
        lines[gpus] = json.loads(js[0])
    one, two = lines[1], lines[2]
    # the line reports the faster of its two timed regions (one build after the other / three in flight): which one wins on two
    # ranks sharing one card is a matter of timing, what was tried and what is reported must be said either way
    tried = two["config"]["regions_timed"]
    assert two["n_gpus"] == 2 and two["scaling"] == "strong" and tried["builds_in_flight_tried"] == 3
    assert two["config"]["pipeline_depth"] in (1, 3)
    assert tried["reported"] == ("in flight" if two["config"]["pipeline_depth"] == 3 else "one after the other")
    if two["config"]["pipeline_depth"] == 3:
        assert "ticket order" in two["config"]["parallelism"]
    else:
        assert "not faster" in tried["note"]                      # (it ran to the end and agreed: the QE check below covers both regions)
    assert "kNN query rows" in two["config"]["parallelism"]
    assert two["parity_selfcheck"]["batched_assign_equals_fused"] is True
    assert two["parity_selfcheck"]["qe"] == one["parity_selfcheck"]["qe"]
    assert two["config"]["graph"] == one["config"]["graph"]


def test_pipelined_builds_equal_builds_one_after_the_other():
    """vqvae_amd/pipeline.py: several independent builds in flight on one GPU (one host thread + HIP stream + workspace per
    slot) return exactly what the same builds return one after the other -- graph, edge lengths, medoids, codes, QE -- for
    latent sets of different sizes (so the slots drift apart) and more sets than slots."""
    from oracle import metric as om
    from oracle import synthetic as syn
    from vqvae_amd._device import device
    from vqvae_amd.scripts.build_codebook import build_codebook_device, build_codebooks_pipelined
    from vqvae_amd.spatial_decoder import SpatialDecoder
    dev = device()
    sd = om.make_decoder_state(4, 16, 1, norm_type="batch")
    dec = SpatialDecoder(1, (256, 128, 64), 16, 28, "batch")
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    dec = dec.to(dev).train()
    sizes = [6000, 2500, 9000, 4096, 7000, 3000, 5000]
    sets = [torch.from_numpy(syn.gauss_latents(n, 16, 100 + i)).to(dev) for i, n in enumerate(sizes)]
    kw = dict(k=12, sym="union", K=48, init="kpp", seed=42, batch_size=512)
    import copy
    ref = [build_codebook_device(z, copy.deepcopy(dec), **kw) for z in sets]
    got = build_codebooks_pipelined(sets, dec, depth=3, **kw)
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a["W_lcc"].indices.cpu().numpy(), b["W_lcc"].indices.cpu().numpy())
        np.testing.assert_array_equal(a["edge_lengths"].cpu().numpy(), b["edge_lengths"].cpu().numpy())
        np.testing.assert_array_equal(a["medoids"], b["medoids"])
        np.testing.assert_array_equal(a["assign_flat"], b["assign_flat"])
        assert a["qe"] == b["qe"]


def test_repeated_pipelined_calls_reuse_their_streams_and_workspaces():
    """Advisor (round 3): the workspace cache is keyed by stream handle, so every pipelined call must run on the SAME slot
    streams (`_device.slot_streams`), not on fresh ones: the number of cached scratch buffers stays put from the second call on."""
    from oracle import metric as om
    from oracle import synthetic as syn
    from vqvae_amd import _device
    from vqvae_amd._device import device
    from vqvae_amd.scripts.build_codebook import build_codebooks_pipelined
    from vqvae_amd.spatial_decoder import SpatialDecoder
    dev = device()
    sd = om.make_decoder_state(4, 16, 1, norm_type="batch")
    dec = SpatialDecoder(1, (256, 128, 64), 16, 28, "batch")
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    dec = dec.to(dev).train()
    sets = [torch.from_numpy(syn.gauss_latents(3000 + 500 * i, 16, 200 + i)).to(dev) for i in range(4)]
    kw = dict(k=12, sym="union", K=24, init="kpp", seed=42, batch_size=512)
    first = build_codebooks_pipelined(sets, dec, depth=3, **kw)
    n_buffers = _device.workspace_buffers()
    streams = [s.cuda_stream for s in _device.slot_streams(dev, 3)]
    for _ in range(3):
        again = build_codebooks_pipelined(sets, dec, depth=3, **kw)
        assert _device.workspace_buffers() == n_buffers
        assert [s.cuda_stream for s in _device.slot_streams(dev, 3)] == streams
        assert [a["qe"] for a in again] == [a["qe"] for a in first]
