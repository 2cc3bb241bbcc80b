"""GPU checks of the Riemannian graph experiments against the golden run of the reference's two scripts
(tests/golden/riemann_experiments*.npz, tools/gen_golden_riemann_experiments.py): the graph, the seeded picks, the path
statistics stage by stage and end to end, the sanity check, block invariance, both CLIs and mode="full".

eps_len is the largest relative deviation of this run's lengths from the golden reference lengths on the selected edges.
The end-to-end bound on mean_sp_riem and ratio_sp, max(eps_len, 2^-23) + 2^-24, is derived, not measured: if every weight
moves by a factor in 1 +- eps, every path sum does, hence every minimum over paths and every mean of such minima
(DESIGN.md section 16); 2^-23 is the 1 ulp the stored Euclidean weights may differ by, 2^-24 the float32 rounding of the
distances."""
import numpy as np
import pytest
import torch
from scipy import sparse

pytestmark = pytest.mark.gpu

EFFECT_KEYS = {"ncomp_euc", "lcc_size_euc", "mean_sp_euc", "ncomp_riem", "lcc_size_riem", "mean_sp_riem", "ratio_sp",
               "reweight_mode", "sample_edges", "k", "num_sources", "dataset"}
SANITY_KEYS = {"corr", "ratio", "de", "dr", "dataset", "decoder_type"}


@pytest.fixture(scope="module")
def g(golden):
    return golden("riemann_experiments")


@pytest.fixture(scope="module")
def state(golden):
    f = golden("riemann_experiments_vae")
    return {k[len("sd/"):]: torch.from_numpy(f[k]) for k in f.files if k.startswith("sd/")}


@pytest.fixture(scope="module")
def decoder(state):
    from vqvae_amd.vae import VAE
    model = VAE(in_channels=1, enc_channels=(32, 64, 128), dec_channels=(128, 64, 32), latent_dim=8, norm_type="batch",
                output_image_size=28)
    model.load_state_dict(state)
    return model.eval().decoder.to(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def effects(g, decoder):
    from vqvae_amd.geo.experiments import riemann_graph_effects
    return riemann_graph_effects(g["z"], decoder)


@pytest.fixture(scope="module")
def sanity(g, decoder):
    from vqvae_amd.geo.experiments import riemann_sanity
    return riemann_sanity(g["z"], decoder)


@pytest.fixture(scope="module")
def golden_graph(g):
    from vqvae_amd._device import DeviceCSR
    n = len(g["indptr"]) - 1
    W = sparse.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=(n, n))
    return DeviceCSR.from_scipy(W, torch.device("cuda", 0))


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def section_15_criterion(got, f64, what):
    r = np.abs(got.astype(np.float64) - f64) / f64
    print(f"{what}: {np.mean(r <= 1e-5):.4%} within 1e-5 of fp64 autograd, max rel {r.max():.3e}")
    assert np.mean(r <= 1e-5) >= 0.995 and r.max() < 1e-3, (np.mean(r <= 1e-5), r.max())


def eps_len(effects, g):
    return float(np.max(np.abs(effects["riem_lengths"].astype(np.float64) - g["riem_lengths"]) / g["riem_lengths"]))


def test_graph_is_the_golden_graph(effects, g):
    G = effects["graph_euc"]
    assert np.array_equal(G.indptr.cpu().numpy(), g["indptr"]) and np.array_equal(G.indices.cpu().numpy(), g["indices"])
    assert ulps(G.data.cpu().numpy(), g["data"]).max() <= 1


def test_counts_sources_and_selection_are_exact(effects, g):
    for key in ("ncomp_euc", "lcc_size_euc", "ncomp_riem", "lcc_size_riem", "sample_edges", "k", "num_sources"):
        assert int(effects[key]) == int(g[f"effects/{key}"]), key
    assert effects["reweight_mode"] == str(g["effects/reweight_mode"])
    assert np.array_equal(effects["sources"], g["sources"])
    assert np.array_equal(effects["i_sel"], g["i_sel"]) and np.array_equal(effects["j_sel"], g["j_sel"])
    assert effects["n_zero_lengths"] == 0


def test_path_statistics_stage_wise(golden_graph, g):
    """Golden graph data and golden reference lengths injected: only the solve and the reduction differ from the reference
    (scipy's fp64 distances rounded once to float32: 2^-24; fp64 accumulation of positive terms: N 2^-53) -- within 1e-7."""
    from vqvae_amd.geo.experiments import mean_shortest_path_device, reweight_edges_symmetric_device
    euc = mean_shortest_path_device(golden_graph, g["sources"])
    riem_graph = reweight_edges_symmetric_device(golden_graph, g["i_sel"], g["j_sel"], g["riem_lengths"])
    riem = mean_shortest_path_device(riem_graph, g["sources"])
    print(f"stage-wise: mean_sp_euc rel {rel(euc['mean'], g['effects/mean_sp_euc']):.3e}, "
          f"mean_sp_riem rel {rel(riem['mean'], g['effects/mean_sp_riem']):.3e}")
    assert rel(euc["mean"], g["effects/mean_sp_euc"]) <= 1e-7
    assert rel(riem["mean"], g["effects/mean_sp_riem"]) <= 1e-7
    n, lcc = golden_graph.n, int(g["effects/lcc_size_euc"])
    assert euc["n_unreached"] == riem["n_unreached"] == len(g["sources"]) * (n - lcc)
    assert np.array_equal(euc["count"], np.full(len(g["sources"]), lcc - 1))
    assert euc["max"] > 0 and np.isfinite(euc["max"])


def test_effects_end_to_end(effects, g):
    section_15_criterion(effects["riem_lengths"], g["riem_lengths_f64"], "selected edges")
    eps = eps_len(effects, g)
    bound = max(eps, 2.0 ** -23) + 2.0 ** -24
    print(f"eps_len {eps:.3e}, bound {bound:.3e}: mean_sp_euc rel {rel(effects['mean_sp_euc'], g['effects/mean_sp_euc']):.3e}, "
          f"mean_sp_riem rel {rel(effects['mean_sp_riem'], g['effects/mean_sp_riem']):.3e}, "
          f"ratio_sp rel {rel(effects['ratio_sp'], g['effects/ratio_sp']):.3e}")
    assert rel(effects["mean_sp_riem"], g["effects/mean_sp_riem"]) <= bound
    assert rel(effects["ratio_sp"], g["effects/ratio_sp"]) <= bound
    n = len(g["indptr"]) - 1
    W = sparse.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=(n, n))
    stored = np.asarray(W[g["i_sel"], g["j_sel"]]).ravel().astype(np.float32)
    assert ulps(effects["euc_lengths"], stored).max() <= 1


def test_sanity_check(sanity, effects, g):
    assert np.array_equal(sanity["indices"], g["sanity/indices"])
    assert np.array_equal(sanity["i"], g["sanity/i"]) and np.array_equal(sanity["j"], g["sanity/j"])
    assert ulps(sanity["de"], g["sanity/de"]).max() <= 1
    section_15_criterion(sanity["dr"], g["sanity/dr_f64"], "sanity entries")
    assert sanity["ratio"].dtype == np.float32
    eps = eps_len(effects, g)
    allowed = max(2.0 * abs(float(g["sanity/corr_f32"]) - float(g["sanity/corr_f64"])), 1e-6)
    print(f"sanity: ratio rel {rel(sanity['ratio'], g['sanity/ratio']):.3e} (bound {eps + 2.0 ** -22:.3e}), "
          f"corr {sanity['corr']!r} vs {float(g['sanity/corr'])!r} (allowed {allowed:.3e})")
    assert rel(sanity["ratio"], g["sanity/ratio"]) <= eps + 2.0 ** -22
    assert abs(sanity["corr"] - float(g["sanity/corr"])) <= allowed


def test_block_size_changes_nothing(golden_graph, g):
    from vqvae_amd.geo.experiments import mean_shortest_path_device
    sources = np.concatenate([g["sources"], (g["sources"][:3][::-1] + 1) % golden_graph.n])          # 11 sources: blocks of 3 leave a remainder
    n = golden_graph.n
    one = mean_shortest_path_device(golden_graph, sources, max_block_bytes=4 * n)
    three = mean_shortest_path_device(golden_graph, sources, max_block_bytes=12 * n)
    whole = mean_shortest_path_device(golden_graph, sources, max_block_bytes=1 << 40)
    for other in (three, whole):
        assert other.keys() == one.keys()
        for key, v in one.items():
            if isinstance(v, np.ndarray):
                assert v.tobytes() == other[key].tobytes(), key
            else:
                assert v == other[key], key


def test_mean_shortest_path_reference_api(golden_graph, g):
    from vqvae_amd.geo import mean_shortest_path, pick_sources_from_lcc
    W = golden_graph.to_scipy()
    m = mean_shortest_path(W, g["sources"])
    assert isinstance(m, float) and rel(m, g["effects/mean_sp_euc"]) <= 1e-7
    assert np.array_equal(pick_sources_from_lcc(W, 8, np.random.RandomState(0)), g["sources"])
    lonely = sparse.csr_matrix((np.ones(2, np.float32), ([1, 2], [2, 1])), shape=(3, 3))     # node 0 reaches nothing
    assert mean_shortest_path(lonely, [0]) == float("inf")


def test_both_clis_write_the_reference_files(g, state, tmp_path, monkeypatch, capsys):
    from vqvae_amd.scripts import riemann_sanity_check, run_riemann_experiments
    (tmp_path / "experiments/vae_mnist/checkpoints").mkdir(parents=True)
    (tmp_path / "experiments/vae_mnist/latents_val").mkdir(parents=True)
    torch.save({"model_state_dict": state}, tmp_path / "experiments/vae_mnist/checkpoints/best.pt")
    torch.save({"z": torch.from_numpy(g["z"])}, tmp_path / "experiments/vae_mnist/latents_val/z.pt")
    monkeypatch.chdir(tmp_path)
    riemann_sanity_check.main(["--dataset", "mnist"])
    run_riemann_experiments.main([])
    out = capsys.readouterr().out
    for line in ("Running Riemann sanity check on MNIST dataset", "Loaded 4000 latent vectors of dimension 8",
                 "Sampled 2000 edges from k-NN graph", "Results: correlation=0.995, mean_ratio=0.203",
                 "Running Riemann graph effects analysis on MNIST dataset", "[Euclidean] components=220, LCC size=2510, mean_sp=23.7210",
                 "Re-weighting 5000 edges (stratified sampling)", "[Effect]   mean shortest-path ratio (Riem/Eucl) = 0.382"):
        assert line in out, line
    s_dir, e_dir = tmp_path / "experiments/geo/riemann_sanity/mnist", tmp_path / "experiments/geo/riemann_graph_effects/mnist"
    s, e = np.load(s_dir / "sanity_stats_mnist.npz"), np.load(e_dir / "graph_effects_mnist.npz")
    assert set(s.files) == SANITY_KEYS and set(e.files) == EFFECT_KEYS
    assert str(s["dataset"]) == "mnist" and str(s["decoder_type"]) == "real_VAE_MNIST" and str(e["reweight_mode"]) == "subset"
    assert s["de"].dtype == s["dr"].dtype == np.float32 and len(s["de"]) == 2000
    assert int(e["sample_edges"]) == 5000 and int(e["ncomp_euc"]) == int(g["effects/ncomp_euc"])
    for png in (s_dir / "riemann_analysis_mnist.png", e_dir / "graph_effects_mnist.png"):
        assert png.stat().st_size > 1000 and png.read_bytes()[:4] == b"\x89PNG"
    # --out_dir and the extra flags
    run_riemann_experiments.main(["--out_dir", "elsewhere", "--num_sources", "3", "--sample_edges", "500", "--seed", "1"])
    e2 = np.load(tmp_path / "elsewhere/graph_effects_mnist.npz")
    assert int(e2["num_sources"]) == 3 and int(e2["sample_edges"]) == 500


def test_full_mode_reweights_every_edge(g, decoder):
    from vqvae_amd.geo.experiments import riemann_graph_effects
    from vqvae_amd.geo.riemannian_metric import edge_lengths_vanilla_device
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    z = g["z"][:600]
    res = riemann_graph_effects(z, decoder, mode="full", num_sources=4)
    before, after = res["graph_euc"].to_scipy(), res["graph_riem"].to_scipy()
    assert res["reweight_mode"] == "full" and res["sample_edges"] == before.nnz // 2 == len(res["riem_lengths"])
    assert np.all(before.data != after.data)                                            # every stored entry changes
    T = after.T.tocsr()
    T.sort_indices()
    assert np.array_equal(T.indices, after.indices) and T.data.tobytes() == after.data.tobytes()   # symmetric, bit for bit
    dev = torch.device("cuda", 0)
    zd = torch.from_numpy(z).to(dev)
    i, j = torch.from_numpy(res["i_sel"]).to(dev).long(), torch.from_numpy(res["j_sel"]).to(dev).long()
    want = edge_lengths_vanilla_device(VanillaDecoderExport(decoder, dev), zd[i].contiguous(), zd[j].contiguous())
    assert want.cpu().numpy().tobytes() == res["riem_lengths"].tobytes()
    assert np.array_equal(np.asarray(after[res["i_sel"], res["j_sel"]]).ravel(), res["riem_lengths"])
    assert np.isfinite(res["mean_sp_riem"]) and res["ncomp_riem"] == res["ncomp_euc"]


def test_sanity_cli_prints_the_draw_before_it_needs_the_decoder(g, tmp_path, monkeypatch, capsys):
    """The reference builds the graph and draws the entries before it loads the decoder: without a checkpoint its stdout
    still carries those lines, in that order, and no file is written."""
    from vqvae_amd.scripts import riemann_sanity_check
    monkeypatch.chdir(tmp_path)
    torch.save(torch.from_numpy(g["z"][:500]), tmp_path / "z.pt")
    assert riemann_sanity_check.main(["--latents_path", "z.pt", "--checkpoint_path", "none.pt", "--out_dir", "out"]) is None
    out = capsys.readouterr().out
    order = [out.index(line) for line in ("Loaded 500 latent vectors of dimension 8", "Building k-NN graph with k=10",
                                          "Sampled 2000 edges from k-NN graph", "Cannot load decoder. Exiting.")]
    assert order == sorted(order)
    assert not list((tmp_path / "out").glob("*.npz"))


def test_sanity_above_the_moment_kernels_row_length(g, decoder):
    from vqvae_amd.geo.experiments import riemann_sanity
    res = riemann_sanity(g["z"], decoder, max_edges=20000)
    assert len(res["de"]) == 20000
    want = float(np.corrcoef(res["de"].astype(np.float64), res["dr"].astype(np.float64))[0, 1])
    assert abs(res["corr"] - want) <= 1e-12
