"""Host-side checks of the Riemannian graph experiments (no GPU): the seeded selection rules against the golden run of the
reference's scripts, vqvae_amd.utils.checkpoint_utils on the golden checkpoint in its three layouts, the CLI defaults and the
dataset path pairs (tests/golden/riemann_experiments*.npz, tools/gen_golden_riemann_experiments.py)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g(golden):
    return golden("riemann_experiments")


@pytest.fixture(scope="module")
def state_dict(golden):
    f = golden("riemann_experiments_vae")
    return {k[len("sd/"):]: torch.from_numpy(f[k]) for k in f.files if k.startswith("sd/")}, json.loads(str(f["config_json"]))


def golden_graph(g):
    n = len(g["indptr"]) - 1
    return sparse.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=(n, n))


def test_source_pick_and_stratified_sample_reproduce_the_golden_run(g, monkeypatch):
    from scipy.sparse.csgraph import connected_components
    from vqvae_amd.geo import experiments
    W = golden_graph(g)

    def lcc_on_the_host(M):                                # the device routine's rule (first largest label), by scipy
        _, labels = connected_components(M, directed=False)
        return labels == np.argmax(np.bincount(labels))

    monkeypatch.setattr(experiments, "largest_connected_component", lcc_on_the_host)
    rng = np.random.RandomState(0)
    src = experiments.pick_sources_from_lcc(W, 8, rng)
    assert np.array_equal(src, g["sources"])
    rows, cols = W.nonzero()
    upper = rows < cols
    selected = experiments.stratified_edge_sample(W.data[upper], 5000, 5, rng)        # the STORED distances, not recomputed norms
    assert np.array_equal(rows[upper][selected], g["i_sel"]) and np.array_equal(cols[upper][selected], g["j_sel"])
    assert len(selected) == int(g["effects/sample_edges"]) == 5000


def test_stratified_sample_rule():
    from vqvae_amd.geo.experiments import stratified_edge_sample
    lengths = np.arange(100, dtype=np.float32)
    sel = stratified_edge_sample(lengths, 20, 4, np.random.RandomState(3))
    assert len(sel) == 20 and len(set(sel.tolist())) == 20
    assert [int(((sel >= lo) & (sel < lo + 25)).sum()) for lo in (0, 25, 50, 75)] == [5, 5, 5, 5]    # bins in order, 5 each
    assert all(((sel[5 * b:5 * b + 5] // 25) == b).all() for b in range(4))
    assert len(stratified_edge_sample(lengths[:3], 20, 4, np.random.RandomState(3))) == 3            # a bin gives what it has
    assert len(stratified_edge_sample(lengths, 2, 4, np.random.RandomState(3))) == 4                 # at least one per bin


@pytest.mark.parametrize("layout", ("model_state_dict", "model", "bare"))
def test_checkpoint_utils_load_every_layout(state_dict, layout, tmp_path, capsys):
    from vqvae_amd.utils import checkpoint_utils as cu
    sd, config = state_dict
    path = tmp_path / "best.pt"
    torch.save(sd if layout == "bare" else {layout: sd, "epoch": 3}, path)
    model, cfg = cu.load_vae_from_checkpoint(str(path), latent_dim=None, device="cpu", verbose=True)
    out = capsys.readouterr().out
    assert "Auto-detected: 1ch, (32, 64, 128), 28x28, batch, latent_dim=8" in out and "VAE loaded successfully" in out
    assert model is not None and not model.training
    assert {k: list(v) if isinstance(v, tuple) else v for k, v in cfg.items()} == config
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    dec = cu.get_vae_decoder(str(path), latent_dim=8, device="cpu")
    assert dec is not None and not dec.training and not dec.deconv1[1].training
    assert torch.equal(dec.fc.weight, sd["decoder.fc.weight"])
    assert cu.load_decoder(str(path), 8).fc.in_features == 8
    assert cu.extract_state_dict(torch.load(path, weights_only=False)).keys() == sd.keys()
    assert cu.auto_detect_vae_config_legacy(sd) == cu.auto_detect_vae_config(sd) == cfg


def test_checkpoint_utils_forgive(tmp_path, capsys):
    from vqvae_amd.utils import checkpoint_utils as cu
    missing = str(tmp_path / "nope.pt")
    assert cu.load_vae_from_checkpoint(missing) == (None, {})
    assert "Checkpoint not found" in capsys.readouterr().out
    assert cu.load_vae_from_checkpoint(missing, verbose=False) == (None, {}) and capsys.readouterr().out == ""
    assert cu.get_vae_decoder(missing) is None and cu.load_decoder(missing, 8) is None
    broken = tmp_path / "broken.pt"
    torch.save({"model_state_dict": {"decoder.fc.weight": torch.zeros(3, 3)}}, broken)
    assert cu.load_vae_from_checkpoint(str(broken)) == (None, {})
    assert "Error loading VAE" in capsys.readouterr().out
    assert cu.get_vae_decoder(str(broken)) is None


def test_cli_defaults_are_the_reference_constants(g):
    from vqvae_amd.scripts import riemann_sanity_check as sanity_cli
    from vqvae_amd.scripts import run_riemann_experiments as effects_cli
    a = effects_cli.parse_args([])
    # run_riemann_experiments.py:79-84: k 10, "subset", 5000 edges, 5 bins, 8 sources, RandomState(0); what it saved agrees
    assert (a.dataset, a.k, a.mode, a.sample_edges, a.num_bins, a.num_sources, a.seed) == ("mnist", 10, "subset", 5000, 5, 8, 0)
    assert a.k == int(g["effects/k"]) and a.mode == str(g["effects/reweight_mode"])
    assert a.num_sources == int(g["effects/num_sources"]) and a.sample_edges == int(g["effects/sample_edges"])
    assert a.latents_path is None and a.checkpoint_path is None and a.out_dir is None
    assert set(effects_cli.SAVED_KEYS) | {"dataset"} == {k[len("effects/"):] for k in g.files if k.startswith("effects/")}
    s = sanity_cli.parse_args([])
    assert (s.dataset, s.latents_path, s.checkpoint_path, s.out_dir) == ("mnist", None, None, None)
    # riemann_sanity_check.py:64-65, :81, :99: k 10, 2000 entries, RandomState(0), batch 256
    assert (sanity_cli.K_NEIGHBORS, sanity_cli.MAX_EDGES, sanity_cli.SEED, sanity_cli.BATCH_SIZE) == (10, 2000, 0, 256)
    assert len(g["sanity/de"]) == sanity_cli.MAX_EDGES
    with pytest.raises(SystemExit):
        effects_cli.parse_args(["--dataset", "svhn"])
    with pytest.raises(SystemExit):
        effects_cli.parse_args(["--mode", "half"])


def test_dataset_paths_are_the_recorded_ones(g):
    from vqvae_amd.scripts import riemann_sanity_check as sanity_cli
    from vqvae_amd.scripts import run_riemann_experiments as effects_cli
    recorded = {str(n): {"latents_path": str(l), "checkpoint_path": str(c)}
                for n, l, c in zip(g["dataset_names"], g["latents_paths"], g["checkpoint_paths"])}
    assert len(recorded) == 3 and sanity_cli.DATASET_CONFIGS == recorded and effects_cli.DATASET_CONFIGS == recorded
    args = effects_cli.parse_args(["--dataset", "cifar10"])
    lat, ckpt, out = effects_cli.resolve_paths(args, "riemann_graph_effects")
    assert (lat, ckpt) == (recorded["cifar10"]["latents_path"], recorded["cifar10"]["checkpoint_path"])
    assert out.as_posix() == "experiments/geo/riemann_graph_effects/cifar10"
    args = sanity_cli.parse_args(["--latents_path", "a.pt", "--checkpoint_path", "b.pt", "--out_dir", "o"])
    assert tuple(map(str, sanity_cli.resolve_paths(args, "riemann_sanity"))) == ("a.pt", "b.pt", "o")


def test_cli_without_decoder_exits_quietly(tmp_path, capsys, monkeypatch):
    from vqvae_amd.scripts import run_riemann_experiments as effects_cli
    from vqvae_amd import _device
    monkeypatch.setattr(_device, "device", lambda: torch.device("cpu"))
    monkeypatch.chdir(tmp_path)
    torch.save(torch.zeros(4, 8), tmp_path / "z.pt")
    assert effects_cli.main(["--latents_path", "z.pt", "--checkpoint_path", "none.pt", "--out_dir", "out"]) is None
    assert "Cannot load decoder. Exiting." in capsys.readouterr().out


def test_new_symbols_are_declared_bound_and_exported():
    from vqvae_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "geo_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("geo_path_stats", "geo_csr_set_symmetric"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS, name
        assert re.search(r" T %s\b" % name, out), name
    assert _lib.load().geo_version() >= 106
    import vqvae_amd.geo as geo
    for name in ("mean_shortest_path", "mean_shortest_path_device", "pick_sources_from_lcc", "stratified_edge_sample",
                 "reweight_edges_symmetric_device", "riemann_sanity", "riemann_graph_effects"):
        assert name in geo.__all__ and callable(getattr(geo, name))
