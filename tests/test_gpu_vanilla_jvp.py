"""The native pull-back metric of the eval-mode vanilla VAE decoder (csrc/vanilla_jvp.hip) on the GPU: accuracy against fp64
autograd, that the route really is native, swap symmetry, the graph entry against the pairs entry, independence of the pass
size and of batch_size, determinism, and the legacy builder end to end."""
import copy

import numpy as np
import pytest
import torch

import vanilla_jvp_cases as V

pytestmark = pytest.mark.gpu


def _native(dec, zs, ze, **kw):
    from vqvae_amd.geo.riemannian_metric import edge_lengths_vanilla_device
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    dev = torch.device("cuda", 0)
    ex = VanillaDecoderExport(dec, dev)
    return edge_lengths_vanilla_device(ex, zs.to(dev).contiguous(), ze.to(dev).contiguous(), **kw)


def _forbid_autograd(monkeypatch):
    from vqvae_amd.geo import riemannian_metric

    def boom(*a, **k):
        raise AssertionError("autograd route taken")
    monkeypatch.setattr(riemannian_metric, "_generic_jvp_norms", boom)


@pytest.mark.parametrize("name", list(V.CASES))
def test_accuracy_against_fp64_and_the_route_is_native(name, monkeypatch):
    """The three criteria of vanilla_jvp_cases.check_against_fp64 for the kernels AND for float32 autograd on the CPU on the
    same inputs (which ties the inputs to the 0.5 % cap); with the autograd route made to raise, the public entry still
    returns, on the decoder's device, whatever batch_size is."""
    from vqvae_amd.geo.riemannian_metric import edge_lengths_riemannian
    dec, zs, ze, want64, auto32 = V.case(name)
    V.check_against_fp64(auto32, want64, f"{name}: float32 autograd (CPU)")
    _forbid_autograd(monkeypatch)
    got = edge_lengths_riemannian(dec, zs, ze, batch_size=512)                     # CPU decoder: result back on the CPU
    assert got.device.type == "cpu" and got.dtype == torch.float32 and got.shape == (V.N_EDGES,)
    V.check_against_fp64(got.numpy(), want64, f"{name}: native")
    on_gpu = edge_lengths_riemannian(copy.deepcopy(dec).cuda(), zs, ze, batch_size=37)
    assert on_gpu.is_cuda and np.array_equal(on_gpu.cpu().numpy(), got.numpy())    # batch_size does not enter


@pytest.mark.parametrize("norm,eval_mode", [("group", True), ("batch", False)])
def test_uncovered_vanilla_decoders_keep_the_autograd_route(norm, eval_mode, monkeypatch):
    from vqvae_amd.geo.riemannian_metric import edge_lengths_riemannian
    dec = V.make_decoder((128, 64, 32), 16, 1, 28, norm, eval_mode=eval_mode).cuda()
    zs, ze = V.make_edges(16, n_edges=40)
    assert edge_lengths_riemannian(dec, zs, ze, batch_size=16).shape == (40,)
    _forbid_autograd(monkeypatch)
    with pytest.raises(AssertionError, match="autograd route taken"):
        edge_lengths_riemannian(dec, zs, ze, batch_size=16)


@pytest.mark.parametrize("name", ["wide-bn-32x3", "narrow-none-28"])
def test_swap_passes_batch_size_determinism(name):
    """Bit for bit: endpoints swapped; the workspace at its documented minimum (one edge per pass, 2085 passes) and at a size
    in between; two runs; a run on a side stream."""
    from vqvae_amd import _lib
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    dec, zs, ze, _, _ = V.case(name)
    base = _native(dec, zs, ze).cpu().numpy()
    assert np.all(np.isfinite(base)) and np.all(base > 0)
    assert np.array_equal(_native(dec, ze, zs).cpu().numpy(), base)
    assert np.array_equal(_native(dec, zs, ze).cpu().numpy(), base)
    lib = _lib.load()
    ex = VanillaDecoderExport(dec, torch.device("cuda", 0))
    least = lib.geo_vanilla_jvp_workspace_bytes(ex.desc, 1)
    assert np.array_equal(_native(dec, zs, ze, max_workspace_bytes=least).cpu().numpy(), base)
    assert np.array_equal(_native(dec, zs, ze, max_workspace_bytes=lib.geo_vanilla_jvp_workspace_bytes(ex.desc, 333)).cpu().numpy(), base)
    with pytest.raises(_lib.GeoHipError):
        _native(dec, zs, ze, max_workspace_bytes=least - 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _native(dec, zs, ze)
    side.synchronize()
    assert np.array_equal(other.cpu().numpy(), base)


@pytest.mark.parametrize("name", ["wide-bn-28", "narrow-none-32x3-d5"])
def test_graph_entry_equals_pairs_entry(name):
    """300 latents, 1500 random (src, dst) pairs with self loops: the graph entry (per-point work once per latent; with the
    minimal workspace once per edge end) is bit for bit the pairs entry on the gathered endpoints; self loops are exactly 0."""
    from vqvae_amd import _lib
    from vqvae_amd.geo.riemannian_metric import edge_lengths_vanilla_device, edge_lengths_vanilla_graph_device
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    dev = torch.device("cuda", 0)
    dec = V.case(name)[0]
    ex = VanillaDecoderExport(dec, dev)
    z, src, dst = (t.to(dev) for t in V.small_graph(ex.latent_dim))
    pairs = edge_lengths_vanilla_device(ex, z[src.long()].contiguous(), z[dst.long()].contiguous()).cpu().numpy()
    graph = edge_lengths_vanilla_graph_device(ex, z, src, dst).cpu().numpy()
    assert np.array_equal(graph, pairs)
    loops = (src == dst).cpu().numpy()
    assert loops.sum() >= 30 and np.all(pairs[loops] == 0.0) and np.all(pairs[~loops] > 0)
    least = _lib.load().geo_vanilla_jvp_workspace_bytes(ex.desc, 1)
    assert np.array_equal(edge_lengths_vanilla_graph_device(ex, z, src, dst, max_workspace_bytes=least).cpu().numpy(), pairs)
    few = edge_lengths_vanilla_graph_device(ex, z, src[:100], dst[:100]).cpu().numpy()          # fewer edges than latents / 2
    assert np.array_equal(few, pairs[:100])
    with pytest.raises(ValueError):
        edge_lengths_vanilla_graph_device(ex, z, src, dst.clamp(min=300))


@pytest.mark.parametrize("name", ["wide-bn-28", "narrow-none-32x3-d5"])
def test_graph_entry_in_slices_equals_the_whole_call(name):
    """geo_vanilla_jvp_edges works per latent when n_nodes <= 2 n_edges and per edge end otherwise, and promises the same bits
    either way.  The 1500 edges of test_graph_entry_equals_pairs_entry over its 300 latents, whole (per latent) and in 15
    slices of 100 through the edges entry (300 > 200: per edge end, every slice with the workspace its own query sizes):
    the slices put together are the whole call and the pairs entry, bit for bit."""
    from vqvae_amd.geo.riemannian_metric import edge_lengths_vanilla_device, edge_lengths_vanilla_graph_device
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    dev = torch.device("cuda", 0)
    ex = VanillaDecoderExport(V.case(name)[0], dev)
    z, src, dst = (t.to(dev) for t in V.small_graph(ex.latent_dim))
    n_nodes, n_edges, step = z.shape[0], src.numel(), 100
    assert n_nodes <= 2 * n_edges and n_nodes > 2 * step and n_edges % step == 0
    whole = edge_lengths_vanilla_graph_device(ex, z, src, dst).cpu().numpy()
    pairs = edge_lengths_vanilla_device(ex, z[src.long()].contiguous(), z[dst.long()].contiguous()).cpu().numpy()
    sliced = torch.cat([edge_lengths_vanilla_graph_device(ex, z, src[e0:e0 + step].contiguous(), dst[e0:e0 + step].contiguous())
                        for e0 in range(0, n_edges, step)]).cpu().numpy()
    assert sliced.shape == whole.shape and np.all(np.isfinite(sliced))
    np.testing.assert_array_equal(sliced, whole)
    np.testing.assert_array_equal(sliced, pairs)


@pytest.mark.parametrize("mode", ["full", "subset"])
def test_legacy_builder_re_weighting_native_against_autograd(mode, monkeypatch):
    """reweight_graph_device on 600 x 16 latents with an eval-BatchNorm decoder: same structure as with the predicate forced
    to False (the autograd route), weights within the accuracy criteria of that run.  The output layer is scaled up so that
    the pull-back lengths exceed the Euclidean weights: the contract keeps the larger of an entry's two directions, and in
    subset mode a shorter length would be hidden behind the partner entry's Euclidean weight."""
    from vqvae_amd.geo.knn_graph_optimized import knn_graph_device
    from vqvae_amd.training import build_riemannian_codebook_legacy as B
    dev = torch.device("cuda", 0)
    dec = V.make_decoder((128, 64, 32), 16, 1, 28, "batch", seed=2).to(dev)
    with torch.no_grad():
        dec.output_layer.weight.mul_(20.0)
    z = torch.randn(600, 16, generator=torch.Generator().manual_seed(8)).to(dev)
    G, _, _ = knn_graph_device(z, 10, mode="distance", sym="union", metric="euclidean")
    np.random.seed(123)
    native = B.reweight_graph_device(G, z, dec, mode, max_edges=1000, batch_size=256)
    monkeypatch.setattr(B, "vanilla_kernels_cover", lambda m: False)
    monkeypatch.setattr("vqvae_amd.geo.riemannian_metric.vanilla_kernels_cover", lambda m: False)
    np.random.seed(123)
    auto = B.reweight_graph_device(G, z, dec, mode, max_edges=1000, batch_size=256)
    assert torch.equal(native.indptr, auto.indptr) and torch.equal(native.indices, auto.indices)
    a, b = native.data.cpu().numpy(), auto.data.cpu().numpy()
    changed = b != G.data.cpu().numpy()
    assert np.array_equal(a != G.data.cpu().numpy(), changed) and changed.sum() >= (G.nnz if mode == "full" else 900)
    assert np.array_equal(a[~changed], b[~changed])
    V.check_against_fp64(a[changed], b[changed], f"builder {mode}: native against the autograd route")
    sym = native.to_scipy()
    assert (sym != sym.T).nnz == 0
