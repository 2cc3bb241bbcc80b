"""Pull-back lengths of decoders with fixed statistics (eval-mode BatchNorm, no norm, GroupNorm) must not depend on how the edges
of a graph are divided among calls: the per-latent Jacobian route (csrc/jvp.hip, make_route) is chosen from the edges per latent,
it differs from the per-edge-end path in its last bits, and a rank of a sharded build sees only its share of the edges.  Told the
edge count of the whole build (`build_edges`, geo_decoder_jvp_edges_part) every part takes the route the whole graph takes.

One process; graphs of a few chunks at sizes where the whole has at least 0.75 d edges per latent and no proper part has."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5      # test_gpu_metric.py's gate: >= 99.9 % of a vector's edges within 1e-5 (relative) of the fp64 closed form

# name: (norm, d, out_channels, out_size, n_nodes, n_edges, batch_size)
CASES = {
    "bn_eval-96x1536": ("batch", 16, 1, 28, 96, 1536, 512),         # 3 chunks, 16 edges per latent; a proper part has <= 1024 (< 12)
    "none-96x1536": ("none", 16, 1, 28, 96, 1536, 512),
    "group-96x1536": ("group", 16, 1, 28, 96, 1536, 512),
    "bn_eval-97x1700-bs100": ("batch", 16, 1, 28, 97, 1700, 100),   # odd latent count (the last is its own partner), ragged last chunk
    "none-d5-200x1000-bs64": ("none", 5, 1, 28, 200, 1000, 64),     # narrow latent: 3.75 edges per latent; a chunk has fewer slots than latents
    "bn_eval-3ch32-96x1536": ("batch", 16, 3, 32, 96, 1536, 512),   # 192-output head
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Decoder export, latents and edges on the GPU, the edges on the host and their fp64 closed-form lengths: made once, read-only."""
    from oracle import metric as om
    from vqvae_amd._device import device
    from vqvae_amd.spatial_decoder import DecoderExport, SpatialDecoder
    norm, d, cout, size, n_nodes, n_edges, bs = CASES[name]
    dev = device()
    sd = om.make_decoder_state(17, d, cout, norm_type=norm)
    dec = SpatialDecoder(cout, (256, 128, 64), d, size, norm)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    dec = dec.to(dev).eval()
    r = np.random.RandomState(n_edges + n_nodes)
    z_h = r.randn(n_nodes, d).astype(np.float32)
    src_h = r.randint(0, n_nodes, n_edges).astype(np.int32)
    dst_h = (src_h + 1 + r.randint(0, n_nodes - 1, n_edges)).astype(np.int32) % n_nodes
    src_h[:3], dst_h[:3] = n_nodes - 1, [0, 1, n_nodes - 2]     # the last latent is on edges, on both sides
    dst_h[3], src_h[3] = n_nodes - 1, 0
    assert np.all(src_h != dst_h)
    ref64 = om.edge_lengths(sd, norm, size, z_h[src_h], z_h[dst_h], bs, False, dtype=torch.float64).numpy()
    ref64.setflags(write=False)
    z, src, dst = (torch.from_numpy(a).to(dev) for a in (z_h, src_h, dst_h))
    return DecoderExport(dec, dev), z, src, dst, ref64


@pytest.fixture()
def default_options(request):
    from vqvae_amd import _lib
    lib = _lib.load()

    def restore():
        lib.geo_set_option(b"jvp_per_node", 1)
        lib.geo_set_option(b"jvp_node_jacobian", 1)
    request.addfinalizer(restore)
    restore()
    return lib


def _jacobian(lib, ex, n_nodes, n_edges, build_edges, bs):
    """Does this call take the per-latent Jacobian route?  (geo_jvp_plan_part: the decision the call makes, host arithmetic)"""
    from vqvae_amd import _lib
    code = lib.geo_jvp_plan_part(ex.desc, n_nodes, n_edges, build_edges, bs, 1, 0)
    assert code >= 0, lib.geo_last_error()
    return _lib.decode_jvp_plan(code)["node_jacobian"]


def _lengths(ex, z, src, dst, e0, e1, bs, build_edges=None):
    from vqvae_amd.geo.riemannian_metric import edge_lengths_graph_device
    return edge_lengths_graph_device(ex, z, src[e0:e1], dst[e0:e1], bs, build_edges=build_edges).cpu().numpy()


def _gate(got, ref64, what):
    rel = np.abs(got - ref64) / np.abs(ref64)
    print(f"{what}: {len(got)} edges, {np.mean(rel <= TOL):.4%} within {TOL}, max {rel.max():.2e}, median {np.median(rel):.2e}")
    assert got.shape == ref64.shape and np.all(np.isfinite(got))
    assert np.mean(rel <= TOL) >= 0.999, (what, rel.max(), int((rel > TOL).sum()))


def _cuts(n_edges, bs):
    """The edge ranges of 2, 3 and 5 ranks, and every chunk on its own."""
    from vqvae_amd import parallel
    cuts = {f"{w} ranks": [parallel.chunk_range(n_edges, bs, r, w) for r in range(w)] for w in (2, 3, 5)}
    cuts["single chunks"] = [(e0, min(e0 + bs, n_edges)) for e0 in range(0, n_edges, bs)]
    for parts in cuts.values():
        assert parts[0][0] == 0 and parts[-1][1] == n_edges and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
    return {k: [(e0, e1) for e0, e1 in parts if e1 > e0] for k, parts in cuts.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_parts_told_the_build_s_edge_count_equal_the_whole_call(name, default_options):
    lib = default_options
    n_nodes, n_edges, bs = CASES[name][4:]
    d = CASES[name][1]
    ex, z, src, dst, ref64 = _case(name)
    assert 4 * n_edges >= 3 * n_nodes * d
    # (a) the whole call: the Jacobian route, by the rule itself
    assert _jacobian(lib, ex, n_nodes, n_edges, n_edges, bs)
    whole = _lengths(ex, z, src, dst, 0, n_edges, bs)
    _gate(whole, ref64, f"{name}: whole")
    np.testing.assert_array_equal(_lengths(ex, z, src, dst, 0, n_edges, bs, build_edges=n_edges), whole)
    # (b) parts with build_edges: the same route, the same bits
    for how, parts in _cuts(n_edges, bs).items():
        assert len(parts) >= 2
        got = []
        for e0, e1 in parts:
            assert not _jacobian(lib, ex, n_nodes, e1 - e0, e1 - e0, bs), (how, e0, e1)     # on its own it would not
            assert _jacobian(lib, ex, n_nodes, e1 - e0, n_edges, bs), (how, e0, e1)
            got.append(_lengths(ex, z, src, dst, e0, e1, bs, build_edges=n_edges))
        got = np.concatenate(got)
        np.testing.assert_array_equal(got, whole, err_msg=f"{name}, {how}")
        _gate(got, ref64, f"{name}: {how}")
    # (c) the tripwire: the same parts without build_edges take the per-edge-end path, whose last bits differ
    for e0, e1 in _cuts(n_edges, bs)["2 ranks"]:
        alone = _lengths(ex, z, src, dst, e0, e1, bs)
        assert alone.shape == (e1 - e0,) and not np.array_equal(alone, whole[e0:e1]), (e0, e1)
        _gate(alone, ref64[e0:e1], f"{name}: edges [{e0}, {e1}) on their own")
    with pytest.raises(ValueError):
        _lengths(ex, z, src, dst, 0, bs, bs, build_edges=bs - 1)


@pytest.mark.parametrize("name", list(CASES))
def test_below_the_threshold_whole_and_parts_keep_the_per_edge_end_path(name, default_options):
    """(d) One edge fewer than 0.75 d per latent: no call takes the Jacobian route, with or without build_edges, and the per-node
    primal path is independent of the other edges of a call by itself."""
    lib = default_options
    d, n_nodes, bs = CASES[name][1], CASES[name][4], CASES[name][6]
    ex, z, src, dst, ref64 = _case(name)
    n_edges = (3 * n_nodes * d + 3) // 4 - 1
    assert 4 * n_edges < 3 * n_nodes * d <= 4 * (n_edges + 1) and n_edges > 2 * bs
    assert not _jacobian(lib, ex, n_nodes, n_edges, n_edges, bs)
    whole = _lengths(ex, z, src, dst, 0, n_edges, bs)
    _gate(whole, ref64[:n_edges], f"{name}: whole, {n_edges} edges")
    for how, parts in _cuts(n_edges, bs).items():
        for build in (n_edges, None):
            for e0, e1 in parts:
                assert not _jacobian(lib, ex, n_nodes, e1 - e0, build or e1 - e0, bs)
            got = np.concatenate([_lengths(ex, z, src, dst, e0, e1, bs, build_edges=build) for e0, e1 in parts])
            np.testing.assert_array_equal(got, whole, err_msg=f"{name}, {how}, build_edges={build}")
