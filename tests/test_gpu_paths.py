"""csrc/paths.hip on the GPU (geo_sssp_paths_count / _fill, geo_polyline_resample) through vqvae_amd.geo, against the numpy
restatement of tests/path_cases.py.  Every comparison is bit for bit; the acceptance property needs no oracle: the fp64
running sum along an extracted path, rounded to float32, is the solver's own distance."""
import numpy as np
import pytest
import torch
from scipy import sparse

import path_cases as pc
from conftest import csr_from_golden, latents, swiss_roll_latents

pytestmark = pytest.mark.gpu

S = pc.SENTINEL


def _dev():
    from vqvae_amd._device import device
    return device()


def _t(x, dtype=torch.int32):
    return torch.as_tensor(np.asarray(x), device=_dev()).to(dtype)


def _host(paths):
    return tuple(x.cpu().numpy() for x in (paths.nodes, paths.offsets, paths.cum, paths.hops, paths.status))


def _assert_same(got, want):
    for name, g, w in zip(("nodes", "offsets", "cum", "hops", "status"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(pc.bits(g) if g.dtype == np.float64 else g, pc.bits(w) if w.dtype == np.float64 else w), name


def _line(n, weights=None):
    w = np.ones(n - 1, dtype=np.float32) if weights is None else np.asarray(weights, dtype=np.float32)
    i = np.arange(n - 1)
    return sparse.csr_matrix((np.concatenate([w, w]), (np.concatenate([i, i + 1]), np.concatenate([i + 1, i]))), shape=(n, n))


def _solve(W, sources, unweighted=False):
    """(G, D f32 [S, n], P i32 [S, n]) of the GPU's own solve on the symmetric scipy graph W."""
    from vqvae_amd._device import DeviceCSR
    from vqvae_amd.geo.geo_shortest_paths import sssp_multi_device
    G = DeviceCSR.from_scipy(W, _dev())
    D, P, _, _, _ = sssp_multi_device(G, _t(sources), unweighted=unweighted, want_D=True, want_P=True)
    return G, D, P


def _extract(G, P, sources, rows, targets, **kw):
    from vqvae_amd.geo import paths_from_predecessors_device
    return paths_from_predecessors_device(G, P, _t(sources), _t(rows), _t(targets), **kw)


def _check_all_pairs(W, sources, unweighted, seed):
    """Every (source, target) pair of the GPU's own solve, in shuffled order: the kernels equal the numpy walker on the same P,
    each path runs from its source to its target, and f32(cum[hops]) is D bit for bit."""
    W = W.tocsr()
    W.sort_indices()
    n, ns = W.shape[0], len(sources)
    G, D, P = _solve(W, sources, unweighted)
    order = np.random.RandomState(seed).permutation(ns * n)
    rows, targets = (order // n).astype(np.int32), (order % n).astype(np.int32)
    got = _host(_extract(G, P, sources, rows, targets, unweighted=unweighted))
    P_h, D_h = P.cpu().numpy(), D.cpu().numpy()
    want = pc.extract(P_h, sources, rows, targets, W.indptr, W.indices, None if unweighted else W.data)
    _assert_same(got, want)
    nodes, offsets, cum, hops, status = got
    ok = status == 0
    assert np.array_equal(ok, np.isfinite(D_h[rows, targets])) and not (status == 2).any()
    assert np.array_equal(status[~ok], np.ones((~ok).sum(), dtype=np.int32)) and (hops[~ok] == -1).all()
    first, last = offsets[:-1][ok], offsets[1:][ok] - 1
    assert np.array_equal(nodes[first], np.asarray(sources)[rows[ok]]) and np.array_equal(nodes[last], targets[ok])
    assert np.array_equal(last - first, hops[ok])
    assert np.array_equal(pc.bits(cum[last].astype(np.float32)), pc.bits(D_h[rows[ok], targets[ok]]))
    return hops


def test_unit_line_graph():
    G, D, P = _solve(_line(5), [0, 2])
    nodes, offsets, cum, hops, status = _host(_extract(G, P, [0, 2], [0, 1], [4, 2]))
    assert nodes.tolist() == [0, 1, 2, 3, 4, 2] and offsets.tolist() == [0, 5, 6]
    assert cum.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 0.0] and hops.tolist() == [4, 0] and status.tolist() == [0, 0]
    nodes, _, cum, hops, _ = _host(_extract(G, P, [0, 2], [1, 1], [0, 4], unweighted=True))
    assert nodes.tolist() == [2, 1, 0, 2, 3, 4] and cum.tolist() == [0.0, 1.0, 2.0, 0.0, 1.0, 2.0] and hops.tolist() == [2, 2]


def test_a_path_longer_than_a_wave_and_a_block():
    w = (1.0 + np.arange(199) % 7 / 8.0).astype(np.float32)
    hops = _check_all_pairs(_line(200, w), [0, 199, 77], False, 1)
    assert hops.max() == 199


@pytest.mark.parametrize("M", [0, 1, 65, 257])
def test_pair_counts_across_a_wave_and_a_block(M, golden):
    W = csr_from_golden(golden("knn"), "g16/k20/distance/union", 2048)
    W.sort_indices()
    sources = [5, 900, 5]                                         # a repeated source: two rows of P with the same content
    G, D, P = _solve(W, sources)
    r = np.random.RandomState(M)
    rows = r.randint(0, 3, size=M).astype(np.int32)
    targets = r.randint(0, 40, size=M).astype(np.int32)          # 40 targets for up to 257 pairs: repeats
    paths = _extract(G, P, sources, rows, targets)
    _assert_same(_host(paths), pc.extract(P.cpu().numpy(), sources, rows, targets, W.indptr, W.indices, W.data))
    assert len(paths) == M and paths.offsets.shape == (M + 1,)
    lists = paths.to_lists()
    for m in range(min(M, 3)):
        a, b = paths.path(m)
        assert np.array_equal(a, lists[0][m]) and np.array_equal(pc.bits(b), pc.bits(lists[1][m]))


@pytest.mark.parametrize("unweighted", [False, True])
def test_golden_graph_every_pair(unweighted, golden):
    W = csr_from_golden(golden("knn"), "g16/k20/distance/union", 2048)
    hops = _check_all_pairs(W, golden("sssp")["g16/sources"].astype(np.int32), unweighted, 2)
    assert hops.max() >= 3


def _wide_weights(W):
    """Symmetric weights over a factor ~16 (0.0136 .. 0.21, the range of decoder pull-back lengths), skewed to the top of the
    range: min-hop and min-weight paths differ, and long geodesics leave the 32-bit fixed-point units."""
    from oracle.synthetic import formula_weights
    rows = np.repeat(np.arange(W.shape[0]), np.diff(W.indptr))
    f = formula_weights(np.minimum(rows, W.indices), np.maximum(rows, W.indices)).astype(np.float64)     # in [0.5, 1.5)
    W = W.copy()
    W.data = (0.0136 * np.exp2(np.clip(f - 0.5, 0.0, 1.0) ** 0.25 * 4.0)).astype(np.float32)
    return W


def test_swiss_roll_with_wide_weights_every_pair():
    from oracle import knn as okn
    W, _ = okn.build_knn_graph(swiss_roll_latents(1024, 3, 3), k=6, mode="connectivity", sym="union")
    hops = _check_all_pairs(_wide_weights(W.tocsr().astype(np.float32)), np.array([0, 511, 1023, 300], dtype=np.int32), False, 3)
    assert hops.max() > 20                                         # long geodesics: tens of hops across the roll


def test_disconnected_graph():
    from oracle import knn as okn
    W, _ = okn.build_knn_graph(latents(240, 12, 1), k=1, mode="distance", sym="mutual")
    W = W.tocsr().astype(np.float32)
    a = int(np.flatnonzero(np.diff(W.indptr) > 0)[0])              # a node with a mutual nearest neighbour; 0 and 10 have none
    hops = _check_all_pairs(W, np.array([0, 10, a], dtype=np.int32), False, 4)
    assert (hops == -1).sum() > 700 and (hops == 0).sum() == 3 and (hops == 1).sum() == 1


def test_malformed_predecessors_are_answered_not_followed():
    """Hand-written rows on a 10-node line graph: 3 <-> 4 name each other, 8 names -5, 6 names n, 5 has no predecessor and
    7 hangs below it.  Good pairs sit between the bad ones in the same launch."""
    from vqvae_amd._device import DeviceCSR
    n = 10
    G = DeviceCSR.from_scipy(_line(n), _dev())
    P = np.array([[S, 0, 1, 4, 3, S, n, 5, -5, 2],
                  [1, 2, S, 2, 3, 4, 5, 6, 7, 8]], dtype=np.int32)
    sources = [0, 2]
    rows = [0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0]
    targets = [2, 3, 9, 9, 6, 5, 0, 7, 8, 1, 2, 4]
    got = _host(_extract(G, _t(P), sources, rows, targets))
    assert got[4].tolist() == [0, 2, 0, 0, 2, 1, 0, 1, 2, 0, 0, 2]
    assert got[3].tolist() == [2, -1, 3, 7, -1, -1, 2, -1, -1, 1, 0, -1]
    _assert_same(got, pc.extract(P, sources, rows, targets, G.indptr.cpu().numpy(), G.indices.cpu().numpy(), None))
    assert got[0].tolist() == [0, 1, 2, 0, 1, 2, 9, 2, 3, 4, 5, 6, 7, 8, 9, 2, 1, 0, 0, 1, 2]
    # 2 -> 9 on row 1 is 7 hops: max_hops 6 makes that pair malformed and leaves the shorter ones alone
    short = _host(_extract(G, _t(P), sources, rows, targets, max_hops=6))
    assert short[4].tolist() == [0, 2, 0, 2, 2, 1, 0, 1, 2, 0, 0, 2]
    _assert_same(short, pc.extract(P, sources, rows, targets, G.indptr.cpu().numpy(), G.indices.cpu().numpy(), None, max_hops=6))
    exact = _host(_extract(G, _t(P), sources, rows, targets, max_hops=7))
    assert exact[4].tolist() == got[4].tolist()
    with pytest.raises(ValueError, match="max_hops"):
        _extract(G, _t(P), sources, rows, targets, max_hops=n)


def test_parallel_entries_take_the_minimum():
    """Two stored entries of different weight between the same two nodes, in both rows (a pull CSR of an undirected solve on an
    asymmetric matrix has them): the hop weighs the smaller one, and the distance identity holds."""
    from vqvae_amd._device import DeviceCSR
    from vqvae_amd.geo.geo_shortest_paths import sssp_multi_device
    indptr = np.array([0, 2, 6, 9, 10], dtype=np.int32)
    indices = np.array([1, 1, 0, 2, 0, 2, 1, 3, 1, 2], dtype=np.int32)
    data = np.array([3.0, 1.25, 3.0, 0.5, 1.25, 2.0, 2.0, 0.75, 0.5, 0.75], dtype=np.float32)
    dev = _dev()
    G = DeviceCSR(4, torch.from_numpy(indptr).to(dev), torch.from_numpy(indices).to(dev), torch.from_numpy(data).to(dev))
    D, P, _, _, _ = sssp_multi_device(G, _t([0]), want_D=True, want_P=True)
    got = _host(_extract(G, P, [0], [0, 0, 0, 0], [3, 2, 1, 0]))
    assert got[0].tolist() == [0, 1, 2, 3, 0, 1, 2, 0, 1, 0] and got[2].tolist() == [0, 1.25, 1.75, 2.5, 0, 1.25, 1.75, 0, 1.25, 0]
    _assert_same(got, pc.extract(P.cpu().numpy(), [0], [0, 0, 0, 0], [3, 2, 1, 0], indptr, indices, data))
    last = got[1][1:] - 1
    assert np.array_equal(pc.bits(got[2][last].astype(np.float32)), pc.bits(D.cpu().numpy()[0, [3, 2, 1, 0]]))


# ----------------------------------------------------------------------------------------------------------- resampling
def _golden_paths(golden, n_targets=24, unweighted=False):
    W = csr_from_golden(golden("knn"), "g16/k20/distance/union", 2048)
    W.sort_indices()
    G, D, P = _solve(W, [3, 1500], unweighted)
    r = np.random.RandomState(11)
    rows, targets = r.randint(0, 2, size=n_targets), r.randint(0, 2048, size=n_targets)
    targets[0] = 3                                                # a 0-hop path (row 0's source)
    rows[0] = 0
    return _extract(G, P, [3, 1500], rows, targets, unweighted=unweighted)


@pytest.mark.parametrize("d", [2, 16, 33, 64])
@pytest.mark.parametrize("F", [2, 3, 17, 65])
def test_resampling_equals_numpy(d, F, golden):
    from vqvae_amd.geo import resample_paths_device
    paths = _golden_paths(golden)
    z = latents(2048, d, 5)
    got = resample_paths_device(torch.from_numpy(z).to(_dev()), paths, F).cpu().numpy()
    nodes, offsets, cum, hops, _ = _host(paths)
    assert got.shape == (len(paths), F, d) and got.dtype == np.float32 and hops[0] == 0 and hops.max() >= 3
    assert np.array_equal(pc.bits(got), pc.bits(pc.resample(z, nodes, offsets, cum, F)))
    assert np.array_equal(pc.bits(got[:, 0]), pc.bits(z[nodes[offsets[:-1]]]))
    assert np.array_equal(pc.bits(got[:, -1]), pc.bits(z[nodes[offsets[1:] - 1]]))
    assert np.array_equal(pc.bits(got[0]), pc.bits(np.repeat(z[3][None], F, axis=0)))


@pytest.mark.parametrize("F", [7, 12])
def test_frame_counts_whose_positions_are_inexact(F, golden):
    """F - 1 no power of two: s and u are rounded quotients.  With u = f / 6 on a chord, a fused multiply-add in a + u (b - a)
    changes the float32 result of about one coordinate in 200; the rule is three fp64 roundings, then one to float32."""
    from vqvae_amd.geo import chord_frames_device, resample_paths_device
    paths = _golden_paths(golden)
    z = latents(2048, 16, 5)
    z_dev = torch.from_numpy(z).to(_dev())
    nodes, offsets, cum, _, _ = _host(paths)
    got = resample_paths_device(z_dev, paths, F).cpu().numpy()
    assert np.array_equal(pc.bits(got), pc.bits(pc.resample(z, nodes, offsets, cum, F)))
    r = np.random.RandomState(F)
    src, dst = r.randint(0, 2048, size=64), r.randint(0, 2048, size=64)
    assert np.array_equal(pc.bits(chord_frames_device(z_dev, src, dst, F).cpu().numpy()), pc.bits(pc.chord(z, src, dst, F)))


def test_resampling_zero_length_segments_empty_slices_and_chords():
    from vqvae_amd.geo import GeodesicPaths, chord_frames_device, resample_paths_device
    dev = _dev()
    z = latents(12, 5, 9)
    # path 0: a zero-length first and middle segment; path 1: no path; path 2: one node; path 3: every segment zero
    nodes = np.array([0, 1, 2, 3, 4, 7, 8, 9, 10], dtype=np.int32)
    offsets = np.array([0, 5, 5, 6, 9], dtype=np.int64)
    cum = np.array([0.0, 0.0, 0.75, 0.75, 2.0, 0.0, 0.0, 0.0, 0.0])
    paths = GeodesicPaths(_t(nodes), _t(offsets, torch.int64), _t(cum, torch.float64), _t([4, -1, 0, 2]), _t([0, 1, 0, 0]))
    for F in (2, 9, 17):
        got = resample_paths_device(torch.from_numpy(z).to(dev), paths, F).cpu().numpy()
        assert np.array_equal(pc.bits(got), pc.bits(pc.resample(z, nodes, offsets, cum, F)))
        assert np.isnan(got[1]).all() and np.array_equal(pc.bits(got[1]), pc.bits(np.full((F, 5), np.nan, dtype=np.float32)))
        assert np.array_equal(pc.bits(got[0, 0]), pc.bits(z[0])) and np.array_equal(pc.bits(got[0, -1]), pc.bits(z[4]))
        assert np.array_equal(pc.bits(got[2]), pc.bits(np.repeat(z[7][None], F, axis=0)))
    src, dst = np.array([0, 5, 11, 4]), np.array([3, 5, 0, 10])
    for F in (2, 3, 7, 17):
        got = chord_frames_device(torch.from_numpy(z).to(dev), src, dst, F).cpu().numpy()
        assert np.array_equal(pc.bits(got), pc.bits(pc.chord(z, src, dst, F)))
        assert np.array_equal(pc.bits(got[:, 0]), pc.bits(z[src])) and np.array_equal(pc.bits(got[:, -1]), pc.bits(z[dst]))
    assert chord_frames_device(torch.from_numpy(z).to(dev), [], [], 4).shape == (0, 4, 5)


def test_unweighted_path_with_one_frame_per_node_is_the_node_latents(golden):
    from vqvae_amd.geo import paths_from_predecessors_device, resample_paths_device
    paths = _golden_paths(golden, unweighted=True)
    nodes, offsets, cum, hops, _ = _host(paths)
    z = latents(2048, 16, 6)
    z_dev = torch.from_numpy(z).to(_dev())
    seen = set()
    for m in range(len(paths)):
        if hops[m] < 1 or hops[m] in seen:
            continue
        seen.add(int(hops[m]))
        one = type(paths)(paths.nodes[offsets[m]:offsets[m + 1]], _t([0, hops[m] + 1], torch.int64),
                          paths.cum[offsets[m]:offsets[m + 1]], paths.hops[m:m + 1], paths.status[m:m + 1])
        got = resample_paths_device(z_dev, one, int(hops[m]) + 1).cpu().numpy()
        assert np.array_equal(pc.bits(got[0]), pc.bits(z[nodes[offsets[m]:offsets[m + 1]]]))
    assert len(seen) >= 2


def test_two_streams_give_the_same_bits(golden):
    from vqvae_amd.geo import resample_paths_device
    W = csr_from_golden(golden("knn"), "g16/k20/distance/union", 2048)
    sources = [9, 1000]
    G, D, P = _solve(W, sources)
    r = np.random.RandomState(12)
    rows, targets = r.randint(0, 2, size=300), r.randint(0, 2048, size=300)
    z = torch.from_numpy(latents(2048, 16, 7)).to(_dev())
    runs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            paths = _extract(G, P, sources, rows, targets)
            frames = resample_paths_device(z, paths, 9)
        s.synchronize()
        runs.append(_host(paths) + (frames.cpu().numpy(),))
    _assert_same(runs[0][:5], runs[1][:5])
    assert np.array_equal(pc.bits(runs[0][5]), pc.bits(runs[1][5]))


def test_a_strided_view_of_a_wider_buffer_is_honoured(golden):
    W = csr_from_golden(golden("knn"), "g16/k20/distance/union", 2048)
    sources = [9, 1000, 77]
    G, D, P = _solve(W, sources)
    wide = torch.full((3, 2048 + 13), 2047, dtype=torch.int32, device=_dev())
    wide[:, :2048] = P
    view = wide[:, :2048]
    assert view.stride(0) == 2061 and not view.is_contiguous()
    r = np.random.RandomState(13)
    rows, targets = r.randint(0, 3, size=100), r.randint(0, 2048, size=100)
    _assert_same(_host(_extract(G, view, sources, rows, targets)), _host(_extract(G, P, sources, rows, targets)))


def test_one_source_per_block_equals_the_single_block_answer(golden):
    from vqvae_amd._device import DeviceCSR
    from vqvae_amd.geo import geodesic_paths_device
    W = csr_from_golden(golden("knn"), "g16/k20/distance/union", 2048)
    G = DeviceCSR.from_scipy(W, _dev())
    r = np.random.RandomState(14)
    src = r.choice([4, 4, 800, 1999, 31], size=60)                # five sources, repeated, in shuffled pair order
    dst = r.randint(0, 2048, size=60)
    dst[7] = src[7]
    one, d_one = geodesic_paths_device(G, src, dst)
    per, d_per = geodesic_paths_device(G, src, dst, max_block_bytes=1)
    _assert_same(_host(per), _host(one))
    assert np.array_equal(pc.bits(d_per.cpu().numpy()), pc.bits(d_one.cpu().numpy()))
    nodes, offsets, cum, hops, status = _host(one)
    assert (status == 0).all() and hops[7] == 0
    assert np.array_equal(nodes[offsets[:-1]], src) and np.array_equal(nodes[offsets[1:] - 1], dst)
    assert np.array_equal(pc.bits(cum[offsets[1:] - 1].astype(np.float32)), pc.bits(d_one.cpu().numpy()))
    from vqvae_amd.geo.geo_shortest_paths import distances_between
    want = distances_between(W, src, dst)[np.arange(60), np.arange(60)]
    assert np.array_equal(pc.bits(d_one.cpu().numpy()), pc.bits(want))
    empty, d_empty = geodesic_paths_device(G, [], [])
    assert len(empty) == 0 and d_empty.shape == (0,) and empty.offsets.tolist() == [0]


def test_host_wrapper_equals_the_device_lists(golden):
    from vqvae_amd._device import DeviceCSR
    from vqvae_amd.geo import geodesic_paths, geodesic_paths_device
    from oracle import knn as okn
    W, _ = okn.build_knn_graph(latents(240, 12, 1), k=1, mode="distance", sym="mutual")
    W = W.tocsr().astype(np.float32)
    a = int(np.flatnonzero(np.diff(W.indptr) > 0)[0])              # a node with a mutual nearest neighbour ...
    b = int(W.indices[W.indptr[a]])                                # ... and that neighbour
    src, dst = [0, 10, 0, -230, 5, a], [0, 11, 239, 10, -1, b]
    lists, dist = geodesic_paths(W, src, dst)
    G = DeviceCSR.from_scipy(W, _dev())
    paths, d_dev = geodesic_paths_device(G, [0, 10, 0, 10, 5, a], [0, 11, 239, 10, 239, b])
    want = paths.to_lists()[0]
    assert dist.dtype == np.float32 and np.array_equal(pc.bits(dist), pc.bits(d_dev.cpu().numpy()))
    assert len(lists) == 6 and all(x.dtype == np.int32 and np.array_equal(x, y) for x, y in zip(lists, want))
    assert lists[0].tolist() == [0] and lists[3].tolist() == [10] and dist[0] == 0.0
    assert lists[5].tolist() == [a, b] and dist[5] == W[a, b]
    status = paths.status.cpu().numpy()
    assert (status == 1).any() and all((len(a) == 0) == (s == 1) and (np.isinf(x)) == (s == 1)
                                        for a, s, x in zip(lists, status, dist))


def test_host_wrapper_raises_on_zero_weight_ties():
    """0 -1- 3 -0- 2 -0- 1: nodes 1, 2, 3 are all at distance 1.  The solver's tie rule (smallest d[u], then smallest index)
    gives 3 the predecessor 0, but 2 names 1 (index 1 < 3) and 1 names 2: a 2-cycle away from the source."""
    from vqvae_amd.geo import geodesic_paths
    r, c, w = [0, 3, 3, 2, 2, 1], [3, 0, 2, 3, 1, 2], [1.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    W = sparse.csr_matrix((np.array(w, dtype=np.float32), (r, c)), shape=(4, 4))
    assert W.nnz == 6                                              # the zero weights are stored entries
    lists, dist = geodesic_paths(W, [0], [3])
    assert lists[0].tolist() == [0, 3] and dist.tolist() == [1.0]
    with pytest.raises(ValueError, match="zero-weight"):
        geodesic_paths(W, [0, 0], [3, 1])
