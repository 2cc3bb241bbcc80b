"""GPU parity of csrc/sssp.hip through vqvae_amd.geo (the reference's API) against the golden
vectors, the oracle and the reference's own known-answer tests
(reference tests/test_geo_shortest_paths.py, tests/test_integration_knn_geo.py)."""
import numpy as np
import pytest
from scipy import sparse

from conftest import csr_from_golden, latents, swiss_roll_latents

pytestmark = pytest.mark.gpu


def line_graph(N, w=1.0):
    rows, cols, data = [], [], []
    for i in range(N - 1):
        rows += [i, i + 1]
        cols += [i + 1, i]
        data += [w, w]
    return sparse.csr_matrix((data, (rows, cols)), shape=(N, N), dtype=np.float32)


def test_line_graph_exact():
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source, dijkstra_single_source
    W = line_graph(5)
    D = dijkstra_multi_source(W, sources=[0, 2])
    assert D.shape == (2, 5) and D.dtype == np.float32
    np.testing.assert_array_equal(D[0], np.array([0, 1, 2, 3, 4], np.float32))
    np.testing.assert_array_equal(D[1], np.array([2, 1, 0, 1, 2], np.float32))
    d = dijkstra_single_source(line_graph(6), source=3)
    np.testing.assert_array_equal(d, np.array([3, 2, 1, 0, 1, 2], np.float32))


def test_long_chain_needs_many_sweeps():
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source
    n = 3000
    D = dijkstra_multi_source(line_graph(n, 0.1), sources=[0, n - 1])
    from oracle import sssp as osp
    np.testing.assert_array_equal(D, osp.dijkstra_multi_source(line_graph(n, 0.1), [0, n - 1]))


def test_weighted_vs_unweighted_and_predecessors():
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source
    W = sparse.csr_matrix((np.array([1, 1, 10, 10], np.float32), ([0, 1, 1, 2], [1, 0, 2, 1])), shape=(3, 3))
    Dw, P = dijkstra_multi_source(W, [0], return_predecessors=True)
    Du = dijkstra_multi_source(W, [0], unweighted=True)
    assert Dw[0, 2] == 11.0 and Du[0, 2] == 2.0
    assert P.dtype == np.int32 and list(P[0]) == [-9999, 0, 1]


def test_unreachable_is_inf():
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source
    W = sparse.block_diag((line_graph(3), line_graph(4)), format="csr", dtype=np.float32)
    D = dijkstra_multi_source(W, [0, 3])
    assert np.isinf(D[0, 3:]).all() and np.isfinite(D[0, :3]).all()
    assert np.isinf(D[1, :3]).all() and np.isfinite(D[1, 3:]).all()


def test_golden_distances_bit_exact(golden):
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source, distances_between
    gk, gs = golden("knn"), golden("sssp")
    W = csr_from_golden(gk, "g16/k20/distance/union", 2048)
    D, P = dijkstra_multi_source(W, gs["g16/sources"], return_predecessors=True)
    np.testing.assert_array_equal(D, gs["g16/D"])
    assert np.mean(P == gs["g16/P"]) > 0.999
    # every predecessor is a valid tight parent
    Dd = D.astype(np.float64)
    np.testing.assert_array_equal(dijkstra_multi_source(W, gs["g16/sources"][:3], unweighted=True), gs["g16/D_unweighted"])
    Wt = sparse.triu(W).tocsr()
    np.testing.assert_array_equal(dijkstra_multi_source(Wt, [0, 5], directed=True), gs["g16/D_triu_directed"])
    np.testing.assert_array_equal(dijkstra_multi_source(Wt, [0, 5], directed=False), gs["g16/D_triu_undirected"])
    sub = distances_between(W, [0, 7], [1, 5, 25])
    np.testing.assert_array_equal(sub, gs["g16/D"][:2][:, [1, 5, 25]])


def test_golden_disconnected(golden):
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source
    gk, gs = golden("knn"), golden("sssp")
    # graph regenerated through the oracle (same structure as the reference: REPORT.txt)
    from oracle import knn as okn
    W, _ = okn.build_knn_graph(latents(240, 12, 1), k=1, mode="distance", sym="mutual")
    np.testing.assert_array_equal(dijkstra_multi_source(W, [0, 10]), gs["disc/D"])


@pytest.mark.parametrize("n_sources", [1, 63, 64, 65, 200])
def test_many_sources_vs_oracle(n_sources):
    from oracle import knn as okn
    from oracle import sssp as osp
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source
    W, _ = okn.build_knn_graph(latents(1500, 16, 7), k=8, mode="distance", sym="union")
    src = np.random.RandomState(n_sources).randint(0, 1500, size=n_sources)
    np.testing.assert_array_equal(dijkstra_multi_source(W, src), osp.dijkstra_multi_source(W, src))


@pytest.mark.parametrize("group", ["0", "1", "2"])
def test_long_geodesics_16_source_batches(group, request):
    """Manifold-like latents (noisy swiss roll, ~100-hop geodesics) at a size that takes the 16-source chunk
    sweep, without / with automatic / with forced regrouping of the sources along landmark distances: distances,
    predecessors, column minimum and first-row argmin (duplicate sources force ties) against the oracle."""
    import torch
    from oracle import knn as okn
    from oracle import sssp as osp
    from vqvae_amd._device import DeviceCSR, device
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source, sssp_multi_device
    from vqvae_amd import _lib
    _lib.check(_lib.load().geo_set_option(b"sssp_group", int(group)), "geo_set_option")
    request.addfinalizer(lambda: _lib.load().geo_set_option(b"sssp_group", 1))
    n = 14000
    W, _ = okn.build_knn_graph(swiss_roll_latents(n, 16, 3), k=10, mode="distance", sym="union")
    src = np.random.RandomState(5).choice(n, 70, replace=False)
    src = np.concatenate([src, src[[3, 40, 69]]])                  # rows 70..72 repeat rows 3, 40, 69
    Do, Po = osp.dijkstra_multi_source(W, src, return_predecessors=True)
    D, P = dijkstra_multi_source(W, src, return_predecessors=True)
    np.testing.assert_array_equal(D, Do)
    reach = np.isfinite(Do)
    # predecessors: same tree distances (ties between equal-length paths may pick another parent)
    rows, cols = np.nonzero(reach & (P >= 0))
    Wd = W.tocsr()
    w_pv = np.asarray(Wd[P[rows, cols], cols]).ravel().astype(np.float64)
    np.testing.assert_array_equal((P < 0), (Po < 0))
    assert np.all(np.abs(Do[rows, P[rows, cols]].astype(np.float64) + w_pv - Do[rows, cols]) <= 1e-5 * (1 + Do[rows, cols]))
    G = DeviceCSR.from_scipy(W, device())
    _, _, dmin, arg, sweeps = sssp_multi_device(G, torch.from_numpy(src.astype(np.int32)).to(device()),
                                                want_D=False, want_min=True)
    np.testing.assert_array_equal(dmin.cpu().numpy(), Do.min(axis=0))
    np.testing.assert_array_equal(arg.cpu().numpy(), Do.argmin(axis=0))
    assert sweeps > 30                                              # long paths really were exercised


@pytest.mark.parametrize("group", [1, 2])
def test_long_geodesics_in_the_fixed_point_kernel_with_ordered_sources(group, request):
    """The swiss-roll structure with weights of one binade (seeded formula): ~60-hop geodesics fit 32 bits of weight units,
    so the fixed-point kernel answers -- and when few pairs moved in the first sweeps (or grouping is forced) it orders the
    sources along the landmark distances itself and starts over.  Same distances, minima and first-row argmin as the
    oracle; distances that cannot fit (a few weights scaled by 2^-4: finer units) send the ordered sources to the fp64 kernels."""
    import torch
    from oracle import knn as okn
    from oracle import sssp as osp
    from oracle.synthetic import formula_weights
    from vqvae_amd._device import DeviceCSR, device
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source, sssp_multi_device
    from vqvae_amd import _lib
    _lib.check(_lib.load().geo_set_option(b"sssp_group", int(group)), "geo_set_option")
    request.addfinalizer(lambda: _lib.load().geo_set_option(b"sssp_group", 1))
    n = 14000
    W, _ = okn.build_knn_graph(swiss_roll_latents(n, 16, 3), k=10, mode="connectivity", sym="union")
    W = W.tocsr()
    rows = np.repeat(np.arange(n), np.diff(W.indptr))
    W.data = formula_weights(np.minimum(rows, W.indices), np.maximum(rows, W.indices)).astype(np.float32)   # symmetric
    src = np.random.RandomState(6).choice(n, 96, replace=False)
    Do = osp.dijkstra_multi_source(W, src)
    np.testing.assert_array_equal(dijkstra_multi_source(W, src), Do)
    assert _lib.load().geo_sssp_last_profile(None, None) == 2032
    G = DeviceCSR.from_scipy(W, device())
    _, _, dmin, arg, sweeps = sssp_multi_device(G, torch.from_numpy(src.astype(np.int32)).to(device()), want_D=False, want_min=True)
    np.testing.assert_array_equal(dmin.cpu().numpy(), Do.min(axis=0))
    np.testing.assert_array_equal(arg.cpu().numpy(), Do.argmin(axis=0))
    assert sweeps > 30
    Tiny = W.copy()
    Tiny.data = (Tiny.data * np.where(formula_weights(np.minimum(rows, W.indices), np.maximum(rows, W.indices)) > 1.45,
                                      np.float32(2.0 ** -4), np.float32(1.0))).astype(np.float32)          # 5 binades: eligible, but 60 hops overflow
    np.testing.assert_array_equal(dijkstra_multi_source(Tiny, src), osp.dijkstra_multi_source(Tiny, src))


def test_seeded_sweep_over_graphs_sources_and_weight_ranges():
    """Twelve seeded combinations of structure (Gaussian cloud / swiss roll), size, degree, number of sources and weight
    range (one binade ... eleven): whichever kernels the dispatch picks (fixed point with or without ordered sources,
    16- or 64-source fp64 batches, small-graph kernel), D, the column minimum and the first-row argmin equal the oracle's."""
    import torch
    from oracle import knn as okn
    from oracle import sssp as osp
    from oracle.synthetic import formula_weights
    from vqvae_amd._device import DeviceCSR, device
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source, nearest_source_device, sssp_multi_device
    from vqvae_amd import _lib
    rs = np.random.RandomState(2024)
    seen = set()
    cases = [(3000, 6, 17, False, 0), (9000, 4, 33, True, 1), (15000, 10, 70, False, 2), (26000, 6, 130, True, 2),
             (40000, 10, 33, False, 1), (15000, 4, 70, True, 1), (26000, 10, 17, False, 0), (9000, 10, 130, False, 2),
             (40000, 4, 33, True, 0), (3000, 4, 130, True, 2), (15000, 6, 33, False, 0), (26000, 10, 70, True, 1)]
    for case, (n, k, S, roll, mode) in enumerate(cases):
        z = swiss_roll_latents(n, 8, case) if roll else latents(n, 8, case)
        W, _ = okn.build_knn_graph(z, k=k, mode="distance", sym="union")
        W = W.tocsr()
        if mode:                                                        # seeded weights: one binade, or stretched over many
            rows = np.repeat(np.arange(n), np.diff(W.indptr))
            f = formula_weights(rows, W.indices).astype(np.float64)
            W.data = (f if mode == 1 else f * np.exp2(np.floor((f - 0.5) * 11.0))).astype(np.float32)
        src = rs.choice(n, S, replace=False)
        Do = osp.dijkstra_multi_source(W, src)
        np.testing.assert_array_equal(dijkstra_multi_source(W, src), Do, err_msg=str((case, n, k, S, roll, mode)))
        seen.add(int(_lib.load().geo_sssp_last_profile(None, None)))
        G = DeviceCSR.from_scipy(W, device())
        _, _, dmin, arg, _ = sssp_multi_device(G, torch.from_numpy(src.astype(np.int32)).to(device()), want_D=False, want_min=True)
        np.testing.assert_array_equal(dmin.cpu().numpy(), Do.min(axis=0))
        np.testing.assert_array_equal(arg.cpu().numpy(), Do.argmin(axis=0))
        # the same pair from ONE label-carrying solve (declined, and answered by the K-source solve, for the wide weight ranges)
        d1, a1, _ = nearest_source_device(G, torch.from_numpy(src.astype(np.int32)).to(device()))
        np.testing.assert_array_equal(d1.cpu().numpy(), Do.min(axis=0), err_msg=str((case, "nearest")))
        np.testing.assert_array_equal(a1.cpu().numpy(), Do.argmin(axis=0), err_msg=str((case, "nearest")))
    assert len(seen) >= 3, seen                                         # several kernels really answered


def test_errors():
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source, distances_between, ensure_valid_graph
    W = line_graph(4)
    with pytest.raises(ValueError):
        dijkstra_multi_source(W, [])
    with pytest.raises(ValueError):
        distances_between(W, [0], [])
    Wn = W.copy()
    Wn.data[0] = -1
    with pytest.raises(ValueError):
        dijkstra_multi_source(Wn, [0])
    with pytest.raises(TypeError):
        ensure_valid_graph(np.zeros((3, 3)))
    with pytest.raises(ValueError):
        ensure_valid_graph(sparse.csr_matrix((3, 4)))


def test_kmedoids_golden(golden):
    from vqvae_amd.geo.kmeans_optimized import (assign_points_to_medoids, compute_quantization_error,
                                                fit_kmedoids_optimized, kpp_initialization_graph)
    from oracle import knn as okn
    gk, gm = golden("knn"), golden("kmedoids")
    Wd = csr_from_golden(gk, "g16/k20/distance/union", 2048)
    Wm, _ = okn.build_knn_graph(latents(240, 12, 1), k=1, mode="distance", sym="mutual")
    for gname, W in (("g16", Wd), ("disc", Wm)):
        for K in (1, 8, 64):
            for init in ("kpp", "random"):
                for seed in (0, 42):
                    tag = f"{gname}/K{K}/{init}/s{seed}"
                    med, assign, qe = fit_kmedoids_optimized(W, K=K, init=init, seed=seed)
                    assert med.dtype == int and assign.dtype == int and isinstance(qe, float)
                    np.testing.assert_array_equal(med, gm[f"{tag}/medoids"], err_msg=tag)
                    np.testing.assert_array_equal(assign, gm[f"{tag}/assign"], err_msg=tag)
                    gq = float(gm[f"{tag}/qe"])
                    assert qe == gq or (np.isinf(qe) and np.isinf(gq)), tag
    # the staged API (reference call structure) agrees with the fused driver
    med = gm["g16/K64/kpp/s42/medoids"].astype(int)
    assert kpp_initialization_graph(Wd, 64, seed=42) == list(med)
    assign = assign_points_to_medoids(Wd, med)
    np.testing.assert_array_equal(assign, gm["g16/K64/kpp/s42/assign"])
    assert compute_quantization_error(Wd, med, assign) == float(gm["g16/K64/kpp/s42/qe"])


def test_device_kpp_chain_equals_host_draw_and_oracle():
    """csrc/kpp.hip reproduces numpy's RandomState.choice draw bit for bit: same medoids as the host-drawn
    chain and as the oracle, on a graph large enough for multi-chunk float32 sums (N > 8192) and with a
    ragged last reduction chunk."""
    import os
    from oracle import kmedoids as ok
    from oracle import knn as okn
    from vqvae_amd.geo.kmeans_optimized import fit_kmedoids_optimized, kpp_initialization_graph
    W, _ = okn.build_knn_graph(latents(20011, 16, 11), k=10, mode="distance", sym="union")
    for K, seed in ((96, 42), (33, 7)):
        med_d, assign_d, qe_d = fit_kmedoids_optimized(W, K=K, init="kpp", seed=seed)
        os.environ["GEO_KPP_HOST_DRAW"] = "1"
        try:
            med_h, assign_h, qe_h = fit_kmedoids_optimized(W, K=K, init="kpp", seed=seed)
        finally:
            os.environ.pop("GEO_KPP_HOST_DRAW")
        np.testing.assert_array_equal(med_d, med_h)
        np.testing.assert_array_equal(assign_d, assign_h)
        assert qe_d == qe_h
        med_o, assign_o, qe_o = ok.fit_kmedoids_single_pass(W, K=K, seed=seed)
        np.testing.assert_array_equal(med_d, med_o)
        np.testing.assert_array_equal(assign_d, assign_o)
        assert qe_d == qe_o
    assert kpp_initialization_graph(W, 20, seed=3) == ok.kpp_initialization_graph(W, 20, seed=3)


@pytest.mark.parametrize("n", [150_011, 163_840])
def test_device_kpp_chain_at_large_n_equals_host_draw(n):
    """Above ~133 000 nodes numpy's reduction tree no longer fits the sum launch's LDS: every numpy buffer (8 192 elements) is
    reduced by the last of its four blocks, the buffer sums added in order by the last of those (kpp_sum_body, large n).  Same
    medoids / assignments / QE as the chain whose draws numpy itself makes on the host; 150 011 has a ragged last buffer (2 555
    elements, its own tree), 163 840 = 20 full buffers."""
    import os
    import torch
    from vqvae_amd._device import device
    from vqvae_amd.geo.kmeans_optimized import fit_kmedoids_optimized
    from vqvae_amd.geo.knn_graph_optimized import knn_graph_device
    G, _, _ = knn_graph_device(torch.from_numpy(latents(n, 8, 5)).to(device()), 8, mode="distance", sym="union")
    K = 160                                                      # (~2 % of the approximate draws decline: the exact draw runs too)
    med_d, assign_d, qe_d = fit_kmedoids_optimized(G, K=K, init="kpp", seed=11)
    os.environ["GEO_KPP_HOST_DRAW"] = "1"
    try:
        med_h, assign_h, qe_h = fit_kmedoids_optimized(G, K=K, init="kpp", seed=11)
    finally:
        os.environ.pop("GEO_KPP_HOST_DRAW")
    np.testing.assert_array_equal(med_d, med_h)
    np.testing.assert_array_equal(assign_d, assign_h)
    assert qe_d == qe_h and len(set(med_d.tolist())) == K


def test_kpp_small_and_degenerate_graphs():
    """Reference tests/test_kmeans_optimized.py:39-79,175-214 shapes: complete graphs, K=1, K>N, disconnected."""
    from oracle import kmedoids as ok
    from vqvae_amd.geo.kmeans_optimized import fit_kmedoids_optimized, kpp_initialization_graph

    def complete(N, w=1.0):
        A = np.full((N, N), w, np.float32) - np.diag(np.full(N, w, np.float32))
        return sparse.csr_matrix(A)

    tri = sparse.csr_matrix(np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]], np.float32))
    two = sparse.block_diag((tri, tri), format="csr", dtype=np.float32)
    for W, K, seed in ((complete(10), 3, 42), (complete(8), 3, 42), (tri, 1, 42), (two, 2, 42), (complete(5), 9, 1),
                       (two, 6, 3)):
        c = kpp_initialization_graph(W, K, seed=seed)
        assert c == ok.kpp_initialization_graph(W, K, seed=seed), (W.shape, K)
        med, assign, qe = fit_kmedoids_optimized(W, K=K, init="kpp", seed=seed)
        mo, ao, qo = ok.fit_kmedoids_optimized(W, K=K, init="kpp", seed=seed)
        np.testing.assert_array_equal(med, mo)
        np.testing.assert_array_equal(assign, ao)
        assert qe == qo or (np.isinf(qe) and np.isinf(qo))
        for i, m in enumerate(med):
            assert assign[m] == i                     # every medoid is its own nearest centre (positive weights)


def test_repeated_uniform_fallbacks_follow_the_reference_stream(golden):
    """Zero-weight cliques: draws degenerate (sum of weights == 0) several times in ONE chain, each taking the
    reference's uniform fallback (kmeans_optimized.py:62-69), which consumes the RandomState stream differently from a
    weighted draw.  Expected values are the reference's own outputs (tests/golden/kmedoids_zero.npz)."""
    import os
    from oracle import synthetic as syn
    from vqvae_amd.geo.kmeans_optimized import fit_kmedoids_optimized
    g = golden("kmedoids_zero")
    for i, (sizes, K, seed) in enumerate(syn.ZERO_CASES):
        W = syn.zero_clusters(sizes)
        for host_draw in (False, True):
            if host_draw:
                os.environ["GEO_KPP_HOST_DRAW"] = "1"
            try:
                med, assign, qe = fit_kmedoids_optimized(W, K=K, init="kpp", seed=seed)
            finally:
                os.environ.pop("GEO_KPP_HOST_DRAW", None)
            np.testing.assert_array_equal(med, g[f"case{i}/medoids"], err_msg=str((sizes, K, seed, host_draw)))
            np.testing.assert_array_equal(assign, g[f"case{i}/assign"])
            assert qe == float(g[f"case{i}/qe"])


def test_resident_chain_equals_step_kernel_and_oracle():
    """The resident single-workgroup chain (kpp_resident_kernel: LDS hash solve, incremental numpy sum, in-workgroup
    draw) against the step kernel and the oracle; entering it at centre 1 makes the first cells overflow its table, which
    exercises the hand-back (abort reason 4 -> that centre by the step kernel -> resume)."""
    from oracle import kmedoids as ok
    from oracle import knn as okn
    from vqvae_amd.geo import kmeans_optimized as km
    cases = [(okn.build_knn_graph(latents(20011, 16, 11), k=10, mode="distance", sym="union")[0], 96, 42),
             (okn.build_knn_graph(latents(8200, 8, 5), k=6, mode="distance", sym="union")[0], 200, 7),     # ragged numpy chunk
             (okn.build_knn_graph(swiss_roll_latents(6000, 16, 3), k=8, mode="distance", sym="union")[0], 64, 1)]
    saved = dict(km._KNOBS)
    try:
        for W, K, seed in cases:
            got = {}
            for tag, knobs in (("step", {"resident": False}), ("resident", {"resident": True, "resident_from": 16}),
                               ("resident_early", {"resident": True, "resident_from": 1})):
                km._KNOBS.update(saved)
                km._KNOBS.update(knobs)
                got[tag] = km.fit_kmedoids_optimized(W, K=K, init="kpp", seed=seed)
            mo, ao, qo = ok.fit_kmedoids_single_pass(W, K=K, seed=seed)
            for tag, (med, assign, qe) in got.items():
                np.testing.assert_array_equal(med, mo, err_msg=tag)
                np.testing.assert_array_equal(assign, ao, err_msg=tag)
                assert qe == qo, tag
    finally:
        km._KNOBS.update(saved)


def test_chain_stays_budgeted_while_a_component_is_unreached(capfd):
    """Two components (700 + 900 Gaussian latents in 8 dimensions, k = 6, union): until a centre sits in each, d_min keeps
    inf entries and the chain keeps its budgeted mode -- sweeps enqueued per solve, the maximum pass and the
    inf -> 2 * max_finite rule before every draw.  1 600 nodes are one ragged numpy buffer whose tree has several levels.
    Seeds chosen with the oracle: seed 1 puts its first three centres into the second component (centre 3 is the first in
    the other one), so two draws are made with inf entries present; seed 2 reaches both with centres 0 and 1."""
    import re
    from oracle import kmedoids as ok
    from oracle import knn as okn
    from vqvae_amd.geo import kmeans_optimized as km
    parts = [okn.build_knn_graph(latents(n, 8, s), k=6, mode="distance", sym="union")[0] for n, s in ((700, 21), (900, 22))]
    W = sparse.block_diag(parts, format="csr", dtype=np.float32)
    for seed, first_other in ((1, 3), (2, 1)):
        mo, ao, qo = ok.fit_kmedoids_optimized(W, K=24, init="kpp", seed=seed)
        side = np.asarray(ok.kpp_initialization_graph(W, 24, seed=seed)) >= 700
        assert first_other == int(np.argmax(side != side[0]))              # the seed does what the docstring says
        capfd.readouterr()
        km._KNOBS["log"] = True
        try:
            med, assign, qe = km.fit_kmedoids_optimized(W, K=24, init="kpp", seed=seed)
        finally:
            km._KNOBS["log"] = False
        log = capfd.readouterr().err
        np.testing.assert_array_equal(med, mo)
        np.testing.assert_array_equal(assign, ao)
        assert qe == qo
        calls = [(int(m.group(1)), m.group(2)) for m in re.finditer(r"\[kpp-log\] it (\d+)\.\.\d+ mode (\S+) ", log)]
        assert calls and calls[0][0] == 0, log
        # iteration first_other folds the first centre of the other component in: every call that starts at or before it
        # still sees inf entries
        early = [mode for it0, mode in calls if it0 <= first_other]
        assert early and all(mode.isdigit() for mode in early), log


def _with_option(name, value, fn):
    from vqvae_amd import _lib
    lib = _lib.load()
    _lib.check(lib.geo_set_option(name, value), "geo_set_option")
    try:
        return fn()
    finally:
        lib.geo_set_option(name, 1)


def test_fixed_point_solve_equals_fp64_solve_and_oracle():
    """The 32-bit fixed-point multi-source kernel (32 sources per row; exact while the weights span few binades and no
    distance reaches 2^32 units) against the fp64 kernels and the oracle: distances, predecessors, column minimum and
    first-row argmin; weighted, unweighted and duplicate sources."""
    import torch
    from oracle import knn as okn
    from oracle import sssp as osp
    from vqvae_amd import _lib
    from vqvae_amd._device import DeviceCSR, device
    from vqvae_amd.geo.geo_shortest_paths import _pull_structure, dijkstra_multi_source, sssp_multi_device
    n = 20011
    W, _ = okn.build_knn_graph(latents(n, 16, 11), k=10, mode="distance", sym="union")
    src = np.random.RandomState(9).choice(n, 77, replace=False)
    src = np.concatenate([src, src[[5, 60]]])
    Do, Po = osp.dijkstra_multi_source(W, src, return_predecessors=True)
    for u32 in (1, 0):
        D, P = _with_option(b"sssp_u32", u32, lambda: dijkstra_multi_source(W, src, return_predecessors=True))
        np.testing.assert_array_equal(D, Do, err_msg=f"u32={u32}")
        assert np.mean(P == Po) > 0.999                       # parents differ only where two are equally good
        np.testing.assert_array_equal((P < 0), (Po < 0))
        rows, cols = np.nonzero(np.isfinite(Do) & (P >= 0))      # ... and every parent is tight
        w_pv = np.asarray(W[P[rows, cols], cols]).ravel().astype(np.float64)
        assert np.all(np.abs(Do[rows, P[rows, cols]].astype(np.float64) + w_pv - Do[rows, cols]) <= 1e-5 * (1 + Do[rows, cols]))
    dev = device()
    G = DeviceCSR.from_scipy(_pull_structure(W, False), dev)
    st = torch.from_numpy(src.astype(np.int32)).to(dev)
    _, _, dmin, arg, _ = _with_option(b"sssp_u32", 1, lambda: sssp_multi_device(G, st, want_D=False, want_min=True))
    layout = _lib.load().geo_sssp_last_profile(None, None)
    assert layout == 2032, layout                                  # the fixed-point kernel really ran
    np.testing.assert_array_equal(dmin.cpu().numpy(), Do.min(axis=0))
    np.testing.assert_array_equal(arg.cpu().numpy(), Do.argmin(axis=0))
    Du = _with_option(b"sssp_u32", 1, lambda: dijkstra_multi_source(W, src[:40], unweighted=True))
    np.testing.assert_array_equal(Du, osp.dijkstra_multi_source(W, src[:40], unweighted=True))


def test_fixed_point_solve_declines_and_falls_back():
    """Weights spanning too many binades (not representable in 28-bit units) and distances that overflow 2^32 units:
    the call is answered by the fp64 kernels, bit-equal to the oracle."""
    from oracle import knn as okn
    from oracle import sssp as osp
    from vqvae_amd import _lib
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source
    n = 20011
    W, _ = okn.build_knn_graph(latents(n, 16, 11), k=10, mode="distance", sym="union")
    Wide = W.copy()
    Wide.data = (Wide.data * np.where(np.arange(Wide.nnz) % 7 == 0, 1e-4, 1.0)).astype(np.float32)
    Wide = Wide.maximum(Wide.T).tocsr()                            # keep it symmetric
    src = np.random.RandomState(4).choice(n, 48, replace=False)
    np.testing.assert_array_equal(dijkstra_multi_source(Wide, src), osp.dijkstra_multi_source(Wide, src))
    assert _lib.load().geo_sssp_last_profile(None, None) < 2000    # declined: 1e-4 x spread needs > 28 bits
    # a long unit-weight path: 13 000 hops x 2^23 units overflows 32 bits -> saturates -> fp64 takes over
    m = 13000
    L = line_graph(m)
    ls = np.arange(0, m, m // 40)[:40]
    got = _with_option(b"sssp_group", 0, lambda: dijkstra_multi_source(L, ls))
    np.testing.assert_array_equal(got, osp.dijkstra_multi_source(L, ls))
    assert _lib.load().geo_sssp_last_profile(None, None) < 2000


def test_large_graph_takes_fixed_point_layout_and_falls_back_to_64_source_batches():
    """Beyond the L2-sized range (n * 128 B > 12 MB) the 16/32-source layout is chosen only as the carrier of the
    fixed-point solve; weights it declines are solved by the 64-source fp64 kernel.  Both equal the oracle."""
    from oracle import knn as okn
    from oracle import sssp as osp
    from vqvae_amd import _lib
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source
    n = 100003
    W, _ = okn.build_knn_graph(latents(n, 16, 23), k=12, mode="distance", sym="union")     # short geodesics
    src = np.random.RandomState(9).choice(n, 40, replace=False)
    np.testing.assert_array_equal(dijkstra_multi_source(W, src), osp.dijkstra_multi_source(W, src))
    assert _lib.load().geo_sssp_last_profile(None, None) == 2032          # 32-bit fixed point
    Wide = W.copy()
    Wide.data = (Wide.data * np.where(np.arange(Wide.nnz) % 5 == 0, 1e-4, 1.0)).astype(np.float32)
    Wide = Wide.maximum(Wide.T).tocsr()
    np.testing.assert_array_equal(dijkstra_multi_source(Wide, src), osp.dijkstra_multi_source(Wide, src))
    assert _lib.load().geo_sssp_last_profile(None, None) == 64            # declined -> 64 sources per batch



def _set_options(request, **opts):
    from vqvae_amd import _lib
    lib = _lib.load()
    defaults = {"sssp_sb": -1, "sssp_push": 1, "sssp_delta": 8, "sssp_u32": 1, "sssp_group": 1, "sssp_push_blocks": 64,
                "sssp_order": 0}
    for name, value in opts.items():
        _lib.check(lib.geo_set_option(name.encode(), int(value)), "geo_set_option")
        request.addfinalizer(lambda name=name: lib.geo_set_option(name.encode(), defaults[name]))


def _jvp_like_weights(W, seed):
    """Symmetric weights spread over a factor ~16 (0.0136 .. 0.21, as the decoder pull-back lengths of the swiss bench
    graph): min-hop and min-weight paths differ a lot, which is what makes plain label correcting expensive.  seed 0
    skews them towards the top of the range, so that ~120-hop geodesics reach 3-4 x 2^32 units of the smallest weight's
    last bit: eligible for the 32-bit fixed-point solve by their range (5 binades), too long for it."""
    from oracle.synthetic import formula_weights
    rows = np.repeat(np.arange(W.shape[0]), np.diff(W.indptr))
    f = formula_weights(np.minimum(rows, W.indices), np.maximum(rows, W.indices)).astype(np.float64)     # in [0.5, 1.5)
    W = W.copy()
    W.data = (0.0136 * np.exp2(np.clip(f - 0.5, 0.0, 1.0) ** (0.25 if seed == 0 else 1.0) * 4.0)).astype(np.float32)
    return W


def test_long_geodesics_with_wide_weights_take_the_near_far_push_solve(request):
    """The bench's `swiss` regime in small: ~100-hop geodesics whose weights need more than 32 bits of fixed-point
    units.  The dispatch must order the sources and hand them to the near-far push solve (layout 4016); distances,
    predecessors, column minimum and first-row argmin equal the oracle's."""
    import torch
    from oracle import knn as okn
    from oracle import sssp as osp
    from vqvae_amd import _lib
    from vqvae_amd._device import DeviceCSR, device
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source, sssp_multi_device
    n = 40000                                  # (k = 6: ~250-hop geodesics, landmark eccentricity beyond 2^32 weight units)
    W, _ = okn.build_knn_graph(swiss_roll_latents(n, 16, 3), k=6, mode="connectivity", sym="union")
    W = _jvp_like_weights(W.tocsr(), 0)
    src = np.random.RandomState(5).choice(n, 100, replace=False)
    src = np.concatenate([src, src[[3, 40, 69]]])
    Do, Po = osp.dijkstra_multi_source(W, src, return_predecessors=True)
    D, P = dijkstra_multi_source(W, src, return_predecessors=True)
    assert _lib.load().geo_sssp_last_profile(None, None) == 4016       # the near-far push solve, one launch per sweep
    np.testing.assert_array_equal(D, Do)
    np.testing.assert_array_equal((P < 0), (Po < 0))
    rows, cols = np.nonzero(np.isfinite(Do) & (P >= 0))
    w_pv = np.asarray(W[P[rows, cols], cols]).ravel().astype(np.float64)
    assert np.all(np.abs(Do[rows, P[rows, cols]].astype(np.float64) + w_pv - Do[rows, cols]) <= 1e-5 * (1 + Do[rows, cols]))
    G = DeviceCSR.from_scipy(W, device())
    _, _, dmin, arg, sweeps = sssp_multi_device(G, torch.from_numpy(src.astype(np.int32)).to(device()), want_D=False, want_min=True)
    np.testing.assert_array_equal(dmin.cpu().numpy(), Do.min(axis=0))
    np.testing.assert_array_equal(arg.cpu().numpy(), Do.argmin(axis=0))


@pytest.mark.parametrize("delta,order", [(1, 1), (4, 2), (1000000, 1), (4, 1), (1, 0), (8, 0), (8, 2)])
def test_near_far_push_solve_forced_on_every_graph_equals_oracle(delta, order, request):
    """`sssp_push=2` + 16-source batches send EVERY call with more than 16 sources through the push solve, whatever the
    graph: Gaussian clouds and swiss rolls, one binade of weights or eleven, unweighted, a disconnected graph (inf
    columns, idle batches), duplicate and padded sources, for a narrow bucket (delta = 1 mean weight: many release
    sweeps), the default and an infinite one (plain push label correcting), for the three source orders (layout 4016).  All
    equal the oracle bit for bit."""
    import torch
    from oracle import knn as okn
    from oracle import sssp as osp
    from oracle.synthetic import formula_weights
    from vqvae_amd import _lib
    from vqvae_amd._device import DeviceCSR, device
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source, sssp_multi_device
    _set_options(request, sssp_sb=16, sssp_push=2, sssp_delta=delta, sssp_order=order,
                 sssp_group=2)                                  # group 2: the sources are always ordered first (cells / landmarks)
    layouts = (4016,)
    rs = np.random.RandomState(77)
    cases = [(3000, 6, 17, False, 0), (9000, 4, 33, True, 1), (15000, 10, 70, False, 2), (12000, 6, 130, True, 2),
             (6000, 4, 40, True, 0), (3000, 4, 130, True, 3)]
    for case, (n, k, S, roll, mode) in enumerate(cases):
        z = swiss_roll_latents(n, 8, case) if roll else latents(n, 8, case)
        W, _ = okn.build_knn_graph(z, k=k, mode="distance", sym="union")
        W = W.tocsr()
        if mode == 3:
            W = _jvp_like_weights(W, case)
        elif mode:
            rows = np.repeat(np.arange(n), np.diff(W.indptr))
            f = formula_weights(rows, W.indices).astype(np.float64)
            W.data = (f if mode == 1 else f * np.exp2(np.floor((f - 0.5) * 11.0))).astype(np.float32)
        src = rs.choice(n, S, replace=False)
        src[-1] = src[0]                                                # a duplicate source
        Do = osp.dijkstra_multi_source(W, src)
        np.testing.assert_array_equal(dijkstra_multi_source(W, src), Do, err_msg=str((case, n, k, S, roll, mode)))
        assert _lib.load().geo_sssp_last_profile(None, None) in layouts
        G = DeviceCSR.from_scipy(W, device())
        _, _, dmin, arg, _ = sssp_multi_device(G, torch.from_numpy(src.astype(np.int32)).to(device()), want_D=False, want_min=True)
        np.testing.assert_array_equal(dmin.cpu().numpy(), Do.min(axis=0))
        np.testing.assert_array_equal(arg.cpu().numpy(), Do.argmin(axis=0))
    # unweighted + predecessors, and two components (sources in both; unreachable = inf, predecessor -9999)
    W, _ = okn.build_knn_graph(latents(5000, 8, 9), k=6, mode="distance", sym="union")
    src = rs.choice(5000, 40, replace=False)
    np.testing.assert_array_equal(dijkstra_multi_source(W, src, unweighted=True), osp.dijkstra_multi_source(W, src, unweighted=True))
    A, _ = okn.build_knn_graph(latents(3000, 8, 1), k=6, mode="distance", sym="union")
    B, _ = okn.build_knn_graph(swiss_roll_latents(2500, 8, 2), k=6, mode="distance", sym="union")
    Wd = sparse.block_diag((A, B), format="csr", dtype=np.float32)
    src = np.concatenate([rs.choice(3000, 20, replace=False), 3000 + rs.choice(2500, 20, replace=False)])
    Do, Po = osp.dijkstra_multi_source(Wd, src, return_predecessors=True)
    D, P = dijkstra_multi_source(Wd, src, return_predecessors=True)
    np.testing.assert_array_equal(D, Do)
    np.testing.assert_array_equal(P < 0, Po < 0)
    assert np.isinf(D[:20, 3000:]).all() and np.isinf(D[20:, :3000]).all()


def _check_small_chunked_route(request, W, layout, **opts):
    """40 sources (one repeated) on a 3000-node graph with `sssp_sb=16` (the chunked layout below 12 289 nodes) and `opts`:
    D, column minimum and first-row argmin equal the oracle's, and the call reports `layout`."""
    import torch
    from oracle import sssp as osp
    from vqvae_amd import _lib
    from vqvae_amd._device import DeviceCSR, device
    from vqvae_amd.geo.geo_shortest_paths import dijkstra_multi_source, sssp_multi_device
    _set_options(request, sssp_sb=16, sssp_push=0, sssp_group=2, **opts)
    src = np.random.RandomState(8).choice(W.shape[0], 40, replace=False)
    src[-1] = src[2]                                                # a duplicate source: ties for the first-row argmin
    Do = osp.dijkstra_multi_source(W, src)
    np.testing.assert_array_equal(dijkstra_multi_source(W, src), Do)
    assert _lib.load().geo_sssp_last_profile(None, None) == layout
    G = DeviceCSR.from_scipy(W, device())
    _, _, dmin, arg, sweeps = sssp_multi_device(G, torch.from_numpy(src.astype(np.int32)).to(device()), want_D=False, want_min=True)
    assert _lib.load().geo_sssp_last_profile(None, None) == layout
    np.testing.assert_array_equal(dmin.cpu().numpy(), Do.min(axis=0))
    np.testing.assert_array_equal(arg.cpu().numpy(), Do.argmin(axis=0))
    assert sweeps >= 8                                              # the first group of 4, then the restarted solve's groups


def test_ordered_fp64_chunk_sweeps_without_the_push_solve(request):
    """`sssp_push=0, sssp_u32=0, sssp_group=2` on a small forced-chunked swiss roll: after its first group the fp64 chunk sweep
    orders the sources along the landmark distances and starts over with the grouped grid cap (layout 1016)."""
    from oracle import knn as okn
    W, _ = okn.build_knn_graph(swiss_roll_latents(3000, 16, 3), k=6, mode="distance", sym="union")
    _check_small_chunked_route(request, W.tocsr(), 1016, sssp_u32=0)


def test_fixed_point_solve_restarts_ordered_by_hop_counts(request):
    """`sssp_push=0, sssp_group=2, sssp_order=2`, weights of one binade: the fixed-point solve orders the sources by two
    landmark hop counts after its first group, starts over and answers (layout 2032)."""
    from oracle import knn as okn
    from oracle.synthetic import formula_weights
    W, _ = okn.build_knn_graph(swiss_roll_latents(3000, 16, 3), k=6, mode="connectivity", sym="union")
    W = W.tocsr()
    rows = np.repeat(np.arange(3000), np.diff(W.indptr))
    W.data = formula_weights(np.minimum(rows, W.indices), np.maximum(rows, W.indices)).astype(np.float32)   # symmetric
    _check_small_chunked_route(request, W, 2032, sssp_order=2)


def _nearest_both_ways(W, sources, unweighted=False):
    """(dmin, argmin) from the ONE-solve nearest-source kernel and from the K-source solve, plus the layout the former took."""
    import torch
    from vqvae_amd._device import DeviceCSR, device
    from vqvae_amd.geo.geo_shortest_paths import nearest_source_device, sssp_multi_device
    from vqvae_amd import _lib
    dev = device()
    G = DeviceCSR.from_scipy(W, dev)
    src = torch.from_numpy(np.asarray(sources, np.int32)).to(dev)
    lib = _lib.load()
    status = np.zeros(4, np.int32)
    from vqvae_amd._device import ptr, stream_ptr, workspace
    ws = workspace(lib.geo_sssp_nearest_workspace_bytes(G.n, G.nnz), dev)
    d1 = torch.empty(G.n, dtype=torch.float32, device=dev)
    a1 = torch.empty(G.n, dtype=torch.int32, device=dev)
    _lib.check(lib.geo_sssp_nearest_source(ptr(G.indptr), ptr(G.indices), ptr(None if unweighted else G.data), G.n, G.nnz,
                                           ptr(src), int(src.numel()), ptr(d1), ptr(a1), ptr(ws), ws.numel(),
                                           status.ctypes.data, stream_ptr()), "geo_sssp_nearest_source")
    dn, an, _ = nearest_source_device(G, src, unweighted=unweighted)             # (falls back by itself when declined)
    _, _, dk, ak, _ = sssp_multi_device(G, src, unweighted=unweighted, want_D=False, want_min=True)
    if status[0] == 0:
        np.testing.assert_array_equal(d1.cpu().numpy(), dn.cpu().numpy())
        np.testing.assert_array_equal(a1.cpu().numpy(), an.cpu().numpy())
    return (dn.cpu().numpy(), an.cpu().numpy()), (dk.cpu().numpy(), ak.cpu().numpy()), int(status[0]), int(status[1])


def test_nearest_source_in_one_solve_equals_the_k_source_solve_and_the_oracle():
    """geo_sssp_nearest_source: min_s D[s][v] and its FIRST row from one label-carrying fixed-point solve -- against the K-source
    solve (bit for bit, ties included) on a kNN distance graph with repeated sources, the same graph unweighted and with all
    weights equal (ties everywhere: lowest source row wins), a long-geodesics graph, two components (unreachable nodes:
    +inf, row 0); against the oracle's matrix on the first; and declined + answered by the K-source solve when the weights
    span too many binades."""
    from oracle import knn as ok
    from oracle import sssp as osp
    r = np.random.RandomState(11)
    W, _ = ok.build_knn_graph(latents(6000, 16, 3), k=10, sym="union")
    W = W.tocsr().astype(np.float32)
    src = r.choice(6000, 200, replace=False)
    src[17] = src[3]                                            # a repeated medoid: the lower row owns the cell
    (dn, an), (dk, ak), declined, sweeps = _nearest_both_ways(W, src)
    assert declined == 0 and 2 <= sweeps < 200
    np.testing.assert_array_equal(dn, dk)
    np.testing.assert_array_equal(an, ak)
    D = osp.dijkstra_multi_source(W, src)
    np.testing.assert_array_equal(dn, D.min(axis=0))
    np.testing.assert_array_equal(an, D.argmin(axis=0))
    assert not (an == 17).any()
    # ties everywhere
    for Wt, unw in ((W, True), (sparse.csr_matrix((np.ones_like(W.data), W.indices, W.indptr), shape=W.shape), False)):
        (dn, an), (dk, ak), declined, _ = _nearest_both_ways(Wt, src, unweighted=unw)
        assert declined == 0
        np.testing.assert_array_equal(dn, dk)
        np.testing.assert_array_equal(an, ak)
    # long geodesics, JVP-like weights
    Ws, _ = ok.build_knn_graph(swiss_roll_latents(8000, 16, 2), k=8, sym="union")
    Ws = _jvp_like_weights(Ws.tocsr().astype(np.float32), 1)
    srcs = r.choice(8000, 64, replace=False)
    (dn, an), (dk, ak), declined, sweeps = _nearest_both_ways(Ws, srcs)
    assert declined == 0 and sweeps > 8
    np.testing.assert_array_equal(dn, dk)
    np.testing.assert_array_equal(an, ak)
    # two components, sources in one of them only
    Wd = sparse.block_diag((W[:3000][:, :3000], W[3000:][:, 3000:]), format="csr", dtype=np.float32)
    (dn, an), (dk, ak), declined, _ = _nearest_both_ways(Wd, r.choice(3000, 40, replace=False))
    np.testing.assert_array_equal(dn, dk)
    np.testing.assert_array_equal(an, ak)
    assert np.isinf(dn).any() and (an[np.isinf(dn)] == 0).all()
    # weights over 12 binades: not ours -- the wrapper answers with the K-source solve
    Ww = W.copy()
    Ww.data = (Ww.data * np.exp2(r.randint(0, 12, Ww.nnz))).astype(np.float32)
    Ww = Ww.maximum(Ww.T).tocsr()
    (dn, an), (dk, ak), declined, _ = _nearest_both_ways(Ww, src)
    assert declined == 1
    np.testing.assert_array_equal(dn, dk)
    np.testing.assert_array_equal(an, ak)


def _collision_gadget(extras, hops):
    """A star of chains: medoid_i --(hops edges of 1.0, one of them + extras[i] * 2^-23)-- hub, plus a tail node behind the hub
    (edge 0.5).  Exact distances hub <- medoid_i differ by multiples of 2^-23 and ROUND TO THE SAME float32 (hops in [4, 8):
    spacing 2^-21, so +0, +1 and +2 units all give float32(hops); the tail sees hops + 0.5 likewise).  Returns (W, medoid
    nodes, hub, tail)."""
    m = len(extras)
    n = m * hops + 2                                            # per chain: medoid + hops-1 inner nodes; hub; tail
    hub, tail = n - 2, n - 1
    rows, cols, data, meds = [], [], [], []
    for i, ex in enumerate(extras):
        chain = [i * hops + j for j in range(hops)] + [hub]
        meds.append(chain[0])
        for j in range(hops):
            w = np.float32(1.0) + (np.float32(ex * 2.0 ** -23) if j == hops // 2 else np.float32(0))
            rows += [chain[j], chain[j + 1]]
            cols += [chain[j + 1], chain[j]]
            data += [w, w]
    rows += [hub, tail]
    cols += [tail, hub]
    data += [0.5, 0.5]
    return sparse.csr_matrix((np.asarray(data, np.float32), (rows, cols)), shape=(n, n)), meds, hub, tail


def _nearest_with_info(W, sources):
    import torch
    from vqvae_amd._device import DeviceCSR, device
    from vqvae_amd.geo.geo_shortest_paths import nearest_source_device
    info = {}
    G = DeviceCSR.from_scipy(W, device())
    d, a, _ = nearest_source_device(G, torch.from_numpy(np.asarray(sources, np.int32)).to(device()), info=info)
    return d.cpu().numpy(), a.cpu().numpy(), info


def test_nearest_source_breaks_float32_collisions_like_the_reference_nine_node_counter_example():
    """Round-3 review, "what's weak" 1: medoid row 0 -- 1.0, 1.0, 1.0, 1 + 2^-23 -- v; medoid row 1 -- four edges of 1.0 -- v.
    D[:, v] = [4.00000012, 4.0] in fp64, [4.0, 4.0] after the reference's float32 cast (geo_shortest_paths.py:50), so
    D.argmin(axis=0)[v] = 0 (kmeans_optimized.py:100) although medoid 1 is exactly nearer.  Both row orders, the public API, and
    the K-source path."""
    from oracle import sssp as osp
    from vqvae_amd.geo.kmeans_optimized import assign_points_to_medoids
    rows, cols, data = [], [], []
    def edge(a, b, w):
        rows.extend([a, b]); cols.extend([b, a]); data.extend([w, w])
    edge(0, 1, 1.0); edge(1, 2, 1.0); edge(2, 3, 1.0); edge(3, 8, np.float32(1.0) + np.float32(2.0 ** -23))
    edge(4, 5, 1.0); edge(5, 6, 1.0); edge(6, 7, 1.0); edge(7, 8, 1.0)
    W = sparse.csr_matrix((np.asarray(data, np.float32), (rows, cols)), shape=(9, 9))
    for src, expect_v in (([0, 4], 0), ([4, 0], 0)):
        D = osp.dijkstra_multi_source(W, src)
        assert D.dtype == np.float32 and D[0, 8] == D[1, 8] == 4.0
        assert D.argmin(axis=0)[8] == expect_v
        d, a, info = _nearest_with_info(W, src)
        assert not info["declined"] and info["suspects"] >= 1
        np.testing.assert_array_equal(a, D.argmin(axis=0))
        np.testing.assert_array_equal(d, D.min(axis=0))
        np.testing.assert_array_equal(assign_points_to_medoids(W, np.asarray(src)), D.argmin(axis=0))
        (dn, an), (dk, ak), declined, _ = _nearest_both_ways(W, src)
        assert declined == 0
        np.testing.assert_array_equal(an, ak)
        np.testing.assert_array_equal(dn, dk)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_nearest_source_float32_collisions_seeded_family_equals_the_oracle_matrix(seed):
    """A kNN distance graph with generic float32 weights plus planted collision gadgets (two- and three-medoid stars whose exact
    distances differ by 1-2 units of 2^-23 but round to one float32; with three medoids the LOWEST row can be the exactly
    FARTHEST of the three, i.e. outside the two keys the relaxation carries), source rows shuffled so that both row orders
    occur: argmin / min of the oracle's float32 matrix, and the K-source solve, bit for bit; the suspects are counted."""
    from oracle import knn as ok
    from oracle import sssp as osp
    r = np.random.RandomState(100 + seed)
    Wm, _ = ok.build_knn_graph(latents(1500, 8, 20 + seed), k=8, sym="union")
    blocks, meds, off, planted = [Wm.tocsr().astype(np.float32)], list(r.choice(1500, 24, replace=False)), 1500, 0
    for g in range(3):
        m = 2 + (g + seed) % 2
        hops = int(r.randint(4, 8))
        extras = list(r.permutation(3)[:m])                     # distinct multiples of 2^-23 within the rounding window
        Wg, gm, hub, tail = _collision_gadget(extras, hops)
        blocks.append(Wg)
        meds += [off + x for x in gm]
        planted += 2                                            # hub and tail
        off += Wg.shape[0]
    W = sparse.block_diag(blocks, format="csr", dtype=np.float32)
    src = np.asarray(meds)[r.permutation(len(meds))]
    D = osp.dijkstra_multi_source(W, src)
    d, a, info = _nearest_with_info(W, src)
    assert not info["declined"], info
    assert planted <= info["suspects"] <= 32
    np.testing.assert_array_equal(a, D.argmin(axis=0))
    np.testing.assert_array_equal(d, D.min(axis=0))
    (dn, an), (dk, ak), declined, _ = _nearest_both_ways(W, src)
    np.testing.assert_array_equal(an, ak)
    np.testing.assert_array_equal(dn, dk)
    # the case the two carried keys alone cannot decide must occur in the family: lowest row exactly farthest of three
    if seed == 0:
        Wg, gm, hub, _ = _collision_gadget([2, 1, 0], 5)
        Dg = osp.dijkstra_multi_source(Wg, gm)
        assert Dg.argmin(axis=0)[hub] == 0
        d3, a3, info3 = _nearest_with_info(Wg, gm)
        assert not info3["declined"] and a3[hub] == 0 and info3["suspects"] >= 2
        np.testing.assert_array_equal(a3, Dg.argmin(axis=0))


def test_nearest_source_declines_when_float32_collisions_are_everywhere():
    """Weights drawn from {1, 1 + 2^-23} on a kNN structure: distances from two hops on exceed 2^24 units and most nodes see
    two medoids inside one float32 rounding window -> more suspects than the call resolves; it declines (reason 3) and the
    wrapper's K-source solve gives the oracle's rows."""
    from oracle import knn as ok
    from oracle import sssp as osp
    r = np.random.RandomState(5)
    W, _ = ok.build_knn_graph(latents(2000, 8, 9), k=6, sym="union")
    W = sparse.triu(W.tocsr(), k=1).tocsr().astype(np.float32)
    W.data = (1.0 + r.randint(0, 2, W.nnz) * 2.0 ** -23).astype(np.float32)
    W = (W + W.T).tocsr().astype(np.float32)
    src = r.choice(2000, 40, replace=False)
    D = osp.dijkstra_multi_source(W, src)
    d, a, info = _nearest_with_info(W, src)
    assert info["declined"] and info["reason"] == 3 and info["suspects"] > 32
    np.testing.assert_array_equal(a, D.argmin(axis=0))
    np.testing.assert_array_equal(d, D.min(axis=0))


def test_nearest_source_never_wraps_on_heavy_long_paths():
    """Advisor (round 3): intermediate upper bounds may pass 2^40 units although final distances do not.  A path of 6 000
    edges whose weights alternate between 1 and 30 (28-bit units): the distance limit is checked before every add, the call
    declines (reason 2) instead of wrapping, and the wrapper's answer is the oracle's."""
    from oracle import sssp as osp
    n = 6000
    w = np.where(np.arange(n - 1) % 2 == 0, np.float32(1.0 + 2.0 ** -23), np.float32(30.0)).astype(np.float32)
    rows = np.concatenate([np.arange(n - 1), np.arange(1, n)])
    cols = np.concatenate([np.arange(1, n), np.arange(n - 1)])
    W = sparse.csr_matrix((np.concatenate([w, w]), (rows, cols)), shape=(n, n))
    src = [0, 5]
    D = osp.dijkstra_multi_source(W, src)
    d, a, info = _nearest_with_info(W, src)
    assert info["declined"] and info["reason"] == 2, info
    np.testing.assert_array_equal(a, D.argmin(axis=0))
    np.testing.assert_array_equal(d, D.min(axis=0))


def test_quantization_error_of_an_arbitrary_assignment_takes_the_matrix():
    """compute_quantization_error answers the nearest-medoid assignment from the one-solve path (golden cases above); any
    other assignment must still read D[assign[v]][v] from the K-source matrix -- against the oracle."""
    from oracle import kmedoids as okm
    from oracle import knn as ok
    from vqvae_amd.geo.kmeans_optimized import assign_points_to_medoids, compute_quantization_error
    W, _ = ok.build_knn_graph(latents(1500, 8, 4), k=8, sym="union")
    W = W.tocsr().astype(np.float32)
    med = np.random.RandomState(2).choice(1500, 12, replace=False)
    nearest = assign_points_to_medoids(W, med)
    other = (nearest + 1) % 12
    assert compute_quantization_error(W, med, nearest) == okm.compute_quantization_error(W, med, nearest)
    assert compute_quantization_error(W, med, other) == okm.compute_quantization_error(W, med, other)
