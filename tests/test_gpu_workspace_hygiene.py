"""The geometry side's kernels that take their scratch from vqvae_amd._device.workspace() -- graph build, clustering, shortest
paths, the spatial pull-back, the feature moments -- run at EXACTLY the size their *_workspace_bytes query answers, between
guard bands, on scratch that holds zeros, ones or the leftovers of another problem (tests/ws_guard.py).  The model side (image
encode and decode, LPIPS, the vanilla pull-back, the metric tensor, and the entry points that allocate their scratch per call:
k-means, the quantizer, the ELBO, the prior's decode) is in tests/test_gpu_workspace_hygiene_models.py; between them the two
reach every module of the package that hands a kernel scratch.

Production hands the library a grow-only buffer that is at least 256 bytes (after a JVP stage: gigabytes) larger than asked
for and holds what the last kernel left there, so a query that under-reports, an index a little past the last carve and a read
of scratch the call never wrote cannot fail any other test.  Each case runs its wrapper four times:

    P  production allocator                                            input B
    Z  guarded, zeros                                                  input B
    O  guarded, every 32-bit word 1                                    input B
    S  guarded, stale: right after one call on input A (same shapes)   input B

and asserts (a) no library error, (b) intact guards, (c) every documented output of Z, O, S equal to P's bit for bit
(predecessors: same tree distances, the rule of test_gpu_sssp.py; mode-dependent counters are not outputs), (d) that the route
the case names is the one the library reports."""
import functools
import re

import numpy as np
import pytest
import torch
from scipy import sparse

from conftest import latents, swiss_roll_latents
from ws_guard import four_runs as _four_runs

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ helpers
def _dev():
    from vqvae_amd._device import device
    return device()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _options(request, defaults, **opts):
    from vqvae_amd import _lib
    lib = _lib.load()
    for name, value in opts.items():
        request.addfinalizer(lambda name=name: lib.geo_set_option(name.encode(), defaults[name]))
        _lib.check(lib.geo_set_option(name.encode(), int(value)), "geo_set_option")


# ------------------------------------------------------------------------------------------------------------------- graphs
@functools.lru_cache(maxsize=None)
def _knn_graph(kind, n, d, seed, k, mode="distance", sym="union"):
    """The kNN graph the shortest-path tests build with the oracle, built on the GPU (canonical CSR, float32)."""
    from vqvae_amd.geo.knn_graph_optimized import knn_graph_device
    z = swiss_roll_latents(n, d, seed) if kind == "swiss" else latents(n, d, seed)
    G, _, _ = knn_graph_device(_t(z), k, mode=mode, sym=sym)
    W = G.to_scipy().tocsr()
    W.sort_indices()
    return W


def _relabel(W, seed, scale=np.float32(1.37)):
    """(W', perm): W with node i renamed perm[i] and every weight scaled -- same n, same nnz, other rows and other values."""
    W = W.tocoo()
    perm = np.random.RandomState(seed).permutation(W.shape[0])
    A = sparse.csr_matrix(((W.data.astype(np.float32) * scale).astype(np.float32), (perm[W.row], perm[W.col])), shape=W.shape)
    A.sort_indices()
    assert A.nnz == W.nnz
    return A, perm


def _device_csr(W):
    from vqvae_amd._device import DeviceCSR
    return DeviceCSR.from_scipy(W, _dev())


def _csr_out(G, prefix=""):
    return {prefix + "indptr": G.indptr, prefix + "indices": G.indices, prefix + "data": G.data}


# ------------------------------------------------------------------------------------------- kNN and graph construction
EXACT, WIDE, BF16, F32, TWO = 1, 2, 3, 4, 5            # geo_knn_last_path() (GEO_KNN_PATH_* of include/geo_hip.h)


@pytest.mark.parametrize("n,d,kq,filt,rows,path", [
    (3000, 16, 10, 1, None, EXACT),
    (3000, 16, 10, 1, (1000, 1500), EXACT),
    (3000, 16, 65, 1, None, WIDE),
    (16384, 64, 21, 1, None, BF16),
    (16384, 64, 21, 2, None, F32),
    (200000, 8, 2, 1, None, TWO),
], ids=["exact", "exact_rows_1000_1500", "exact_wide", "filter_bf16", "filter_f32", "two_level"])
def test_knn_search(n, d, kq, filt, rows, path, monkeypatch, request):
    from vqvae_amd import _lib
    from vqvae_amd.geo.knn_graph_optimized import knn_search_device
    _options(request, {"knn_filter": 1}, knn_filter=filt)
    r0, r1 = rows if rows else (0, None)

    def call(z):
        idx, d2 = knn_search_device(z, kq, r0, r1)
        return {"idx": idx, "d2": d2}, _lib.load().geo_knn_last_path()

    out = _four_runs(monkeypatch, call, _t(latents(n, d, 2)), _t(latents(n, d, 1)), path)
    assert out["idx"].shape == ((r1 - r0) if rows else n, kq)


@functools.lru_cache(maxsize=None)
def _neighbour_lists(seed):
    """Directed lists int32 [1000, 10] and float32 weights of 1 000 Gaussian latents in 8 dimensions (self dropped)."""
    from vqvae_amd.geo.knn_graph_optimized import knn_search_device
    idx, d2 = knn_search_device(_t(latents(1000, 8, seed)), 11)
    return idx[:, 1:].contiguous(), torch.sqrt(d2[:, 1:]).to(torch.float32).contiguous()


@pytest.mark.parametrize("weighted", [True, False], ids=["weights", "no_weights"])
@pytest.mark.parametrize("sym", ["mutual", "union"])
def test_symmetrize(sym, weighted, monkeypatch):
    from vqvae_amd.geo.knn_graph_optimized import symmetrize_device

    def call(inp):
        idx, w = inp
        return _csr_out(symmetrize_device(idx, w if weighted else None, sym)), sym

    out = _four_runs(monkeypatch, call, _neighbour_lists(4), _neighbour_lists(3), sym)
    assert 1000 < out["indices"].numel() < 20000


@functools.lru_cache(maxsize=None)
def _three_components():
    """(W, z, keep): 1 500 nodes, three kNN components of 500 (Gaussian blobs 40 apart, k = 6, union), 5 % of the edges with a
    stored weight of zero; a keep mask over 80 % of the nodes."""
    from oracle import knn as okn
    r = np.random.RandomState(8)
    zs = [latents(500, 8, 30 + c) + np.float32(40 * c) for c in range(3)]
    parts = [okn.build_knn_graph(z, k=6, mode="distance", sym="union")[0] for z in zs]
    assert all(okn.connected_components(Wc)[0] == 1 for Wc in parts)
    W = sparse.block_diag(parts, format="csr", dtype=np.float32)
    up = sparse.triu(W, k=1).tocoo()
    zero = r.rand(up.nnz) < 0.05
    data = np.where(zero, np.float32(0), up.data).astype(np.float32)
    rows, cols = np.concatenate([up.row, up.col]), np.concatenate([up.col, up.row])
    W0 = sparse.csr_matrix((np.concatenate([data, data]), (rows, cols)), shape=W.shape)        # (explicit zeros stay stored)
    W0.sort_indices()
    assert W0.nnz == W.nnz and (W0.data == 0).sum() == 2 * zero.sum() > 0
    return W0, np.concatenate(zs).astype(np.float32), r.rand(1500) < 0.8


def _three_components_inputs():
    """B = (G, z, keep) and A: the same graph relabelled and rescaled, its latents and keep mask moved with the nodes."""
    W, z, keep = _three_components()
    WA, perm = _relabel(W, 5)
    zA, keepA = np.empty_like(z), np.empty_like(keep)
    zA[perm], keepA[perm] = z * np.float32(1.37), keep
    return (_device_csr(WA), _t(zA), _t(keepA)), (_device_csr(W), _t(z), _t(keep))


def test_connected_components(monkeypatch):
    from vqvae_amd.geo.knn_graph_optimized import connected_components_device

    def call(inp):
        ncomp, labels = connected_components_device(inp[0])
        return {"ncomp": ncomp, "labels": labels}, ncomp

    A, B = _three_components_inputs()
    out = _four_runs(monkeypatch, call, A, B, 3)
    assert np.array_equal(out["labels"].cpu().numpy(), np.repeat(np.arange(3), 500))


def test_compact_with_keep_mask_and_drop_zero(monkeypatch):
    from vqvae_amd.geo.knn_graph_optimized import compact_device

    def call(inp):
        G, _, keep = inp
        G2, new_index = compact_device(G, keep, drop_zero=True)
        return dict(_csr_out(G2), n=G2.n, new_index=new_index), "keep+drop_zero"

    A, B = _three_components_inputs()
    out = _four_runs(monkeypatch, call, A, B, "keep+drop_zero")
    W, _, keep = _three_components()
    sub = W[keep][:, keep].tocsr()
    sub.eliminate_zeros()
    assert out["n"] == int(keep.sum()) and out["indices"].numel() == sub.nnz < W[keep][:, keep].nnz


def test_upper_edges(monkeypatch):
    from vqvae_amd.geo.knn_graph_optimized import upper_edges_device

    def call(inp):
        src, dst, entry_edge = upper_edges_device(inp[0])
        return {"src": src, "dst": dst, "entry_edge": entry_edge}, "upper"

    A, B = _three_components_inputs()
    out = _four_runs(monkeypatch, call, A, B, "upper")
    assert out["src"].numel() * 2 == _three_components()[0].nnz


def test_bridge_components(monkeypatch):
    """connected components, geo_nearest_foreign / geo_bridge_components and geo_csr_insert_* in one wrapper."""
    from vqvae_amd.geo.knn_graph_optimized import bridge_components_device, connected_components_device

    def call(inp):
        G, z, _ = inp
        G2, edges, keys, info = bridge_components_device(G, z, mode="distance")
        return dict(_csr_out(G2), edges=edges, keys=keys, queries=info["queries"], rounds=info["rounds"]), info["components"]

    A, B = _three_components_inputs()
    out = _four_runs(monkeypatch, call, A, B, 3)
    assert out["edges"].shape == (2, 2) and out["indices"].numel() == B[0].nnz + 4
    from vqvae_amd._device import DeviceCSR
    assert connected_components_device(DeviceCSR(1500, out["indptr"], out["indices"], out["data"]))[0] == 1


def test_csr_insert(monkeypatch):
    """geo_csr_insert_count / _fill on their own: 7 undirected edges into a 300-node graph."""
    from vqvae_amd.geo.knn_graph_optimized import csr_insert_device
    W = _knn_graph("gauss", 300, 8, 41, 6)
    WA, perm = _relabel(W, 6)

    def edges(seed, Wg):
        r = np.random.RandomState(seed)
        src = r.choice(300, 7, replace=False).astype(np.int32)
        dst = ((src + 1 + r.randint(0, 298, 7)) % 300).astype(np.int32)              # never a self edge
        src[6], dst[6] = int(Wg.indices[Wg.indptr[5]]), 5                             # one pair the graph already stores
        return _device_csr(Wg), _t(src), _t(dst), _t(r.rand(7).astype(np.float32) + np.float32(0.5))

    def call(inp):
        return _csr_out(csr_insert_device(*inp)), "insert"

    out = _four_runs(monkeypatch, call, edges(2, WA), edges(1, W), "insert")
    assert W.nnz < out["indices"].numel() <= W.nnz + 12


@pytest.mark.parametrize("resident_nodes_max,cells", [(None, (5, 0)), (1, (0, 5))], ids=["resident", "slices"])
def test_cell_costs(resident_nodes_max, cells, monkeypatch):
    """geo_cell_costs on 600 nodes in 5 cells: every cell's rows in LDS, and (resident_nodes_max = 1) every cell in a slice of
    the workspace."""
    from vqvae_amd.geo.kmeans_optimized import cell_medoid_update_device
    z = latents(600, 8, 43)
    W = _knn_graph("gauss", 600, 8, 43, 6)
    med = np.random.RandomState(3).choice(600, 5, replace=False).astype(np.int32)
    assign = ((z[:, None, :] - z[med][None]) ** 2).sum(-1).argmin(1).astype(np.int32)
    assert np.bincount(assign, minlength=5).min() > 1
    WA, perm = _relabel(W, 7)
    assignA = np.empty_like(assign)
    assignA[perm] = assign

    def call(inp):
        info = {}
        new, cost = cell_medoid_update_device(inp[0], inp[1], inp[2], resident_nodes_max=resident_nodes_max, info=info)
        return {"medoids": new, "cost": cost}, (info["resident_cells"], info["workspace_cells"])

    out = _four_runs(monkeypatch, call, (_device_csr(WA), _t(assignA), _t(perm[med].astype(np.int32))),
                     (_device_csr(W), _t(assign), _t(med)), cells)
    assert out["cost"].shape == (600,) and len(set(out["medoids"].tolist())) == 5


def test_nearest_foreign(monkeypatch):
    from vqvae_amd.geo.knn_graph_optimized import nearest_foreign_device

    def inputs(seed):
        r = np.random.RandomState(seed)
        return (_t(latents(500, 5, seed)), _t(r.randint(0, 3, 500).astype(np.int32)),
                _t(r.choice(500, 60, replace=False).astype(np.int32)))

    def call(inp):
        nbr, key = nearest_foreign_device(*inp)
        return {"nbr": nbr, "key": key}, "foreign"

    z, labels, rows = inputs(1)
    out = _four_runs(monkeypatch, call, inputs(2), (z, labels, rows), "foreign")
    nbr = out["nbr"].long()
    assert out["nbr"].shape == (60,) and bool((labels[nbr] != labels[rows.long()]).all()) and bool(torch.isfinite(out["key"]).all())


def test_knn_thresholds(monkeypatch):
    """geo_knn_thresholds has no wrapper and no query of its own: twice geo_knn_workspace_bytes, as include/geo_hip.h says."""
    from vqvae_amd import _device, _lib
    lib = _lib.load()
    n, d, kq, stride = 500, 5, 5, 8

    def call(z):
        tau = torch.full((n,), -7.0, dtype=torch.float64, device=z.device)
        nbytes = 2 * lib.geo_knn_workspace_bytes(n, d)
        with torch.cuda.device(z.device):
            ws = _device.workspace(nbytes, z.device)
            _lib.check(lib.geo_knn_thresholds(_device.ptr(z), n, d, kq, 0, 0, n, stride, _device.ptr(tau), _device.ptr(ws), nbytes,
                                              _device.stream_ptr()), "geo_knn_thresholds")
        return {"tau": tau}, "thresholds"

    out = _four_runs(monkeypatch, call, _t(latents(n, d, 2)), _t(latents(n, d, 1)), "thresholds")
    assert bool((out["tau"] >= 0).all()) and bool(torch.isfinite(out["tau"]).all())


@pytest.mark.parametrize("n,d,m,kq,path", [(500, 5, 200, 10, EXACT), (16384, 64, 200, 10, BF16)], ids=["exact", "filter_bf16"])
def test_knn_query(n, d, m, kq, path, monkeypatch):
    """geo_knn_query: without the filter, and at the smallest corpus where the filter applies (d = 64)."""
    from vqvae_amd import _lib
    from vqvae_amd.geo.knn_graph_optimized import knn_query_device

    def call(inp):
        idx, d2 = knn_query_device(inp[0], inp[1], kq)
        return {"idx": idx, "d2": d2}, _lib.load().geo_knn_last_path()

    out = _four_runs(monkeypatch, call, (_t(latents(n, d, 2)), _t(latents(m, d, 4))), (_t(latents(n, d, 1)), _t(latents(m, d, 3))), path)
    assert out["idx"].shape == (m, kq) and bool((out["d2"][:, 1:] >= out["d2"][:, :-1]).all())


# --------------------------------------------------------------------------------------------- shortest paths and seeding
SSSP_DEFAULTS = {"sssp_sb": -1, "sssp_push": 1, "sssp_delta": 8, "sssp_u32": 1, "sssp_group": 1, "sssp_push_blocks": 64,
                 "sssp_order": 0}


def _edge_weights(W, p, v):
    """w(p[i] -> v[i]) of a canonical symmetric CSR, looked up by binary search; every pair must be a stored entry."""
    n = W.shape[0]
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(W.indptr)) * n + W.indices
    q = p.astype(np.int64) * n + v
    pos = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
    assert np.array_equal(keys[pos], q), "a predecessor is not a neighbour"
    return W.data[pos].astype(np.float64)


def _same_tree_distances(W, D, P, P_want):
    """The rule of test_gpu_sssp.py: ties between equal-length paths may pick another parent, every parent is tight."""
    D, P, P_want = (x.cpu().numpy() for x in (D, P, P_want))
    assert np.array_equal(P < 0, P_want < 0)
    rows, cols = np.nonzero(np.isfinite(D) & (P >= 0))
    par = P[rows, cols]
    assert par.max(initial=0) < W.shape[0]
    d_v = D[rows, cols].astype(np.float64)
    assert np.all(np.abs(D[rows, par].astype(np.float64) + _edge_weights(W, par, cols) - d_v) <= 1e-5 * (1 + d_v))


def _wide_weights(W):
    """test_fixed_point_solve_declines_and_falls_back: every 7th weight scaled by 1e-4 -- more than 28 bits of units."""
    Wide = W.copy()
    Wide.data = (Wide.data * np.where(np.arange(Wide.nnz) % 7 == 0, 1e-4, 1.0)).astype(np.float32)
    Wide = Wide.maximum(Wide.T).tocsr()
    Wide.sort_indices()
    return Wide


# name: (graph, n_sources, options, geo_sssp_plan's answer, layout the call reports)
SSSP_CASES = {
    "plain_16_sources": (lambda: _knn_graph("gauss", 2000, 16, 7, 8), 5, {}, 16, 16),
    "plain_64_sources": (lambda: _knn_graph("gauss", 2000, 16, 7, 8), 65, {}, 64, 64),
    "chunked_fixed_point": (lambda: _knn_graph("gauss", 12289, 16, 11, 10), 40, {}, 3016, 2032),
    "chunked_fp64": (lambda: _knn_graph("gauss", 12289, 16, 11, 10), 40, {"sssp_u32": 0}, 1016, 1016),
    "near_far_push_forced": (lambda: _knn_graph("gauss", 12289, 16, 11, 10), 40,
                             {"sssp_sb": 16, "sssp_push": 2, "sssp_delta": 4, "sssp_order": 1, "sssp_group": 2}, 3016, 4016),
    "fixed_point_declines": (lambda: _wide_weights(_knn_graph("gauss", 20011, 16, 11, 10)), 48, {}, 3016, 1016),
    # long geodesics, the sources ordered by graph cells (order_by_cells keeps its labels in the landmark distances' buffer)
    "ordered_by_cells_then_push": (lambda: _knn_graph("swiss", 14000, 16, 3, 10), 40, {"sssp_order": 1, "sssp_group": 2},
                                   3016, 4016),
}


def test_chunked_layout_starts_just_above_12288_nodes():
    from vqvae_amd import _lib
    lib = _lib.load()
    assert lib.geo_sssp_plan(12288, 40) == 64 and lib.geo_sssp_plan(12289, 40) == 3016


@pytest.mark.parametrize("name", list(SSSP_CASES))
def test_sssp_multi(name, monkeypatch, request):
    from vqvae_amd import _lib
    from vqvae_amd.geo.geo_shortest_paths import sssp_multi_device
    make, S, opts, plan, layout = SSSP_CASES[name]
    lib = _lib.load()
    W = make()
    n = W.shape[0]
    _options(request, SSSP_DEFAULTS, **opts)
    assert lib.geo_sssp_plan(n, S) == plan
    src = np.random.RandomState(S).choice(n, S, replace=False).astype(np.int32)
    src[-1] = src[0]                                                    # a duplicate source: ties in the argmin
    WA, perm = _relabel(W, 9)

    def call(inp):
        Wg, G, s = inp
        D, P, dmin, amin, _ = sssp_multi_device(G, s, want_D=True, want_P=True, want_min=True)
        return {"D": D, "P": (Wg, D, P), "dmin": dmin, "argmin": amin}, lib.geo_sssp_last_profile(None, None)

    def compare(key, got, want):
        if key == "P":
            _same_tree_distances(got[0], got[1], got[2], want[2])
        return key == "P"

    out = _four_runs(monkeypatch, call, (WA, _device_csr(WA), _t(perm[src].astype(np.int32))), (W, _device_csr(W), _t(src)),
                     layout, compare)
    assert out["D"].shape == (S, n) and bool(torch.isfinite(out["D"]).all())


def _nearest_inputs(declined):
    """The first and the last graph of test_nearest_source_in_one_solve_equals_the_k_source_solve_and_the_oracle."""
    r = np.random.RandomState(11)
    W = _knn_graph("gauss", 6000, 16, 3, 10).astype(np.float32)
    src = r.choice(6000, 200, replace=False)
    src[17] = src[3]
    if declined:                                                        # weights over 12 binades
        W = W.copy()
        W.data = (W.data * np.exp2(r.randint(0, 12, W.nnz))).astype(np.float32)
        W = W.maximum(W.T).tocsr()
        W.sort_indices()
    return W, src.astype(np.int32)


@pytest.mark.parametrize("declined", [False, True], ids=["answered", "declined_to_the_k_source_solve"])
def test_nearest_source(declined, monkeypatch):
    from vqvae_amd.geo.geo_shortest_paths import nearest_source_device
    W, src = _nearest_inputs(declined)
    WA, perm = _relabel(W, 12)

    def call(inp):
        G, s = inp
        info = {}
        dmin, amin, _ = nearest_source_device(G, s, info=info)
        return {"dmin": dmin, "argmin": amin, "suspects": info["suspects"]}, (info["declined"], info["reason"])

    out = _four_runs(monkeypatch, call, (_device_csr(WA), _t(perm[src].astype(np.int32))), (_device_csr(W), _t(src)),
                     (True, 1) if declined else (False, 0))
    assert not bool((out["argmin"] == 17).any())                        # the repeated medoid: the lower row owns the cell


def _kpp_log_modes(log):
    """[(first iteration, mode, centres handed back / sweeps used)] of the chain's library calls."""
    return [(int(m.group(1)), m.group(2), int(m.group(3)))
            for m in re.finditer(r"\[kpp-log\] it (\d+)\.\.\d+ mode (\S+) -> abort -?\d+ reason \d+ used (\d+)", log)]


def _fit(km, W, K, seed, capfd):
    capfd.readouterr()
    km._KNOBS["log"] = True
    try:
        med, assign, qe = km.fit_kmedoids_optimized(W, K=K, init="kpp", seed=seed)
    finally:
        km._KNOBS["log"] = False
    return {"medoids": med, "assign": assign, "qe": np.float64(qe)}, _kpp_log_modes(capfd.readouterr().err)


@pytest.mark.parametrize("host_draw", [False, True], ids=["budgeted_chain", "host_draw_single_update"])
def test_kpp_fit_on_two_components(host_draw, monkeypatch, capfd, request):
    """The 700 + 900 graph of test_chain_stays_budgeted_while_a_component_is_unreached, seed 1 (centre 3 is the first in the
    other component).  Default: the chain stays budgeted while d_min has inf entries.  GEO_KPP_HOST_DRAW=1: one
    geo_sssp_single_update per centre."""
    from vqvae_amd.geo import kmeans_optimized as km
    parts = [_knn_graph("gauss", n, 8, s, 6) for n, s in ((700, 21), (900, 22))]
    W = sparse.block_diag(parts, format="csr", dtype=np.float32)
    W.sort_indices()
    WA, _ = _relabel(W, 13)
    K = 24
    saved = dict(km._KNOBS)
    request.addfinalizer(lambda: km._KNOBS.update(saved))
    absorbed = []
    absorb = km._Chain.absorb
    monkeypatch.setattr(km._Chain, "absorb", lambda self, source, pos: (absorbed.append(pos), absorb(self, source, pos))[1])
    if host_draw:
        monkeypatch.setenv("GEO_KPP_HOST_DRAW", "1")

    def call(Wg):
        del absorbed[:]
        out, modes = _fit(km, Wg, K, 1, capfd)
        if host_draw:
            return out, ("single_update", len(absorbed), len(modes))
        early = [mode for it0, mode, _ in modes if it0 <= 3]
        return out, ("budgeted", bool(early) and all(mode.isdigit() for mode in early), len(absorbed))

    out = _four_runs(monkeypatch, call, WA, W, ("single_update", K, 0) if host_draw else ("budgeted", True, 0))
    assert len(set(out["medoids"].tolist())) == K and np.isfinite(out["qe"])


KPP_KNOBS = {"step": {"resident": False}, "resident": {"resident": True, "resident_from": 16},
             "resident_early": {"resident": True, "resident_from": 1}}


@pytest.mark.parametrize("knobs", list(KPP_KNOBS))
def test_kpp_fit_on_the_swiss_roll(knobs, monkeypatch, capfd, request):
    """The 6 000-node swiss-roll graph of test_resident_chain_equals_step_kernel_and_oracle, K = 64: the step kernel alone, the
    resident workgroup from centre 16, and from centre 1 -- where the first cells outgrow its table and are handed back."""
    from vqvae_amd.geo import kmeans_optimized as km
    W = _knn_graph("swiss", 6000, 16, 3, 8)
    WA, _ = _relabel(W, 14)
    saved = dict(km._KNOBS)
    request.addfinalizer(lambda: km._KNOBS.update(saved))
    km._KNOBS.update(KPP_KNOBS[knobs])

    def call(Wg):
        out, modes = _fit(km, Wg, 64, 1, capfd)
        resident = [(it0, used) for it0, mode, used in modes if mode == "resident"]
        if knobs == "step":
            return out, ("step", any(mode == "step" for _, mode, _ in modes), len(resident))
        # (the chain enters the resident kernel at `resident_from`; a declined draw may re-enter it later)
        return out, ("resident", resident[0][0] if resident else None, knobs == "resident_early" and
                     sum(used for _, used in resident) > 0)

    route = {"step": ("step", True, 0), "resident": ("resident", 16, False), "resident_early": ("resident", 1, True)}[knobs]
    out = _four_runs(monkeypatch, call, WA, W, route)
    assert len(set(out["medoids"].tolist())) == 64


# ---------------------------------------------------------------------------------------------- spatial-decoder pull-back
STATS = ("rm1", "rv1", "rm2", "rv2")
CHANNELS = (256, 128, 64)


def _decoder_factory(norm, train, d, cout, size):
    """A fresh default decoder (256, 128, 64) per call: train-mode BatchNorm folds its running statistics into the module."""
    from oracle import metric as om
    from vqvae_amd.spatial_decoder import SpatialDecoder
    sd = om.make_decoder_state(5, d, cout, CHANNELS, norm_type=norm)

    def make():
        dec = SpatialDecoder(cout, CHANNELS, d, size, norm if norm != "none" else None)
        dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        dec = dec.to(_dev())
        return dec.train() if train else dec.eval()
    return make


def _jvp_outputs(ex, L):
    out = {"lengths": L}
    out.update({k: ex.tensors[k].clone() for k in STATS if ex.tensors.get(k) is not None})
    return out


def _route(plan, head_stream):
    return (plan["front"], plan["dmax"], plan["mid"], plan["back"], plan["node_jacobian"], plan.get("front_once", False),
            bool(head_stream))


# name: (norm, train, d, out channels, size, route)
PAIR_CASES = {
    "bn_train_pipe_head_stream": ("batch", True, 16, 1, 28, ("valu", 16, "pipe", "mfma", False, False, True)),
    "no_norm": ("none", False, 16, 1, 28, ("valu", 16, "pipe", "mfma", False, False, True)),
    "group_norm": ("group", False, 16, 1, 28, ("valu", 16, "all", "mfma", False, False, False)),
    "bn_train_d40_mfma_front": ("batch", True, 40, 1, 28, ("mfma", 64, "pipe", "mfma", False, False, True)),
    "bn_train_192_output_head": ("batch", True, 16, 3, 32, ("valu", 16, "pipe", "mfma", False, False, False)),
}


@pytest.mark.parametrize("name", list(PAIR_CASES))
def test_edge_lengths_pairs(name, monkeypatch):
    """E = 1 025 at batch 512: the last chunk is one slot."""
    from vqvae_amd import _lib
    from vqvae_amd.geo.riemannian_metric import edge_lengths_device
    from vqvae_amd.spatial_decoder import DecoderExport
    norm, train, d, cout, size, route = PAIR_CASES[name]
    make = _decoder_factory(norm, train, d, cout, size)
    lib = _lib.load()
    E, bs = 1025, 512

    def inputs(seed):
        r = np.random.RandomState(seed)
        return _t(r.randn(E, d).astype(np.float32)), _t(r.randn(E, d).astype(np.float32))

    def call(inp):
        ex = DecoderExport(make(), _dev())
        code = lib.geo_jvp_plan(ex.desc, 0, E, bs, 0, 0)
        assert code >= 0, lib.geo_last_error()
        L = edge_lengths_device(ex, inp[0], inp[1], bs)
        return _jvp_outputs(ex, L), _route(_lib.decode_jvp_plan(code), lib.geo_jvp_head_stream(ex.desc, 0, E, bs, 0))

    out = _four_runs(monkeypatch, call, inputs(2), inputs(1), route)
    assert bool(torch.isfinite(out["lengths"]).all()) and float(out["lengths"].min()) > 0


def _edge_list(kind, n_nodes, n_edges, seed):
    from test_gpu_jvp_start_dedup import _graph
    src, dst = _graph(kind, n_nodes, n_edges, seed)
    return _t(src), _t(dst)


# name: (norm, train, d, out channels, size, graph kind, nodes, edges of the call, build_edges, route)
GRAPH_CASES = {
    "bn_train_dedup_front_once_head_stream": ("batch", True, 16, 1, 28, "mixed", 3000, 5001, None,
                                              ("valu", 16, "pipe_dedup", "dedup", False, True, True)),
    "bn_train_d24_dedup_mfma_front": ("batch", True, 24, 1, 28, "mixed", 3000, 5001, None,
                                      ("mfma", 32, "pipe_dedup", "dedup", False, False, True)),
    "bn_train_192_output_head": ("batch", True, 16, 3, 32, "mixed", 3000, 5001, None,
                                 ("valu", 16, "pipe_dedup", "dedup", False, True, False)),
    "bn_eval_node_jacobian": ("batch", False, 16, 1, 28, "shuffled", 96, 1536, None,
                              ("valu", 16, "all_tangent", "per_node", True, False, False)),
    "bn_eval_per_node": ("batch", False, 16, 1, 28, "distinct", 3000, 3000, None,
                         ("valu", 16, "all_tangent", "per_node", False, False, False)),
    "group_norm_per_node": ("group", False, 16, 1, 28, "distinct", 3000, 3000, None,
                            ("valu", 16, "all_tangent", "per_node", False, False, False)),
    "bn_eval_part_of_a_build": ("batch", False, 16, 1, 28, "shuffled", 96, 700, 1536,
                                ("valu", 16, "all_tangent", "per_node", True, False, False)),
}


@pytest.mark.parametrize("name", list(GRAPH_CASES))
def test_edge_lengths_graph(name, monkeypatch):
    from vqvae_amd import _lib
    from vqvae_amd.geo.riemannian_metric import edge_lengths_graph_device
    from vqvae_amd.spatial_decoder import DecoderExport
    norm, train, d, cout, size, kind, N, E, build, route = GRAPH_CASES[name]
    make = _decoder_factory(norm, train, d, cout, size)
    lib = _lib.load()
    bs = 512

    def inputs(seed):
        src, dst = _edge_list(kind, N, build or E, seed)
        return _t(np.random.RandomState(seed).randn(N, d).astype(np.float32)), src[:E].contiguous(), dst[:E].contiguous()

    def call(inp):
        z, src, dst = inp
        ex = DecoderExport(make(), _dev())
        code = lib.geo_jvp_plan_part(ex.desc, N, E, build or E, bs, 1, 0)
        assert code >= 0, lib.geo_last_error()
        L = edge_lengths_graph_device(ex, z, src, dst, bs, build_edges=build)
        return _jvp_outputs(ex, L), _route(_lib.decode_jvp_plan(code), lib.geo_jvp_head_stream(ex.desc, N, E, bs, 1))

    out = _four_runs(monkeypatch, call, inputs(12), inputs(11), route)
    assert out["lengths"].numel() == E and bool(torch.isfinite(out["lengths"]).all())


# ------------------------------------------------------------------------------------------------ distance-feature PCA
def _feature_matrix(K, n, seed):
    """The matrix of test_feature_moments_inf_handling_and_tiles: 30 % inf, a row with nothing finite but one 0, NaN and -inf."""
    r = np.random.RandomState(seed)
    D = np.abs(r.randn(K, n)).astype(np.float32) * 3
    D[r.rand(K, n) < 0.3] = np.inf
    D[5] = np.inf
    D[5, 17] = 0.0
    D[6, 100:200] = np.nan
    D[7, 3] = -np.inf
    for k in (9, K // 2 + 12):
        D[k] = np.abs(r.randn(n)).astype(np.float32)
    return D


@pytest.mark.parametrize("K,n", [(130, 9001), (65, 40000)], ids=["K130_n9001", "K65_n40000_three_statistics_slices"])
def test_feature_moments(K, n, monkeypatch):
    """K = 65, n = 40 000: three 16 384-column statistics slices and a partial second tile -- also against the fp64 restatement,
    with the bounds of test_feature_moments_inf_handling_and_tiles."""
    import kmedoids_analysis_cases as C
    from vqvae_amd.geo.analysis import feature_moments_device

    def call(D):
        colmax, fill, mean, gram = feature_moments_device(D)
        return {"colmax": colmax, "fill": fill, "mean": mean, "gram": gram}, "moments"

    D = _feature_matrix(K, n, 11)
    out = {k: v.cpu().numpy() for k, v in _four_runs(monkeypatch, call, _t(_feature_matrix(K, n, 12)), _t(D), "moments").items()}
    want_max = np.where(np.isfinite(D), D, -np.inf).max(axis=1)
    assert np.array_equal(out["colmax"], want_max) and out["colmax"][5] == 0.0 and out["fill"][5] == np.float32(1.1)
    if n == 40000:
        X = C.replaced_features(D).astype(np.float64)
        np.testing.assert_allclose(out["mean"], X.mean(axis=0), rtol=n * 2.0 ** -53, atol=0)
        Xc = X - X.mean(axis=0)
        G = Xc.T @ Xc
        scale = np.sqrt(np.outer(np.diag(G), np.diag(G)))
        err = np.abs(out["gram"] - G) / scale
        print(f"K={K} n={n}: gram error / scale max {err.max():.3e}, bound {4 * n * 2.0 ** -53:.3e}")
        assert (np.abs(out["gram"] - G) <= 4 * n * 2.0 ** -53 * scale).all()
        assert np.array_equal(out["gram"], out["gram"].T)
