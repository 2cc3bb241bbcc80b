"""The kernels of csrc/graph.hip and the recursive scan of csrc/common.hip against scipy / numpy references
(tests/graph_cases.py) on the graphs a kNN search at small N never produces.  Integer and byte work: every comparison is
exact.  Which case reaches which path:

  compact_fill_kernel, second ballot chunk and its `base` carry    wide_rows / with_diagonal rows of 65, 128, 129 ... 300
                                                                   entries (64: the loop ends exactly on the chunk)
  upper_fill_kernel, second trip of the lane loop                  the same rows; rows 283 - 331 have the diagonal inside a
                                                                   later trip, with_diagonal stores it, one_sided has no mirror
  cc_hook_kernel / cc_jump_kernel over many rounds                 path_perm, path_desc, path_zigzag (one component of 40 000),
                                                                   forest (permuted ids, 3 000 components), star_grid (all
                                                                   leaves pulled down through the highest id)
  grid stride of cc_hook_kernel (n > 32 768)                       path_*, forest (n = 40 000)
  grid stride of init / jump / roots / number / keep flags /       huge_sparse (n = 4 194 305)
    new index (n > 524 288)
  grid stride of seg_count_kernel (n > 262 144)                    many_rows (n = 262 445)
  sym_sort_kernel on a hub (79 segments of one row)                hub; two_hubs_wide (k = 130: out part alone is three trips)
  ids outside [0, n) in the lists                                  invalid_ids (-1, n, n + 7; one row of nothing else)
  atomic cursor order of fill_in_kernel                            hub, repeated and on a side stream, bit-identical
  scan: third level, tile boundaries                               huge_sparse at n = 2048, 2049, 4 194 304, 4 194 305
                                                                   through geo_upper_edges_count / geo_csr_compact_count
"""
import functools

import numpy as np
import pytest
import torch

import graph_cases as gc

pytestmark = pytest.mark.gpu

GEO_E_ARG, GEO_E_WORKSPACE = -1, -2
SYMS = ("union", "mutual")


def dev():
    from vqvae_amd._device import device
    return device()


def host(t):
    return t.cpu().numpy()


def assert_csr_equal(G, want, err=""):
    """DeviceCSR against a scipy CSR: n, indptr, indices and data, all exact."""
    assert G.n == want.shape[0], err
    np.testing.assert_array_equal(host(G.indptr), want.indptr, err_msg=err)
    np.testing.assert_array_equal(host(G.indices), want.indices, err_msg=err)
    assert G.data.dtype == torch.float32
    np.testing.assert_array_equal(host(G.data), want.data, err_msg=err)


# ----------------------------------------------------------------------------------------------- symmetrisation
@functools.lru_cache(maxsize=None)
def lists_on_device(name):
    n, idx, w = gc.sym_lists(name)
    return n, idx, w, torch.from_numpy(idx).to(dev()), torch.from_numpy(w).to(dev())


@pytest.mark.parametrize("weighted", [True, False], ids=["weights", "ones"])
@pytest.mark.parametrize("sym", SYMS)
@pytest.mark.parametrize("name", gc.SYM_CASES)
def test_symmetrize_vs_scipy(name, sym, weighted):
    from vqvae_amd.geo.knn_graph_optimized import symmetrize_device
    n, idx, w, idx_d, w_d = lists_on_device(name)
    G = symmetrize_device(idx_d, w_d if weighted else None, sym)
    assert_csr_equal(G, gc.sym_ref(n, idx, w if weighted else None, sym), f"{name}/{sym}")


@pytest.mark.parametrize("sym", SYMS)
def test_hub_is_bit_identical_across_runs_and_streams(sym):
    """fill_in_kernel hands out the slots of row 0's 4 999 in-entries through an atomic cursor: their order differs from run
    to run, the sorted row and the weight paired with every column must not."""
    from vqvae_amd.geo.knn_graph_optimized import symmetrize_device
    n, idx, w, idx_d, w_d = lists_on_device("hub")
    want = gc.sym_ref(n, idx, w, sym)
    runs = [symmetrize_device(idx_d, w_d, sym) for _ in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runs.append(symmetrize_device(idx_d, w_d, sym))
    side.synchronize()
    for G in runs:
        assert_csr_equal(G, want, sym)
        assert torch.equal(G.indptr, runs[0].indptr) and torch.equal(G.indices, runs[0].indices)
        assert torch.equal(G.data, runs[0].data)


# ---------------------------------------------------------------------------------------------------- CSR cases
@functools.lru_cache(maxsize=None)
def graph_on_device(name):
    """(W scipy, DeviceCSR, known n_components or None, known LCC mask or None), built once per module."""
    from vqvae_amd._device import DeviceCSR
    if name == "huge_sparse":
        W, ncomp, lcc = gc.huge_sparse(gc.HUGE_N)
    else:
        W, ncomp, lcc = gc.csr_graph(name), None, None
    return W, DeviceCSR.from_scipy(W, dev()), ncomp, lcc


@functools.lru_cache(maxsize=None)
def upper_on_device(name):
    from vqvae_amd.geo.knn_graph_optimized import upper_edges_device
    return upper_edges_device(graph_on_device(name)[1])


@pytest.mark.parametrize("name", ["wide_rows", "with_diagonal", "one_sided", "huge_sparse"])
def test_upper_edges_and_gather_vs_numpy(name):
    from vqvae_amd.geo.knn_graph_optimized import reweight_device
    W, G, _, _ = graph_on_device(name)
    src, dst, entry_edge = upper_on_device(name)
    want_src, want_dst, want_ee = gc.upper_ref(W)
    np.testing.assert_array_equal(host(src), want_src)
    np.testing.assert_array_equal(host(dst), want_dst)
    np.testing.assert_array_equal(host(entry_edge), want_ee)               # -1 exactly where the reference says so
    rows = gc._rows_of(W)
    orphan = want_ee < 0
    if name in ("wide_rows", "huge_sparse"):
        assert not orphan.any()
    elif name == "with_diagonal":
        np.testing.assert_array_equal(orphan, W.indices == rows)
    else:
        assert orphan.any() and (W.indices[orphan] < rows[orphan]).all()
    lengths = np.random.RandomState(5).rand(max(1, len(want_src))).astype(np.float32) + np.float32(0.5)
    lengths[::13] = 0.0
    Wg = reweight_device(G, entry_edge, torch.from_numpy(lengths).to(dev()))
    assert Wg.indptr is G.indptr and Wg.indices is G.indices
    np.testing.assert_array_equal(host(Wg.data), np.where(orphan, np.float32(0.0), lengths[np.maximum(want_ee, 0)]))


COMPACT_VARIANTS = ("mask", "drop_zero", "both", "all", "none", "one", "structure")


@pytest.mark.parametrize("variant", COMPACT_VARIANTS)
@pytest.mark.parametrize("name", ["wide_rows", "with_diagonal", "huge_sparse"])
def test_compact_vs_numpy(name, variant):
    from vqvae_amd._device import DeviceCSR
    from vqvae_amd.geo.knn_graph_optimized import compact_device
    W, G, _, _ = graph_on_device(name)
    n = W.shape[0]
    masks = gc.masks_for(n, 11)
    random_mask = gc.huge_mask(n) if name == "huge_sparse" else masks["random"]
    mask, drop_zero = {"mask": (random_mask, False), "drop_zero": (None, True), "both": (random_mask, True),
                       "all": (masks["all"], False), "none": (masks["none"], True), "one": (masks["one"], False),
                       "structure": (random_mask, True)}[variant]
    if variant == "structure":                     # data == NULL through the ABI: nothing to drop, data_out is ones
        G = DeviceCSR(G.n, G.indptr, G.indices, None)
        W = type(W)((np.ones(W.nnz, np.float32), W.indices, W.indptr), shape=W.shape)
    want, want_index = gc.compact_ref(W, mask, drop_zero)
    got, new_index = compact_device(G, None if mask is None else torch.from_numpy(mask).to(dev()), drop_zero)
    np.testing.assert_array_equal(host(new_index), want_index)
    assert got.n == want.shape[0] and got.nnz == want.nnz
    assert_csr_equal(got, want, f"{name}/{variant}")
    if variant == "none":
        assert got.n == 0 and got.nnz == 0 and (host(new_index) == -1).all() and host(got.indptr).tolist() == [0]
    elif variant == "all":
        assert got.n == n and got.nnz == W.nnz                            # stored zeros stay without drop_zero
    elif variant == "one":
        assert got.n == 1 and int(host(new_index).max()) == 0
    elif variant == "structure":
        assert (host(got.data) == 1.0).all()
    elif drop_zero:
        assert got.nnz < W.nnz and (host(got.data) != 0).all()


@pytest.mark.parametrize("name", ["wide_rows", "with_diagonal"] + list(gc.CC_ONLY) + ["huge_sparse"])
def test_components_vs_scipy(name):
    """Labels are scipy's: components numbered by their lowest node.  geo_connected_components gives up (GEO_E_NOCONV, an
    exception here) after n + 2 hooking rounds; the permuted path needs about ten in a synchronous simulation of the rule."""
    from vqvae_amd._device import DeviceCSR
    from vqvae_amd.geo.knn_graph_optimized import connected_components_device, lcc_mask_device
    W, G, known_ncomp, known_lcc = graph_on_device(name)
    G = DeviceCSR(G.n, G.indptr, G.indices, None)
    want_ncomp, want_labels = gc.cc_ref(W)
    ncomp, labels = connected_components_device(G)
    assert labels.dtype == torch.int32
    assert ncomp == want_ncomp
    np.testing.assert_array_equal(host(labels), want_labels)
    want_lcc = gc.lcc_ref(want_ncomp, want_labels)
    np.testing.assert_array_equal(host(lcc_mask_device(G)), want_lcc)
    if known_ncomp is not None:                    # huge_sparse: known by construction, not only from scipy
        assert ncomp == known_ncomp
        np.testing.assert_array_equal(want_lcc, known_lcc)
    if name.startswith("path_"):
        assert ncomp == 1
    elif name == "forest":
        assert ncomp == gc.FOREST_COMPONENTS and int(want_lcc.sum()) == gc.FOREST_LARGEST


def test_graphs_without_an_edge():
    """k1 under `mutual` has no entry at all (no two nodes of a cycle list each other), and a graph may store nothing but
    diagonal entries: E = 0, nnz = 0.  Arrays without an element have no address; every call must still answer."""
    from vqvae_amd._device import DeviceCSR
    from vqvae_amd.geo.knn_graph_optimized import (compact_device, connected_components_device, lcc_mask_device,
                                                   reweight_device, symmetrize_device, upper_edges_device)
    n, idx, w, idx_d, w_d = lists_on_device("k1")
    assert gc.sym_ref(n, idx, w, "mutual").nnz == 0
    empty = symmetrize_device(idx_d, w_d, "mutual")
    diagonal = gc.csr_from_entries(5, [1, 3], [1, 3], [0.5, 0.0])
    for W, G in ((gc.sym_ref(n, idx, w, "mutual"), empty), (diagonal, DeviceCSR.from_scipy(diagonal, dev()))):
        assert_csr_equal(G, W)
        src, dst, entry_edge = upper_edges_device(G)
        assert src.numel() == 0 and dst.numel() == 0
        np.testing.assert_array_equal(host(entry_edge), gc.upper_ref(W)[2])
        assert bool((entry_edge == -1).all())
        Wg = reweight_device(G, entry_edge, torch.empty(0, dtype=torch.float32, device=dev()))
        assert bool((Wg.data == 0).all()) and Wg.nnz == W.nnz
        ncomp, labels = connected_components_device(G)
        assert ncomp == W.shape[0]
        np.testing.assert_array_equal(host(labels), np.arange(W.shape[0]))
        np.testing.assert_array_equal(host(lcc_mask_device(G)), gc.lcc_ref(*gc.cc_ref(W)))
        for drop_zero in (False, True):
            want, want_index = gc.compact_ref(W, None, drop_zero)
            got, new_index = compact_device(G, None, drop_zero)
            assert_csr_equal(got, want)
            np.testing.assert_array_equal(host(new_index), want_index)


# ---------------------------------------------------------------------------------------------- scan boundaries
@pytest.mark.parametrize("n", gc.HUGE_SIZES)
def test_scan_at_tile_boundaries_through_the_count_calls(n):
    """exclusive_scan_i32 is not in the ABI; its output is upper_ptr, new_index and indptr_new of the *_count calls.  One
    tile (2048), one item into the second (2049), two full levels (2048 x 2048) and one item into the third level."""
    from vqvae_amd import _lib
    from vqvae_amd._device import DeviceCSR, ptr, stream_ptr, workspace
    lib = _lib.load()
    if n == gc.HUGE_N:
        W, G, _, _ = graph_on_device("huge_sparse")
    else:
        W = gc.huge_sparse(n)[0]
        G = DeviceCSR.from_scipy(W, dev())
    rows = gc._rows_of(W)
    ws = workspace(max(lib.geo_cc_workspace_bytes(n), lib.geo_csr_compact_workspace_bytes(n)), dev())
    # upper_ptr = exclusive scan of the per-row count of columns above the diagonal
    upper_ptr = torch.full((n + 1,), -7, dtype=torch.int32, device=dev())
    n_edges = np.zeros(1, dtype=np.int64)
    _lib.check(lib.geo_upper_edges_count(ptr(G.indptr), ptr(G.indices), n, ptr(upper_ptr), n_edges.ctypes.data, ptr(ws),
                                         ws.numel(), stream_ptr()), "geo_upper_edges_count")
    want = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[W.indices > rows], minlength=n), out=want[1:])
    np.testing.assert_array_equal(host(upper_ptr), want)
    assert int(n_edges[0]) == want[-1] == W.nnz // 2
    # new_index = exclusive scan of the keep flags; indptr_new = exclusive scan of the kept rows' counts -- under a mask
    # (n_new < n items) and with every node kept (n items: the row-count scan itself reaches the level under test)
    for mask in (gc.huge_mask(n), None):
        want_csr, want_index = gc.compact_ref(W, mask, True)
        m = want_csr.shape[0]
        new_index = torch.full((n,), -7, dtype=torch.int32, device=dev())
        indptr_new = torch.full((n + 1,), -7, dtype=torch.int32, device=dev())
        n_new, nnz_new = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
        keep = None if mask is None else torch.from_numpy(mask.astype(np.uint8)).to(dev())
        _lib.check(lib.geo_csr_compact_count(ptr(G.indptr), ptr(G.indices), ptr(G.data), n, ptr(keep), 1, ptr(new_index),
                                             ptr(indptr_new), n_new.ctypes.data, nnz_new.ctypes.data, ptr(ws), ws.numel(),
                                             stream_ptr()), "geo_csr_compact_count")
        torch.cuda.synchronize()
        assert int(n_new[0]) == m and int(nnz_new[0]) == want_csr.nnz
        np.testing.assert_array_equal(host(new_index), want_index)
        np.testing.assert_array_equal(host(indptr_new[:m + 1]), want_csr.indptr)
        assert bool((indptr_new[m + 1:] == -7).all())                      # nothing written past the total


# ---------------------------------------------------------------------------------------------- argument checks
def test_bad_arguments_are_errors_before_any_launch():
    from vqvae_amd import _lib
    from vqvae_amd._device import DeviceCSR, ptr, stream_ptr
    lib = _lib.load()
    n, k = 100, 4
    idx_d = torch.from_numpy(gc._distinct_columns(np.random.RandomState(1), n, k)).to(dev())
    need = int(lib.geo_symmetrize_workspace_bytes(n, k))
    ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=dev())
    indptr = torch.full((n + 1,), -7, dtype=torch.int32, device=dev())
    out_i = torch.full((2 * n * k,), -7, dtype=torch.int32, device=dev())
    out_f = torch.full((2 * n * k,), -7.0, dtype=torch.float32, device=dev())
    nnz = np.full(1, -7, dtype=np.int64)

    def count(n=n, k=k, mode=0, ws_bytes=need):
        return lib.geo_symmetrize_count(ptr(idx_d), None, n, k, mode, ptr(indptr), nnz.ctypes.data, ptr(ws), ws_bytes,
                                        stream_ptr())

    def fill(n=n, k=k, mode=0, ws_bytes=need):
        return lib.geo_symmetrize_fill(ptr(idx_d), None, n, k, mode, ptr(indptr), ptr(out_i), ptr(out_f), ptr(ws), ws_bytes,
                                       stream_ptr())

    for call in (count, fill):
        for kw in (dict(n=1 << 20, k=1 << 10), dict(n=1 << 30, k=1), dict(k=0), dict(n=0), dict(mode=2), dict(mode=-1)):
            assert call(**kw) == GEO_E_ARG, (call.__name__, kw)
            assert call.__name__.encode() in lib.geo_last_error()
        assert call(ws_bytes=need - 1) == GEO_E_WORKSPACE
        assert b"workspace" in lib.geo_last_error() and call.__name__.encode() in lib.geo_last_error()
    with pytest.raises(_lib.GeoHipError, match="geo_symmetrize_count"):
        _lib.check(count(mode=2), "geo_symmetrize_count")

    # components and compaction: a workspace one byte short of their query
    W = gc.csr_graph("wide_rows")
    G = DeviceCSR.from_scipy(W, dev())
    labels = torch.full((G.n + 1,), -7, dtype=torch.int32, device=dev())
    new_index = torch.full((G.n + 1,), -7, dtype=torch.int32, device=dev())
    ncomp, n_new = np.full(1, -7, dtype=np.int32), np.full(1, -7, dtype=np.int32)
    need_cc, need_compact = int(lib.geo_cc_workspace_bytes(G.n)), int(lib.geo_csr_compact_workspace_bytes(G.n))
    assert max(need_cc, need_compact) <= ws.numel()

    def components(ws_bytes):
        return lib.geo_connected_components(ptr(G.indptr), ptr(G.indices), G.n, ptr(labels), ncomp.ctypes.data, ptr(ws),
                                            ws_bytes, stream_ptr())

    def compact_count(ws_bytes):
        return lib.geo_csr_compact_count(ptr(G.indptr), ptr(G.indices), ptr(G.data), G.n, None, 1, ptr(new_index),
                                         ptr(indptr), n_new.ctypes.data, nnz.ctypes.data, ptr(ws), ws_bytes, stream_ptr())

    upper_ptr = torch.full((G.n + 1,), -7, dtype=torch.int32, device=dev())
    n_edges = np.full(1, -7, dtype=np.int64)

    def upper_count(ws_bytes):                     # no size query of its own: geo_cc_workspace_bytes sizes it
        return lib.geo_upper_edges_count(ptr(G.indptr), ptr(G.indices), G.n, ptr(upper_ptr), n_edges.ctypes.data, ptr(ws),
                                         ws_bytes, stream_ptr())

    assert components(need_cc - 1) == GEO_E_WORKSPACE and b"geo_connected_components" in lib.geo_last_error()
    assert upper_count(need_cc - 1) == GEO_E_WORKSPACE and b"geo_upper_edges_count" in lib.geo_last_error()
    assert compact_count(need_compact - 1) == GEO_E_WORKSPACE and b"geo_csr_compact_count" in lib.geo_last_error()

    torch.cuda.synchronize()                       # no launch: no output, no scratch byte and no host result was touched
    assert bool((ws == 0x5A).all()) and bool((indptr == -7).all()) and bool((out_i == -7).all())
    assert bool((out_f == -7.0).all()) and bool((labels == -7).all()) and bool((new_index == -7).all())
    assert nnz[0] == -7 and ncomp[0] == -7 and n_new[0] == -7 and n_edges[0] == -7 and bool((upper_ptr == -7).all())

    # and the same calls with the workspace the queries ask for go through
    assert count() == 0 and int(nnz[0]) > 0
    assert components(need_cc) == 0 and int(ncomp[0]) == gc.cc_ref(W)[0]
    assert upper_count(need_cc) == 0 and int(n_edges[0]) == W.nnz // 2
    assert compact_count(need_compact) == 0 and int(n_new[0]) == G.n
