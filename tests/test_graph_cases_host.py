"""The references and the cases of tests/graph_cases.py, pinned on the CPU: the references against the oracle's independent
restatements, and every case against the property it exists for -- so that test_gpu_graph_kernels.py cannot degenerate into
tame graphs unnoticed.  These are conditions on the committed seeds, not measurements."""
import numpy as np
import pytest
from scipy import sparse

import graph_cases as gc
from conftest import latents


def assert_same_csr(got, want):
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.indptr, want.indptr)
    np.testing.assert_array_equal(got.indices, want.indices)
    np.testing.assert_array_equal(got.data, want.data)
    assert got.data.dtype == np.float32


# ------------------------------------------------------------------------------------------ references vs the oracle
@pytest.mark.parametrize("N,d,k", [(500, 16, 6), (300, 8, 20), (65, 3, 1)])
def test_sym_ref_equals_the_oracle_on_real_knn_lists(N, d, k):
    from oracle import knn as okn
    dist, idx = okn.drop_self(*okn.knn_search(latents(N, d, N + k), k + 1))
    w = dist.astype(np.float32)
    for sym in ("union", "mutual"):
        for weights in (w, None):
            want = okn.symmetrise(N, idx, np.ones_like(w) if weights is None else weights, sym)
            want.sort_indices()
            assert_same_csr(gc.sym_ref(N, idx.astype(np.int32), weights, sym), want)


@pytest.fixture(scope="module")
def oracle_graph():
    """The graph of test_upper_edges_and_reweight_vs_oracle (500 latents, k = 6, union, connectivity)."""
    from oracle import knn as okn
    W, _ = okn.build_knn_graph(latents(500, 16, 9), k=6, mode="connectivity", sym="union")
    W = sparse.csr_matrix(W, dtype=np.float32)
    W.sort_indices()
    return W


def test_upper_ref_and_compact_ref_equal_the_oracle(oracle_graph):
    from oracle import pipeline as op
    W = oracle_graph
    src, dst, entry_edge = gc.upper_ref(W)
    edges = op.upper_edges(W)
    np.testing.assert_array_equal(src, edges[:, 0])
    np.testing.assert_array_equal(dst, edges[:, 1])
    assert (entry_edge >= 0).all()                                   # symmetric, no diagonal: every entry has its edge
    lengths = np.random.RandomState(0).rand(len(edges)).astype(np.float32)
    lengths[::17] = 0.0
    Wg = sparse.csr_matrix((lengths[entry_edge], W.indices, W.indptr), shape=W.shape)     # U + U^T as a gather
    want = op.reweighted_graph(500, edges, lengths)
    want.sort_indices()
    want.eliminate_zeros()
    got, new_index = gc.compact_ref(Wg, None, True)
    assert_same_csr(got, want)
    np.testing.assert_array_equal(new_index, np.arange(500))
    mask = np.random.RandomState(1).rand(500) > 0.3
    wantm = want[mask][:, mask]
    wantm.sort_indices()
    gotm, new_index = gc.compact_ref(got, mask, False)
    assert_same_csr(gotm, wantm)
    np.testing.assert_array_equal(new_index[mask], np.arange(mask.sum()))
    assert (new_index[~mask] == -1).all()
    # stored zeros stay without drop_zero, and the mask and drop_zero together are the two steps one after the other
    kept, _ = gc.compact_ref(Wg, mask, False)
    assert kept.nnz > gotm.nnz and (kept.data == 0).sum() == kept.nnz - gotm.nnz
    both, _ = gc.compact_ref(Wg, mask, True)
    assert_same_csr(both, gotm)


def test_cc_ref_equals_the_oracle_and_numbers_by_lowest_node(oracle_graph):
    from oracle import knn as okn
    Wm, _ = okn.build_knn_graph(latents(240, 12, 1), k=1, mode="distance", sym="mutual")
    for W in (oracle_graph, sparse.csr_matrix(Wm), gc.csr_graph("forest")):
        ncomp, labels = gc.cc_ref(W)
        no, lo = okn.connected_components(W)
        assert ncomp == no
        np.testing.assert_array_equal(labels, lo)
        first = np.full(ncomp, W.shape[0])
        np.minimum.at(first, labels, np.arange(W.shape[0]))
        assert (np.diff(first) > 0).all()                            # component c's lowest node precedes c + 1's


# ---------------------------------------------------------------------------------------------------- list cases
def test_list_cases_are_valid_and_distinct():
    for name in gc.SYM_CASES:
        n, idx, w = gc.sym_lists(name)
        assert idx.dtype == np.int32 and w.dtype == np.float32 and idx.shape == w.shape == (n, idx.shape[1])
        valid = (idx >= 0) & (idx < n)
        s = np.sort(np.where(valid, idx, -1 - np.arange(idx.shape[1])[None, :]), axis=1)
        assert (s[:, 1:] != s[:, :-1]).all(), name                   # no column twice in a list (scipy would sum them)
        pos = w[w != 0]
        assert np.unique(pos).shape[0] == pos.shape[0], name         # a wrong pairing shows
        if name != "invalid_ids":
            assert valid.all(), name
        if name != "self_and_zero":
            assert (idx != np.arange(n)[:, None]).all() and (w > 0).all(), name


def test_hub_rows():
    n, idx, w = gc.sym_lists("hub")
    assert (n, idx.shape[1]) == (5000, 3) and (idx[1:] == 0).any(axis=1).all() and 0 not in idx[0]
    union = gc.sym_ref(n, idx, w, "union")
    assert np.diff(union.indptr)[0] >= 4999                          # 79 sort segments of 64
    assert np.diff(gc.sym_ref(n, idx, w, "mutual").indptr)[0] == 3
    n, idx, w = gc.sym_lists("two_hubs_wide")
    assert idx.shape == (1500, 130)
    deg = np.diff(gc.sym_ref(n, idx, w, "union").indptr)
    assert deg[0] == deg[1] == 1499 and deg[2:].min() > 130


def test_invalid_ids_case():
    n, idx, _ = gc.sym_lists("invalid_ids")
    bad = (idx < 0) | (idx >= n)
    assert bad.mean() > 0.15 and bad.all(axis=1).sum() >= 1
    assert {int(v) for v in np.unique(idx[bad])} == {-1, n, n + 7}
    assert bad.any(axis=1).sum() > n // 2 and (~bad).any(axis=1).sum() > n // 2


def test_self_and_zero_case():
    n, idx, w = gc.sym_lists("self_and_zero")
    me = np.arange(n)[:, None]
    assert (idx == me).any(axis=1).sum() >= 20 and (w == 0).sum() >= 50
    a, b = 10, 20
    assert w[a][idx[a] == b] == 0.0 and w[b][idx[b] == a] > 0
    union, mutual = gc.sym_ref(n, idx, w, "union"), gc.sym_ref(n, idx, w, "mutual")
    assert union[a, b] == union[b, a] == w[b][idx[b] == a] and mutual[a, b] == 0
    assert union.diagonal().sum() == 0 and (union.data != 0).all()
    # a zero weight that is the only entry of its pair vanishes from the union
    rows = np.repeat(np.arange(n), idx.shape[1])
    A = sparse.csr_matrix((np.ones(idx.size), (rows, idx.ravel())), shape=(n, n))
    pattern = ((A + A.T) != 0).sum() - ((A + A.T).diagonal() != 0).sum()
    assert union.nnz < pattern


def test_many_rows_and_k1_cases():
    n, idx, _ = gc.sym_lists("many_rows")
    assert n > 262144 and idx.shape == (n, 2)                         # seg_count_kernel: 1024 blocks x 256 threads
    n, idx, _ = gc.sym_lists("k1")
    assert idx.shape == (65, 1)
    v, seen = 0, set()
    while v not in seen:
        seen.add(v)
        v = int(idx[v, 0])
    assert len(seen) == 65 and v == 0                                 # one cycle through every node


# ----------------------------------------------------------------------------------------------------- CSR cases
def is_symmetric(W):
    """Values and stored pattern (a stored zero counts as stored)."""
    P = sparse.csr_matrix((np.ones(W.nnz), W.indices, W.indptr), shape=W.shape)
    return abs(W - W.T).nnz == 0 and (P != P.T).nnz == 0


@pytest.mark.parametrize("name", gc.CSR_SMALL + gc.CC_ONLY)
def test_csr_cases_are_canonical(name):
    W = gc.csr_graph(name)
    assert W.indptr.dtype == np.int32 and W.indices.dtype == np.int32 and W.data.dtype == np.float32
    rows = gc._rows_of(W)
    key = rows * W.shape[0] + W.indices
    assert (np.diff(key) > 0).all()                                   # sorted rows, no entry twice
    assert (W.data == 0).sum() > 0 and (W.data != 0).sum() > 0        # stored zeros are planted and kept
    assert is_symmetric(W) == (name != "one_sided")


def test_wide_rows_case():
    W = gc.csr_graph("wide_rows")
    deg = np.diff(W.indptr)
    assert W.shape == (600, 600) and deg.max() == 300
    for want in (0, 64, 65, 128, 129):
        assert (deg == want).any(), want
    assert (deg == 0).sum() == 3 and deg[0] == 0 and deg[-1] == 0
    for row, want in gc.WIDE_DEGREES.items():
        assert deg[row] == want
    assert W.diagonal().sum() == 0 and (W.indices == gc._rows_of(W)).sum() == 0
    # rows that start above and below the diagonal in their second 64-entry trip (upper_fill_kernel's lane loop)
    upper = np.bincount(gc._rows_of(W)[W.indices > gc._rows_of(W)], minlength=600)
    assert ((upper > 64) & (deg - upper > 64)).any()


def test_with_diagonal_and_one_sided_cases():
    W, D, S = gc.csr_graph("wide_rows"), gc.csr_graph("with_diagonal"), gc.csr_graph("one_sided")
    diag = D.indices == gc._rows_of(D)
    assert diag.sum() == 60 and D.nnz == W.nnz + 60 and np.diff(D.indptr)[0] == 1
    assert (D.data[diag] == 0).any() and (D.data[diag] != 0).any()
    _, _, ee = gc.upper_ref(D)
    np.testing.assert_array_equal(ee < 0, diag)                       # -1 exactly on the diagonal
    assert S.nnz == W.nnz - 20
    src, dst, ee = gc.upper_ref(S)
    lower_orphans = int((ee < 0).sum())
    upper_orphans = len(src) - int(((ee >= 0) & (S.indices < gc._rows_of(S))).sum())
    assert lower_orphans + upper_orphans == 20 and lower_orphans > 0 and upper_orphans > 0


@pytest.mark.parametrize("name", ["path_perm", "path_desc", "path_zigzag"])
def test_path_cases(name):
    W = gc.csr_graph(name)
    n = W.shape[0]
    deg = np.diff(W.indptr)
    assert n == 40000 > 32768 and W.nnz == 2 * (n - 1) and (deg == 1).sum() == 2 and deg.max() == 2
    ncomp, labels = gc.cc_ref(W)
    assert ncomp == 1 and (labels == 0).all()
    step = np.abs(W.indices - gc._rows_of(W))
    if name == "path_desc":
        assert (step == 1).all()
    elif name == "path_zigzag":
        assert n - 1 in W.indices[W.indptr[0]:W.indptr[1]] and step.max() == n - 1
    else:
        assert np.median(step) > n // 8                               # ids along the path are in no order


def test_forest_case():
    W = gc.csr_graph("forest")
    ncomp, labels = gc.cc_ref(W)
    sizes = np.bincount(labels)
    assert W.shape[0] == 40000 and ncomp == 3000 and sizes.max() >= 2000 and sizes.min() == 1
    assert W.nnz == 2 * (40000 - 3000)                                # trees
    # a component's lowest node is not where any ordered visit meets it first: the ids are permuted
    big = np.nonzero(labels == np.argmax(sizes))[0]
    assert np.diff(W.indptr)[big].max() == 2 and big.max() - big.min() > 30000
    assert gc.lcc_ref(ncomp, labels).sum() == sizes.max()


def test_star_grid_case():
    W = gc.csr_graph("star_grid")
    n = W.shape[0]
    deg = np.diff(W.indptr)
    assert n == 15001 and deg[n - 1] == 5000 and int(np.argmax(deg)) == n - 1
    ncomp, labels = gc.cc_ref(W)
    sizes = np.bincount(labels)
    assert ncomp == 2 and sorted(sizes) == [5001, 10000]
    assert (deg[labels == labels[n - 1]] == 1).sum() == 5000            # every leaf hangs on the highest id alone


# --------------------------------------------------------------------------------------------------- huge_sparse
@pytest.fixture(scope="module")
def huge():
    return gc.huge_sparse(gc.HUGE_N)


def test_huge_sparse_reaches_the_third_scan_level_and_no_tile_sum_is_constant(huge):
    W, ncomp, lcc = huge
    n = W.shape[0]
    assert n == 2048 * 2048 + 1 and gc.HUGE_SIZES == (2048, 2049, 4194304, 4194305)
    assert n > 524288                                                 # every 2048-block grid of graph.hip strides
    deg = np.diff(W.indptr)
    assert deg.min() == 0 and deg.max() == 3 and np.bincount(deg).min() > n // 50
    assert 0.8 * n < W.nnz < 1.6 * n
    upper = np.bincount(gc._rows_of(W)[W.indices > gc._rows_of(W)], minlength=n)
    mask = gc.huge_mask(n)
    kept_rows, _ = gc.compact_ref(W, mask, True)
    nonzero_rows, _ = gc.compact_ref(W, None, True)
    # scanned over all n rows (three levels): symmetric row counts, upper counts, keep flags, row counts without stored zeros
    for counts in (deg, upper, mask.astype(np.int64), np.diff(nonzero_rows.indptr)):
        assert counts.shape[0] == n
        level1, level2 = check_tiles(counts)
        assert len(level1) == 2049 and len(level2) == 2
        assert np.unique(level2).shape[0] > 1
    # the row counts under the mask are scanned over the kept rows only: two levels at this size
    kept = np.diff(kept_rows.indptr)
    assert 2048 < kept.shape[0] == mask.sum() <= 2048 * 2048
    level1, level2 = check_tiles(kept)
    assert len(level1) > 1000 and len(level2) == 1


def check_tiles(counts):
    """Every full scan tile of 2048 items holds more than one distinct value, and the tile sums differ from tile to tile: a
    shifted, dropped or repeated tile offset cannot cancel out.  Returns the first- and second-level tile sums."""
    full = counts[:counts.shape[0] // 2048 * 2048].reshape(-1, 2048)
    assert (full.min(axis=1) != full.max(axis=1)).all()
    level1 = gc.tile_sums(counts)
    assert np.unique(level1).shape[0] > 100
    return level1, gc.tile_sums(level1)


def test_huge_sparse_components_are_known_by_construction(huge):
    W, ncomp, lcc = huge
    rc, labels = gc.cc_ref(W)
    assert rc == ncomp and ncomp > W.shape[0] // 4
    np.testing.assert_array_equal(gc.lcc_ref(rc, labels), lcc)
    assert lcc.sum() == 3000 and np.bincount(labels).max() == 3000
    first, last = np.nonzero(lcc)[0][[0, -1]]
    assert last - first == 2999 and first // 2048 != last // 2048      # the largest component crosses a scan tile
    assert is_symmetric(W)


@pytest.mark.parametrize("n", gc.HUGE_SIZES[:2])
def test_huge_sparse_at_the_small_tile_boundaries(n):
    W, ncomp, lcc = gc.huge_sparse(n)
    assert W.shape == (n, n) and is_symmetric(W)
    rc, labels = gc.cc_ref(W)
    assert rc == ncomp
    np.testing.assert_array_equal(gc.lcc_ref(rc, labels), lcc)
    deg = np.diff(W.indptr)
    assert deg.max() == 3 and deg.min() == 0 and lcc.sum() == n // 3
    mask = gc.huge_mask(n)
    assert 0 < mask.sum() < n


def test_generators_are_seeded_and_huge_sparse_costs_under_a_second():
    import time
    runs, seconds = [], []
    for _ in range(2):
        t0 = time.perf_counter()
        runs.append(gc.huge_sparse(gc.HUGE_SIZES[2]))
        seconds.append(time.perf_counter() - t0)
    a, b = runs
    np.testing.assert_array_equal(a[0].indptr, b[0].indptr)
    np.testing.assert_array_equal(a[0].indices, b[0].indices)
    np.testing.assert_array_equal(a[0].data, b[0].data)
    assert a[1] == b[1]
    print(f"huge_sparse({gc.HUGE_SIZES[2]}): {seconds[0]:.2f} s, {seconds[1]:.2f} s")
    assert min(seconds) < 1.0                          # the largest generator call (about 0.3 - 0.5 s); the better of two runs
    for make, names in ((gc.sym_lists, gc.SYM_CASES), (gc.csr_graph, gc.CSR_SMALL + gc.CC_ONLY)):
        for name in names:
            t0 = time.perf_counter()
            make(name)
            assert time.perf_counter() - t0 < 1.0, name
    for name in gc.SYM_CASES:
        x, y = gc.sym_lists(name), gc.sym_lists(name)
        np.testing.assert_array_equal(x[1], y[1])
        np.testing.assert_array_equal(x[2], y[2])
    for name in gc.CSR_SMALL + gc.CC_ONLY:
        x, y = gc.csr_graph(name), gc.csr_graph(name)
        np.testing.assert_array_equal(x.indices, y.indices)
        np.testing.assert_array_equal(x.data, y.data)
