"""Case generators and scipy / numpy references for the kernels of csrc/graph.hip (symmetrisation, upper-triangle edge
list and weight gather, connected components, CSR compaction) and the recursive scan of csrc/common.hip behind them.
Shared by test_graph_cases_host.py (pins the references against the oracle and every case's reason to exist) and
test_gpu_graph_kernels.py.  Everything is seeded; nothing here touches the GPU or a fixture file."""
import warnings

import numpy as np
from scipy import sparse
from scipy.sparse.csgraph import connected_components

SCAN_TILE = 2048                 # items per scan block (common.hip: 256 threads x 8 items)


# ------------------------------------------------------------------------------------------------------- references
def sym_ref(n, idx, w, sym):
    """csr_matrix of the lists, maximum / minimum with the transpose, setdiag(0), eliminate_zeros, sorted indices
    (what graph.hip replaces).  Entries whose id is outside [0, n) are removed from the lists first."""
    idx = np.asarray(idx)
    rows = np.repeat(np.arange(n, dtype=np.int64), idx.shape[1])
    cols = idx.ravel().astype(np.int64)
    vals = np.ones(cols.shape[0], np.float32) if w is None else np.asarray(w, dtype=np.float32).ravel()
    ok = (cols >= 0) & (cols < n)
    A = sparse.csr_matrix((vals[ok], (rows[ok], cols[ok])), shape=(n, n), dtype=np.float32)
    if sym == "union":
        S = A.maximum(A.T)
    elif sym == "mutual":
        S = A.minimum(A.T)
    else:
        raise ValueError(sym)
    S = sparse.csr_matrix(S, dtype=np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", sparse.SparseEfficiencyWarning)
        S.setdiag(0)
    S.eliminate_zeros()
    S.sort_indices()
    return S


def _rows_of(W):
    return np.repeat(np.arange(W.shape[0], dtype=np.int64), np.diff(W.indptr))


def upper_ref(W):
    """(src, dst, entry_edge) of a CSR with sorted rows: the stored entries with row < col in row-major order, and per stored
    entry the index of its undirected edge -- -1 for a diagonal entry and for an entry whose mirror is not stored."""
    n = W.shape[0]
    rows, cols = _rows_of(W), W.indices.astype(np.int64)
    up = rows < cols
    src, dst = rows[up], cols[up]
    keys = src * n + dst                                    # ascending: row-major order of sorted rows
    entry_edge = np.full(W.nnz, -1, dtype=np.int64)
    entry_edge[up] = np.arange(keys.shape[0])
    low = np.nonzero(rows > cols)[0]
    want = cols[low] * n + rows[low]
    pos = np.searchsorted(keys, want)
    hit = pos < keys.shape[0]
    hit[hit] = keys[pos[hit]] == want[hit]
    entry_edge[low[hit]] = pos[hit]
    return src.astype(np.int32), dst.astype(np.int32), entry_edge.astype(np.int32)


def compact_ref(W, mask, drop_zero):
    """(W[mask][:, mask] as sorted CSR, new_index): stored entries between kept nodes, exact zeros dropped when asked and kept
    as stored entries otherwise; new_index[v] = position of v among the kept nodes, -1 for the others.  mask None = all."""
    n = W.shape[0]
    mask = np.ones(n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    new_index = np.where(mask, np.cumsum(mask) - 1, -1).astype(np.int32)
    rows, cols = _rows_of(W), W.indices
    keep = mask[rows] & mask[cols]
    if drop_zero:
        keep &= W.data != 0
    m = int(mask.sum())
    indptr = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(new_index[rows[keep]], minlength=m), out=indptr[1:])
    out = sparse.csr_matrix((W.data[keep].astype(np.float32), new_index[cols[keep]], indptr), shape=(m, m))
    return out, new_index


def cc_ref(W):
    """(n_components, labels int32) of the stored pattern; scipy numbers components by their lowest node."""
    P = sparse.csr_matrix((np.ones(W.nnz, np.float32), W.indices, W.indptr), shape=W.shape)
    ncomp, labels = connected_components(P, directed=False)
    return int(ncomp), labels.astype(np.int32)


def lcc_ref(ncomp, labels):
    """Mask of the largest component, the first label on ties; everything when the graph is connected."""
    if ncomp <= 1:
        return np.ones(labels.shape[0], dtype=bool)
    return labels == int(np.argmax(np.bincount(labels, minlength=ncomp)))


# ------------------------------------------------------------------------------------------- symmetrisation lists
def _distinct_columns(r, n, k, forced=()):
    """int32 [n][k]: per row, `forced` (minus the row itself) first, then random distinct columns, never the row itself."""
    if n <= 2048:
        score = r.rand(n, n)
        for rank, c in enumerate(forced):
            score[:, c] = -1.0 - (len(forced) - rank)
        score[np.arange(n), np.arange(n)] = 2.0
        return np.argsort(score, axis=1, kind="stable")[:, :k].astype(np.int32)
    me = np.arange(n)[:, None]
    idx = r.randint(0, n, size=(n, k))
    idx[:, :len(forced)] = np.asarray(forced, dtype=np.int64)[None, :]
    while True:                                              # k << n: a few rows collide, redraw their free columns
        s = np.sort(idx, axis=1)
        bad = (s[:, 1:] == s[:, :-1]).any(axis=1) | (idx[:, len(forced):] == me).any(axis=1)
        if not bad.any():
            return idx.astype(np.int32)
        idx[bad, len(forced):] = r.randint(0, n, size=(int(bad.sum()), k - len(forced)))


def _distinct_weights(r, shape):
    """float32, all different and all > 0, so an entry paired with another entry's weight cannot go unnoticed."""
    count = int(np.prod(shape))
    return ((r.permutation(count) + 1).astype(np.float32) * np.float32(1.0 / 1024.0)).reshape(shape)


SYM_CASES = ("hub", "two_hubs_wide", "invalid_ids", "self_and_zero", "many_rows", "k1")
MANY_ROWS_N = 262145 + 300          # seg_count_kernel strides its grid (1024 blocks x 256 threads) from n > 262 144


def sym_lists(name):
    """(n, idx int32 [n][k], w float32 [n][k]) of a symmetrisation case; run it with w and with None."""
    r = np.random.RandomState(SYM_CASES.index(name) + 100)
    if name == "hub":                        # union: row 0 collects 4 999 in-entries = 79 sort segments of 64
        n, k = 5000, 3
        idx = _distinct_columns(r, n, k, forced=(0,))
        idx[0] = (1234, 17, 4321)            # (row 0's forced column 0 was itself)
    elif name == "two_hubs_wide":            # k > 64: the out part of a row alone spans three lane trips
        n, k = 1500, 130
        idx = _distinct_columns(r, n, k, forced=(0, 1))
    elif name == "invalid_ids":
        n, k = 300, 8
        idx = _distinct_columns(r, n, k)
        bad = r.rand(n, k) < 0.2
        idx[bad] = r.choice(np.array([-1, n, n + 7], dtype=np.int32), size=int(bad.sum()))
        idx[123] = (-1, n, n + 7, -1, n, n + 7, -1, n)
    elif name == "self_and_zero":
        n, k = 200, 5
        idx = _distinct_columns(r, n, k)
        selfish = r.choice(n, size=30, replace=False)
        idx[selfish, r.randint(0, k, size=30)] = selfish.astype(np.int32)
    elif name == "many_rows":
        n, k = MANY_ROWS_N, 2
        idx = _distinct_columns(r, n, k)
    elif name == "k1":                       # one cycle through all 65 nodes, ids in random order
        n, k = 65, 1
        p = r.permutation(n)
        idx = np.empty((n, 1), dtype=np.int32)
        idx[p, 0] = np.roll(p, -1)
    else:
        raise KeyError(name)
    w = _distinct_weights(r, idx.shape)
    if name == "self_and_zero":
        w[r.rand(n, k) < 0.15] = 0.0
        a, b = 10, 20                        # a -> b stored with weight 0.0, b -> a with a positive weight
        pa = int(np.nonzero(idx[a] == b)[0][0]) if (idx[a] == b).any() else 0
        pb = int(np.nonzero(idx[b] == a)[0][0]) if (idx[b] == a).any() else 0
        idx[a, pa], idx[b, pb] = b, a
        w[a, pa], w[b, pb] = 0.0, 3.25
    return n, np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(w, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------- CSR graphs
def csr_from_entries(n, rows, cols, data):
    """Sorted CSR of the given directed entries as they are: nothing summed, nothing dropped, stored zeros stay."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.lexsort((cols, rows))
    indptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    W = sparse.csr_matrix((np.asarray(data, dtype=np.float32)[order], cols[order].astype(np.int32), indptr), shape=(n, n))
    W.has_sorted_indices = True
    return W


def _edge_weights(r, m):
    """float32 in (0, 1] with every 7th edge exactly 0.0 (a stored zero on both of its entries)."""
    w = (r.rand(m).astype(np.float32) * np.float32(0.75) + np.float32(0.25))
    w[::7] = 0.0
    return w


def symmetric_csr(n, src, dst, w):
    return csr_from_entries(n, np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([w, w]))


WIDE_N = 600
WIDE_EMPTY = (0, 300, WIDE_N - 1)
# row -> exact number of entries: one entry short of, at, and one past one and two 64-entry wave trips, and the widest;
# rows near the middle have the diagonal inside their second or third trip
WIDE_DEGREES = {7: 64, 211: 65, 313: 128, 417: 129, 299: 300, 523: 63, 29: 127, 331: 200, 37: 1, 283: 191, 593: 193}


def _wide_edges(r):
    special = np.array(sorted(WIDE_DEGREES))
    ordinary = np.setdiff1d(np.arange(WIDE_N), np.concatenate([special, np.array(WIDE_EMPTY)]))
    src, dst = [], []
    for s in special:                                        # special rows meet ordinary nodes only: degrees stay exact
        nb = r.choice(ordinary, size=WIDE_DEGREES[int(s)], replace=False)
        src.append(np.full(nb.shape[0], s)), dst.append(nb)
    a, b = ordinary[r.randint(0, len(ordinary), 900)], ordinary[r.randint(0, len(ordinary), 900)]
    a, b = np.concatenate([a, ordinary[:-1]]), np.concatenate([b, ordinary[1:]])      # a chain: no ordinary row is empty
    keep = a != b
    pairs = np.unique(np.stack([np.minimum(a, b)[keep], np.maximum(a, b)[keep]], axis=1), axis=0)
    src.append(pairs[:, 0]), dst.append(pairs[:, 1])
    return np.concatenate(src), np.concatenate(dst)


CSR_SMALL = ("wide_rows", "with_diagonal", "one_sided")
CC_ONLY = ("path_perm", "path_desc", "path_zigzag", "forest", "star_grid")
PATH_N = 40000                      # cc_hook_kernel strides its grid (2048 blocks x 16 groups) from n > 32 768
FOREST_N, FOREST_COMPONENTS, FOREST_LARGEST = 40000, 3000, 2000
STAR_LEAVES, GRID_SIDE = 5000, 100


def _path_order(name, r):
    n = PATH_N
    if name == "path_perm":
        return r.permutation(n)
    if name == "path_desc":
        return np.arange(n - 1, -1, -1)
    order = np.empty(n, dtype=np.int64)                      # 0, n-1, 1, n-2, ...
    order[0::2] = np.arange(n // 2)
    order[1::2] = n - 1 - np.arange(n // 2)
    return order


def _forest_edges(r):
    """(src, dst) in node POSITIONS (the ids are permuted afterwards): the largest tree and the next two are paths (deep),
    the others random recursive trees (bushy); 200 single nodes."""
    fixed = [FOREST_LARGEST, 1000, 500]
    rest = FOREST_COMPONENTS - len(fixed)
    sizes = np.ones(rest, dtype=np.int64)
    extra = FOREST_N - sum(fixed) - rest
    sizes[200:] += r.multinomial(extra, r.dirichlet(np.ones(rest - 200)))
    sizes = np.concatenate([np.array(fixed), sizes])
    start = np.concatenate([[0], np.cumsum(sizes)])
    assert start[-1] == FOREST_N and sizes[3:].max() < FOREST_LARGEST
    comp = np.repeat(np.arange(FOREST_COMPONENTS), sizes)
    pos = np.arange(FOREST_N)
    first = start[comp]
    child = pos[pos > first]
    parent = first[child] + (r.rand(child.shape[0]) * (child - first[child])).astype(np.int64)
    deep = comp[child] < 3
    parent[deep] = child[deep] - 1
    return child, parent, sizes


def csr_graph(name):
    """A symmetric (except `one_sided`), sorted CSR with float32 data and stored exact zeros."""
    names = CSR_SMALL + CC_ONLY
    r = np.random.RandomState(names.index(name) + 200)
    if name in CSR_SMALL:
        src, dst = _wide_edges(np.random.RandomState(200))   # the same graph under all three names
        W = symmetric_csr(WIDE_N, src, dst, _edge_weights(np.random.RandomState(201), src.shape[0]))
        if name == "with_diagonal":                          # a tenth of the rows, one of them otherwise empty
            d = np.concatenate([[0], r.choice(np.arange(1, WIDE_N - 1), size=WIDE_N // 10 - 1, replace=False)])
            dv = r.rand(d.shape[0]).astype(np.float32)
            dv[::3] = 0.0
            rows = np.concatenate([_rows_of(W), d])
            W = csr_from_entries(WIDE_N, rows, np.concatenate([W.indices, d]), np.concatenate([W.data, dv]))
        elif name == "one_sided":                            # 20 entries lose their mirror
            drop = r.choice(W.nnz, size=20, replace=False)
            keep = np.ones(W.nnz, dtype=bool)
            keep[drop] = False
            W = csr_from_entries(WIDE_N, _rows_of(W)[keep], W.indices[keep], W.data[keep])
        return W
    if name.startswith("path_"):
        order = _path_order(name, r)
        return symmetric_csr(PATH_N, order[:-1], order[1:], _edge_weights(r, PATH_N - 1))
    if name == "forest":
        child, parent, _ = _forest_edges(r)
        ids = r.permutation(FOREST_N)
        return symmetric_csr(FOREST_N, ids[child], ids[parent], _edge_weights(r, child.shape[0]))
    if name == "star_grid":                                  # centre = highest id: every leaf has to be pulled down through it
        n = STAR_LEAVES + 1 + GRID_SIDE * GRID_SIDE
        ids = r.permutation(n - 1)
        leaves, cell = ids[:STAR_LEAVES], ids[STAR_LEAVES:].reshape(GRID_SIDE, GRID_SIDE)
        src = np.concatenate([np.full(STAR_LEAVES, n - 1), cell[:, :-1].ravel(), cell[:-1, :].ravel()])
        dst = np.concatenate([leaves, cell[:, 1:].ravel(), cell[1:, :].ravel()])
        return symmetric_csr(n, src, dst, _edge_weights(r, src.shape[0]))
    raise KeyError(name)


# --------------------------------------------------------------------------------------------------- huge_sparse
HUGE_N = SCAN_TILE * SCAN_TILE + 1          # 4 194 305 rows: the scan recurses three times
HUGE_SIZES = (SCAN_TILE, SCAN_TILE + 1, SCAN_TILE * SCAN_TILE, HUGE_N)
_SEG_LEN = (1, 2, 3, 4, 5, 7)
_SEG_P = ((0.55, 0.25, 0.08, 0.06, 0.03, 0.03), (0.25, 0.25, 0.15, 0.15, 0.10, 0.10))
# one random byte -> segment length, per mix (the probabilities in 256ths)
_SEG_LUT = tuple(np.repeat(np.array(_SEG_LEN, dtype=np.int32), np.diff(np.round(np.cumsum((0.0,) + p) * 256).astype(int)))
                 for p in _SEG_P)
_REGIME = 30000                                   # segments per stretch of one mix
# a row's neighbours by its 4 flags (bit 0: v-2, bit 1: v-1, bit 2: v+1, bit 3: v+2): column offset of its j-th entry
_ROW_OFFSETS = np.zeros((16, 4), dtype=np.int32)
for _code in range(16):
    _offs = [o for bit, o in enumerate((-2, -1, 1, 2)) if _code >> bit & 1]
    _ROW_OFFSETS[_code, :len(_offs)] = _offs
_ROW_DEGREE = np.array([bin(c).count("1") for c in range(16)], dtype=np.int64)


def huge_sparse(n):
    """(W, n_components, lcc_mask).  Consecutive node ids are cut into segments of 1-7 nodes, one long segment in the
    middle is the largest component; a segment is a path, from 4 nodes on with a chord from its first to its third node, so
    row degrees are 0-3.  Two segment-length mixes alternate every 30 000 segments, so neither the rows of a scan tile nor
    the tiles of a second-level tile sum to a constant.  Built without a sort or a scatter: one random byte per segment,
    four flags per row, and every row's columns (ascending) from a table of its flags."""
    r = np.random.RandomState(n % 1000003)
    m = int(0.62 * n) + 64                                   # more segments than can fit (mean length >= 1.89)
    u = np.frombuffer(r.bytes(m), dtype=np.uint8)
    length = _SEG_LUT[0][u]
    for b in range(_REGIME, m, 2 * _REGIME):
        length[b:b + _REGIME] = _SEG_LUT[1][u[b:b + _REGIME]]
    big_at, big = int(0.2 * n), max(8, min(3000, n // 3))    # lands near the middle of the node range
    length[big_at] = big
    end = np.cumsum(length)
    used = int(np.searchsorted(end, n)) + 1                  # segments that begin inside [0, n)
    assert big_at < used - 1 <= m - 1 and end[used - 1] >= n
    start, length = end[:used] - length[:used], length[:used]
    length[-1] = n - start[-1]
    is_start = np.zeros(n + 2, dtype=np.uint8)
    is_start[start] = 1
    is_start[n:] = 1
    chord = np.zeros(n + 2, dtype=np.uint8)                  # s of the chord (s, s + 2), stored at s + 2
    chord[start[length >= 4] + 2] = 1
    code = chord[:n] | (1 - is_start[:n]) << 1 | (1 - is_start[1:n + 1]) << 2 | chord[2:] << 3
    indptr = np.zeros(n + 1, dtype=np.int32)
    degree = _ROW_DEGREE[code]
    np.cumsum(degree, out=indptr[1:])
    rows = np.repeat(np.arange(n, dtype=np.int32), degree)
    nth = np.arange(indptr[-1], dtype=np.int32) - indptr[rows]          # position of the entry inside its row
    off = _ROW_OFFSETS.ravel()[code[rows].astype(np.int32) * 4 + nth]
    indices = rows + off
    # per undirected edge (lower end, span 1 or 2): a multiplicative hash, 0.0 on one edge in sixteen
    key = (np.minimum(rows, indices) * 2 + np.abs(off)).astype(np.uint32)
    data = ((key * np.uint32(2654435761)) >> np.uint32(20) & np.uint32(15)).astype(np.float32) * np.float32(0.125)
    W = sparse.csr_matrix((data, indices, indptr), shape=(n, n))
    W.has_sorted_indices = True
    lcc = np.zeros(n, dtype=bool)
    lcc[start[big_at]:start[big_at] + big] = True
    return W, used, lcc


def huge_mask(n):
    """Keep mask whose density changes every 50 000 nodes (tile sums of the keep flags differ from tile to tile)."""
    r = np.random.RandomState(n % 1000003 + 1)
    p = np.where((np.arange(n) // 50000) % 2 == 0, 0.8, 0.35)
    return r.rand(n) < p


def tile_sums(counts):
    """Sums of `counts` over scan tiles of 2048 items (the last one padded with zeros)."""
    counts = np.asarray(counts, dtype=np.int64)
    pad = (-counts.shape[0]) % SCAN_TILE
    return np.concatenate([counts, np.zeros(pad, dtype=np.int64)]).reshape(-1, SCAN_TILE).sum(axis=1)


def masks_for(n, seed):
    """The compaction masks every CSR case is run with: name -> bool [n] or None."""
    r = np.random.RandomState(seed)
    one = np.zeros(n, dtype=bool)
    one[int(r.randint(0, n))] = True
    return {"random": r.rand(n) > 0.3, "all": np.ones(n, dtype=bool), "none": np.zeros(n, dtype=bool), "one": one}
