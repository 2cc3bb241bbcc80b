"""geo_knn_query / knn_query_device: the exact search of csrc/knn.hip for queries that are not rows of the corpus.
  (a) queries that ARE corpus rows give the self-search's lists and path, bit for bit, on every path;
  (b) foreign queries (fresh Gaussians, copies of corpus rows, rows scaled by 30) against the oracle's own key of every
      (query, corpus row) pair (oracle.knn.knn_pair_keys on [z; q]): nothing of the project's code in the check;
  (c) lattice inputs, where every fp64 operation is exact and an int64 brute force is the truth: ties by corpus index, both
      forms alike, the overflow fallback;
  (d) the result does not depend on the workspace, the slices, the stream, the run or the batch a query is in;
  (e) refusals before any launch;  (f) sklearn's indices where sklearn is installed."""
import numpy as np
import pytest
import torch

from conftest import latents

pytestmark = pytest.mark.gpu

EXACT, WIDE, BF16, F32, TWO, OVERFLOW = 1, 2, 3, 4, 5, 16
FILTER_CAP = 1024                      # csrc/knn.hip: candidates a query's list holds

# (n, d, kq, knn_filter, path): one case per path and padded dimension (size thresholds: tests/test_gpu_knn_exact.py)
MATRIX = [
    (1500, 3, 1, 1, EXACT),
    (1500, 12, 12, 1, EXACT),
    (1500, 16, 64, 1, EXACT),
    (1500, 100, 12, 1, EXACT),
    (3000, 8, 65, 1, WIDE),
    (3000, 8, 256, 1, WIDE),
    (40000, 12, 21, 1, BF16),
    (40000, 16, 64, 1, BF16),
    (20000, 32, 21, 1, BF16),
    (16384, 64, 64, 1, BF16),
    (80000, 8, 21, 1, BF16),
    (40000, 16, 21, 2, F32),
    (200000, 16, 21, 1, TWO),
    (200000, 8, 21, 1, TWO),
]
IDS = [f"n{n}-d{d}-k{k}-f{f}" for n, d, k, f, _ in MATRIX]
RANGES = ((7, 1), (101, 37), (613, 130), (1111, 300))          # (first row, rows): no multiple of 4, 32 or 128


def _dev(a):
    from vqvae_amd._device import device
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(device())


def _with_filter(filt, fn):
    """fn() and the path it took, under the given knn_filter option (restored afterwards)."""
    from vqvae_amd import _lib
    lib = _lib.load()
    _lib.check(lib.geo_set_option(b"knn_filter", int(filt)), "geo_set_option")
    try:
        out = fn()
        path = lib.geo_knn_last_path()
    finally:
        lib.geo_set_option(b"knn_filter", 1)
    return out, path


def _query(z, q, kq, form=None, filt=1, cap=None):
    from vqvae_amd.geo.knn_graph_optimized import knn_query_device
    (idx, d2), path = _with_filter(filt, lambda: knn_query_device(_dev(z), _dev(q), kq, form=form, max_workspace_bytes=cap))
    return idx, d2, path


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))


# ---------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("n,d,kq,filt,path", MATRIX, ids=IDS)
def test_corpus_rows_as_queries_give_the_self_search(n, d, kq, filt, path):
    from vqvae_amd.geo.knn_graph_optimized import knn_search_device
    z = _dev(latents(n, d, 2000 + d + kq))
    for r0, rows in RANGES:
        ref, ref_path = _with_filter(filt, lambda: knn_search_device(z, kq, r0, r0 + rows))
        idx, d2, got = _query(z, z[r0:r0 + rows], kq, filt=filt)
        assert ref_path == path and got == path, f"rows [{r0}, {r0 + rows}): paths {ref_path} (self) / {got} (query), expected {path}"
        assert idx.dtype == torch.int32 and d2.dtype == torch.float64 and idx.shape == (rows, kq) == d2.shape
        assert _same((idx, d2), ref), f"rows [{r0}, {r0 + rows}) differ from the self-search"


# ---------------------------------------------------------------------------------------------------- (b)
def _foreign_queries(z, V, seed):
    """Thirds: fresh Gaussians, exact copies of corpus rows, corpus rows scaled by 30 (far out: the filter's margin is relative)."""
    r = np.random.RandomState(seed)
    n, d = z.shape
    a = V // 3
    q = np.empty((V, d), np.float32)
    q[:a] = r.randn(a, d).astype(np.float32)
    q[a:2 * a] = z[r.randint(0, n, size=a)]
    q[2 * a:] = np.float32(30.0) * z[r.randint(0, n, size=V - 2 * a)]
    return q


def _check_against_pair_keys(z, q, idx, d2, kq, form):
    """Every query's list against the oracle's key of all n pairs: the entries at or below the reported kq-th key, ordered by
    (key, index), must begin with exactly the reported list -- a missed neighbour, a wrong key or a wrong order all show."""
    from oracle.knn import knn_pair_keys
    n, V = z.shape[0], q.shape[0]
    ih, dh = idx.cpu().numpy(), d2.cpu().numpy()
    assert ih.shape == (V, kq) == dh.shape
    zq = np.concatenate([z, q], axis=0)
    cols = np.arange(n, dtype=np.int64)
    B = 32
    for b0 in range(0, V, B):
        b1 = min(V, b0 + B)
        qi = np.repeat(np.arange(n + b0, n + b1, dtype=np.int64), n)
        keys = knn_pair_keys(zq, qi, np.tile(cols, b1 - b0), form).reshape(b1 - b0, n)
        for i in range(b0, b1):
            row = keys[i - b0]
            cand = np.flatnonzero(row <= dh[i, -1])
            order = cand[np.argsort(row[cand], kind="stable")]          # cand ascends: equal keys keep ascending index
            assert order.size >= kq, f"query {i}: {order.size} corpus rows at or below the reported kq-th key {dh[i, -1]!r}"
            np.testing.assert_array_equal(ih[i], order[:kq], err_msg=f"query {i}: indices")
            np.testing.assert_array_equal(dh[i].view(np.int64), row[order[:kq]].view(np.int64), err_msg=f"query {i}: keys")


FOREIGN = [(n, d, kq, filt, path, None) for n, d, kq, filt, path in MATRIX if (n, d) not in ((40000, 12), (40000, 16))]
FOREIGN += [(40000, 12, 21, 1, BF16, 0), (40000, 12, 21, 1, BF16, 1), (40000, 16, 64, 1, BF16, 0), (40000, 16, 64, 1, BF16, 1),
            (40000, 16, 21, 2, F32, 0), (40000, 16, 21, 2, F32, 1), (1500, 12, 12, 1, EXACT, 1), (1500, 16, 64, 1, EXACT, 0)]


@pytest.mark.parametrize("n,d,kq,filt,path,form", FOREIGN,
                         ids=[f"n{n}-d{d}-k{k}-f{f}-form{fo}" for n, d, k, f, _, fo in FOREIGN])
def test_foreign_queries_every_row_exact(n, d, kq, filt, path, form):
    z = latents(n, d, 3000 + d + kq)
    q = _foreign_queries(z, 130 if n >= 200000 else 300, 17 + d)
    idx, d2, got = _query(z, q, kq, form=form, filt=filt)
    assert got == path, f"geo_knn_last_path() = {got}, expected {path}"
    _check_against_pair_keys(z, q, idx, d2, kq, (1 if d > 15 else 0) if form is None else form)


# ---------------------------------------------------------------------------------------------------- (c)
def _lattice(r, rows, d):
    return (r.randint(-64, 65, size=(rows, d)) / 16.0).astype(np.float32)          # multiples of 2^-4 in [-4, 4]


def _int_truth(z, q, kq):
    """(idx, d2) by int64 arithmetic on 16 x the coordinates: exact, ties by corpus index."""
    zi, qi = np.rint(z.astype(np.float64) * 16).astype(np.int64), np.rint(q.astype(np.float64) * 16).astype(np.int64)
    D = (qi * qi).sum(1)[:, None] - 2 * (qi @ zi.T) + (zi * zi).sum(1)[None, :]
    order = np.argsort(D, axis=1, kind="stable")[:, :kq]
    return order, np.take_along_axis(D, order, axis=1) / 256.0


@pytest.mark.parametrize("n,d,kq,path", [(1500, 12, 12, EXACT), (3000, 8, 65, WIDE), (40000, 16, 21, None)],
                         ids=["exact", "wide", "filter"])
def test_lattice_ties_follow_the_corpus_index_in_both_forms(n, d, kq, path):
    r = np.random.RandomState(5 + d)
    z = _lattice(r, n, d)
    z[n // 2:n // 2 + 40] = z[11]                                  # and plain duplicates
    q = _lattice(r, 96, d)
    q[64:] += np.float32(1000.0)                                   # far queries: every corpus row nearly equally far
    q[:8] = z[[11, 12, 13, 14, n // 2, n // 2 + 1, n - 1, 0]]
    want_i, want_d = _int_truth(z, q, kq)
    for form in (0, 1):
        idx, d2, got = _query(z, q, kq, form=form)
        if path is not None:
            assert got == path
        else:                                                      # the far queries may or may not overflow their lists
            assert got & ~OVERFLOW == BF16
        np.testing.assert_array_equal(idx.cpu().numpy(), want_i, err_msg=f"form {form}")
        np.testing.assert_array_equal(d2.cpu().numpy(), want_d, err_msg=f"form {form}")


def test_overflowing_candidate_lists_fall_back_and_stay_exact():
    """30 distinct points, each more than FILTER_CAP times: a query at one of them keeps more candidates than its list holds."""
    n, d, kq = 40000, 16, 21
    r = np.random.RandomState(9)
    pts = _lattice(r, 30, d)
    z = pts[np.arange(n) % 30]
    assert np.bincount(np.arange(n) % 30).min() > FILTER_CAP
    q = np.concatenate([pts, _lattice(r, 10, d)], axis=0)
    idx, d2, got = _query(z, q, kq)
    assert got == BF16 | OVERFLOW, f"geo_knn_last_path() = {got}"
    want_i, want_d = _int_truth(z, q, kq)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
    np.testing.assert_array_equal(d2.cpu().numpy(), want_d)


# ---------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("n,d,kq,filt,path", [(1500, 12, 12, 1, EXACT), (40000, 16, 21, 1, BF16), (40000, 16, 21, 2, F32),
                                              (200000, 8, 21, 1, TWO)], ids=["exact", "bf16", "f32", "two"])
def test_result_is_independent_of_workspace_stream_run_and_batch(n, d, kq, filt, path):
    from vqvae_amd import _lib
    lib = _lib.load()
    z = _dev(latents(n, d, 4000 + d))
    q = _dev(_foreign_queries(z.cpu().numpy(), 700, 23))
    m = q.shape[0]
    lo, full = lib.geo_knn_query_min_workspace_bytes(n, d), lib.geo_knn_query_workspace_bytes(n, m, d)
    assert lo < full
    ref = _query(z, q, kq, filt=filt)                              # the queried workspace: one slice
    assert ref[2] == path
    for cap in (1, lo, (lo + full) // 2, full + 12345):            # below the minimum -> the minimum; slices of ~126 / ~400 rows
        got = _query(z, q, kq, filt=filt, cap=cap)
        assert got[2] == path and _same(got, ref), f"max_workspace_bytes = {cap}"
    outs = []
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):           # two streams (a workspace each), and so two runs
        with torch.cuda.stream(s):
            outs.append(_query(z, q, kq, filt=filt))
        s.synchronize()
    assert _same(outs[0], ref) and _same(outs[1], ref)
    for i in (0, 299, 500, 699):                                   # a Gaussian, a copy, two scaled rows
        one = _query(z, q[i:i + 1], kq, filt=filt)
        assert one[2] == path and _same(one, (ref[0][i:i + 1], ref[1][i:i + 1])), f"query {i} alone"


# ---------------------------------------------------------------------------------------------------- (e)
def test_refusals_leave_the_outputs_untouched():
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    lib = _lib.load()
    n, m, d, kq = 500, 40, 12, 5
    z, q = _dev(latents(n, d, 1)), _dev(latents(m, d, 2))
    idx = torch.full((m, 256), -7, dtype=torch.int32, device=z.device)
    d2 = torch.full((m, 256), -7.0, dtype=torch.float64, device=z.device)
    nbytes = lib.geo_knn_query_workspace_bytes(n, m, d)
    lo = lib.geo_knn_query_min_workspace_bytes(n, d)
    assert 0 < lo <= nbytes
    ws = torch.empty(nbytes, dtype=torch.uint8, device=z.device)

    def call(zp=ptr(z), qp=ptr(q), ip=ptr(idx), dp=ptr(d2), wp=ptr(ws), n_=n, m_=m, d_=d, k_=kq, wb=nbytes):
        return lib.geo_knn_query(zp, n_, qp, m_, d_, k_, 0, ip, dp, wp, wb, stream_ptr())

    E_ARG, E_WORKSPACE = -1, -2
    for what in ("zp", "qp", "ip", "dp", "wp"):
        assert call(**{what: None}) == E_ARG, f"null {what}"
    for bad in (dict(d_=0), dict(d_=129), dict(k_=0), dict(k_=n + 1), dict(k_=257), dict(n_=0), dict(m_=-1)):
        assert call(**bad) == E_ARG, bad
        assert lib.geo_knn_last_path() == 0
    assert call(wb=lo - 1) == E_WORKSPACE
    assert b"minimum" in lib.geo_last_error()
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((d2 == -7.0).all())
    assert call(m_=0) == 0 and lib.geo_knn_last_path() == 0        # nothing to do: GEO_OK, nothing written
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((d2 == -7.0).all())
    assert call(wb=lo) == 0                                        # ... and the minimum itself is enough
    torch.cuda.synchronize()
    assert bool((idx.view(-1)[: m * kq] >= 0).all()) and bool((idx.view(-1)[m * kq:] == -7).all())


def test_no_queries_give_empty_tensors():
    from vqvae_amd.geo import knn_query_device
    z = _dev(latents(100, 8, 3))
    idx, d2 = knn_query_device(z, z[:0], 4)
    assert idx.shape == (0, 4) and idx.dtype == torch.int32 and d2.shape == (0, 4) and d2.dtype == torch.float64


# ---------------------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("d", [8, 32])
def test_kneighbors_returns_sklearn_indices(d):
    sk = pytest.importorskip("sklearn.neighbors")
    from oracle.knn import knn_pair_keys
    from vqvae_amd.geo import kneighbors
    n, m, k = 5000, 200, 10
    z, q = latents(n, d, 31 + d), latents(m, d, 32 + d)
    dist, ind = kneighbors(z, q, k)
    assert dist.dtype == np.float64 and ind.dtype == np.int64 and dist.shape == (m, k) == ind.shape
    # no case left out silently: every query's k-th and (k+1)-th exact keys are apart, so the order cannot hinge on rounding
    zq = np.concatenate([z, q], axis=0)
    keys = knn_pair_keys(zq, np.repeat(np.arange(n, n + m, dtype=np.int64), n), np.tile(np.arange(n, dtype=np.int64), m),
                         1 if d > 15 else 0).reshape(m, n)
    part = np.sort(np.partition(keys, k, axis=1)[:, :k + 1], axis=1)
    gaps = np.diff(part, axis=1) / part[:, 1:]
    assert gaps.min() > 1e-9, f"smallest relative gap between consecutive keys {gaps.min()}"
    _, ref_i = sk.NearestNeighbors(n_neighbors=k).fit(z).kneighbors(q)
    np.testing.assert_array_equal(ind, ref_i)
