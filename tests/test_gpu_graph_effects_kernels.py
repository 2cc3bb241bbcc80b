"""GPU checks of csrc/graph_effects.hip: geo_path_stats against numpy on values whose fp64 sums are exact in every order
(equality, not a tolerance), its independence of stream, call and companion rows; geo_csr_set_symmetric against scipy's lil
assignment, its no-op and its refusal of a pair that is not an edge."""
import numpy as np
import pytest
import torch
from scipy import sparse

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 4099)


def _block(n, rows, ld, seed):
    """rows x ld float32: multiples of 2^-10 below 2^20 with +inf and 0.0 mixed in; the last row of a 3-row block has no
    qualifying entry (zeros and +inf only).  Columns past n hold a large finite value that must not be read."""
    r = np.random.RandomState(seed)
    a = (r.randint(1, 1 << 30, size=(rows, ld)).astype(np.float64) / 1024.0).astype(np.float32)
    assert np.array_equal(a.astype(np.float64) * 1024.0, np.round(a.astype(np.float64) * 1024.0))
    kind = r.randint(0, 10, size=(rows, ld))
    a[kind == 0] = np.inf
    a[kind == 1] = 0.0
    if rows == 3:
        a[2] = np.where(kind[2] % 2 == 0, np.inf, 0.0).astype(np.float32)
    a[:, n:] = 3.0e8
    return a


def _expected(a, n):
    v = a[:, :n].astype(np.float64)
    ok = np.isfinite(v) & (v > 0)
    fin = np.isfinite(v)
    return {"sum": np.where(ok, v, 0.0).sum(axis=1), "n_pos": ok.sum(axis=1), "n_unreached": np.isposinf(v).sum(axis=1),
            "max": np.array([row[f].max() if f.any() else 0.0 for row, f in zip(a[:, :n], fin)], dtype=np.float32)}


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("pad", (0, 5))
@pytest.mark.parametrize("rows", (1, 3))
@pytest.mark.parametrize("n", SIZES)
def test_path_stats_equals_numpy(n, rows, pad):
    from vqvae_amd.geo.experiments import path_stats_device
    dev = torch.device("cuda", 0)
    a = _block(n, rows, n + pad, 100 * n + 10 * rows + pad)
    want = _expected(a, n)
    if rows == 3:
        assert want["n_pos"][2] == 0 and want["sum"][2] == 0.0 and want["max"][2] == 0.0
    D = torch.from_numpy(a).to(dev)
    view = D[:, :n]
    if pad and rows == 3 and (n + pad) % 4:                               # row starts that are not 16-byte aligned
        assert view[1].data_ptr() % 16 != 0 or view[2].data_ptr() % 16 != 0
    got = _host(path_stats_device(view))
    for key in want:
        assert np.array_equal(got[key], want[key]), (key, got[key], want[key])
    # a second call and a side stream: equal again
    again = _host(path_stats_device(view))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = _host(path_stats_device(view))
    side.synchronize()
    for key in want:
        assert np.array_equal(again[key], got[key]) and np.array_equal(other[key], got[key]), key
    # every row alone gives what it gave among the others
    if rows == 3:
        for r in range(3):
            alone = _host(path_stats_device(view[r:r + 1]))
            for key in want:
                assert np.array_equal(alone[key], got[key][r:r + 1]), (key, r)


def test_path_stats_bits_do_not_depend_on_companions():
    """Values whose sum is NOT exact (random float32 distances): bit-identical alone, in a block, on a side stream."""
    from vqvae_amd.geo.experiments import path_stats_device
    dev = torch.device("cuda", 0)
    r = np.random.RandomState(5)
    a = r.rand(3, 4099 + 5).astype(np.float32) * 7.3
    a[r.rand(*a.shape) < 0.1] = np.inf
    view = torch.from_numpy(a).to(dev)[:, :4099]
    got = _host(path_stats_device(view))
    ref = np.where(np.isfinite(a[:, :4099]), a[:, :4099].astype(np.float64), 0.0).sum(axis=1)
    assert np.allclose(got["sum"], ref, rtol=4099 * 2.0 ** -53, atol=0)
    for row in range(3):
        alone = _host(path_stats_device(view[row:row + 1]))
        assert alone["sum"].tobytes() == got["sum"][row:row + 1].tobytes()


def _hub_graph(n, seed):
    """Random symmetric CSR without diagonal: degrees from 1 up to a hub of min(n - 1, 300)."""
    r = np.random.RandomState(seed)
    pairs = set()
    hub = 0
    for j in r.permutation(np.arange(1, n))[:min(n - 1, 300)]:
        pairs.add((hub, int(j)))
    for i in range(1, n):
        for j in (i + 1 + r.randint(0, n - 1, size=r.randint(1, 4))) % n:        # one to three neighbours other than i
            pairs.add((min(i, int(j)), max(i, int(j))))
    p = np.array(sorted(pairs))
    w = r.rand(len(p)).astype(np.float32) + 0.5
    W = sparse.coo_matrix((np.concatenate([w, w]), (np.concatenate([p[:, 0], p[:, 1]]), np.concatenate([p[:, 1], p[:, 0]]))),
                          shape=(n, n)).tocsr()
    W.sort_indices()
    return W, p


@pytest.mark.parametrize("n", (2, 65, 1000))
def test_csr_set_symmetric_equals_scipy_lil(n):
    from vqvae_amd._device import DeviceCSR
    from vqvae_amd.geo.experiments import reweight_edges_symmetric_device
    dev = torch.device("cuda", 0)
    W, p = _hub_graph(n, n)
    deg = np.diff(W.indptr)
    assert deg.min() >= 1 and (n == 65 or deg.min() == 1) and deg.max() >= min(n - 1, 300)
    r = np.random.RandomState(n + 1)
    take = r.permutation(len(p))[:max(1, (2 * len(p)) // 3)]
    hub_cols = np.sort(p[p[:, 0] == 0][:, 1])
    wanted = {(0, int(hub_cols[0])), (0, int(hub_cols[-1])), (0, int(hub_cols[len(hub_cols) // 2]))}   # first, last, middle of the hub row
    take = np.unique(np.concatenate([take, [t for t, (a, b) in enumerate(p) if (int(a), int(b)) in wanted]]))
    i, j = p[take, 0], p[take, 1]
    v = (r.rand(len(take)).astype(np.float32) + 2.0)
    L = W.tolil()
    L[i, j] = L[j, i] = v
    want = L.tocsr()
    want.sort_indices()
    G = DeviceCSR.from_scipy(W, dev)
    before = G.data.clone()
    out = reweight_edges_symmetric_device(G, i, j, v)
    assert np.array_equal(want.indptr, W.indptr) and np.array_equal(want.indices, W.indices)
    assert np.array_equal(out.data.cpu().numpy(), want.data)
    assert torch.equal(G.data, before)                                    # a copy: the input keeps its weights
    # m = 0 is a no-op
    empty = reweight_edges_symmetric_device(G, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32))
    assert torch.equal(empty.data, before)
    # a pair that is not an edge raises and leaves the data unchanged
    dense = W.toarray()
    absent = [(a, b) for a in range(n) for b in range(a + 1, n) if dense[a, b] == 0][:1]
    bad_i = np.concatenate([i[:3], [absent[0][0]] if absent else [0]])
    bad_j = np.concatenate([j[:3], [absent[0][1]] if absent else [0]])       # n = 2: the diagonal (0, 0) is no entry either
    with pytest.raises(ValueError):
        reweight_edges_symmetric_device(G, bad_i, bad_j, np.full(len(bad_i), 9.0, np.float32))
    assert torch.equal(G.data, before)
    with pytest.raises(ValueError):                                          # a repeated edge, in either orientation
        reweight_edges_symmetric_device(G, np.array([i[0], j[0]]), np.array([j[0], i[0]]), np.ones(2, np.float32))


def test_csr_set_symmetric_kernel_skips_incomplete_pairs():
    """The entry point itself, on a CSR that is NOT symmetric: a pair stored in one direction only, a pair stored in neither
    and a pair with an endpoint outside [0, n) write nothing and are counted; complete pairs in the same call are written."""
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    dev = torch.device("cuda", 0)
    # rows: 0 -> {1, 2}, 1 -> {0}, 2 -> {}, 3 -> {3}: (0, 1) both ways, (0, 2) one way, (3, 3) the diagonal
    indptr = torch.tensor([0, 2, 3, 3, 4], dtype=torch.int32, device=dev)
    indices = torch.tensor([1, 2, 0, 3], dtype=torch.int32, device=dev)
    start = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float32, device=dev)

    def call(pairs, vals):
        data = start.clone()
        src = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device=dev)
        dst = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device=dev)
        val = torch.tensor(vals, dtype=torch.float32, device=dev)
        missing = torch.full((1,), 77, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().geo_csr_set_symmetric(ptr(indptr), ptr(indices), ptr(data), 4, ptr(src), ptr(dst), ptr(val),
                                                         len(pairs), ptr(missing), stream_ptr()), "geo_csr_set_symmetric")
        return data.cpu().tolist(), int(missing.item())

    assert call([(0, 2)], [9.0]) == ([1.0, 2.0, 3.0, 4.0], 1)              # stored as (0, 2) only
    assert call([(2, 0)], [9.0]) == ([1.0, 2.0, 3.0, 4.0], 1)              # the same pair from its empty side
    assert call([(1, 2)], [9.0]) == ([1.0, 2.0, 3.0, 4.0], 1)              # stored in neither direction
    assert call([(0, 4)], [9.0]) == ([1.0, 2.0, 3.0, 4.0], 1)              # endpoint == n
    assert call([(-1, 0)], [9.0]) == ([1.0, 2.0, 3.0, 4.0], 1)             # negative endpoint
    assert call([(1, 0), (0, 2), (3, 3), (7, 1)], [5.0, 9.0, 6.0, 9.0]) == ([5.0, 2.0, 5.0, 6.0], 2)
    assert call([(0, 1)], [8.0]) == ([8.0, 2.0, 8.0, 4.0], 0)


@pytest.mark.parametrize("E", (2, 16384, 16385, 40000))
def test_pearson_device_pools_pieces(E):
    """Vectors longer than geo_image_pair_moments' 16 384 pixels are reduced in pieces and pooled in fp64: against numpy's
    fp64 corrcoef within 1e-12 (E fp64 roundings of 1.1e-16 each, far below)."""
    from vqvae_amd.geo.experiments import pearson_device
    r = np.random.RandomState(E)
    x = (r.rand(E) + 0.5).astype(np.float32)
    y = (0.3 * x + 0.05 * r.randn(E) + np.linspace(0, 0.2, E)).astype(np.float32)
    dev = torch.device("cuda", 0)
    got = pearson_device(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    want = float(np.corrcoef(x.astype(np.float64), y.astype(np.float64))[0, 1])
    assert abs(got - want) <= 1e-12, (got, want)
