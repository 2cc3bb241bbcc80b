"""The thresholds of csrc/knn.hip's filter on their own (geo_knn_thresholds).  The lists are exact under any valid threshold and
tests/test_gpu_knn_exact.py checks them row by row; a wrong bound hides behind them: too loose shows only as overflow
fallbacks, too tight only on unlucky rows.  Here every row's tau is set against the checker's own fp64 keys
(oracle.knn.knn_pair_keys, the same C chains), so all comparisons are exact:
  - validity: at least kq corpus rows have key <= tau;
  - tau is the key of a subset row (rows 0, S, 2 S, ...) and at least the subset's kq-th smallest key;
  - tau is the kq-th smallest of the per-lane minima as include/geo_hip.h defines them (subset row p in lane p % 64, two
    minima per lane for kq <= 24, three above);
  - tightness: the bound keeps at most 1.15 x the candidates of the subset's exact kq-th key.
Subset sizes m = ceil(n / S) around the kernel's seams: m = kq, m < 64, m just above 64, m <= 128 and m <= 192 (every subset
row is one of the values), a partial last 64-row step, more than four steps (a wave of the workgroup takes two).
The symmetrisation tests at the end belong to the same change: csrc/graph.hip evaluates every row element once."""
import numpy as np
import pytest
import torch

from conftest import latents

pytestmark = pytest.mark.gpu


def _tau(z, kq, S, r0, r1):
    from vqvae_amd import _lib
    from vqvae_amd._device import device, ptr, stream_ptr, workspace
    lib = _lib.load()
    zt = torch.from_numpy(np.ascontiguousarray(z)).to(device())
    n, d = z.shape
    tau = torch.full((max(r1 - r0, 1),), -7.0, dtype=torch.float64, device=zt.device)
    ws = workspace(2 * lib.geo_knn_workspace_bytes(n, d), zt.device)
    with torch.cuda.device(zt.device):
        _lib.check(lib.geo_knn_thresholds(ptr(zt), n, d, kq, 1 if d > 15 else 0, r0, r1, S, ptr(tau), ptr(ws), ws.numel(),
                                          stream_ptr()), "geo_knn_thresholds")
        torch.cuda.synchronize()
    return tau.cpu().numpy()[:r1 - r0]


def _keys(z, r0, r1):
    """Oracle keys [r1 - r0, n] of the query rows against the whole corpus."""
    from oracle.knn import knn_pair_keys
    n = z.shape[0]
    qi = np.repeat(np.arange(r0, r1, dtype=np.int64), n)
    qj = np.tile(np.arange(n, dtype=np.int64), r1 - r0)
    return knn_pair_keys(z, qi, qj, 1 if z.shape[1] > 15 else 0).reshape(r1 - r0, n)


def _lane_bound(sub, kq):
    """The documented bound from the subset's keys [rows, m]: subset row p in lane p % 64, the 2 (kq <= 24) or 3 smallest per
    lane, the kq-th smallest of those."""
    rows, m = sub.shape
    keep = 2 if kq <= 24 else 3
    pad = (-m) % 64
    lanes = np.concatenate([sub, np.full((rows, pad), np.inf)], 1).reshape(rows, -1, 64)
    lanes = np.concatenate([lanes, np.full((rows, keep, 64), np.inf)], 1)
    vals = np.sort(lanes, 1)[:, :keep, :].reshape(rows, -1)
    return np.sort(vals, 1)[:, kq - 1]


def _check(z, kq, S, r0, r1):
    tau = _tau(z, kq, S, r0, r1)
    K = _keys(z, r0, r1)
    sub = K[:, ::S]
    kth = np.sort(sub, 1)[:, kq - 1]
    count = (K <= tau[:, None]).sum(1)
    print(f"n={z.shape[0]} d={z.shape[1]} kq={kq} S={S} m={sub.shape[1]} rows {r0}..{r1}: min count {count.min()}, "
          f"tau == subset kq-th on {np.mean(tau == kth):.1%} of the rows")
    assert np.isfinite(tau).all()
    assert (count >= kq).all(), f"row {r0 + int(np.argmin(count))}: only {count.min()} keys <= tau, kq = {kq}"
    assert (sub == tau[:, None]).any(1).all(), "tau is not the key of a subset row"
    assert (tau >= kth).all(), "tau below the subset's kq-th smallest key"
    np.testing.assert_array_equal(tau, _lane_bound(sub, kq))
    return tau, K


# (n, d, kq, S, row0, row1)
CASES = [
    (21 * 16, 16, 21, 16, 0, 336),          # m = kq: lanes with one entry and with none
    (300, 16, 64, 4, 0, 300),               # m = 75, kq = 64: three minima, 11 lanes with two entries
    (1000, 15, 21, 16, 0, 1000),            # m = 63: not one full step; direct form, dp 16
    (1025, 3, 21, 16, 3, 1022),             # m = 65: one row in the second wave's step; direct form, dp 8
    (3000, 16, 21, 16, 1001, 1508),         # m = 188: partial third step; 507 rows, no multiple of the workgroup's 8
    (5000, 33, 2, 16, 4000, 4203),          # m = 313: wave 0 takes two steps; expansion form, dp 64 in two chunks; kq = 2
    (5000, 64, 1, 16, 4990, 5000),          # kq = 1; the last rows
    (2100, 16, 40, 8, 7, 400),              # m = 263, S = 8, three minima
    (4000, 64, 64, 4, 100, 357),            # m = 1 000, S = 4, three minima, dp 64
    (2000, 8, 24, 16, 0, 301),              # the longest list on two minima
    (2000, 9, 25, 8, 0, 301),               # the shortest on three
    (700, 16, 64, 4, 0, 700),               # m = 175 <= 192: every subset row is one of the values
]


@pytest.mark.parametrize("n,d,kq,S,r0,r1", CASES, ids=[f"n{c[0]}-d{c[1]}-k{c[2]}-S{c[3]}" for c in CASES])
def test_threshold_is_a_valid_subset_key_on_every_row(n, d, kq, S, r0, r1):
    z = latents(n, d, 300 + d + kq)
    tau, K = _check(z, kq, S, r0, r1)
    m = (n + S - 1) // S
    if m <= 64 * (2 if kq <= 24 else 3):                   # all subset rows kept: the exact subset threshold
        np.testing.assert_array_equal(tau, np.sort(K[:, ::S], 1)[:, kq - 1])


def test_empty_row_range_writes_nothing():
    z = latents(1000, 16, 7)
    assert _tau(z, 21, 16, 500, 500).size == 0
    from vqvae_amd import _lib
    from vqvae_amd._device import device, ptr, stream_ptr, workspace
    lib = _lib.load()
    zt = torch.from_numpy(z).to(device())
    tau = torch.full((8,), -7.0, dtype=torch.float64, device=zt.device)
    ws = workspace(2 * lib.geo_knn_workspace_bytes(1000, 16), zt.device)
    with torch.cuda.device(zt.device):
        _lib.check(lib.geo_knn_thresholds(ptr(zt), 1000, 16, 21, 1, 500, 500, 16, ptr(tau), ptr(ws), ws.numel(), stream_ptr()),
                   "geo_knn_thresholds")
        torch.cuda.synchronize()
    assert (tau == -7.0).all()


@pytest.mark.parametrize("kq,S", [(21, 16), (64, 4)])
def test_all_rows_equal_gives_zero(kq, S):
    z = np.tile(latents(1, 16, 11), (2000, 1))
    tau = _tau(z, kq, S, 0, 2000)
    assert (tau == 0).all()


def test_two_points_alternating():
    """Two distinct points a, b with n / 2 >= kq S.  Alternating by subset position (blocks of S rows) every lane sees one of
    the two points only: a query's zeros sit in every other lane, two per lane.  Alternating by row with an odd stride the
    subset alternates as well; with S = 16 the subset is all a, and b's threshold is the key of (b, a)."""
    n, d, kq = 2000, 16, 21
    ab = latents(2, d, 13)
    blocks = ab[(np.arange(n) // 16) % 2]
    assert (_tau(blocks, kq, 16, 0, n) == 0).all()
    rows = ab[np.arange(n) % 2]
    assert (_tau(rows, kq, 3, 0, n) == 0).all()
    tau = _tau(rows, kq, 16, 0, n)
    from oracle.knn import knn_pair_keys
    kba = knn_pair_keys(rows, np.array([1]), np.array([0]), 1)[0]
    assert kba > 0
    np.testing.assert_array_equal(tau, np.where(np.arange(n) % 2 == 0, 0.0, kba))


@pytest.mark.parametrize("kq,S", [(21, 16), (40, 8), (64, 4)])
def test_bound_keeps_at_most_15_percent_more_than_the_exact_subset_threshold(kq, S):
    """20 000 x 16 standard-normal rows, 256 queries: mean #{j : key <= tau} against the same count under the subset's exact
    kq-th key.  The per-lane scheme alone (numpy, same shape): 1.015 with two minima at (21, 16); 1.006 and 1.022 with three at
    (40, 8) and (64, 4) -- two minima would give 1.05 and 1.14 there, too close to the cap, hence three above kq = 24.  (The
    longest list is not held to half of FILTER_CAP: under the exact subset threshold it is 523 at (21, 16) on these rows.)"""
    z = latents(20000, 16, 5)
    r0, r1 = 5000, 5256
    tau, K = _check(z, kq, S, r0, r1)
    kth = np.sort(K[:, ::S], 1)[:, kq - 1]
    got, ref = (K <= tau[:, None]).sum(1), (K <= kth[:, None]).sum(1)
    print(f"kq={kq} S={S}: candidates mean {got.mean():.1f} max {got.max()} against {ref.mean():.1f} / {ref.max()} exact: "
          f"ratio {got.mean() / ref.mean():.4f}")
    assert got.mean() <= 1.15 * ref.mean()
    assert got.max() < 1024                                  # FILTER_CAP: a longer list sends the whole call to the exact scan


# ------------------------------------------------------------------------------------------------- symmetrisation
# csrc/graph.hip evaluates every element of a row once (sym_count_kernel) and leaves the kept ones at r k + off_in[r];
# sym_sort_kernel ranks them from there.  Same CSR as before, bit for bit: against oracle.knn.symmetrise.
SYM_N, SYM_K = 3000, 20


def _sym_lists():
    """k = 20 random lists with distinct columns; node 7 is in the lists of 2 500 of the rows 0 .. 2 520 (a hub: 40 segments
    of its row); rows 100 .. 119 hold invalid ids only (-1); rows 200 .. 260 list themselves."""
    r = np.random.RandomState(401)
    idx = np.empty((SYM_N, SYM_K), np.int32)
    for row in range(SYM_N):
        perm = r.permutation(SYM_N)[:SYM_K + 2]
        idx[row] = perm[(perm != 7) & (perm != row)][:SYM_K]
    idx[:2521, 0] = 7
    idx[7, 0] = next(c for c in range(8, 40) if c not in idx[7, 1:])
    idx[200:261, 3] = np.arange(200, 261)
    idx[100:120] = -1
    w = (0.5 + r.rand(SYM_N, SYM_K)).astype(np.float32)
    return idx, w


@pytest.mark.parametrize("sym", ["union", "mutual"])
@pytest.mark.parametrize("weighted", [True, False])
def test_symmetrise_from_provisional_positions(sym, weighted):
    from oracle.knn import symmetrise
    from vqvae_amd._device import device
    from vqvae_amd.geo.knn_graph_optimized import symmetrize_device
    idx, w = _sym_lists()
    assert all(len(set(row)) == SYM_K for row in idx[:100]) and (idx[:, 0] == 7).sum() == 2500
    G = symmetrize_device(torch.from_numpy(idx).to(device()), torch.from_numpy(w).to(device()) if weighted else None, sym)
    # the reference has no notion of an invalid id: a row listing itself gives no entry either
    idx_ref = np.where(idx < 0, np.arange(SYM_N)[:, None], idx)
    ref = symmetrise(SYM_N, idx_ref, w if weighted else np.ones_like(w), sym)
    ref.sort_indices()
    np.testing.assert_array_equal(G.indptr.cpu().numpy(), ref.indptr)
    np.testing.assert_array_equal(G.indices.cpu().numpy(), ref.indices)
    np.testing.assert_array_equal(G.data.cpu().numpy(), ref.data)
    if sym == "union":
        assert ref.indptr[8] - ref.indptr[7] >= 2500            # the hub's row
    else:
        assert (np.diff(ref.indptr)[100:120] == 0).all()        # nothing lists back what lists nothing
