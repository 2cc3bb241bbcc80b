"""Every row of csrc/knn.hip's search against the exact checker (oracle/knn.py check_knn_lists), on every path the search can
take.  geo_knn_topk picks its path from the padded dimension dp (8 / 16 / 32 / 64 for the filter), the corpus size, the list
length kq and the knn_filter option; geo_knn_last_path() proves which one ran:
  - exact fp64 scan (below the filter's size threshold, or knn_filter = 0) and exact wide lists (kq > 64);
  - one-level filter: thresholds from every S-th row (S = 16 for kq <= 24, 8 up to 40, 4 above), bf16 hi/lo (knn_filter = 1)
    or float32 (2) matrix-core scan, fp64 refinement and selection of the kq best;
  - two levels (bf16, n >= 200 000): the thresholds themselves from a filtered pass over every S-th row.
The key form follows the dimension as in the product: direct for d <= 15, expansion above."""
import numpy as np
import pytest
import torch

from conftest import latents, swiss_roll_latents

pytestmark = pytest.mark.gpu

EXACT, WIDE, BF16, F32, TWO, OVERFLOW = 1, 2, 3, 4, 5, 16
FILTER_STRIDE = 16                     # csrc/knn.hip: kq <= 24 takes its thresholds from every 16th corpus row, kq > 40 from
#                                        every 4th: rows 16 apart are in the subset either way


def _search(z, kq, filt=1, r0=0, r1=None):
    """(idx, d2, path) of one geo_knn_topk call with the given knn_filter option (restored afterwards)."""
    from vqvae_amd import _lib
    from vqvae_amd._device import device
    from vqvae_amd.geo.knn_graph_optimized import knn_search_device
    lib = _lib.load()
    zt = z if isinstance(z, torch.Tensor) else torch.from_numpy(z).to(device())
    _lib.check(lib.geo_set_option(b"knn_filter", int(filt)), "geo_set_option")
    try:
        idx, d2 = knn_search_device(zt, kq, r0, r1)
        path = lib.geo_knn_last_path()
    finally:
        lib.geo_set_option(b"knn_filter", 1)
    return idx, d2, path


def _check(z, idx, d2, kq, row0=0):
    from oracle.knn import check_knn_lists
    return check_knn_lists(z, idx, d2, kq, 1 if z.shape[1] > 15 else 0, row0=row0, device="cuda")


def _run(z, kq, filt, path, shard=None):
    idx, d2, got = _search(z, kq, filt)
    assert got == path, f"geo_knn_last_path() = {got}, expected {path}"
    _check(z, idx, d2, kq)
    if shard is not None:                                  # a rank's share of the query rows: same path, same rows
        r0, r1 = shard
        i_s, d_s, got = _search(z, kq, filt, r0, r1)
        assert got == path, f"row range: geo_knn_last_path() = {got}, expected {path}"
        assert torch.equal(i_s, idx[r0:r1]) and torch.equal(d_s, d2[r0:r1])
        _check(z, i_s, d_s, kq, row0=r0)
    return idx, d2


# (n, d, kq, knn_filter, path).  Size thresholds of the filter: n >= max(640 000 / dp, 16 384) -- 80 000 (dp 8), 40 000 (dp 16),
# 20 000 (dp 32), 16 384 (dp 64); two levels from 200 000 rows (bf16 scan only).  Every dp x form x levels x {kq <= 21, kq = 64}
# cell appears at least once, the float32 scan in every dp, each size threshold from both sides.
MATRIX = [
    # dp = 8 (d <= 8, direct form; bf16 parts padded to 16 columns)
    (79999, 8, 21, 1, EXACT),
    (80000, 8, 21, 1, BF16),
    (80001, 2, 64, 1, BF16),
    (80000, 3, 1, 2, F32),
    (80017, 8, 64, 2, F32),
    (199999, 8, 2, 1, BF16),
    (200000, 8, 21, 1, TWO),
    (200000, 3, 64, 1, TWO),
    # dp = 16, direct form (d 9 .. 15)
    (39999, 15, 21, 1, EXACT),
    (40000, 9, 63, 1, BF16),
    (40000, 15, 64, 1, BF16),
    (40001, 12, 2, 2, F32),
    (199999, 15, 21, 1, BF16),
    (200000, 15, 21, 1, TWO),
    (200000, 9, 64, 1, TWO),
    # dp = 16, expansion form (d = 16)
    (39999, 16, 64, 1, EXACT),
    (40000, 16, 1, 1, BF16),
    (40000, 16, 64, 2, F32),
    (199999, 16, 64, 1, BF16),
    (200000, 16, 2, 1, TWO),
    (200000, 16, 64, 1, TWO),
    # dp = 32
    (19999, 32, 21, 1, EXACT),
    (20000, 17, 21, 1, BF16),
    (20000, 32, 64, 2, F32),
    (60000, 24, 63, 1, BF16),
    (200000, 17, 64, 1, TWO),
    (200000, 32, 1, 1, TWO),
    # dp = 64
    (16383, 64, 21, 1, EXACT),
    (16384, 33, 2, 1, BF16),
    (16384, 64, 64, 2, F32),
    (50000, 64, 64, 1, BF16),
    (50000, 40, 21, 2, F32),
    (199999, 64, 21, 1, BF16),
    (200000, 64, 64, 1, TWO),
    (200000, 33, 21, 1, TWO),
    # the filter switched off at a size that would take it
    (45000, 16, 21, 0, EXACT),
    # lists longer than one wave at scale: the exact wide kernel (the filter serves kq <= 64)
    (45000, 16, 65, 1, WIDE),
    (45000, 8, 256, 1, WIDE),
    (82000, 33, 128, 1, WIDE),
]


@pytest.mark.parametrize("n,d,kq,filt,path", MATRIX, ids=[f"n{n}-d{d}-k{k}-f{f}" for n, d, k, f, _ in MATRIX])
def test_dispatch_matrix_every_row_exact(n, d, kq, filt, path):
    z = latents(n, d, 1000 + d + kq)
    _run(z, kq, filt, path, shard=(70001, 140777) if path == TWO else None)


def test_swiss_roll_every_row_exact():
    """The bench's second distribution: small neighbour distances against large norms along a thin manifold."""
    z = swiss_roll_latents(60000, 16, 4)
    for kq, filt, path in ((21, 1, BF16), (64, 1, BF16), (21, 2, F32)):
        _run(z, kq, filt, path)


@pytest.mark.parametrize("d,filt", [(8, 1), (24, 1), (24, 2), (64, 1)])
def test_clusters_with_norms_10_4_apart_every_row_exact(d, filt):
    """Clusters whose centres' norms range over four decades (0.01 .. 100): the filter's margin is relative to |x|^2 + |y|^2,
    so it is wide in the far clusters and tight near the origin; spreads proportional to the centre norm (wide enough that
    the candidate lists fit their cap: the filter itself must run)."""
    n = 100000 if d == 8 else 60000
    r = np.random.RandomState(77 + d)
    scales = np.float64(10.0) ** np.linspace(-2, 2, 8)
    centres = r.randn(8, d) / np.sqrt(d) * scales[:, None]
    lab = r.randint(0, 8, size=n)
    z = (centres[lab] + 0.3 * scales[lab, None] * r.randn(n, d) / np.sqrt(d)).astype(np.float32)
    for kq in (21, 64):
        _run(z, kq, filt, BF16 if filt == 1 else F32)


def test_a_few_far_groups_every_row_exact():
    """Gaussian latents plus five groups of 400 rows around centres at |c| = 10^3 .. 10^4: those rows' thresholds and margins
    are 10^6 .. 10^8 times the bulk's, their lists are their own group (400 candidates fit the list of 1 024)."""
    n, d = 90000, 16
    z = latents(n, d, 51)
    r = np.random.RandomState(52)
    for g, s in enumerate((1e3, 3e3, 1e4, 2e3, 5e3)):
        rows = 1000 + 17000 * g + 13 * np.arange(400)
        c = r.randn(d) / np.sqrt(d) * s
        z[rows] = (c + r.randn(400, d)).astype(np.float32)
    for kq, filt, path in ((21, 1, BF16), (64, 2, F32)):
        _run(z, kq, filt, path)


@pytest.mark.parametrize("d,kq", [(16, 21), (8, 64), (64, 64)])
def test_duplicates_a_filter_stride_apart_every_row_exact(d, kq):
    """Groups of identical rows exactly FILTER_STRIDE rows apart: all of them are in the threshold subset, so for their rows
    the subset's kq-th distance -- the threshold -- is 0 and only the margin keeps anything.  40 copies at kq = 21 (more zero
    keys than kq), 100 at kq = 64 (more zero keys than the 64-lane compaction holds)."""
    n = 90000
    z = latents(n, d, 61 + d)
    copies = 40 if kq <= 21 else 100
    for g in range(6):
        rows = FILTER_STRIDE * (100 + 800 * g) + FILTER_STRIDE * np.arange(copies)
        z[rows] = z[rows[0]]
    idx, d2 = _run(z, kq, 1, BF16)
    last = FILTER_STRIDE * 100 + FILTER_STRIDE * (copies - 1)
    np.testing.assert_array_equal(idx[last].cpu().numpy(), FILTER_STRIDE * 100 + FILTER_STRIDE * np.arange(kq))
    assert (d2[last] == 0).all()


@pytest.mark.parametrize("filt,path", [(1, BF16), (2, F32)])
def test_ties_at_the_kq_th_distance_beyond_the_compaction_every_row_exact(filt, path):
    """kq = 64 and rows whose list ends in a tie wider than the 64-lane compaction: 150 copies of a point y near a row x -- x's
    list is x and 63 of the copies, all tied at the kq-th key with 150 entries there; the copies' own lists are 64 of 150 zero
    keys.  The refinement's one-by-one extraction must cut both ties by index."""
    n, d, kq = 50000, 16, 64
    z = latents(n, d, 71)
    xs = (3000, 21000, 37000)
    for x in xs:
        rows = x + 1 + 3 * np.arange(150)
        y = z[x].copy()
        y[0] += np.float32(0.25)
        z[rows] = y
    idx, d2 = _run(z, kq, filt, path)
    for x in xs:
        assert (d2[x, 1:] == d2[x, 1]).all() and (d2[x, 1] > 0)    # the tie fills the list ...
        np.testing.assert_array_equal(idx[x, 1:].cpu().numpy(), x + 1 + 3 * np.arange(kq - 1))   # ... lowest indices first
