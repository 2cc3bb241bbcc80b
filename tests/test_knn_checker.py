"""The exact full-row kNN checker (oracle/knn.py check_knn_lists) on the CPU: it accepts the oracle's own lists in both key
forms and rejects each kind of defect a filtered search could produce.  No GPU and no project code involved."""
import numpy as np
import pytest

from conftest import latents

N, KQ = 3000, 21


def _oracle_lists(z, kq, form):
    import ctypes
    from oracle import _clib
    n, d = z.shape
    io = np.empty((n, kq), np.int64)
    do = np.empty((n, kq), np.float64)
    rc = _clib.lib().oracle_knn(ctypes.c_void_p(z.ctypes.data), n, d, kq, form, 0, n, ctypes.c_void_p(io.ctypes.data),
                                ctypes.c_void_p(do.ctypes.data))
    assert rc == 0
    return io, do


def _data(form):
    """Gaussian latents (d = 16, expansion form / d = 8, direct form) with a group of five identical rows."""
    z = latents(N, 16 if form else 8, 7 + form)
    z[[100, 700, 1300, 1900, 2500]] = z[100]
    return z


@pytest.fixture(scope="module", params=[1, 0], ids=["expansion", "direct"])
def case(request):
    form = request.param
    z = _data(form)
    io, do = _oracle_lists(z, KQ + 1, form)
    return z, form, io, do


def test_accepts_the_oracle_lists(case):
    from oracle.knn import check_knn_lists
    z, form, io, do = case
    st = check_knn_lists(z, io[:, :KQ], do[:, :KQ], KQ, form)
    assert st["rows"] == N and st["flagged_pairs"] >= N * KQ
    check_knn_lists(z, io, do, KQ + 1, form)
    # a row range, screened in blocks of 7 rows
    st = check_knn_lists(z, io[1000:1400, :KQ], do[1000:1400, :KQ], KQ, form, row0=1000, block_bytes=8 * N * 7)
    assert st["block_rows"] == 7


def test_rejects_the_kq_th_neighbour_replaced_by_the_next(case):
    from oracle.knn import check_knn_lists
    z, form, io, do = case
    i, d2 = io[:, :KQ].copy(), do[:, :KQ].copy()
    i[1234, KQ - 1], d2[1234, KQ - 1] = io[1234, KQ], do[1234, KQ]
    with pytest.raises(AssertionError, match=rf"kNN row 1234 .*misses neighbour {io[1234, KQ - 1]}\b"):
        check_knn_lists(z, i, d2, KQ, form)


def test_rejects_a_list_cut_short(case):
    from oracle.knn import check_knn_lists
    z, form, io, do = case
    with pytest.raises(AssertionError, match="shape"):
        check_knn_lists(z, io[:, :KQ - 1], do[:, :KQ - 1], KQ, form)


def test_rejects_a_repeated_index(case):
    from oracle.knn import check_knn_lists
    z, form, io, do = case
    i = io[:, :KQ].copy()
    i[42, KQ - 1] = i[42, KQ - 2]
    with pytest.raises(AssertionError, match="kNN row 42 .*repeated index"):
        check_knn_lists(z, i, do[:, :KQ], KQ, form)


def test_rejects_an_index_out_of_range(case):
    from oracle.knn import check_knn_lists
    z, form, io, do = case
    i = io[:, :KQ].copy()
    i[N - 1, 3] = N
    with pytest.raises(AssertionError, match=rf"kNN row {N - 1} .*outside"):
        check_knn_lists(z, i, do[:, :KQ], KQ, form)


def test_rejects_a_key_one_ulp_off(case):
    from oracle.knn import check_knn_lists
    z, form, io, do = case
    for pos in (0, 7, KQ - 1):                                  # the self key 0, a middle entry, the last one
        d2 = do[:, :KQ].copy()
        r = 2222
        d2[r, pos] = np.nextafter(d2[r, pos], np.inf)
        assert d2[r, pos] != do[r, pos] and (pos == KQ - 1 or d2[r, pos] < d2[r, pos + 1])   # order still holds
        with pytest.raises(AssertionError, match=rf"kNN row {r} .*key of neighbour {io[r, pos]} \(position {pos}\)"):
            check_knn_lists(z, io[:, :KQ], d2, KQ, form)


def test_rejects_tied_indices_out_of_index_order(case):
    from oracle.knn import check_knn_lists
    z, form, io, do = case
    r = 700                                                     # one of the five identical rows: keys 0 at positions 0 .. 4
    assert (do[r, :5] == 0).all() and io[r, :5].tolist() == [100, 700, 1300, 1900, 2500]
    i = io[:, :KQ].copy()
    i[r, [1, 2]] = i[r, [2, 1]]
    with pytest.raises(AssertionError, match=rf"kNN row {r} .*not ordered"):
        check_knn_lists(z, i, do[:, :KQ], KQ, form)


def test_rejects_a_neighbour_dropped_at_a_near_tie():
    """Far from the origin (|x|^2 ~ 1.6e7) two corpus rows sit at the same exact distance from a query row, on different
    axes: their keys tie or differ by rounding only, far inside the screening margin.  Keeping the later one and dropping
    the earlier must be caught by the exact re-evaluation, in both forms."""
    from oracle.knn import check_knn_lists, knn_pair_keys
    for form, d in ((1, 16), (0, 8)):
        z = (latents(N, d, 11) + np.float32(1000.0)).astype(np.float32)
        q = 500
        a, b = 1500, 2600                                       # a < b: (key, index) puts a first on a tie
        z[a] = z[q]
        z[b] = z[q]
        z[a, 0] += np.float32(0.0078125)                        # exactly representable offsets, same length, other axes
        z[b, 1] += np.float32(0.0078125)
        io, do = _oracle_lists(z, 3, form)
        assert io[q].tolist() == [q, a, b]
        keys = knn_pair_keys(z, np.array([q, q]), np.array([a, b]), form)
        margin = 16.0 * (d + 2) * 2.0 ** -53 * 2 * float(np.dot(z[q].astype(np.float64), z[q]))
        assert abs(keys[0] - keys[1]) < margin                  # indistinguishable for the screen alone
        check_knn_lists(z, io[:, :2], do[:, :2], 2, form)
        i, d2 = io[:, :2].copy(), do[:, :2].copy()
        i[q, 1], d2[q, 1] = b, do[q, 2]
        with pytest.raises(AssertionError, match=rf"kNN row {q} .*misses neighbour {a}\b"):
            check_knn_lists(z, i, d2, 2, form)


def test_pair_keys_equal_the_oracle_search_keys(case):
    from oracle.knn import knn_pair_keys
    z, form, io, do = case
    qi = np.repeat(np.arange(N), KQ + 1)
    keys = knn_pair_keys(z, qi, io.ravel(), form)
    np.testing.assert_array_equal(keys.view(np.int64), do.ravel().view(np.int64))
    with pytest.raises(RuntimeError):
        knn_pair_keys(z, np.array([0]), np.array([N]), form)
