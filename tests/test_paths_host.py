"""Geodesic paths without a GPU: the ABI of csrc/paths.hip, the numpy restatement (tests/path_cases.py) against the committed
solver fixture, and the argument errors of the host API, which are raised before any GPU call."""
import ctypes

import numpy as np
import pytest
from scipy import sparse

import path_cases as pc
from conftest import csr_from_golden


def test_the_library_exports_the_path_entry_points():
    from vqvae_amd import _lib
    c_p, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    want = {
        "geo_sssp_paths_count": [c_p, i64, i32, c_p, c_p, c_p, i64, i32, i32, c_p, c_p, c_p],
        "geo_sssp_paths_fill": [c_p, i64, i32, c_p, c_p, c_p, i64, i32, c_p, c_p, c_p, c_p, i64, c_p, c_p, c_p],
        "geo_polyline_resample": [c_p, i64, i32, c_p, c_p, c_p, i64, i32, c_p, c_p],
    }
    lib = _lib.load()
    for name, args in want.items():
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args, name


def test_bad_arguments_are_refused_without_a_launch():
    """Pointer and shape checks come first: none of these reaches the HIP runtime, so they run without a GPU."""
    from vqvae_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.geo_sssp_paths_count(p, 4, 1, p, p, p, 1, 4, 4, p, p, None) == -1          # max_hops > n - 1
    assert b"max_hops" in lib.geo_last_error()
    assert lib.geo_sssp_paths_count(p, 3, 1, p, p, p, 1, 4, 3, p, p, None) == -1          # ld < n
    assert lib.geo_sssp_paths_count(None, 4, 1, p, p, p, 1, 4, 3, p, p, None) == -1       # null P
    assert lib.geo_sssp_paths_count(None, 4, 1, None, None, None, 0, 4, 3, None, None, None) == 0   # M == 0: nothing to do
    assert lib.geo_sssp_paths_fill(p, 4, 1, p, p, p, 1, 4, None, p, None, p, 2, p, p, None) == -1   # null indptr
    assert lib.geo_sssp_paths_fill(None, 4, 1, None, None, None, 0, 4, None, None, None, None, 0, None, None, None) == 0
    assert lib.geo_polyline_resample(p, 4, 2, p, p, p, 1, 1, p, None) == -1               # F < 2
    assert b"F=1" in lib.geo_last_error()
    assert lib.geo_polyline_resample(None, 4, 2, None, None, None, 0, 2, None, None) == 0


def test_the_numpy_walker_reproduces_the_golden_distances(golden):
    """Every one of the 8 x 2048 pairs of the committed solve: consecutive path nodes are edges, and the fp64 running sum,
    rounded to float32, is the fixture's distance bit for bit."""
    gk, gs = golden("knn"), golden("sssp")
    W = csr_from_golden(gk, "g16/k20/distance/union", 2048)
    W.sort_indices()
    P, D, sources = gs["g16/P"], gs["g16/D"], gs["g16/sources"]
    n = W.shape[0]
    assert np.isfinite(D).all()
    rows = np.repeat(np.arange(len(sources)), n)
    targets = np.tile(np.arange(n), len(sources))
    nodes, offsets, cum, hops, status = pc.extract(P, sources, rows, targets, W.indptr, W.indices, W.data)
    assert (status == 0).all() and (hops >= 0).all()
    assert np.array_equal(offsets[1:] - offsets[:-1], hops + 1)
    first, last = offsets[:-1], offsets[1:] - 1
    assert np.array_equal(nodes[first], sources[rows]) and np.array_equal(nodes[last], targets)
    assert np.isfinite(cum).all()                                   # +inf would be a hop that is no edge
    assert np.array_equal(pc.bits(cum[last].astype(np.float32)), pc.bits(D.reshape(-1)))
    assert hops.max() > 3 and (hops == 0).sum() == len(sources)


def test_the_walker_tells_the_three_statuses():
    P = np.array([[pc.SENTINEL, 0, 1, 4, 3, pc.SENTINEL, 5, 8, -5, 2]], dtype=np.int32)
    n = 10
    assert pc.walk(P[0], 0, 2, n)[0] == 0 and pc.walk(P[0], 0, 2, n)[1].tolist() == [0, 1, 2]
    assert pc.walk(P[0], 0, 0, n) == (0, pc.walk(P[0], 0, 0, n)[1]) and pc.walk(P[0], 0, 0, n)[1].tolist() == [0]
    assert pc.walk(P[0], 0, 3, n)[0] == 2                            # 3 <-> 4 name each other
    assert pc.walk(P[0], 0, 5, n)[0] == 1 and pc.walk(P[0], 0, 6, n)[0] == 1      # sentinel at the target, and in mid-walk
    assert pc.walk(P[0], 0, 7, n)[0] == 2                            # 8 -> -5
    assert pc.walk(P[0], 0, 9, n, max_hops=2)[0] == 2 and pc.walk(P[0], 0, 9, n, max_hops=3)[0] == 0
    assert pc.walk(np.array([pc.SENTINEL, 2], dtype=np.int32), 0, 1, 2)[0] == 2  # an entry equal to n


def test_resampling_rule_on_a_hand_computed_polyline():
    z = np.array([[0.0], [1.0], [1.0], [3.0]], dtype=np.float32)
    nodes, cum = np.array([0, 1, 2, 3]), np.array([0.0, 1.0, 1.0, 3.0])
    out = pc.resample_one(z, nodes, cum, 7)                           # s = 0, .5, 1, 1.5, 2, 2.5, 3
    assert out[:, 0].tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
    assert pc.resample_one(z, np.array([2]), np.array([0.0]), 3)[:, 0].tolist() == [1.0, 1.0, 1.0]
    assert pc.chord(z, [0], [3], 4)[0, :, 0].tolist() == [0.0, 1.0, 2.0, 3.0]


def test_host_api_argument_errors_come_before_any_gpu_call():
    import torch
    from vqvae_amd.geo import chord_frames_device, geodesic_paths, resample_paths_device
    W = sparse.csr_matrix(np.array([[0, 1, 0], [1, 0, 2], [0, 2, 0]], dtype=np.float32))
    with pytest.raises(ValueError, match="non-empty"):
        geodesic_paths(W, [], [])
    with pytest.raises(ValueError, match="non-empty"):
        geodesic_paths(W, [0], [])
    with pytest.raises(ValueError, match="one target per source"):
        geodesic_paths(W, [0, 1], [2])
    with pytest.raises(ValueError, match="out of range"):
        geodesic_paths(W, [0], [3])
    with pytest.raises(ValueError, match="out of range"):
        geodesic_paths(W, [-4], [1])
    with pytest.raises(ValueError, match="square"):
        geodesic_paths(sparse.csr_matrix(np.ones((2, 3), dtype=np.float32)), [0], [1])
    with pytest.raises(TypeError):
        geodesic_paths(np.ones((3, 3)), [0], [1])
    with pytest.raises(ValueError, match="Negative"):
        geodesic_paths(-W, [0], [1])
    z = torch.zeros(3, 2)
    with pytest.raises(ValueError, match="n_frames"):
        chord_frames_device(z, [0], [1], 1)
    with pytest.raises(ValueError, match="n_frames"):
        resample_paths_device(z, None, 1)
