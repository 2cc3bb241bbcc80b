"""Shared cases and the numpy fp64 oracle of the precision / recall / density / coverage tests (test_prdc_host.py,
test_gpu_prdc.py).  The oracle: keys summed dimension by dimension in fp64, the radius by np.sort, the four definitions of
vqvae_amd/eval/prdc.py.  Each case's oracle is computed once and shared; nobody writes into it."""
import functools

import numpy as np

# (n, m, d, k): reals randn, fakes randn shifted by 0.5 / sqrt(d)
GAUSSIAN = [(2, 2, 1, 1), (65, 63, 3, 5), (300, 257, 129, 5), (1000, 777, 512, 5), (130, 70, 1024, 3), (200, 129, 16, 64)]
NARROW = (500, 400, 32, 5)          # fakes scaled by 0.5, no shift: recall about 0.002, density about 26
# (n, m, d, k, hi): randint(0, hi) as float32 -- every key an exact integer in any summation order, full of key == radius ties
GRID = [(257, 130, 2, 5, 4), (193, 200, 5, 3, 3), (129, 65, 300, 5, 2)]

CASE_IDS = ([f"gauss-{n}x{m}x{d}-k{k}" for n, m, d, k in GAUSSIAN] + ["narrow-500x400x32-k5"]
            + [f"grid-{n}x{m}x{d}-k{k}-hi{hi}" for n, m, d, k, hi in GRID])
GRID_IDS = CASE_IDS[len(GAUSSIAN) + 1:]
MARGIN = 1e-9                       # no compared key of a non-grid case lies within this (relative) of its threshold


def inputs(case_id: str):
    """(real f32 [n, d], fake f32 [m, d], k, exact) of a case; `exact`: keys are integers, compared bit for bit."""
    at = CASE_IDS.index(case_id)
    r = np.random.RandomState(1000 + at)
    if at < len(GAUSSIAN):
        n, m, d, k = GAUSSIAN[at]
        return r.randn(n, d).astype(np.float32), (r.randn(m, d) + 0.5 / np.sqrt(d)).astype(np.float32), k, False
    if at == len(GAUSSIAN):
        n, m, d, k = NARROW
        return r.randn(n, d).astype(np.float32), (0.5 * r.randn(m, d)).astype(np.float32), k, False
    n, m, d, k, hi = GRID[at - len(GAUSSIAN) - 1]
    return r.randint(0, hi, (n, d)).astype(np.float32), r.randint(0, hi, (m, d)).astype(np.float32), k, True


def keys(q: np.ndarray, z: np.ndarray) -> np.ndarray:
    """fp64 keys [len(q), len(z)], one dimension after the other."""
    acc = np.zeros((len(q), len(z)), np.float64)
    q64, z64 = q.astype(np.float64), z.astype(np.float64)
    for c in range(q.shape[1]):
        t = q64[:, c, None] - z64[None, :, c]
        acc += t * t
    return acc


def kth_radius(a: np.ndarray, k: int) -> np.ndarray:
    K = keys(a, a)
    np.fill_diagonal(K, np.inf)                     # self by index: duplicates stay, at key 0
    return np.sort(K, axis=1)[:, k - 1].copy()


def ball_count(z: np.ndarray, r2: np.ndarray, q: np.ndarray):
    """(count int32 [m], near_key f64 [m], near_idx int32 [m], keys [m, n])"""
    K = keys(q, z)
    return ((K <= r2[None, :]).sum(1).astype(np.int32), K.min(1), K.argmin(1).astype(np.int32), K)      # argmin: the first


def _gap(K: np.ndarray, thr: np.ndarray) -> float:
    """smallest relative distance of a key from the threshold it is compared with"""
    scale = np.maximum(np.maximum(np.abs(K), np.abs(thr)), np.finfo(np.float64).tiny)
    return float((np.abs(K - thr) / scale).min())


@functools.lru_cache(maxsize=None)
def oracle(case_id: str) -> dict:
    real, fake, k, exact = inputs(case_id)
    n, m = len(real), len(fake)
    r2_R, r2_F = kth_radius(real, k), kth_radius(fake, k)
    cF, _, _, K_FR = ball_count(real, r2_R, fake)
    cR, near_key, near_idx, K_RF = ball_count(fake, r2_F, real)
    res = {"k": k, "exact": exact, "real_radius2": r2_R, "fake_radius2": r2_F, "fake_count": cF, "real_count": cR,
           "real_near_key": near_key, "real_near_idx": near_idx,
           "precision": int((cF > 0).sum()) / m, "recall": int((cR > 0).sum()) / n,
           "density": int(cF.astype(np.int64).sum()) / (k * m), "coverage": int((near_key <= r2_R).sum()) / n,
           "ties": int((K_FR == r2_R[None, :]).sum() + (K_RF == r2_F[None, :]).sum())}
    # how far every comparison is from flipping: the ball tests, the coverage test, the nearest fake against the runner-up
    two = np.sort(K_RF, axis=1)[:, :2]
    res["gap"] = min(_gap(K_FR, r2_R[None, :]), _gap(K_RF, r2_F[None, :]), _gap(near_key, r2_R),
                     float(((two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], np.finfo(np.float64).tiny)).min()))
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def assert_margin(case_id: str) -> None:
    """A non-grid case must keep every compared key clear of its threshold, so that the oracle's and the kernel's different
    rounding of a key (about d 2^-53 relative) cannot flip a comparison; a grid case must have its exact ties."""
    o = oracle(case_id)
    if o["exact"]:
        assert o["ties"] > 0, (case_id, o["ties"])
    else:
        assert o["gap"] > MARGIN, (case_id, o["gap"])
