"""Writes tests/golden/kmeans.npz from the installed scikit-learn: outputs and seeds only, the tests regenerate the inputs
with `make_input`.  A case is admitted only when its result cannot hinge on rounding (asserted, margins stored):
  - seeding: every draw u * pot lies >= 2^-20 * pot from every cumulative-sum boundary, and the best candidate pot is
    >= 2^-20 (relative) below the pot of every candidate whose min array differs from the winner's (equal arrays tie exactly
    everywhere, and the first wins);
  - Lloyd: a float64 scikit-learn run gives the same labels and n_iter as the float32 run (and for the fits from
    random_state the restated centres equal sklearn's: with K above the number of distinct rows, sklearn's float32 means of
    duplicates can round away from the row and trigger a relocation, so that case uses integer rows, 64 copies each, mean 0);
  - and the restatement of the rules in tests/kmeans_rules.py reproduces scikit-learn's indices / labels / n_iter.
The seeding margins are 2^-20 (16 float32 ulps), not 1e-5: a draw lands within eps * pot of one of the N boundaries with
probability about 2 eps N, so at K = 256 (1 785 draws, N >= K) a 1e-5 margin admits about one seed in 10^4, and at d = 128 the
last centres' candidate pots differ by a few 1e-5 relative, routinely below 1e-5 somewhere among 255 steps.  The device's pots
and the restatement's are both float32 of an fp64 sum (at most one float32 ulp apart), sklearn's a float32 BLAS sum; the
restated indices equal sklearn's on every admitted case.

    python tools/gen_golden_kmeans.py        (needs scikit-learn)
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_rules as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kmeans.npz")
DRAW_MARGIN = 2.0 ** -20
POT_MARGIN = 2.0 ** -20


def make_input(kind: str, n: int, d: int, seed: int) -> np.ndarray:
    """The fixture inputs (float32 [n][d])."""
    r = np.random.RandomState(seed)
    if kind == "blobs":
        cen = r.randn(max(n // 50, 4), d) * 4
        return (cen[r.randint(0, len(cen), n)] + r.randn(n, d)).astype(np.float32)
    if kind == "uniform":
        return r.rand(n, d).astype(np.float32)
    if kind == "dups":                      # 5 distinct integer rows {a, b, -a, -b, 0}, n / 5 copies each, shuffled
        a, b = r.randint(-3, 4, size=(2, d)).astype(np.float32)
        base = np.stack([a, b, -a, -b, np.zeros(d, np.float32)])
        return base[r.permutation(np.arange(n) % 5)]
    raise ValueError(kind)


def far_init(X: np.ndarray, K: int, seed: int) -> np.ndarray:
    """K - 1 rows of X plus one centre far from every row: it is empty after the first assignment."""
    r = np.random.RandomState(seed)
    init = X[r.choice(len(X), K, replace=False)].copy()
    init[K // 2] = X.max(axis=0) + 100.0
    return init


def main():
    import sklearn
    from sklearn.cluster import KMeans, kmeans_plusplus
    warnings.simplefilter("ignore")
    out = {"sklearn_version": np.array(sklearn.__version__)}
    # --- seeding: d in {16, 32, 128} x K in {8, 64, 256}
    for d in (16, 32, 128):
        for K in (8, 64, 256):
            n = {8: 2000, 64: 1000, 256: 300}[K]
            L = 2 + int(np.log(K))
            for seed in range(3000):
                X = make_input("blobs", n, d, seed)
                first, u = R.seeding_draws(np.random.RandomState(seed), n, K, 1, L)
                mine, dg, pg = R.kmeans_plusplus(X, K, int(first[0]), u[0])
                if dg < DRAW_MARGIN or pg < POT_MARGIN:
                    continue
                _, idx = kmeans_plusplus(X, K, random_state=seed)
                if np.array_equal(mine, idx):
                    break
            else:
                raise SystemExit(f"no admissible seed for pp d={d} K={K}")
            tag = f"pp_d{d}_K{K}"
            out[tag + "_meta"] = np.array([n, d, K, seed])
            out[tag + "_indices"] = idx.astype(np.int64)
            out[tag + "_margins"] = np.array([dg, pg])
            print(tag, "seed", seed, "draw margin %.2e pot margin %.2e" % (dg, pg))
    # --- Lloyd from a given init: strict, tol, max_iter-capped, empty-cluster relocation
    lloyd_cases = [("strict", "blobs", 3000, 16, 24, 0.0, 300, False), ("tol", "blobs", 3000, 16, 24, 1e-2, 300, False),
                   ("maxiter", "uniform", 3000, 8, 32, 0.0, 4, False), ("relocate", "blobs", 2000, 16, 16, 0.0, 300, True)]
    for name, kind, n, d, K, tol, max_iter, far in lloyd_cases:
        for seed in range(200):
            X = make_input(kind, n, d, seed)
            init = far_init(X, K, seed) if far else X[np.random.RandomState(seed).choice(n, K, replace=False)].copy()
            sk = KMeans(K, init=init, n_init=1, max_iter=max_iter, tol=tol).fit(X)
            sk64 = KMeans(K, init=init.astype(np.float64), n_init=1, max_iter=max_iter, tol=tol).fit(X.astype(np.float64))
            mean = X.mean(axis=0)
            tol_abs = np.mean(np.var(X, axis=0)) * tol if tol else 0
            c, lab, inertia, n_iter, strict, reloc = R.lloyd(X - mean, init - mean, max_iter, float(tol_abs))
            ok = (np.array_equal(sk.labels_, sk64.labels_) and sk.n_iter_ == sk64.n_iter_ and np.array_equal(lab, sk.labels_)
                  and n_iter == sk.n_iter_)
            ok = ok and {"strict": strict and n_iter > 1, "tol": not strict and n_iter < max_iter,
                         "maxiter": n_iter == max_iter and not strict, "relocate": reloc == 1}[name]
            if ok:
                break
        else:
            raise SystemExit(f"no admissible seed for lloyd {name}")
        tag = f"lloyd_{name}"
        out[tag + "_meta"] = np.array([n, d, K, seed, max_iter])
        out[tag + "_kind"] = np.array(kind)
        out[tag + "_tol"] = np.array(tol)
        out[tag + "_labels"] = sk.labels_.astype(np.int32)
        out[tag + "_centers"] = sk.cluster_centers_.astype(np.float32)
        out[tag + "_inertia"] = np.array(sk.inertia_)
        out[tag + "_n_iter"] = np.array(sk.n_iter_)
        print(tag, "seed", seed, "n_iter", sk.n_iter_, "strict", strict, "relocations", reloc)
    # --- full KMeans(n_init=10) from random_state, and K above the number of distinct rows
    full_cases = [("full", "blobs", 4000, 16, 32, 10), ("dups", "dups", 320, 8, 8, 1)]
    for name, kind, n, d, K, n_init in full_cases:
        for seed in range(200):
            X = make_input(kind, n, d, seed)
            sk = KMeans(K, random_state=seed, n_init=n_init).fit(X)
            sk64 = KMeans(K, random_state=seed, n_init=n_init).fit(X.astype(np.float64))
            mine = R.fit(X, K, seed, n_init=n_init)
            ok = (np.array_equal(sk.labels_, sk64.labels_) and sk.n_iter_ == sk64.n_iter_
                  and np.array_equal(mine["labels"], sk.labels_) and mine["n_iter"] == sk.n_iter_
                  and np.allclose(mine["centers"], sk.cluster_centers_, rtol=1e-5, atol=1e-6))
            if ok:
                break
        else:
            raise SystemExit(f"no admissible seed for {name}")
        tag = f"fit_{name}"
        out[tag + "_meta"] = np.array([n, d, K, seed, n_init])
        out[tag + "_kind"] = np.array(kind)
        out[tag + "_labels"] = sk.labels_.astype(np.int32)
        out[tag + "_centers"] = sk.cluster_centers_.astype(np.float32)
        out[tag + "_inertia"] = np.array(sk.inertia_)
        out[tag + "_n_iter"] = np.array(sk.n_iter_)
        out[tag + "_best_start"] = np.array(mine["best_start"])
        print(tag, "seed", seed, "n_iter", sk.n_iter_, "best start", mine["best_start"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
