"""Writes tests/golden/kmeans_edges.npz: the Lloyd update and the seeding on the routes tests/golden/kmeans.npz never takes
(several relocations in one iteration, a donor left empty, d = 1..3 and d that does not divide 256, K above 1024, relocation
ties, n above 2^20, 20 and 64 local trials, segment edges, K = n, several starts in one call).

The method is that of tools/gen_golden_kmeans.py: outputs and seeds only (the tests rebuild the inputs with `lloyd_case`,
`tie_case` and `pp_input`), seeds 0, 1, ... walked and the first admissible one kept, an error when none of the first 200 is.
  - Lloyd: scikit-learn in float32 and in float64 give equal labels and n_iter, tests/kmeans_rules.py gives the same labels
    and n_iter, and the case's stated property holds in the rules' run (its trace).  Stored from scikit-learn float32: labels,
    centres, inertia, n_iter; from the rules: centres (centred frame) and inertia.
  - relocation ties (tie_rows, tie_rounds, zero_keys): scikit-learn takes the far rows with argpartition, so with equal
    distances its pick is arbitrary.  These cases hold THE RULES' RESULT ONLY ("rules_only" = 1): (key descending, row
    ascending).  They are built by hand, not walked; `check_tie_case` asserts that they are what they claim.
  - seeding: the rules' indices equal scikit-learn's, and both margins of kmeans_rules.kmeans_plusplus clear 2^-20; but
    pp_n1100000_d2_K6 needs a draw gap of 2^-28 only: the mean step of its cumulative sum is 1 / n = 9e-7 of the pot, so no seed
    meets 2^-20, while two fp64 summation orders of n non-negative terms differ by at most 2 (n - 1) 2^-53 = 2.4e-10 of the sum,
    a fifteenth of 2^-28.

    python tools/gen_golden_kmeans_edges.py        (needs scikit-learn)
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kmeans_rules as R  # noqa: E402
from gen_golden_kmeans import DRAW_MARGIN, POT_MARGIN, make_input  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kmeans_edges.npz")
SEED_CAP = 200
BIG_N_DRAW_MARGIN = 2.0 ** -28

# name: (n, d, K, recipe, number of far centres, max_iter)
LLOYD_CASES = {
    "reloc3": (600, 5, 12, "far", 3, 300),
    "reloc5_d3_K33": (1000, 3, 33, "far", 5, 300),
    "reloc4_d17_K40": (1500, 17, 40, "far", 4, 300),
    "donor_below": (800, 5, 12, "donor_below", 0, 300),
    "donor_above": (800, 5, 12, "donor_above", 0, 300),
    "K1025_d3": (5000, 3, 1025, "far", 2, 3),
    "K4096_d4": (6144, 4, 4096, "far", 2, 3),                # n = 6 chunks; larger n only slows the rules on the host
    "d1": (3000, 1, 64, "far", 2, 3),
    "d2": (3000, 2, 64, "far", 2, 3),
    "d100": (3000, 100, 64, "far", 2, 3),
    "d127": (3000, 127, 64, "far", 2, 3),
}
TIE_CASES = ("tie_rows", "tie_rounds", "zero_keys")
# name: (n, d, K, n_local_trials or None for sklearn's 2 + int(log K), starts)
PP_CASES = {
    "pp_n1100000_d2_K6": (1_100_000, 2, 6, None, 1),
    "pp_L20": (3000, 3, 12, 20, 1),
    "pp_L64": (3000, 5, 12, 64, 1),
    "pp_n1023": (1023, 1, 5, None, 1),
    "pp_n1024": (1024, 1, 5, None, 1),
    "pp_n1025": (1025, 1, 5, None, 1),
    "pp_K_equals_n": (40, 7, 40, None, 1),
    "pp_multistart": (2000, 16, 8, None, 3),
}


def far_slots(K: int, m: int):
    """The indices of the m far centres: spread over 0..K-1, never the first or the last."""
    return [(j + 1) * K // (m + 1) for j in range(m)]


def lloyd_case(name: str, seed: int):
    """Input, init, max_iter and tol of a Lloyd case (float32 X [n][d] and init [K][d])."""
    n, d, K, recipe, m, max_iter = LLOYD_CASES[name]
    X = make_input("blobs", n, d, seed)
    r = np.random.RandomState(seed)
    if recipe == "far":
        init = X[r.choice(n, K, replace=False)].copy()
        for j, slot in enumerate(far_slots(K, m)):
            init[slot] = X.max(axis=0) + 100.0 + j           # empty after the first assignment
    else:
        X[n // 2] = X.max(axis=0) + 50.0                      # one row far from all the others ...
        rows = r.choice(np.delete(np.arange(n), n // 2), K, replace=False)
        init = X[rows].copy()
        donor, empty = (0, K - 1) if recipe == "donor_below" else (K - 1, 0)
        init[donor] = X[n // 2] + 10.0                        # ... alone in its cluster and the farthest from its centre
        init[empty] = X.min(axis=0) - 1000.0                  # takes that row and leaves the donor empty
    return X, init.astype(np.float32), max_iter, 0.0


def tie_case(name: str):
    """Input (integer valued, to be used as it is: no centring) and init of a relocation-tie case; both run one iteration."""
    r = np.random.RandomState(7)
    if name in ("tie_rows", "tie_rounds"):
        # 96 rows and their negatives (mean exactly 0) around 5 centres; rows 150 and 40 lie exactly 9 from centres 1 and 3
        # along different axes -- keys 81 and 81, above every other key -- and their negatives are centres themselves
        d = 6
        half = r.randint(-3, 4, size=(96, d)).astype(np.float32)
        c1, c3 = half[10].copy(), half[20].copy()
        half[40] = c3 + np.float32(9) * np.eye(d, dtype=np.float32)[4]
        half[54] = -(c1 + np.float32(9) * np.eye(d, dtype=np.float32)[1])      # row 150 = -half[54]
        X = np.concatenate([half, -half])
        far = X.max(axis=0) + 100.0
        # tie_rows: one empty centre, the lower row moves; tie_rounds: two, both move, in row order (equal keys across rounds)
        init = np.stack([half[5], c1, -half[40], c3, -X[150], half[30], far, half[70] if name == "tie_rows" else far + 1])
        return X, init.astype(np.float32)
    if name == "zero_keys":
        # every row is a copy of one of 5 centres but rows 0 and 2; centres 1, 4 and 6 are far from everything
        d = 4
        base = r.randint(-6, 7, size=(5, d)).astype(np.float32) * 4
        X = base[r.permutation(np.arange(240) % 5)]
        X[0] = X[0] + np.float32([1, 0, 0, 0])
        X[2] = X[2] + np.float32([0, 1, 1, 0])                # the third pick is row 1, the lowest with key 0
        far = X.max(axis=0) + 100.0
        init = np.stack([base[0], far, base[1], base[2], far + 1, base[3], far + 2, base[4]])
        return X, init.astype(np.float32)
    raise ValueError(name)


def pp_input(name: str, seed: int):
    n, d, K, L, S = PP_CASES[name]
    return make_input("blobs", n, d, seed), K, (2 + int(np.log(K)) if L is None else L), S


def lloyd_property(name: str, trace: list, K: int):
    """The stated property of a Lloyd case, read from the rules' trace; a description when it holds, else None."""
    recipe, m = LLOYD_CASES[name][3], LLOYD_CASES[name][4]
    it0 = trace[0]
    if recipe == "far":
        if len(it0["moved"]) < m:
            return None
        donors = [mv[1] for mv in it0["moved"]]
        if name == "reloc3" and len(set(donors)) == len(donors):
            return None                                       # reloc3: two of the moved rows share a donor
        return f"{len(it0['moved'])} rows moved in iteration 0, donors {donors}"
    for it, t in enumerate(trace):
        donors = {mv[1] for mv in t["moved"]}
        hit = [e for e in t["left_empty"] if e in donors and (e < t["big"] if recipe == "donor_below" else e > t["big"])]
        if hit:
            return f"iteration {it}: donor {hit[0]} left empty, biggest cluster {t['big']}"
    return None


def check_tie_case(name: str, X: np.ndarray, init: np.ndarray, moved: list):
    """The hand-built tie cases are what their descriptions say (exact keys: the data are small integers)."""
    lab, keys, _ = R.exact_argmin(X, init)
    order = np.lexsort((np.arange(len(X)), -keys))
    rows = [mv[0] for mv in moved]
    empty = [k for k in range(len(init)) if not (lab == k).any()]
    assert [mv[2] for mv in moved] == empty, (moved, empty)
    if name in ("tie_rows", "tie_rounds"):
        assert (X.mean(axis=0) == 0).all()
        a, b, c = order[:3]
        assert keys[a] == keys[b] > keys[c] and lab[a] != lab[b] and a < b, (keys[order[:3]], lab[order[:3]])
        assert rows == ([a] if name == "tie_rows" else [a, b]), rows
    else:
        assert (keys > 0).sum() == 2 and len(empty) == 3
        zero = int(np.nonzero(keys == 0)[0][0])
        assert rows[:2] == list(order[:2]) and rows[2] == zero and zero > 0, rows


def main():
    import sklearn
    from sklearn.cluster import KMeans, kmeans_plusplus
    warnings.simplefilter("ignore")
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name, (n, d, K, recipe, m, max_iter) in LLOYD_CASES.items():
        for seed in range(SEED_CAP):
            X, init, max_iter, tol = lloyd_case(name, seed)
            sk = KMeans(K, init=init, n_init=1, max_iter=max_iter, tol=tol).fit(X)
            sk64 = KMeans(K, init=init.astype(np.float64), n_init=1, max_iter=max_iter, tol=tol).fit(X.astype(np.float64))
            if not (np.array_equal(sk.labels_, sk64.labels_) and sk.n_iter_ == sk64.n_iter_):
                continue
            mean = X.mean(axis=0)
            trace = []
            c, lab, inertia, n_iter, strict, reloc = R.lloyd(X - mean, init - mean, max_iter, tol, trace)
            if not (np.array_equal(lab, sk.labels_) and n_iter == sk.n_iter_):
                continue
            prop = lloyd_property(name, trace, K)
            if prop:
                break
        else:
            raise SystemExit(f"no admissible seed for lloyd {name}")
        tag = f"lloyd_{name}"
        out[tag + "_meta"] = np.array([n, d, K, seed, max_iter])
        out[tag + "_kind"] = np.array("blobs")
        out[tag + "_recipe"] = np.array(recipe if recipe != "far" else f"far{m}")
        out[tag + "_rules_only"] = np.array(0)
        out[tag + "_labels"] = sk.labels_.astype(np.uint16)
        out[tag + "_centers"] = sk.cluster_centers_.astype(np.float32)
        out[tag + "_inertia"] = np.array(sk.inertia_)
        out[tag + "_n_iter"] = np.array(sk.n_iter_)
        out[tag + "_rules_centers"] = c
        out[tag + "_rules_inertia"] = np.array(inertia)
        out[tag + "_relocations"] = np.array(reloc)
        print(tag, "seed", seed, "n_iter", sk.n_iter_, "strict", strict, "relocations", reloc, "|", prop)
    for name in TIE_CASES:
        X, init = tie_case(name)
        trace = []
        c, lab, inertia, n_iter, strict, reloc = R.lloyd(X, init, 1, 0.0, trace)
        tag = f"lloyd_{name}"
        out[tag + "_meta"] = np.array([X.shape[0], X.shape[1], len(init), -1, 1])
        out[tag + "_rules_only"] = np.array(1)
        out[tag + "_labels"] = lab.astype(np.uint16)
        out[tag + "_n_iter"] = np.array(n_iter)
        out[tag + "_rules_centers"] = c
        out[tag + "_rules_inertia"] = np.array(inertia)
        out[tag + "_moved"] = np.array(trace[0]["moved"], dtype=np.int64).reshape(-1, 3)
        check_tie_case(name, X, init, trace[0]["moved"])
        print(tag, "rules only; moved (row, donor, cluster):", trace[0]["moved"])
    for name, (n, d, K, L_, S) in PP_CASES.items():
        draw_margin = BIG_N_DRAW_MARGIN if n > (1 << 20) else DRAW_MARGIN
        for seed in range(SEED_CAP):
            X, K, L, S = pp_input(name, seed)
            first, u = R.seeding_draws(np.random.RandomState(seed), n, K, S, L)
            runs = [R.kmeans_plusplus(X, K, int(first[s]), u[s]) for s in range(S)]
            dg, pg = min(r[1] for r in runs), min(r[2] for r in runs)
            if dg < draw_margin or pg < POT_MARGIN:
                continue
            rs = np.random.RandomState(seed)                   # consecutive seedings of one stream = the starts of one call
            sk = [kmeans_plusplus(X, K, random_state=rs, n_local_trials=L_)[1] for _ in range(S)]
            if all(np.array_equal(r[0], i) for r, i in zip(runs, sk)):
                break
        else:
            raise SystemExit(f"no admissible seed for {name}")
        out[name + "_meta"] = np.array([n, d, K, seed, L, S])
        out[name + "_indices"] = np.stack([r[0] for r in runs]).astype(np.int64)
        out[name + "_margins"] = np.array([dg, pg])
        out[name + "_draw_bound"] = np.array(draw_margin)
        print(name, "seed", seed, "trials", L, "starts", S, "draw margin %.2e pot margin %.2e" % (dg, pg))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
