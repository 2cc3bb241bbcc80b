"""Wall time of vqvae_amd.cluster.KMeans(K, random_state=0, n_init).fit on one MI355X, split into seeding and Lloyd, with the
assignment kernel's matrix-core and HBM bounds; scikit-learn on the same host when it imports.  Writes
profiles/kmeans_<config>.json (or --out).

    python tools/exp_kmeans.py [--configs c60k,c960k1,c960k10,c200k128] [--reps 3] [--sklearn c60k]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vqvae_amd import cluster  # noqa: E402

# name: (N, d, K, n_init)
CONFIGS = {"c60k": (60_000, 16, 512, 10), "c960k1": (960_000, 16, 512, 1), "c960k10": (960_000, 16, 512, 10),
           "c200k128": (200_000, 128, 256, 1)}
MFMA_F32_FLOPS = 155e12      # measured f32-input MFMA peak (MI355X_MICROARCH.md)
HBM_BPS = 6.29e12            # measured float4 copy


def blobs(n, d, k, seed):
    r = np.random.RandomState(seed)
    cen = r.randn(k, d) * 4
    return (cen[r.randint(0, k, n)] + r.randn(n, d)).astype(np.float32)


def run(name, reps, with_sklearn):
    N, d, K, n_init = CONFIGS[name]
    X = blobs(N, d, 40, 0)
    dev = torch.device("cuda", 0)
    times, seed_t, lloyd_t = [], [], []
    km = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        km = cluster.KMeans(K, random_state=0, n_init=n_init).fit(X)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        # the two device phases alone, same inputs
        Xc = torch.from_numpy(X - X.mean(axis=0)).to(dev)
        first, u = cluster.seeding_draws(np.random.RandomState(0), N, K, n_init, cluster.n_local_trials_for(K))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        init, _ = cluster.plusplus_device(Xc, K, first, u)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        tol = float(np.mean(np.var(X, axis=0)) * 1e-4)
        res = cluster.lloyd_device(Xc, init, 300, tol)
        t3 = time.perf_counter()
        seed_t.append(t2 - t1)
        lloyd_t.append(t3 - t2)
    iters = int(res["n_iter"].sum())
    assigns = iters + int((res["strict"] == 0).sum())
    kpad, dpad = (K + 31) // 32 * 32, max(2, 1 << (d - 1).bit_length())
    flops = 2.0 * N * kpad * dpad * assigns
    out = {"config": name, "N": N, "d": d, "K": K, "n_init": n_init, "path": km.path_,
           "fit_s_median": float(np.median(times)), "fit_s_all": times,
           "seeding_s_median": float(np.median(seed_t)), "lloyd_s_median": float(np.median(lloyd_t)),
           "n_iter_per_start": res["n_iter"].tolist(), "assignments": assigns, "fallback_rows": res["n_fallback"],
           "inertia": km.inertia_,
           "assign_mfma_bound_s": flops / MFMA_F32_FLOPS,
           "assign_hbm_bound_s": assigns * N * (4 * d + 4 + 8) / HBM_BPS,
           "device": torch.cuda.get_device_name(0)}
    if with_sklearn:
        try:
            import sklearn
            from sklearn.cluster import KMeans
            t0 = time.perf_counter()
            sk = KMeans(K, random_state=0, n_init=n_init).fit(X)
            out["sklearn_s"] = time.perf_counter() - t0
            out["sklearn_version"] = sklearn.__version__
            out["sklearn_inertia"] = float(sk.inertia_)
            out["sklearn_threads"] = os.environ.get("OMP_NUM_THREADS")
        except ImportError:
            out["sklearn_s"] = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c60k,c960k1,c960k10,c200k128")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sklearn", default="c60k", help="configs also timed with scikit-learn on the CPU")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    sk = set(a.sklearn.split(",")) if a.sklearn else set()
    for name in a.configs.split(","):
        res = run(name, a.reps, name in sk)
        print(json.dumps(res))
        with open(os.path.join(a.out, f"kmeans_{name}.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
