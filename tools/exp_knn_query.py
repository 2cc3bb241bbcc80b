"""Timing of knn_query_device (held-out queries against a corpus) next to its two baselines.

    python tools/exp_knn_query.py --out profiles/knn_query_mi355x.json

Per shape (corpus n x d, V queries, k = 20): knn_query_device(corpus, queries, 20) and, as baseline 1, the self-search
knn_search_device(corpus, 21, 0, V) over the same number of query rows -- the same kernels on the same number of pairs; the query
call adds the preparation of V query rows and drops the fp64 copy of the corpus.  One warm-up each, then five alternating repeats,
every call bracketed by device synchronisation; median and spread (max - min) in milliseconds.
Baseline 2: attach_neighbors_device (the torch search of assign_codes_geodesic) on the first 1 024 queries of the first shape,
scaled linearly to V and labelled as extrapolated."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(960000, 16, 160000), (800000, 32, 160000), (960000, 16, 256)]
K = 20
REPEATS = 5


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return {"median_ms": float(np.median(ms)), "spread_ms": float(max(ms) - min(ms)), "runs_ms": [float(x) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/knn_query_mi355x.json")
    args = ap.parse_args()
    from vqvae_amd import _lib
    from vqvae_amd._device import device
    from vqvae_amd.geo.knn_graph_optimized import knn_query_device, knn_search_device
    from vqvae_amd.training.assign_codes_val_geodesic import attach_neighbors_device
    lib = _lib.load()
    dev = device()
    results = {"device": torch.cuda.get_device_name(dev), "k": K, "repeats": REPEATS, "shapes": []}
    for n, d, V in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(n + d + V)
        z = torch.randn(n, d, generator=g).to(dev)
        q = torch.randn(V, d, generator=g).to(dev)
        runs = {"query": lambda: knn_query_device(z, q, K), "self": lambda: knn_search_device(z, K + 1, 0, V)}
        paths = {}
        for name, fn in runs.items():                              # warm-up: workspace allocation, code object load
            timed(fn)
            paths[name] = int(lib.geo_knn_last_path())
        ms = {name: [] for name in runs}
        for _ in range(REPEATS):                                   # alternating
            for name, fn in runs.items():
                ms[name].append(timed(fn))
        entry = {"corpus": [n, d], "queries": V, "paths": paths, "knn_query_device": stats(ms["query"]),
                 "self_search_same_rows": stats(ms["self"])}
        entry["query_minus_self_ms"] = entry["knn_query_device"]["median_ms"] - entry["self_search_same_rows"]["median_ms"]
        if (n, d, V) == SHAPES[0]:
            sub = q[:1024].contiguous()
            timed(lambda: attach_neighbors_device(sub, z, K))
            t = [timed(lambda: attach_neighbors_device(sub, z, K)) for _ in range(REPEATS)]
            entry["torch_search_1024_queries"] = stats(t)
            entry["torch_search_extrapolated_ms"] = float(np.median(t)) * V / 1024.0
            entry["torch_over_kernel_extrapolated"] = entry["torch_search_extrapolated_ms"] / entry["knn_query_device"]["median_ms"]
        print(json.dumps(entry), flush=True)
        results["shapes"].append(entry)
        del z, q
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
