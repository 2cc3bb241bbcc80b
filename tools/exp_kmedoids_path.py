"""K sweep of the k-medoids analysis: fit_kmedoids_path(K_values) against the same fit_kmedoids_optimized calls made one after
the other (the only way to do the sweep without the path), in one process: warm-up, alternating blocks, medians of the wall
time per sweep (host clock around a synchronised call: the chain is host-driven, so wall time is what a user waits for).
Also the solve counts, and the device time of the label scores and of the PCA of the K x N matrix of the largest K.

    python tools/exp_kmedoids_path.py [out.json] [N] [d] [k]       (default: the c2 size, 60 000 x 16, k = 20)
"""
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_VALUES = (64, 128, 256, 512)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "kmedoids_path_exp.json"
    N, d, k = (int(sys.argv[i]) if len(sys.argv) > i else v for i, v in ((2, 60000), (3, 16), (4, 20)))
    from vqvae_amd._device import DeviceCSR, device
    from vqvae_amd.geo import build_knn_graph, fit_kmedoids_path
    from vqvae_amd.geo import kmeans_optimized as KO
    from vqvae_amd.geo.analysis import clustering_scores, distance_feature_pca
    from vqvae_amd.geo.geo_shortest_paths import _pull_structure, sssp_multi_device
    dev = device()
    r = np.random.RandomState(0)
    z = r.randn(N, d).astype(np.float32)
    y = r.randint(0, 10, N).astype(np.int32)
    quiet = io.StringIO()
    with contextlib.redirect_stdout(quiet):
        W, _ = build_knn_graph(z, k=k, metric="euclidean", mode="distance", sym="union")
    G = DeviceCSR.from_scipy(_pull_structure(W, directed=False), dev)
    solves = {}

    def path():
        info = {}
        res = fit_kmedoids_path(G, K_VALUES, init="kpp", seed=42, info=info)
        solves["path"] = info["solves"]
        return res

    def loop():
        total, res = 0, []
        for K in K_VALUES:
            centers, chain = KO._kpp_chain(G, K, 42, absorb_last=True)      # counted the way fit_kmedoids_optimized runs it
            total += chain.solves
        solves["loop"] = total
        return [KO.fit_kmedoids_optimized(G, K=K, init="kpp", seed=42) for K in K_VALUES]

    def wall(fn):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        with contextlib.redirect_stdout(quiet):
            res = fn()
        torch.cuda.synchronize(dev)
        return 1e3 * (time.perf_counter() - t), res

    def loop_timed():
        return [KO.fit_kmedoids_optimized(G, K=K, init="kpp", seed=42) for K in K_VALUES]

    with contextlib.redirect_stdout(quiet):
        loop()                                                              # solve count of the baseline, and warm-up
    fns = {"path": path, "loop": loop_timed}
    times = {name: [] for name in fns}
    for name, fn in fns.items():
        for _ in range(2):
            wall(fn)
    results = {}
    for block in range(7):
        for name, fn in (list(fns.items()) if block % 2 == 0 else list(fns.items())[::-1]):
            for _ in range(3):
                ms, res = wall(fn)
                times[name].append(ms)
                results[name] = res
    same = all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
               for a, b in zip(results["path"], results["loop"]))

    def device_ms(fn, reps=7):
        fn()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    medoids, assign, _ = results["path"][-1]
    a_d, y_d = torch.from_numpy(assign.astype(np.int32)).to(dev), torch.from_numpy(y).to(dev)
    D = sssp_multi_device(G, torch.from_numpy(medoids.astype(np.int32)).to(dev), want_D=True)[0]
    summary = {
        "what": "fit_kmedoids_path vs the per-K fit_kmedoids_optimized loop, wall ms per sweep of K_values; 7 alternating blocks "
                "of 3 sweeps after 2 warm-up sweeps each, medians",
        "graph": f"Euclidean-weight union kNN graph, N={N}, d={d}, k={k} (standard normal latents, the c2 size), edges={G.nnz // 2}",
        "K_values": list(K_VALUES), "init": "kpp", "seed": 42, "results_identical": bool(same),
        "solves": solves,
        "wall_ms": {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)} for name, v in times.items()},
        "label_scores_ms": {"what": f"clustering_scores(assign, labels, K={K_VALUES[-1]}) incl. its host copies, n={N}, 10 classes",
                            "median": device_ms(lambda: clustering_scores(a_d, y_d, K_VALUES[-1], 10))},
        "pca_ms": {"what": f"distance_feature_pca(D [{K_VALUES[-1]}][{N}], 2) incl. numpy eigh of the K x K matrix and the host copy "
                           "of the coordinates", "median": device_ms(lambda: distance_feature_pca(D, 2))},
        "device": torch.cuda.get_device_name(dev),
    }
    with open(out_path, "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
