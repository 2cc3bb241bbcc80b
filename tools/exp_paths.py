"""Geodesic path extraction and resampling on one MI355X, against the numpy walker.  Writes profiles/geodesic_paths_mi355x.json
(or --out).

The graph is the one the flagship bench configuration builds (60 000 seeded Gaussian latents, d = 16, k = 20, union, pull-back
weights of the seeded train-mode decoder: build_codebook_device, as bench.py's c2).  64 random sources are solved once with
predecessors (sssp_multi_device); 16 384 random (source row, target) pairs are then extracted and resampled:
  - count_fill: paths_from_predecessors_device (geo_sssp_paths_count, the cumsum, geo_sssp_paths_fill and the one host read of
    the total that sizes the outputs);
  - resample: resample_paths_device with 9 frames (the NaN fill and geo_polyline_resample);
  - numpy_walker: tests/path_cases.py extract() on the same P on the host, once -- the reference, not a contestant.
A repetition is the host clock around --inner consecutive calls ending in a device synchronise, divided by the count; three
warm-ups; every repetition is listed.  The device outputs are compared bit for bit with the walker's before anything is timed.

    python tools/exp_paths.py [--out profiles/geodesic_paths_mi355x.json] [--reps 7] [--inner 1000]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import path_cases as pc  # noqa: E402
from vqvae_amd.geo.geo_shortest_paths import (paths_from_predecessors_device, resample_paths_device,  # noqa: E402
                                              sssp_multi_device)
from vqvae_amd.scripts.build_codebook import build_codebook_device  # noqa: E402
from vqvae_amd.spatial_decoder import SpatialDecoder  # noqa: E402

N, D, K_NN, K_CODES, N_SOURCES, N_PAIRS, FRAMES = 60_000, 16, 20, 512, 64, 16_384, 9


def sync_time(f, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def stats(ts):
    return {"s": ts, "s_min": min(ts), "s_median": float(np.median(ts)), "s_max": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geodesic_paths_mi355x.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=1000)   # ~0.1 s per window at ~0.1 ms per call
    ap.add_argument("--n", type=int, default=N, help="latents (the recorded run uses the default)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_paths.py measures on the MI355X; no GPU here")
    dev = torch.device("cuda", 0)
    z = torch.from_numpy(np.random.RandomState(0).randn(args.n, D).astype(np.float32)).to(dev)
    torch.manual_seed(0)
    dec = SpatialDecoder(1, (256, 128, 64), D, 28, "batch").to(dev).train()
    res = build_codebook_device(z, dec, k=K_NN, sym="union", K=min(K_CODES, args.n // 4), init="kpp", seed=42, batch_size=512)
    G = res["W_lcc"]
    z_lcc = z[torch.from_numpy(np.flatnonzero(res["mask_lcc"])).to(dev)].contiguous()      # the graph's nodes, in node order
    r = np.random.RandomState(1)
    sources = np.sort(r.choice(G.n, N_SOURCES, replace=False)).astype(np.int32)
    rows = r.randint(0, N_SOURCES, size=N_PAIRS).astype(np.int32)
    targets = r.randint(0, G.n, size=N_PAIRS).astype(np.int32)
    src_t, rows_t, tgt_t = (torch.from_numpy(a).to(dev) for a in (sources, rows, targets))
    Dm, P, _, _, _ = sssp_multi_device(G, src_t, want_D=True, want_P=True)

    def count_fill():
        return paths_from_predecessors_device(G, P, src_t, rows_t, tgt_t)

    paths = count_fill()

    def resample():
        return resample_paths_device(z_lcc, paths, FRAMES)

    frames = resample()
    indptr, indices, data = (t.cpu().numpy() for t in (G.indptr, G.indices, G.data))
    P_h = P.cpu().numpy()
    t0 = time.perf_counter()
    want = pc.extract(P_h, sources, rows, targets, indptr, indices, data)
    walker_s = time.perf_counter() - t0
    got = tuple(x.cpu().numpy() for x in (paths.nodes, paths.offsets, paths.cum, paths.hops, paths.status))
    for name, g, w in zip(("nodes", "offsets", "cum", "hops", "status"), got, want):
        if not np.array_equal(pc.bits(g) if g.dtype == np.float64 else g, pc.bits(w) if w.dtype == np.float64 else w):
            raise SystemExit(f"{name}: the kernels and the numpy walker differ")
    nodes, offsets, cum, hops, status = got
    ok = status == 0
    last = offsets[1:][ok] - 1
    if not np.array_equal(pc.bits(cum[last].astype(np.float32)), pc.bits(Dm.cpu().numpy()[rows[ok], targets[ok]])):
        raise SystemExit("f32(cum[hops]) differs from the solver's distance")
    some = np.flatnonzero(ok)[:256]
    want_fr = pc.resample(z_lcc.cpu().numpy(), nodes, offsets, cum, FRAMES)[some]
    if not np.array_equal(pc.bits(frames.cpu().numpy()[some]), pc.bits(want_fr)):
        raise SystemExit("resampled frames differ from the numpy rule")

    for _ in range(3):
        count_fill(), resample()
    times = {"count_fill": [], "resample": []}
    for _ in range(args.reps):
        times["count_fill"].append(sync_time(count_fill, args.inner))
        times["resample"].append(sync_time(resample, args.inner))
    h = hops[ok]
    rep = {"device": torch.cuda.get_device_name(0), "graph": {"n": G.n, "nnz": G.nnz, "k": K_NN, "latent_dim": D},
           "sources": N_SOURCES, "pairs": N_PAIRS, "frames": FRAMES, "reps": args.reps, "calls_per_timed_window": args.inner,
           "timing": "host clock around calls_per_timed_window consecutive calls ending in a device synchronise, per call; three "
                     "warm-ups; count_fill includes the cumsum and the one host read of the total path length",
           "hops": {"min": int(h.min()), "median": float(np.median(h)), "mean": float(h.mean()), "max": int(h.max()),
                    "path_nodes_total": int(offsets[-1])},
           "status_counts": [int((status == s).sum()) for s in (0, 1, 2)],
           "count_fill": stats(times["count_fill"]), "resample": stats(times["resample"]),
           "count_fill_resample_s_min": min(times["count_fill"]) + min(times["resample"]),
           "numpy_walker_s": walker_s, "numpy_walker_runs": 1,
           "numpy_walker_over_count_fill_min": walker_s / min(times["count_fill"]),
           "bitwise_equal_to_numpy_walker": True}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=2)
    print(json.dumps({k: v for k, v in rep.items() if k not in ("count_fill", "resample")}))
    print(f"count_fill min {min(times['count_fill']) * 1e3:.3f} ms, resample min {min(times['resample']) * 1e3:.3f} ms, "
          f"numpy walker {walker_s:.2f} s; wrote {args.out}")


if __name__ == "__main__":
    main()
