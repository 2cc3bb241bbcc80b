"""Timing of bridge_components_device (bridging the components of a kNN graph) next to its yardsticks.

    python tools/exp_bridge.py --out profiles/bridge_mi355x.json

Per shape (n x d standard normal latents, sym, k): the connectivity graph as build_codebook_device builds it, then
  - knn_stage: knn_graph_device + upper_edges_device, the calls build_codebook_device's "knn" timer brackets (flag off: the
    code of a build that never heard of the flag);
  - bridge: bridge_components_device on that graph (components, one nearest-foreign scan per round, insertion), and its share
    of knn_stage;
  - components: connected_components_device alone -- all the flag adds to a build whose graph is connected (C == 1);
  - scan: nearest_foreign_device on the first round's queries (the nodes outside the largest component) and, as the yardstick of
    the inner loop, knn_search_device's exact fp64 scan (option knn_filter = 0) over the same number of query rows, both as
    fp64 FMA/s = rows x n x padded d / time (both calls include the preparation of the corpus);
  - torch: what a user would write today -- fp64 torch.cdist in row blocks, own component masked with +inf, argmin -- on at most
    1 024 of those queries, scaled linearly to all of them and labelled as extrapolated.
One warm-up each, then five repeats bracketed by device synchronisation; median and spread (max - min) in milliseconds.
Prints the DESIGN.md table at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(60000, 16, "union", 20), (60000, 16, "mutual", 10), (960000, 16, "mutual", 10), (800000, 32, "mutual", 10)]
REPEATS = 5
TORCH_QUERIES = 1024


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(fn, repeats=REPEATS):
    timed(fn)                                                      # warm-up: workspace allocation, code object load
    ms = [timed(fn) for _ in range(repeats)]
    return {"median_ms": float(np.median(ms)), "spread_ms": float(max(ms) - min(ms)), "runs_ms": [float(x) for x in ms]}


def torch_nearest_foreign(z, labels, rows, block=128):
    """fp64 cdist in row blocks, own component masked, argmin (ties: torch's first minimum)."""
    z64 = z.double()
    out_i, out_k = [], []
    for r0 in range(0, rows.numel(), block):
        r = rows[r0:r0 + block].long()
        D = torch.cdist(z64[r], z64)
        D = D.masked_fill(labels[r][:, None] == labels[None, :], float("inf"))
        k, i = D.min(dim=1)
        out_i.append(i)
        out_k.append(k * k)
    return torch.cat(out_i), torch.cat(out_k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/bridge_mi355x.json")
    ap.add_argument("--shapes", type=int, nargs="*", default=None, help="indices into SHAPES (default: all)")
    args = ap.parse_args()
    from vqvae_amd import _lib
    from vqvae_amd._device import device
    from vqvae_amd.geo.knn_graph_optimized import (bridge_components_device, connected_components_device, knn_graph_device,
                                                   knn_search_device, nearest_foreign_device, upper_edges_device)
    lib = _lib.load()
    dev = device()
    results = {"device": torch.cuda.get_device_name(dev), "repeats": REPEATS, "shapes": []}
    for si, (n, d, sym, k) in enumerate(SHAPES):
        if args.shapes is not None and si not in args.shapes:
            continue
        z = torch.randn(n, d, generator=torch.Generator(device="cpu").manual_seed(n + d + k)).to(dev)
        dp = 8 if d <= 8 else (16 if d <= 16 else (d + 31) // 32 * 32)

        def knn_stage():
            G, _, _ = knn_graph_device(z, k, mode="connectivity", sym=sym, need_dist=False)
            upper_edges_device(G)
            return G

        G = knn_stage()
        C, labels = connected_components_device(G)
        sizes = torch.bincount(labels.long(), minlength=C)
        G2, edges, keys, info = bridge_components_device(G, z)
        entry = {"latents": [n, d], "sym": sym, "k": k, "components": C, "largest": int(sizes.max()), "rounds": info["rounds"],
                 "queries_first_round": info["queries_first_round"], "queries_all_rounds": info["queries"],
                 "knn_stage": stats(knn_stage), "components_call": stats(lambda: connected_components_device(G)),
                 "bridge": stats(lambda: bridge_components_device(G, z))}
        entry["bridge_share_of_knn_stage"] = entry["bridge"]["median_ms"] / entry["knn_stage"]["median_ms"]
        if C > 1:
            big = int(torch.argmax(sizes))
            rows = torch.nonzero(labels != big).flatten().to(torch.int32)
            m = int(rows.numel())
            entry["scan"] = stats(lambda: nearest_foreign_device(z, labels, rows))
            entry["scan_fma_per_s"] = m * n * dp / (entry["scan"]["median_ms"] * 1e-3)
            lib.geo_set_option(b"knn_filter", 0)
            entry["knn_exact_same_rows"] = stats(lambda: knn_search_device(z, k + 1, 0, m))
            lib.geo_set_option(b"knn_filter", 1)
            entry["knn_exact_fma_per_s"] = m * n * dp / (entry["knn_exact_same_rows"]["median_ms"] * 1e-3)
            sub = rows[:TORCH_QUERIES].contiguous()
            entry["torch_cdist_queries"] = int(sub.numel())
            entry["torch_cdist"] = stats(lambda: torch_nearest_foreign(z, labels, sub), repeats=3)
            entry["torch_cdist_extrapolated_ms"] = entry["torch_cdist"]["median_ms"] * m / sub.numel()
            entry["torch_over_scan_extrapolated"] = entry["torch_cdist_extrapolated_ms"] / entry["scan"]["median_ms"]
        print(json.dumps(entry), flush=True)
        results["shapes"].append(entry)
        del z, G, G2, labels
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print("| latents | graph | components | queries (round 1 / all) | rounds | kNN stage ms | bridge ms (share) | components call ms "
          "| scan GFMA/s | exact kNN scan GFMA/s | torch cdist ms (extrapolated) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for e in results["shapes"]:
        sc = (f"{e['scan_fma_per_s'] / 1e9:.0f} | {e['knn_exact_fma_per_s'] / 1e9:.0f} | {e['torch_cdist_extrapolated_ms']:.0f}"
              if "scan" in e else "- | - | -")
        print(f"| {e['latents'][0]} x {e['latents'][1]} | {e['sym']} k={e['k']} | {e['components']} | {e['queries_first_round']} / "
              f"{e['queries_all_rounds']} | {e['rounds']} | {e['knn_stage']['median_ms']:.2f} +- {e['knn_stage']['spread_ms']:.2f} | "
              f"{e['bridge']['median_ms']:.2f} +- {e['bridge']['spread_ms']:.2f} ({100 * e['bridge_share_of_knn_stage']:.1f} %) | "
              f"{e['components_call']['median_ms']:.2f} +- {e['components_call']['spread_ms']:.2f} | {sc} |")


if __name__ == "__main__":
    main()
