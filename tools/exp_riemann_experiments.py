"""Measures the Riemannian graph-effects experiment on one MI355X and writes profiles/riemann_experiments.json.

60 000 random latents of width 128, the 256-128-64 vanilla decoder (random weights, eval mode), k = 10 mutual.  Two cases:
  (a) the reference's defaults: subset mode, 5 000 edges, 8 sources;
  (b) --mode full with 512 sources.
Per case, after one warm-up, three timings (host wall clock around a device synchronisation, seconds; every repetition listed)
of the part the experiment adds to graph construction and edge lengths, on the SAME resident graph, sources and lengths:
  new      reweight_edges_symmetric_device (a: geo_csr_set_symmetric; b: the entry gather) + mean_shortest_path_device on both
           graphs (geo_sssp_multi + geo_path_stats, nothing to the host but the per-source sums);
  parent   what the parent commit's public calls compose to: graph to scipy, lil re-weighting, dijkstra_multi_source to the
           host on both graphs, numpy masked mean;
  oracle   (a) only: scipy.sparse.csgraph.dijkstra on both graphs + the same masked mean (the reference's own code path).
Also recorded once per case: the whole riemann_graph_effects call (graph + lengths + everything), and that new and parent agree.

    python tools/exp_riemann_experiments.py [--n 60000] [--out profiles/riemann_experiments.json]
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


def timed(fn, reps=3):
    fn()                                                   # warm-up
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "riemann_experiments.json"))
    ap.add_argument("--skip_oracle", action="store_true")
    args = ap.parse_args()
    from scipy.sparse.csgraph import dijkstra
    from vqvae_amd.geo import dijkstra_multi_source
    from vqvae_amd.geo.experiments import (mean_shortest_path_device, reweight_edges_symmetric_device, riemann_graph_effects)
    from vqvae_amd.geo.knn_graph_optimized import reweight_device, upper_edges_device
    from vqvae_amd.vae import Decoder

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    dec = Decoder(1, (256, 128, 64), 128, 28, "batch").to(dev).eval()
    z = np.random.RandomState(0).randn(args.n, 128).astype(np.float32)
    result = {"device": torch.cuda.get_device_name(0), "n": args.n, "d": 128, "k": 10, "decoder": "256-128-64, batch norm, eval",
              "clock": "time.perf_counter around torch.cuda.synchronize, seconds, every repetition listed", "cases": {}}

    def masked_mean(D):
        v = D[np.isfinite(D) & (D > 0)]
        return float(v.mean()) if v.size else float("inf")

    for name, kw in (("a_reference_defaults", dict(mode="subset", sample_edges=5000, num_sources=8)),
                     ("b_full_512_sources", dict(mode="full", num_sources=512))):
        riemann_graph_effects(z, dec, **kw)                                        # warm-up of the whole call
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = riemann_graph_effects(z, dec, **kw)
        torch.cuda.synchronize()
        whole = time.perf_counter() - t0
        G, src = res["graph_euc"], res["sources"]
        i_sel = torch.from_numpy(res["i_sel"]).to(dev)
        j_sel = torch.from_numpy(res["j_sel"]).to(dev)
        riem = torch.from_numpy(res["riem_lengths"]).to(dev)
        entry_edge = upper_edges_device(G)[2] if kw["mode"] == "full" else None

        def new_path():
            Gr = (reweight_device(G, entry_edge, riem) if entry_edge is not None
                  else reweight_edges_symmetric_device(G, i_sel, j_sel, riem))
            return mean_shortest_path_device(G, src)["mean"], mean_shortest_path_device(Gr, src)["mean"]

        def parent_path():
            W = G.to_scipy()
            L = W.tolil()
            L[res["i_sel"], res["j_sel"]] = L[res["j_sel"], res["i_sel"]] = res["riem_lengths"]
            Wr = L.tocsr()
            return masked_mean(dijkstra_multi_source(W, src)), masked_mean(dijkstra_multi_source(Wr, src))

        def oracle_path():
            W = G.to_scipy()
            L = W.tolil()
            L[res["i_sel"], res["j_sel"]] = L[res["j_sel"], res["i_sel"]] = res["riem_lengths"]
            Wr = L.tocsr()
            return (masked_mean(np.asarray(dijkstra(W, directed=False, indices=src))),
                    masked_mean(np.asarray(dijkstra(Wr, directed=False, indices=src))))

        case = {"settings": kw, "edges_reweighted": int(res["sample_edges"]), "nnz": int(G.nnz),
                "ncomp": int(res["ncomp_euc"]), "lcc_size": int(res["lcc_size_euc"]),
                "mean_sp_euc": res["mean_sp_euc"], "mean_sp_riem": res["mean_sp_riem"], "whole_call_s": whole}
        case["new_s"], got = timed(new_path)
        case["parent_s"], parent = timed(parent_path)
        case["new_vs_parent_rel"] = [abs(a - b) / abs(b) for a, b in zip(got, parent)]
        if name.startswith("a_") and not args.skip_oracle:
            case["oracle_s"], oracle = timed(oracle_path)
            case["new_vs_oracle_rel"] = [abs(a - b) / abs(b) for a, b in zip(got, oracle)]
        result["cases"][name] = case
        print(name, json.dumps(case), flush=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
