"""Cell-restricted k-medoids refinement (fit_kmedoids_voronoi_graph, csrc/cell.hip) on the bench's workloads.

c2 (60 000 x 16, K = 512): wall time from the seeded codebook to the refined one, max_iter = 10, on the new route
(refine_voronoi_graph: no matrix) and on the matrix route (all_pairs_geodesic_device + the rounds of fit_kmedoids_voronoi,
forming the matrix included), in one process: one warm-up run each, then alternating runs, medians; both final objectives.
real (960 000 x 16, K = 512) and c4 (1 000 000 x 16, K = 1024): the matrix route does not exist there (all_pairs_geodesic_device
stops at about 230 000 nodes), so only the new route: per round the time of the update and of the re-assignment, sweeps, cells
per route, kept cells, and the objective history.  Host clock around calls that end in a synchronise (geo_cell_costs
synchronises; the rounds are host-driven, so wall time is what a user waits for).

    python tools/exp_voronoi_graph.py [out.json] [workloads, comma separated: c2,real,c4] [max_iter at the large sizes]
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


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "voronoi_graph.json")
    names = (sys.argv[2] if len(sys.argv) > 2 else "c2,real,c4").split(",")
    large_iters = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    import bench
    from vqvae_amd._device import device
    from vqvae_amd.geo import kmeans_optimized as KO
    from vqvae_amd.geo.geo_shortest_paths import all_pairs_geodesic_device
    from vqvae_amd.scripts.build_codebook import build_codebook_device
    dev = device()
    quiet = io.StringIO()
    summary = {"what": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(dev), "workloads": {}}
    if os.path.exists(out_path):                                  # a run of some workloads keeps the others' entries
        with open(out_path) as f:
            summary["workloads"] = json.load(f).get("workloads", {})

    def wall(fn):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        with contextlib.redirect_stdout(quiet):
            res = fn()
        torch.cuda.synchronize(dev)
        return 1e3 * (time.perf_counter() - t), res

    def timed_rounds(G, med0, max_iter, power=2):
        """The rounds of refine_voronoi_graph with the two halves of a round timed apart."""
        med = torch.from_numpy(np.asarray(med0, dtype=np.int32)).to(dev)
        dmin, assign = KO._assign_device(G, np.asarray(med0))
        history, rounds = [KO._objective(dmin, power)], []
        for _ in range(max_iter):
            step = {}
            in_cell = torch.where(torch.isfinite(dmin), assign, torch.full_like(assign, -1))
            sizes = torch.bincount(in_cell[in_cell >= 0].long(), minlength=len(med0))
            ms_u, (new, _) = wall(lambda: KO.cell_medoid_update_device(G, in_cell, med, power, info=step))
            step.update(update_ms=ms_u, largest_cell=int(sizes.max()), distance_entries=int((sizes * sizes).sum()),
                        moved=int((new != med).sum()))
            rounds.append(step)
            if step["moved"] == 0:
                break
            ms_a, (dmin_new, assign_new) = wall(lambda: KO._assign_device(G, new.cpu().numpy()))
            step.update(assign_ms=ms_a, objective=KO._objective(dmin_new, power))
            if not step["objective"] < history[-1]:
                step["rejected"] = True
                break
            med, dmin, assign = new, dmin_new, assign_new
            history.append(step["objective"])
        return history, rounds

    for name in names:
        z, dec, cfg = bench.make_inputs(name, dev)
        with contextlib.redirect_stdout(quiet):
            res = build_codebook_device(z, dec, k=cfg["k"], sym="union", K=cfg["K"], init="kpp", seed=42, batch_size=512)
        G, med0 = res["W_lcc"], res["medoids"]
        entry = {"nodes": G.n, "entries": G.nnz, "K": cfg["K"], "seeded_qe": res["qe"]}
        del res, dec, z
        if name == "c2":
            def new_route():
                return KO.refine_voronoi_graph(G, med0, 10, 2)

            def matrix_route():
                D = all_pairs_geodesic_device(G)
                med = torch.from_numpy(np.asarray(med0, dtype=np.int32)).to(dev)
                dmin, assign = KO.assign_from_rows_device(D, med)
                history = [KO._objective(dmin, 2)]
                for _ in range(10):
                    new, _ = KO.medoid_update_device(D, assign, med, 2)
                    if bool((new == med).all()):
                        break
                    med = new
                    dmin, assign = KO.assign_from_rows_device(D, med)
                    history.append(KO._objective(dmin, 2))
                return med, history

            fns = {"cell_restricted": new_route, "matrix": matrix_route}
            times, last = {k_: [] for k_ in fns}, {}
            for fn in fns.values():
                wall(fn)                                          # warm-up: code objects, workspaces, the 14 GB matrix buffer
            for block in range(4):
                for key, fn in (list(fns.items()) if block % 2 == 0 else list(fns.items())[::-1]):
                    ms, last[key] = wall(fn)
                    times[key].append(ms)
            entry["seed_to_refined_ms"] = {k_: {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}
                                           for k_, v in times.items()}
            entry["ratio_matrix_over_cell_restricted"] = (statistics.median(times["matrix"]) /
                                                          statistics.median(times["cell_restricted"]))
            entry["history"] = {"cell_restricted": last["cell_restricted"][3], "matrix": last["matrix"][1]}
            entry["guard_fired"] = bool(last["cell_restricted"][5])
            del last
        iters = 10 if name == "c2" else large_iters
        timed_rounds(G, med0, 1)                                  # warm-up of this size: code objects, workspace allocation
        history, rounds = timed_rounds(G, med0, iters)
        entry.update(max_iter=iters, rounds=rounds, objective_history=history,
                     compared_against=("matrix route, above" if name == "c2" else
                                       "nothing: no other refinement exists at this size (the all-pairs matrix does not fit)"))
        summary["workloads"][name] = entry
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(summary, f, indent=1)
        print(json.dumps({name: entry}), flush=True)
        del G
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
