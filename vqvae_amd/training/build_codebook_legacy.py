"""Euclidean-graph codebook over VECTOR latents of the vanilla VAE, resident on the MI355X.

Drop-in for the reference's legacy builder (src/training/build_codebook_legacy.py: `build_and_save(config)` and its
`__main__`), which the two vanilla/euclidean pipelines call: same YAML keys and fall-backs, same artefacts -- knn_graph.npz
(the graph of the largest component), codebook.pt with medoid_indices / z_medoid / config, codes.npy -- pinned by
tests/golden/legacy_euclidean.npz, the reference's own output.

The steps are the Riemannian builder's without the re-weighting: kNN graph of the latents (graph.k / metric / sym / mode),
connectivity report, compaction to the largest component, geodesic k-medoids (quantize.K / init / seed) on the kNN weights.
The graph stays in HBM between the kNN search and k-medoids; configuration parsing, `read_latents` and
`connectivity_report` are the Riemannian builder's.

A quirk of the reference, kept: with a connected graph codes.npy is k-medoids' own assignment array (whatever integer type
it has); otherwise it is an int32 array holding -1 outside the largest component.
"""
import argparse
from pathlib import Path
from typing import Dict, Optional

import numpy as np
import torch
from scipy import sparse

from .._device import device
from ..geo.kmeans_optimized import fit_kmedoids_optimized
from ..geo.knn_graph_optimized import compact_device, knn_graph_device
from .build_riemannian_codebook_legacy import GraphJob, connectivity_report, read_latents


def build_and_save(config: Dict, dev: Optional[torch.device] = None) -> Path:
    job = GraphJob.from_config(config)
    job.out_dir.mkdir(parents=True, exist_ok=True)
    dev = dev or device()

    z_host = read_latents(job.latents)
    N, D = z_host.shape
    print(f"Loaded latents: N={N}, D={D}")
    z = z_host.contiguous().to(dev)

    print(f"Building k-NN graph: N={N}, k={job.k}, method=hip")
    G, _, _ = knn_graph_device(z, job.k, mode=job.graph_mode, sym=job.sym, metric=job.metric)
    _, mask = connectivity_report(G)
    n_lcc = int(mask.sum())
    if n_lcc < N:
        print(f"Using LCC: {n_lcc}/{N} nodes")
        G, _ = compact_device(G, mask, drop_zero=False)
        z_lcc = z[mask]
    else:
        z_lcc = z
    sparse.save_npz(job.out_dir / "knn_graph.npz", G.to_scipy())

    medoids, assign_lcc, qe = fit_kmedoids_optimized(G, K=job.K, init=job.init, seed=job.seed)
    codes = assign_lcc
    if n_lcc < N:
        codes = np.full(N, -1, dtype=np.int32)
        codes[mask.cpu().numpy()] = assign_lcc
    torch.save({"medoid_indices": medoids.astype(np.int32),
                "z_medoid": z_lcc[torch.from_numpy(medoids).to(dev)].float().cpu(), "config": config},
               job.out_dir / "codebook.pt")
    np.save(job.out_dir / "codes.npy", codes)
    print(f"Quantization error: {qe:.3f}")
    print(f"Saved artifacts to: {job.out_dir}")
    return job.out_dir


if __name__ == "__main__":
    import yaml
    cli = argparse.ArgumentParser()
    cli.add_argument("--config", type=str, default="configs/quantize.yaml")
    with open(cli.parse_args().config, "r") as fh:
        print(f"Completed: {build_and_save(yaml.safe_load(fh))}")
