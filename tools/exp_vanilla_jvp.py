"""Pull-back edge lengths of the eval-mode vanilla VAE decoder on one MI355X: the native route (csrc/vanilla_jvp.hip) against
the autograd route it replaces, alternating in one process, at the two shapes of the legacy Riemannian builder on a
FashionMNIST-shaped decoder (dec_channels 256-128-64, latent_dim 128, 28 px, eval-mode BatchNorm):

    subset   5 000 stored entries of a 20 000-node k = 20 union graph (the reference's default riemannian.max_edges)
    full     every stored entry of that graph (native: each undirected edge once; autograd: every entry, as the parent did)

Times are host clocks around work that ends in a device synchronise; every repetition is reported (the spread is the
run-to-run noise).  Writes profiles/vanilla_jvp_mi355x.json (or --out).

    python tools/exp_vanilla_jvp.py [--nodes 20000] [--reps 5] [--full-autograd-reps 2] [--out FILE]
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

from vqvae_amd.geo import riemannian_metric as rm  # noqa: E402
from vqvae_amd.geo.knn_graph_optimized import knn_graph_device, upper_edges_device  # noqa: E402
from vqvae_amd.training.build_riemannian_codebook_legacy import entry_rows  # noqa: E402
from vqvae_amd.vae import Decoder  # noqa: E402
from vqvae_amd.vanilla_decoder import VanillaDecoderExport  # noqa: E402

MFMA_F32_FLOPS = 157.3e12        # f32 matrix peak (MI355X_MICROARCH.md)
CHANNELS, D, C, SIZE = (256, 128, 64), 128, 1, 28


def flop_model(n_points, n_edges):
    """Multiply-adds x 2 of the native route: per point front + ConvT2 + ConvT3, per edge the front once and ConvT2 + ConvT3
    at both ends."""
    c1, c2 = CHANNELS[1], CHANNELS[2]
    s1, s2 = SIZE // 4, SIZE // 2
    front = 2 * s1 * s1 * c1 * D
    conv2 = 2 * s2 * s2 * c2 * 4 * c1
    conv3 = 2 * SIZE * SIZE * C * 4 * c2
    return n_points * (front + conv2 + conv3) + n_edges * (front + 2 * (conv2 + conv3))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def autograd_route(dec, z_start, z_end, batch_size=512):
    """The parent's route for this decoder: chunks of batch_size through torch.autograd.functional.jvp at both ends."""
    delta = z_end - z_start
    pieces = [0.5 * (rm._generic_jvp_norms(dec, z_start[lo:lo + batch_size], delta[lo:lo + batch_size])
                     + rm._generic_jvp_norms(dec, z_end[lo:lo + batch_size], delta[lo:lo + batch_size]))
              for lo in range(0, z_start.size(0), batch_size)]
    return torch.cat(pieces).float()


def compare(a, b):
    rel = ((a.double() - b.double()).abs() / b.double().abs()).cpu().numpy()
    return {"within_1e-5": float(np.mean(rel <= 1e-5)), "max_rel": float(rel.max()), "q99_rel": float(np.quantile(rel, 0.99))}


def main():
    cli = argparse.ArgumentParser()
    cli.add_argument("--nodes", type=int, default=20000)
    cli.add_argument("--reps", type=int, default=5)
    cli.add_argument("--full-autograd-reps", type=int, default=2)
    cli.add_argument("--out", default=os.path.join(ROOT, "profiles", "vanilla_jvp_mi355x.json"))
    args = cli.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    dec = Decoder(C, CHANNELS, D, SIZE, "batch")
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.05)
                m.running_var.uniform_(0.02, 0.12)
    dec = dec.to(dev).eval()
    z = torch.randn(args.nodes, D, device=dev)
    G, _, _ = knn_graph_device(z, 20, mode="distance", sym="union", metric="euclidean")
    rows, cols = entry_rows(G), G.indices.long()
    src_u, dst_u, entry_edge = upper_edges_device(G)
    pick = torch.randperm(G.nnz, device=dev, generator=torch.Generator(dev).manual_seed(1))[:5000]
    result = {"device": torch.cuda.get_device_name(0), "decoder": {"dec_channels": CHANNELS, "latent_dim": D, "size": SIZE},
              "nodes": args.nodes, "stored_entries": G.nnz, "undirected_edges": int(src_u.numel()), "shapes": {}}

    def native_subset():
        ex = VanillaDecoderExport(dec, dev)
        return rm.edge_lengths_vanilla_graph_device(ex, z, rows[pick].int(), cols[pick].int())

    def native_full():
        ex = VanillaDecoderExport(dec, dev)
        return rm.edge_lengths_vanilla_graph_device(ex, z, src_u, dst_u)[entry_edge.long()]

    shapes = {"subset": (native_subset, lambda: autograd_route(dec, z[rows[pick]], z[cols[pick]]), args.reps,
                         flop_model(10000, 5000)),
              "full": (native_full, lambda: autograd_route(dec, z[rows], z[cols]), args.full_autograd_reps,
                       flop_model(args.nodes, int(src_u.numel())))}
    for name, (native, autograd, auto_reps, flops) in shapes.items():
        native()                                                       # warm-up of both routes at this shape
        if name == "subset":
            autograd()
        t_nat, t_auto, got, ref = [], [], None, None
        for rep in range(args.reps):                                   # alternating
            t, got = timed(native)
            t_nat.append(t)
            if rep < auto_reps:
                t, ref = timed(autograd)
                t_auto.append(t)
        best = min(t_nat)
        result["shapes"][name] = {
            "native_s": t_nat, "autograd_s": t_auto, "speedup_min_over_min": min(t_auto) / best,
            "model_flops": flops, "fraction_of_f32_matrix_peak": flops / best / MFMA_F32_FLOPS,
            "note": "native time includes the export (fp64 composition on the host) and, in full mode, the gather to entries",
            "native_against_autograd": compare(got, ref)}
        print(name, json.dumps(result["shapes"][name]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
