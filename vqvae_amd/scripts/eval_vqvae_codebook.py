"""python -m vqvae_amd.scripts.eval_vqvae_codebook --config config.yaml [--ckpt --split train|test --batch_size]: the reference
baseline's eval_codebook_metrics.py.  Loss, rec, vq, q_mse, perplexity, usage and dead over the split in order (no AMP),
weighted by batch size, then the embedding-norm stats; printed, and appended to outputs/codebook_eval_<split>.csv (header
written when the file is new)."""
import argparse
import os

import torch

from ..baseline.data import load_split
from ..baseline.model import model_from_config
from ..baseline.train import embed_norms, evaluate, load_config

CSV_HEADER = ["split", "loss", "rec", "vq", "q_mse", "perplex", "usage", "dead", "embed_norm_mean", "embed_norm_min",
              "embed_norm_max"]


def compute_codebook_metrics(model, data, batch_size, device) -> dict:
    m = evaluate(model, data, batch_size, device, use_amp=False)
    en = embed_norms(model, device)
    out = {k: m[k] for k in ("loss", "rec", "vq", "q_mse", "perplex", "usage", "dead")}
    out.update(embed_norm_mean=en[0], embed_norm_min=en[1], embed_norm_max=en[2])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="Codebook metrics of a baseline VQ-VAE checkpoint")
    ap.add_argument("--config", type=str, default="config.yaml")
    ap.add_argument("--ckpt", type=str, default=os.path.join("outputs", "checkpoints", "ckpt_best.pt"))
    ap.add_argument("--split", type=str, choices=["train", "test"], default="test")
    ap.add_argument("--batch_size", type=int, default=None)
    args = ap.parse_args(argv)
    cfg = load_config(args.config)
    if args.batch_size is not None:
        cfg["train"]["batch_size"] = args.batch_size
    if not torch.cuda.is_available():
        raise SystemExit("eval_vqvae_codebook needs a GPU: the quantizer runs as HIP kernels")
    device = torch.device("cuda")
    model = model_from_config(cfg).to(device)
    if not os.path.isfile(args.ckpt):
        raise FileNotFoundError(f"Checkpoint not found: {args.ckpt}")
    model.load_state_dict(torch.load(args.ckpt, map_location=device)["model"])
    data = load_split(cfg, args.split, device)
    metrics = compute_codebook_metrics(model, data, cfg["train"]["batch_size"], device)

    print(f"Split: {args.split}")
    for k, v in metrics.items():
        print(f"{k}: {v:.6f}")
    out_csv = os.path.join("outputs", f"codebook_eval_{args.split}.csv")
    os.makedirs("outputs", exist_ok=True)
    fresh = not os.path.isfile(out_csv)
    with open(out_csv, "a") as f:
        if fresh:
            f.write(",".join(CSV_HEADER) + "\n")
        row = [args.split] + [metrics[k] for k in CSV_HEADER[1:]]
        f.write(",".join(f"{x}" for x in row) + "\n")
    return metrics


if __name__ == "__main__":
    main()
