"""Training loop of the reference's baseline (train.py): L1 reconstruction + the quantizer's commitment loss, Adam, GradScaler
under AMP, clip_grad_norm_, a NaN/Inf guard that skips the batch, a 256-row-per-step latent sample bank capped at 8192 rows,
dead-code reseeding, test evaluation and embedding-norm stats at every epoch end, log.csv, ckpt_last.pt / ckpt_best.pt and a
reconstruction grid every samples_every epochs.

The per-batch metrics (loss, rec, vq, q_mse, perplexity, usage, dead), each weighted by the batch size, accumulate in fp64 on
the device; the host reads them once per epoch.  The only per-step host sync is the NaN guard, which the reference's semantics
need (a skipped batch is neither stepped nor counted).
"""
import argparse
import csv
import os
import random
import time
from contextlib import nullcontext

import numpy as np
import torch
import torch.nn.functional as F
import yaml
from torch import amp

from ..scripts.generate_samples import save_image
from .data import load_split
from .model import model_from_config

LOG_HEADER = ["epoch", "split", "loss", "rec", "vq", "q_mse", "perplex", "usage", "dead", "embed_norm_mean", "embed_norm_min",
              "embed_norm_max"]
METRICS = ["loss", "rec", "vq", "q_mse", "perplex", "usage", "dead"]
MAX_BANK = 8192


def set_seed(seed: int) -> None:
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def load_config(path: str, args=None) -> dict:
    """The reference's config.yaml with its CLI overrides (epochs, batch_size, lr, beta, n_codes, ema_decay)."""
    with open(path, "r") as f:
        cfg = yaml.safe_load(f)
    if args is not None:
        for key, section in (("epochs", "train"), ("batch_size", "train"), ("lr", "train"), ("beta", "model"),
                             ("n_codes", "model"), ("ema_decay", "model")):
            v = getattr(args, key, None)
            if v is not None:
                cfg[section][key] = v
    return cfg


class CSVLogger:
    """Appends rows to a CSV file, writing the header only when the file is new."""

    def __init__(self, path, header):
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        fresh = not os.path.exists(path)
        self.file = open(path, "a", newline="")
        self.writer = csv.writer(self.file)
        if fresh:
            self.writer.writerow(header)
            self.file.flush()

    def log(self, row):
        self.writer.writerow(row)
        self.file.flush()

    def close(self):
        self.file.close()


def _autocast(device, enabled):
    return amp.autocast(device_type="cuda", enabled=enabled) if device.type == "cuda" else nullcontext()


def _batch_metrics(model, loss, loss_rec, loss_vq) -> torch.Tensor:
    """fp64 [7] = loss, rec, vq, q_mse, perplexity, usage, dead of one batch (float32 values widened)."""
    return torch.cat([torch.stack([loss.detach().float(), loss_rec.detach().float(), loss_vq.detach().float()]),
                      model.quant.last_stats.to(loss.device)]).double()


def _finish(acc: torch.Tensor, n: int) -> dict:
    vals = (acc / max(1, n)).tolist()
    out = dict(zip(METRICS, vals))
    out["n"] = n
    return out


def train_one_epoch(model, data, batch_size, opt, scaler, device, grad_clip, sample_bank, max_bank=MAX_BANK):
    model.train()
    acc = torch.zeros(len(METRICS), dtype=torch.float64, device=device)
    n = 0
    for x in data.shuffled_batches(batch_size):
        opt.zero_grad(set_to_none=True)
        with _autocast(device, scaler is not None):
            x_rec, loss_vq, idx, z_q, z_e = model(x)
            loss_rec = F.l1_loss(x_rec, x)
            loss = loss_rec + loss_vq
        with torch.no_grad():
            flat = z_e.detach().permute(0, 2, 3, 1).contiguous().view(-1, z_e.size(1))
            take = min(256, flat.size(0))
            sel = flat[torch.randperm(flat.size(0), device=flat.device)[:take]]
            if sample_bank is None:
                sample_bank = sel
            else:
                sample_bank = torch.cat([sample_bank, sel], dim=0)
                if sample_bank.size(0) > max_bank:
                    sample_bank = sample_bank[-max_bank:]
        stats = _batch_metrics(model, loss, loss_rec, loss_vq)
        if not torch.isfinite(loss):
            opt.zero_grad(set_to_none=True)
            continue
        if scaler is not None:
            scaler.scale(loss).backward()
            if grad_clip and grad_clip > 0:
                scaler.unscale_(opt)
                torch.nn.utils.clip_grad_norm_(model.parameters(), grad_clip)
            scaler.step(opt)
            scaler.update()
        else:
            loss.backward()
            if grad_clip and grad_clip > 0:
                torch.nn.utils.clip_grad_norm_(model.parameters(), grad_clip)
            opt.step()
        bs = x.size(0)
        acc += stats * bs
        n += bs
    return _finish(acc, n), sample_bank


@torch.no_grad()
def evaluate(model, data, batch_size, device, use_amp=True):
    """Per-batch metrics over the split in order, weighted by batch size; AMP on CUDA when use_amp (the training loop's
    evaluation), off for the codebook-metrics CLI."""
    model.eval()
    acc = torch.zeros(len(METRICS), dtype=torch.float64, device=device)
    n = 0
    for x in data.ordered_batches(batch_size):
        with _autocast(device, use_amp):
            x_rec, loss_vq, idx, z_q, z_e = model(x)
            loss_rec = F.l1_loss(x_rec, x)
            loss = loss_rec + loss_vq
        acc += _batch_metrics(model, loss, loss_rec, loss_vq) * x.size(0)
        n += x.size(0)
    return _finish(acc, n)


def embed_norms(model, device):
    norms = torch.linalg.norm(model.quant.embed.to(device), dim=1)
    return norms.mean().item(), norms.min().item(), norms.max().item()


def save_samples(model, data, batch_size, out_dir, epoch):
    os.makedirs(out_dir, exist_ok=True)
    x = next(iter(data.ordered_batches(batch_size)))[:32]
    x_rec = model(x)[0]
    save_image((x_rec.clamp(-1, 1) + 1) / 2, os.path.join(out_dir, f"recon_epoch{epoch:04d}.png"), nrow=8)


def checkpoint_state(model, opt, cfg, epoch) -> dict:
    """The reference's checkpoint layout."""
    return {"model": model.state_dict(), "opt": opt.state_dict(), "cfg": cfg, "epoch": epoch}


def main(argv=None):
    ap = argparse.ArgumentParser(description="Train the baseline EMA VQ-VAE (the reference's train.py)")
    ap.add_argument("--config", type=str, default="config.yaml")
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--batch_size", type=int, default=None)
    ap.add_argument("--lr", type=float, default=None)
    ap.add_argument("--beta", type=float, default=None)
    ap.add_argument("--n_codes", type=int, default=None)
    ap.add_argument("--ema_decay", type=float, default=None)
    ap.add_argument("--out_dir", type=str, default="outputs")
    args = ap.parse_args(argv)
    cfg = load_config(args.config, args)

    set_seed(cfg["seed"])
    if not torch.cuda.is_available():
        raise SystemExit("train_vqvae_baseline needs a GPU: the quantizer runs as HIP kernels")
    device = torch.device("cuda")
    train_data = load_split(cfg, "train", device)
    test_data = load_split(cfg, "test", device)
    bs = cfg["train"]["batch_size"]

    model = model_from_config(cfg).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=cfg["train"]["lr"], weight_decay=cfg["train"]["weight_decay"])
    scaler = amp.GradScaler(enabled=True) if cfg["train"]["amp"] else None

    out = args.out_dir
    ckpt_dir = os.path.join(out, "checkpoints")
    os.makedirs(ckpt_dir, exist_ok=True)
    logger = CSVLogger(os.path.join(out, "log.csv"), header=LOG_HEADER)
    best = float("inf")
    t_all = time.perf_counter()
    sample_bank = None
    epochs = cfg["train"]["epochs"]
    for ep in range(1, epochs + 1):
        t_ep = time.perf_counter()
        tr, sample_bank = train_one_epoch(model, train_data, bs, opt, scaler, device, cfg["train"]["grad_clip"], sample_bank)
        te = evaluate(model, test_data, bs, device)
        n_re = model.quant.reseed_dead_codes(min_count=5, sample_bank=sample_bank)
        if n_re > 0:
            print(f"[epoch {ep}] reseeded {n_re} codes")
        en = embed_norms(model, device)
        logger.log([ep, "train"] + [tr[k] for k in METRICS] + list(en))
        logger.log([ep, "val"] + [te[k] for k in METRICS] + list(en))
        print(f"Epoch {ep}/{epochs} | train loss: {tr['loss']:.4f}, rec: {tr['rec']:.4f}, vq: {tr['vq']:.4f} | "
              f"val loss: {te['loss']:.4f}, rec: {te['rec']:.4f}, vq: {te['vq']:.4f} | time: {time.perf_counter() - t_ep:.2f}s")
        if ep % cfg["log"]["samples_every"] == 0:
            save_samples(model, test_data, bs, out, ep)
        state = checkpoint_state(model, opt, cfg, ep)
        torch.save(state, os.path.join(ckpt_dir, "ckpt_last.pt"))
        if cfg["log"]["save_best"] and te["loss"] < best:
            best = te["loss"]
            torch.save(state, os.path.join(ckpt_dir, "ckpt_best.pt"))
    logger.close()
    print(f"Training finished in {(time.perf_counter() - t_all) / 60:.2f} min. Check {out}/ for results.")
