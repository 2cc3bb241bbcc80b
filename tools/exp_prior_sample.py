"""ms per generation: (a) the reference algorithm on the GPU -- the repo's Transformer.forward on the growing prefix at every
step + top_k_logits + softmax + multinomial + cat (src/scripts/generate_samples.py:19-31) -- against (b) the KV-cached HIP
decode (vqvae_amd.prior.sample), eager.  Writes profiles/prior_sample_<config>.json (or --out).

    python tools/exp_prior_sample.py [--configs fm100,vanilla100,fm8192] [--only hip] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vqvae_amd.prior import Transformer, sample  # noqa: E402
from vqvae_amd.prior.sampling import top_k_logits  # noqa: E402

CONFIGS = {
    # FashionMNIST spatial: 10 classes x 10 samples, random first token, 15 steps
    "fm100": (dict(num_classes=10, num_tokens=512, embed_dim=256, n_layers=4, n_head=4, max_seq_len=16), 100, False),
    # vanilla: BOS prompt, 1 step
    "vanilla100": (dict(num_classes=10, num_tokens=513, embed_dim=512, n_layers=8, n_head=8, max_seq_len=2), 100, True),
    "fm8192": (dict(num_classes=10, num_tokens=512, embed_dim=256, n_layers=4, n_head=4, max_seq_len=16), 8192, False),
}


@torch.no_grad()
def reference_loop(model, x, steps, temperature, top_k, y):
    model.eval()
    for _ in range(steps):
        logits = model(x, y=y)[:, -1, :] / temperature
        if top_k is not None:
            logits = top_k_logits(logits, top_k)
        ix = torch.multinomial(torch.softmax(logits, dim=-1), num_samples=1)
        x = torch.cat((x, ix), dim=1)
    return x


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="fm100,vanilla100,fm8192")
    ap.add_argument("--only", default="both", choices=["both", "hip", "reference"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in args.configs.split(","):
        cfg, B, vanilla = CONFIGS[name]
        torch.manual_seed(0)
        model = Transformer(**cfg, dropout=0.1).to(dev).eval()
        V, T = cfg["num_tokens"], cfg["max_seq_len"]
        x = torch.full((B, 1), V - 1, dtype=torch.int64, device=dev) if vanilla else torch.randint(0, V, (B, 1), device=dev)
        y = torch.arange(B, device=dev) % cfg["num_classes"]
        steps = T - 1
        res = {"config": name, "model": cfg, "B": B, "steps": steps, "top_k": 50, "temperature": 1.0,
               "device": torch.cuda.get_device_name(dev)}
        if args.only in ("both", "reference"):
            res["a_reference_loop"] = timed(lambda: reference_loop(model, x, steps, 1.0, 50, y), max(3, args.reps // 4))
        if args.only in ("both", "hip"):
            res["b_hip_eager"] = timed(lambda: sample(model, x, steps, 1.0, 50, y), args.reps)
        if "a_reference_loop" in res and "b_hip_eager" in res:
            res["speedup_b_over_a"] = res["a_reference_loop"]["median_ms"] / res["b_hip_eager"]["median_ms"]
        print(json.dumps(res), flush=True)
        if args.only == "both":
            with open(os.path.join(args.outdir, f"prior_sample_{name}.json"), "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
