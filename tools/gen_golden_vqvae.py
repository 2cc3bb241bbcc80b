"""Writes tests/golden/vqvae_baseline.npz from the reference's baseline VQ-VAE (baseline VQVAE/vqvae_cifar10_clean/models/vqvae.py),
on the CPU in float32.  Only inputs and outputs are stored; nothing of the reference's code.

  - quantizer: VectorQuantizerEMA(n_codes=K, code_dim=C) after torch.manual_seed(SEED), three training-mode forwards on fixed
    random z_e (B x C x H x W) and one eval-mode forward: idx, z_q, z_q_st, loss and all three buffers after each;
  - admission: a seed is taken only when, on every row of every forward, the reference's float32 |x|^2 - 2 x.e + |e|^2 argmin
    equals the fp64 argmin and the fp64 gap between the two best codes exceeds 8 (d + 2) 2^-24 (|x|^2 + max |e|^2), the error
    bound of the float32 expansion (csrc/kmeans.hip), so the change of assignment rule cannot move a label;
  - initial weights: names, shapes and per-tensor SHA-256 of VQVAE(**CIFAR config) right after torch.manual_seed(42).

    python tools/gen_golden_vqvae.py /path/to/reference/checkout
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
K, C, B, H, W = 64, 32, 4, 8, 8
STEPS = 3
CIFAR = dict(in_channels=3, z_channels=128, hidden=256, n_res_blocks=2, n_codes=512, beta=0.25, ema_decay=0.99, ema_eps=1e-5)


def inputs(seed: int) -> np.ndarray:
    """(STEPS + 1) z_e batches float32 [B][C][H][W]: unit normals, scaled like encoder outputs."""
    return (np.random.RandomState(seed).randn(STEPS + 1, B, C, H, W) * 1.5).astype(np.float32)


def state_hashes(sd) -> tuple:
    names = list(sd.keys())
    shapes = np.full((len(names), 4), -1, dtype=np.int64)
    hashes = []
    for i, k in enumerate(names):
        t = sd[k].detach().cpu().contiguous()
        shapes[i, :t.dim()] = t.shape
        hashes.append(hashlib.sha256(t.numpy().tobytes()).hexdigest())
    return np.array(names), shapes, np.array(hashes)


def admitted(z: np.ndarray, embed: np.ndarray) -> bool:
    x = z.transpose(0, 2, 3, 1).reshape(-1, C).astype(np.float64)
    e = embed.astype(np.float64)
    key = ((x[:, None, :] - e[None]) ** 2).sum(-1)
    two = np.sort(key, axis=1)[:, :2]
    bound = 8 * (C + 2) * 2.0 ** -24 * ((x ** 2).sum(1) + (e ** 2).sum(1).max())
    xf, ef = torch.from_numpy(x.astype(np.float32)), torch.from_numpy(embed)
    d32 = (xf ** 2).sum(1, keepdim=True) - 2 * xf @ ef.t() + (ef ** 2).sum(1)
    return bool(np.all(two[:, 1] - two[:, 0] > bound) and np.array_equal(d32.argmin(1).numpy(), key.argmin(1)))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else None
    if not ref:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.join(ref, "baseline VQVAE", "vqvae_cifar10_clean"))
    from models.vqvae import VQVAE, VectorQuantizerEMA
    out = {}
    for seed in range(100, 200):
        torch.manual_seed(seed)
        q = VectorQuantizerEMA(n_codes=K, code_dim=C, decay=0.99, eps=1e-5, beta=0.25)
        out["embed0"] = q.embed.numpy().copy()
        zs = inputs(seed)
        ok = True
        for s in range(STEPS + 1):
            if not admitted(zs[s], q.embed.numpy()):
                ok = False
                break
            q.train(s < STEPS)
            z = torch.from_numpy(zs[s])
            z_q_st, loss, idx, z_q, _ = q(z)
            out[f"idx_{s}"] = idx.numpy()
            out[f"z_q_{s}"] = z_q.numpy()
            out[f"z_q_st_{s}"] = z_q_st.numpy()
            out[f"loss_{s}"] = np.float32(loss.item())
            for b in ("embed", "cluster_size", "embed_avg"):
                out[f"{b}_{s}"] = getattr(q, b).numpy().copy()
        if ok:
            out["seed"] = np.int64(seed)
            out["z_e"] = zs
            break
    else:
        raise SystemExit("no seed admitted")
    torch.manual_seed(42)
    names, shapes, hashes = state_hashes(VQVAE(**CIFAR).state_dict())
    out.update(sd_names=names, sd_shapes=shapes, sd_sha256=hashes)
    out["dims"] = np.array([K, C, B, H, W, STEPS])
    path = os.path.join(GOLDEN, "vqvae_baseline.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes), seed {int(out['seed'])}")


if __name__ == "__main__":
    main()
