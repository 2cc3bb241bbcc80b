"""Writes tests/golden/spatial_vae.npz from the reference's SpatialVAE.loss (src/models/spatial_vae.py), on the CPU.  Only
inputs and outputs are stored; nothing of the reference's code.

Cases (name: batch, image, recon mode; every case has mu, logvar [B, 2, 4, 4] and is run with beta in BETAS):
  bce_28      B = 3, x [3, 1, 28, 28] in [0, 1], BCE with logits
  mse_sig_32  B = 3, x [3, 3, 32, 32] normalised (roughly [-2, 2]), squared error of sigmoid(x_logits)
  mse_log_32  B = 3, the same shapes, squared error of x_logits
  one_28      B = 1, BCE
logvar carries values near +8 and -8 (exp matters) and logits near +-30 (saturated sigmoid); the rest is seeded noise.
Stored per case `c`: c/x, c/x_logits, c/mu, c/logvar (float32), c/recon_mode (0 bce, 1 mse + sigmoid, 2 mse on logits),
c/triples float32 [len(BETAS)][3] = (total, recon, kl), c/triples_f64 = the same call on the float64 copies of the same
float32 values, and the float32 call's gradients of `total`: c/d_x_logits (the same for every beta, stored once) and c/d_mu,
c/d_logvar [len(BETAS)][...].

    python tools/gen_golden_spatial_vae.py /path/to/reference/checkout
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BETAS = (0.0, 0.25, 1.0)
CASES = {"bce_28": (3, 1, 28, 0), "mse_sig_32": (3, 3, 32, 1), "mse_log_32": (3, 3, 32, 2), "one_28": (1, 1, 28, 0)}
MODEL = dict(enc_channels=(4, 8, 8), dec_channels=(8, 8, 8), latent_dim=2, norm_type="batch")


def case_inputs(name: str):
    B, ch, size, mode = CASES[name]
    r = np.random.RandomState(100 + sorted(CASES).index(name))
    x = r.rand(B, ch, size, size) if mode == 0 else 2.0 * r.randn(B, ch, size, size).clip(-1, 1)
    logits = 3.0 * r.randn(B, ch, size, size)
    logits.flat[:4] = [30.0, -30.0, 0.0, -0.0]
    mu = r.randn(B, 2, 4, 4)
    logvar = r.uniform(-3.0, 1.5, (B, 2, 4, 4))
    logvar.flat[:4] = [8.0, -8.0, 7.75, -7.5]
    mu.flat[:2] = [0.0, 0.5]
    return [a.astype(np.float32) for a in (x, logits, mu, logvar)]


def run(model, tensors, beta, dtype):
    x, logits, mu, logvar = (torch.from_numpy(a).to(dtype) for a in tensors)
    leaves = [t.requires_grad_(True) for t in (logits, mu, logvar)]
    total, recon, kl = model.loss(x, leaves[0], leaves[1], leaves[2], beta=beta, step=3)
    total.backward()
    return [float(v.detach()) for v in (total, recon, kl)], [t.grad.numpy() for t in leaves]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else None
    if not ref:
        raise SystemExit(__doc__)
    sys.path.insert(0, ref)
    from src.models.spatial_vae import SpatialVAE
    torch.set_num_threads(1)
    out = {"betas": np.array(BETAS, dtype=np.float64)}
    for name, (B, ch, size, mode) in CASES.items():
        model = SpatialVAE(in_channels=ch, output_image_size=size, recon_loss="bce" if mode == 0 else "mse",
                           mse_use_sigmoid=mode != 2, **MODEL)
        tensors = case_inputs(name)
        t32, t64, grads = [], [], []
        for beta in BETAS:
            triple, g = run(model, tensors, beta, torch.float32)
            t32.append(triple), grads.append(g)
            t64.append(run(model, tensors, beta, torch.float64)[0])
        for key, a in zip(("x", "x_logits", "mu", "logvar"), tensors):
            out[f"{name}/{key}"] = a
        out[f"{name}/recon_mode"] = np.int64(mode)
        out[f"{name}/triples"] = np.array(t32, dtype=np.float32)
        out[f"{name}/triples_f64"] = np.array(t64, dtype=np.float64)
        assert all(np.array_equal(g[0], grads[0][0]) for g in grads)           # beta does not reach x_logits: stored once
        out[f"{name}/d_x_logits"] = grads[0][0]
        for i, key in ((1, "d_mu"), (2, "d_logvar")):
            out[f"{name}/{key}"] = np.stack([g[i] for g in grads])
        print(name, out[f"{name}/triples_f64"].tolist())
    path = os.path.join(GOLDEN, "spatial_vae.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
