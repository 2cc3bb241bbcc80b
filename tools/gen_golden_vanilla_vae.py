"""Writes tests/golden/vanilla_vae.npz and tests/golden/legacy_euclidean.npz from the reference (src/models/vae.py and
src/training/build_codebook_legacy.py), on the CPU.  Only inputs and outputs are stored; nothing of the reference's code.

vanilla_vae.npz, for each configuration `c` in CONFIGS (28 px / 1 channel and 32 px / 3 channels, batch norm and none,
enc (8, 16, 32), dec (32, 16, 8), latent_dim 4):
  (all of it computed with ONE torch thread: the CPU transposed convolution's summation order depends on the thread count)
  c/sd/<name>          the reference VAE's state dict after torch.manual_seed(SEED) and two train-mode forwards (so that
                       the batch-norm running statistics are not the initial ones);
  c/x, c/eps           5 input images in [0, 1]; the normal draw of an eval-mode forward after torch.manual_seed(EPS_SEED);
  c/x_logits, c/mu, c/logvar, c/z      that forward's outputs;
  c/triples            float32 [rows][3]: (total, recon, kl) of the reference's loss on those outputs, one row per row of
                       the settings table; c/triples_f64: the same call on the float64 copies of the same float32 values.
settings table (shared): recon_mode (0 bce, 1 mse + sigmoid, 2 mse on logits), free_bits (NaN = None, through
free_bits_default None), beta, capacity_max (0 = off), capacity_anneal_steps, step, capacity_mode (0 abs, 1 clipped).  The
capacity rows take step 0 (target 0: kl above it) and step = capacity_anneal_steps (target capacity_max = 1000: kl below it).

legacy_euclidean.npz: the reference's build_and_save (k=10, sym=union, mode=connectivity, K=16, init=kpp, seed=42) on
  split/      600 latents, d=8: two far-apart blobs and a 5-point island (largest component < N: codes carry -1);
  connected/  300 latents of one blob (connected graph: codes.npy is the assignment array itself).
Stored per case: z, the graph (indptr, indices, data), medoid_indices, z_medoid, codes and the dtype of codes.npy.

    python tools/gen_golden_vanilla_vae.py /path/to/reference/checkout
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED, EPS_SEED, BATCH = 7, 11, 5
CONFIGS = {f"{size}px_{norm}": dict(in_channels=ch, enc_channels=(8, 16, 32), dec_channels=(32, 16, 8), latent_dim=4,
                                   output_image_size=size, norm_type=norm)
           for size, ch in ((28, 1), (32, 3)) for norm in ("batch", "none")}
CAPACITY_MAX, ANNEAL = 1000.0, 100


def settings_table() -> np.ndarray:
    rows = []
    for recon_mode in (0, 1, 2):
        for free_bits in (np.nan, 0.25):
            rows.append((recon_mode, free_bits, 1.0, 0.0, ANNEAL, 0, 0))                           # capacity off
            for mode in (0, 1):
                for step in (0, ANNEAL):
                    rows.append((recon_mode, free_bits, 0.7, CAPACITY_MAX, ANNEAL, step, mode))
    return np.array(rows, dtype=np.float64)


def apply_setting(model, row):
    """Puts a settings row on the model (its loss configuration is plain attributes); returns the loss keyword arguments."""
    recon_mode, free_bits, beta, cmax, anneal, step, mode = row
    model.recon_loss = "bce" if recon_mode == 0 else "mse"
    model.mse_use_sigmoid = recon_mode != 2
    model.free_bits_default = None if np.isnan(free_bits) else float(free_bits)
    return dict(beta=float(beta), capacity_max=float(cmax), capacity_anneal_steps=int(anneal), step=int(step),
                capacity_mode="abs" if mode == 0 else "clipped")


def vae_part(VAE) -> dict:
    torch.set_num_threads(1)                 # torch's CPU transposed convolution sums in an order that depends on the thread count
    out = {"settings": settings_table(), "seed": np.int64(SEED), "eps_seed": np.int64(EPS_SEED)}
    for name, cfg in CONFIGS.items():
        torch.manual_seed(SEED)
        model = VAE(**cfg)
        model.train()
        for _ in range(2):
            model(torch.rand(16, cfg["in_channels"], cfg["output_image_size"], cfg["output_image_size"]))
        model.eval()
        x = torch.rand(BATCH, cfg["in_channels"], cfg["output_image_size"], cfg["output_image_size"])
        torch.manual_seed(EPS_SEED)
        eps = torch.randn(BATCH, cfg["latent_dim"])
        torch.manual_seed(EPS_SEED)
        with torch.no_grad():
            x_logits, mu, logvar, z = model(x)
        assert torch.equal(z, mu + eps * torch.exp(0.5 * logvar))
        for k, v in model.state_dict().items():
            out[f"{name}/sd/{k}"] = v.numpy().copy()
        out.update({f"{name}/x": x.numpy(), f"{name}/eps": eps.numpy(), f"{name}/x_logits": x_logits.numpy(),
                    f"{name}/mu": mu.numpy(), f"{name}/logvar": logvar.numpy(), f"{name}/z": z.numpy()})
        t32, t64 = [], []
        for row in out["settings"]:
            kw = apply_setting(model, row)
            t32.append([float(v) for v in model.loss(x, x_logits, mu, logvar, **kw)])
            t64.append([float(v) for v in model.loss(x.double(), x_logits.double(), mu.double(), logvar.double(), **kw)])
        out[f"{name}/triples"] = np.array(t32, dtype=np.float32)
        out[f"{name}/triples_f64"] = np.array(t64, dtype=np.float64)
        kl = out[f"{name}/triples_f64"][:, 2]
        assert kl.min() > 0 and kl.max() < CAPACITY_MAX, (kl.min(), kl.max())                     # both sides of the target
    return out


def legacy_latents(case: str) -> np.ndarray:
    r = np.random.RandomState(5)
    if case == "connected":
        return r.randn(300, 8).astype(np.float32)
    a = r.randn(330, 8)
    b = r.randn(265, 8) + 40.0
    island = 0.05 * r.randn(5, 8) - 40.0
    return np.concatenate([a, b, island]).astype(np.float32)[r.permutation(600)]


def legacy_config(tmp: str) -> dict:
    return {"data": {"latents_path": os.path.join(tmp, "z.pt")},
            "graph": {"k": 10, "metric": "euclidean", "sym": "union", "mode": "connectivity"},
            "quantize": {"K": 16, "init": "kpp", "seed": 42}, "out": {"dir": os.path.join(tmp, "out")}}


def legacy_part(build_and_save) -> dict:
    out = {}
    for case in ("split", "connected"):
        z = legacy_latents(case)
        with tempfile.TemporaryDirectory() as tmp:
            torch.save(torch.from_numpy(z), os.path.join(tmp, "z.pt"))
            with contextlib.redirect_stdout(io.StringIO()):
                d = build_and_save(legacy_config(tmp))
            W = sparse.load_npz(os.path.join(d, "knn_graph.npz")).tocsr()
            W.sort_indices()
            cb = torch.load(os.path.join(d, "codebook.pt"), weights_only=False)
            codes = np.load(os.path.join(d, "codes.npy"))
        out.update({f"{case}/z": z, f"{case}/indptr": W.indptr, f"{case}/indices": W.indices, f"{case}/data": W.data,
                    f"{case}/medoid_indices": cb["medoid_indices"], f"{case}/z_medoid": cb["z_medoid"].numpy(),
                    f"{case}/codes": codes, f"{case}/codes_dtype": np.array(str(codes.dtype))})
        print(f"{case}: component {W.shape[0]} of {len(z)}, nnz {W.nnz}, codes {codes.dtype}, {int((codes < 0).sum())} unassigned")
    assert (out["split/codes"] < 0).any() and not (out["connected/codes"] < 0).any()
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else None
    if not ref:
        raise SystemExit(__doc__)
    sys.path.insert(0, ref)
    from src.models.vae import VAE
    from src.training.build_codebook_legacy import build_and_save
    for name, part in (("vanilla_vae", vae_part(VAE)), ("legacy_euclidean", legacy_part(build_and_save))):
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(path, **part)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
