"""Latent files of the vanilla VAE: the reference's save_latents (src/utils/latents.py) and a resident variant that keeps the
latents on the device, like utils/spatial_latents.py.

These writers call `model(x)`: the torch encoder, the draw of z, and the decoder, whose output is dropped.  Their files are
pinned by fixtures, so they stay as they are; the encoder alone runs natively in vqvae_amd.encode.encode_latents
(DESIGN.md section 18), which scripts/encode_latents.py uses to write the same four files from a checkpoint.  Switching the
writers is a later change, to be argued from the measurements of that section."""
from pathlib import Path
from typing import Iterable

import torch


@torch.no_grad()
def encode_latents_device(model, loader: Iterable, device: torch.device):
    """Runs the VAE in eval mode over `loader` ((x, y) batches); returns (z, mu, logvar, y): the three latent tensors (N, d)
    RESIDENT on `device`, y on the host.  z is a fresh draw per batch, as in the reference (eval mode samples too)."""
    model.eval()
    zs, mus, logvars, ys = [], [], [], []
    for x, y in loader:
        _, mu, logvar, z = model(x.to(device, non_blocking=True))
        zs.append(z), mus.append(mu), logvars.append(logvar), ys.append(y.cpu())
    return torch.cat(zs), torch.cat(mus), torch.cat(logvars), torch.cat(ys)


def save_latents(model, loader: Iterable, device: torch.device, out_dir: Path) -> None:
    """z.pt, mu.pt, logvar.pt (float32 (N, d) CPU tensors) and y.pt in out_dir: the reference's four files."""
    z, mu, logvar, y = encode_latents_device(model, loader, device)
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    torch.save(z.cpu(), out_dir / "z.pt")
    torch.save(mu.cpu(), out_dir / "mu.pt")
    torch.save(logvar.cpu(), out_dir / "logvar.pt")
    torch.save(y, out_dir / "y.pt")
