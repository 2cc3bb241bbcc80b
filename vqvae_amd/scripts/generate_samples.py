"""Images from the code prior: drop-in for the reference's src/scripts/generate_samples.py.

    python -m vqvae_amd.scripts.generate_samples --config configs/<dataset>/<vae>/<codebook>/generate.yaml

Reads the reference's generate.yaml unchanged (transformer, vae, vanilla_vae, class_labels, samples_per_class, temperature,
top_k, transformer_ckpt_path, vae_ckpt_path, codebook_path, output_dir, output_filename).  Codes are sampled with
vqvae_amd.prior.sample (the KV-cached HIP decode on the GPU), all classes in one call: a row's tokens depend only on its
prompt, its label and its uniforms.  Decoding follows the reference exactly (generate_samples.py:91-97): z_medoid[codes]
(spatial: permuted to a latent_dim x 4 x 4 grid), vae.decoder(...).sigmoid(), one class group at a time.  The reference never
calls vae.eval(), so BatchNorm decoders normalise each class group with its own batch statistics; so do we.

Differences, deliberate: `seed` (present in the yaml, unused by the reference) seeds torch when given; the tokens are drawn
by the draw rule of vqvae_amd/prior/sampling.py, not torch.multinomial's stream; a sampled code outside the codebook (the
vanilla prior can draw its BOS token) is rejected with an error instead of indexing out of range.  Next to the PNG grid the
CLI writes generated_codes.npy (int64 [N, T]) and generated_labels.npy (int64 [N], -1 = unconditional).
"""
import argparse
import os
from typing import List, Optional

import numpy as np
import torch
import yaml
from PIL import Image

from ..prior import sample
from ..prior.transformer import Transformer
from ..spatial_vae import SpatialVAE
from ..vae import decoder_from_vae_checkpoint


def make_grid(images: torch.Tensor, nrow: int, padding: int = 2, pad_value: float = 0.0) -> torch.Tensor:
    """torchvision.utils.make_grid(images, nrow, padding, pad_value) for a (N, C, H, W) batch: 1-channel images replicated to
    RGB, a single image returned unpadded."""
    if images.size(1) == 1:
        images = torch.cat((images, images, images), 1)
    if images.size(0) == 1:
        return images.squeeze(0)
    n = images.size(0)
    xmaps = min(nrow, n)
    ymaps = int(np.ceil(float(n) / xmaps))
    height, width = images.size(2) + padding, images.size(3) + padding
    grid = images.new_full((images.size(1), height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= n:
                break
            grid[:, y * height + padding:(y + 1) * height, x * width + padding:(x + 1) * width] = images[k]
            k += 1
    return grid


def save_image(images: torch.Tensor, path: str, nrow: int) -> None:
    """torchvision.utils.save_image(images, path, nrow=nrow): make_grid, then mul(255).add(0.5).clamp(0, 255) to uint8."""
    grid = make_grid(images.detach(), nrow)
    arr = grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()
    Image.fromarray(arr).save(path)


def load_models(cfg: dict, device: torch.device):
    transformer = Transformer(**cfg["transformer"]).to(device)
    transformer.load_state_dict(torch.load(cfg["transformer_ckpt_path"], map_location=device))
    vae_state = torch.load(cfg["vae_ckpt_path"], map_location=device)["model_state_dict"]
    if cfg.get("vanilla_vae", False):
        decoder = decoder_from_vae_checkpoint(vae_state, **cfg["vae"]).to(device)
    else:
        vae = SpatialVAE(**cfg["vae"]).to(device)
        vae.load_state_dict(vae_state)
        decoder = vae.decoder
    codebook = torch.load(cfg["codebook_path"], map_location=device, weights_only=False)
    return transformer, decoder, codebook["z_medoid"].to(device).float()


def generate_codes(transformer: Transformer, class_labels: List[Optional[int]], samples_per_class: int, temperature: float,
                   top_k: Optional[int], vanilla: bool, device: torch.device):
    """Codes of every class group in one sampling call -> (codes int64 [N, T], labels int64 [N] with -1 = unconditional)."""
    V, T = transformer.num_tokens, transformer.max_seq_len
    n = len(class_labels) * samples_per_class
    labels = torch.tensor([-1 if c is None else int(c) for c in class_labels for _ in range(samples_per_class)],
                          dtype=torch.int64, device=device)
    if any(c is None for c in class_labels) and any(c is not None for c in class_labels):
        raise ValueError("class_labels mixes None and class indices")
    y = None if class_labels[0] is None else labels
    if vanilla:
        context = torch.full((n, 1), V - 1, dtype=torch.int64, device=device)          # BOS = num_tokens - 1
        codes = sample(transformer, context, steps=T - 1, temperature=temperature, top_k=top_k, y=y)[:, 1:]
    else:
        first = torch.randint(0, V, (n, 1), device=device)
        codes = sample(transformer, first, steps=T - 1, temperature=temperature, top_k=top_k, y=y)
    return codes, labels


def check_codes(codes: torch.Tensor, n_codes: int) -> None:
    """Every code must index the codebook: checked on the host before any lookup."""
    lo, hi = int(codes.min()), int(codes.max())
    if lo < 0 or hi >= n_codes:
        raise ValueError(f"sampled code {hi if hi >= n_codes else lo} is outside the codebook's {n_codes} entries "
                         "(the vanilla prior drew its BOS token?)")


@torch.no_grad()
def decode(decoder: torch.nn.Module, z_medoid: torch.Tensor, codes: torch.Tensor, n_groups: int, vanilla: bool,
           latent_dim: int) -> torch.Tensor:
    """The reference's decode, one class group at a time, decoder left in train mode."""
    check_codes(codes, z_medoid.shape[0])
    out = []
    for group in codes.chunk(n_groups, dim=0):
        if vanilla:
            zq = z_medoid[group[:, 0]]
        else:
            zq = z_medoid[group].permute(0, 2, 1).reshape(group.shape[0], latent_dim, 4, 4)
        out.append(decoder(zq).sigmoid())
    return torch.cat(out, dim=0)


def main(config_path: str) -> str:
    with open(config_path, "r") as f:
        cfg = yaml.safe_load(f)
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if cfg.get("seed") is not None:
        torch.manual_seed(int(cfg["seed"]))
    transformer, decoder, z_medoid = load_models(cfg, device)
    class_labels = cfg.get("class_labels", [None])
    spc = cfg.get("samples_per_class", 8)
    vanilla = cfg.get("vanilla_vae", False)
    codes, labels = generate_codes(transformer, class_labels, spc, cfg.get("temperature", 1.0), cfg.get("top_k", None),
                                   vanilla, device)
    images = decode(decoder, z_medoid, codes, len(class_labels), vanilla, cfg["vae"]["latent_dim"])
    os.makedirs(cfg["output_dir"], exist_ok=True)
    path = os.path.join(cfg["output_dir"], cfg["output_filename"])
    save_image(images, path, nrow=spc)
    np.save(os.path.join(cfg["output_dir"], "generated_codes.npy"), codes.cpu().numpy())
    np.save(os.path.join(cfg["output_dir"], "generated_labels.npy"), labels.cpu().numpy())
    print(f"Saved generated images to {path}")
    return path


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, required=True, help="Path to the sampling config file.")
    main(parser.parse_args().config)
