"""Latents of a data split from a VAE checkpoint, without training again and without running the decoder:

    python -m vqvae_amd.scripts.encode_latents --checkpoint experiments/.../checkpoints/best.pt --dataset FashionMNIST \
        --data_root data --split val --out_dir experiments/.../latents_val [--config configs/.../vae.yaml]

writes z.pt, mu.pt, logvar.pt and y.pt with the shapes utils.latents.save_latents / utils.spatial_latents.save_spatial_latents
write at the end of a training run: float32 (N, d) for a vanilla VAE, (N, d, 4, 4) for a spatial one, y int64 (N,).

  - The checkpoint: a vanilla VAE is loaded with vqvae_amd.vae.load_vae (architecture auto-detected).  A spatial VAE (its
    `encoder.fc_mu.weight` is a 1 x 1 convolution) needs its architecture: the `model` section of --config (the reference's
    vae.yaml), else the "config" / "model_config" the checkpoint carries, else a vae.yaml or config.yaml next to the
    checkpoint or one directory above it.
  - The data: the un-augmented batches of vqvae_amd.training.data.get_data_loaders in file order, with that data set's
    normalisation (the training split is read unshuffled).  Nothing is downloaded: a missing file is an error naming the path.
  - Per batch, (mu, logvar) = vqvae_amd.encode.encode_latents -- the HIP kernels for encoders they cover, else the module --
    and z = model.reparameterize(mu, logvar): the module's own draw, one per batch in loader order, after
    torch.manual_seed(seed) when --seed is given.  The decoder consumes no random numbers, so after the same seed these are
    the draws the writers make.  The route that ran is printed ("encode route: hip" or "torch").
"""
import argparse
from pathlib import Path
from typing import Optional

import torch
import yaml

from .._device import device
from ..encode import encode_latents, last_encode_path, native_encode_covers
from ..image_encoder import ImageEncoderExport
from ..spatial_vae import SpatialVAE
from ..training.data import ResidentLoader, get_data_loaders
from ..vae import load_vae, read_vae_state


def _model_section(cfg) -> Optional[dict]:
    if not isinstance(cfg, dict):
        return None
    section = cfg.get("model", cfg)
    return section if isinstance(section, dict) and "enc_channels" in section else None


def spatial_model_config(checkpoint: Path, config_path: Optional[str]) -> dict:
    """The SpatialVAE constructor arguments of a spatial checkpoint (module docstring: --config, the checkpoint, a file nearby)."""
    if config_path:
        with open(config_path, "r") as f:
            section = _model_section(yaml.safe_load(f))
        if section is None:
            raise ValueError(f"{config_path} has no model section with enc_channels")
        return section
    ckpt = torch.load(checkpoint, map_location="cpu", weights_only=False)
    for key in ("config", "model_config"):
        section = _model_section(ckpt.get(key)) if isinstance(ckpt, dict) else None
        if section is not None:
            return section
    tried = [folder / name for folder in (checkpoint.parent, checkpoint.parent.parent) for name in ("vae.yaml", "config.yaml")]
    for path in tried:
        if path.exists():
            with open(path, "r") as f:
                section = _model_section(yaml.safe_load(f))
            if section is not None:
                return section
    raise FileNotFoundError("a spatial VAE checkpoint needs its architecture: give --config (the training vae.yaml); none is "
                            f"stored in {checkpoint} nor found at " + ", ".join(str(p) for p in tried))


def load_model(checkpoint: str, config_path: Optional[str], dev):
    """(model in eval mode on `dev`, "vanilla" | "spatial")."""
    state = read_vae_state(checkpoint)
    head = state.get("encoder.fc_mu.weight")
    if head is None:
        raise ValueError(f"{checkpoint} holds no encoder (no encoder.fc_mu.weight)")
    if head.dim() == 2:
        return load_vae(checkpoint, dev)[0], "vanilla"
    section = dict(spatial_model_config(Path(checkpoint), config_path))
    section.setdefault("recon_loss", "mse")
    model = SpatialVAE(**section)
    model.load_state_dict(state, strict=True)
    return model.to(dev).eval(), "spatial"


def split_loader(dataset: str, data_root: str, split: str, batch_size: int, dev) -> ResidentLoader:
    train, val = get_data_loaders(dataset, data_root, batch_size, dev, augment=False)
    if split == "val":
        return val
    return ResidentLoader(train.images, batch_size, False, train.normalize)


@torch.no_grad()
def encode_split(model, loader, max_samples: Optional[int] = None):
    """(z, mu, logvar, y) over `loader`: latents on the device, y on the host; the decoder is never run."""
    encoder = model.encoder
    zs, mus, logvars, ys, seen = [], [], [], [], 0
    for x, y in loader:
        if max_samples is not None and seen >= max_samples:
            break
        if max_samples is not None and seen + x.shape[0] > max_samples:
            x, y = x[:max_samples - seen], y[:max_samples - seen]
        if (seen == 0 and native_encode_covers(encoder, int(x.shape[-1]))
                and x.shape[1] == encoder.conv_layers[0].in_channels):
            encoder = ImageEncoderExport(encoder, x.device if x.is_cuda else device())     # composed once for every batch
        mu, logvar = encode_latents(encoder, x)
        zs.append(model.reparameterize(mu, logvar)), mus.append(mu), logvars.append(logvar), ys.append(y.cpu())
        seen += x.shape[0]
    if not zs:
        raise ValueError("the split holds no image")
    return torch.cat(zs), torch.cat(mus), torch.cat(logvars), torch.cat(ys)


def make_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Encode a data split with a VAE checkpoint: z.pt, mu.pt, logvar.pt, y.pt")
    p.add_argument("--checkpoint", required=True, help="VAE checkpoint (best.pt / latest.pt)")
    p.add_argument("--config", default=None, help="the training vae.yaml (needed for a spatial VAE unless stored with the checkpoint)")
    p.add_argument("--dataset", required=True, help="MNIST, FashionMNIST or CIFAR10")
    p.add_argument("--data_root", default="data")
    p.add_argument("--split", choices=("train", "val"), default="val")
    p.add_argument("--out_dir", required=True)
    p.add_argument("--batch_size", type=int, default=512)
    p.add_argument("--seed", type=int, default=None, help="torch.manual_seed before the first draw of z")
    p.add_argument("--max_samples", type=int, default=None, help="encode only the first images of the split")
    return p


def main(argv=None) -> Path:
    args = make_parser().parse_args(argv)
    dev = device()
    model, kind = load_model(args.checkpoint, args.config, dev)
    loader = split_loader(args.dataset, args.data_root, args.split, args.batch_size, dev)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    z, mu, logvar, y = encode_split(model, loader, args.max_samples)
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    for name, t in (("z", z), ("mu", mu), ("logvar", logvar)):
        torch.save(t.cpu(), out_dir / f"{name}.pt")
    torch.save(y, out_dir / "y.pt")
    print(f"encode route: {last_encode_path()}")
    print(f"Saved {kind} latents {tuple(z.shape)} of {args.dataset} ({args.split}) to {out_dir}")
    return out_dir


if __name__ == "__main__":
    main()
