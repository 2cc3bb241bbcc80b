"""Score the samples of the code prior against real images: precision, recall, density, coverage.

    python -m vqvae_amd.scripts.evaluate_generation --config configs/<dataset>/<vae>/<codebook>/generate.yaml \
        --dataset FashionMNIST --data_root data --split test --num_samples 10000 --k 5 --out_dir experiments/.../generation

Reads the reference's generate.yaml unchanged, exactly as generate_samples does (transformer, vae, vanilla_vae, class_labels,
temperature, top_k and the three checkpoint paths).  Steps:

  1. N code sequences from the prior (generate_samples.generate_codes), the yaml's class labels cycled over the N samples.
  2. The codes are decoded from the codebook table with vqvae_amd.decode.decode_images, sigmoid applied as generate_samples
     applies it.  The decoder runs in EVAL mode here: generate_samples reproduces the reference's train-mode batch
     statistics, under which an image depends on the samples that share its batch -- a score must not.
  3. The real split (--split test | train, the first --max_real images) is read through vqvae_amd.eval.data.
  4. Reals and fakes are encoded with vqvae_amd.encode.encode_latents: the experiment's own encoder, in eval mode; an
     image's feature is its mu, flattened (d for a vanilla VAE, 16 d for a spatial one).  Fakes are normalised the way the
     data set's batches are before they are encoded.
  5. vqvae_amd.eval.prdc.prdc_device on the two feature sets.

The same four figures are also reported for one half of the real features against the other half (a seeded split): what a
perfect generator would score at this sample size.  Without that ceiling the figures cannot be read.

Writes generation_metrics.json (the four figures, the ceiling, k, n, m, the feature width, the encode, decode and scoring
routes taken) and generation_prdc.npz (the per-sample arrays of prdc_device: which reals are uncovered, which fakes fall off
the manifold).  A vanilla checkpoint that holds only decoder.* entries cannot be scored: the error names the missing keys.
"""
import argparse
import json
import os
from typing import Dict, List, Optional

import numpy as np
import torch
import yaml

FIGURES = ("precision", "recall", "density", "coverage")
ENCODER_KEYS = ("encoder.conv_layers.*", "encoder.fc_mu.weight", "encoder.fc_mu.bias", "encoder.fc_logvar.weight",
                "encoder.fc_logvar.bias")


def make_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Precision, recall, density and coverage of the code prior's samples")
    p.add_argument("--config", required=True, help="the sampling config (the reference's generate.yaml)")
    p.add_argument("--dataset", required=True, help="MNIST, FashionMNIST or CIFAR10")
    p.add_argument("--data_root", default="data")
    p.add_argument("--split", choices=("test", "train"), default="test")
    p.add_argument("--num_samples", type=int, default=10000, help="N generated samples")
    p.add_argument("--k", type=int, default=5, help="neighbours of the radii")
    p.add_argument("--max_real", type=int, default=None, help="score against the first M images of the split")
    p.add_argument("--out_dir", default=None, help="default: the yaml's output_dir")
    p.add_argument("--seed", type=int, default=None, help="seeds the draws and the ceiling's split; default: the yaml's seed, else 0")
    return p


def check_has_encoder(state: Dict[str, torch.Tensor], path: str) -> None:
    """A checkpoint without encoder.* entries (the decoder-only files the builders accept) cannot produce features."""
    if not any(k.startswith("encoder.") for k in state):
        found = sorted({k.split(".")[0] + ".*" for k in state})
        raise ValueError(f"{path} holds no encoder: scoring needs the experiment's encoder entries "
                         f"({', '.join(ENCODER_KEYS)}), found only {', '.join(found) or 'nothing'}")


def load_model(cfg: dict, device):
    """The experiment's whole VAE (encoder and decoder) in eval mode on `device`."""
    from ..spatial_vae import SpatialVAE
    from ..vae import VAE
    path = cfg["vae_ckpt_path"]
    state = torch.load(path, map_location="cpu")["model_state_dict"]
    check_has_encoder(state, path)
    model = (VAE if cfg.get("vanilla_vae", False) else SpatialVAE)(**cfg["vae"])
    model.load_state_dict(state)
    return model.to(device).eval()


def real_images(dataset: str, data_root: str, split: str, max_real: Optional[int], device):
    """The split as a ResidentLoader of un-augmented batches in file order, through vqvae_amd.eval.data."""
    from ..eval import data as files
    from ..training.data import CIFAR_MEAN, CIFAR_STD, ResidentLoader, resident_images
    key = dataset.strip().lower()
    train = split == "train"
    if key == "cifar10":
        images, labels = files.cifar10_train(data_root) if train else files.cifar10_test(data_root)
        norm = (CIFAR_MEAN, CIFAR_STD)
    elif key in ("mnist", "fashionmnist", "fashion-mnist", "fashion_mnist"):
        images, labels = files.idx_split(data_root, "MNIST" if key == "mnist" else "FashionMNIST", train=train)
        norm = None
    else:
        raise ValueError(f"Unknown dataset: {dataset}")
    if max_real is not None:
        images, labels = images[:max_real], labels[:max_real]
    return ResidentLoader(resident_images(images, labels, device, norm), 512, False, norm), norm


@torch.no_grad()
def features(encoder, batches) -> torch.Tensor:
    """mu of every image, flattened: f32 [n, width] on the device."""
    from ..encode import encode_latents
    out = [encode_latents(encoder, x)[0].reshape(x.shape[0], -1) for x in batches]
    return torch.cat(out).contiguous()


@torch.no_grad()
def generate_images(cfg: dict, model, device, num_samples: int, dataset: str, seed: int) -> torch.Tensor:
    """N images in [0, 1] from the prior's codes, decoded in eval mode from the codebook table.  torch is seeded right before
    the draw, after every module is built: the codes depend on the seed and the checkpoints, not on what was constructed."""
    from ..decode import decode_images
    from ..prior.transformer import Transformer
    from .generate_samples import check_codes, generate_codes
    transformer = Transformer(**cfg["transformer"]).to(device)
    transformer.load_state_dict(torch.load(cfg["transformer_ckpt_path"], map_location=device))
    table = torch.load(cfg["codebook_path"], map_location=device, weights_only=False)["z_medoid"].to(device).float()
    classes: List[Optional[int]] = cfg.get("class_labels", [None])
    labels = [classes[i % len(classes)] for i in range(num_samples)]
    vanilla = cfg.get("vanilla_vae", False)
    torch.manual_seed(seed)
    codes, _ = generate_codes(transformer, labels, 1, cfg.get("temperature", 1.0), cfg.get("top_k", None), vanilla, device)
    check_codes(codes, table.shape[0])
    codes = codes[:, 0].contiguous() if vanilla else codes.reshape(num_samples, 4, 4)       # token t sits at (t // 4, t % 4)
    return decode_images(model.decoder, table=table, codes=codes, dataset=dataset, apply_sigmoid=True)


def _figures(res: dict) -> Dict[str, float]:
    return {name: float(res[name]) for name in FIGURES}


def main(argv=None) -> str:
    from .._device import device as gpu
    from ..decode import last_decode_path
    from ..encode import last_encode_path
    from ..eval.prdc import prdc_device
    args = make_parser().parse_args(argv)
    with open(args.config, "r") as f:
        cfg = yaml.safe_load(f)
    if args.num_samples <= args.k:
        raise ValueError(f"--num_samples {args.num_samples} must exceed --k {args.k}")
    seed = args.seed if args.seed is not None else int(cfg.get("seed") or 0)
    dev = gpu()
    model = load_model(cfg, dev)
    fake_images = generate_images(cfg, model, dev, args.num_samples, args.dataset, seed)
    decode_path = last_decode_path()
    loader, norm = real_images(args.dataset, args.data_root, args.split, args.max_real, dev)
    if norm is not None:
        mean = torch.tensor(list(norm[0]), device=dev).view(1, -1, 1, 1)
        std = torch.tensor(list(norm[1]), device=dev).view(1, -1, 1, 1)
        fake_images = (fake_images - mean) / std
    real = features(model.encoder, (x for x, _ in loader))
    fake = features(model.encoder, fake_images.split(512))
    encode_path = last_encode_path()
    if real.shape[0] < 2 * (args.k + 1):
        raise ValueError(f"{real.shape[0]} real images are too few for k = {args.k} and the ceiling's two halves")
    res = prdc_device(real, fake, args.k)
    order = torch.from_numpy(np.random.RandomState(seed).permutation(real.shape[0])).to(dev)
    half = real.shape[0] // 2
    ceiling = prdc_device(real[order[:half]].contiguous(), real[order[half:]].contiguous(), args.k)

    out_dir = args.out_dir or cfg["output_dir"]
    os.makedirs(out_dir, exist_ok=True)
    summary = dict(_figures(res), ceiling=_figures(ceiling), k=args.k, n=int(real.shape[0]), m=int(fake.shape[0]),
                   feature_width=int(real.shape[1]), dataset=args.dataset, split=args.split, seed=seed,
                   encode_path=encode_path, decode_path=decode_path, prdc_route=res["route"])
    path = os.path.join(out_dir, "generation_metrics.json")
    with open(path, "w") as f:
        json.dump(summary, f, indent=2, sort_keys=True)
    np.savez(os.path.join(out_dir, "generation_prdc.npz"),
             **{name: t.cpu().numpy() for name, t in res.items() if isinstance(t, torch.Tensor)})
    print(json.dumps(summary, sort_keys=True))
    print(f"Saved generation metrics to {path}")
    return path


if __name__ == "__main__":
    main()
