"""Experiment directories as the reference's pipeline drivers leave them, and the decoder of each.

  vanilla   <exp>/vae/checkpoints/best.pt, <exp>/vae/latents_val/{z,mu}.pt, <exp>/codebook/{codebook.pt, codes.npy}
  spatial   <exp>/vae/<run>/checkpoints/best.pt, <exp>/vae/<run>/latents_val/{z,mu}.pt, <exp>/codebook/{codebook.pt, codes.npy}

--vae_ckpt_path, --latents_path (the z.pt file) and --codebook_path override any of the three.  Which decoder a checkpoint holds
is read from its state dict (decoder.fc: vanilla, decoder.conv_in: spatial).  Vanilla decoders are auto-detected as the
reference's loader does (vqvae_amd.vae.auto_detect_vae_config); spatial ones take the architecture flags build_codebook takes,
each defaulting to the value build_codebook recorded in codebook.pt's "config".
"""
import argparse
import glob
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import torch

from ..spatial_decoder import SpatialDecoder
from ..vae import load_vae_decoder


@dataclass
class ExperimentPaths:
    layout: str              # "vanilla" or "spatial"
    vae_ckpt: Path
    latents: Path            # z.pt; mu.pt sits next to it
    codebook: Path
    codes: Path              # codebook/codes.npy (may not exist)


def detect_layout(experiment: str, vae_ckpt_path: Optional[str] = None, latents_path: Optional[str] = None,
                  codebook_path: Optional[str] = None) -> ExperimentPaths:
    """The files of an experiment directory (module docstring).  Raises FileNotFoundError when no layout matches."""
    exp = Path(experiment)
    layout, run = None, None
    if (exp / "vae" / "checkpoints" / "best.pt").exists():
        layout, run = "vanilla", exp / "vae"
    else:
        found = sorted(glob.glob(str(exp / "vae" / "*" / "checkpoints" / "best.pt")))
        if len(found) == 1:
            layout, run = "spatial", Path(found[0]).parent.parent
        elif len(found) > 1 and vae_ckpt_path is None:
            raise FileNotFoundError(f"{exp}: several VAE runs under vae/ ({', '.join(found)}); pass --vae_ckpt_path")
    if vae_ckpt_path is not None:
        ckpt = Path(vae_ckpt_path)
        run = run or ckpt.parent.parent
    elif run is None:
        raise FileNotFoundError(f"{exp}: neither vae/checkpoints/best.pt (vanilla) nor vae/<run>/checkpoints/best.pt (spatial) "
                                "exists; pass --vae_ckpt_path")
    else:
        ckpt = run / "checkpoints" / "best.pt"
    latents = Path(latents_path) if latents_path is not None else run / "latents_val" / "z.pt"
    codebook = Path(codebook_path) if codebook_path is not None else exp / "codebook" / "codebook.pt"
    state = _state_dict(ckpt)
    if "decoder.conv_in.weight" in state:
        layout = "spatial"
    elif "decoder.fc.weight" in state:
        layout = "vanilla"
    elif layout is None:
        raise ValueError(f"{ckpt}: no decoder.fc (vanilla) or decoder.conv_in (spatial) entry in the state dict")
    return ExperimentPaths(layout, ckpt, latents, codebook, codebook.parent / "codes.npy")


def _state_dict(path: Path) -> dict:
    if not path.exists():
        raise FileNotFoundError(f"Checkpoint not found: {path}")
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    return ckpt.get("model_state_dict") or ckpt.get("model") or ckpt


def add_experiment_args(parser: argparse.ArgumentParser) -> None:
    """Path overrides and the spatial architecture flags (build_codebook's names)."""
    g = parser.add_argument_group("experiment files (default: detected under --experiment)")
    for name in ("vae_ckpt_path", "latents_path", "codebook_path"):
        g.add_argument(f"--{name}", type=str, default=None)
    a = parser.add_argument_group("spatial decoder (default: the config build_codebook recorded in codebook.pt)")
    for name in ("in_channels", "output_image_size", "latent_dim"):
        a.add_argument(f"--{name}", type=int, default=None)
    a.add_argument("--dec_channels", type=int, nargs="+", default=None)
    a.add_argument("--norm_type", type=str, default=None)
    a.add_argument("--recon_loss", type=str, default=None)
    a.add_argument("--mse_use_sigmoid", action="store_true", default=None)


def load_decoder(paths: ExperimentPaths, args, device, codebook: Optional[dict] = None):
    """(decoder in eval mode, vae_config dict with in_channels / recon_loss / mse_use_sigmoid).  Vanilla: auto-detected, no
    recon_loss / mse_use_sigmoid keys (the reference's loader records none, so its scripts fall back to mse + sigmoid)."""
    if paths.layout == "vanilla":
        return load_vae_decoder(str(paths.vae_ckpt), device=device)
    recorded = (codebook or {}).get("config", {}) or {}
    cfg = {}
    for key in ("in_channels", "output_image_size", "latent_dim", "dec_channels", "norm_type", "recon_loss", "mse_use_sigmoid"):
        v = getattr(args, key, None)
        cfg[key] = v if v is not None else recorded.get(key)
    cfg["recon_loss"] = cfg["recon_loss"] or "mse"
    cfg["mse_use_sigmoid"] = True if cfg["mse_use_sigmoid"] is None else bool(cfg["mse_use_sigmoid"])
    missing = [k for k in ("in_channels", "output_image_size", "latent_dim", "dec_channels", "norm_type") if cfg[k] is None]
    if missing:
        raise ValueError("spatial experiment: pass " + ", ".join(f"--{k}" for k in missing)
                         + f" (codebook.pt at {paths.codebook} records none)")
    state = _state_dict(paths.vae_ckpt)
    dec = SpatialDecoder(int(cfg["in_channels"]), tuple(cfg["dec_channels"]), int(cfg["latent_dim"]),
                         int(cfg["output_image_size"]), str(cfg["norm_type"]))
    dec.load_state_dict({k[len("decoder."):]: v for k, v in state.items() if k.startswith("decoder.")})
    return dec.to(device).eval(), cfg


def latents_file(paths: ExperimentPaths, name: str) -> Path:
    """z.pt or mu.pt next to the latents path."""
    return paths.latents if name == "z" else paths.latents.parent / f"{name}.pt"
