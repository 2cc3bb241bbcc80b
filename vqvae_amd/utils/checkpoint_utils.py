"""Loading vanilla VAEs from checkpoints with an auto-detected architecture -- same API as the reference's
src/utils/checkpoint_utils.py (auto_detect_vae_config :11, extract_state_dict :44, load_vae_from_checkpoint :56,
get_vae_decoder :122, load_decoder :138) and its forgiving behaviour: a missing file or a failed load prints (when verbose)
and returns (None, {}) / None instead of raising.  Thin wrappers: the detection and the model are vqvae_amd.vae's
(auto_detect_vae_config there already returns latent_dim, which the reference adds in load_vae_from_checkpoint)."""
from pathlib import Path
from typing import Dict, Optional, Tuple

import torch

from ..vae import VAE, auto_detect_vae_config, load_vae

__all__ = ["auto_detect_vae_config", "extract_state_dict", "load_vae_from_checkpoint", "get_vae_decoder", "load_decoder",
           "auto_detect_vae_config_legacy"]


def extract_state_dict(checkpoint: Dict) -> Dict:
    """The checkpoint's 'model_state_dict', else its 'model', else the checkpoint itself (checkpoint_utils.py:44-53)."""
    return checkpoint.get("model_state_dict") or checkpoint.get("model") or checkpoint


def load_vae_from_checkpoint(checkpoint_path: str, latent_dim: Optional[int] = None, device: str = "cpu",
                             verbose: bool = True) -> Tuple[Optional[VAE], Dict]:
    """(VAE in eval mode on `device`, detected config), or (None, {}) when the file is missing or does not load."""
    if not Path(checkpoint_path).exists():
        if verbose:
            print(f"Checkpoint not found: {checkpoint_path}")
        return None, {}
    try:
        vae, config = load_vae(str(checkpoint_path), device=device, latent_dim=latent_dim)
    except Exception as e:                                      # the reference's catch-all: report, do not raise
        if verbose:
            print(f"Error loading VAE: {e}")
        return None, {}
    if verbose:
        print(f"Auto-detected: {config['in_channels']}ch, {config['enc_channels']}, "
              f"{config['output_image_size']}x{config['output_image_size']}, {config['norm_type']}, "
              f"latent_dim={config['latent_dim']}")
        print(f"VAE loaded successfully from: {checkpoint_path}")
    return vae, config


def get_vae_decoder(checkpoint_path: str, latent_dim: Optional[int] = None, device: str = "cpu") -> Optional[torch.nn.Module]:
    """The decoder of the checkpoint's VAE in eval mode, or None if loading fails (checkpoint_utils.py:122-134)."""
    vae, _ = load_vae_from_checkpoint(checkpoint_path, latent_dim, device, verbose=False)
    return vae.decoder if vae is not None else None


def load_decoder(checkpoint_path: str, latent_dim: int, device: str = "cpu"):
    """Legacy name used by the experiments/geo scripts (checkpoint_utils.py:138-140)."""
    return get_vae_decoder(checkpoint_path, latent_dim, device)


def auto_detect_vae_config_legacy(state_dict):
    """Legacy name used by the experiments/geo scripts (checkpoint_utils.py:143-145)."""
    return auto_detect_vae_config(state_dict)
