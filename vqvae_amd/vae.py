"""The decoder of the vanilla (vector-latent) VAE of the legacy builders (reference src/models/vae.py:53-85): Linear -> ConvT
stack with the reference's parameter names, so the `decoder.*` entries of a reference checkpoint load unchanged.  The legacy
Riemannian builder differentiates this module -- Linear-first, so edge_lengths_riemannian takes its autograd path on the GPU
(riemannian_metric.py:18-22).  Encoder, loss and sampling of the reference's VAE are not part of the hot path and not built."""
import os
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from .spatial_decoder import make_norm


class Decoder(nn.Module):
    """fc to a 4x4 grid, ConvT(k3,s2,p1[,output_padding for 32-px]) -> 7x7 | 8x8, ConvT(k4,s2,p1) x 2 -> 28 | 32 px."""

    def __init__(self, out_channels: int = 1, channels: Sequence[int] = (128, 64, 32), latent_dim: int = 16,
                 output_image_size: int = 28, norm_type: str = "none"):
        super().__init__()
        self.fc = nn.Linear(latent_dim, channels[0] * 4 * 4)
        self.deconv1 = nn.Sequential(
            nn.ConvTranspose2d(channels[0], channels[1], 3, stride=2, padding=1,
                               output_padding=1 if output_image_size == 32 else 0),
            make_norm(norm_type, channels[1]), nn.ReLU(inplace=True))
        self.deconv2 = nn.Sequential(nn.ConvTranspose2d(channels[1], channels[2], 4, stride=2, padding=1),
                                     make_norm(norm_type, channels[2]), nn.ReLU(inplace=True))
        self.output_layer = nn.ConvTranspose2d(channels[2], out_channels, 4, stride=2, padding=1)

    def forward(self, z: torch.Tensor) -> torch.Tensor:
        h = self.fc(z).view(z.size(0), -1, 4, 4)
        return self.output_layer(self.deconv2(self.deconv1(h)))


def decoder_from_vae_checkpoint(state: Dict[str, torch.Tensor], in_channels: int = 1, dec_channels: Sequence[int] = (128, 64, 32),
                                latent_dim: int = 16, output_image_size: int = 28, norm_type: str = "none", **_other) -> Decoder:
    """The decoder of a vanilla-VAE checkpoint (reference `VAE.state_dict()`: `encoder.*` and `decoder.*` entries).  Only the
    `decoder.*` entries are read -- the builders differentiate the decoder and never encode -- and they must match exactly."""
    dec = Decoder(in_channels, tuple(dec_channels), latent_dim, output_image_size, norm_type)
    own = {k[len("decoder."):]: v for k, v in state.items() if k.startswith("decoder.")}
    dec.load_state_dict(own if own else state)           # (a bare decoder state dict is accepted too)
    return dec


def auto_detect_vae_config(state: Dict[str, torch.Tensor]) -> Dict:
    """The architecture of a vanilla-VAE state dict, as the reference's checkpoint loader detects it
    (src/utils/checkpoint_utils.py auto_detect_vae_config and load_vae_from_checkpoint): in_channels from the first encoder
    convolution, enc_channels from every third encoder layer (dec_channels reversed), batch norm iff the first norm layer has
    running statistics, 32 px for 3 channels else 28, latent_dim from encoder.fc_mu (128 when absent)."""
    first = state.get("encoder.conv_layers.0.weight")
    in_channels = int(first.shape[1]) if first is not None else 1
    enc, i = [], 0
    while f"encoder.conv_layers.{i * 3}.weight" in state:
        enc.append(int(state[f"encoder.conv_layers.{i * 3}.weight"].shape[0]))
        i += 1
    enc = enc or [32, 64, 128]
    mu = state.get("encoder.fc_mu.weight")
    return {"in_channels": in_channels, "enc_channels": tuple(enc), "dec_channels": tuple(reversed(enc)),
            "norm_type": "batch" if "encoder.conv_layers.1.running_mean" in state else "none",
            "output_image_size": 32 if in_channels == 3 else 28,
            "latent_dim": int(mu.shape[0]) if mu is not None else 128}


def load_vae_decoder(checkpoint_path: str, device="cpu", latent_dim: Optional[int] = None) -> Tuple[Decoder, Dict]:
    """(decoder in eval mode, detected config) of a vanilla-VAE checkpoint: the decoder half of the reference's
    load_vae_from_checkpoint.  The state dict is the checkpoint's 'model_state_dict', else its 'model', else the checkpoint
    itself.  Raises FileNotFoundError for a missing file (the reference prints and returns None)."""
    if not os.path.exists(checkpoint_path):
        raise FileNotFoundError(f"Checkpoint not found: {checkpoint_path}")
    ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    state = ckpt.get("model_state_dict") or ckpt.get("model") or ckpt
    cfg = auto_detect_vae_config(state)
    if latent_dim is not None:
        cfg["latent_dim"] = int(latent_dim)
    dec = decoder_from_vae_checkpoint(state, **cfg)
    return dec.to(device).eval(), cfg
