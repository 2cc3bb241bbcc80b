"""SpatialVAE on the MI355X: the reference's model (src/models/spatial_vae.py) -- its encoder half next to the
decoder of vqvae_amd/spatial_decoder.py -- with the SAME parameter names, so a `best.pt` written by either trainer
({'model_state_dict', 'epoch'}, spatial_engine.py:142) loads into the other's model unchanged.

Inference (encode -> mu, logvar, z) feeds the geodesic-codebook path; `loss` is the reference's spatial ELBO and is what
training/spatial_engine.py and scripts/train_vae.py train with.  On CUDA tensors it is the fused HIP
ELBO the vanilla VAE uses (`elbo_hip` of vae.py, csrc/vae_loss.hip) on the latent grids viewed as [B][d h w], and returns
float64 scalars that live on the device; on CPU tensors it is the reference's formula in torch ops.  The layers are
PyTorch-ROCm modules, and training, `forward` and the latent writers run them as such.  Inference of the encoder alone also
exists in HIP: vqvae_amd.encode.encode_latents (csrc/encode.hip) runs a SpatialEncoder with fixed
statistics natively, and scripts/encode_latents.py is the command that uses it; the callers of `model(x)` are not switched."""
from typing import Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .spatial_decoder import SpatialDecoder, make_norm
from .vae import CAPACITY_MODES, RECON_MODES, elbo_hip


class SpatialEncoder(nn.Module):
    """Stride-2 3x3 convolutions with norm + ReLU, then 1x1 heads for the mean and log-variance grids."""

    def __init__(self, input_channels: int, channels: Sequence[int], latent_dim: int, norm_type: str):
        super().__init__()
        layers, prev = [], input_channels
        for ch in channels:
            layers += [nn.Conv2d(prev, ch, 3, stride=2, padding=1), make_norm(norm_type, ch), nn.ReLU(inplace=True)]
            prev = ch
        self.conv_layers = nn.Sequential(*layers)
        self.fc_mu = nn.Conv2d(prev, latent_dim, 1)
        self.fc_logvar = nn.Conv2d(prev, latent_dim, 1)

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        h = self.conv_layers(x)
        return self.fc_mu(h), self.fc_logvar(h)


class SpatialVAE(nn.Module):
    """encoder + decoder under the reference's attribute names (spatial_vae.py:84-104); forward returns
    (x_logits, mu, logvar, z) with z = mu + eps * exp(logvar / 2), eps ~ N(0, 1) from torch's generator."""

    def __init__(self, in_channels, enc_channels, dec_channels, latent_dim, recon_loss, output_image_size, norm_type,
                 **kwargs):
        super().__init__()
        assert recon_loss in {"bce", "mse"}
        self.encoder = SpatialEncoder(in_channels, tuple(enc_channels), latent_dim, norm_type)
        self.decoder = SpatialDecoder(in_channels, tuple(dec_channels), latent_dim, output_image_size, norm_type)
        self.recon_loss = recon_loss
        self.mse_use_sigmoid = kwargs.get("mse_use_sigmoid", True)
        self._step = 0

    @staticmethod
    def reparameterize(mu: torch.Tensor, logvar: torch.Tensor) -> torch.Tensor:
        std = torch.exp(0.5 * logvar)
        return mu + torch.randn_like(std) * std

    def forward(self, x: torch.Tensor):
        mu, logvar = self.encoder(x)
        z = self.reparameterize(mu, logvar)
        return self.decoder(z), mu, logvar, z

    def loss(self, x, x_logits, mu, logvar, beta: float, **kwargs) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(total, recon, kl) of the reference (spatial_vae.py:110-125): recon = the summed BCE-with-logits, or squared error
        of sigmoid(x_logits) or of x_logits, over the batch size; kl = the batch mean of the sum over (d, h, w) of
        -0.5 (1 + logvar - mu^2 - exp(logvar)); total = recon + beta kl.  Other keywords (the engine's `step=`) are ignored."""
        B = x.size(0)
        if x_logits.is_cuda:
            mode = RECON_MODES["bce" if self.recon_loss == "bce" else "mse_sigmoid" if self.mse_use_sigmoid else "mse_logits"]
            # reshape copies a grid that is not contiguous (a channels-last convolution output) once; elbo_hip does the same
            # for x_logits and x
            out = elbo_hip(x_logits, x, mu.reshape(B, -1), logvar.reshape(B, -1), mode, None, beta, 0.0, CAPACITY_MODES["off"])
            return out[0], out[1].detach(), out[2].detach()
        if self.recon_loss == "bce":
            recon = F.binary_cross_entropy_with_logits(x_logits, x, reduction="sum") / B
        else:
            x_pred = torch.sigmoid(x_logits) if self.mse_use_sigmoid else x_logits
            recon = F.mse_loss(x_pred, x, reduction="sum") / B
        kl = (-0.5 * (1 + logvar - mu.pow(2) - logvar.exp())).sum(dim=[1, 2, 3]).mean()
        return recon + beta * kl, recon, kl
