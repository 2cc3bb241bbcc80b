"""The decoder of the vanilla (vector-latent) VAE of the legacy builders (reference src/models/vae.py:53-85): Linear -> ConvT
stack with the reference's parameter names, so the `decoder.*` entries of a reference checkpoint load unchanged.  The legacy
Riemannian builder differentiates this module: in eval mode (BatchNorm with running statistics, or no norm) in the HIP kernels
of csrc/vanilla_jvp.hip (vqvae_amd.vanilla_decoder), otherwise -- GroupNorm, train-mode BatchNorm -- by
autograd on the GPU (riemannian_metric.py:18-22).

`Encoder` and `VAE` complete the reference's model (src/models/vae.py:22-50, :88-198) with its constructor arguments, attribute
and parameter names: a reference `model_state_dict` loads with strict=True and `VAE(**cfg['model'])` takes the reference's YAML.
`VAE.loss` keeps the reference's signature, defaults and `_step` counter.  On CUDA tensors it runs the fused HIP ELBO
(csrc/vae_loss.hip) and returns float64 scalars that live on the device; on CPU tensors, or with
`VAE.native_loss = False`, it evaluates the reference's formula with torch ops in the inputs' dtype."""
import ctypes
import os
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .spatial_decoder import make_norm

RECON_MODES = {"bce": 0, "mse_sigmoid": 1, "mse_logits": 2}          # GEO_VAE_RECON_* of include/geo_hip.h
CAPACITY_MODES = {"off": 0, "abs": 1, "clipped": 2}                  # GEO_VAE_CAPACITY_*


class Encoder(nn.Module):
    """Conv(k3,s2,p1) -> norm -> ReLU per channel count, flattened 4x4 grid -> fc_mu, fc_logvar."""

    def __init__(self, input_channels: int = 1, channels: Sequence[int] = (32, 64, 128), latent_dim: int = 16,
                 norm_type: str = "none"):
        super().__init__()
        layers, prev = [], input_channels
        for ch in channels:
            layers.extend([nn.Conv2d(prev, ch, 3, stride=2, padding=1), make_norm(norm_type, ch), nn.ReLU(inplace=True)])
            prev = ch
        self.conv_layers = nn.Sequential(*layers)
        self.feature_dim = channels[-1] * 4 * 4
        self.fc_mu = nn.Linear(self.feature_dim, latent_dim)
        self.fc_logvar = nn.Linear(self.feature_dim, latent_dim)

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        h = self.conv_layers(x)
        h = h.reshape(h.size(0), -1)          # (the reference's view; reshape also takes a channels-last convolution output)
        return self.fc_mu(h), self.fc_logvar(h)


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
    state = read_vae_state(checkpoint_path)
    cfg = auto_detect_vae_config(state)
    if latent_dim is not None:
        cfg["latent_dim"] = int(latent_dim)
    dec = decoder_from_vae_checkpoint(state, **cfg)
    return dec.to(device).eval(), cfg


def _ptr(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


def _workspace(nbytes: int, dev) -> torch.Tensor:
    """The ELBO's scratch: one exact-size allocation per call from the stream-ordered caching allocator (no device sync)."""
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


class _ElboFunction(torch.autograd.Function):
    """out f64 [4] = total, recon, kl, regulated kl (geo_vae_elbo_forward); only out[0] carries a gradient."""

    @staticmethod
    def forward(ctx, x_logits, x, mu, logvar, recon_mode, free_bits, beta, target, capacity_mode):
        from . import _lib
        for name, t in (("x_logits", x_logits), ("x", x), ("mu", mu), ("logvar", logvar)):
            if not (t.is_cuda and t.dtype == torch.float32 and t.device == x_logits.device):
                raise ValueError(f"the HIP ELBO needs float32 CUDA tensors on one device; {name} is {t.dtype} on {t.device}")
        B = x.size(0)
        if x_logits.numel() != x.numel() or x_logits.size(0) != B or mu.shape != logvar.shape or mu.dim() != 2 or mu.size(0) != B:
            raise ValueError(f"ELBO shapes: x_logits {tuple(x_logits.shape)}, x {tuple(x.shape)}, mu {tuple(mu.shape)}, "
                             f"logvar {tuple(logvar.shape)}")
        l, t, m, v = (a.detach().contiguous() for a in (x_logits, x, mu, logvar))
        P, d = l.numel() // B, m.size(1)
        L = _lib.load()
        nbytes = L.geo_vae_elbo_workspace_bytes(B, P, d)
        if nbytes == 0:
            raise _lib.GeoHipError(f"geo_vae_elbo_workspace_bytes rejected B={B} P={P} d={d}")
        dev = l.device
        ws = _workspace(nbytes, dev)
        out = torch.empty(4, dtype=torch.float64, device=dev)
        has_fb = free_bits is not None
        args = (B, P, d, int(recon_mode), int(has_fb), float(free_bits) if has_fb else 0.0, float(beta), float(target),
                int(capacity_mode))
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(L.geo_vae_elbo_forward(_ptr(l), _ptr(t), _ptr(m), _ptr(v), *args, _ptr(out), _ptr(ws), nbytes, stream),
                       "geo_vae_elbo_forward")
        ctx.save_for_backward(l, t, m, v, out)
        ctx.args = args
        ctx.shapes = (x_logits.shape, mu.shape)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from . import _lib
        l, t, m, v, out = ctx.saved_tensors
        g = grad_out.to(torch.float64).contiguous()                   # g[0] = d / d total; recon and kl are handed out detached
        d_l, d_m, d_v = torch.empty_like(l), torch.empty_like(m), torch.empty_like(v)
        with torch.cuda.device(l.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(l.device).cuda_stream)
            _lib.check(_lib.load().geo_vae_elbo_backward(_ptr(g), _ptr(out), _ptr(l), _ptr(t), _ptr(m), _ptr(v), *ctx.args,
                                                         _ptr(d_l), _ptr(d_m), _ptr(d_v), stream), "geo_vae_elbo_backward")
        return d_l.view(ctx.shapes[0]), None, d_m.view(ctx.shapes[1]), d_v.view(ctx.shapes[1]), None, None, None, None, None


def elbo_hip(x_logits: torch.Tensor, x: torch.Tensor, mu: torch.Tensor, logvar: torch.Tensor, recon_mode: int,
             free_bits: Optional[float], beta: float, capacity_target: float, capacity_mode: int) -> torch.Tensor:
    """The fused ELBO: float64 [4] on the device = total, recon, kl, regulated kl.  No host synchronisation; gradients flow
    from element 0 to x_logits, mu and logvar (float32)."""
    return _ElboFunction.apply(x_logits, x, mu, logvar, recon_mode, free_bits, beta, capacity_target, capacity_mode)


class VAE(nn.Module):
    """The reference's vanilla VAE: Encoder -> reparameterisation (a fresh normal draw in train AND eval mode) -> Decoder."""

    native_loss = True            # CUDA tensors: HIP ELBO; False: the torch formula everywhere (the in-repo oracle)

    def __init__(self, in_channels=1, enc_channels=(32, 64, 128), dec_channels=(128, 64, 32), latent_dim=16, recon_loss="bce",
                 output_image_size: int = 28, norm_type: str = "none", mse_use_sigmoid: bool = True,
                 free_bits_default: float = 0.5, capacity_max_default: float = 15.0,
                 capacity_anneal_steps_default: int = 50_000, capacity_mode_default: str = "abs"):
        super().__init__()
        self.encoder = Encoder(in_channels, enc_channels, latent_dim, norm_type)
        self.decoder = Decoder(in_channels, dec_channels, latent_dim, output_image_size, norm_type)
        assert recon_loss in {"bce", "mse"}, f"recon_loss must be 'bce' or 'mse', got {recon_loss}"
        self.recon_loss = recon_loss
        self.mse_use_sigmoid = mse_use_sigmoid
        self.free_bits_default = free_bits_default
        self.capacity_max_default = capacity_max_default
        self.capacity_anneal_steps_default = capacity_anneal_steps_default
        self.capacity_mode_default = capacity_mode_default
        self._step = 0

    @staticmethod
    def reparameterize(mu: torch.Tensor, logvar: torch.Tensor) -> torch.Tensor:
        std = torch.exp(0.5 * logvar)
        eps = torch.randn_like(std)
        return mu + eps * std

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        mu, logvar = self.encoder(x)
        z = self.reparameterize(mu, logvar)
        return self.decoder(z), mu, logvar, z

    def _compute_reconstruction_loss(self, x_logits: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        batch_size = x.size(0)
        if self.recon_loss == "bce":
            return F.binary_cross_entropy_with_logits(x_logits, x, reduction="sum") / batch_size
        x_pred = torch.sigmoid(x_logits) if self.mse_use_sigmoid else x_logits
        return F.mse_loss(x_pred, x, reduction="sum") / batch_size

    def _compute_kl_loss(self, mu: torch.Tensor, logvar: torch.Tensor, free_bits: Optional[float] = None) -> torch.Tensor:
        kl_per_dim = -0.5 * (1 + logvar - mu.pow(2) - logvar.exp())
        if free_bits is not None:
            kl_per_dim = torch.clamp(kl_per_dim, min=free_bits)
        return kl_per_dim.sum(dim=1).mean()

    def _compute_capacity_target(self, capacity_max: float, capacity_anneal_steps: int, step: int) -> float:
        return capacity_max * min(1.0, step / max(1, capacity_anneal_steps))

    def recon_mode(self) -> int:
        if self.recon_loss == "bce":
            return RECON_MODES["bce"]
        return RECON_MODES["mse_sigmoid" if self.mse_use_sigmoid else "mse_logits"]

    def loss(self, x, x_logits, mu, logvar, *, beta: float = 1.0, free_bits: Optional[float] = None,
             capacity_max: Optional[float] = None, capacity_anneal_steps: Optional[int] = None, step: Optional[int] = None,
             capacity_mode: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(total, recon, kl) of the reference's ELBO: free bits clamp each KL dimension from below, capacity annealing
        replaces kl by |kl - C(step)| ("abs") or max(kl - C(step), 0) (any other mode) in the total.  As in the reference, an
        argument left None takes the model's default (free bits are off only when `free_bits_default` is None too) and
        `step=None` uses and advances the model's own counter."""
        free_bits = self.free_bits_default if free_bits is None else free_bits
        capacity_max = self.capacity_max_default if capacity_max is None else capacity_max
        capacity_anneal_steps = self.capacity_anneal_steps_default if capacity_anneal_steps is None else capacity_anneal_steps
        capacity_mode = self.capacity_mode_default if capacity_mode is None else capacity_mode
        if step is None:
            step = self._step
            self._step += 1
        use_capacity = capacity_max > 0 and capacity_anneal_steps > 0
        target = self._compute_capacity_target(capacity_max, capacity_anneal_steps, step) if use_capacity else 0.0

        if self.native_loss and x_logits.is_cuda:
            mode = CAPACITY_MODES["off"] if not use_capacity else CAPACITY_MODES["abs" if capacity_mode == "abs" else "clipped"]
            out = elbo_hip(x_logits, x, mu, logvar, self.recon_mode(), free_bits, beta, target, mode)
            return out[0], out[1].detach(), out[2].detach()

        recon_loss = self._compute_reconstruction_loss(x_logits, x)
        kl_loss = self._compute_kl_loss(mu, logvar, free_bits)
        if use_capacity:
            if capacity_mode == "abs":
                kl_regulated = torch.abs(kl_loss - target)
            else:
                kl_regulated = torch.clamp(kl_loss - target, min=0.0)
            total_loss = recon_loss + beta * kl_regulated
        else:
            total_loss = recon_loss + beta * kl_loss
        return total_loss, recon_loss, kl_loss


def read_vae_state(checkpoint_path: str) -> Dict[str, torch.Tensor]:
    """The state dict of a vanilla-VAE checkpoint: its 'model_state_dict', else its 'model', else the checkpoint itself."""
    if not os.path.exists(checkpoint_path):
        raise FileNotFoundError(f"Checkpoint not found: {checkpoint_path}")
    ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    return ckpt.get("model_state_dict") or ckpt.get("model") or ckpt


def load_vae(checkpoint_path: str, device="cpu", latent_dim: Optional[int] = None) -> Tuple[VAE, Dict]:
    """(VAE in eval mode, detected config): the full-model sibling of load_vae_decoder, same lookup and auto-detection.
    The loss settings are not part of a state dict: the model carries the constructor's defaults (recon_loss "bce")."""
    state = read_vae_state(checkpoint_path)
    cfg = auto_detect_vae_config(state)
    if latent_dim is not None:
        cfg["latent_dim"] = int(latent_dim)
    model = VAE(**cfg)
    model.load_state_dict(state, strict=True)
    return model.to(device).eval(), cfg
