"""The baseline VQ-VAE with an EMA codebook (the reference's baseline VQVAE/vqvae_cifar10_clean): modules and quantizer in
.model, the training loop in .train, CIFAR-10 on the device in .data.  DESIGN.md section 11."""
from .model import VQVAE, Decoder, Encoder, ResBlock, VectorQuantizerEMA, model_from_config  # noqa: F401
