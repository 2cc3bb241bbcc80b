"""The evaluation stage: drop-in for the reference's src/eval (metrics and the per-image reductions on the MI355X).

    from vqvae_amd.eval.metrics import psnr, ssim_simple, codebook_stats
"""
from .metrics import codebook_stats, psnr, ssim_simple  # noqa: F401
