"""Training loop of the spatial VAE: the reference's SpatialTrainingEngine (src/training/spatial_engine.py) with its constructor,
`run_epoch` and `train` signatures and return tuples.  The reference's two engines are one loop that differs in the model's
`loss` and in the latent writer, so this is `TrainingEngine` (engine.py: the contract and the allowed differences are stated
at its top, DESIGN.md sections 13 and 14) with `utils.spatial_latents.save_spatial_latents` -- z.pt, mu.pt, logvar.pt as
(N, d, h, w) grids -- as the writer.  The loss is `SpatialVAE.loss`; its `step=` keyword is accepted and unused there."""
from ..utils.spatial_latents import save_spatial_latents
from .engine import TrainingEngine


class SpatialTrainingEngine(TrainingEngine):
    latent_writer = staticmethod(save_spatial_latents)
