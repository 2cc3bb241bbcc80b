"""Train the spatial VAE: the reference's src/scripts/train_vae.py on its YAML, unchanged keys.

    python -m vqvae_amd.scripts.train_vae --config configs/cifar10/spatial/geodesic/vae.yaml

Artifacts go to <out_dir>/spatial_vae_<data.name in lower case>/: checkpoints/best.pt and latest.pt, latents_train/ and
latents_val/ (z.pt, mu.pt, logvar.pt as (N, d, h, w) grids, y.pt), recon_grid.png -- what scripts/build_codebook.py reads.
The data set is resident on the device and each batch is one kernel (training/data.py), the loss is the fused HIP ELBO, MLflow
is used when installed and metrics.csv is written next to the artifacts otherwise.  As in the reference, the optimizer is
AdamW, `scheduler` (any truthy value) means CosineAnnealingLR over max_epochs, `model.beta` goes to the engine and
`kl_anneal_epochs` is not passed on: beta is constant.
"""
import argparse
from pathlib import Path

import yaml
from torch.optim import AdamW
from torch.optim.lr_scheduler import CosineAnnealingLR

from ..spatial_vae import SpatialVAE
from ..training.data import get_data_loaders
from ..training.spatial_engine import SpatialTrainingEngine
from ..utils.logger import make_logger
from .train_vanilla_vae import get_device, set_seed


def run(cfg: dict, loaders=None) -> Path:
    """The training run of a parsed config; `loaders` = (train_loader, val_loader) replaces the data set named by cfg['data']."""
    set_seed(cfg['seed'])
    device = get_device(cfg['device'])
    print(f"Using device: {device}")
    out_dir = Path(cfg['out_dir']) / f"spatial_vae_{str(cfg['data']['name']).lower()}"

    logger = make_logger(cfg['mlflow_tracking_uri'], cfg['experiment_name'], cfg['run_name'], out_dir)
    logger.log_params({'seed': cfg['seed'], 'device': str(device), 'max_epochs': cfg['max_epochs'], 'lr': cfg['lr'],
                       'weight_decay': cfg['weight_decay'], 'latent_dim': cfg['model']['latent_dim'],
                       'recon_loss': cfg['model']['recon_loss']})

    if loaders is None:
        data_cfg = cfg['data']
        loaders = get_data_loaders(name=str(data_cfg['name']), root=data_cfg['root'], batch_size=data_cfg['batch_size'],
                                   device=device, augment=bool(data_cfg.get('augment', False)))
    train_loader, val_loader = loaders

    model = SpatialVAE(**cfg['model']).to(device)
    opt = AdamW(model.parameters(), lr=float(cfg['lr']), weight_decay=float(cfg['weight_decay']))
    scheduler = CosineAnnealingLR(opt, T_max=int(cfg['max_epochs'])) if cfg.get('scheduler') else None

    engine = SpatialTrainingEngine(model=model, optimizer=opt, device=device)
    engine.train(train_loader=train_loader, val_loader=val_loader, num_epochs=cfg['max_epochs'], early_stop=cfg['early_stop'],
                 checkpoint_dir=out_dir / 'checkpoints', logger=logger, output_dir=out_dir,
                 save_latents_flag=bool(cfg['save_latents']), beta=float(cfg['model']['beta']),
                 grad_clip_max_norm=float(cfg.get('grad_clip_max_norm', 0.0)), scheduler=scheduler)
    logger.end()
    print("Done. Artifacts in:", out_dir)
    return out_dir


def main(config_path: str) -> Path:
    with open(config_path, "r") as f:
        return run(yaml.safe_load(f))


if __name__ == '__main__':
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, required=True, help="Path to the training config file.")
    main(parser.parse_args().config)
