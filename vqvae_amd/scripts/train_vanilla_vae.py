"""Train the vanilla VAE: the reference's src/scripts/train_vanilla_vae.py on its YAML, unchanged keys.

    python -m vqvae_amd.scripts.train_vanilla_vae --config configs/fashionmnist/vanilla/euclidean/vae.yaml

The data set is resident on the device (training/data.py), the loss is the fused HIP ELBO, MLflow is used when installed and
<out_dir>/metrics.csv is written otherwise.  As in the reference, `kl_anneal_epochs` of the YAML is not passed on: beta is
constant.
"""
import argparse
import random
from pathlib import Path

import numpy as np
import torch
import yaml
from torch.optim import Adam, AdamW
from torch.optim.lr_scheduler import CosineAnnealingLR

from ..training.data import get_data_loaders
from ..training.engine import TrainingEngine
from ..utils.logger import make_logger
from ..vae import VAE


def set_seed(seed: int) -> None:
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def get_device(device_arg: str) -> torch.device:
    if device_arg == "auto":
        return torch.device("cuda" if torch.cuda.is_available() else "cpu")
    return torch.device(device_arg)


def run(cfg: dict, loaders=None) -> Path:
    """The training run of a parsed config; `loaders` = (train_loader, val_loader) replaces the data set named by cfg['data']."""
    set_seed(cfg['seed'])
    device = get_device(cfg['device'])
    print(f"Using device: {device}")
    out_dir = Path(cfg['out_dir'])

    logger = make_logger(cfg['mlflow_tracking_uri'], cfg['experiment_name'], cfg['run_name'], out_dir)
    logger.log_params({'seed': cfg['seed'], 'device': str(device), 'max_epochs': cfg['max_epochs'], 'lr': cfg['lr'],
                       'weight_decay': cfg['weight_decay'], 'latent_dim': cfg['model']['latent_dim'],
                       'recon_loss': cfg['model']['recon_loss']})

    if loaders is None:
        data_cfg = cfg['data']
        loaders = get_data_loaders(name=str(data_cfg['name']), root=data_cfg['root'], batch_size=data_cfg['batch_size'],
                                   device=device, augment=bool(data_cfg.get('augment', False)))
    train_loader, val_loader = loaders

    model = VAE(**cfg['model']).to(device)
    optimizer_class = AdamW if cfg.get('optimizer', 'adamw') == 'adamw' else Adam
    opt = optimizer_class(model.parameters(), lr=float(cfg['lr']), weight_decay=float(cfg['weight_decay']))
    scheduler = None
    if cfg.get('scheduler') and cfg['scheduler'].get('name') == 'cosine':
        scheduler = CosineAnnealingLR(opt, T_max=int(cfg['max_epochs']))

    engine = TrainingEngine(model=model, optimizer=opt, device=device)
    engine.train(train_loader=train_loader, val_loader=val_loader, num_epochs=int(cfg['max_epochs']),
                 early_stop=int(cfg.get('early_stop', 0)), checkpoint_dir=out_dir / 'checkpoints', logger=logger,
                 output_dir=out_dir, save_latents_flag=bool(cfg.get('save_latents', True)), beta=float(cfg.get('beta', 1.0)),
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
