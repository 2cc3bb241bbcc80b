"""python -m vqvae_amd.scripts.train_vqvae_baseline --config config.yaml [--epochs --batch_size --lr --beta --n_codes --ema_decay
--out_dir]: the reference's baseline train.py, with the quantizer in HIP and the data resident on the GPU (vqvae_amd.baseline).
--out_dir (default outputs) is where the reference writes into the current directory."""
from ..baseline.train import main

if __name__ == "__main__":
    main()
