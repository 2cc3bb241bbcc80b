"""Training loop of the vanilla VAE: the reference's TrainingEngine (src/training/engine.py), eager, MIOpen convolutions,
torch optimizer; the loss is `VAE.loss` (the fused HIP ELBO on the GPU).

Kept as the reference has them:
  - the loss's capacity step is a global step that carries across epochs; validation batches all use the step the training
    epoch ended on;
  - current_beta = beta * min(1, epoch / kl_anneal_epochs) when kl_anneal_epochs > 0, else beta;
  - the epoch averages divide the per-batch sums by len(loader), whatever the batch sizes;
  - best.pt = {'model_state_dict', 'epoch'} on a strictly lower validation loss, latest.pt at the end with epoch = num_epochs
    (also after an early stop); early stop after `early_stop` epochs without improvement, before that epoch's scheduler step;
  - the scheduler steps once per epoch; clip_grad_norm_ runs only when grad_clip_max_norm > 0;
  - recon_grid.png: the first 8 validation images over their reconstructions, un-normalised when the loader normalises.

Different from the reference:
  - the running loss / recon / kl sums accumulate in fp64 on the device and are read once per epoch (the reference calls
    .item() three times per step), so there is no per-step progress postfix; one line is printed per epoch;
  - validation PSNR and SSIM come from the per-image pair moments of eval/metrics.py (geo_image_pair_moments on the GPU),
    collected per batch and read once per epoch; the weighting (per-batch value times batch size, over the image count) is
    the reference's.
"""
from typing import Tuple

import numpy as np
import torch

from ..eval import metrics
from ..scripts.generate_samples import save_image
from ..utils.latents import save_latents


def _batch_moments(x_rec: torch.Tensor, x: torch.Tensor):
    """Per-image pair moments f64 [B][6] of a batch: a device tensor for CUDA inputs (no sync), a numpy array otherwise."""
    B = x.size(0)
    if x.is_cuda:
        return metrics.image_pair_moments(x_rec.reshape(B, -1), x.reshape(B, -1))
    return metrics.image_pair_moments_numpy(x_rec.reshape(B, -1).double().numpy(), x.reshape(B, -1).double().numpy())


class TrainingEngine:
    latent_writer = staticmethod(save_latents)          # (model, loader, device, out_dir); spatial_engine.py swaps it

    def __init__(self, model, optimizer: torch.optim.Optimizer, device: torch.device) -> None:
        self.model = model
        self.optimizer = optimizer
        self.device = device

    def run_epoch(self, loader, train: bool, epoch: int, num_epochs: int, beta: float, grad_clip_max_norm: float = 0.0,
                  global_step_start: int = 0) -> Tuple[float, float, float, int, float, float]:
        """(avg_loss, avg_recon, avg_kl, global_step, avg_psnr, avg_ssim); PSNR / SSIM are 0 for a training epoch."""
        self.model.train() if train else self.model.eval()
        sums = torch.zeros(3, dtype=torch.float64, device=self.device)
        global_step = int(global_step_start)
        apply_sigmoid = (getattr(self.model, 'recon_loss', 'mse') == 'bce') or getattr(self.model, 'mse_use_sigmoid', True)
        moments = []

        for x, _ in loader:
            x = x.to(self.device)
            if train:
                x_logits, mu, logvar, _ = self.model(x)
                loss, recon, kl = self.model.loss(x, x_logits, mu, logvar, beta=beta, step=global_step)
                self.optimizer.zero_grad(set_to_none=True)
                loss.backward()
                if grad_clip_max_norm > 0:
                    torch.nn.utils.clip_grad_norm_(self.model.parameters(), max_norm=grad_clip_max_norm)
                self.optimizer.step()
                global_step += 1
            else:
                with torch.no_grad():
                    x_logits, mu, logvar, _ = self.model(x)
                    loss, recon, kl = self.model.loss(x, x_logits, mu, logvar, beta=beta, step=global_step)
                    x_rec = torch.sigmoid(x_logits) if apply_sigmoid else x_logits
                    x_rec.clamp_(0, 1)
                    moments.append(_batch_moments(x_rec, x))
            sums += torch.stack([loss.detach(), recon.detach(), kl.detach()]).double()

        avg_loss, avg_recon, avg_kl = (sums / len(loader)).tolist()          # the epoch's one read of the device sums
        psnr_sum, ssim_sum, count = 0.0, 0.0, 0
        for m in moments:
            m = m.cpu().numpy() if torch.is_tensor(m) else m
            psnr_sum += metrics.psnr_from_moments(m, x[0].numel()) * len(m)
            ssim_sum += metrics.ssim_from_moments(m) * len(m)
            count += len(m)
        avg_psnr = psnr_sum / count if count > 0 else 0
        avg_ssim = ssim_sum / count if count > 0 else 0
        print(f"{'Train' if train else 'Val'} [{epoch}/{num_epochs}] loss={avg_loss:.4f} recon={avg_recon:.4f} kl={avg_kl:.4f}"
              + (f" psnr={avg_psnr:.2f} ssim={avg_ssim:.4f}" if count else ""))
        return avg_loss, avg_recon, avg_kl, global_step, avg_psnr, avg_ssim

    def train(self, train_loader, val_loader, num_epochs: int, early_stop: int, checkpoint_dir, logger, output_dir,
              save_latents_flag: bool, kl_anneal_epochs: int = 0, beta: float = 1.0, grad_clip_max_norm: float = 0.0,
              scheduler=None) -> None:
        """Train for num_epochs with early stopping."""
        best_val = float('inf')
        no_improve = 0
        num_pixels = None
        global_step = 0
        if checkpoint_dir is not None:
            checkpoint_dir.mkdir(parents=True, exist_ok=True)
        if output_dir is not None:
            output_dir.mkdir(parents=True, exist_ok=True)

        for epoch in range(1, num_epochs + 1):
            current_beta = beta * min(1.0, epoch / kl_anneal_epochs) if kl_anneal_epochs > 0 else beta
            print(f"Epoch {epoch}/{num_epochs} (beta={current_beta:.4f})")
            train_loss, train_recon, train_kl, global_step, _, _ = self.run_epoch(
                train_loader, train=True, epoch=epoch, num_epochs=num_epochs, beta=current_beta,
                grad_clip_max_norm=grad_clip_max_norm, global_step_start=global_step)
            val_loss, val_recon, val_kl, _, val_psnr, val_ssim = self.run_epoch(
                val_loader, train=False, epoch=epoch, num_epochs=num_epochs, beta=current_beta, grad_clip_max_norm=0.0,
                global_step_start=global_step)

            if num_pixels is None:
                # (the reference opens a loader iterator for one sample here: the same base-seed draw from the CPU generator)
                x_sample, _ = next(iter(val_loader))
                num_pixels = int(x_sample[0].numel())
                del x_sample

            if logger is not None:
                metrics_row = {'train_loss': train_loss, 'train_recon': train_recon, 'train_kl': train_kl, 'val_loss': val_loss,
                               'val_recon': val_recon, 'val_kl': val_kl, 'beta': current_beta, 'val_psnr': val_psnr,
                               'val_ssim': val_ssim}
                if num_pixels and num_pixels > 0:
                    metrics_row.update({'train_recon_per_pixel': train_recon / num_pixels,
                                        'val_recon_per_pixel': val_recon / num_pixels})
                logger.log_metrics(metrics_row, step=epoch)

            if val_loss < best_val:
                best_val = val_loss
                no_improve = 0
                if checkpoint_dir is not None:
                    torch.save({'model_state_dict': self.model.state_dict(), 'epoch': epoch}, checkpoint_dir / 'best.pt')
            else:
                no_improve += 1
                if early_stop and no_improve >= early_stop:
                    print(f"Early stopping at epoch {epoch}")
                    break

            if scheduler is not None:
                scheduler.step()

        if save_latents_flag and output_dir is not None:
            self.latent_writer(self.model, train_loader, self.device, output_dir / 'latents_train')
            self.latent_writer(self.model, val_loader, self.device, output_dir / 'latents_val')
        if output_dir is not None:
            self._save_recon_grid(val_loader, output_dir, logger)
        if checkpoint_dir is not None:
            torch.save({'model_state_dict': self.model.state_dict(), 'epoch': num_epochs}, checkpoint_dir / 'latest.pt')

    def _save_recon_grid(self, val_loader, output_dir, logger) -> None:
        """recon_grid.png: 8 originals over their 8 reconstructions, both mapped back to [0, 1]."""
        if output_dir is None:
            return
        self.model.eval()
        x, _ = next(iter(val_loader))
        x = x.to(self.device)
        with torch.no_grad():
            x_logits, _, _, _ = self.model(x)
            if getattr(self.model, 'recon_loss', 'mse') == 'bce' or getattr(self.model, 'mse_use_sigmoid', True):
                x_rec = torch.sigmoid(x_logits)
            else:
                x_rec = x_logits
        norm = getattr(val_loader, 'normalize', None)

        def unnormalize(img_batch):
            if norm is None:
                return img_batch
            mean = torch.as_tensor(norm[0], device=img_batch.device).view(1, -1, 1, 1)
            std = torch.as_tensor(norm[1], device=img_batch.device).view(1, -1, 1, 1)
            return img_batch * std + mean

        x_disp = unnormalize(x).clamp(0, 1)
        x_rec_disp = unnormalize(x_rec).clamp(0, 1)
        img_path = output_dir / 'recon_grid.png'
        save_image(torch.cat([x_disp[:8], x_rec_disp[:8]], dim=0), str(img_path), nrow=8)
        if logger is not None:
            logger.log_artifact(img_path)
