"""Generated samples against real ones on the MI355X: drop-in for the reference's src/eval/evaluate_model.py (same
--config yaml, same metrics.yaml PSNR / SSIM strings and comparison_grid.png).

    python -m vqvae_amd.scripts.evaluate_model --config configs/fashionmnist/spatial/geodesic/evaluate.yaml [--data_root data]

The generated grid (`generated_path`) is cut into num_samples // samples_per_class rows of samples_per_class cells, each cell
resized to image_size with F.interpolate(mode="bilinear", antialias=True) -- what torchvision's tensor resize calls -- unless
it already has that size.  Real images are the first samples_per_class test images of each class, in class order, read from
the files torchvision leaves under --data_root (vqvae_amd.eval.data; nothing is downloaded).  PSNR and SSIM run on the GPU
(vqvae_amd.eval.metrics).

LPIPS (AlexNet, v0.1) is computed when its weights are given, by --lpips_weights PATH or the config key `lpips_weights` (the
flag wins): the file `torch.save(lpips.LPIPS(net='alex').state_dict(), PATH)` writes on a machine that has the package
(vqvae_amd.eval.lpips).  Both image sets go through the reference's preprocess_for_lpips (three channels,
bilinear resize to 64, [-1, 1]) and the pairs through the HIP kernels; metrics.yaml gains the reference's "LPIPS" string and
the printed line is the reference's.  Without weights nothing can be fetched here, so metrics.yaml has no LPIPS key and the
output is what it was before.
"""
import argparse
from pathlib import Path
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F
import yaml
from PIL import Image

from .._device import device
from ..eval.data import load_test_split, to_tensor
from ..eval.lpips import load_lpips_weights, lpips_mean, preprocess_for_lpips
from ..eval.metrics import psnr, ssim_simple
from .generate_samples import save_image


def load_images(path_or_name: str, num_images: int, size: int, dataset_name: str, is_real_data: bool = False,
                samples_per_class: Optional[int] = None, data_root: str = "data") -> torch.Tensor:
    if is_real_data:
        images, labels = load_test_split(dataset_name, data_root)
        if samples_per_class is not None:
            num_classes = num_images // samples_per_class
            class_samples = {i: [] for i in range(num_classes)}
            for img, label in zip(images, labels.tolist()):
                if len(class_samples[label]) < samples_per_class:
                    class_samples[label].append(to_tensor(img, size))
                if all(len(s) >= samples_per_class for s in class_samples.values()):
                    break
            out = []
            for class_id in range(num_classes):
                out.extend(class_samples[class_id][:samples_per_class])
            return torch.stack(out)
        return torch.stack([to_tensor(images[i], size) for i in range(num_images)])
    grid = np.array(Image.open(path_or_name).convert("RGB"), copy=True)
    grid_tensor = torch.from_numpy(grid).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    if samples_per_class is None:
        raise ValueError("`samples_per_class` must be provided for loading an image grid.")
    num_rows = num_images // samples_per_class
    _, grid_h, grid_w = grid_tensor.shape
    cell_h, cell_w = grid_h // num_rows, grid_w // samples_per_class
    cells = []
    for row in range(num_rows):
        for col in range(samples_per_class):
            img = grid_tensor[:, row * cell_h:(row + 1) * cell_h, col * cell_w:(col + 1) * cell_w]
            if tuple(img.shape[1:]) != (size, size):
                img = F.interpolate(img.unsqueeze(0), size=(size, size), mode="bilinear", align_corners=False,
                                    antialias=True).squeeze(0)
            cells.append(img)
    return torch.stack(cells)


def normalize_each(images: torch.Tensor) -> torch.Tensor:
    """make_grid's normalize=True, scale_each=True: every image mapped from its own [min, max] to [0, 1]."""
    out = images.clone()
    for t in out:
        low, high = float(t.min()), float(t.max())
        t.clamp_(min=low, max=high)
        t.sub_(low).div_(max(high - low, 1e-5))
    return out


def main(config_path: str, data_root: str = "data", lpips_weights: Optional[str] = None) -> int:
    with open(config_path, "r") as f:
        config = yaml.safe_load(f)
    dev = device()
    dataset_name = config.get("dataset_name", config.get("data", {}).get("dataset_name", "fashionmnist"))
    samples_per_class = config.get("samples_per_class")

    generated = load_images(config["generated_path"], config["num_samples"], config["image_size"], dataset_name,
                            is_real_data=False, samples_per_class=samples_per_class).to(dev)
    real = load_images(dataset_name, config["num_samples"], config["image_size"], dataset_name, is_real_data=True,
                       samples_per_class=samples_per_class, data_root=data_root).to(dev)

    psnr_val = psnr(generated, real)
    ssim_val = ssim_simple(generated, real)
    results = {"PSNR": f"{psnr_val:.4f}", "SSIM": f"{ssim_val:.4f}"}
    weights = lpips_weights if lpips_weights is not None else config.get("lpips_weights")
    if weights is not None:
        lpips_val = lpips_mean(load_lpips_weights(weights), preprocess_for_lpips(generated), preprocess_for_lpips(real))
        results["LPIPS"] = f"{lpips_val:.4f}"
        print(f"PSNR: {psnr_val:.4f}, SSIM: {ssim_val:.4f}, LPIPS: {lpips_val:.4f}")
    else:
        print(f"PSNR: {psnr_val:.4f}, SSIM: {ssim_val:.4f}")
        print("LPIPS not computed: it needs AlexNet weights, which are not available here")

    out_dir = Path(config["out_dir"])
    out_dir.mkdir(parents=True, exist_ok=True)
    with open(out_dir / "metrics.yaml", "w") as f:
        yaml.dump(results, f)

    if samples_per_class is not None:
        num_classes = config["num_samples"] // samples_per_class
        comparison = []
        for class_id in range(min(num_classes, 5)):
            start = class_id * samples_per_class
            for i in range(2):
                comparison.append(real[start + i])
                comparison.append(generated[start + i])
        save_image(normalize_each(torch.stack(comparison)), out_dir / "comparison_grid.png", nrow=4)
    else:
        save_image(torch.cat([real[:8], generated[:8]], 0), out_dir / "comparison_grid.png", nrow=8)
    print(f"Results saved to {out_dir}")
    return 0


def make_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Compare generated samples with real ones (PSNR, SSIM, LPIPS)")
    parser.add_argument("--config", type=str, required=True, help="Path to the evaluation config file.")
    parser.add_argument("--data_root", type=str, default="data", help="Where torchvision left the test split")
    parser.add_argument("--lpips_weights", type=str, default=None,
                        help="State dict of lpips.LPIPS(net='alex'); overrides the config key lpips_weights.  Without it no LPIPS")
    return parser


if __name__ == "__main__":
    a = make_parser().parse_args()
    raise SystemExit(main(a.config, a.data_root, a.lpips_weights))
