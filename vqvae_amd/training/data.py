"""Resident data for the vanilla-VAE trainer: the reference's `get_data_loaders` (src/data/factory.py) without torchvision and
without host workers.  A split's uint8 images live on the device (`DeviceImages` of baseline/data.py); a `ResidentLoader`
yields the (x, y) batches a `DataLoader(dataset, batch_size, shuffle, drop_last=False)` would: ToTensor (x / 255 in float32)
and, for CIFAR-10, Normalize(mean, std) as the same float32 operations.

Order and RNG: every `iter()` makes the DataLoader iterator's base-seed draw from the CPU generator and, when shuffling, the
RandomSampler's (`shuffled_order`), so a seeded run sees the batches a seeded reference run sees.

augment=True.  CIFAR-10: RandomCrop(32, padding=4) + RandomHorizontalFlip on the device, per image, drawn from a generator of
the loader's own that is seeded from the CPU generator when the loader is built: seeded and reproducible, but NOT torchvision's
random stream (torchvision draws inside each worker process, per image).  The grey sets' RandomRotation(10) is not implemented.

Batch assembly.  On a CUDA device a batch is ONE kernel (`assemble_batch`: geo_batch_assemble of csrc/batch.hip, DESIGN.md
section 14) that writes the normalised float32 NCHW batch from the resident uint8 rows, after ONE host-to-device copy that
carries the batch's rows, crop offsets and flips.  On the CPU, or with `fused=False`, a batch is the torch expression the
kernel reproduces bit for bit (`DeviceImages.batch`, `ResidentLoader._augmented`).  Both paths make the same random draws.

Nothing is downloaded: a missing file is eval/data.py's FileNotFoundError.
"""
import ctypes
from typing import Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

from ..baseline.data import DeviceImages, _iterator_seed_draw, shuffled_order
from ..eval import data as files

CIFAR_MEAN = (0.4914, 0.4822, 0.4465)
CIFAR_STD = (0.2470, 0.2430, 0.2610)
ROTATION_MESSAGE = ("augment=True on MNIST / FashionMNIST is torchvision's RandomRotation(10) in the reference; it is not "
                    "implemented for resident data")


CROP_PAD = 4                              # RandomCrop(32, padding=4)


def assemble_batch(images: DeviceImages, rows: torch.Tensor, offset: Optional[torch.Tensor] = None,
                   flip: Optional[torch.Tensor] = None, pad: int = 0) -> torch.Tensor:
    """The float32 NCHW batch of `rows` (host int64 [B], checked against len(images) here) by geo_batch_assemble; `offset`
    (host integers [B][2] = (oy, ox)) and `flip` (host booleans [B]) select the crop of the image padded by `pad` and the
    mirror, None = none.  One host-to-device copy: rows | offsets | flips in one byte buffer.  Asynchronous."""
    from .. import _lib
    if not images.u8.is_cuda:
        raise ValueError("assemble_batch needs images resident on a CUDA device")
    rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1)
    B, (N, H, W, C) = rows.numel(), images.u8.shape
    if B == 0 or int(rows.min()) < 0 or int(rows.max()) >= N:
        raise IndexError(f"batch rows must be a non-empty set of indices in [0, {N})")
    parts = [rows.view(torch.uint8)]
    if offset is not None:
        parts.append(offset.to(torch.int32).reshape(B, 2).contiguous().view(torch.uint8).reshape(-1))
    if flip is not None:
        parts.append(flip.to(torch.uint8).reshape(B))
    dev = images.device
    packed = (torch.cat(parts) if len(parts) > 1 else parts[0]).to(dev)
    at = 8 * B
    p_off = p_flip = None
    if offset is not None:
        p_off, at = packed.data_ptr() + at, at + 8 * B
    if flip is not None:
        p_flip = packed.data_ptr() + at
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.load().geo_batch_assemble(images.u8.data_ptr(), N, H, W, C, packed.data_ptr(), B, p_off, p_flip, int(pad),
                                                  images.mean.data_ptr(), images.std.data_ptr(), out.data_ptr(), stream),
                   "geo_batch_assemble")
    return out


class ResidentLoader:
    """(x float32 NCHW on the device, y int64 on the host) batches over `images`; len() = number of batches.
    `fused`: None = the batch kernel when the images are on a CUDA device, False = the torch expression everywhere."""

    def __init__(self, images: DeviceImages, batch_size: int, shuffle: bool, normalize: Optional[Tuple[Sequence[float], Sequence[float]]] = None,
                 crop_flip: bool = False, fused: Optional[bool] = None):
        self.images, self.batch_size, self.shuffle = images, int(batch_size), bool(shuffle)
        self.normalize = normalize            # (mean, std) the batches carry, for un-normalising a display; None = plain [0, 1]
        self.crop_flip = bool(crop_flip)
        self.fused = images.u8.is_cuda if fused is None else bool(fused)
        if self.fused and not images.u8.is_cuda:
            raise ValueError("fused=True needs images resident on a CUDA device")
        self.aug_rng = None
        if self.crop_flip:
            self.aug_rng = torch.Generator().manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))

    def __len__(self) -> int:
        return (len(self.images) + self.batch_size - 1) // self.batch_size

    def _augmented(self, rows: torch.Tensor) -> torch.Tensor:
        """Pad 4 with zeros, crop at a uniform offset in [0, 8]^2, mirror with probability 1/2: index arithmetic on uint8."""
        im = self.images
        B, H, W = rows.numel(), im.u8.size(1), im.u8.size(2)
        off = torch.randint(0, 2 * CROP_PAD + 1, (B, 2), generator=self.aug_rng)
        flip = torch.rand(B, generator=self.aug_rng) < 0.5
        if self.fused:
            return assemble_batch(im, rows, off, flip, CROP_PAD)
        u8 = torch.nn.functional.pad(im.u8[rows.to(im.device)], (0, 0, 4, 4, 4, 4))        # [B, H + 8, W + 8, C]
        ys = off[:, :1] + torch.arange(H)                                                   # [B, H]
        xs = off[:, 1:] + torch.arange(W)
        xs = torch.where(flip[:, None], xs.flip(1), xs)
        ys, xs = ys.to(im.device), xs.to(im.device)
        crop = u8[torch.arange(B, device=im.device)[:, None, None], ys[:, :, None], xs[:, None, :]]
        x = crop.permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
        return x.sub_(im.mean).div_(im.std)

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        n = len(self.images)
        if self.shuffle:
            batches = [torch.as_tensor(b, dtype=torch.int64) for b in shuffled_order(n, self.batch_size, drop_last=False)]
        else:
            _iterator_seed_draw()
            batches = [torch.arange(s, min(s + self.batch_size, n)) for s in range(0, n, self.batch_size)]
        for rows in batches:
            if self.crop_flip:
                x = self._augmented(rows)
            else:
                x = assemble_batch(self.images, rows) if self.fused else self.images.batch(rows)
            # plain NCHW strides: a one-channel batch permuted from NHWC would otherwise pass for channels-last
            yield x.reshape(x.size(0), -1).view(x.shape), self.images.labels[rows]


def resident_images(images: np.ndarray, labels: np.ndarray, device, normalize=None) -> DeviceImages:
    """uint8 [N, H, W] (grey) or [N, H, W, C] images as DeviceImages; without `normalize` the batches are x / 255 exactly
    (mean 0, std 1 change no bit)."""
    if images.ndim == 3:
        images = images[..., None]
    c = images.shape[-1]
    mean, std = normalize if normalize is not None else ((0.0,) * c, (1.0,) * c)
    return DeviceImages(images, labels, device, mean, std, img_size=images.shape[1])


def get_data_loaders(name: str, root: str, batch_size: int, device, augment: bool = False, **_host_loader_options):
    """(train_loader, val_loader) for "MNIST", "FashionMNIST" (also fashion-mnist, fashion_mnist) or "CIFAR10", case-insensitive;
    an unknown name falls back to MNIST as in the reference.  num_workers / pin_memory / persistent_workers of the
    reference's YAML are accepted and unused: there is no host loader."""
    key = str(name).strip().lower()
    if key == "cifar10":
        norm = (CIFAR_MEAN, CIFAR_STD)
        train = resident_images(*files.cifar10_train(root), device, norm)
        test = resident_images(*files.cifar10_test(root), device, norm)
        return (ResidentLoader(train, batch_size, True, norm, crop_flip=augment), ResidentLoader(test, batch_size, False, norm))
    if augment:
        raise NotImplementedError(ROTATION_MESSAGE)
    folder = "FashionMNIST" if key in {"fashionmnist", "fashion-mnist", "fashion_mnist"} else "MNIST"
    train = resident_images(*files.idx_split(root, folder, train=True), device)
    test = resident_images(*files.idx_split(root, folder, train=False), device)
    return ResidentLoader(train, batch_size, True), ResidentLoader(test, batch_size, False)
