"""CIFAR-10 for the baseline without torchvision: the uint8 images stay resident on the device and each batch gets the
reference's transform, Resize(img_size) -> ToTensor -> Normalize(mean, std), as the same float32 operations (x / 255, then
(x - mean) / std).  Resize at the native 32 x 32 returns the image unchanged; another size is PIL's bilinear resize, applied
once when the split is loaded.

Batch order and RNG: every `iter(DataLoader)` of the reference draws one int64 from the CPU generator (the iterator's base seed)
and, with shuffle=True, RandomSampler draws its seed from it at the first batch.  `shuffled_batches` and `ordered_batches` make
exactly those draws, so a run consumes the CPU RNG in the reference's order and a shuffled epoch holds the same images in the
same batches.
"""
from typing import Iterator, List, Sequence

import numpy as np
import torch
from PIL import Image
from torch.utils.data import RandomSampler

from ..eval.data import cifar10_test, cifar10_train


def _iterator_seed_draw() -> None:
    """The base-seed draw of torch.utils.data's _BaseDataLoaderIter.__init__ (generator=None)."""
    torch.empty((), dtype=torch.int64).random_()


class DeviceImages:
    """uint8 images [N, H, W, 3] resident on `device`; batch(i) = the normalised float32 NCHW batch of rows i."""

    def __init__(self, images: np.ndarray, labels: np.ndarray, device, mean: Sequence[float], std: Sequence[float],
                 img_size: int = 32):
        if images.shape[1] != img_size or images.shape[2] != img_size:
            images = np.stack([np.array(Image.fromarray(im).resize((img_size, img_size), Image.BILINEAR)) for im in images])
        self.device = torch.device(device)
        self.u8 = torch.from_numpy(np.ascontiguousarray(images)).to(self.device)
        self.labels = torch.from_numpy(np.asarray(labels, dtype=np.int64))
        self.mean = torch.as_tensor(mean, dtype=torch.float32, device=self.device).view(-1, 1, 1)
        self.std = torch.as_tensor(std, dtype=torch.float32, device=self.device).view(-1, 1, 1)

    def __len__(self) -> int:
        return self.u8.shape[0]

    def batch(self, rows) -> torch.Tensor:
        if not isinstance(rows, slice):
            rows = torch.as_tensor(rows, dtype=torch.int64).to(self.device)
        x = self.u8[rows].permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
        return x.sub_(self.mean).div_(self.std)

    def shuffled_batches(self, batch_size: int) -> Iterator[torch.Tensor]:
        """DataLoader(shuffle=True, drop_last=True): the iterator's seed draw now, the sampler's at the first batch."""
        _iterator_seed_draw()
        return self._shuffled(batch_size)

    def _shuffled(self, batch_size: int) -> Iterator[torch.Tensor]:
        order: List[int] = []
        for i in RandomSampler(range(len(self))):
            order.append(i)
            if len(order) == batch_size:
                yield self.batch(order)
                order = []

    def ordered_batches(self, batch_size: int) -> Iterator[torch.Tensor]:
        """DataLoader(shuffle=False, drop_last=False)."""
        _iterator_seed_draw()
        return (self.batch(slice(s, s + batch_size)) for s in range(0, len(self), batch_size))


def shuffled_order(n: int, batch_size: int, drop_last: bool = True) -> List[List[int]]:
    """The batches of indices a DataLoader(shuffle=True, drop_last=drop_last) over n items yields, with the same CPU RNG draws."""
    _iterator_seed_draw()
    out, cur = [], []
    for i in RandomSampler(range(n)):
        cur.append(i)
        if len(cur) == batch_size:
            out.append(cur)
            cur = []
    if cur and not drop_last:
        out.append(cur)
    return out


def load_split(cfg: dict, split: str, device) -> DeviceImages:
    """The "train" or "test" split of CIFAR-10 under cfg["data"]["root"], on `device`, with the config's transform."""
    d = cfg["data"]
    images, labels = (cifar10_train if split == "train" else cifar10_test)(d["root"])
    return DeviceImages(images, labels, device, d["normalize_mean"], d["normalize_std"], d.get("img_size", 32))
