"""Test images without torchvision: readers for the files torchvision's FashionMNIST and CIFAR10 datasets leave under their
root, and the transforms the reference's evaluation scripts apply (Resize, ToTensor, grey to RGB).  Nothing is downloaded:
a missing file is a FileNotFoundError that names the paths looked for.

    <root>/FashionMNIST/raw/t10k-images-idx3-ubyte[.gz], t10k-labels-idx1-ubyte[.gz]
    <root>/FashionMNIST/raw/train-images-idx3-ubyte[.gz], train-labels-idx1-ubyte[.gz]      (MNIST/raw likewise)
    <root>/cifar-10-batches-py/test_batch, data_batch_1 .. data_batch_5
"""
import gzip
import os
import pickle
from typing import Optional, Tuple

import numpy as np
import torch
from PIL import Image

_IDX_DTYPES = {0x08: np.uint8, 0x09: np.int8, 0x0B: np.dtype(">i2"), 0x0C: np.dtype(">i4"), 0x0D: np.dtype(">f4"),
               0x0E: np.dtype(">f8")}


def _find(path: str) -> str:
    for p in (path, path + ".gz"):
        if os.path.exists(p):
            return p
    raise FileNotFoundError(f"dataset file not found: {path} (or {path}.gz); nothing is downloaded, place the file there")


def read_idx(path: str) -> np.ndarray:
    """An idx file (the MNIST format: zero, zero, type, rank, big-endian u32 dims, data), gzipped or not."""
    p = _find(path)
    with (gzip.open(p, "rb") if p.endswith(".gz") else open(p, "rb")) as f:
        raw = f.read()
    if len(raw) < 4 or raw[0] != 0 or raw[1] != 0 or raw[2] not in _IDX_DTYPES:
        raise ValueError(f"{p}: not an idx file")
    rank = raw[3]
    dims = tuple(int.from_bytes(raw[4 + 4 * i:8 + 4 * i], "big") for i in range(rank))
    dt = np.dtype(_IDX_DTYPES[raw[2]])
    data = np.frombuffer(raw, dtype=dt, offset=4 + 4 * rank, count=int(np.prod(dims)))
    return data.reshape(dims).astype(dt.newbyteorder("="))


def fashionmnist_test(root: str) -> Tuple[np.ndarray, np.ndarray]:
    """(images uint8 [N, 28, 28], labels int64 [N]) of the FashionMNIST test split under `root`."""
    raw = os.path.join(root, "FashionMNIST", "raw")
    images = read_idx(os.path.join(raw, "t10k-images-idx3-ubyte"))
    labels = read_idx(os.path.join(raw, "t10k-labels-idx1-ubyte")).astype(np.int64)
    return images, labels


def idx_split(root: str, dataset: str, train: bool) -> Tuple[np.ndarray, np.ndarray]:
    """(images uint8 [N, 28, 28], labels int64 [N]) of one split of an idx-format data set ("FashionMNIST" or "MNIST":
    torchvision's folder names) under `root`: train-* for the training split, t10k-* for the test split."""
    raw = os.path.join(root, dataset, "raw")
    stem = "train" if train else "t10k"
    images = read_idx(os.path.join(raw, f"{stem}-images-idx3-ubyte"))
    labels = read_idx(os.path.join(raw, f"{stem}-labels-idx1-ubyte")).astype(np.int64)
    return images, labels


def fashionmnist_train(root: str) -> Tuple[np.ndarray, np.ndarray]:
    """(images uint8 [N, 28, 28], labels int64 [N]) of the FashionMNIST training split under `root`."""
    return idx_split(root, "FashionMNIST", train=True)


def mnist_train(root: str) -> Tuple[np.ndarray, np.ndarray]:
    return idx_split(root, "MNIST", train=True)


def mnist_test(root: str) -> Tuple[np.ndarray, np.ndarray]:
    return idx_split(root, "MNIST", train=False)


def _cifar10_batches(root: str, names) -> Tuple[np.ndarray, np.ndarray]:
    images, labels = [], []
    for name in names:
        path = os.path.join(root, "cifar-10-batches-py", name)
        if not os.path.exists(path):
            raise FileNotFoundError(f"dataset file not found: {path}; nothing is downloaded, place the file there")
        with open(path, "rb") as f:
            entry = pickle.load(f, encoding="latin1")
        images.append(np.asarray(entry["data"], dtype=np.uint8).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1))
        labels.append(np.asarray(entry["labels"] if "labels" in entry else entry["fine_labels"], dtype=np.int64))
    return np.ascontiguousarray(np.concatenate(images)), np.concatenate(labels)


def cifar10_test(root: str) -> Tuple[np.ndarray, np.ndarray]:
    """(images uint8 [N, 32, 32, 3], labels int64 [N]) of the CIFAR-10 test batch under `root` (torchvision's layout)."""
    return _cifar10_batches(root, ["test_batch"])


def cifar10_train(root: str) -> Tuple[np.ndarray, np.ndarray]:
    """(images uint8 [N, 32, 32, 3], labels int64 [N]) of the CIFAR-10 training split under `root`: data_batch_1 .. 5
    concatenated in that order, which is torchvision's CIFAR10(train=True) order."""
    return _cifar10_batches(root, [f"data_batch_{i}" for i in range(1, 6)])


def load_test_split(name: str, root: str = "data") -> Tuple[np.ndarray, np.ndarray]:
    """The test split of "fashionmnist" or "cifar10" (case-insensitive)."""
    if name.lower() == "fashionmnist":
        return fashionmnist_test(root)
    if name.lower() == "cifar10":
        return cifar10_test(root)
    raise ValueError(f"Unknown dataset: {name}")


def to_tensor(img: np.ndarray, size: Optional[int] = None) -> torch.Tensor:
    """transforms.Compose([Resize((size, size)) if size, ToTensor(), grey -> 3 channels]) of one uint8 image (H, W) or
    (H, W, 3).  Resize is PIL's bilinear resize, which is what torchvision calls on PIL images; at the native size PIL returns
    a copy, so it changes nothing."""
    if size is not None:
        pil = Image.fromarray(img, mode="L" if img.ndim == 2 else "RGB")
        img = np.array(pil.resize((size, size), Image.BILINEAR), copy=True)
    t = torch.from_numpy(np.array(img, copy=True))
    t = t.view(t.shape[0], t.shape[1], -1).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return t.repeat(3, 1, 1) if t.size(0) == 1 else t
