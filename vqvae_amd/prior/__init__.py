"""Autoregressive prior over geodesic codes: the consumer of codes.npy, trained data-parallel, sampled with a
KV-cached HIP decode."""
from .sampling import sample  # noqa: F401
from .transformer import Transformer  # noqa: F401
