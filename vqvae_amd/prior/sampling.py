"""Sampling from the code prior: the reference's `sample` (src/scripts/generate_samples.py:19-31) with a KV-cached HIP decode.

The reference re-runs the whole forward on the growing prefix at every step and draws with torch.multinomial.  On the GPU,
inside the covered envelope (`kernel_covers`), `sample` computes every position once in csrc/prior_sample.hip and draws each
token from a uniform u handed to the kernel by the draw rule below.  Elsewhere -- CPU tensors, shapes outside the envelope,
a checkpoint with non-standard attention masks -- it runs the reference's loop over `Transformer.forward`.

Draw rule (`draw_rule`; the kernel and this restatement share it):
  1. l = logits / temperature (f32 division, as the reference);
  2. with top_k: keep every i with l_i >= the k-th largest l -- ties at the k-th value are all kept (top_k_logits);
  3. p_i = exp(l_i - max l) over the kept i, 0 elsewhere;
  4. the token is the smallest i whose prefix sum in index order exceeds u * sum(p); if rounding leaves none, the last
     kept index.  A dropped index is never drawn.
Stochastic sequences are therefore reproducible per torch seed (the uniforms come from torch.rand, Philox on the GPU) but
are NOT the reference's torch.multinomial stream.  Greedy (top_k=1) and explicit-uniform results are exact.
"""
import ctypes
from typing import Optional

import torch

from .. import _lib
from .._device import ptr, stream_ptr
from .transformer import Transformer

MAX_SEQ_LEN, MAX_TOKENS, MAX_EMBED = 16, 1024, 512
_BLOCK_TENSORS = ("ln1.weight", "ln1.bias", "ln2.weight", "ln2.bias", "attn.c_attn.weight", "attn.c_attn.bias",
                  "attn.c_proj.weight", "attn.c_proj.bias", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias")


def top_k_logits(logits: torch.Tensor, k: int) -> torch.Tensor:
    """The reference's filter (generate_samples.py:12-16): -inf below the k-th largest value, every tie at it kept."""
    v, _ = torch.topk(logits, k)
    out = logits.clone()
    out[out < v[:, [-1]]] = -float("Inf")
    return out


def kept_mask(l: torch.Tensor, top_k: Optional[int]) -> torch.Tensor:
    """Step 2 of the draw rule on already-tempered logits l [B, V]."""
    if not top_k:
        return torch.ones_like(l, dtype=torch.bool)
    return l >= torch.topk(l, top_k).values[:, -1:]


def draw_rule(logits: torch.Tensor, u: torch.Tensor, temperature: float = 1.0, top_k: Optional[int] = None) -> torch.Tensor:
    """Host restatement of the kernel's draw: logits f32 [B, V], u f32 [B] -> int64 [B]."""
    l = logits.float() / temperature
    keep = kept_mask(l, top_k)
    p = torch.where(keep, torch.exp(l - l.max(dim=-1, keepdim=True).values), torch.zeros_like(l))
    c = torch.cumsum(p, dim=-1)
    over = c > u.float()[:, None] * c[:, -1:]
    V = l.shape[-1]
    last_kept = V - 1 - keep.flip(-1).to(torch.int64).argmax(dim=-1)
    first = over.to(torch.int64).argmax(dim=-1)
    return torch.where(over.any(dim=-1), first, last_kept)


def kernel_covers(model: Transformer) -> bool:
    """The shapes csrc/prior_sample.hip is built for, with the standard lower-triangular attention mask."""
    C, H = model.embed_dim, model.n_head
    return (model.max_seq_len <= MAX_SEQ_LEN and C % H == 0 and C // H in (16, 32, 64) and C % 64 == 0 and C <= MAX_EMBED
            and model.num_tokens <= MAX_TOKENS and model._standard_mask)


def _check_limits(model: Transformer, T0: int, steps: int, top_k: Optional[int]) -> None:
    if T0 + steps - 1 > model.max_seq_len:       # the reference's model asserts on its last call's input (length T0+steps-1)
        raise AssertionError(f"Sequence length {T0 + steps - 1} exceeds model max length {model.max_seq_len}")
    if top_k is not None and not 1 <= top_k <= model.num_tokens:
        raise ValueError(f"top_k {top_k} outside 1..num_tokens ({model.num_tokens})")


def _desc(model: Transformer):
    idx = {s.name: s.offset for s in model.layout}
    blocks = (ctypes.c_int64 * (12 * model.n_layers))(*[idx[f"blocks.{i}.{n}"] for i in range(model.n_layers)
                                                         for n in _BLOCK_TENSORS])
    d = _lib.PriorDesc(model.num_tokens, model.embed_dim, model.n_layers, model.n_head, model.max_seq_len, model.num_classes,
                       ctypes.c_void_p(model.arena.data_ptr()), idx["pos_emb"], idx["token_emb.weight"],
                       idx.get("class_emb.weight", -1), idx["ln_f.weight"], idx["ln_f.bias"], idx["head.weight"],
                       ctypes.cast(blocks, ctypes.POINTER(ctypes.c_int64)))
    return d, blocks


def _workspace(nbytes: int, dev) -> torch.Tensor:
    """The decode's scratch: one exact-size allocation per call from the stream-ordered caching allocator (no device sync)."""
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def sample_native(model: Transformer, x: torch.Tensor, steps: int, temperature: float, top_k: Optional[int],
                  y: Optional[torch.Tensor], uniforms: Optional[torch.Tensor], return_logits: bool = False):
    """The HIP decode (csrc/prior_sample.hip).  Returns tokens int64 [B, T0 + steps] (and, with return_logits, the logits of
    every position f32 [B, T0 + steps - 1, V], teacher-forced over the prompt)."""
    B, T0 = x.shape
    dev = x.device
    _check_limits(model, T0, steps, top_k)
    if not kernel_covers(model):
        raise _lib.GeoHipError("the model is outside the decode kernel's envelope (use sample())")
    V = model.num_tokens
    x = x.to(torch.int64).contiguous()
    if int(x.min()) < 0 or int(x.max()) >= V:
        raise ValueError(f"prompt tokens outside [0, {V})")
    if y is not None:
        y = y.to(device=dev, dtype=torch.int64).contiguous()
        if y.shape != (B,) or model.num_classes == 0 or int(y.min()) < 0 or int(y.max()) >= model.num_classes:
            raise ValueError(f"labels must be int [B] in [0, {model.num_classes})")
    if steps > 0:
        if uniforms is None:
            raise ValueError("uniforms required")
        uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
        if uniforms.shape != (B, steps):
            raise ValueError(f"uniforms must be [{B}, {steps}], got {tuple(uniforms.shape)}")
    arena = model.arena.detach()
    if not (arena.is_cuda and arena.device == dev and arena.is_contiguous()):
        raise ValueError("model and prompt must be on the same GPU")
    tokens = torch.empty((B, T0 + steps), dtype=torch.int64, device=dev)
    logits = (torch.empty((B, max(T0 + steps - 1, 1), V), dtype=torch.float32, device=dev) if return_logits else None)
    L = _lib.load()
    desc, _blocks = _desc(model)
    nbytes = L.geo_prior_sample_workspace_bytes(ctypes.byref(desc), B, max(T0 + steps - 1, 1))
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(L.geo_prior_sample(ctypes.byref(desc), ptr(x), T0, steps, ptr(y), ptr(uniforms) if steps else None,
                                      float(temperature), int(top_k or 0), ptr(tokens), ptr(logits), B, ptr(ws), nbytes,
                                      stream_ptr()), "geo_prior_sample")
    return (tokens, logits) if return_logits else tokens


@torch.no_grad()
def sample(model: Transformer, x: torch.Tensor, steps: int, temperature: float = 1.0, top_k: Optional[int] = None,
           y: Optional[torch.Tensor] = None, *, uniforms: Optional[torch.Tensor] = None,
           generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """`x` (int64 [B, T0]) extended by `steps` tokens, as the reference's sample(model, x, steps, temperature, top_k, y).

    On the GPU inside `kernel_covers(model)`: the KV-cached HIP decode, tokens picked by the draw rule from
    uniforms = torch.rand(B, steps, generator=generator) (or the `uniforms` given).  Otherwise the reference's loop over
    Transformer.forward: torch.multinomial as the reference when neither `uniforms` nor `generator` is given (identical
    results on the CPU under the same torch seed), the draw rule when either is."""
    model.eval()
    B, T0 = x.shape
    _check_limits(model, T0, steps, top_k)
    if uniforms is None and (generator is not None or (x.is_cuda and kernel_covers(model))):
        uniforms = torch.rand((B, steps), device=x.device, generator=generator)
    if x.is_cuda and kernel_covers(model):
        return sample_native(model, x, steps, temperature, top_k, y, uniforms)
    for k in range(steps):
        logits = model(x, y=y)[:, -1, :]
        if uniforms is not None:
            ix = draw_rule(logits, uniforms[:, k].to(logits.device), temperature, top_k)[:, None]
        else:
            logits = logits / temperature
            if top_k is not None:
                logits = top_k_logits(logits, top_k)
            ix = torch.multinomial(torch.softmax(logits, dim=-1), num_samples=1)
        x = torch.cat((x, ix), dim=1)
    return x


__all__ = ["sample", "sample_native", "draw_rule", "top_k_logits", "kept_mask", "kernel_covers"]
