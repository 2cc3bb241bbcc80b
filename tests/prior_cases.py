"""Shared inputs of the code prior's envelope tests (test_prior_cases_host.py checks them on the CPU,
test_gpu_prior_envelope.py and test_gpu_prior_sample.py run the kernels against them).  Not a test module.

forward_fp64       Transformer.forward in eval mode restated with elementary float64 operations: the reference every
                   decode test compares with, so that no kernel of this project stands on both sides.
DECODE_SHAPES      model configurations of the decode envelope no other test launches.
exact_logit_model  a model whose logits are a given vector s exactly, in any summation order.
DRAW_CASES         (name, s, temperature, top_k, u, want): rows of uniforms whose draw is decided by the inputs alone.
"""
import math

import numpy as np
import torch

# ------------------------------------------------------------------------------------------------ float64 forward


def _layer_norm64(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)                       # biased, as F.layer_norm
    return (x - mu) / torch.sqrt(var + 1e-5) * w + b


def forward_fp64(model, idx, y=None):
    """Logits float64 [B, T, num_tokens] of the eval-mode model on idx int64 [B, T] (and labels y [B]), on idx's device."""
    p = {k: v.detach().to(device=idx.device, dtype=torch.float64) for k, v in model.views().items()}
    (B, T), C, H = idx.shape, model.embed_dim, model.n_head
    D = C // H
    x = p["token_emb.weight"][idx] + p["pos_emb"][0, :T]
    if y is not None:
        x = x + p["class_emb.weight"][y][:, None, :]
    causal = torch.ones(T, T, dtype=torch.bool, device=idx.device).tril()
    for i in range(model.n_layers):
        b = f"blocks.{i}."
        qkv = _layer_norm64(x, p[b + "ln1.weight"], p[b + "ln1.bias"]) @ p[b + "attn.c_attn.weight"].T + p[b + "attn.c_attn.bias"]
        q, k, v = qkv.view(B, T, 3, H, D).permute(2, 0, 3, 1, 4)         # each [B, H, T, D]
        s = torch.where(causal, q @ k.transpose(-2, -1) / math.sqrt(D), torch.full((), -math.inf, dtype=torch.float64, device=idx.device))
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        a = ((e / e.sum(-1, keepdim=True)) @ v).transpose(1, 2).reshape(B, T, C)
        x = x + a @ p[b + "attn.c_proj.weight"].T + p[b + "attn.c_proj.bias"]
        h = _layer_norm64(x, p[b + "ln2.weight"], p[b + "ln2.bias"]) @ p[b + "mlp.0.weight"].T + p[b + "mlp.0.bias"]
        h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))             # exact GELU
        x = x + h @ p[b + "mlp.2.weight"].T + p[b + "mlp.2.bias"]
    return _layer_norm64(x, p["ln_f.weight"], p["ln_f.bias"]) @ p["head.weight"].T


# ------------------------------------------------------------------------------------------------ decode shapes
# embed_dim 192 / 320 / 448: ps_linear_kernel<EPI, 64> with 3 / 5 / 7 chunks (its register prefetch), LayerNorm statistics
# over a K that is no multiple of 128; H = 3 and 7: partly filled attention workgroups; num_tokens 1024 / 1023 / 2 / 1: the
# draw workgroup's last thread full, partly valid, and a single valid thread; max_seq_len 1: a single position.
DECODE_SHAPES = {
    "c192_h3_v1024": dict(num_classes=0, num_tokens=1024, embed_dim=192, n_layers=2, n_head=3, max_seq_len=16),
    "c192_h12_v1023": dict(num_classes=3, num_tokens=1023, embed_dim=192, n_layers=2, n_head=12, max_seq_len=7),
    "c320_h10_v100": dict(num_classes=0, num_tokens=100, embed_dim=320, n_layers=2, n_head=10, max_seq_len=16),
    "c448_h7_v2": dict(num_classes=2, num_tokens=2, embed_dim=448, n_layers=1, n_head=7, max_seq_len=5),
    "c64_h1_v1": dict(num_classes=0, num_tokens=1, embed_dim=64, n_layers=2, n_head=1, max_seq_len=16),
    "c384_h6_v513": dict(num_classes=0, num_tokens=513, embed_dim=384, n_layers=1, n_head=6, max_seq_len=1),
}



def seeded_model(cfg, seed, device="cpu"):
    """An eval-mode Transformer of configuration cfg with oracle.synthetic's seeded weights (non-trivial LayerNorm scales and
    biases everywhere) and the standard causal mask."""
    from oracle import synthetic as syn
    from vqvae_amd.prior import Transformer
    model = Transformer(**cfg, dropout=0.1)
    sd = syn.seeded_state_dict(model.state_dict(), seed)
    T = cfg["max_seq_len"]
    for k in sd:
        if k.endswith(".attn.bias"):
            sd[k] = torch.tril(torch.ones(T, T)).view(1, 1, T, T)
    model.load_state_dict(sd)
    return model.to(device).eval()


# ------------------------------------------------------------------------------------------------ exact logits
EXACT_C = 64


def exact_logit_model(s, device="cpu"):
    """A one-layer model whose logits are s (f32 [V]) at every position.  ln_f has weight 0 and bias 1, so the head sees a
    row of ones, and head.weight[i, :] = s[i] / 64.  For s made of multiples of 2^-11 below 1 in magnitude every partial sum
    m * s[i] / 64 (m <= 64) of the head's 64 products has at most 17 significant bits: exact in float32 in any order.
    (A sum that starts from +0.0 never ends in -0.0: an s[i] of -0.0 comes out as +0.0.)"""
    from vqvae_amd.prior import Transformer
    s = torch.as_tensor(s, dtype=torch.float32)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1234)
        model = Transformer(num_classes=0, num_tokens=len(s), embed_dim=EXACT_C, n_layers=1, n_head=4, max_seq_len=2, dropout=0.1)
    with torch.no_grad():
        v = model.views()
        v["ln_f.weight"].zero_()
        v["ln_f.bias"].fill_(1.0)
        v["head.weight"].copy_((s / EXACT_C)[:, None].expand(len(s), EXACT_C))
    return model.to(device).eval()


# ------------------------------------------------------------------------------------------------ draw cases
MIN_HALF_STEP = 3e-4     # of the total mass: 5x the worst float32 prefix-sum error over 1024 terms, 1024 * 2^-24 = 6.1e-5
U_BELOW_ONE = 1.0 - 2.0 ** -24


def tempered(s, temperature):
    """l = s / temperature as the kernel and draw_rule form it: one float32 division."""
    return torch.as_tensor(s, dtype=torch.float32) / temperature


def cdf64(s, temperature, top_k):
    """(kept bool [V], inclusive prefix sums float64 [V] of p over the kept set in index order).  Each p is exp in float64
    rounded to the float32 number a mass is held in (so a mass that underflows in float32 is 0 here too); the sums, which
    are where the order of a float32 scan could matter, are float64."""
    from vqvae_amd.prior.sampling import kept_mask
    l = tempered(s, temperature)
    kept = kept_mask(l[None], top_k)[0].numpy()
    l64 = l.double().numpy()
    p = np.where(kept, np.exp(l64 - l64.max()).astype(np.float32).astype(np.float64), 0.0)
    return kept, np.cumsum(p)


def midpoint_rows(s, temperature, top_k):
    """One u per kept index with positive mass: the midpoint of its step in the float64 CDF.  -> (u f32, want int64)."""
    kept, c = cdf64(s, temperature, top_k)
    lo = np.concatenate(([0.0], c[:-1]))
    idx = np.nonzero(kept & (c > lo))[0]
    u = (0.5 * (lo[idx] + c[idx]) / c[-1]).astype(np.float32)
    return u, idx.astype(np.int64)


def _flat_rows(V, on_steps):
    """Rows for V equal logits (p = 1 each, integer prefix sums): the midpoint of every step, u = 0, the largest u below 1
    and u = 1; with on_steps (V a power of two, so b / V and u * V are exact) also every u that lands ON a step: the prefix
    sum must EXCEED u * S, so u = b / V gives b and not b - 1."""
    b = np.arange(V)
    u = [(b + 0.5) / V, [0.0, U_BELOW_ONE, 1.0]]
    want = [b, [0, V - 1, V - 1]]
    if on_steps:
        u.append(b / V)
        want.append(b)
    return np.concatenate(u).astype(np.float32), np.concatenate(want).astype(np.int64)


def spread_logits():
    """Case d: the 1024 multiples of 2^-11 in [-0.25, 0.25) in a seeded permutation with a positive value at index 17 and a
    negative one at 900, which then become +0.0 and -0.0: with the permutation's own 0.0, 510 positive values, three zeros
    and 511 negative ones."""
    r = np.random.RandomState(2024)
    s = (np.arange(-512, 512) * 2.0 ** -11)[r.permutation(1024)]
    for at, sign in ((17, 1.0), (900, -1.0)):
        if s[at] * sign <= 0:
            j = next(j for j in range(1024) if j not in (17, 900) and s[j] * sign > 0 and abs(s[j]) > 2.0 ** -11)
            s[at], s[j] = s[j], s[at]
    s[17], s[900] = 0.0, -0.0
    return s.astype(np.float32)


def tied_logits(value):
    """Case e: spread_logits with indices 5, 300 and 1023 (waves 0, 1 and 3 of the draw workgroup) at one common value.
    -> (s, number of entries above the value, number of entries at it)."""
    s = spread_logits()
    s[[5, 300, 1023]] = value
    return s, int((s > value).sum()), int((s == value).sum())


TOP_KS_D = (None, 1, 2, 3, 255, 256, 257, 511, 512, 513, 1023)
TEMPERATURES_D = (0.7, 1.0, 1.5)


def _build_draw_cases():
    cases = []
    flat = np.zeros(1024, np.float32)
    cases.append(("a_flat_v1024", flat, 1.0, None) + _flat_rows(1024, True))
    for k in (1, 2, 511, 1023):                                 # all keys equal: everything ties, everything is kept
        cases.append((f"b_flat_v1024_k{k}", flat, 1.0, k) + _flat_rows(1024, True))
    for V in (1023, 513, 5, 1):
        cases.append((f"c_flat_v{V}", np.zeros(V, np.float32), 1.0, None) + _flat_rows(V, False))
    d = spread_logits()
    for temperature in TEMPERATURES_D:
        for k in TOP_KS_D:
            cases.append((f"d_spread_T{temperature}_k{k}", d, temperature, k) + midpoint_rows(d, temperature, k))
    for value in (0.125, -0.125):                               # the tie on the positive and on the negative arm of the key
        s, above, at = tied_logits(value)
        for k in (above + 1, above + at):                       # the k-th place is the first and the last of the tied entries
            cases.append((f"e_tied_{value}_k{k}", s, 1.0, k) + midpoint_rows(s, 1.0, k))
    # f: temperature 1e-3 turns +-0.5 into +-500: expf(l - max) is exactly 0 for everything but the maximum
    us = np.array([0.0, 0.25, 0.5, U_BELOW_ONE, 1.0], np.float32)
    last_max = np.array([-0.5, 0, 0, 0, 0, 0, 0, 0.5], np.float32)      # kept index 0 (and 1..6) without mass
    cases.append(("f_underflow_max_last", last_max, 1e-3, None, us, np.full(5, 7, np.int64)))
    # all the mass at index 0 and a mass-less last index: u = 1 leaves no prefix sum above u * S, so the last kept index
    first_max = last_max[::-1].copy()
    cases.append(("f_underflow_max_first", first_max, 1e-3, None, us, np.array([0, 0, 0, 0, 7], np.int64)))
    return cases


DRAW_CASES = _build_draw_cases()
