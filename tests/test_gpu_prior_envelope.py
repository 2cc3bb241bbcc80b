"""The code prior's kernels (csrc/prior_sample.hip, csrc/prior.hip) over their whole admitted envelope on the MI355X, against
float64 restatements that run none of this project's kernels (tests/prior_cases.py):

  decode     teacher-forced logits against forward_fp64 at embed_dim 192 / 320 / 448 (the 64-wide multi-chunk ps_linear), head
             counts that leave attention workgroups partly filled, the row-tile edges B = 15 / 16 / 17, V = 1 .. 1024; the KV
             cache against teacher forcing, bit for bit;
  draw       exact cases through a model whose logits are known exactly: every thread and wave boundary of the scan, ties of
             every size, a k-th value of either sign, u = 0 / below 1 / 1, masses that underflow;
  attention  forward, saved probabilities and backward through the C entry points: odd B * H, T = 1, a large grid, dropped
             rows, scores that overflow expf without the max subtraction;
  AdamW      parameters and both moments against float64 over one to three trips of the grid-stride loop;
  refusals   every argument the entry points must refuse, with the outputs untouched.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import prior_cases as pc
from test_gpu_prior_sample import LOGIT_TOL

pytestmark = pytest.mark.gpu

E_ARG, E_WORKSPACE = -1, -2


def dev():
    return torch.device("cuda", 0)


def bits(t):
    return t.contiguous().view(torch.int32)


# ================================================================================================ decode
@functools.lru_cache(maxsize=None)
def decode_model(shape):
    return pc.seeded_model(pc.DECODE_SHAPES[shape], 31, dev())


# Bound on max |logits - fp64| / max |fp64| per shape: the project's LOGIT_TOL unless a shape is listed here.  Measured on the
# MI355X over all cases below: 4.8e-7 .. 1.8e-6 for the kernel, 1.3e-7 .. 1.9e-6 for torch's float32 forward (DESIGN.md
# section 8 has the table per shape), so no shape is listed.
DECODE_TOL = {}


@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("shape,labelled", [(s, lab) for s, c in pc.DECODE_SHAPES.items() for lab in (False, True)
                                             if not lab or c["num_classes"] > 0])
def test_teacher_forced_logits_equal_the_float64_forward(shape, labelled, B):
    """The prompt fills every position (max_seq_len + 1 tokens: logits of positions 0 .. max_seq_len - 1, one position for
    max_seq_len = 1).  Printed next to the kernel's ratio: torch's own float32 forward (no fused attention) against the same
    float64 values."""
    from vqvae_amd.prior.sampling import sample_native
    cfg = pc.DECODE_SHAPES[shape]
    model = decode_model(shape)
    g = torch.Generator(device=dev()).manual_seed(B)
    T = cfg["max_seq_len"]
    x = torch.randint(0, cfg["num_tokens"], (B, T + 1), device=dev(), generator=g)
    y = torch.randint(0, cfg["num_classes"], (B,), device=dev(), generator=g) if labelled else None
    tokens, logits = sample_native(model, x, 0, 1.0, None, y, None, return_logits=True)
    assert torch.equal(tokens, x)
    assert logits.shape == (B, T, cfg["num_tokens"])
    want = pc.forward_fp64(model, x[:, :T], y)
    model.fused_attention = False
    try:
        with torch.no_grad():
            stock = model(x[:, :T], y=y)
    finally:
        model.fused_attention = True
    scale = want.abs().max()
    err = float((logits.double() - want).abs().max() / scale)
    err_torch = float((stock.double() - want).abs().max() / scale)
    print(f"{shape} B={B} labelled={labelled}: kernel vs fp64 {err:.2e}, torch f32 vs fp64 {err_torch:.2e}")
    assert err < DECODE_TOL.get(shape, LOGIT_TOL)


@pytest.mark.parametrize("shape", ["c192_h3_v1024", "c320_h10_v100"])
def test_kv_cache_equals_teacher_forcing_bit_for_bit(shape):
    """Generated and teacher-forced positions run the same kernels in the same order; only where the next token comes from
    differs.  So the logits of a greedy generation equal those of its own output fed back as a prompt, bit for bit, however
    the sequence is split between prompt and steps."""
    from vqvae_amd.prior.sampling import sample_native
    cfg = pc.DECODE_SHAPES[shape]
    model = decode_model(shape)
    B, T = 17, cfg["max_seq_len"]
    g = torch.Generator(device=dev()).manual_seed(5)
    x = torch.randint(0, cfg["num_tokens"], (B, 1), device=dev(), generator=g)
    u = torch.rand((B, T), device=dev(), generator=g)
    tokens, logits = sample_native(model, x, T, 1.0, 1, None, u, return_logits=True)
    assert tokens.shape == (B, T + 1) and torch.equal(tokens[:, :1], x)
    assert torch.equal(tokens[:, 1:], logits.argmax(-1))                        # greedy
    assert len(set(tokens[:, 1:].flatten().tolist())) > 1
    again, forced = sample_native(model, tokens, 0, 1.0, None, None, None, return_logits=True)          # T0 = T + 1, steps 0
    assert torch.equal(again, tokens) and torch.equal(bits(forced), bits(logits))
    last, mixed = sample_native(model, tokens[:, :T].contiguous(), 1, 1.0, 1, None, u[:, -1:].contiguous(), return_logits=True)
    assert torch.equal(last, tokens) and torch.equal(bits(mixed), bits(logits))                        # T0 = T, steps 1


# ================================================================================================ draw
DRAW = {c[0]: c for c in pc.DRAW_CASES}


@functools.lru_cache(maxsize=None)
def _exact_model(key):
    return pc.exact_logit_model(np.frombuffer(key, dtype=np.float32).copy(), dev())


@pytest.mark.parametrize("name", list(DRAW))
def test_draws_decided_by_their_inputs_are_exact(name):
    """One row per u, one generated token.  test_prior_cases_host.py guarantees that every row is decidable (exact masses, or
    u * S at least 3e-4 * S inside its token's step), so every row must give `want`: no near-step allowance."""
    from vqvae_amd.prior.sampling import sample_native
    _, s, temperature, top_k, u, want = DRAW[name]
    model = _exact_model(s.tobytes())
    B, V = len(u), len(s)
    x = torch.zeros((B, 1), dtype=torch.int64, device=dev())
    tokens, logits = sample_native(model, x, 1, temperature, top_k, None, torch.from_numpy(u).to(dev())[:, None], return_logits=True)
    # the logits are s bit for bit (a sum that starts at +0.0 cannot end in -0.0: a -0.0 entry arrives as +0.0)
    assert torch.equal(bits(logits), bits(torch.from_numpy(s + 0.0).to(dev())).expand(B, 1, V))
    got = tokens[:, 1].cpu().numpy()
    wrong = np.nonzero(got != want)[0]
    assert len(wrong) == 0, f"{len(wrong)} of {B} rows; first: u={u[wrong[0]]!r} gave {got[wrong[0]]}, want {want[wrong[0]]}"


# ================================================================================================ training attention
def attention_fwd(qkv, keep, keep_scale, H):
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    B, T, C3 = qkv.shape
    C = C3 // 3
    out = torch.full((B, T, C), float("nan"), device=qkv.device)
    probs = torch.full((B, H, T, T), float("nan"), device=qkv.device)
    _lib.check(_lib.load().geo_prior_attention_fwd(ptr(qkv), ptr(keep), keep_scale, B, T, H, C // H, ptr(out), ptr(probs),
                                                   stream_ptr()), "geo_prior_attention_fwd")
    return out, probs


def attention_bwd(qkv, probs, keep, keep_scale, dout, H):
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    B, T, C3 = qkv.shape
    dqkv = torch.full_like(qkv, float("nan"))
    _lib.check(_lib.load().geo_prior_attention_bwd(ptr(qkv), ptr(probs), ptr(keep), keep_scale, ptr(dout), B, T, H, C3 // 3 // H,
                                                   ptr(dqkv), stream_ptr()), "geo_prior_attention_bwd")
    return dqkv


def attention64(qkv, keep, keep_scale, H, dout):
    """(out, probs, dqkv) in float64 with plain torch operations and autograd."""
    B, T, C3 = qkv.shape
    C = C3 // 3
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = x.view(B, T, 3, H, C // H).permute(2, 0, 3, 1, 4)
    w = (q @ k.transpose(-2, -1)) / np.sqrt(C // H)
    w = w.masked_fill(torch.triu(torch.ones(T, T, device=qkv.device), 1).bool(), float("-inf"))
    probs = torch.softmax(w, dim=-1)
    pd = probs * keep.double() * keep_scale if keep is not None else probs
    out = (pd @ v).transpose(1, 2).reshape(B, T, C)
    out.backward(dout.double())
    return out.detach(), probs.detach(), x.grad


def check_attention(qkv, keep, keep_scale, H, dout):
    B, T, _ = qkv.shape
    out, probs = attention_fwd(qkv, keep, keep_scale, H)
    dqkv = attention_bwd(qkv, probs, keep, keep_scale, dout, H)
    out64, probs64, dqkv64 = attention64(qkv, keep, keep_scale, H, dout)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(probs).all()) and bool(torch.isfinite(dqkv).all())
    np.testing.assert_allclose(out.cpu().numpy(), out64.cpu().numpy(), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(probs.cpu().numpy(), probs64.cpu().numpy(), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(dqkv.cpu().numpy(), dqkv64.cpu().numpy(), rtol=2e-4, atol=2e-5)
    above = torch.triu(torch.ones(T, T, device=qkv.device), 1).bool()
    assert bool((probs[..., above] == 0.0).all())
    assert float((probs.sum(-1) - 1.0).abs().max()) <= 16 * 2.0 ** -24


@pytest.mark.parametrize("C,H,T,B", [(192, 3, 16, 1), (192, 12, 1, 5), (320, 10, 9, 7), (64, 1, 16, 1), (64, 4, 3, 1025)])
def test_attention_kernels_equal_float64_over_the_envelope(C, H, T, B):
    """head_dim 64 with B * H = 3 (a half-filled backward workgroup of two waves), T = 1, head_dim 32 with H = 10, a single
    wave, a large grid of short sequences; without dropout, with a mask that drops a quarter and one whole row, and with a
    mask that drops nothing (keep_scale still applies)."""
    g = torch.Generator(device="cpu").manual_seed(1000 * C + 10 * T + H)
    qkv = torch.randn(B, T, 3 * C, generator=g).to(dev())
    dout = torch.randn(B, T, C, generator=g).to(dev())
    check_attention(qkv, None, 1.0, H, dout)
    keep = torch.rand(B, H, T, T, generator=g) >= 0.25
    keep[B - 1, 0, 0, :] = True                                                 # one row keeps everything,
    keep[0, H - 1, T - 1, :] = False                                            # one loses every probability
    check_attention(qkv, keep.to(dev()), 1.0 / 0.75, H, dout)
    check_attention(qkv, torch.ones(B, H, T, T, dtype=torch.bool, device=dev()), 1.0 / 0.75, H, dout)


@pytest.mark.parametrize("D", [64, 16])
def test_attention_survives_scores_beyond_the_range_of_expf(D):
    """q and k are multiples of 0.5 and scale = 1 / sqrt(D) is a power of two: every score is exact in float32.  One score per
    chosen row is exactly 128 > log(FLT_MAX) = 88.7 -- exp of it overflows unless the row maximum is subtracted first."""
    B, H, T = 3, 3, 16
    g = torch.Generator(device="cpu").manual_seed(D)
    qkv = torch.randn(B, T, 3, H, D, generator=g)
    qkv[:, :, :2] = torch.randint(-4, 5, (B, T, 2, H, D), generator=g) * 0.5
    big = 128.0 * np.sqrt(D) / (D * 4.0)                                        # q = big, k = 4: D * big * 4 / sqrt(D) = 128
    assert big in (4.0, 8.0)
    for b, h, i, j in ((0, 1, T - 1, 5), (2, 2, 7, 7), (1, 0, 0, 0)):
        qkv[b, i, 0, h] = big
        qkv[b, j, 1, h] = 4.0
    scores = torch.einsum("bihd,bjhd->bhij", qkv[:, :, 0], qkv[:, :, 1]) / np.sqrt(D)
    assert float(torch.tril(scores).max()) == 128.0
    qkv = qkv.view(B, T, 3 * H * D).to(dev())
    dout = torch.randn(B, T, H * D, generator=g).to(dev())
    check_attention(qkv, None, 1.0, H, dout)
    keep = (torch.rand(B, H, T, T, generator=g) >= 0.25).to(dev())
    check_attention(qkv, keep, 1.0 / 0.75, H, dout)


# ================================================================================================ AdamW
def adamw64(p, m, v, g, lr, t, beta1, beta2, eps, weight_decay):
    """torch.optim.AdamW's update of step t (1-based) in float64, nothing rounded."""
    p = p * (1.0 - lr * weight_decay)
    m = m + (1.0 - beta1) * (g - m)
    v = beta2 * v + (1.0 - beta2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps
    return p - (lr / (1.0 - beta1 ** t)) * (m / denom), m, v


ADAMW_CONFIGS = {"decay": dict(weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8),
                 "no_decay": dict(weight_decay=0.0, betas=(0.8, 0.95), eps=1e-6)}


@pytest.mark.parametrize("config", list(ADAMW_CONFIGS))
@pytest.mark.parametrize("n", [1, 255, 257, 524288, 524289, 1200003])
def test_arena_adamw_equals_float64_on_every_trip_of_the_grid_stride_loop(n, config):
    """The grid is capped at 2048 x 256 = 524 288 lanes: n = 524 289 and 1 200 003 take a second and a third trip.  Checked
    after step 1 (where bias correction is largest) and after step 12; the learning rate moves once, one gradient is all zero.

    Every element's gradient keeps its sign and its scale (10^-3 .. 10^1.5 across elements, times 0.25 .. 1 per step): no
    moment is the small remainder of large cancelling terms, so each float32 operation's 2^-24 is relative to the moment
    itself -- at most 3 roundings per step and moment, 36 * 2^-24 = 2.1e-6 after 12 steps in the worst case, within
    rtol 2e-6 + atol 1e-7 -- and the moments of the large-gradient elements are far above atol, where rtol alone decides."""
    from vqvae_amd.prior.native import ArenaAdamW
    cfg = ADAMW_CONFIGS[config]
    r = np.random.RandomState(n % 1000 + len(config))
    p0 = r.standard_normal(n).astype(np.float32)
    scale = 10.0 ** r.uniform(-3.0, 1.5, n) * np.where(r.rand(n) < 0.5, -1.0, 1.0)
    a = torch.nn.Parameter(torch.from_numpy(p0).to(dev()))
    b = torch.nn.Parameter(torch.from_numpy(p0).to(dev()))
    mine = ArenaAdamW(a, lr=3e-4, weight_decay=cfg["weight_decay"], betas=cfg["betas"], eps=cfg["eps"])
    ref = torch.optim.AdamW([b], lr=3e-4, weight_decay=cfg["weight_decay"], betas=cfg["betas"], eps=cfg["eps"])
    P, M, V = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t in range(1, 13):
        grad = np.zeros(n, np.float32) if t == 9 else (scale * r.uniform(0.25, 1.0, n)).astype(np.float32)
        a.grad, b.grad = torch.from_numpy(grad).to(dev()), torch.from_numpy(grad).to(dev())
        if t == 7:
            for opt in (mine, ref):
                opt.param_groups[0]["lr"] *= 0.5
        mine.step()
        ref.step()
        lr = float(np.float32(mine.param_groups[0]["lr"]))                      # the kernel reads lr as a float32 on the device
        P, M, V = adamw64(P, M, V, grad.astype(np.float64), lr, t, *cfg["betas"], cfg["eps"], cfg["weight_decay"])
        assert int(mine.step_dev) == t
        if t in (1, 12):
            for what, got, want in (("param", a, P), ("exp_avg", mine.exp_avg, M), ("exp_avg_sq", mine.exp_avg_sq, V)):
                np.testing.assert_allclose(got.detach().cpu().numpy(), want, rtol=2e-6, atol=1e-7, err_msg=f"{what} at step {t}")
            np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=2e-6, atol=1e-7)
    assert float(np.abs(P - p0).min()) > 1e-5                                   # every element moved: no lane was skipped


# ================================================================================================ refusals
def test_sample_refuses_what_it_does_not_cover_and_writes_nothing():
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    from vqvae_amd.prior.sampling import _desc
    lib = _lib.load()
    cfg = dict(num_classes=0, num_tokens=64, embed_dim=64, n_layers=1, n_head=4, max_seq_len=8)
    plain, labelled = pc.seeded_model(cfg, 3, dev()), pc.seeded_model(dict(cfg, num_classes=5), 3, dev())
    B, T0, steps = 6, 2, 3
    x = torch.randint(0, 64, (B, T0), device=dev())
    y = torch.zeros(B, dtype=torch.int64, device=dev())
    u = torch.rand((B, steps), device=dev())
    tokens = torch.full((B, T0 + steps), -7, dtype=torch.int64, device=dev())
    logits = torch.full((B, T0 + steps - 1, 64), -7.0, device=dev())
    desc, _keep = _desc(plain)
    nbytes = lib.geo_prior_sample_workspace_bytes(ctypes.byref(desc), B, T0 + steps - 1)
    assert nbytes > 0
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev())
    assert ws.data_ptr() % 256 == 0

    def call(model=plain, edit=None, xp=ptr(x), T0_=T0, steps_=steps, yp=None, up=ptr(u), temperature=1.0, top_k=0, B_=B,
             wp=ws.data_ptr(), wb=nbytes):
        d, _blocks = _desc(model)
        for field, value in (edit or {}).items():
            setattr(d, field, value)
        return lib.geo_prior_sample(ctypes.byref(d), xp, T0_, steps_, yp, up, temperature, top_k, ptr(tokens), ptr(logits), B_,
                                    wp, wb, stream_ptr())

    refused = [dict(edit=dict(n_head=8)),                                       # head_dim 8
               dict(edit=dict(embed_dim=576, n_head=9)), dict(edit=dict(embed_dim=96, n_head=3)),
               dict(edit=dict(num_tokens=1025)), dict(edit=dict(num_tokens=0)), dict(edit=dict(max_seq_len=17)),
               dict(T0_=0), dict(T0_=7, steps_=3), dict(T0_=10, steps_=0), dict(xp=None), dict(up=None),
               dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
               dict(top_k=65), dict(top_k=-1), dict(yp=ptr(y)), dict(B_=0), dict(wp=None), dict(wp=ws.data_ptr() + 64)]
    for bad in refused:
        assert call(**bad) == E_ARG, bad
        assert lib.geo_last_error()
    assert call(wb=nbytes - 1) == E_WORKSPACE
    assert b"workspace" in lib.geo_last_error()
    assert lib.geo_prior_sample_workspace_bytes(ctypes.byref(desc), 0, 4) == 0
    assert lib.geo_prior_sample_workspace_bytes(ctypes.byref(desc), B, 0) == 0
    torch.cuda.synchronize()
    assert bool((tokens == -7).all()) and bool((logits == -7.0).all())
    # legal calls straight afterwards: null uniforms without steps, labels for a model that has classes, the exact workspace
    assert call(up=None, T0_=2, steps_=0) == 0
    assert call(model=labelled, yp=ptr(y)) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(tokens[:, :T0], x) and bool(((tokens >= 0) & (tokens < 64)).all()) and bool(torch.isfinite(logits).all())


def test_attention_and_adamw_refuse_bad_arguments_and_write_nothing():
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    lib = _lib.load()
    B, T, H, D = 2, 4, 2, 16
    C = H * D
    qkv, dout = torch.randn(B, T, 3 * C, device=dev()), torch.randn(B, T, C, device=dev())
    out, probs = torch.full((B, T, C), -7.0, device=dev()), torch.full((B, H, T, T), -7.0, device=dev())
    dqkv = torch.full((B, T, 3 * C), -7.0, device=dev())

    def fwd(qp=ptr(qkv), op=ptr(out), pp=ptr(probs), B_=B, T_=T, D_=D):
        return lib.geo_prior_attention_fwd(qp, None, 1.0, B_, T_, H, D_, op, pp, stream_ptr())

    def bwd(qp=ptr(qkv), pp=ptr(probs), gp=ptr(dout), dp=ptr(dqkv), B_=B, T_=T, D_=D):
        return lib.geo_prior_attention_bwd(qp, pp, None, 1.0, gp, B_, T_, H, D_, dp, stream_ptr())

    for bad in (dict(T_=0), dict(T_=17), dict(D_=48), dict(B_=0), dict(qp=None), dict(pp=None)):
        assert fwd(**bad) == E_ARG, bad
        assert bwd(**bad) == E_ARG, bad
    assert fwd(op=None) == E_ARG and bwd(gp=None) == E_ARG and bwd(dp=None) == E_ARG

    n = 1000
    p, g, m, v = (torch.full((n,), -7.0, device=dev()) for _ in range(4))
    lr, step = torch.full((1,), 1e-3, device=dev()), torch.ones(1, dtype=torch.int64, device=dev())

    def adamw(pp=ptr(p), gp=ptr(g), mp=ptr(m), vp=ptr(v), n_=n, lp=ptr(lr), sp=ptr(step)):
        return lib.geo_prior_adamw(pp, gp, mp, vp, n_, lp, sp, 0.9, 0.999, 1e-8, 0.01, stream_ptr())

    for bad in (dict(n_=0), dict(n_=-1), dict(pp=None), dict(gp=None), dict(mp=None), dict(vp=None), dict(lp=None), dict(sp=None)):
        assert adamw(**bad) == E_ARG, bad
    torch.cuda.synchronize()
    for t in (out, probs, dqkv, p, g, m, v):
        assert bool((t == -7.0).all())
    m.zero_()
    v.zero_()
    assert fwd() == 0 and bwd() == 0 and adamw() == 0                            # legal calls straight afterwards
    torch.cuda.synchronize()
    assert float((probs.sum(-1) - 1.0).abs().max()) <= 16 * 2.0 ** -24 and bool(torch.isfinite(dqkv).all())
    assert bool((p != -7.0).all()) and bool((g == -7.0).all())
