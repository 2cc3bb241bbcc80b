"""The KV-cached HIP decode of the code prior (csrc/prior_sample.hip) on the MI355X: teacher-forced logits against
Transformer.forward and against a float64 restatement of it, greedy sequences against the reference (tests/golden/prior_sample.npz), the draw rule on explicit
uniforms, the distribution of draws, reproducibility across seeds and concurrent streams, the fallback for non-standard
masks, and the generate_samples CLI end to end."""
import threading

import numpy as np
import pytest
import torch

from prior_cases import forward_fp64
from test_prior_sample_host import check_cli_outputs, fixture_inputs, fixture_model, tiny_setup

pytestmark = pytest.mark.gpu

# f32 end to end; the decode sums in another order than the GEMMs under Transformer.forward.  Measured on the MI355X: max
# |diff| / max |logit| 4.9e-7 .. 1.41e-6 over the shapes and batch sizes below (the test prints it); the bound leaves ~14x.
# Against the float64 restatement (prior_cases.forward_fp64, no kernel of this project): 3.9e-7 .. 1.32e-6.
LOGIT_TOL = 2e-5
SHAPES = {
    "prior_hd16": dict(num_classes=10, num_tokens=64, embed_dim=64, n_layers=2, n_head=4, max_seq_len=16),
    "hd32": dict(num_classes=0, num_tokens=100, embed_dim=128, n_layers=2, n_head=4, max_seq_len=16),
    "fm_hd64": dict(num_classes=10, num_tokens=512, embed_dim=256, n_layers=4, n_head=4, max_seq_len=16),
    "vanilla_hd64": dict(num_classes=10, num_tokens=513, embed_dim=512, n_layers=8, n_head=8, max_seq_len=2),
}


def dev():
    return torch.device("cuda", 0)


def random_model(cfg, seed):
    from oracle import synthetic as syn
    from vqvae_amd.prior import Transformer
    model = Transformer(**cfg, dropout=0.1)
    sd = syn.seeded_state_dict(model.state_dict(), seed)
    T = cfg["max_seq_len"]
    for k in sd:
        if k.endswith(".attn.bias"):
            sd[k] = torch.tril(torch.ones(T, T)).view(1, 1, T, T)
    model.load_state_dict(sd)
    return model.to(dev()).eval()


@pytest.mark.parametrize("shape,labelled", [(s, lab) for s in SHAPES for lab in (True, False)
                                             if lab is False or SHAPES[s]["num_classes"] > 0])
@pytest.mark.parametrize("B", [1, 37, 100, 4096])
def test_teacher_forced_logits_equal_forward(shape, B, labelled):
    """(the hd32 shape is an unconditional model: no class embedding in its arena)"""
    from vqvae_amd.prior.sampling import sample_native
    cfg = SHAPES[shape]
    model = random_model(cfg, 31)
    g = torch.Generator(device=dev()).manual_seed(B)
    T = cfg["max_seq_len"]
    x = torch.randint(0, cfg["num_tokens"], (B, T), device=dev(), generator=g)
    y = torch.randint(0, cfg["num_classes"], (B,), device=dev(), generator=g) if labelled else None
    tokens, logits = sample_native(model, x, 0, 1.0, None, y, None, return_logits=True)
    assert torch.equal(tokens, x)
    with torch.no_grad():
        want = model(x[:, :T - 1], y=y)
    err = float((logits - want).abs().max() / want.abs().max())
    # ... and against the float64 restatement, which runs no kernel of this project (the forward above runs csrc/prior.hip's
    # attention, so an error the two attention kernels shared would cancel in `err`); all rows, float64 on the GPU
    want64 = forward_fp64(model, x[:, :T - 1], y)
    err64 = float((logits.double() - want64).abs().max() / want64.abs().max())
    print(f"{shape} B={B} labelled={labelled}: max |diff| / max |logit| = {err:.2e} (forward), {err64:.2e} (float64)")
    assert err < LOGIT_TOL
    assert err64 < LOGIT_TOL


@pytest.mark.parametrize("name", ["prior", "prior_nolabel", "fm", "vanilla", "vanilla_nolabel", "limit", "nonstd"])
def test_greedy_sequences_equal_reference(golden, name):
    from vqvae_amd.prior import sample
    from vqvae_amd.prior.sampling import kernel_covers
    g = golden("prior_sample")
    model = fixture_model(g, name, dev())
    x, y, want = fixture_inputs(g, name, dev())
    assert kernel_covers(model) == (name != "nonstd")            # nonstd: the torch loop on the GPU
    got = sample(model, x, want.shape[1] - x.shape[1], top_k=1, y=y)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def near_step(logits, u, tok, temperature, top_k, rel=1e-5):
    """Is u * S within `rel` * S of the CDF step at which `tok` starts or ends (float64 restatement)?"""
    from vqvae_amd.prior.sampling import kept_mask
    l = logits.double() / temperature
    keep = kept_mask(logits.float() / temperature, top_k)
    p = torch.where(keep, torch.exp(l - l.max()), torch.zeros_like(l))
    c = torch.cumsum(p, 0)
    S = c[-1]
    lo = c[tok - 1] if tok > 0 else torch.zeros_like(S)
    t = u * S
    return bool(min(abs(t - lo), abs(t - c[tok])) < rel * S)


@pytest.mark.parametrize("temperature", [0.7, 1.0, 1.5])
@pytest.mark.parametrize("top_k", [None, 1, 20, 50, 512])
def test_explicit_uniforms_follow_the_draw_rule(temperature, top_k):
    from vqvae_amd.prior.sampling import draw_rule, kept_mask, sample_native
    cfg = SHAPES["fm_hd64"]
    model = random_model(cfg, 41)
    B, T0, steps = 300, 2, 14
    g = torch.Generator(device=dev()).manual_seed(7)
    x = torch.randint(0, 512, (B, T0), device=dev(), generator=g)
    y = torch.randint(0, 10, (B,), device=dev(), generator=g)
    u = torch.rand((B, steps), device=dev(), generator=g)
    tokens, logits = sample_native(model, x, steps, temperature, top_k, y, u, return_logits=True)
    drawn = logits[:, T0 - 1:]                                  # the logits each drawn token came from
    with torch.no_grad():
        fwd = model(tokens[:, :-1], y=y)[:, T0 - 1:]
    assert float((drawn - fwd).abs().max() / fwd.abs().max()) < LOGIT_TOL
    fwd64 = forward_fp64(model, tokens[:, :-1], y)[:, T0 - 1:]           # no kernel of this project on the reference side
    assert float((drawn.double() - fwd64).abs().max() / fwd64.abs().max()) < LOGIT_TOL
    near = 0
    for s in range(steps):
        want = draw_rule(drawn[:, s], u[:, s], temperature, top_k)
        got = tokens[:, T0 + s]
        kept = kept_mask(drawn[:, s] / temperature, top_k)
        assert bool(kept.gather(1, got[:, None]).all()), "a dropped token was drawn"
        for b in torch.nonzero(got != want).flatten().tolist():
            assert near_step(drawn[b, s].cpu(), u[b, s].double().cpu(), int(got[b]), temperature, top_k), (s, b)
            near += 1
        # against the torch forward's logits: only draws within reach of a CDF step may differ
        host = draw_rule(fwd[:, s], u[:, s], temperature, top_k)
        assert int((host != got).sum()) <= max(2, B // 100)
    print(f"T={temperature} top_k={top_k}: {near} draw(s) within rounding reach of a CDF step")


def test_tied_rows_at_the_kth_place_are_both_drawn():
    from vqvae_amd.prior.sampling import sample_native
    cfg = SHAPES["prior_hd16"]
    model = random_model(cfg, 43)
    s = torch.tensor([2.0, 1.8, 0.5, 1.5, 0.2, -1.0, 0.9, 1.5] + [0.0] * 56)       # logits: rows 3 and 7 tie at 3rd place
    with torch.no_grad():
        v = model.views()
        v["ln_f.weight"].zero_()
        v["ln_f.bias"].fill_(1.0)                              # LN_f output = ones: logit i = sum of head row i
        v["head.weight"].copy_((s / cfg["embed_dim"])[:, None].expand(64, cfg["embed_dim"]).to(dev()))
    B = 4096
    x = torch.zeros((B, 1), dtype=torch.int64, device=dev())
    u = torch.rand((B, 1), device=dev(), generator=torch.Generator(device=dev()).manual_seed(1))
    tokens = sample_native(model, x, 1, 1.0, 3, None, u)
    assert set(tokens[:, 1].tolist()) == {0, 1, 3, 7}


def test_distribution_of_draws_matches_softmax():
    from vqvae_amd.prior import sample
    cfg = SHAPES["prior_hd16"]
    model = random_model(cfg, 47)
    N = 65536
    x = torch.full((N, 1), 5, dtype=torch.int64, device=dev())
    y = torch.full((N,), 3, dtype=torch.int64, device=dev())
    torch.manual_seed(0)
    tokens = sample(model, x, 1, temperature=1.3, y=y)[:, 1]
    with torch.no_grad():
        p = torch.softmax(model(x[:1], y=y[:1])[0, -1].double() / 1.3, 0).cpu().numpy()
    counts = np.bincount(tokens.cpu().numpy(), minlength=64)
    sigma = np.sqrt(N * p * (1 - p))
    assert np.all(np.abs(counts - N * p) <= 5 * sigma + 1), np.max(np.abs(counts - N * p) / (sigma + 1e-12))


def test_seeded_and_concurrent_streams_reproduce():
    from vqvae_amd.prior import sample
    from vqvae_amd.prior.sampling import sample_native
    cfg = SHAPES["fm_hd64"]
    model = random_model(cfg, 53)
    x = torch.randint(0, 512, (100, 1), device=dev(), generator=torch.Generator(device=dev()).manual_seed(2))
    y = torch.arange(100, device=dev()) % 10
    torch.manual_seed(9)
    a = sample(model, x, 15, top_k=50, y=y)
    torch.manual_seed(9)
    b = sample(model, x, 15, top_k=50, y=y)
    assert torch.equal(a, b)
    us = [torch.rand((100, 15), device=dev()) for _ in range(2)]
    seq = [sample_native(model, x, 15, 1.0, 50, y, u) for u in us]
    out = [None, None]
    errors = []

    def run(i):
        try:
            s = torch.cuda.Stream(device=dev())
            s.wait_stream(torch.cuda.current_stream(dev()))
            with torch.cuda.stream(s):
                for _ in range(3):
                    out[i] = sample_native(model, x, 15, 1.0, 50, y, us[i])
            s.synchronize()
        except Exception as e:                                # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        assert torch.equal(out[i], seq[i])


@pytest.mark.parametrize("vanilla", [False, True])
def test_cli_on_the_gpu(tmp_path, vanilla):
    from vqvae_amd.scripts import generate_samples as gs
    path, cfg = tiny_setup(str(tmp_path), vanilla, classes=(0, 1, 2, 3), spc=10)
    gs.main(path)
    check_cli_outputs(cfg, dev())
