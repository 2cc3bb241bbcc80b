"""The inputs of the code prior's envelope tests (tests/prior_cases.py), checked without a GPU: the float64 forward equals the
module, the exact-logit models return their logits bit for bit, and every draw case is decided by its inputs -- the draw
rule gives the expected token for every row in float32 and in float64, and no row sits within rounding reach of a CDF step."""
import numpy as np
import pytest
import torch

import prior_cases as pc

LOGIT_TOL = 2e-5          # the decode tests' bound (test_gpu_prior_sample.py): max |diff| / max |logit|
CASES = {c[0]: c for c in pc.DRAW_CASES}


def bits(t):
    return torch.as_tensor(t, dtype=torch.float32).contiguous().view(torch.int32)


@pytest.mark.parametrize("shape,labelled,B", [("c192_h12_v1023", True, 5), ("c320_h10_v100", False, 3)])
def test_forward_fp64_equals_the_module(shape, labelled, B):
    cfg = pc.DECODE_SHAPES[shape]
    model = pc.seeded_model(cfg, 31)
    g = torch.Generator().manual_seed(B)
    x = torch.randint(0, cfg["num_tokens"], (B, cfg["max_seq_len"]), generator=g)
    y = torch.randint(0, cfg["num_classes"], (B,), generator=g) if labelled else None
    with torch.no_grad():
        got = model(x, y=y)
    want = pc.forward_fp64(model, x, y)
    assert want.dtype == torch.float64 and want.shape == got.shape
    err = float((got.double() - want).abs().max() / want.abs().max())
    print(f"{shape} labelled={labelled}: module f32 vs forward_fp64 {err:.2e}")
    assert err < LOGIT_TOL
    if labelled:                                               # the labels matter: another class moves the logits
        other = pc.forward_fp64(model, x, (y + 1) % cfg["num_classes"])
        assert float((other - want).abs().max() / want.abs().max()) > 100 * LOGIT_TOL


def test_case_names_are_unique_and_shapes_are_in_the_envelope():
    from vqvae_amd.prior import Transformer
    from vqvae_amd.prior.sampling import kernel_covers
    assert len(CASES) == len(pc.DRAW_CASES)
    for name, s, temperature, top_k, u, want in pc.DRAW_CASES:
        assert s.dtype == np.float32 and u.dtype == np.float32 and want.dtype == np.int64 and u.shape == want.shape, name
        assert 1 <= len(s) <= 1024 and len(u) >= 1 and (top_k is None or 1 <= top_k <= len(s)), name
        assert np.all(np.abs(s) < 1) and np.all(s * 2048 == np.round(s * 2048)), name       # multiples of 2^-11
    for cfg in pc.DECODE_SHAPES.values():
        assert kernel_covers(Transformer(**cfg))


@pytest.mark.parametrize("name", list(CASES))
def test_exact_logit_model_returns_its_logits_bit_for_bit(name):
    s = torch.from_numpy(CASES[name][1])
    model = pc.exact_logit_model(s)
    with torch.no_grad():
        logits = model(torch.tensor([[0, len(s) - 1], [len(s) // 2, 0]]))
    # a sum that starts at +0.0 cannot end in -0.0, in any order: the one -0.0 entry is +0.0 as a logit
    assert torch.equal(bits(logits), bits(s + 0.0).expand(2, 2, len(s)))


def rule64(s, u, temperature, top_k):
    """The draw rule in float64 on the float32 quotient l = s / temperature."""
    kept, c = pc.cdf64(s, temperature, top_k)
    t = u.astype(np.float64) * c[-1]
    over = c[None, :] > t[:, None]
    last_kept = len(s) - 1 - int(np.argmax(kept[::-1]))
    return np.where(over.any(1), over.argmax(1), last_kept)


@pytest.mark.parametrize("name", list(CASES))
def test_draw_rule_gives_the_expected_token_for_every_row(name):
    from vqvae_amd.prior.sampling import draw_rule
    _, s, temperature, top_k, u, want = CASES[name]
    logits = torch.from_numpy(s)[None].expand(len(u), len(s))
    got = draw_rule(logits, torch.from_numpy(u), temperature, top_k)
    np.testing.assert_array_equal(got.numpy(), want)
    np.testing.assert_array_equal(rule64(s, u, temperature, top_k), want)


@pytest.mark.parametrize("name", list(CASES))
def test_no_row_is_within_rounding_reach_of_a_step(name):
    """Either every kept mass is exactly 0 or 1 in float32 (all prefix sums are integers and the row is decided exactly; the
    float32 draw rule above has confirmed it), or u * S is at least MIN_HALF_STEP * S away from both ends of its token's step."""
    _, s, temperature, top_k, u, want = CASES[name]
    kept, c = pc.cdf64(s, temperature, top_k)
    l = pc.tempered(s, temperature)
    p32 = torch.exp(l - l.max()).numpy()[kept]
    if name[0] in "abcf":
        assert np.all((p32 == 0.0) | (p32 == 1.0))
        return
    assert np.all(kept[want])
    lo = np.concatenate(([0.0], c[:-1]))
    t = u.astype(np.float64) * c[-1]
    margin = np.minimum(t - lo[want], c[want] - t) / c[-1]
    print(f"{name}: {len(u)} rows, smallest half step {margin.min():.2e} of the total")
    assert margin.min() >= pc.MIN_HALF_STEP


def test_spread_and_tied_logits_have_the_structure_the_cases_rely_on():
    from vqvae_amd.prior.sampling import kept_mask
    s = pc.spread_logits()
    assert (s > 0).sum() == 510 and (s == 0).sum() == 3 and (s < 0).sum() == 511 and len(np.unique(s)) == 1022
    assert not np.signbit(s[17]) and np.signbit(s[900]) and s[900] == 0
    for temperature in pc.TEMPERATURES_D:
        l = pc.tempered(s, temperature)[None]
        sizes = {k: int(kept_mask(l, k).sum()) for k in pc.TOP_KS_D}
        assert sizes == {None: 1024, 1: 1, 2: 2, 3: 3, 255: 255, 256: 256, 257: 257, 511: 513, 512: 513, 513: 513, 1023: 1023}
        kth = {k: float(torch.topk(l[0], k).values[-1]) for k in pc.TOP_KS_D if k}
        assert kth[255] > 0 and kth[512] == 0 and kth[1023] < 0      # the k-th value on both arms of the key and at zero
    for name, case in CASES.items():
        if name[0] == "d":                                          # one row per kept index, each index once
            assert sorted(case[5].tolist()) == np.nonzero(pc.cdf64(case[1], case[2], case[3])[0])[0].tolist()
    for value in (0.125, -0.125):
        t, above, at = pc.tied_logits(value)
        assert at >= 3 and t[5] == t[300] == t[1023] == value
        for k in (above + 1, above + at):
            want = CASES[f"e_tied_{value}_k{k}"][5]
            assert len(want) == above + at and {5, 300, 1023} <= set(want.tolist())
