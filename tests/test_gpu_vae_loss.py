"""The fused HIP ELBO (csrc/vae_loss.hip) against the torch formula of `VAE.loss` (native_loss = False) evaluated in float64 on
the same float32 inputs.

Tolerances.  Forward: relative 1e-10 -- both sides form every term in fp64, only the order of the sum differs (n terms of
one sign, or a KL sum dominated by its largest terms), n <= 4.2e6.  Neither side adds the terms one after the other: the kernel
sums at most 8 terms per lane, then folds lanes, waves and workgroup partials as a tree, and torch's reduction is tree-shaped
too.  The error of such a sum of same-sign terms grows with the depth of the tree times eps_64 (about 40 levels here: 1e-14),
not with n; even the worst case n eps_64 = 5e-10 of one long chain is not approached.  Gradients:
|got - ref| <= 1e-6 |ref| + 1e-9 -- the kernel rounds an fp64 value to float32 once (relative 6e-8); the bound is one order
over that, the absolute term covers float32 underflow next to saturated logits.

Free bits at equality: k = -0.5 (1 + logvar - mu^2 - exp(logvar)) of float32 inputs equals 0.25 exactly for no input this test
could build without depending on the last bit of an exp (logvar = 0 gives k = mu^2 / 2 and 0.5 has no float32 square root), so
the shapes carry elements with logvar = 0, mu = +-0.5 (k = 0.125 exactly on both sides) and every shape is also run with
free_bits = 0.125, where those elements sit exactly on the clamp; with free_bits = 0.25 they lie below it.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(B, P, d) for B in (1, 3, 257) for P in (784, 3072) for d in (2, 128)]
# B P % 4 = 1, 3, 2: the scalar loops by size.  8200 x 512: B P > 4 x 256 x 4096 and B d > 256 x 4096, so the grids are capped
# and both grid-stride loops (float4 reconstruction, KL) go round a second time.
SHAPES += [(1, 1, 1), (3, 785, 2), (5, 786, 3), (8200, 512, 128)]
RECON = {0: ("bce", True), 1: ("mse", True), 2: ("mse", False)}


def make_inputs(B, P, d, seed=0):
    r = np.random.RandomState(seed + B * 7 + P + d)
    logits = (3 * r.randn(B, P)).astype(np.float32)
    logits.flat[:4] = [80.0, -80.0, 0.0, -0.0]
    x = r.rand(B, P).astype(np.float32)
    x.flat[:4] = [0.25, 0.75, 1.0, 0.0]
    mu = r.randn(B, d).astype(np.float32)
    logvar = r.uniform(-3, 1.5, (B, d)).astype(np.float32)
    # (mu, logvar): on the 0.125 clamp (twice), logvar +-20, below and above 0.25; two slots only when B d == 2
    special = [(0.5, 0.0), (0.0, 20.0)] if B * d == 2 else [(0.5, 0.0), (-0.5, 0.0), (0.0, 20.0), (0.3, -20.0), (0.1, 0.0),
                                                            (2.0, 1.0)]
    for i, (m, lv) in enumerate(special[:B * d]):
        mu.flat[i], logvar.flat[i] = m, lv
    return [torch.from_numpy(a).cuda() for a in (logits, x, mu, logvar)]


@pytest.fixture(scope="module")
def models():
    from vqvae_amd.vae import VAE
    hip, ref = (VAE(latent_dim=2, enc_channels=(8, 16, 32), dec_channels=(32, 16, 8)) for _ in range(2))
    ref.native_loss = False
    assert hip.native_loss
    return hip, ref


def configure(model, recon_mode, free_bits):
    model.recon_loss, model.mse_use_sigmoid = RECON[recon_mode]
    model.free_bits_default = free_bits


def run(model, inputs, dtype, **kw):
    """(triple, grads) of one loss call; inputs float32 CUDA tensors, evaluated in `dtype`."""
    logits, x, mu, logvar = (t.to(dtype) for t in inputs)
    leaves = [t.clone().requires_grad_(True) for t in (logits, mu, logvar)]
    total, recon, kl = model.loss(x, leaves[0], leaves[1], leaves[2], **kw)
    total.backward()
    return torch.stack([total.detach(), recon.detach(), kl.detach()]).double(), [t.grad for t in leaves]


def assert_close(got, ref, what):
    triple, grads = got
    triple_ref, grads_ref = ref
    rel = ((triple - triple_ref).abs() / triple_ref.abs().clamp_min(1e-300)).max().item()
    assert rel <= 1e-10, (what, "forward", rel, triple.tolist(), triple_ref.tolist())
    for name, g, gr in zip(("d_logits", "d_mu", "d_logvar"), grads, grads_ref):
        assert g.dtype == torch.float32 and g.shape == gr.shape
        excess = ((g.double() - gr).abs() - (1e-6 * gr.abs() + 1e-9)).max().item()
        assert excess <= 0, (what, name, excess)


@pytest.mark.parametrize("B,P,d", SHAPES)
def test_kernel_matches_float64_formula(models, B, P, d):
    hip, ref = models
    inputs = make_inputs(B, P, d)
    for recon_mode in RECON:
        for free_bits in (None, 0.25, 0.125):
            configure(hip, recon_mode, free_bits)
            configure(ref, recon_mode, free_bits)
            off = dict(beta=1.0, capacity_max=0.0, capacity_anneal_steps=100, step=0)
            plain = run(ref, inputs, torch.float64, **off)
            assert_close(run(hip, inputs, torch.float32, **off), plain, (recon_mode, free_bits, "off"))
            kl = plain[0][2].item()
            for mode in ("abs", "clipped"):
                for step in (0, 100):                      # target 0 (kl above it) and 2 kl (kl below it)
                    kw = dict(beta=0.7, capacity_max=2.0 * kl, capacity_anneal_steps=100, step=step, capacity_mode=mode)
                    want = run(ref, inputs, torch.float64, **kw)
                    got = run(hip, inputs, torch.float32, **kw)
                    assert_close(got, want, (recon_mode, free_bits, mode, step))
                    if mode == "clipped" and step == 100:
                        assert got[0][0].item() == got[0][1].item() and not got[1][1].any() and not got[1][2].any()


def misaligned(t):
    """The values of t as a contiguous view that starts 4 bytes past a 16-byte boundary."""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    base[1:] = t.flatten()
    view = base[1:].view(t.shape)
    assert base.data_ptr() % 16 == 0 and view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


@pytest.mark.parametrize("which", ["x", "logits", "both"])
def test_misaligned_views_take_the_scalar_route_and_change_no_gradient_bit(models, which):
    """B P % 4 == 0, but a base pointer off the 16-byte boundary: the launch picks the scalar kernels.  The views go to elbo_hip
    as leaves (run() would clone them onto an aligned allocation).  Forward: the 1e-10 of this file against the float64 formula.
    Gradients are elementwise, so they equal those of the aligned (float4) call on the same values bit for bit."""
    from vqvae_amd.vae import CAPACITY_MODES, elbo_hip
    _, ref = models
    B, P, d = 3, 784, 2
    assert (B * P) % 4 == 0
    logits, x, mu, logvar = make_inputs(B, P, d)
    for recon_mode in RECON:
        configure(ref, recon_mode, 0.125)
        kw = dict(beta=0.7, capacity_max=5.0, capacity_anneal_steps=10, step=3, capacity_mode="abs")
        want = run(ref, (logits, x, mu, logvar), torch.float64, **kw)[0]
        results = []
        for off in (False, True):
            lg = misaligned(logits) if off and which in ("logits", "both") else logits.clone()
            xs = misaligned(x) if off and which in ("x", "both") else x.clone()
            assert (lg.data_ptr() % 16 != 0 or xs.data_ptr() % 16 != 0) == off
            leaves = [t.detach().requires_grad_() for t in (lg, mu, logvar)]
            assert leaves[0].data_ptr() == lg.data_ptr()
            out = elbo_hip(leaves[0], xs, leaves[1], leaves[2], recon_mode, 0.125, 0.7, ref._compute_capacity_target(5.0, 10, 3),
                           CAPACITY_MODES["abs"])
            out[0].backward()
            rel = ((out[:3].detach() - want).abs() / want.abs()).max().item()
            assert rel <= 1e-10, (recon_mode, which, off, rel)
            results.append([t.grad for t in leaves])
        for name, a, b in zip(("d_logits", "d_mu", "d_logvar"), *results):
            assert a.dtype == torch.float32 and a.any() and torch.equal(a, b), (recon_mode, which, name)


def test_free_bits_gradient_at_below_and_above_the_clamp(models):
    """torch.clamp(min=) passes the gradient where the value equals the bound: so does the kernel."""
    hip, ref = models
    inputs = make_inputs(3, 784, 128)
    for m in (hip, ref):
        configure(m, 0, 0.125)
    kw = dict(beta=1.0, capacity_max=0.0, capacity_anneal_steps=1, step=0)
    _, (_, d_mu, d_lv) = run(hip, inputs, torch.float32, **kw)
    _, (_, d_mu_ref, _) = run(ref, inputs, torch.float64, **kw)
    assert d_mu.flatten()[0].item() == pytest.approx(0.5 / 3) and d_mu.flatten()[1].item() == pytest.approx(-0.5 / 3)   # at
    assert d_mu_ref.flatten()[0].item() == pytest.approx(0.5 / 3)
    assert d_mu.flatten()[4].item() == 0.0 and d_lv.flatten()[4].item() == 0.0                    # k = 0.005: below
    assert d_mu.flatten()[5].item() == pytest.approx(2.0 / 3)                                      # above
    for m in (hip, ref):
        configure(m, 0, 0.25)
    _, (_, d_mu, _) = run(hip, inputs, torch.float32, **kw)
    assert d_mu.flatten()[0].item() == 0.0 and d_mu.flatten()[5].item() == pytest.approx(2.0 / 3)


def test_abs_capacity_has_zero_subgradient_at_the_target(models):
    hip, _ = models
    inputs = make_inputs(3, 784, 2)
    configure(hip, 1, None)
    kl = run(hip, inputs, torch.float32, beta=1.0, capacity_max=0.0, capacity_anneal_steps=1, step=0)[0][2].item()
    triple, (d_logits, d_mu, d_lv) = run(hip, inputs, torch.float32, beta=3.0, capacity_max=kl, capacity_anneal_steps=1, step=1,
                                         capacity_mode="abs")
    assert triple[2].item() == kl and triple[0].item() == triple[1].item()
    assert not d_mu.any() and not d_lv.any() and d_logits.any()


def test_outputs_are_bit_identical_across_runs_and_streams(models):
    hip, _ = models
    inputs = make_inputs(257, 3072, 128)
    configure(hip, 0, 0.25)
    kw = dict(beta=0.7, capacity_max=5.0, capacity_anneal_steps=10, step=3, capacity_mode="abs")
    first = run(hip, inputs, torch.float32, **kw)
    again = run(hip, inputs, torch.float32, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = run(hip, inputs, torch.float32, **kw)
    side.synchronize()
    for got in (again, other):
        assert torch.equal(got[0], first[0])
        for a, b in zip(got[1], first[1]):
            assert torch.equal(a, b)


def test_golden_triples_on_the_gpu(golden):
    from test_vanilla_vae_host import CONFIGS, apply_setting
    from vqvae_amd.vae import VAE
    g = golden("vanilla_vae")
    for name in sorted(CONFIGS):
        model = VAE(**CONFIGS[name])
        x, x_logits, mu, logvar = (torch.from_numpy(g[f"{name}/{k}"]).cuda() for k in ("x", "x_logits", "mu", "logvar"))
        for row, want in zip(g["settings"], g[f"{name}/triples_f64"]):
            kw = apply_setting(model, row)
            got = torch.stack(model.loss(x, x_logits, mu, logvar, **kw)).cpu().numpy()
            assert got.dtype == np.float64
            assert np.all(np.abs(got - want) <= 1e-10 * np.abs(want)), (name, row, got, want)


def test_rejects_what_the_kernel_cannot_take(models):
    from vqvae_amd.vae import elbo_hip
    logits, x, mu, logvar = make_inputs(3, 784, 2)
    with pytest.raises(ValueError):
        elbo_hip(logits.double(), x, mu, logvar, 0, None, 1.0, 0.0, 0)
    with pytest.raises(ValueError):
        elbo_hip(logits, x, mu, logvar[:2], 0, None, 1.0, 0.0, 0)
