"""Spatial VAE training on the MI355X: the batch kernel (csrc/batch.hip) against the torch expression it replaces, bit for bit;
ResidentLoader with and without it; `SpatialVAE.loss` (the fused HIP ELBO on latent grids) against the reference's values
(tests/golden/spatial_vae.npz) and a float64 restatement; a two-epoch run of the SpatialTrainingEngine.

Loss tolerances are those of test_gpu_vae_loss.py for the same kernel: forward relative 1e-10 (both sides form every term in
fp64; only the order of the sums differs), gradients |got - ref| <= 1e-6 |ref| + 1e-9 (one rounding of an fp64 value to
float32, relative 6e-8, and float32 underflow next to saturated logits)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_spatial_vae_host import CASES, TINY, _Recorder, case_model, loss_and_grads, tiny_model

pytestmark = pytest.mark.gpu

MEAN = (0.4914, 0.4822, 0.4465, 0.37)
STD = (0.2470, 0.2430, 0.2610, 0.3)


def images_on_gpu(N, size, C, seed):
    from vqvae_amd.baseline.data import DeviceImages
    r = np.random.RandomState(seed)
    u8 = r.randint(0, 256, (N, size, size, C)).astype(np.uint8)
    u8[0, 0, :8, 0] = [0, 1, 2, 3, 127, 128, 254, 255]
    return DeviceImages(u8, r.randint(0, 10, N), "cuda", MEAN[:C], STD[:C], img_size=size)


def torch_batch(im, rows, off=None, flip=None, pad=0):
    """DeviceImages.batch / ResidentLoader._augmented restated for any pad, torch ops on the images' device."""
    dev = im.device
    u8 = im.u8[torch.as_tensor(rows, dtype=torch.int64).to(dev)]
    if off is not None:
        u8 = F.pad(u8, (0, 0, pad, pad, pad, pad))
        B, H, W = u8.size(0), im.u8.size(1), im.u8.size(2)
        ys = off[:, :1] + torch.arange(H)
        xs = off[:, 1:] + torch.arange(W)
        xs = torch.where(flip[:, None], xs.flip(1), xs)
        ys, xs = ys.to(dev), xs.to(dev)
        u8 = u8[torch.arange(B, device=dev)[:, None, None], ys[:, :, None], xs[:, None, :]]
    x = u8.permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    return x.sub_(im.mean).div_(im.std)


def test_batch_kernel_equals_the_torch_path_bit_for_bit():
    from vqvae_amd.training.data import assemble_batch
    # every byte value through every channel's mean and std: each of the three roundings, exhaustively
    ramp = images_on_gpu(1, 16, 4, 0)
    ramp.u8.copy_(torch.arange(256, dtype=torch.uint8).repeat_interleave(4).view(1, 16, 16, 4))
    assert torch.equal(assemble_batch(ramp, torch.tensor([0])), torch_batch(ramp, [0]))

    rgb = images_on_gpu(7, 32, 3, 1)
    rows = torch.tensor([6, 0, 3, 3, 1])
    off = torch.tensor([[0, 0], [8, 8], [0, 8], [4, 4], [5, 2]])
    flip = torch.tensor([True, False, True, False, True])
    got = assemble_batch(rgb, rows, off, flip, 4)
    want = torch_batch(rgb, rows, off, flip, 4)
    assert got.shape == (5, 3, 32, 32) and got.is_contiguous() and torch.equal(got, want)
    assert torch.equal(got[3], rgb.batch([3])[0])                                  # offset (pad, pad), no flip: the image itself
    assert torch.equal(assemble_batch(rgb, rows, off, ~flip, 4), torch_batch(rgb, rows, off, ~flip, 4))
    assert torch.equal(assemble_batch(rgb, rows), rgb.batch(rows))

    grey = images_on_gpu(5, 28, 1, 2)
    assert torch.equal(assemble_batch(grey, torch.arange(5)), grey.batch(slice(0, 5)))

    two = images_on_gpu(4, 30, 2, 3)                                               # W % 4 != 0: scalar stores, partial last group
    rows = torch.tensor([3, 1, 0, 2])
    off = torch.tensor([[0, 6], [6, 0], [3, 3], [1, 5]])
    flip = torch.tensor([False, True, True, False])
    assert torch.equal(assemble_batch(two, rows), two.batch(rows))
    assert torch.equal(assemble_batch(two, rows, off, flip, 3), torch_batch(two, rows, off, flip, 3))

    with pytest.raises(IndexError):
        assemble_batch(grey, torch.tensor([0, 5]))
    with pytest.raises(IndexError):
        assemble_batch(grey, torch.tensor([-1]))


def test_batch_kernel_limits_are_errors_before_any_launch():
    from vqvae_amd import _lib
    L = _lib.load()
    u8 = torch.zeros(2 * 8 * 8 * 5, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(2, dtype=torch.int64, device="cuda")
    stat = torch.ones(5, device="cuda")
    out = torch.full((2 * 5 * 8 * 8,), -7.0, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(C=3, H=8, W=8, pad=0):
        return L.geo_batch_assemble(u8.data_ptr(), 2, H, W, C, rows.data_ptr(), 2, None, None, pad, stat.data_ptr(), stat.data_ptr(),
                                    out.data_ptr(), stream)

    for kw in (dict(C=5), dict(pad=17), dict(C=0), dict(H=257), dict(W=0), dict(pad=-1)):
        assert call(**kw) == -1, kw                                               # GEO_E_ARG
        assert b"limits" in L.geo_last_error()
    with pytest.raises(_lib.GeoHipError, match="geo_batch_assemble"):
        _lib.check(call(C=5), "geo_batch_assemble")
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call() == 0 and call(pad=16, C=4) == 0
    torch.cuda.synchronize()
    assert bool((out[:2 * 4 * 8 * 8] == -1.0).all()) and bool((out[2 * 4 * 8 * 8:] == -7.0).all())    # black, mean 1, std 1


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("crop_flip", [False, True])
def test_loader_with_the_kernel_equals_the_loader_without(shuffle, crop_flip):
    from vqvae_amd.training.data import ResidentLoader
    data = images_on_gpu(11, 32, 3, 4)
    norm = (MEAN[:3], STD[:3])
    epochs = {}
    for fused in (True, False):
        torch.manual_seed(9)
        loader = ResidentLoader(data, 4, shuffle, norm, crop_flip=crop_flip, fused=fused)
        assert loader.fused is fused
        epochs[fused] = [list(loader), list(loader)]                              # two epochs: the generators move on alike
    assert ResidentLoader(data, 4, shuffle, norm).fused is True                   # None: the kernel on a CUDA device
    for a, b in zip(epochs[True], epochs[False]):
        assert [x.shape[0] for x, _ in a] == [4, 4, 3]
        for (xa, ya), (xb, yb) in zip(a, b):
            assert xa.is_cuda and xa.is_contiguous() and torch.equal(xa, xb) and torch.equal(ya, yb)
    first, second = epochs[True]
    if shuffle or crop_flip:
        assert not all(torch.equal(x1, x2) for (x1, _), (x2, _) in zip(first, second))


def formula64(x, logits, mu, logvar, beta, mode):
    """The reference's spatial ELBO restated in float64 torch ops."""
    B = x.size(0)
    if mode == 0:
        recon = F.binary_cross_entropy_with_logits(logits, x, reduction="sum") / B
    else:
        recon = F.mse_loss(torch.sigmoid(logits) if mode == 1 else logits, x, reduction="sum") / B
    kl = (-0.5 * (1 + logvar - mu.pow(2) - logvar.exp())).sum(dim=[1, 2, 3]).mean()
    return recon + beta * kl, recon, kl


@pytest.mark.parametrize("name", CASES)
def test_gpu_loss_against_the_golden_values_and_a_float64_restatement(golden, name):
    g = golden("spatial_vae")
    model = case_model(g, name)
    mode = int(g[f"{name}/recon_mode"])
    for i, beta in enumerate(g["betas"]):
        triple, grads = loss_and_grads(model, g, name, float(beta), device="cuda", step=i)
        got = torch.stack(triple).cpu().numpy()
        assert got.dtype == np.float64
        want = g[f"{name}/triples_f64"][i]
        print(name, beta, "golden rel", (np.abs(got - want) / np.abs(want)).max())
        assert np.all(np.abs(got - want) <= 1e-10 * np.abs(want)), (name, beta, got, want)

        x, logits, mu, logvar = (torch.from_numpy(g[f"{name}/{k}"]).cuda().double() for k in ("x", "x_logits", "mu", "logvar"))
        leaves = [t.requires_grad_(True) for t in (logits, mu, logvar)]
        ref = formula64(x, *leaves, float(beta), mode)
        ref[0].backward()
        ref_triple = torch.stack([t.detach() for t in ref])
        rel = ((torch.stack(triple) - ref_triple).abs() / ref_triple.abs().clamp_min(1e-300)).max().item()
        assert rel <= 1e-10, (name, beta, rel)
        for what, got_g, leaf in zip(("d_x_logits", "d_mu", "d_logvar"), grads, leaves):
            assert got_g.dtype == torch.float32 and got_g.shape == leaf.grad.shape
            excess = ((got_g.double() - leaf.grad).abs() - (1e-6 * leaf.grad.abs() + 1e-9)).max().item()
            print(name, beta, what, "excess", excess)
            assert excess <= 0, (name, beta, what, excess)


def test_gpu_loss_takes_grids_that_are_not_contiguous(golden):
    g = golden("spatial_vae")
    model = case_model(g, "mse_log_32")
    x, logits, mu, logvar = (torch.from_numpy(g[f"mse_log_32/{k}"]).cuda() for k in ("x", "x_logits", "mu", "logvar"))
    want = torch.stack(model.loss(x, logits, mu, logvar, beta=0.25))
    last = [t.contiguous(memory_format=torch.channels_last) for t in (x, logits, mu, logvar)]
    assert not last[2].is_contiguous()
    assert torch.equal(torch.stack(model.loss(*last, beta=0.25)), want)


def test_gpu_loss_is_bit_identical_across_streams(golden):
    g = golden("spatial_vae")
    model = case_model(g, "mse_sig_32")
    first = loss_and_grads(model, g, "mse_sig_32", 0.25, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = loss_and_grads(model, g, "mse_sig_32", 0.25, device="cuda")
    side.synchronize()
    assert torch.equal(torch.stack(other[0]), torch.stack(first[0]))
    for a, b in zip(other[1], first[1]):
        assert torch.equal(a, b)


def test_two_epoch_spatial_training_run(tmp_path):
    from vqvae_amd.spatial_decoder import load_decoder_from_checkpoint
    from vqvae_amd.training.data import ResidentLoader, resident_images
    from vqvae_amd.training.spatial_engine import SpatialTrainingEngine
    from vqvae_amd.utils.spatial_latents import flatten_latents_device
    r = np.random.RandomState(0)
    data = resident_images(r.randint(0, 256, (64, 28, 28)).astype(np.uint8), r.randint(0, 10, 64), "cuda")
    torch.manual_seed(0)
    dev = torch.device("cuda")
    model = tiny_model().to(dev)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-2)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=2)
    log = _Recorder()
    train, val = ResidentLoader(data, 16, True), ResidentLoader(data, 16, False)
    assert train.fused
    SpatialTrainingEngine(model, opt, dev).train(train, val, num_epochs=2, early_stop=0, checkpoint_dir=tmp_path / "checkpoints",
                                                 logger=log, output_dir=tmp_path, save_latents_flag=True, beta=1.0,
                                                 grad_clip_max_norm=1.0, scheduler=sched)
    assert len(log.rows) == 2
    for _, row in log.rows:
        assert all(np.isfinite(v) for v in row.values()), row
    print("train loss", [row["train_loss"] for _, row in log.rows])
    assert log.rows[1][1]["train_loss"] < log.rows[0][1]["train_loss"]
    best = torch.load(tmp_path / "checkpoints" / "best.pt", weights_only=False)
    assert set(best) == {"model_state_dict", "epoch"}
    tiny_model().load_state_dict(best["model_state_dict"], strict=True)
    dec = load_decoder_from_checkpoint(str(tmp_path / "checkpoints" / "best.pt"), in_channels=1, dec_channels=TINY["dec_channels"],
                                       latent_dim=2, output_image_size=28, norm_type="batch", device=dev)
    assert dec(torch.zeros(2, 2, 4, 4, device=dev)).shape == (2, 1, 28, 28)
    z = torch.load(tmp_path / "latents_train" / "z.pt")
    assert z.shape == (64, 2, 4, 4) and not z.is_cuda and torch.isfinite(z).all()
    flat = flatten_latents_device(z.to(dev))
    assert flat.shape == (64 * 16, 2) and flat.is_contiguous()
    assert (tmp_path / "recon_grid.png").exists() and (tmp_path / "latents_val" / "mu.pt").exists()
