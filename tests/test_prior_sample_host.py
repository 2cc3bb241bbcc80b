"""Sampling from the code prior on the host: vqvae_amd.prior.sample against the reference's own `sample` / `top_k_logits`
(tests/golden/prior_sample.npz, tools/gen_golden_prior_sample.py), the draw rule the HIP decode shares, the limits, and the
generate_samples CLI end to end from tiny checkpoints (PNG grid against a numpy restatement of torchvision's save_image)."""
import os

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

FIXTURE_CASES = ("prior", "prior_nolabel", "fm", "vanilla", "vanilla_nolabel", "limit", "nonstd")
CASE_CFG = {
    "prior": dict(num_classes=10, num_tokens=64, embed_dim=64, n_layers=2, n_head=4, max_seq_len=16),
    "fm": dict(num_classes=10, num_tokens=512, embed_dim=256, n_layers=4, n_head=4, max_seq_len=16),
    "vanilla": dict(num_classes=10, num_tokens=513, embed_dim=512, n_layers=8, n_head=8, max_seq_len=2),
}


def case_cfg(name):
    return CASE_CFG[{"prior_nolabel": "prior", "limit": "prior", "nonstd": "prior", "vanilla_nolabel": "vanilla"}.get(name, name)]


def fixture_model(g, name, device="cpu"):
    """The fixture's weights (oracle.synthetic.seeded_state_dict), masks reset to the lower triangle except for `nonstd`."""
    from oracle import synthetic as syn
    from vqvae_amd.prior import Transformer
    cfg = case_cfg(name)
    model = Transformer(**cfg, dropout=0.1)
    sd = syn.seeded_state_dict(model.state_dict(), int(g[f"{name}/seed"]))
    if name != "nonstd":
        T = cfg["max_seq_len"]
        for k in sd:
            if k.endswith(".attn.bias"):
                sd[k] = torch.tril(torch.ones(T, T)).view(1, 1, T, T)
    model.load_state_dict(sd)
    return model.to(device)


def fixture_inputs(g, name, device="cpu"):
    x = torch.from_numpy(g[f"{name}/prompt"]).to(device)
    y = torch.from_numpy(g[f"{name}/y"]).to(device) if f"{name}/y" in g.files else None
    return x, y, g[f"{name}/tokens"]


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_greedy_sequences_equal_reference(golden, name):
    from vqvae_amd.prior import sample
    g = golden("prior_sample")
    model = fixture_model(g, name)
    x, y, want = fixture_inputs(g, name)
    got = sample(model, x, want.shape[1] - x.shape[1], top_k=1, y=y)
    assert got.dtype == torch.int64 and not model.training
    np.testing.assert_array_equal(got.numpy(), want)
    assert model._standard_mask == (name != "nonstd")


def test_kept_sets_equal_reference_top_k_logits_with_ties(golden):
    from vqvae_amd.prior.sampling import kept_mask, top_k_logits
    g = golden("prior_sample")
    rows = torch.from_numpy(g["ties/rows"])
    for k in (1, 2, 3, 5):
        ref = g[f"ties/k{k}"]
        np.testing.assert_array_equal(kept_mask(rows, k).numpy(), np.isfinite(ref))
        np.testing.assert_array_equal(top_k_logits(rows, k).numpy(), ref)
    assert kept_mask(rows, 2)[0].tolist() == [False, True, True, False, True, False, False, False]   # all three 3.0 kept


def test_draw_rule_on_hand_made_rows():
    from vqvae_amd.prior.sampling import draw_rule
    logits = torch.log(torch.tensor([[1.0, 2.0, 3.0, 4.0]])).repeat(7, 1)          # p = 0.1, 0.2, 0.3, 0.4
    u = torch.tensor([0.0, 0.05, 0.15, 0.35, 0.65, 0.999, 1.0])
    # 0 -> first index with positive mass; 1.0 leaves no prefix above u * S: the last kept index
    assert draw_rule(logits, u).tolist() == [0, 0, 1, 2, 3, 3, 3]
    # top_k=2 keeps {2, 3}: p = 3/7, 4/7
    assert draw_rule(logits, u, top_k=2).tolist() == [2, 2, 2, 2, 3, 3, 3]
    # a dropped last index is never drawn, even when rounding leaves no prefix above u * S
    rev = logits.flip(-1)
    assert draw_rule(rev, torch.ones(7), top_k=2).tolist() == [1] * 7
    # temperature divides: a very low temperature is the argmax, ties at the k-th value all kept
    tied = torch.tensor([[0.0, 2.0, 1.0, 2.0, 1.0]])
    assert draw_rule(tied.repeat(2, 1), torch.tensor([0.25, 0.75]), temperature=1e-3, top_k=1).tolist() == [1, 3]
    assert draw_rule(tied, torch.tensor([0.999]), temperature=0.5, top_k=2).tolist() == [3]


def test_limits_raise_like_the_reference(golden):
    from vqvae_amd.prior import sample
    g = golden("prior_sample")
    assert bool(g["limit/over_raises"])
    model = fixture_model(g, "limit")
    x = torch.zeros((1, 4), dtype=torch.int64)
    assert sample(model, x, 13, top_k=1).shape == (1, 17)                 # T0 + steps - 1 == max_seq_len is allowed
    with pytest.raises(AssertionError):
        sample(model, x, 14, top_k=1)
    with pytest.raises(ValueError):
        sample(model, x, 2, top_k=65)


def test_sample_with_uniforms_follows_the_draw_rule_and_is_seeded():
    from vqvae_amd.prior import Transformer, sample
    from vqvae_amd.prior.sampling import draw_rule
    torch.manual_seed(3)
    model = Transformer(num_classes=4, num_tokens=32, embed_dim=64, n_layers=2, n_head=2, max_seq_len=6, dropout=0.0)
    x = torch.randint(0, 32, (9, 2))
    y = torch.randint(0, 4, (9,))
    u = torch.rand(9, 4)
    got = sample(model, x, 4, temperature=0.8, top_k=7, y=y, uniforms=u)
    seq = x
    for k in range(4):
        seq = torch.cat((seq, draw_rule(model(seq, y=y)[:, -1], u[:, k], 0.8, 7)[:, None]), 1)
    assert torch.equal(got, seq)
    a = sample(model, x, 4, generator=torch.Generator().manual_seed(5))
    b = sample(model, x, 4, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------- the CLI
def np_save_image(images: np.ndarray, nrow: int) -> np.ndarray:
    """torchvision.utils.save_image(images, nrow=nrow) restated: make_grid (padding 2, pad value 0, gray -> RGB; a single image
    unpadded), x * 255 + 0.5 clamped to [0, 255], truncated to uint8, HWC."""
    if images.shape[1] == 1:
        images = np.repeat(images, 3, axis=1)
    n, c, h, w = images.shape
    if n == 1:
        grid = images[0]
    else:
        xm = min(nrow, n)
        ym = -(-n // xm)
        grid = np.zeros((c, ym * (h + 2) + 2, xm * (w + 2) + 2), np.float32)
        for k in range(n):
            r, q = divmod(k, xm)
            grid[:, r * (h + 2) + 2:r * (h + 2) + 2 + h, q * (w + 2) + 2:q * (w + 2) + 2 + w] = images[k]
    return np.clip(grid * np.float32(255) + np.float32(0.5), 0, 255).astype(np.uint8).transpose(1, 2, 0)


def tiny_setup(tmp, vanilla: bool, classes=(0, 2, 1), spc=3, top_k=5):
    """Tiny checkpoints in the reference's formats and a generate.yaml pointing at them."""
    from vqvae_amd.prior import Transformer
    from vqvae_amd.spatial_vae import SpatialVAE
    from vqvae_amd.vae import Decoder
    torch.manual_seed(11)
    d, K = (8, 16)
    tcfg = dict(num_tokens=K + 1 if vanilla else K, embed_dim=64, n_layers=2, n_head=4, max_seq_len=2 if vanilla else 16,
                num_classes=4, dropout=0.1)
    prior = Transformer(**tcfg)
    if vanilla:                                            # make BOS (the last token) practically undrawable
        with torch.no_grad():
            v = prior.views()
            v["head.weight"][-1].fill_(-1.0)
            v["head.weight"][:-1].uniform_(0.0, 0.2)
            v["ln_f.weight"].zero_()
            v["ln_f.bias"].fill_(1.0)
    torch.save(prior.state_dict(), os.path.join(tmp, "best.pt"))
    vcfg = dict(in_channels=1, output_image_size=28, latent_dim=d, enc_channels=[8, 16, 32], dec_channels=[32, 16, 8],
                recon_loss="mse", norm_type="batch", mse_use_sigmoid=True)
    if vanilla:
        dec = Decoder(1, (32, 16, 8), d, 28, "batch")
        state = {"decoder." + k: v for k, v in dec.state_dict().items()}
    else:
        state = SpatialVAE(**vcfg).state_dict()
    torch.save({"model_state_dict": state, "epoch": 3}, os.path.join(tmp, "vae.pt"))
    torch.save({"z_medoid": torch.randn(K, d), "medoid_indices": np.arange(K)}, os.path.join(tmp, "codebook.pt"))
    cfg = dict(transformer_ckpt_path=os.path.join(tmp, "best.pt"), vae_ckpt_path=os.path.join(tmp, "vae.pt"),
               codebook_path=os.path.join(tmp, "codebook.pt"), transformer=tcfg, vae=vcfg, num_samples=len(classes) * spc,
               temperature=1.0, top_k=top_k, class_labels=list(classes), samples_per_class=spc,
               output_dir=os.path.join(tmp, "out"), output_filename="generated_samples.png", device="cuda", seed=42,
               vanilla_vae=vanilla)
    path = os.path.join(tmp, "generate.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path, cfg


def check_cli_outputs(cfg, device):
    """The PNG equals save_image of the torch decoder (train mode, one class group at a time, sigmoid) on the written codes."""
    from vqvae_amd.scripts.generate_samples import load_models
    out = cfg["output_dir"]
    codes = torch.from_numpy(np.load(os.path.join(out, "generated_codes.npy")))
    labels = np.load(os.path.join(out, "generated_labels.npy"))
    spc, classes = cfg["samples_per_class"], cfg["class_labels"]
    T = cfg["transformer"]["max_seq_len"]
    assert codes.dtype == torch.int64 and codes.shape == (len(classes) * spc, 1 if cfg["vanilla_vae"] else T)
    np.testing.assert_array_equal(labels, np.repeat(classes, spc))
    _, decoder, z = load_models(cfg, device)
    assert decoder.training
    d = cfg["vae"]["latent_dim"]
    imgs = []
    with torch.no_grad():
        for i in range(len(classes)):
            c = codes[i * spc:(i + 1) * spc].to(device)
            zq = z[c[:, 0]] if cfg["vanilla_vae"] else z[c].permute(0, 2, 1).reshape(spc, d, 4, 4)
            imgs.append(decoder(zq).sigmoid().cpu())
    want = np_save_image(torch.cat(imgs).numpy(), spc)
    got = np.asarray(Image.open(os.path.join(out, cfg["output_filename"])).convert("RGB"))
    assert got.shape == want.shape
    assert np.abs(got.astype(int) - want.astype(int)).max() <= (0 if device.type == "cpu" else 1)
    return codes


@pytest.mark.parametrize("vanilla", [False, True])
def test_cli_on_cpu_writes_grid_and_codes(tmp_path, vanilla, monkeypatch):
    from vqvae_amd.scripts import generate_samples as gs
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    path, cfg = tiny_setup(str(tmp_path), vanilla)
    gs.main(path)
    codes = check_cli_outputs(cfg, torch.device("cpu"))
    first = codes.clone()
    gs.main(path)                                                         # seeded from the yaml's `seed`
    np.testing.assert_array_equal(np.load(os.path.join(cfg["output_dir"], "generated_codes.npy")), first.numpy())


def test_make_grid_restatement_edges():
    from vqvae_amd.scripts.generate_samples import make_grid
    r = np.random.RandomState(0)
    for n, nrow, c in ((1, 4, 1), (5, 3, 1), (4, 4, 3), (7, 10, 1)):
        x = r.rand(n, c, 5, 6).astype(np.float32)
        g = make_grid(torch.from_numpy(x), nrow).numpy()
        want = np_save_image(x, nrow).transpose(2, 0, 1)
        got = np.clip(g * np.float32(255) + np.float32(0.5), 0, 255).astype(np.uint8)
        np.testing.assert_array_equal(got, want)


def test_codes_outside_the_codebook_are_rejected_before_indexing():
    from vqvae_amd.scripts.generate_samples import decode
    from vqvae_amd.vae import Decoder
    dec = Decoder(1, (32, 16, 8), 8, 28, "batch")
    z = torch.randn(16, 8)
    bos = torch.full((4, 1), 16, dtype=torch.int64)                      # the vanilla prior's BOS = num_tokens - 1 = 16
    with pytest.raises(ValueError, match="outside the codebook"):
        decode(dec, z, bos, 2, True, 8)
    spatial = torch.zeros((2, 16), dtype=torch.int64)
    spatial[1, 5] = -1
    with pytest.raises(ValueError, match="outside the codebook"):
        decode(dec, z, spatial, 1, False, 8)
    assert decode(dec, z, torch.zeros((4, 1), dtype=torch.int64), 2, True, 8).shape == (4, 1, 28, 28)
