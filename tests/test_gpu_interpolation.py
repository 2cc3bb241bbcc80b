"""vqvae_amd.geo.interpolation and python -m vqvae_amd.scripts.geodesic_interpolation end to end: a codebook built by the
build_codebook CLI on 128 seeded 16 x 4 x 4 latents (2 048 nodes) with a seeded 28-px decoder, then curves between node pairs
(both decoders) and between image pairs (the CLI).  Every comparison is bit for bit.  Nothing here says "the geodesic is
shorter than the chord": on seeded random latents and weights that is no property of the code."""
import json
import os

import numpy as np
import pytest
import torch
from scipy import sparse

import path_cases as pc

pytestmark = pytest.mark.gpu

D, COUT, SIZE, N_IMG, F_CLI = 16, 1, 28, 128, 5
PAIRS = [(3, 100), (77, 4)]
NPZ_SHAPES = {"pairs": (2, 2), "frames_lin": (2, F_CLI, D, 4, 4), "frames_geo": (2, F_CLI, D, 4, 4),
              "images_lin": (2, F_CLI, COUT, SIZE, SIZE), "images_geo": (2, F_CLI, COUT, SIZE, SIZE), "graph_dist": (2, 16),
              "hops": (2, 16), "status": (2, 16), "curve_len_lin": (2,), "curve_len_geo": (2,), "image_len_lin": (2,),
              "image_len_geo": (2,)}
PAIR_KEYS = ["curve_len_geo", "curve_len_lin", "fallback_positions", "graph_dist", "image_len_geo", "image_len_lin", "pair",
             "ratio_curve", "ratio_image"]


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    """A seeded decoder checkpoint and one build_codebook run on seeded latents."""
    from oracle import metric as om
    from vqvae_amd.scripts.build_codebook import main, make_parser
    tmp = str(tmp_path_factory.mktemp("interpolation"))
    sd = om.make_decoder_state(7, D, COUT, norm_type="batch")
    torch.save({"model_state_dict": {"decoder." + k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, "epoch": 0},
               os.path.join(tmp, "best.pt"))
    z4 = np.random.RandomState(7).randn(N_IMG * 16, D).astype(np.float32).reshape(N_IMG, 4, 4, D)
    z_path = os.path.join(tmp, "z.pt")
    torch.save(torch.from_numpy(np.ascontiguousarray(np.transpose(z4, (0, 3, 1, 2)))), z_path)
    out = os.path.join(tmp, "codebook")
    main(make_parser().parse_args([
        "--latents_path", z_path, "--out_dir", out, "--vae_ckpt_path", os.path.join(tmp, "best.pt"),
        "--in_channels", str(COUT), "--output_image_size", str(SIZE), "--latent_dim", str(D),
        "--enc_channels", "64", "128", "256", "--dec_channels", "256", "128", "64", "--recon_loss", "mse",
        "--norm_type", "batch", "--mse_use_sigmoid", "--k", "20", "--sym", "union", "--K", "64", "--init", "kpp",
        "--seed", "42", "--batch_size", "512"]))
    return {"tmp": tmp, "codebook": out, "z": z_path}


def _resident(build):
    """(z grids on the host, lcc_index, W, z_lcc on the GPU, G, the eval-mode decoder of the checkpoint)."""
    from vqvae_amd._device import DeviceCSR, device
    from vqvae_amd.spatial_decoder import load_decoder_from_checkpoint
    dev = device()
    cfg = torch.load(os.path.join(build["codebook"], "codebook.pt"), weights_only=False)["config"]
    codes = np.load(os.path.join(build["codebook"], "codes.npy"))
    W = sparse.load_npz(os.path.join(build["codebook"], "knn_graph_geodesic.npz")).tocsr()
    z = torch.load(build["z"]).float()
    lcc = np.flatnonzero(codes.reshape(-1) >= 0)
    z_lcc = z.permute(0, 2, 3, 1).reshape(-1, D)[torch.from_numpy(lcc)].contiguous().to(dev)
    dec = load_decoder_from_checkpoint(cfg["vae_ckpt_path"], in_channels=COUT, dec_channels=cfg["dec_channels"], latent_dim=D,
                                       output_image_size=SIZE, norm_type="batch", device=dev).eval()
    return z, lcc, W, z_lcc, DeviceCSR.from_scipy(W, dev), dec


def _bits(t):
    return pc.bits(t.cpu().numpy())


@pytest.mark.parametrize("kind", ["spatial", "vanilla"])
def test_node_pair_interpolation(kind, build):
    from vanilla_jvp_cases import make_decoder
    from vqvae_amd.geo import geodesic_interpolation
    from vqvae_amd.geo.geo_shortest_paths import distances_between
    from vqvae_amd.geo.riemannian_metric import edge_lengths_riemannian
    _, _, W, z_lcc, G, dec = _resident(build)
    if kind == "vanilla":
        dec = make_decoder((128, 64, 32), D, COUT, SIZE, "batch", seed=3).to(z_lcc.device)
    n = z_lcc.shape[0]
    r = np.random.RandomState(21)
    src, dst = r.randint(0, n, size=8), r.randint(0, n, size=8)
    src[5] = src[2]                                                 # a repeated source, and a pair that is one node
    dst[6] = src[6]
    before = {k: v.clone() for k, v in dec.state_dict().items()}
    out = geodesic_interpolation(z_lcc, G, dec, src, dst, 7, batch_size=512)
    for k, v in dec.state_dict().items():
        assert torch.equal(v, before[k]), k
    z_h = z_lcc.cpu().numpy()
    for name in ("frames_geo", "frames_lin"):
        fr = out[name]
        assert fr.shape == (8, 7, D) and fr.dtype == torch.float32
        assert np.array_equal(_bits(fr[:, 0]), pc.bits(z_h[src])) and np.array_equal(_bits(fr[:, -1]), pc.bits(z_h[dst]))
        want = torch.zeros(8, dtype=torch.float32, device=fr.device)
        for f in range(6):
            want = want + edge_lengths_riemannian(dec, fr[:, f].contiguous(), fr[:, f + 1].contiguous(), 512)
        got = out["curve_len_" + name[-3:]]
        assert got.shape == (8,) and got.dtype == torch.float32 and np.array_equal(_bits(got), _bits(want))
        assert bool(torch.isfinite(got).all()) and float(got[6]) == 0.0
    assert np.array_equal(_bits(out["frames_lin"]), pc.bits(pc.chord(z_h, src, dst, 7)))
    assert out["status"].tolist() == [0] * 8 and out["hops"][6].item() == 0 and int(out["hops"].max()) >= 2
    want_d = distances_between(W, src, dst)[np.arange(8), np.arange(8)]
    assert np.array_equal(_bits(out["graph_dist"]), pc.bits(want_d))
    with pytest.raises(ValueError, match="n_frames"):
        geodesic_interpolation(z_lcc, G, dec, src, dst, 1)


@pytest.fixture(scope="module")
def cli(build):
    from vqvae_amd.scripts.geodesic_interpolation import main, make_parser
    out = os.path.join(build["tmp"], "interp")
    main(make_parser().parse_args(["--codebook_dir", build["codebook"], "--out_dir", out, "--frames", str(F_CLI),
                                   "--pairs", *[f"{i}:{j}" for i, j in PAIRS]]))
    return out


def test_cli_artefacts_equal_the_api(build, cli):
    from PIL import Image
    from vqvae_amd.decode import decode_images
    from vqvae_amd.geo import interpolate_images_spatial
    z, lcc, _, _, G, dec = _resident(build)
    npz = np.load(os.path.join(cli, "interpolation.npz"))
    summary = json.load(open(os.path.join(cli, "interpolation.json")))
    assert sorted(npz.files) == sorted(list(NPZ_SHAPES) + ["fallback_pair", "fallback_position"])
    for k, shape in NPZ_SHAPES.items():
        assert npz[k].shape == shape, (k, npz[k].shape)
    assert npz["pairs"].tolist() == [list(p) for p in PAIRS]
    with Image.open(os.path.join(cli, "interpolation.png")) as im:
        assert im.size == (F_CLI * (SIZE + 2) + 2, 2 * len(PAIRS) * (SIZE + 2) + 2)
    for route in ("lin", "geo"):
        grids = torch.from_numpy(npz["frames_" + route]).to(G.indptr.device).view(-1, D, 4, 4)
        want = decode_images(dec, grids, dataset="other", apply_sigmoid=True)
        assert np.array_equal(pc.bits(npz["images_" + route].reshape(want.shape)), _bits(want))
    zf = z.permute(0, 2, 3, 1).reshape(-1, D).numpy()
    for m, (i, j) in enumerate(PAIRS):                               # every position's curve runs from image i to image j
        for route in ("lin", "geo"):
            fr = npz["frames_" + route][m]                           # [F, d, 4, 4]
            assert np.array_equal(pc.bits(fr[0]), pc.bits(z[i].numpy())) and np.array_equal(pc.bits(fr[-1]), pc.bits(z[j].numpy()))
        a, b = i * 16 + np.arange(16), j * 16 + np.arange(16)
        chord = pc.chord(zf, a, b, F_CLI)                            # [16, F, d]
        assert np.array_equal(pc.bits(npz["frames_lin"][m]), pc.bits(chord.reshape(4, 4, F_CLI, D).transpose(2, 3, 0, 1)))
    api = interpolate_images_spatial(z, lcc, G, dec, PAIRS, F_CLI, "other", True)
    assert sorted(summary) == ["apply_sigmoid", "codebook_dir", "dataset", "frames", "pairs", "totals"]
    assert summary["frames"] == F_CLI and summary["apply_sigmoid"] is True and len(summary["pairs"]) == 2
    for m, rec in enumerate(summary["pairs"]):
        assert sorted(rec) == PAIR_KEYS and rec["pair"] == list(PAIRS[m])
        for k in ("curve_len_lin", "curve_len_geo", "image_len_lin", "image_len_geo"):
            assert rec[k] == float(api[k][m]) and rec[k] == float(npz[k][m]), k
        ok = api["status"][m].cpu().numpy() == 0
        assert rec["graph_dist"] == float(api["graph_dist"][m].cpu().numpy()[ok].astype(np.float64).sum())
        assert rec["fallback_positions"] == api["fallback_positions"][m].tolist()
        assert rec["ratio_curve"] == rec["curve_len_geo"] / rec["curve_len_lin"]
        assert rec["ratio_image"] == rec["image_len_geo"] / rec["image_len_lin"]
    for k in ("graph_dist", "curve_len_lin", "curve_len_geo", "image_len_lin", "image_len_geo"):
        assert summary["totals"][k] == float(sum(r[k] for r in summary["pairs"]))
    assert np.array_equal(npz["status"], api["status"].cpu().numpy()) and np.array_equal(npz["hops"], api["hops"].cpu().numpy())
    assert np.array_equal(pc.bits(npz["graph_dist"]), _bits(api["graph_dist"]))
    assert len(npz["fallback_pair"]) == len(npz["fallback_position"]) == summary["totals"]["fallback_positions"]


def test_a_position_outside_the_graph_takes_the_chord(build):
    """The build's graph holds every position (codes.npy has no -1), so the case is made at the API: one node -- position 5
    of image 3 -- is taken out of the graph and of lcc_index.  That position, and any the removal cut off, get the chord."""
    from vqvae_amd._device import DeviceCSR
    from vqvae_amd.geo import interpolate_images_spatial
    z, lcc, W, _, G, dec = _resident(build)
    gone = int(np.searchsorted(lcc, 3 * 16 + 5))
    assert lcc[gone] == 3 * 16 + 5
    keep = np.delete(np.arange(W.shape[0]), gone)
    G_cut = DeviceCSR.from_scipy(W[keep][:, keep].tocsr(), G.indptr.device)
    out = interpolate_images_spatial(z, lcc[keep], G_cut, dec, PAIRS, F_CLI, "other", True)
    full = interpolate_images_spatial(z, lcc, G, dec, PAIRS, F_CLI, "other", True)
    status = out["status"].cpu().numpy()
    assert status[0, 5] == 3 and out["hops"][0, 5].item() == -1 and bool(torch.isnan(out["graph_dist"][0, 5]))
    assert 5 in out["fallback_positions"][0].tolist() and (status[1] != 3).all()
    geo, lin = out["frames_geo"].cpu().numpy(), out["frames_lin"].cpu().numpy()      # [M, F, d, 4, 4]
    assert np.array_equal(pc.bits(lin), _bits(full["frames_lin"]))
    for m in range(2):
        fb = out["fallback_positions"][m]
        assert fb.tolist() == np.flatnonzero(status[m] != 0).tolist()
        for p in range(16):
            same = np.array_equal(pc.bits(geo[m, :, :, p // 4, p % 4]), pc.bits(lin[m, :, :, p // 4, p % 4]))
            assert same or p not in fb, (m, p)
    moved = [(m, p) for m in range(2) for p in range(16) if status[m, p] == 0 and out["hops"][m, p].item() >= 2
             and not np.array_equal(pc.bits(geo[m, :, :, p // 4, p % 4]), pc.bits(lin[m, :, :, p // 4, p % 4]))]
    assert moved                                                     # a multi-hop geodesic is not the chord
    assert full["status"].cpu().numpy().tolist() == [[0] * 16] * 2 and all(len(p) == 0 for p in full["fallback_positions"])
    with pytest.raises(ValueError, match="lcc_index"):
        interpolate_images_spatial(z, lcc, G_cut, dec, PAIRS, F_CLI, "other", True)
