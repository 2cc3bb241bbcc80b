"""interpolate_images_spatial(relax_metric=...) and geodesic_interpolation --relax_metric end to end on a 300-image synthetic
spatial build (made as test_gpu_interpolation.py makes its own): "position" is what the call always did, "image" relaxes whole
grids under the whole decoder."""
import json
import os

import numpy as np
import pytest
import torch
from scipy import sparse

import path_cases as pc

pytestmark = pytest.mark.gpu

D, COUT, SIZE, N_IMG, F_CLI, ITERS = 16, 1, 28, 300, 5, 4
PAIRS = [(3, 100), (277, 4)]


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    from oracle import metric as om
    from vqvae_amd.scripts.build_codebook import main, make_parser
    tmp = str(tmp_path_factory.mktemp("grid_interpolation"))
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
    from vqvae_amd._device import DeviceCSR, device
    from vqvae_amd.spatial_decoder import load_decoder_from_checkpoint
    dev = device()
    cfg = torch.load(os.path.join(build["codebook"], "codebook.pt"), weights_only=False)["config"]
    codes = np.load(os.path.join(build["codebook"], "codes.npy"))
    W = sparse.load_npz(os.path.join(build["codebook"], "knn_graph_geodesic.npz")).tocsr()
    z = torch.load(build["z"]).float()
    dec = load_decoder_from_checkpoint(cfg["vae_ckpt_path"], in_channels=COUT, dec_channels=cfg["dec_channels"], latent_dim=D,
                                       output_image_size=SIZE, norm_type="batch", device=dev).eval()
    return z, np.flatnonzero(codes.reshape(-1) >= 0), DeviceCSR.from_scipy(W, dev), dec


def _cli(build, name, *extra):
    from vqvae_amd.scripts.geodesic_interpolation import main, make_parser
    out = os.path.join(build["tmp"], name)
    main(make_parser().parse_args(["--codebook_dir", build["codebook"], "--out_dir", out, "--frames", str(F_CLI),
                                   "--pairs", *[f"{i}:{j}" for i, j in PAIRS], *extra]))
    return out


def _same(a, b):
    if torch.is_tensor(a):
        return a.dtype == b.dtype and np.array_equal(pc.bits(a.cpu().numpy()), pc.bits(b.cpu().numpy()))
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_position_is_what_the_call_always_did(build):
    """relax_metric="position" returns the default call's fields bit for bit (with and without relaxation), and the CLI with
    --relax_metric position writes what it writes without the flag: the same arrays, the same JSON and PNG bytes."""
    from vqvae_amd.geo import interpolate_images_spatial
    z, lcc, G, dec = _resident(build)
    for iters in (0, ITERS):
        plain = interpolate_images_spatial(z, lcc, G, dec, PAIRS, F_CLI, "other", True, relax_iters=iters)
        named = interpolate_images_spatial(z, lcc, G, dec, PAIRS, F_CLI, "other", True, relax_iters=iters, relax_metric="position")
        assert sorted(plain) == sorted(named) and all(_same(plain[k], named[k]) for k in plain)
        assert ("energy_relaxed" in plain) == (iters > 0)
    assert plain["energy_relaxed"].shape == (2, 16) and plain["relax_from"].shape == (2, 16)
    a, b = _cli(build, "plain", "--relax_iters", str(ITERS)), _cli(build, "named", "--relax_iters", str(ITERS), "--relax_metric", "position")
    na, nb = np.load(os.path.join(a, "interpolation.npz")), np.load(os.path.join(b, "interpolation.npz"))
    assert na.files == nb.files and all(np.array_equal(pc.bits(na[k]), pc.bits(nb[k])) for k in na.files if na[k].dtype.kind == "f")
    assert all(np.array_equal(na[k], nb[k]) for k in na.files if na[k].dtype.kind != "f")
    ja, jb = (open(os.path.join(p, "interpolation.json")).read().replace(p, "") for p in (a, b))
    assert ja == jb and "relax_metric" not in ja
    assert open(os.path.join(a, "interpolation.png"), "rb").read() == open(os.path.join(b, "interpolation.png"), "rb").read()
    for k in ("energy_relaxed", "frames_relaxed", "images_relaxed"):
        assert np.array_equal(pc.bits(na[k]), pc.bits(plain[k].cpu().numpy())), k
    with pytest.raises(ValueError, match="relax_metric"):
        interpolate_images_spatial(z, lcc, G, dec, PAIRS, F_CLI, "other", True, relax_iters=1, relax_metric="pixel")


def test_image_metric_relaxes_whole_grids(build):
    """relax_metric="image": per pair energy_relaxed <= min(energy_geo, energy_lin), relax_from names the lower result (a tie the
    geodesic), the fields are relax_grid_curves_device's over frames_geo / frames_lin, images_relaxed are decode_images of
    frames_relaxed bit for bit, the ends stay, and the CLI writes the same fields."""
    from PIL import Image
    from vqvae_amd.decode import decode_images
    from vqvae_amd.geo import interpolate_images_spatial, relax_grid_curves_device
    z, lcc, G, dec = _resident(build)
    out = interpolate_images_spatial(z, lcc, G, dec, PAIRS, F_CLI, "other", True, relax_iters=ITERS, relax_metric="image")
    M = len(PAIRS)
    for k in ("energy_geo", "energy_lin", "energy_relaxed"):
        assert out[k].shape == (M,) and out[k].dtype == torch.float64
    for k in ("accepted_geo", "accepted_lin", "relax_from"):
        assert out[k].shape == (M,) and out[k].dtype == torch.int32
    assert out["frames_relaxed"].shape == (M, F_CLI, D, 4, 4) and out["images_relaxed"].shape == (M, F_CLI, COUT, SIZE, SIZE)
    assert out["image_len_relaxed"].shape == (M,) and out["curve_len_relaxed"].shape == (M,)
    geo = relax_grid_curves_device(dec, out["frames_geo"], ITERS)
    lin = relax_grid_curves_device(dec, out["frames_lin"], ITERS)
    assert geo.route == "native"
    assert _same(out["energy_geo"], geo.energy0) and _same(out["energy_lin"], lin.energy0)
    assert _same(out["accepted_geo"], geo.accepted) and _same(out["accepted_lin"], lin.accepted)
    e_geo, e_lin, e_rel = (t.cpu().numpy() for t in (geo.energy, lin.energy, out["energy_relaxed"]))
    start = np.minimum(out["energy_geo"].cpu().numpy(), out["energy_lin"].cpu().numpy())
    assert np.all(e_rel <= start) and np.array_equal(e_rel, np.minimum(e_geo, e_lin))
    assert out["relax_from"].tolist() == [int(a <= b) for a, b in zip(e_geo, e_lin)]
    assert int(out["accepted_geo"].min()) >= 1 and int(out["accepted_lin"].min()) >= 1 and np.all(e_rel < start)
    for m in range(M):
        assert _same(out["frames_relaxed"][m], (geo if out["relax_from"][m] else lin).frames[m])
    want = decode_images(dec, out["frames_relaxed"].view(-1, D, 4, 4), dataset="other", apply_sigmoid=True)
    assert _same(out["images_relaxed"].view(want.shape), want)
    for m, (i, j) in enumerate(PAIRS):
        assert _same(out["frames_relaxed"][m, 0].cpu(), z[i]) and _same(out["frames_relaxed"][m, -1].cpu(), z[j])
    plain = interpolate_images_spatial(z, lcc, G, dec, PAIRS, F_CLI, "other", True, relax_iters=ITERS)
    for k in ("frames_geo", "frames_lin", "images_geo", "images_lin", "curve_len_geo", "image_len_lin", "graph_dist"):
        assert _same(out[k], plain[k]), k
    with pytest.raises(ValueError, match="4x4"):
        interpolate_images_spatial(z[:, :, :2], lcc, G, dec, PAIRS, F_CLI, "other", True, relax_iters=1, relax_metric="image")
    cli = _cli(build, "image", "--relax_iters", str(ITERS), "--relax_metric", "image")
    npz = np.load(os.path.join(cli, "interpolation.npz"))
    for k in ("frames_relaxed", "images_relaxed", "image_len_relaxed", "curve_len_relaxed", "energy_geo", "energy_lin",
              "energy_relaxed", "accepted_geo", "accepted_lin", "relax_from"):
        assert npz[k].shape == tuple(out[k].shape) and np.array_equal(pc.bits(npz[k]) if npz[k].dtype.kind == "f" else npz[k],
                                                                      pc.bits(out[k].cpu().numpy()) if npz[k].dtype.kind == "f"
                                                                      else out[k].cpu().numpy()), k
    summary = json.load(open(os.path.join(cli, "interpolation.json")))
    assert summary["relax_metric"] == "image" and summary["relax_iters"] == ITERS
    for m, rec in enumerate(summary["pairs"]):
        assert rec["energy_relaxed"] == float(out["energy_relaxed"][m]) and rec["relax_from"] == [int(out["relax_from"][m])]
        assert rec["accepted_geo"] == [int(out["accepted_geo"][m])]
    with Image.open(os.path.join(cli, "interpolation.png")) as im:
        assert im.size == (F_CLI * (SIZE + 2) + 2, 3 * M * (SIZE + 2) + 2)
