"""geo_vanilla_metric_tensor (csrc/vanilla_jvp.hip: the unit-tangent column pass, vm_gram_kernel; csrc/sym_spectrum.hip) and
pullback_metric_device on vanilla decoders, on the GPU: the Gram against the call's own columns, G and the
columns against fp64 autograd with float32 autograd as the yardstick, the spectrum against numpy on the call's own G, the
cross-checks against geo_vanilla_curve_energy's trace and geo_vanilla_jvp_pairs, bit equality under everything a latent's results
must not depend on, and the refusals."""
import copy

import numpy as np
import pytest
import torch

import vanilla_curve_cases as K
import vanilla_jvp_cases as V
import vanilla_metric_cases as M
from metric_tensor_cases import normalised_error, rank_rule

pytestmark = pytest.mark.gpu
GEO_E_ARG, GEO_E_WORKSPACE = -1, -2


def _dev():
    return torch.device("cuda", 0)


def _export(name):
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    return VanillaDecoderExport(K.decoder(name), _dev())


def _raw(ex, z, *, index=None, ws_bytes=None, fill=None, spectrum=True, jac=True):
    """geo_vanilla_metric_tensor on a workspace of this test's own: (status, G, J, eig, logvol, rank) as numpy arrays (None
    where not asked for), the outputs pre-filled."""
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    lib = _lib.load()
    dev = z.device
    n = int(z.shape[0] if index is None else index.numel())
    d, nout = ex.latent_dim, ex.n_out
    if ws_bytes is None:
        ws_bytes = lib.geo_vanilla_metric_workspace_bytes(ex.desc, n)
    ws = torch.empty(max(int(ws_bytes), 256), dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    G = torch.full((n, d, d), float("nan"), dtype=torch.float64, device=dev)
    J = torch.full((n, d, nout), float("nan"), dtype=torch.float32, device=dev) if jac else None
    eig = torch.full((n, d), float("nan"), dtype=torch.float64, device=dev) if spectrum else None
    logvol = torch.full((n,), float("nan"), dtype=torch.float64, device=dev) if spectrum else None
    rank = torch.full((n,), -7, dtype=torch.int32, device=dev) if spectrum else None
    with torch.cuda.device(dev):
        status = lib.geo_vanilla_metric_tensor(ex.desc, ptr(z), ptr(index), n, ptr(G), ptr(J), ptr(eig), ptr(logvol), ptr(rank),
                                               ptr(ws), int(ws_bytes), stream_ptr())
        torch.cuda.current_stream().synchronize()
    return (status,) + tuple(None if t is None else t.cpu().numpy() for t in (G, J, eig, logvol, rank))


def _same_bits(a, b):
    for x, y in zip(a[1:], b[1:]):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.tobytes() == y.tobytes()


_results = {}


def _case_result(name):
    """The raw call on a case's 33 reference latents, computed once."""
    if name not in _results:
        z = M.reference(name)[0]
        out = _raw(_export(name), z.to(_dev()))
        assert out[0] == 0
        _results[name] = out
    return _results[name]


_torch_errors = {}


def _torch_error(name):
    """e of float32 torch's own answer on the same GPU (jacfwd of the float32 module, the Gram matrix in fp64); computed once."""
    if name not in _torch_errors:
        z, _, G64 = M.reference(name)
        dec_gpu = copy.deepcopy(K.decoder(name)).to(_dev())

        def image(latent):
            return torch.sigmoid(dec_gpu(latent.view(1, -1))).reshape(-1)

        with torch.no_grad():
            J = torch.func.vmap(torch.func.jacfwd(image))(z.to(_dev())).double()
        _torch_errors[name] = normalised_error(torch.bmm(J.transpose(1, 2), J).cpu().numpy(), G64)
    return _torch_errors[name]


# ------------------------------------------------------------------------------------------------ 1. the Gram kernel
@pytest.mark.parametrize("name", M.CASES)
def test_gram_of_the_calls_own_columns(name):
    """G against the numpy fp64 Gram of jac_out: both add exact products, at most nout roundings each."""
    _, G, J, eig, logvol, rank = _case_result(name)
    nout = J.shape[2]
    assert not np.isnan(G).any() and not np.isnan(J).any()
    assert G.transpose(0, 2, 1).tobytes() == G.tobytes()                          # G[a][b] and G[b][a]: the same bits
    J = J.astype(np.float64)
    Gnp = np.einsum("nao,nbo->nab", J, J)
    diag = np.sqrt(np.einsum("naa->na", G))
    err = np.abs(G - Gnp) / (2 * nout * M.DBL_EPS * diag[:, :, None] * diag[:, None, :])
    print(f"{name}: max |G - Gnp| / (2 nout eps sqrt(G_aa G_bb)) = {err.max():.3e}")
    assert err.max() <= 1.0


# ------------------------------------------------------------------------------------------------ 2. G against fp64
@pytest.mark.parametrize("name", M.CASES)
def test_G_against_fp64(name):
    z, _, G64 = M.reference(name)
    G = _case_result(name)[1]
    e_torch = _torch_error(name)
    e = normalised_error(G, G64)
    print(f"{name}: e = {e:.3e}, e_torch = {e_torch:.3e}, ratio = {e / e_torch:.2f}")
    assert e <= 4 * e_torch + 1e-7


# ------------------------------------------------------------------------------------------------ 3. the columns
@pytest.mark.parametrize("name", M.CASES)
def test_columns_against_fp64(name):
    """Per row (latent, k): e = |J[i][k] - ref|_2 / |ref|_2 against fp64 forward-mode autograd.  Gates as for geo_vanilla_vjp:
    median and 0.99-quantile at most 4 x float32 autograd's on the same rows, rows above 1e-5 at most the cap of
    vanilla_curve_cases scaled to the row count; float32 autograd itself (on the CPU) stays inside the cap."""
    _, J64, _ = M.reference(name)
    J32 = M.reference32(name)
    J = _case_result(name)[2]
    nout = J.shape[2]
    assert J.dtype == np.float32 and J.shape == J64.shape
    e = K.row_error(J.reshape(-1, nout), J64.reshape(-1, nout))
    e_t = K.row_error(J32.reshape(-1, nout), J64.reshape(-1, nout))
    cap = M.boundary_cap(e.size)
    med, q99, above = np.median(e), np.quantile(e, 0.99), int((e > 1e-5).sum())
    med_t, q99_t, above_t = np.median(e_t), np.quantile(e_t, 0.99), int((e_t > 1e-5).sum())
    print(f"{name}: native median {med:.3e} q99 {q99:.3e} max {e.max():.3e} above 1e-5: {above} of {e.size} (cap {cap}) | float32 "
          f"autograd median {med_t:.3e} q99 {q99_t:.3e} max {e_t.max():.3e} above 1e-5: {above_t} | ratios {med / med_t:.2f} "
          f"{q99 / q99_t:.2f}")
    assert above_t <= cap
    assert med <= 4 * med_t and q99 <= 4 * q99_t and above <= cap


# ------------------------------------------------------------------------------------------------ 4. the spectrum
def _sweeps(G, p_out, want):
    """The sweeps geo_sym_spectrum_sweeps takes on G [n, d, d]; its three results are the bits of `want`, the call's own."""
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    lib = _lib.load()
    dev = _dev()
    g = torch.from_numpy(G).to(dev)
    n, d = g.shape[0], g.shape[1]
    eig = torch.empty(n, d, dtype=torch.float64, device=dev)
    logvol = torch.empty(n, dtype=torch.float64, device=dev)
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    sweeps = torch.full((n,), -1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        assert lib.geo_sym_spectrum_sweeps(ptr(g), n, d, p_out, ptr(eig), ptr(logvol), ptr(rank), ptr(sweeps), stream_ptr()) == 0
        torch.cuda.current_stream().synchronize()
    for got, ref in zip((eig, logvol, rank), want):
        assert got.cpu().numpy().tobytes() == ref.tobytes()
    sweeps = sweeps.cpu().numpy()
    assert np.all(sweeps >= 0) and sweeps.max() < lib.geo_sym_spectrum_sweep_cap()
    return sweeps


@pytest.mark.parametrize("name", M.CASES)
def test_spectrum_against_eigvalsh_of_own_G(name):
    _, _, G64 = M.reference(name)
    _, G, J, eig, logvol, rank = _case_result(name)
    d, nout = G.shape[1], J.shape[2]
    assert eig.dtype == np.float64 and logvol.dtype == np.float64 and rank.dtype == np.int32
    assert not np.isnan(eig).any() and not np.isnan(logvol).any()
    ref = np.linalg.eigvalsh(G)
    assert np.all(np.diff(eig, axis=1) >= 0)
    err = np.abs(eig - ref) / (64 * d * M.DBL_EPS * ref[:, -1:])
    print(f"{name}: max |eig - eigvalsh(G)| / (64 d eps eig_max) = {err.max():.3e}")
    assert err.max() <= 1.0
    sweeps = _sweeps(G, nout, (eig, logvol, rank))
    print(f"{name}: Jacobi sweeps {sweeps.min()} .. {sweeps.max()}")
    thr = (max(nout, d) * M.FLT_EPS) ** 2 * ref[:, -1:]
    assert not np.any((ref > thr / 4) & (ref < thr * 4))                          # no eigenvalue near the rank threshold
    np.testing.assert_array_equal(rank, rank_rule(ref, nout))
    ref64 = np.linalg.eigvalsh(G64)
    cond64 = ref64[:, -1] / ref64[:, 0]
    print(f"{name}: cond(G64) {cond64.min():.3e} .. {cond64.max():.3e}, lambda_min {ref64[:, 0].min():.3e}, rank min {rank.min()}")
    if name in M.WELL_CONDITIONED:
        assert cond64.max() <= 1e3
        assert np.all(rank == d) and np.all(np.isfinite(logvol))
        cond = ref[:, -1] / ref[:, 0]
        d_own = np.abs(logvol - 0.5 * np.sum(np.log(ref), axis=1))
        assert np.all(d_own <= d * 64 * d * M.DBL_EPS * cond)
        d_64 = np.abs(logvol - 0.5 * np.linalg.slogdet(G64)[1])
        e_torch = _torch_error(name)
        print(f"{name}: logvol vs own spectrum max {d_own.max():.3e}, vs slogdet(G64) max {d_64.max():.3e}")
        assert np.all(d_64 <= d * cond64 * (4 * e_torch + 1e-7))


# ------------------------------------------------------------------------------------------------ 5. other entry points
@pytest.mark.parametrize("name", ["wide-bn-32x3", "narrow-none-28", "wide-none-28x3-d127", "narrow-none-32x1-d1"])
def test_trace_of_the_curve_energy(name):
    """trace_out of geo_vanilla_curve_energy sums the squares of the same columns in f32, sum_k G[k][k] in fp64: all terms
    non-negative, so the relative difference is at most nout * FLT_EPSILON."""
    from vqvae_amd.geo import curve_energy_device
    ex = _export(name)
    z = K.rows(name)[0][:36].to(_dev())
    G = _raw(ex, z, spectrum=False, jac=False)[1]
    tr = curve_energy_device(ex, z.view(4, 9, -1), trace=True).trace.cpu().numpy().reshape(-1)
    mine = np.einsum("naa->n", G)
    rel = np.abs(tr - mine) / mine
    print(f"{name}: max relative difference of the traces {rel.max():.3e} (gate {ex.n_out * M.FLT_EPS:.3e})")
    assert np.all(rel <= ex.n_out * M.FLT_EPS)


@pytest.mark.parametrize("name", ["narrow-none-32x3-d5", "narrow-none-28", "wide-bn-32x3"])
def test_consistent_with_edge_lengths(name):
    """0.5 (sqrt(dz^T G_a dz) + sqrt(dz^T G_b dz)) against geo_vanilla_jvp_pairs on 400 edges, the gate of
    test_gpu_metric_tensor.py::test_consistent_with_edge_lengths: 99.9 % within 1e-5 (every case here has cond(G) <= 12)."""
    from vqvae_amd.geo.riemannian_metric import edge_lengths_vanilla_device
    TOL = 1e-5
    ex = _export(name)
    z, src, dst = V.small_graph(M.latent_dim(name), n_nodes=120, n_edges=400)
    src, dst = src.long().numpy(), dst.long().numpy()
    zg = z.to(_dev())
    G = _raw(ex, zg, spectrum=False, jac=False)[1]
    ref = edge_lengths_vanilla_device(ex, zg[src].contiguous(), zg[dst].contiguous()).double().cpu().numpy()
    dz = z[dst].double().numpy() - z[src].double().numpy()
    quad = lambda nodes: np.sqrt(np.einsum("ea,eab,eb->e", dz, G[nodes], dz))      # noqa: E731
    got = 0.5 * (quad(src) + quad(dst))
    keep = ref > 0                                                                # (self loops have length 0)
    rel = np.abs(got[keep] - ref[keep]) / ref[keep]
    print(f"{name}: {np.mean(rel <= TOL):.4%} of {keep.sum()} edges within {TOL}, max rel {rel.max():.3e}")
    assert np.all(got[~keep] == 0.0)
    assert np.mean(rel <= TOL) >= 0.999


# ------------------------------------------------------------------------------------------------ 6. exact properties
@pytest.mark.parametrize("name", M.EXACT_CASES)
def test_results_do_not_depend_on_their_company(name):
    """Bit for bit (G, jac_out, the spectrum): n in {1, 2, 3, 63, 64, 65} under a permutation and through `index`; the minimum
    workspace and one in between, both filled with 0xFF first; a side stream; without jac_out; without the spectrum."""
    from vqvae_amd import _lib
    lib = _lib.load()
    dev = _dev()
    ex = _export(name)
    z65 = K.rows(name)[0][:65].to(dev)
    full = _raw(ex, z65)
    assert full[0] == 0, lib.geo_last_error()
    assert not any(np.isnan(t).any() for t in full[1:5]) and np.all(full[5] >= 0)
    for n in (1, 2, 3, 63, 64, 65):
        perm = np.random.RandomState(n).permutation(n)
        pg = torch.from_numpy(perm).to(dev)
        want = (0,) + tuple(t[:n][perm] for t in full[1:])
        _same_bits(_raw(ex, z65[:n][pg].contiguous()), want)
        _same_bits(_raw(ex, z65, index=pg.to(torch.int32)), want)
    least = lib.geo_vanilla_metric_min_workspace_bytes(ex.desc)
    assert 0 < least == lib.geo_vanilla_metric_workspace_bytes(ex.desc, 1) == lib.geo_vanilla_metric_workspace_bytes(ex.desc, 2)
    assert least < lib.geo_vanilla_metric_workspace_bytes(ex.desc, 7) < lib.geo_vanilla_metric_workspace_bytes(ex.desc, 65)
    for n, cap in ((5, least), (65, lib.geo_vanilla_metric_workspace_bytes(ex.desc, 7) + 1000)):
        _same_bits(_raw(ex, z65[:n].contiguous(), ws_bytes=cap, fill=0xFF), (0,) + tuple(t[:n] for t in full[1:]))
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        _same_bits(_raw(ex, z65, fill=0xFF), full)
    no_jac = _raw(ex, z65, jac=False)
    assert no_jac[2] is None
    _same_bits(no_jac[:2] + no_jac[3:], full[:2] + full[3:])
    no_spec = _raw(ex, z65, spectrum=False)
    assert no_spec[3] is None and no_spec[4] is None and no_spec[5] is None
    _same_bits(no_spec[:3], full[:3])


def test_more_than_one_slice_at_the_queried_size():
    """d = 1: the slice cap is 8192 latents; 8195 latents run two slices at the size the query answers."""
    name = "narrow-none-32x1-d1"
    ex = _export(name)
    z = torch.randn(8195, 1, generator=torch.Generator().manual_seed(5)).to(_dev())
    out = _raw(ex, z, jac=False)
    assert out[0] == 0 and not np.isnan(out[1]).any() and np.all(out[5] == 1)
    tail = _raw(ex, z[8190:].contiguous(), jac=False)
    _same_bits(tail, (0,) + tuple(None if t is None else t[8190:] for t in out[1:]))


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_without_a_launch():
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr
    lib = _lib.load()
    dev = _dev()
    ex = _export("narrow-none-28")
    n, d = 4, 16
    z = torch.zeros(n, d, device=dev)
    G = torch.full((n, d, d), 7.0, dtype=torch.float64, device=dev)
    eig = torch.full((n, d), 7.0, dtype=torch.float64, device=dev)
    lv = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    rk = torch.full((n,), -7, dtype=torch.int32, device=dev)
    nb = lib.geo_vanilla_metric_workspace_bytes(ex.desc, n)
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    call = lib.geo_vanilla_metric_tensor
    for field, value in (("c1", 32), ("latent_dim", 129), ("out_channels", 2), ("out_size", 64)):
        bad = _lib.VanillaDecoderDesc.from_buffer_copy(ex.desc)
        setattr(bad, field, value)
        assert lib.geo_vanilla_metric_workspace_bytes(bad, n) == 0 and lib.geo_vanilla_metric_min_workspace_bytes(bad) == 0, field
        assert call(bad, ptr(z), None, n, ptr(G), None, ptr(eig), ptr(lv), ptr(rk), ptr(ws), nb, None) == GEO_E_ARG, field
    for triple in ((ptr(eig), None, None), (None, ptr(lv), ptr(rk)), (ptr(eig), ptr(lv), None)):
        assert call(ex.desc, ptr(z), None, n, ptr(G), None, *triple, ptr(ws), nb, None) == GEO_E_ARG
    assert call(ex.desc, None, None, n, ptr(G), None, None, None, None, ptr(ws), nb, None) == GEO_E_ARG
    assert call(ex.desc, ptr(z), None, n, None, None, None, None, None, ptr(ws), nb, None) == GEO_E_ARG
    assert call(ex.desc, ptr(z), None, -1, ptr(G), None, None, None, None, ptr(ws), nb, None) == GEO_E_ARG
    least = lib.geo_vanilla_metric_min_workspace_bytes(ex.desc)
    assert call(ex.desc, ptr(z), None, n, ptr(G), None, None, None, None, ptr(ws), least - 1, None) == GEO_E_WORKSPACE
    assert call(ex.desc, None, None, 0, None, None, None, None, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.all(G == 7.0) and torch.all(eig == 7.0) and torch.all(lv == 7.0) and torch.all(rk == -7)


# ------------------------------------------------------------------------------------------------ 8. Python
def test_python_routes_and_jacobian():
    from vqvae_amd.geo import native_metric_covers, native_vanilla_metric_covers, pullback_metric, pullback_metric_device
    name = "narrow-none-28"
    dev = _dev()
    dec = K.decoder(name)
    assert native_vanilla_metric_covers(dec) and not native_metric_covers(dec)
    z = M.reference(name)[0]
    raw = _case_result(name)
    for target in (_export(name), copy.deepcopy(dec).to(dev)):
        res = pullback_metric_device(target, z.to(dev), jacobian=True)
        assert res.route == "native" and res.G.is_cuda and res.J.dtype == torch.float32
        for got, want in zip((res.G, res.J, res.eig, res.logvol, res.rank), raw[1:]):
            assert got.cpu().numpy().tobytes() == want.tobytes()
    plain = pullback_metric_device(_export(name), z.to(dev), spectrum=False,
                                   max_workspace_bytes=_lib_min(_export(name)))
    assert plain.J is None and plain.eig is None and plain.G.cpu().numpy().tobytes() == raw[1].tobytes()
    host = pullback_metric(dec, z.numpy(), jacobian=True)                         # a CPU module: runs on this process's GPU
    assert host.route == "native" and host.G.tobytes() == raw[1].tobytes() and host.J.tobytes() == raw[2].tobytes()
    with pytest.raises(ValueError, match="latent dimensions"):
        pullback_metric_device(_export(name), torch.zeros(3, 15, device=dev))
    with pytest.raises(ValueError, match="latent dimensions"):
        pullback_metric_device(copy.deepcopy(dec).to(dev), torch.zeros(3, 17, device=dev))
    # the autograd route (an uncovered width) carries jacfwd's J in the same layout
    other = V.build((64, 32, 16), 6, 1, 28, "none", seed=3)
    assert not native_vanilla_metric_covers(other)
    zo = torch.randn(5, 6, generator=torch.Generator().manual_seed(1))
    auto = pullback_metric_device(other, zo, jacobian=True)
    assert auto.route == "autograd" and tuple(auto.J.shape) == (5, 6, 784) and auto.J.dtype == torch.float32
    J = auto.J.double()
    assert torch.allclose(torch.bmm(J, J.transpose(1, 2)), auto.G, rtol=1e-12, atol=0)


def _lib_min(ex):
    from vqvae_amd import _lib
    return int(_lib.load().geo_vanilla_metric_min_workspace_bytes(ex.desc))


def test_cli_on_a_legacy_build_runs_natively(tmp_path):
    """python -m vqvae_amd.scripts.vanilla_metric_map --codebook_dir on a covered decoder: route native, the arrays of
    pullback_metric_device, and the same bits whatever --chunk is."""
    import json
    import os
    from vqvae_amd.geo import pullback_metric_device
    from vqvae_amd.scripts import vanilla_metric_map as cli
    tmp = str(tmp_path)
    dec = K.decoder("narrow-none-28")
    vae = dict(in_channels=1, enc_channels=[32, 64, 128], dec_channels=[128, 64, 32], latent_dim=16, recon_loss="bce",
               output_image_size=28, norm_type="none", mse_use_sigmoid=True)
    torch.save({"model_state_dict": {"decoder." + k: v for k, v in dec.state_dict().items()}}, os.path.join(tmp, "best.pt"))
    z = K.rows("narrow-none-28")[0][:10].clone()
    torch.save({"z": z}, os.path.join(tmp, "z.pt"))
    out = os.path.join(tmp, "build")
    os.makedirs(out)
    codes = np.full(10, -1, dtype=np.int32)
    codes[:8] = np.arange(8) % 3
    np.save(os.path.join(out, "codes.npy"), codes)
    config = {"data": {"latents_path": os.path.join(tmp, "z.pt")}, "checkpoint_path": os.path.join(tmp, "best.pt"),
              "vae_config": vae, "graph": {"k": 3, "metric": "euclidean", "sym": "mutual", "mode": "distance"},
              "riemannian": {"mode": "full", "max_edges": 100, "batch_size": 16},
              "quantize": {"K": 3, "init": "kpp", "seed": 42}, "out": {"dir": out}}
    torch.save({"medoid_indices": np.array([0, 1, 2], dtype=np.int32), "z_medoid": z[:3], "config": config, "graph_stats": {},
                "method": "riemannian_geodesic"}, os.path.join(out, "codebook.pt"))
    one = cli.main(cli.make_parser().parse_args(["--codebook_dir", out, "--out_dir", os.path.join(tmp, "a"), "--save_tensors"]))
    cut = cli.main(cli.make_parser().parse_args(["--codebook_dir", out, "--out_dir", os.path.join(tmp, "b"), "--save_tensors",
                                                 "--chunk", "4"]))
    assert one["route"] == "native" and one["decoder"] == "vanilla" and one == cut and set(one["per_code"]) == {"0", "1", "2"}
    a, b = np.load(os.path.join(tmp, "a", "metric_map.npz")), np.load(os.path.join(tmp, "b", "metric_map.npz"))
    assert set(a.files) == {"logvol", "trace", "eig_min", "eig_max", "rank", "index", "G"}
    for key in a.files:
        assert a[key].tobytes() == b[key].tobytes(), key
    res = pullback_metric_device(_export("narrow-none-28"), z.to(_dev()))
    assert a["G"].tobytes() == res.G.cpu().numpy().tobytes() and a["logvol"].tobytes() == res.logvol.cpu().numpy().tobytes()
    assert a["eig_max"].tobytes() == res.eig[:, -1].contiguous().cpu().numpy().tobytes()
    with open(os.path.join(tmp, "a", "metric_map.json")) as fh:
        assert json.load(fh) == json.loads(json.dumps(one))
    assert os.path.getsize(os.path.join(tmp, "a", "metric_map.png")) > 0
