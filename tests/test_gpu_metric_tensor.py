"""geo_decoder_metric_tensor (csrc/jvp.hip: the column pass, jacobian_gram_kernel, metric_spectrum_kernel) and
vqvae_amd.geo.pullback_metric_device on the GPU, against the fp64 autograd reference of tests/metric_tensor_cases.py.

The yardstick of the G gates is float32 torch on the same GPU: torch.func.jacfwd of the float32 module, its Gram matrix formed in
fp64, and that matrix's error e_torch against G64.  Gate: e <= 4 * e_torch + 1e-7 (the project's native paths sit within 0.6-2.6 x
of float32 torch's own error; the floor guards a lucky e_torch).  Every test prints the figures it asserts on.

fm_small (dec_channels 32-32-16) has no per-latent column pass in the library (the per-latent Jacobian route needs
dec_channels[2] == 64), so the Python call takes the autograd route for it; the case stays in the G and spectrum tests."""
import numpy as np
import pytest
import torch

from metric_tensor_cases import (CASES, NATIVE, N_LATENTS, WELL_CONDITIONED, gram64_of, make_decoder, make_latents,
                                 normalised_error, p_out_of, rank_rule, reference)

pytestmark = pytest.mark.gpu

DBL_EPS = float(np.finfo(np.float64).eps)
GEO_E_ARG = -1


def _dev():
    from vqvae_amd._device import device
    return device()


def _torch_gram(dec_gpu, z_gpu):
    """float32 torch's own answer: jacfwd of the float32 module on the GPU, the Gram matrix in fp64."""
    first = next(dec_gpu.children())
    flat = hasattr(first, "in_features")

    def image(latent):
        x = latent.view(1, -1) if flat else latent.view(1, -1, 1, 1)
        return torch.sigmoid(dec_gpu(x)).reshape(-1)

    with torch.no_grad():
        J = torch.func.vmap(torch.func.jacfwd(image))(z_gpu).double()
    return torch.bmm(J.transpose(1, 2), J).cpu().numpy()


_results = {}


def _case_result(name):
    """pullback_metric_device of a case on its 33 reference latents, and float32 torch's error: computed once."""
    if name not in _results:
        from vqvae_amd.geo import pullback_metric_device
        z, G64 = reference(name)
        dec = make_decoder(name)[0].to(_dev())
        zg = torch.tensor(z, device=_dev())
        res = pullback_metric_device(dec, zg)
        e_torch = normalised_error(_torch_gram(dec, zg), G64)
        _results[name] = (res, e_torch)
    return _results[name]


def _raw_call(export, z, *, ws_bytes=None, fill=None, spectrum=True):
    """geo_decoder_metric_tensor on a workspace of this test's own: (status, G, eig, logvol, rank) as numpy arrays."""
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    lib = _lib.load()
    dev = z.device
    n, d = z.shape
    if ws_bytes is None:
        ws_bytes = lib.geo_metric_tensor_workspace_bytes(export.desc, n)
    ws = torch.empty(max(int(ws_bytes), 256), dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    G = torch.full((n, d, d), float("nan"), dtype=torch.float64, device=dev)
    eig = torch.full((n, d), float("nan"), dtype=torch.float64, device=dev) if spectrum else None
    logvol = torch.full((n,), float("nan"), dtype=torch.float64, device=dev) if spectrum else None
    rank = torch.full((n,), -7, dtype=torch.int32, device=dev) if spectrum else None
    with torch.cuda.device(dev):
        status = lib.geo_decoder_metric_tensor(export.desc, ptr(z), n, ptr(G), ptr(eig), ptr(logvol), ptr(rank), ptr(ws),
                                               int(ws_bytes), stream_ptr())
        torch.cuda.current_stream().synchronize()
    return (status,) + tuple(None if t is None else t.cpu().numpy() for t in (G, eig, logvol, rank))


def _export(name, mutate=None):
    from vqvae_amd.spatial_decoder import DecoderExport
    dec = make_decoder(name)[0]
    if mutate is not None:
        mutate(dec)
    return DecoderExport(dec.to(_dev()), _dev())


def _same_bits(a, b):
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------ 1. G against fp64
@pytest.mark.parametrize("name", list(CASES))
def test_G_against_fp64(name):
    from vqvae_amd.geo import native_metric_covers
    z, G64 = reference(name)
    res, e_torch = _case_result(name)
    assert res.route == ("native" if name in NATIVE else "autograd")
    assert native_metric_covers(make_decoder(name)[0]) == (name in NATIVE)
    G = res.G.cpu().numpy()
    assert res.G.is_cuda and res.G.dtype == torch.float64 and G.shape == (N_LATENTS, CASES[name][1], CASES[name][1])
    e = normalised_error(G, G64)
    print(f"{name}: e = {e:.3e}, e_torch = {e_torch:.3e}, ratio = {e / e_torch:.2f}")
    assert e <= 4 * e_torch + 1e-7


# ------------------------------------------------------------------------------------------------ 2. the spectrum
@pytest.mark.parametrize("name", list(CASES))
def test_spectrum_against_eigvalsh_of_own_G(name):
    z, G64 = reference(name)
    res, e_torch = _case_result(name)
    d = CASES[name][1]
    G, eig, logvol, rank = (t.cpu().numpy() for t in (res.G, res.eig, res.logvol, res.rank))
    assert eig.dtype == np.float64 and logvol.dtype == np.float64 and rank.dtype == np.int32
    assert not np.isnan(G).any() and not np.isnan(eig).any() and not np.isnan(logvol).any()
    ref = np.linalg.eigvalsh(G)
    assert np.all(np.diff(eig, axis=1) >= 0)
    err = np.abs(eig - ref) / (64 * d * DBL_EPS * ref[:, -1:])
    print(f"{name}: max |eig - eigvalsh(G)| / (64 d eps eig_max) = {err.max():.3e}")
    assert err.max() <= 1.0
    np.testing.assert_array_equal(rank, rank_rule(ref, p_out_of(name)))
    ref64 = np.linalg.eigvalsh(G64)
    cond64 = ref64[:, -1] / ref64[:, 0]
    if name in WELL_CONDITIONED:
        assert cond64.max() <= 1e3
        assert np.all(rank == d) and np.all(np.isfinite(logvol))
        cond = ref[:, -1] / ref[:, 0]
        d_own = np.abs(logvol - 0.5 * np.sum(np.log(ref), axis=1))
        gate_own = d * 64 * d * DBL_EPS * cond
        d_64 = np.abs(logvol - 0.5 * np.linalg.slogdet(G64)[1])
        gate_64 = d * cond64 * (4 * e_torch + 1e-7)
        print(f"{name}: logvol vs own spectrum {np.max(d_own / gate_own):.3e} of the gate, vs slogdet(G64) "
              f"{np.max(d_64 / gate_64):.3e} of the gate (max |delta| {d_64.max():.3e})")
        assert np.all(d_own <= gate_own)
        assert np.all(d_64 <= gate_64)
    else:                                   # nearly singular: logvol is finite exactly where every eigenvalue is positive
        print(f"{name}: cond(G64) up to {cond64.max():.3e}, rank min {rank.min()}")
        positive = np.all(eig > 0, axis=1)
        assert np.all(np.isfinite(logvol[positive])) and np.all(np.isneginf(logvol[~positive]))
        assert np.all(positive[rank == d])


def test_spectrum_off_and_grid_input():
    from vqvae_amd.geo import pullback_metric_device
    dec = make_decoder("fm_batch")[0].to(_dev())
    z4 = torch.from_numpy(np.random.RandomState(5).randn(2, 16, 3, 4).astype(np.float32)).to(_dev())
    grid = pullback_metric_device(dec, z4)
    flat = pullback_metric_device(dec, z4.permute(0, 2, 3, 1).reshape(-1, 16).contiguous())
    assert grid.route == "native" and grid.G.shape == (2, 3, 4, 16, 16) and grid.eig.shape == (2, 3, 4, 16)
    assert grid.logvol.shape == (2, 3, 4) and grid.rank.shape == (2, 3, 4)
    for a, b in ((grid.G, flat.G), (grid.eig, flat.eig), (grid.logvol, flat.logvol), (grid.rank, flat.rank)):
        assert a.reshape(b.shape).cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    bare = pullback_metric_device(dec, z4, spectrum=False)
    assert bare.eig is None and bare.logvol is None and bare.rank is None
    assert bare.G.cpu().numpy().tobytes() == grid.G.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ 3. exact properties
@pytest.mark.parametrize("name", ["fm_batch", "cf_batch", "fm_group", "fm_none5"])
def test_exact_properties(name):
    from vqvae_amd import _lib
    lib = _lib.load()
    ex = _export(name)
    d = CASES[name][1]
    z65 = torch.from_numpy(make_latents(name, 65, salt=3)).to(_dev())
    full = _raw_call(ex, z65)
    assert full[0] == 0, lib.geo_last_error()
    G = full[1]
    assert G.transpose(0, 2, 1).tobytes() == G.tobytes()                          # G[a][b] and G[b][a]: the same bits
    assert not np.isnan(G).any() and not np.isnan(full[2]).any() and not np.isnan(full[3]).any() and np.all(full[4] >= 0)
    for n in (1, 2, 3, 31, 32, 33, 65):
        perm = np.random.RandomState(n).permutation(n)
        plain = _raw_call(ex, z65[:n].contiguous())
        shuffled = _raw_call(ex, z65[:n][torch.from_numpy(perm).to(_dev())].contiguous())
        assert plain[0] == 0 and shuffled[0] == 0, lib.geo_last_error()
        _same_bits(shuffled, (0,) + tuple(t[perm] for t in plain[1:]))
        _same_bits(plain, (0,) + tuple(t[:n] for t in full[1:]))                  # nor on n or the position
    ws_min = lib.geo_metric_tensor_min_workspace_bytes(ex.desc)
    assert 0 < ws_min < lib.geo_metric_tensor_workspace_bytes(ex.desc, 65)
    for n in (33, 65):                                                            # slices of 32: 32 + 1, 32 + 32 + 1
        sliced = _raw_call(ex, z65[:n].contiguous(), ws_bytes=ws_min)
        assert sliced[0] == 0, lib.geo_last_error()
        _same_bits(sliced, (0,) + tuple(t[:n] for t in full[1:]))
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        _same_bits(_raw_call(ex, z65), full)
    _same_bits(_raw_call(ex, z65, fill=0xFF), full)
    _same_bits(_raw_call(ex, z65, ws_bytes=ws_min, fill=0xFF), full)
    _same_bits(_raw_call(ex, z65), _raw_call(ex, z65))
    no_spec = _raw_call(ex, z65, spectrum=False)
    assert no_spec[0] == 0 and no_spec[1].tobytes() == G.tobytes()


@pytest.mark.parametrize("name", ["fm_batch", "cf_batch"])
def test_zeroed_latent_dimension_and_equal_latents(name):
    k = 6

    def zero_column(dec):
        with torch.no_grad():
            dec.conv_in.weight[:, k] = 0.0

    d = CASES[name][1]
    z = torch.from_numpy(make_latents(name, 40, salt=4)).to(_dev())
    status, G, eig, logvol, rank = _raw_call(_export(name, zero_column), z)
    assert status == 0
    assert np.all(G[:, k, :] == 0.0) and np.all(G[:, :, k] == 0.0)
    assert np.all(rank <= d - 1) and np.all(np.isneginf(logvol))
    assert not np.isnan(eig).any()
    same = _raw_call(_export(name), z[7:8].repeat(40, 1).contiguous())
    assert same[0] == 0
    for t in same[1:]:
        assert all(t[i].tobytes() == t[0].tobytes() for i in range(40))


# ------------------------------------------------------------------------------------------------ 4. the edge lengths
@pytest.mark.parametrize("name", ["cf_batch", "fm_none5"])
def test_consistent_with_edge_lengths(name):
    """The two well-conditioned shapes only: the quadratic form dz^T G dz squares J's condition number into the rounding error
    (why the edge-length route keeps the columns), so the nearly singular shapes are left out on purpose."""
    from oracle import metric as om
    from vqvae_amd.geo import pullback_metric_device
    TOL = 1e-5                                                                    # the gate of tests/test_gpu_metric.py
    norm, d, cout, px, channels, seed = CASES[name]
    dec, sd = make_decoder(name)
    z = make_latents(name, 300, salt=5)
    r = np.random.RandomState(seed)
    src, dst = r.randint(0, 300, 2000), r.randint(0, 300, 2000)
    res = pullback_metric_device(dec.to(_dev()), torch.from_numpy(z).to(_dev()), spectrum=False)
    assert res.route == "native"
    G = res.G.cpu().numpy()
    dz = z[dst].astype(np.float64) - z[src].astype(np.float64)
    quad = lambda nodes: np.sqrt(np.einsum("ea,eab,eb->e", dz, G[nodes], dz))      # noqa: E731
    got = 0.5 * (quad(src) + quad(dst))
    ref = om.edge_lengths(sd, norm, px, z[src], z[dst], batch_size=512, training=False, dtype=torch.float64).numpy()
    keep = ref > 0                                                                # (src == dst draws have length 0)
    rel = np.abs(got[keep] - ref[keep]) / ref[keep]
    print(f"{name}: {np.mean(rel <= TOL):.4%} of {keep.sum()} edges within {TOL}, max rel {rel.max():.3e}")
    assert np.all(got[~keep] == 0.0)
    assert np.mean(rel <= TOL) >= 0.999


# ------------------------------------------------------------------------------------------------ 5. several passes
def _chunked(ex, z, chunk):
    parts = [_raw_call(ex, z[lo:lo + chunk].contiguous()) for lo in range(0, z.shape[0], chunk)]
    assert all(p[0] == 0 for p in parts)
    return (0,) + tuple(np.concatenate([p[i] for p in parts]) for i in range(1, 5))


def _spot_check(name, z, G, n_spots=64):
    spots = np.random.RandomState(9).choice(z.shape[0], n_spots, replace=False)
    dec = make_decoder(name)[0]
    G64 = gram64_of(dec, z[spots].cpu().numpy())
    e = normalised_error(G[spots], G64)
    e_torch = normalised_error(_torch_gram(dec.to(_dev()), z[torch.from_numpy(spots).to(_dev())]), G64)
    print(f"{name}: {n_spots} spot latents, e = {e:.3e}, e_torch = {e_torch:.3e}, ratio = {e / e_torch:.2f}")
    assert e <= 4 * e_torch + 1e-7


def test_more_than_one_pass_of_slots():
    """70 001 latents x 16 unit tangents: more than one pass of 2^20 tangent slots, and an odd count."""
    from vqvae_amd import _lib
    name, n = "fm_batch", 70001
    ex = _export(name)
    z = torch.from_numpy(make_latents(name, n, salt=6)).to(_dev())
    whole = _raw_call(ex, z)
    assert whole[0] == 0, _lib.load().geo_last_error()
    _same_bits(whole, _chunked(ex, z, 4096))
    _spot_check(name, z, whole[1])


def test_32px_head_in_three_or_more_slices():
    from vqvae_amd import _lib
    lib = _lib.load()
    name, n = "cf_batch", 200
    ex = _export(name)
    z = torch.from_numpy(make_latents(name, n, salt=7)).to(_dev())
    ws_small = lib.geo_metric_tensor_workspace_bytes(ex.desc, 64)                 # room for 64 latents: 4 slices
    assert lib.geo_metric_tensor_min_workspace_bytes(ex.desc) <= ws_small < lib.geo_metric_tensor_workspace_bytes(ex.desc, 96)
    sliced = _raw_call(ex, z, ws_bytes=ws_small)
    assert sliced[0] == 0, lib.geo_last_error()
    _same_bits(sliced, _chunked(ex, z, 4096))
    _spot_check(name, z, sliced[1])


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_without_a_launch():
    from vqvae_amd import _lib
    from vqvae_amd.spatial_decoder import DecoderExport, SpatialDecoder
    lib = _lib.load()
    dev = _dev()
    train = DecoderExport(make_decoder("fm_batch", training=True)[0].to(dev), dev)
    wide = DecoderExport(SpatialDecoder(1, (256, 128, 64), 32, 28, "none").eval().to(dev), dev)
    for ex, d, word in ((train, 16, "BatchNorm"), (wide, 32, "latent_dim")):
        assert lib.geo_metric_tensor_workspace_bytes(ex.desc, 100) == 0
        assert lib.geo_metric_tensor_min_workspace_bytes(ex.desc) == 0
        z = torch.zeros(4, d, device=dev)
        status, G, *_ = _raw_call(ex, z, ws_bytes=1 << 20)
        assert status == GEO_E_ARG and word in lib.geo_last_error().decode()
        assert np.isnan(G).all()                                                  # nothing was written
    ok = _export("fm_batch")
    ws_min = lib.geo_metric_tensor_min_workspace_bytes(ok.desc)
    status, G, *_ = _raw_call(ok, torch.zeros(64, 16, device=dev), ws_bytes=ws_min - 256)
    assert status == GEO_E_ARG and "workspace" in lib.geo_last_error().decode()
    assert np.isnan(G).all()
    assert lib.geo_decoder_metric_tensor(ok.desc, None, 0, None, None, None, None, None, 0, None) == 0      # n == 0
    assert lib.geo_decoder_metric_tensor(ok.desc, None, 4, None, None, None, None, None, 0, None) == GEO_E_ARG


def test_option_that_switches_the_pass_off_refuses():
    """jvp_per_node = 0 takes away the per-latent primal pass: the call refuses instead of changing route; jvp_node_jacobian = 0
    does not concern it."""
    from vqvae_amd import _lib
    lib = _lib.load()
    ex = _export("fm_batch")
    z = torch.from_numpy(make_latents("fm_batch", 5)).to(_dev())
    base = _raw_call(ex, z)
    try:
        assert lib.geo_set_option(b"jvp_node_jacobian", 0) == 0
        _same_bits(_raw_call(ex, z), base)
        assert lib.geo_set_option(b"jvp_node_jacobian", 1) == 0
        assert lib.geo_set_option(b"jvp_per_node", 0) == 0
        assert lib.geo_metric_tensor_workspace_bytes(ex.desc, 5) == 0
        status, G, *_ = _raw_call(ex, z, ws_bytes=1 << 20)
        assert status == GEO_E_ARG and "jvp_per_node" in lib.geo_last_error().decode() and np.isnan(G).all()
    finally:
        lib.geo_set_option(b"jvp_node_jacobian", 1)
        lib.geo_set_option(b"jvp_per_node", 1)


def test_python_call_on_wide_latent_takes_autograd_route():
    from vqvae_amd.geo import native_metric_covers, pullback_metric_device
    from vqvae_amd.spatial_decoder import SpatialDecoder
    torch.manual_seed(11)
    dec = SpatialDecoder(1, (256, 128, 64), 32, 28, "batch").eval()
    assert not native_metric_covers(dec)
    z = np.random.RandomState(12).randn(N_LATENTS, 32).astype(np.float32)
    G64 = gram64_of(dec, z)
    dec = dec.to(_dev())
    zg = torch.from_numpy(z).to(_dev())
    res = pullback_metric_device(dec, zg)
    assert res.route == "autograd" and res.G.is_cuda and res.G.shape == (N_LATENTS, 32, 32)
    e, e_torch = normalised_error(res.G.cpu().numpy(), G64), normalised_error(_torch_gram(dec, zg), G64)
    print(f"d = 32 (autograd route): e = {e:.3e}, e_torch = {e_torch:.3e}")
    assert e <= 4 * e_torch + 1e-7
    with pytest.raises(ValueError, match="BatchNorm"):
        pullback_metric_device(dec.train(), zg)
