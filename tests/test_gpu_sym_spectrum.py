"""geo_sym_spectrum (csrc/sym_spectrum.hip) on the GPU, on matrices built for the purpose: eigenvalues
against numpy.linalg.eigvalsh, the rank and logvol rules, what must not be read, bit equality under everything a matrix's
results must not depend on, NaN and inf matrices, the refusals, and the sweep counts against the cap."""
import numpy as np
import pytest
import torch

import vanilla_metric_cases as M
from metric_tensor_cases import rank_rule

pytestmark = pytest.mark.gpu
GEO_E_ARG = -1
P_OUT = M.SPECTRUM_P_OUT


def _dev():
    return torch.device("cuda", 0)


def _raw(G: np.ndarray, p_out=P_OUT, sweeps=False):
    """geo_sym_spectrum(_sweeps) on G [n, d, d]: (eig, logvol, rank[, sweeps]) as numpy arrays, outputs pre-filled."""
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    lib = _lib.load()
    dev = _dev()
    g = torch.from_numpy(np.ascontiguousarray(G)).to(dev)
    n, d = g.shape[0], g.shape[1]
    eig = torch.full((n, d), 7.0, dtype=torch.float64, device=dev)
    logvol = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    rank = torch.full((n,), -7, dtype=torch.int32, device=dev)
    sw = torch.full((n,), -7, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        if sweeps:
            status = lib.geo_sym_spectrum_sweeps(ptr(g), n, d, p_out, ptr(eig), ptr(logvol), ptr(rank), ptr(sw), stream_ptr())
        else:
            status = lib.geo_sym_spectrum(ptr(g), n, d, p_out, ptr(eig), ptr(logvol), ptr(rank), stream_ptr())
        torch.cuda.current_stream().synchronize()
    assert status == 0, lib.geo_last_error()
    out = tuple(t.cpu().numpy() for t in (eig, logvol, rank))
    return out + (sw.cpu().numpy(),) if sweeps else out


@pytest.mark.parametrize("d", M.SPECTRUM_DIMS)
def test_spectra_against_numpy(d):
    """Every kind of matrix at once (65 matrices: n straddles the four matrices per workgroup of the small instantiations),
    the lower triangles overwritten with garbage."""
    kinds = [M.SPECTRA[i % len(M.SPECTRA)] for i in range(65)]
    mats = np.stack([M.matrix(k, d, seed=i) for i, k in enumerate(kinds)])
    ref = np.linalg.eigvalsh(mats)
    garbage = mats.copy()
    low = np.tril_indices(d, -1)
    garbage[:, low[0], low[1]] = np.random.RandomState(d).randn(65, len(low[0])) * 1e6
    garbage[::5, low[0], low[1]] = np.nan
    eig, logvol, rank, sweeps = _raw(garbage, sweeps=True)
    assert np.all(np.diff(eig, axis=1) >= 0) and not np.isnan(eig).any() and not np.isnan(logvol).any()
    emax = np.maximum(ref[:, -1:], np.finfo(np.float64).tiny)
    err = np.abs(eig - ref) / (64 * d * M.DBL_EPS * emax)
    print(f"d = {d}: max |eig - eigvalsh| / (64 d eps eig_max) = {err.max():.3e}; sweeps max {sweeps.max()} "
          f"(per kind: {({k: int(sweeps[[i for i, kk in enumerate(kinds) if kk == k]].max()) for k in M.SPECTRA})})")
    assert err.max() <= 1.0
    for i, k in enumerate(kinds):
        if k == "diagonal":                                  # nothing to rotate: the entries come back exactly, sorted
            assert np.array_equal(eig[i], np.sort(np.diag(mats[i]))) and sweeps[i] == 0
        if k == "zero":
            assert np.all(eig[i] == 0.0) and rank[i] == 0 and np.isneginf(logvol[i]) and sweeps[i] == 0
    # the rank: no eigenvalue of a matrix that enters within a factor 4 of the threshold (asserted first); the geometric
    # spectrum's own values are used for it, rank 1's and zero's are known
    for i, k in enumerate(kinds):
        if k in ("rank1", "zero"):
            assert rank[i] == (1 if k == "rank1" else 0)
            continue
        truth = np.sort(M.spectrum_values(k, d)) if M.spectrum_values(k, d) is not None else ref[i]
        thr = (max(P_OUT, d) * M.FLT_EPS) ** 2 * truth[-1]
        assert not np.any((truth > thr / 4) & (truth < thr * 4)), (k, d)
        assert rank[i] == rank_rule(truth, P_OUT), (k, d)
    # logvol where cond <= 1e3: equal, cluster, diagonal, blocks
    for i, k in enumerate(kinds):
        if k in ("equal", "cluster", "diagonal", "blocks"):
            cond = ref[i, -1] / ref[i, 0]
            assert cond <= 1e3
            assert abs(logvol[i] - 0.5 * np.linalg.slogdet(mats[i])[1]) <= d * 64 * d * M.DBL_EPS * cond, (k, d)
    assert sweeps.max() < _cap()


def _cap():
    from vqvae_amd import _lib
    return int(_lib.load().geo_sym_spectrum_sweep_cap())


@pytest.mark.parametrize("d", (3, 16, 17, 64, 65, 128))
def test_results_do_not_depend_on_the_batch(d):
    """Bit for bit: alone, in batches of 1, 2, 3 and 65, at any position, on a side stream, with NaN neighbours."""
    kinds = [M.SPECTRA[i % 4] for i in range(65)]
    mats = np.stack([M.matrix(k, d, seed=100 + i) for i, k in enumerate(kinds)])
    full = _raw(mats)
    assert not np.isnan(full[0]).any()
    for n in (1, 2, 3):
        for part, whole in zip(_raw(mats[:n]), full):
            assert part.tobytes() == whole[:n].tobytes()
    perm = np.random.RandomState(d).permutation(65)
    for a, b in zip(_raw(mats[perm]), full):
        assert a.tobytes() == b[perm].tobytes()
    for i in (0, 7, 64):
        for a, b in zip(_raw(mats[i:i + 1]), full):
            assert a.tobytes() == b[i:i + 1].tobytes()
    with torch.cuda.stream(torch.cuda.Stream(device=_dev())):
        for a, b in zip(_raw(mats), full):
            assert a.tobytes() == b.tobytes()
    poisoned = mats.copy()
    bad = np.arange(65) % 3 != 1
    poisoned[bad, 0, d - 1] = np.nan
    poisoned[bad & (np.arange(65) % 2 == 0), 0, 0] = np.inf
    eig, logvol, rank = _raw(poisoned)
    assert np.isnan(eig[bad]).all() and np.isnan(logvol[bad]).all() and np.all(rank[bad] == 0)
    for got, whole in zip((eig, logvol, rank), full):
        assert got[~bad].tobytes() == whole[~bad].tobytes()


@pytest.mark.parametrize("d", (1, 2, 33, 128))
def test_nan_and_inf_matrices_return(d):
    mats = np.stack([M.matrix("cluster", d)] * 4)
    mats[0, 0, 0] = np.nan
    mats[1, 0, d - 1] = np.inf
    mats[2, d - 1, d - 1] = -np.inf
    eig, logvol, rank, sweeps = _raw(mats, sweeps=True)
    assert np.isnan(eig[:3]).all() and np.isnan(logvol[:3]).all() and np.all(rank[:3] == 0) and np.all(sweeps[:3] == 0)
    assert not np.isnan(eig[3]).any() and rank[3] == d
    if d > 1:                                               # a NaN below the diagonal is not read
        low = M.matrix("cluster", d)
        low[d - 1, 0] = np.nan
        assert _raw(low[None])[0].tobytes() == eig[3:4].tobytes()


def test_overflow_inside_the_iteration_gives_nan():
    """Finite entries near DBL_MAX whose first rotation overflows: the call returns, that matrix is NaN / NaN / 0, its neighbour's
    bits are what they are alone."""
    mats = np.stack([np.full((2, 2), 1e308), M.matrix("cluster", 2)])
    eig, logvol, rank = _raw(mats)
    assert np.isnan(eig[0]).all() and np.isnan(logvol[0]) and rank[0] == 0
    for got, alone in zip((eig, logvol, rank), _raw(mats[1:])):
        assert got[1:].tobytes() == alone.tobytes()


def test_refusals_without_a_launch():
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr
    lib = _lib.load()
    g = torch.zeros(2, 4, 4, dtype=torch.float64, device=_dev())
    eig = torch.full((2, 4), 7.0, dtype=torch.float64, device=_dev())
    lv = torch.full((2,), 7.0, dtype=torch.float64, device=_dev())
    rk = torch.full((2,), -7, dtype=torch.int32, device=_dev())
    call = lib.geo_sym_spectrum
    for d in (0, 129, -1):
        assert call(ptr(g), 2, d, 16, ptr(eig), ptr(lv), ptr(rk), None) == GEO_E_ARG
    assert call(ptr(g), -1, 4, 16, ptr(eig), ptr(lv), ptr(rk), None) == GEO_E_ARG
    assert call(ptr(g), 2, 4, 0, ptr(eig), ptr(lv), ptr(rk), None) == GEO_E_ARG
    for args in ((None, ptr(eig), ptr(lv), ptr(rk)), (ptr(g), None, ptr(lv), ptr(rk)), (ptr(g), ptr(eig), None, ptr(rk)),
                 (ptr(g), ptr(eig), ptr(lv), None)):
        assert call(args[0], 2, 4, 16, args[1], args[2], args[3], None) == GEO_E_ARG
    assert call(None, 0, 4, 16, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert torch.all(eig == 7.0) and torch.all(lv == 7.0) and torch.all(rk == -7)


def test_python_wrapper():
    from vqvae_amd.geo import sym_spectrum_device
    mats = np.stack([M.matrix("cluster", 17, seed=i) for i in range(5)])
    eig, logvol, rank = sym_spectrum_device(torch.from_numpy(mats).to(_dev()), 784)
    raw = _raw(mats, p_out=784)
    assert eig.cpu().numpy().tobytes() == raw[0].tobytes() and logvol.cpu().numpy().tobytes() == raw[1].tobytes()
    assert rank.dtype == torch.int32 and rank.cpu().numpy().tobytes() == raw[2].tobytes()
    with pytest.raises(ValueError):
        sym_spectrum_device(torch.zeros(2, 3, 4, dtype=torch.float64, device=_dev()), 16)
    with pytest.raises(ValueError):
        sym_spectrum_device(torch.zeros(2, 3, 3, device=_dev()), 16)
