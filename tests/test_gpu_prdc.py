"""geo_kth_radius / geo_ball_count (csrc/prdc.hip) and prdc_device on the GPU:
  (a) every case of prdc_cases.py against the numpy fp64 oracle: counts, nearest indices and the four figures exact, radii
      and nearest keys within 1e-12 relative (bit-equal on the integer grids, which are full of key == radius ties);
  (b) for d <= 128 the radii and nearest pairs are geo_knn_query's form 0 results, bit for bit;
  (c) bit-for-bit invariance: workspace size, stream, the batch a query is in, corpus order, the corpus split;
  (d) workspace honesty: exactly the queried size, 0xFF-filled, guard bytes behind it, then once more on the stale scratch;
  (e) refusals before any launch leave the outputs alone; m = 0; NULL outputs one at a time."""
import numpy as np
import pytest
import torch

import prdc_cases as pc
from conftest import clustered_latents

pytestmark = pytest.mark.gpu

GEO_E_ARG, GEO_E_WORKSPACE = -1, -2
GUARD = 4096


def _dev(a):
    from vqvae_amd._device import device
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(device())


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _with_split(S, fn):
    from vqvae_amd import _lib
    lib = _lib.load()
    _lib.check(lib.geo_set_option(b"prdc_split", int(S)), "geo_set_option")
    try:
        return fn()
    finally:
        lib.geo_set_option(b"prdc_split", -1)


def _all(real, fake, k, cap=None):
    """The four passes of prdc_device as device tensors: (r2_R, r2_F, cF, cR, near_key, near_idx)."""
    from vqvae_amd.eval.prdc import ball_count_device, kth_radius_device
    r2_R, r2_F = kth_radius_device(real, k, cap), kth_radius_device(fake, k, cap)
    cF = ball_count_device(real, r2_R, fake, cap)[0]
    return (r2_R, r2_F, cF) + tuple(ball_count_device(fake, r2_F, real, cap))


# ---------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("case_id", pc.CASE_IDS)
def test_every_case_equals_the_oracle(case_id):
    from vqvae_amd.eval.prdc import FIGURES, prdc_device
    pc.assert_margin(case_id)
    real, fake, k, exact = pc.inputs(case_id)
    o = pc.oracle(case_id)
    got = prdc_device(_dev(real), _dev(fake), k)
    assert got["route"] == "hip"
    for name in ("fake_count", "real_count", "real_near_idx"):
        assert got[name].dtype == torch.int32
        np.testing.assert_array_equal(got[name].cpu().numpy(), o[name], err_msg=name)
    for name in ("real_radius2", "fake_radius2", "real_near_key"):
        g = got[name].cpu().numpy()
        assert g.dtype == np.float64
        rel = np.abs(g - o[name]) / np.maximum(np.abs(o[name]), np.finfo(np.float64).tiny)
        print(f"{case_id} {name}: max rel {rel.max():.3e}")
        if exact:
            np.testing.assert_array_equal(g.view(np.int64), o[name].view(np.int64), err_msg=name)
        else:
            assert rel.max() <= 1e-12, (name, rel.max())
    for name in FIGURES:
        assert got[name] == o[name], (name, got[name], o[name])


# ---------------------------------------------------------------------------------------------------- (b)
def _narrow_inputs():
    for case_id in pc.CASE_IDS:
        real, fake, k, _ = pc.inputs(case_id)
        if real.shape[1] <= 128:                    # k + 1 <= n everywhere: gauss-2x2x1-k1 asks the search for both rows
            yield case_id, real, fake, k
    c = clustered_latents(700, 16, 5)
    c[100:140] = c[:40]                             # duplicates: neighbours at key 0
    c[300:310] = c[0]
    yield "clustered", c[:400].copy(), c[300:].copy(), 5


@pytest.mark.parametrize("name,real,fake,k", [pytest.param(*c, id=c[0]) for c in _narrow_inputs()])
def test_narrow_widths_equal_the_knn_query(name, real, fake, k):
    from vqvae_amd.eval.prdc import ball_count_device, kth_radius_device
    from vqvae_amd.geo.knn_graph_optimized import knn_query_device
    R, F = _dev(real), _dev(fake)
    for a in (R, F):
        ref = knn_query_device(a, a, k + 1, form=0)[1][:, k].contiguous()
        assert _same([kth_radius_device(a, k)], [ref])
    r2_F = kth_radius_device(F, k)
    _, near_key, near_idx = ball_count_device(F, r2_F, R)
    idx, d2 = knn_query_device(F, R, 1, form=0)
    assert _same([near_key, near_idx], [d2[:, 0].contiguous(), idx[:, 0].contiguous()])


# ---------------------------------------------------------------------------------------------------- (c)
INVARIANCE = ["gauss-300x257x129-k5", "gauss-200x129x16-k64", "grid-193x200x5-k3-hi3"]


@pytest.mark.parametrize("case_id", INVARIANCE)
def test_workspace_stream_and_split_do_not_change_a_bit(case_id):
    from vqvae_amd import _lib
    lib = _lib.load()
    real, fake, k, _ = pc.inputs(case_id)
    R, F = _dev(real), _dev(fake)
    d = R.shape[1]
    ref = _all(R, F, k)
    lo = lib.geo_prdc_min_workspace_bytes(d)
    full = lib.geo_prdc_workspace_bytes(len(real), len(real), d)
    assert 0 < lo <= full
    for cap in (lo, (lo + full) // 2, 3 * lo):
        assert _same(_all(R, F, k, cap), ref), f"workspace cap {cap}"
    for S in (1, 2, 3, 32):                                                 # the corpus split, forced both ways
        assert _same(_with_split(S, lambda: _all(R, F, k)), ref), f"split {S}"
        assert _same(_with_split(S, lambda: _all(R, F, k, lo)), ref), f"split {S} in the minimum workspace"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _all(R, F, k)
    side.synchronize()
    assert _same(other, ref), "second stream"


def test_a_query_alone_equals_the_query_in_a_batch():
    from vqvae_amd.eval.prdc import ball_count_device, kth_radius_device
    real, fake, k, _ = pc.inputs("gauss-300x257x129-k5")
    R, F = _dev(real), _dev(fake)
    r2 = kth_radius_device(R, k)
    ref = ball_count_device(R, r2, F)
    for j in (0, 63, 64, 256):
        one = ball_count_device(R, r2, F[j:j + 1].clone())
        assert _same(one, [t[j:j + 1] for t in ref]), j


def test_corpus_permutation_maps_the_nearest_index():
    from vqvae_amd.eval.prdc import ball_count_device, kth_radius_device
    case_id = "gauss-300x257x129-k5"
    pc.assert_margin(case_id)                                              # tie-free: the nearest row is unique
    real, fake, k, _ = pc.inputs(case_id)
    R, F = _dev(real), _dev(fake)
    r2 = kth_radius_device(R, k)
    ref = ball_count_device(R, r2, F)
    perm = torch.from_numpy(np.random.RandomState(3).permutation(len(real))).to(R.device)
    got = ball_count_device(R[perm].contiguous(), r2[perm].contiguous(), F)
    assert _same(got[:2], ref[:2])
    assert torch.equal(perm[got[2].long()], ref[2].long())
    assert _same([kth_radius_device(R[perm].contiguous(), k)], [r2[perm].contiguous()])


# ---------------------------------------------------------------------------------------------------- (d), (e): raw calls
def _raw(real, fake, k, ws, ws_bytes, which, outs=None, nulls=()):
    """One raw entry-point call on the current stream; returns (status, outputs)."""
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    lib = _lib.load()
    n, d = real.shape
    if which == "radius":
        out = outs or [torch.empty(n, dtype=torch.float64, device=real.device)]
        rc = lib.geo_kth_radius(ptr(real), n, d, k, ptr(out[0]), ws, ws_bytes, stream_ptr())
        return rc, out
    m = fake.shape[0]
    out = outs or [torch.empty(m, dtype=torch.int32, device=real.device), torch.empty(m, dtype=torch.float64, device=real.device),
                   torch.empty(m, dtype=torch.int32, device=real.device)]
    r2 = torch.full((n,), 1.5 * d, dtype=torch.float64, device=real.device)
    p = [None if i in nulls else ptr(t) for i, t in enumerate(out)]
    rc = lib.geo_ball_count(ptr(real), ptr(r2), n, ptr(fake) if m else None, m, d, p[0], p[1], p[2], ws, ws_bytes, stream_ptr())
    return rc, out


@pytest.mark.parametrize("which", ["radius", "count"])
@pytest.mark.parametrize("split", [-1, 3])
def test_queried_workspace_guarded_then_stale(which, split):
    from vqvae_amd import _lib
    lib = _lib.load()
    real, fake, k, _ = pc.inputs("gauss-300x257x129-k5")
    R, F = _dev(real), _dev(fake)

    def go():
        need = lib.geo_prdc_workspace_bytes(len(real), len(real) if which == "radius" else len(fake), R.shape[1])
        buf = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=R.device)
        runs = []
        for _ in range(2):                                                 # fresh 0xFF scratch, then the scratch it left
            rc, out = _raw(R, F, k, buf.data_ptr(), need, which)
            assert rc == 0, lib.geo_last_error().decode()
            torch.cuda.synchronize()
            assert bool((buf[need:] == 0xFF).all()), "guard bytes behind the workspace changed"
            runs.append(out)
        assert _same(runs[0], runs[1])
        return runs[0]

    got = _with_split(split, go)
    ws = torch.empty(lib.geo_prdc_workspace_bytes(len(real), len(real), R.shape[1]) + 256, dtype=torch.uint8, device=R.device)
    ref = _raw(R, F, k, ws.data_ptr(), ws.numel(), which)[1]
    assert _same(got, ref)


def test_refusals_write_nothing_and_empty_calls_pass():
    from vqvae_amd import _lib
    lib = _lib.load()
    real, fake, k, _ = pc.inputs("gauss-65x63x3-k5")
    R, F = _dev(real), _dev(fake)
    lo = lib.geo_prdc_min_workspace_bytes(3)
    ws = torch.zeros(lo + 256, dtype=torch.uint8, device=R.device)

    def sentinels(which):
        rows = len(real) if which == "radius" else len(fake)
        if which == "radius":
            return [torch.full((rows,), -7.0, dtype=torch.float64, device=R.device)]
        return [torch.full((rows,), -7, dtype=torch.int32, device=R.device), torch.full((rows,), -7.0, dtype=torch.float64, device=R.device),
                torch.full((rows,), -7, dtype=torch.int32, device=R.device)]

    def untouched(out):
        torch.cuda.synchronize()
        return all(bool((t == -7).all()) for t in out) and bool((ws == 0).all())

    for which in ("radius", "count"):
        out = sentinels(which)
        assert _raw(R, F, k, ws.data_ptr(), lo - 1, which, out)[0] == GEO_E_WORKSPACE and untouched(out)
        assert _raw(R, F, k, None, lo, which, out)[0] == GEO_E_ARG and untouched(out)
    out = sentinels("radius")
    for bad_k in (0, 65, len(real)):
        assert _raw(R, F, bad_k, ws.data_ptr(), lo, "radius", out)[0] == GEO_E_ARG and untouched(out)
    wide = torch.zeros((4, 1025), dtype=torch.float32, device=R.device)
    assert _raw(wide, wide, 1, ws.data_ptr(), lo, "radius", out)[0] == GEO_E_ARG and untouched(out)
    assert _raw(wide, wide, 1, ws.data_ptr(), lo, "count", sentinels("count"))[0] == GEO_E_ARG
    assert lib.geo_prdc_workspace_bytes(4, 4, 1025) == 0 and lib.geo_prdc_min_workspace_bytes(0) == 0
    # m = 0: GEO_OK without a launch, even with a null query pointer
    assert _raw(R, F[:0], k, ws.data_ptr(), lo, "count")[0] == 0
    assert _raw(R, F[:0], k, ws.data_ptr(), lo - 1, "count")[0] == 0          # and whatever the workspace: it is not looked at
    # NULL outputs, one at a time: the others are what a full call writes
    full = _raw(R, F, k, ws.data_ptr(), lo, "count")[1]
    for skip in range(3):
        out = sentinels("count")
        assert _raw(R, F, k, ws.data_ptr(), lo, "count", out, nulls=(skip,))[0] == 0
        torch.cuda.synchronize()
        for i in range(3):
            assert bool((out[i] == -7).all()) if i == skip else torch.equal(_bits(out[i]), _bits(full[i])), (skip, i)
