"""The spatial decoder's pull-back lengths (csrc/jvp.hip) at the corners of the envelope spatial_decoder.hip_kernels_cover admits
that the other suites do not run: dec_channels[1] = 32, dec_channels[2] = 16 and 128, a dec_channels[0] that is no multiple of 8,
heads of 2 and 4 channels, GroupNorm at dec_channels[1] = 64 and 32, the edges of the latent width (1, 2, 3, 17, 33, 63),
BatchNorm2d(affine=False) and BatchNorm2d(track_running_stats=False) -- jvp_envelope_cases.CASES, each in each of its modes at
batch sizes 512 and 100.  The reference is the package's own autograd route in fp64 on the CPU (computed once per case, mode
and batch size); the gate is the one of test_gpu_metric.py.  Every test asserts the route geo_jvp_plan names for the call it
makes and prints the fraction within 1e-5, the 0.99-quantile and the maximum; DESIGN.md section 2 records them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_envelope_cases as C  # noqa: E402
from ws_guard import GUARD, GUARD_BYTE, GuardedWorkspace  # noqa: E402

pytestmark = pytest.mark.gpu

RUNS = [(name, training, bs) for name, case in C.CASES.items() for training in case.modes for bs in C.BATCH_SIZES]
RUN_IDS = [f"{name}-{'train' if training else 'eval'}-bs{bs}" for name, training, bs in RUNS]


def dev():
    return torch.device("cuda", 0)


def _module(name, training):
    return C.build(name).train(training).to(dev())


def _forbid_autograd(monkeypatch):
    from vqvae_amd.geo import riemannian_metric

    def boom(*a, **k):
        raise AssertionError("autograd route taken")
    monkeypatch.setattr(riemannian_metric, "_generic_jvp_norms", boom)


def _state(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


def _check_state(name, training, module, before, want_stats, what):
    """Train-mode BatchNorm with tracked statistics: running_mean / running_var within the bound of
    test_train_mode_jvp_updates_batchnorm_running_statistics of the fp64 reference module's, num_batches_tracked equal.
    Untracked: still no statistics.  Everything else, and every other entry: untouched."""
    case = C.CASES[name]
    after = module.state_dict()
    assert sorted(after) == sorted(before)
    tracked = training and case.norm in ("batch", "batch-plain")
    if case.norm == "batch-untracked":
        assert not any(k.endswith(C.RUNNING_KEYS) for k in after)
        assert all(getattr(module.deconv_layers[i], "running_mean") is None for i in (1, 4))
    assert sorted(want_stats) == sorted(k for k in after if k.endswith(C.RUNNING_KEYS))
    for k, v in after.items():
        if tracked and k.endswith(("running_mean", "running_var")):
            assert not torch.equal(v, before[k]), (what, k)
            np.testing.assert_allclose(v.cpu().numpy(), want_stats[k], rtol=2e-5, atol=1e-6, err_msg=f"{what}: {k}")
        elif tracked and k.endswith("num_batches_tracked"):
            assert int(v) == int(want_stats[k]) > 0, (what, k, int(v), int(want_stats[k]))
        else:
            assert torch.equal(v, before[k]), (what, k)


@pytest.mark.parametrize("name,training,bs", RUNS, ids=RUN_IDS)
def test_pairs_entry_against_fp64(name, training, bs, monkeypatch):
    """geo_jvp_plan names the case's route; edge_lengths_device on the 2 048 pairs passes the gate against the fp64 autograd
    reference; the running statistics are the reference module's; edge_lengths_riemannian on the module gives the same bits
    without the autograd route."""
    from vqvae_amd import _lib
    from vqvae_amd.geo.riemannian_metric import edge_lengths_device, edge_lengths_riemannian
    from vqvae_amd.spatial_decoder import DecoderExport, hip_kernels_cover
    case, lib = C.CASES[name], _lib.load()
    want, want_stats, _ = C.reference(name, training, bs, torch.float64)
    zs, ze = (t.to(dev()) for t in C.edges(name))
    dec = _module(name, training)
    assert hip_kernels_cover(dec)
    before = _state(dec)
    ex = DecoderExport(dec, dev())
    assert C.route_of(lib, ex.desc, 0, C.E, bs, False) == case.pairs_route[training]
    assert lib.geo_jvp_head_stream(ex.desc, 0, C.E, bs, 0) == case.head_stream[training]
    got = edge_lengths_device(ex, zs, ze, bs)
    assert got.dtype == torch.float32 and got.shape == (C.E,) and got.is_cuda
    got = got.cpu().numpy()
    what = f"{name} train={training} bs={bs} pairs {case.pairs_route[training]}"
    C.check_against_fp64(got, want, case.q99_gate, what)
    _check_state(name, training, dec, before, want_stats, what)

    _forbid_autograd(monkeypatch)
    dec2 = _module(name, training)
    again = edge_lengths_riemannian(dec2, zs, ze, batch_size=bs)
    assert again.is_cuda and np.array_equal(again.cpu().numpy(), got), "module and export differ"
    _check_state(name, training, dec2, before, want_stats, what + " (module)")


@pytest.mark.parametrize("name,training,bs", RUNS, ids=RUN_IDS)
def test_graph_entry(name, training, bs, request):
    """300 latents, 1 500 edges (test_gpu_jvp_start_dedup._graph("mixed")).  With jvp_node_jacobian = 0 the graph entry is the
    pairs entry on the gathered end points bit for bit (per_node, dedup and the per-slot routes all promise it); with the
    default options it takes the case's graph route and passes the gate against the fp64 reference on the gathered end points,
    and the running statistics are that reference module's."""
    from vqvae_amd import _lib
    from vqvae_amd.geo.riemannian_metric import edge_lengths_device, edge_lengths_graph_device
    from vqvae_amd.spatial_decoder import DecoderExport
    case, lib = C.CASES[name], _lib.load()
    want, want_stats, _ = C.reference(name, training, bs, torch.float64, "graph")
    z, src, dst = (t.to(dev()) for t in C.graph(name))
    zs, ze = z[src.long()].contiguous(), z[dst.long()].contiguous()
    request.addfinalizer(lambda: lib.geo_set_option(b"jvp_node_jacobian", 1))

    _lib.check(lib.geo_set_option(b"jvp_node_jacobian", 0), "geo_set_option")
    ex = DecoderExport(_module(name, training), dev())
    route = case.graph_route[training]
    assert C.route_of(lib, ex.desc, C.N_NODES, C.N_EDGES, bs, True) == tuple(f for f in route if f != "node_jacobian")
    per_edge_end = edge_lengths_graph_device(ex, z, src, dst, bs).cpu().numpy()
    pairs = edge_lengths_device(DecoderExport(_module(name, training), dev()), zs, ze, bs).cpu().numpy()
    assert per_edge_end.shape == (C.N_EDGES,)
    np.testing.assert_array_equal(per_edge_end, pairs)

    _lib.check(lib.geo_set_option(b"jvp_node_jacobian", 1), "geo_set_option")
    dec = _module(name, training)
    before = _state(dec)
    ex = DecoderExport(dec, dev())
    assert C.route_of(lib, ex.desc, C.N_NODES, C.N_EDGES, bs, True) == route
    got = edge_lengths_graph_device(ex, z, src, dst, bs).cpu().numpy()
    what = f"{name} train={training} bs={bs} graph {route}"
    C.check_against_fp64(got, want, case.q99_gate, what)
    _check_state(name, training, dec, before, want_stats, what)


class _Filled0xFF(GuardedWorkspace):
    """ws_guard's exact, guarded workspace with every payload byte 0xFF: a NaN for every float the call reads before it
    writes.  (As an index 0xFFFFFFFF is out of range; the pairs entry of the routes below reads no index from the workspace
    that the same pass has not written -- slot_valid is its only one, filled by slot_valid_kernel first.)"""

    def __init__(self):
        super().__init__("zeros")

    def _new_buffer(self, nbytes, dev_):
        buf = super()._new_buffer(nbytes, dev_)
        buf[GUARD: GUARD + nbytes] = 0xFF
        assert int(buf[0]) == GUARD_BYTE and int(buf[GUARD]) == 0xFF and int(buf[GUARD + nbytes]) == GUARD_BYTE
        return buf


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", ["c1-32-bn", "c2-16-bn", "c2-128-bn-32px"])
def test_pairs_entry_on_a_workspace_of_0xff(name, training, monkeypatch):
    """One case per ConvT2 kernel off the default route (mid_all_kernel<32>, mid_bf16_kernel at 2 x 8 and at 16 x 1): the same
    bits, and the same running statistics, on a workspace of exactly the queried size whose every byte is 0xFF, with both
    guard bands intact."""
    from vqvae_amd.geo.riemannian_metric import edge_lengths_device
    from vqvae_amd.spatial_decoder import DecoderExport
    bs = 100                                    # 21 chunks, the last of 48 edges: padded slots in every group
    zs, ze = (t.to(dev()) for t in C.edges(name))

    def run():
        dec = _module(name, training)
        L = edge_lengths_device(DecoderExport(dec, dev()), zs, ze, bs)
        return L.cpu().numpy(), _state(dec)

    plain, plain_state = run()
    g = _Filled0xFF()
    with monkeypatch.context() as m:
        assert g.install(m)
        got, got_state = run()
    assert g.records, "the call took no workspace from the guarded allocator"
    g.check()
    assert np.all(np.isfinite(plain))
    np.testing.assert_array_equal(got, plain)
    assert all(torch.equal(got_state[k], plain_state[k]) for k in plain_state)


def test_groupnorm_decoder_with_a_64_output_head_takes_the_autograd_path(monkeypatch):
    """GroupNorm 256-128-64 at 32 px with 1 channel: 64 outputs, for which GroupNorm has no ConvT3.  hip_kernels_cover says so
    (as make_route does), and edge_lengths_riemannian answers through autograd instead of raising a GeoHipError -- within the
    bound of test_gpu_metric.test_groupnorm_decoder_outside_the_kernels_takes_the_autograd_path of the fp64 closed form."""
    from oracle import metric as om
    from vqvae_amd.geo import riemannian_metric
    from vqvae_amd.spatial_decoder import SpatialDecoder, hip_kernels_cover
    sd = om.make_decoder_state(12, 16, 1, channels=(256, 128, 64), norm_type="group")
    dec = SpatialDecoder(1, (256, 128, 64), 16, 32, "group")
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    assert not hip_kernels_cover(dec)
    r = np.random.RandomState(112)
    zs = r.randn(512, 16).astype(np.float32)
    ze = (zs + 0.3 * r.randn(512, 16)).astype(np.float32)
    calls, autograd = [], riemannian_metric._generic_jvp_norms

    def counted(*a, **k):
        calls.append(1)
        return autograd(*a, **k)
    monkeypatch.setattr(riemannian_metric, "_generic_jvp_norms", counted)
    L = riemannian_metric.edge_lengths_riemannian(dec.to(dev()).eval(), torch.from_numpy(zs), torch.from_numpy(ze), batch_size=512)
    assert len(calls) == 2 and L.is_cuda and L.dtype == torch.float32 and L.shape == (512,)
    L64 = om.edge_lengths(sd, "group", 32, zs, ze, batch_size=512, training=False, dtype=torch.float64).numpy()
    rel = np.abs(L.cpu().numpy() - L64) / L64
    print(f"GroupNorm 256-128-64, 1 ch at 32 px (autograd): {np.mean(rel <= 1e-4):.4%} within 1e-4, max {rel.max():.3e}")
    assert np.mean(rel <= 1e-4) >= 0.99
