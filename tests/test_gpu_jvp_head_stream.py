"""The 16-output ConvT3 head without GroupNorm runs as `head_stream_kernel` (`jvp_head_stream`, default on): back_mfma_kernel's
staged values, products and epilogue with the next K block's rows in flight.  Lengths and the folded running statistics must equal
the template's (option 0) array for array -- on the dedup route (end side per slot, start-side tangents through `row_map`), on
route `mfma` (every tile per slot), through the explicit end-point entry, and not at all on the heads the kernel does not serve."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_jvp_front_once import _inputs  # noqa: E402
from test_gpu_jvp_start_dedup import _assert_same, _decoder, _graph  # noqa: E402,F401

pytestmark = pytest.mark.gpu

STATS = ("rm1", "rv1", "rm2", "rv2")


@pytest.fixture()
def option(request):
    from vqvae_amd import _lib

    def restore():
        lib = _lib.load()
        lib.geo_set_option(b"jvp_head_stream", 1)
        lib.geo_set_option(b"jvp_start_dedup", 1)
    request.addfinalizer(restore)


def _set(mode):
    from vqvae_amd import _lib
    lib = _lib.load()
    _lib.check(lib.geo_set_option(b"jvp_head_stream", mode), "geo_set_option")
    return lib


def _stats(ex):
    return {k: ex.tensors[k].cpu().numpy().copy() for k in STATS if ex.tensors.get(k) is not None}


def _run_graph(make_decoder, z, src, dst, bs, mode, serves=True, back=None):
    """Lengths and running statistics of one graph call from a fresh decoder; the query must answer what `mode` asks for."""
    from vqvae_amd import _lib
    from vqvae_amd.geo.riemannian_metric import edge_lengths_graph_device
    from vqvae_amd.spatial_decoder import DecoderExport
    lib = _set(mode)
    ex = DecoderExport(make_decoder(), z.device)
    assert lib.geo_jvp_head_stream(ex.desc, z.shape[0], src.numel(), bs, 1) == int(bool(mode) and serves), lib.geo_last_error()
    if back is not None:
        code = lib.geo_jvp_plan(ex.desc, z.shape[0], src.numel(), bs, 1, 0)
        assert code >= 0 and _lib.decode_jvp_plan(code)["back"] == back
    L = edge_lengths_graph_device(ex, z, src, dst, bs).cpu().numpy()
    return L, _stats(ex)


def _run_pairs(make_decoder, zs, ze, bs, mode, serves=True):
    from vqvae_amd.geo.riemannian_metric import edge_lengths_device
    from vqvae_amd.spatial_decoder import DecoderExport
    lib = _set(mode)
    ex = DecoderExport(make_decoder(), zs.device)
    assert lib.geo_jvp_head_stream(ex.desc, 0, zs.shape[0], bs, 0) == int(bool(mode) and serves), lib.geo_last_error()
    L = edge_lengths_device(ex, zs, ze, bs).cpu().numpy()
    return L, _stats(ex)


def _bn_train(d, cout, size, dev, seed=5):
    from oracle import metric as om
    sd = om.make_decoder_state(seed, d, cout, norm_type="batch")
    return lambda: _decoder(sd, d, cout, size, dev)


@pytest.mark.parametrize("kind,n_nodes,n_edges,bs,cout,size,d", [
    ("mixed", 300, 20, 512, 1, 28, 16),          # one partly filled tile
    ("mixed", 3000, 1025, 512, 1, 28, 16),       # the last chunk is one slot
    ("mixed", 2000, 6000, 200, 1, 28, 16),       # 7 tiles per group, padding slots in every group
    ("distinct", 3000, 2048, 512, 1, 28, 16),    # 512 compact rows per chunk
    ("runs40", 3000, 5000, 512, 1, 28, 16),      # runs cross tile and chunk boundaries: row_map points into other tiles
    ("shuffled", 1000, 7777, 512, 1, 28, 16),    # no order, short runs only
    ("mixed", 3000, 9000, 512, 1, 28, 5),        # d = 5
    ("mixed", 60000, 530000, 512, 1, 28, 16),    # two passes, the second with 12 chunks
])
def test_head_stream_is_bit_identical_on_the_dedup_route(kind, n_nodes, n_edges, bs, cout, size, d, option):
    from vqvae_amd._device import device
    dev = device()
    z, src, dst = _inputs(kind, n_nodes, n_edges, d, dev)
    make = _bn_train(d, cout, size, dev)
    _assert_same({mode: _run_graph(make, z, src, dst, bs, mode, back="dedup") for mode in (1, 0)})


def test_head_stream_is_bit_identical_per_slot(option):
    """jvp_start_dedup = 0: route `mfma`, primal + tangent per slot over every tile of both sides."""
    from vqvae_amd import _lib
    from vqvae_amd._device import device
    dev = device()
    _lib.check(_lib.load().geo_set_option(b"jvp_start_dedup", 0), "geo_set_option")
    z, src, dst = _inputs("mixed", 3000, 9000, 16, dev)
    make = _bn_train(16, 1, 28, dev)
    _assert_same({mode: _run_graph(make, z, src, dst, 512, mode, back="mfma") for mode in (1, 0)})


@pytest.mark.parametrize("n_pairs", [1, 33, 1000])
def test_head_stream_is_bit_identical_on_explicit_end_points(n_pairs, option):
    from vqvae_amd._device import device
    dev = device()
    r = np.random.RandomState(n_pairs)
    zs = torch.from_numpy(r.randn(n_pairs, 16).astype(np.float32)).to(dev)
    ze = torch.from_numpy(r.randn(n_pairs, 16).astype(np.float32)).to(dev)
    make = _bn_train(16, 1, 28, dev)
    _assert_same({mode: _run_pairs(make, zs, ze, 512, mode) for mode in (1, 0)})


def test_head_stream_reads_no_stale_row(option):
    """Another graph first, then the test graph twice in one process: the workspace holds the other graph's rows, maps and sigmoids,
    and the results must not depend on them."""
    from vqvae_amd._device import device
    dev = device()
    d = 16
    make = _bn_train(d, 1, 28, dev)
    other = _inputs("distinct", 3000, 6000, d, dev)
    z, src, dst = _inputs("mixed", 3000, 6000, d, dev)
    _run_graph(make, *other, 512, 1)
    first = _run_graph(make, z, src, dst, 512, 1)
    second = _run_graph(make, z, src, dst, 512, 1)
    _assert_same({1: first, 0: second})
    _assert_same({1: first, 0: _run_graph(make, z, src, dst, 512, 0)})


@pytest.mark.parametrize("what", ["192_outputs", "bn_eval", "group"])
def test_head_stream_stays_off_other_heads(what, option):
    """The 192-output head, the per-latent routes of fixed statistics, and GroupNorm keep back_mfma_kernel: the query answers 0 and
    the option changes nothing."""
    from oracle import metric as om
    from vqvae_amd._device import device
    from vqvae_amd.spatial_decoder import SpatialDecoder
    dev = device()
    d = 16
    if what == "192_outputs":
        make = _bn_train(d, 3, 32, dev)
    elif what == "bn_eval":
        train = _bn_train(d, 1, 28, dev)
        make = lambda: train().eval()  # noqa: E731
    else:
        sd = om.make_decoder_state(5, d, 1, norm_type="group")

        def make():
            dec = SpatialDecoder(1, (256, 128, 64), d, 28, "group")
            dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
            return dec.to(dev).eval()
    z, src, dst = _inputs("mixed", 1500, 6100, d, dev)
    _assert_same({mode: _run_graph(make, z, src, dst, 512, mode, serves=False) for mode in (1, 0)})
    if what == "group":                          # GroupNorm on explicit end points: route `mfma`, still the template
        zs, ze = z[src.long()[:700]].contiguous(), z[dst.long()[:700]].contiguous()
        _assert_same({mode: _run_pairs(make, zs, ze, 512, mode, serves=False) for mode in (1, 0)})
