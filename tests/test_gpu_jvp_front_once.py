"""Train-mode BatchNorm over graph edges, d <= 16: the first layer runs once per edge (`jvp_front_once`, default on) -- the tangent
row is stored for the end slot only and the start-side primal row only at the head of a run of equal `src`.  Lengths and the folded
running statistics must equal the row-per-slot front (option 0) bit for bit, on small graphs that reach every corner of the head
rule and of the reads that replace the rows no longer written."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_jvp_start_dedup import _assert_same, _decoder, _graph  # noqa: E402

pytestmark = pytest.mark.gpu


def _plan(lib, ex, n_nodes, n_edges, bs):
    from vqvae_amd import _lib
    code = lib.geo_jvp_plan(ex.desc, n_nodes, n_edges, bs, 1, 0)
    assert code >= 0, lib.geo_last_error()
    return _lib.decode_jvp_plan(code)


def _run(sd, d, cout, size, z, src, dst, bs, mode):
    """Lengths and running statistics of one call from a fresh decoder; the plan must name the route `mode` asks for."""
    from vqvae_amd import _lib
    from vqvae_amd.geo.riemannian_metric import edge_lengths_graph_device
    from vqvae_amd.spatial_decoder import DecoderExport
    lib = _lib.load()
    _lib.check(lib.geo_set_option(b"jvp_front_once", mode), "geo_set_option")
    ex = DecoderExport(_decoder(sd, d, cout, size, z.device), z.device)
    r = _plan(lib, ex, z.shape[0], src.numel(), bs)
    assert (r["front"], r["mid"], r["back"], r["dedup"]) == ("valu", "pipe_dedup", "dedup", True)
    assert r.get("front_once", False) == bool(mode)
    L = edge_lengths_graph_device(ex, z, src, dst, bs).cpu().numpy()
    return L, {k: ex.tensors[k].cpu().numpy().copy() for k in ("rm1", "rv1", "rm2", "rv2")}


@pytest.fixture()
def option(request):
    from vqvae_amd import _lib
    request.addfinalizer(lambda: _lib.load().geo_set_option(b"jvp_front_once", 1))


def _inputs(kind, n_nodes, n_edges, d, dev):
    if kind == "runs40":                   # runs of 40 slots: heads at 0, 40, 80, ... -- every run crosses a 32-slot tile boundary
        r = np.random.RandomState(n_edges)                               # (its head is in another workgroup's tile); 512 / 40 is
        src_h = (np.arange(n_edges) // 40 % n_nodes).astype(np.int32)    # no integer: runs cross the chunk boundaries too
        dst_h = ((src_h + 1 + r.randint(0, n_nodes - 1, n_edges)) % n_nodes).astype(np.int32)
    else:
        src_h, dst_h = _graph(kind, n_nodes, n_edges, n_edges)
    z = torch.from_numpy(np.random.RandomState(1).randn(n_nodes, d).astype(np.float32)).to(dev)
    return z, torch.from_numpy(src_h).to(dev), torch.from_numpy(dst_h).to(dev)


@pytest.mark.parametrize("kind,n_nodes,n_edges,bs,cout,size,d", [
    ("distinct", 3000, 2048, 512, 1, 28, 16),    # every slot a head: every start-side primal row is stored
    ("runs7", 3000, 5001, 512, 1, 28, 16),       # runs cross chunk boundaries: the head rule restarts at within == 0
    ("mixed", 3000, 9000, 512, 1, 28, 16),
    ("shuffled", 1000, 7777, 512, 1, 28, 16),
    ("mixed", 2000, 6000, 200, 1, 28, 16),       # 7 tiles per group: the last tangent tile of a group has no partner
    ("mixed", 1500, 6100, 512, 3, 32, 16),       # 192-output head
    ("mixed", 3000, 9000, 512, 1, 28, 5),        # padded latent columns
    ("mixed", 300, 20, 512, 1, 28, 16),          # fewer than 32 edges: one partly filled tile
    ("runs40", 3000, 5000, 512, 1, 28, 16),      # runs cross the 32-slot tile boundaries inside a chunk, and the chunk boundaries
    ("mixed", 3000, 1025, 512, 1, 28, 16),       # one edge above a multiple of the batch: the last chunk is one head slot
])
def test_front_once_is_bit_identical_on_small_graphs(kind, n_nodes, n_edges, bs, cout, size, d, option):
    from oracle import metric as om
    from vqvae_amd._device import device
    dev = device()
    sd = om.make_decoder_state(5, d, cout, norm_type="batch")
    z, src, dst = _inputs(kind, n_nodes, n_edges, d, dev)
    _assert_same({mode: _run(sd, d, cout, size, z, src, dst, bs, mode) for mode in (1, 0)})


def test_front_once_reads_no_stale_row(option):
    """Another graph first, then the test graph twice in one process: the workspace (cached between calls or not) holds the other
    graph's start-side rows where the front no longer writes, and the two results must not depend on them."""
    from oracle import metric as om
    from vqvae_amd._device import device
    dev = device()
    d = 16
    sd = om.make_decoder_state(5, d, 1, norm_type="batch")
    other = _inputs("distinct", 3000, 6000, d, dev)
    z, src, dst = _inputs("mixed", 3000, 6000, d, dev)
    _run(sd, d, 1, 28, *other, 512, 1)
    first = _run(sd, d, 1, 28, z, src, dst, 512, 1)
    second = _run(sd, d, 1, 28, z, src, dst, 512, 1)
    _assert_same({1: first, 0: second})
    _assert_same({1: first, 0: _run(sd, d, 1, 28, z, src, dst, 512, 0)})


def test_front_once_stays_off_other_routes(option):
    """Eval-mode BatchNorm (fixed statistics: no dedup) and d = 32 (the matrix-core front) keep their kernels."""
    from oracle import metric as om
    from vqvae_amd import _lib
    from vqvae_amd._device import device
    from vqvae_amd.spatial_decoder import DecoderExport
    dev = device()
    lib = _lib.load()
    _lib.check(lib.geo_set_option(b"jvp_front_once", 1), "geo_set_option")
    ev = DecoderExport(_decoder(om.make_decoder_state(5, 16, 1, norm_type="batch"), 16, 1, 28, dev).eval(), dev)
    r = _plan(lib, ev, 3000, 9000, 512)
    assert not r["dedup"] and not r.get("front_once", False)
    wide = DecoderExport(_decoder(om.make_decoder_state(5, 32, 1, norm_type="batch"), 32, 1, 28, dev), dev)
    r = _plan(lib, wide, 3000, 9000, 512)
    assert (r["front"], r["dmax"], r["dedup"]) == ("mfma", 32, True) and not r.get("front_once", False)
