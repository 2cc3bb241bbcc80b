"""Train-mode BatchNorm over graph edges: each chunk's start-side primal ConvT2 / ConvT3 rows run once per run of equal `src`
(`jvp_start_dedup`, default on).  Lengths and the folded running statistics must equal the once-per-slot path (option 0) bit for
bit: at the C2 size and on small graphs that reach every corner of the run map."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _decoder(sd, d, cout, size, dev):
    from vqvae_amd.spatial_decoder import SpatialDecoder
    dec = SpatialDecoder(cout, (256, 128, 64), d, size, "batch")
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return dec.to(dev).train()


def _both_modes(sd, d, cout, size, z, src, dst, bs, request):
    """Lengths and running statistics with the option on and off, each from a fresh decoder."""
    from vqvae_amd import _lib
    from vqvae_amd.geo.riemannian_metric import edge_lengths_graph_device
    from vqvae_amd.spatial_decoder import DecoderExport
    lib = _lib.load()
    request.addfinalizer(lambda: lib.geo_set_option(b"jvp_start_dedup", 1))
    out = {}
    for mode in (1, 0):
        _lib.check(lib.geo_set_option(b"jvp_start_dedup", mode), "geo_set_option")
        ex = DecoderExport(_decoder(sd, d, cout, size, z.device), z.device)
        r = _lib.decode_jvp_plan(lib.geo_jvp_plan(ex.desc, z.shape[0], src.numel(), bs, 1, 0))
        assert (r["front"], r["mid"], r["back"], r["dedup"]) == (("valu", "pipe_dedup", "dedup", True) if mode else
                                                                 ("valu", "pipe", "mfma", False))
        L = edge_lengths_graph_device(ex, z, src, dst, bs).cpu().numpy()
        stats = {k: ex.tensors[k].cpu().numpy().copy() for k in ("rm1", "rv1", "rm2", "rv2")}
        out[mode] = (L, stats)
    return out


def _assert_same(out):
    np.testing.assert_array_equal(out[1][0], out[0][0])
    for k in out[0][1]:
        np.testing.assert_array_equal(out[1][1][k], out[0][1][k], err_msg=k)


def _graph(kind, n_nodes, n_edges, seed):
    r = np.random.RandomState(seed)
    if kind == "distinct":                 # every run one slot long: 512 compact rows per chunk (> 32 per group)
        src = np.arange(n_edges) % n_nodes
    elif kind == "runs7":                  # runs of 7: several runs straddle a chunk boundary
        src = np.arange(n_edges) // 7 % n_nodes
    elif kind == "mixed":                  # row-major like a kNN graph, 1 to 30 edges per latent
        src = np.repeat(np.arange(n_nodes), r.randint(1, 31, n_nodes))[:n_edges]
    elif kind == "shuffled":               # no order: short runs only
        src = np.repeat(np.arange(n_nodes), 16)[:n_edges]
        src = src[r.permutation(len(src))]
    else:
        raise ValueError(kind)
    src = src.astype(np.int32)
    assert len(src) == n_edges
    dst = ((src + 1 + r.randint(0, n_nodes - 1, n_edges)) % n_nodes).astype(np.int32)
    return src, dst


@pytest.mark.parametrize("kind,n_nodes,n_edges,bs,cout,size", [
    ("distinct", 3000, 2048, 512, 1, 28),
    ("runs7", 3000, 5001, 512, 1, 28),       # n_edges not a multiple of the batch
    ("mixed", 3000, 9000, 512, 1, 28),
    ("shuffled", 1000, 7777, 512, 1, 28),
    ("mixed", 2000, 6000, 200, 1, 28),       # 7 tiles per group: the last tangent tile of a group has no partner
    ("mixed", 1500, 6100, 512, 3, 32),       # 192-output head
])
def test_start_dedup_is_bit_identical_on_small_graphs(kind, n_nodes, n_edges, bs, cout, size, request):
    from oracle import metric as om
    from vqvae_amd._device import device
    dev = device()
    d = 16
    sd = om.make_decoder_state(5, d, cout, norm_type="batch")
    src_h, dst_h = _graph(kind, n_nodes, n_edges, n_edges)
    z = torch.from_numpy(np.random.RandomState(1).randn(n_nodes, d).astype(np.float32)).to(dev)
    src, dst = torch.from_numpy(src_h).to(dev), torch.from_numpy(dst_h).to(dev)
    _assert_same(_both_modes(sd, d, cout, size, z, src, dst, bs, request))


def test_start_dedup_is_bit_identical_at_c2(request):
    """The C2 graph (60 000 latents, d = 16, k = 20: 946 059 edges) with train-mode BatchNorm."""
    from oracle import metric as om
    from oracle import synthetic as syn
    from vqvae_amd._device import device
    from vqvae_amd.scripts.build_codebook import build_codebook_device
    dev = device()
    z_h = syn.gauss_latents(60000, 16, 0)
    sd = om.make_decoder_state(0, 16, 1, norm_type="batch")
    z = torch.from_numpy(z_h).to(dev)
    res = build_codebook_device(z, _decoder(sd, 16, 1, 28, dev), k=20, sym="union", K=512, init="kpp", seed=42,
                                batch_size=512)
    src, dst = res["edges"]
    assert src.numel() == 946059
    _assert_same(_both_modes(sd, 16, 1, 28, z, src, dst, 512, request))
