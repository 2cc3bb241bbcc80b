"""Shared by test_jvp_envelope_host.py and test_gpu_jvp_envelope.py: seeded SpatialDecoders at the corners of the envelope
spatial_decoder.hip_kernels_cover admits, the edge sets, the autograd references (computed once per case,
mode, batch size and dtype, on the CPU) and the accuracy gate of test_gpu_metric.py."""
import copy
import functools
import os
import sys
from typing import NamedTuple, Tuple

import numpy as np
import torch
import torch.nn as nn

from vqvae_amd.geo.riemannian_metric import _generic_jvp_norms as _AUTOGRAD      # bound here, before any monkeypatching

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_jvp_start_dedup import _graph  # noqa: E402

E = 2048                                 # pairs per case
N_NODES, N_EDGES = 300, 1500             # the graph of the graph entry
TOL = 1e-5
RELU_MARGIN = 2.0 ** -23                 # one float32 ulp of 1.0: the normalised pre-activations entering a ReLU are O(1)
BATCH_SIZES = (512, 100)
NORM_CODE = {"none": 0, "batch": 1, "group": 2, "batch-plain": 1, "batch-untracked": 1}


class Case(NamedTuple):
    channels: Tuple[int, int, int]
    d: int
    out_channels: int
    size: int
    norm: str                 # none | batch | group | batch-plain (affine=False) | batch-untracked (track_running_stats=False)
    modes: Tuple[bool, ...]   # module.training of the runs; GroupNorm and no norm do not depend on it: eval only
    seed: int
    outside: int              # edges float32 torch leaves outside 1e-5 of fp64: the most over modes, batch sizes and both edge sets
    f32_q99: float            # float32 torch's 0.99-quantile against fp64 (relative), the most over the same runs, rounded up
    pairs_route: dict         # mode -> (front + width, mid, back, flags...) of the 2 048 pairs
    graph_route: dict         # mode -> the same for 300 latents / 1 500 edges at the default options
    head_stream: dict         # mode -> what geo_jvp_head_stream answers for the pairs

    @property
    def q99_gate(self) -> float:
        """2e-6 (test_gpu_metric.py) where float32 torch itself stays at or below 1e-6, else twice float32 torch's figure."""
        return 2e-6 if self.f32_q99 <= 1e-6 else 2.0 * self.f32_q99


TRAIN, EVAL = True, False

# A seed is admitted only if, in every mode and batch size the case runs in, on the 2 048 pairs and on the graph's 1 500
# gathered pairs,
#   (a) float32 torch (the same autograd route in float32 on the CPU) leaves NO edge outside 1e-5 of the fp64 reference: the gate
#       (99.9 %) then leaves the kernels two edges of 2 048 and one of 1 500.  Any float32 evaluation moves an edge whose ReLU
#       pre-activation sits on a rounding boundary; a seed with such an edge would spend the allowance before a kernel ran;
#   (b) with batch statistics (train-mode BatchNorm) no ReLU pre-activation of the fp64 reference lies within RELU_MARGIN of zero.
#       (a) alone does not do in train mode: which boundary samples flip differs between two float32 evaluations (the kernels
#       compose conv_in and ConvT1 and split ConvT2's operands, torch does neither), and a flipped sample enters the next
#       layer's batch means, so it moves every edge of its chunk -- a few 1e-6 on hundreds of edges, which the per-edge
#       allowance cannot absorb.  Measured on the first seeds that met (a): d33-2ch32 at seed 21, batch 512, has one
#       pre-activation of 1.2e-8 in chunk 1; float32 torch keeps its sign, the kernels do not, and that chunk alone sits at a
#       median of 1.6e-6 (q99 of the run 4.9e-6; the other chunks 1.5e-7).  With fixed statistics a flip moves its own edge
#       only, which is what the allowance is for: every run there has pre-activations of 1e-8 .. 5e-8.
# `outside` and `f32_q99` are the counted figures (test_jvp_envelope_host.test_every_case_is_admitted counts again, and checks
# (b)); after changing a shape or a seed, count again.  A case takes the first seed from 21 upwards that meets (a) and (b).
CASES = {}


def _case(name, channels, d, cout, size, norm, modes, seed, outside, f32_q99, pairs_route, graph_route, head_stream):
    CASES[name] = Case(channels, d, cout, size, norm, modes, seed, outside, f32_q99, pairs_route, graph_route, head_stream)


def descriptor(case: Case, training: bool):
    """The case's integers as a descriptor without weights: what geo_jvp_plan reads (as jvp_plan_cases.descriptor)."""
    from vqvae_amd import _lib
    c0, c1, c2 = case.channels
    groups = (min(32, c1), min(32, c2)) if case.norm == "group" else (0, 0)
    bn_train = int(NORM_CODE[case.norm] == 1 and (training or case.norm == "batch-untracked"))
    return _lib.DecoderDesc(latent_dim=case.d, c0=c0, c1=c1, c2=c2, out_channels=case.out_channels, out_size=case.size,
                            norm=NORM_CODE[case.norm], bn_train=bn_train, groups1=groups[0], groups2=groups[1], eps=1e-5,
                            update_running=int(bn_train and case.norm != "batch-untracked"), momentum=0.1)


def route_of(lib, desc, n_nodes, n_edges, bs, graph):
    """geo_jvp_plan's answer as (front + width, mid, back, flags...)."""
    from vqvae_amd import _lib
    code = lib.geo_jvp_plan(desc, n_nodes, n_edges, bs, int(graph), 0)
    assert code >= 0, lib.geo_last_error()
    r = _lib.decode_jvp_plan(code)
    flags = tuple(f for f in ("per_node", "node_jacobian", "dedup", "front_once") if r.get(f))
    return (f"{r['front']}{r['dmax']}", r["mid"], r["back"]) + flags


def build(name: str) -> nn.Module:
    """A float32 SpatialDecoder on the CPU with oracle.metric.make_decoder_state's seeded weights (train mode, as constructed).
    batch-plain / batch-untracked: the BatchNorm2d layers are replaced afterwards by BatchNorm2d(affine=False) carrying the
    seeded running statistics, or by BatchNorm2d(track_running_stats=False) carrying the seeded gamma and beta."""
    from oracle import metric as om
    from vqvae_amd.spatial_decoder import SpatialDecoder
    case = CASES[name]
    norm = "batch" if case.norm.startswith("batch") else case.norm
    sd = om.make_decoder_state(case.seed, case.d, case.out_channels, channels=case.channels, norm_type=norm)
    dec = SpatialDecoder(case.out_channels, case.channels, case.d, case.size, norm)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    if case.norm in ("batch-plain", "batch-untracked"):
        seq = dec.deconv_layers
        for i in (1, 4):
            old = seq[i]
            if case.norm == "batch-plain":
                new = nn.BatchNorm2d(old.num_features, affine=False)
                new.load_state_dict({"running_mean": old.running_mean, "running_var": old.running_var,
                                     "num_batches_tracked": old.num_batches_tracked})
            else:
                new = nn.BatchNorm2d(old.num_features, track_running_stats=False)
                new.load_state_dict({"weight": old.weight, "bias": old.bias})
            seq[i] = new
    return dec


def state_dict_of(name: str) -> dict:
    """The oracle's state dict of a plain `batch` / `group` / `none` case (what oracle.metric.edge_lengths reads)."""
    from oracle import metric as om
    case = CASES[name]
    assert case.norm in ("none", "batch", "group")
    return om.make_decoder_state(case.seed, case.d, case.out_channels, channels=case.channels, norm_type=case.norm)


@functools.lru_cache(maxsize=None)
def edges(name: str):
    """(z_start, z_end) float32 [E, d] on the CPU: ze = zs + 0.3 * randn, as test_gpu_metric._decoder."""
    case = CASES[name]
    r = np.random.RandomState(100 + case.seed)
    zs = r.randn(E, case.d).astype(np.float32)
    ze = (zs + 0.3 * r.randn(E, case.d)).astype(np.float32)
    return torch.from_numpy(zs), torch.from_numpy(ze)


@functools.lru_cache(maxsize=None)
def graph(name: str):
    """(z [300, d] float32, src, dst int32 [1 500]) on the CPU: test_gpu_jvp_start_dedup._graph("mixed", ...)."""
    case = CASES[name]
    src, dst = _graph("mixed", N_NODES, N_EDGES, 7 + case.seed)
    z = np.random.RandomState(200 + case.seed).randn(N_NODES, case.d).astype(np.float32)
    return torch.from_numpy(z), torch.from_numpy(src), torch.from_numpy(dst)


def end_points(name: str, which: str):
    """The pairs of `which`: "pairs" = edges(name), "graph" = the graph's gathered end points."""
    if which == "pairs":
        return edges(name)
    z, src, dst = graph(name)
    return z[src.long()].contiguous(), z[dst.long()].contiguous()


RUNNING_KEYS = ("running_mean", "running_var", "num_batches_tracked")


@functools.lru_cache(maxsize=None)
def reference(name: str, training: bool, bs: int, dtype=torch.float64, which: str = "pairs"):
    """The package's autograd route (riemannian_metric._generic_jvp_norms as imported here) on a deep copy of the module in
    `dtype` on the CPU, in chunks of `bs`: start side, then end side, per chunk -- the decoder calls of the reference's
    edge_lengths_riemannian, so train-mode BatchNorm sees the same batches in the same order.
    Returns (lengths as a numpy array of `dtype`,
             {"deconv_layers.<i>.<key>": numpy array} of the copy's running_mean, running_var and num_batches_tracked after
             the call; empty where the layers keep none,
             margin [edges]: the smallest |pre-activation| entering either ReLU at either end of the edge).  Read-only."""
    dec = copy.deepcopy(build(name)).to(dtype).train(training)
    zs, ze = (t.to(dtype) for t in end_points(name, which))
    delta = ze - zs
    seen = []
    hooks = [dec.deconv_layers[i].register_forward_pre_hook(
        lambda mod, inp: seen.append(inp[0].detach().abs().flatten(1).amin(1))) for i in (2, 5)]
    out, margin = [], []
    for lo in range(0, zs.shape[0], bs):
        sl = slice(lo, lo + bs)
        seen.clear()
        a = _AUTOGRAD(dec, zs[sl], delta[sl])
        b = _AUTOGRAD(dec, ze[sl], delta[sl])
        out.append((0.5 * (a + b)).detach())
        margin.append(torch.stack(seen).amin(0))
    for h in hooks:
        h.remove()
    stats = {k: v.detach().clone().numpy() for k, v in dec.state_dict().items() if k.endswith(RUNNING_KEYS)}
    lengths, margin = torch.cat(out).numpy(), torch.cat(margin).double().numpy()
    lengths.setflags(write=False)
    margin.setflags(write=False)
    return lengths, stats, margin


def rel_error(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.abs(want.astype(np.float64))


def figures(got: np.ndarray, want: np.ndarray):
    """(fraction within 1e-5, 0.99-quantile, maximum) of the relative error."""
    rel = rel_error(got, want)
    return float(np.mean(rel <= TOL)), float(np.quantile(rel, 0.99)), float(rel.max())


def check_against_fp64(got: np.ndarray, want: np.ndarray, q99_gate: float, what: str = "") -> None:
    """The gate of tests/test_gpu_metric.py: at least 99.9 % of the edges within 1e-5 (relative) of the fp64 lengths and the
    0.99-quantile below `q99_gate`.  Prints the figures first."""
    within, q99, worst = figures(got, want)
    print(f"{what}: {within:.4%} within {TOL}, q99 {q99:.3e}, max {worst:.3e} (q99 gate {q99_gate:.1e})")
    assert np.all(np.isfinite(got)), what
    assert within >= 0.999, (what, within, worst)
    assert q99 < q99_gate, (what, q99, q99_gate)


# name | dec_channels, d, out_channels, size, norm, modes, seed | outside, float32 q99 | routes: pairs, graph, head_stream.
# The routes are what make_route gives for these integers (geo_jvp_plan; the same at batch 512 and 100); the graph is the 300
# latents / 1 500 edges of graph(): 5 edges per latent, so of the fixed-statistics cases only d = 1 and d = 3 (4 E >= 3 N d) take
# the per-latent Jacobian.
_ALL, _CHUNK = ("all", "mfma"), ("chunk", "valu")
_PN = ("all_tangent", "per_node", "per_node")
_PIPE, _PIPE_VALU = ("pipe", "mfma"), ("pipe", "valu")
_DEDUP = ("pipe_dedup", "dedup", "dedup")


def _both(route, head_stream=None):
    return {TRAIN: route, EVAL: route} if head_stream is None else {TRAIN: head_stream, EVAL: head_stream}


# mid_all_kernel<32>; eval on a graph: all_tangent / per_node at c1 = 32
_case("c1-32-bn", (256, 32, 64), 16, 1, 28, "batch", (TRAIN, EVAL), 22, 0, 4.9e-7,
      _both(("valu16",) + _ALL), {TRAIN: ("valu16",) + _ALL, EVAL: ("valu16",) + _PN}, _both(None, 1))
# one channel per group in layer 1; d = 3; back_mfma_kernel<6, true>.  float32 torch's q99 is above 1e-6: the gate is twice it
_case("c1-32-group-192", (256, 32, 64), 3, 3, 32, "group", (EVAL,), 21, 0, 1.53e-6,
      {EVAL: ("valu16",) + _ALL}, {EVAL: ("valu16",) + _PN + ("node_jacobian",)}, {EVAL: 0})
# two channels per group in layer 1
_case("c1-64-group", (256, 64, 64), 16, 1, 28, "group", (EVAL,), 21, 0, 4.9e-7,
      {EVAL: ("valu16",) + _ALL}, {EVAL: ("valu16",) + _PN}, {EVAL: 0})
# mid_bf16_kernel's chunk geometry 2 x 8, back_kernel at its smallest LDS footprint
_case("c2-16-bn", (256, 128, 16), 16, 1, 28, "batch", (TRAIN, EVAL), 21, 0, 4.1e-7,
      _both(("valu16",) + _CHUNK), _both(("valu16",) + _CHUNK), _both(None, 0))
# chunk geometry 16 x 1, back_kernel at 145 664 B of LDS.  Seeds 21 to 29 leave 1 to 3 edges outside (train mode), (a)
_case("c2-128-bn-32px", (256, 128, 128), 16, 1, 32, "batch", (TRAIN, EVAL), 47, 0, 3.5e-7,
      _both(("valu16",) + _CHUNK), _both(("valu16",) + _CHUNK), _both(None, 0))
# c0 = 64, mid_bf16_kernel<32>
_case("small-64-32-16", (64, 32, 16), 16, 1, 28, "batch", (TRAIN,), 21, 0, 2.8e-7,
      {TRAIN: ("valu16",) + _CHUNK}, {TRAIN: ("valu16",) + _CHUNK}, {TRAIN: 0})
# c0 no multiple of 8 (compose_front_kernel's clamped tail); 32 live output columns: back_mfma_kernel<1> and head_stream_kernel
_case("c0-100-2ch28", (100, 64, 64), 7, 2, 28, "batch", (TRAIN, EVAL), 36, 0, 2.6e-7,
      _both(("valu16",) + _ALL), {TRAIN: ("valu16",) + _ALL, EVAL: ("valu16",) + _PN}, _both(None, 1))
# front_mfma_kernel<32> with 15 padded columns; 64 outputs (back_kernel) behind mid_pipe_kernel
_case("d17-4ch28", (256, 128, 64), 17, 4, 28, "batch", (TRAIN,), 22, 0, 2.3e-7,
      {TRAIN: ("mfma32",) + _PIPE_VALU}, {TRAIN: ("mfma32",) + _PIPE_VALU}, {TRAIN: 0})
# front_mfma_kernel<64> with 31 padded columns; 128 outputs
_case("d33-2ch32", (256, 128, 64), 33, 2, 32, "batch", (TRAIN,), 26, 0, 2.2e-7,
      {TRAIN: ("mfma64",) + _PIPE_VALU}, {TRAIN: ("mfma64",) + _PIPE_VALU}, {TRAIN: 0})
# d = 1 on the VALU front (and one Jacobian column per latent on the graph)
_case("d1-none", (256, 128, 64), 1, 1, 28, "none", (EVAL,), 21, 0, 3.1e-7,
      {EVAL: ("valu16",) + _PIPE}, {EVAL: ("valu16",) + _PN + ("node_jacobian",)}, {EVAL: 1})
# front_edge_kernel (front_once) at d = 2 on the graph entry
_case("d2-bn-train", (256, 128, 64), 2, 1, 28, "batch", (TRAIN,), 28, 0, 5.7e-7,
      {TRAIN: ("valu16",) + _PIPE}, {TRAIN: ("valu16",) + _DEDUP + ("front_once",)}, {TRAIN: 1})
# matrix-core front + pipe_dedup + dedup + head_stream on the graph entry
_case("d63-bn-train", (256, 128, 64), 63, 1, 28, "batch", (TRAIN,), 38, 0, 5.2e-7,
      {TRAIN: ("mfma64",) + _PIPE}, {TRAIN: ("mfma64",) + _DEDUP}, {TRAIN: 1})
# BatchNorm2d(affine=False): no gamma / beta in the export.
_case("plain-bn", (256, 128, 64), 16, 1, 28, "batch-plain", (TRAIN, EVAL), 38, 0, 5.0e-7,
      _both(("valu16",) + _PIPE), {TRAIN: ("valu16",) + _DEDUP + ("front_once",), EVAL: ("valu16",) + _PN}, _both(None, 1))
# BatchNorm2d(track_running_stats=False), gamma and beta kept: Route::track false, nothing to fold, batch statistics still used
_case("untracked-bn-train", (256, 128, 64), 16, 1, 28, "batch-untracked", (TRAIN,), 56, 0, 4.9e-7,
      {TRAIN: ("valu16",) + _PIPE}, {TRAIN: ("valu16",) + _DEDUP + ("front_once",)}, {TRAIN: 1})
