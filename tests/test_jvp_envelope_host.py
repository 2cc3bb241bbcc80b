"""The spatial decoder JVP's envelope on the host (no GPU): spatial_decoder.hip_kernels_cover against the library's own decision
(geo_jvp_plan, host arithmetic) over a grid of widths, heads and norms; the fp64 autograd reference of jvp_envelope_cases against
the closed-form oracle; the admission of every case's seed (float32 torch leaves no edge outside 1e-5, and in train mode no
ReLU pre-activation of the fp64 reference sits within a float32 ulp of zero); and the route of every case."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_envelope_cases as C  # noqa: E402


@pytest.fixture()
def lib():
    from vqvae_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- predicate against run

SWEEP_D = (1, 16, 17, 64, 65)
SWEEP_C1 = (16, 32, 48, 64, 128, 256)
SWEEP_C2 = (8, 16, 32, 48, 64, 128, 256)
SWEEP_OUT = (1, 2, 3, 4)
SWEEP_SIZE = (28, 32)
SWEEP_NORM = ("none", "batch", "group32", "group16")
SWEEP_C0 = 8                      # neither the predicate nor the route reads dec_channels[0]: small, so the sweep stays fast


def _norm_layer(kind, channels):
    if kind == "none":
        return nn.Identity()
    if kind == "batch":
        return nn.BatchNorm2d(channels)
    want = int(kind[len("group"):])             # that many groups, or (make_norm's rule) the largest divisor below it
    return nn.GroupNorm(next(g for g in range(min(want, channels), 0, -1) if channels % g == 0), channels)


def module_descriptor(m):
    """A module's integers as a descriptor without weights -- the fields DecoderExport fills, as jvp_plan_cases.descriptor."""
    from vqvae_amd import _lib
    seq = m.deconv_layers
    norm = seq[1]
    code = 1 if isinstance(norm, nn.BatchNorm2d) else 2 if isinstance(norm, nn.GroupNorm) else 0
    bn_train = int(code == 1 and (norm.training or norm.running_mean is None))
    groups = (seq[1].num_groups, seq[4].num_groups) if code == 2 else (0, 0)
    return _lib.DecoderDesc(latent_dim=m.conv_in.in_channels, c0=m.conv_in.out_channels, c1=seq[0].out_channels,
                            c2=seq[3].out_channels, out_channels=seq[6].out_channels, out_size={1: 32, 3: 28}[seq[6].padding[0]],
                            norm=code, bn_train=bn_train, groups1=groups[0], groups2=groups[1], eps=1e-5,
                            update_running=bn_train, momentum=0.1)


def test_the_predicate_answers_what_the_run_answers(lib):
    """hip_kernels_cover(module) == (geo_jvp_plan(descriptor of the module) >= 0) on the whole grid, for pairs and for graph
    edges: edge_lengths_riemannian, build_codebook and assign_codes_val_geodesic send a module to the kernels on the
    predicate's word alone, so a module it admits and make_route refuses raises instead of taking the autograd route."""
    from vqvae_amd.spatial_decoder import SpatialDecoder, hip_kernels_cover, looks_like_spatial_decoder
    wrong, covered = [], 0
    for c1, c2, out, size in itertools.product(SWEEP_C1, SWEEP_C2, SWEEP_OUT, SWEEP_SIZE):
        m = SpatialDecoder(out, (SWEEP_C0, c1, c2), 1, size, "none")
        for norm in SWEEP_NORM:
            m.deconv_layers[1], m.deconv_layers[4] = _norm_layer(norm, c1), _norm_layer(norm, c2)
            for d in SWEEP_D:
                m.conv_in = nn.Conv2d(d, SWEEP_C0, 1)
                assert looks_like_spatial_decoder(m)
                says = hip_kernels_cover(m)
                desc = module_descriptor(m)
                runs = (lib.geo_jvp_plan(desc, 0, C.E, 512, 0, 0) >= 0, lib.geo_jvp_plan(desc, C.N_NODES, C.N_EDGES, 512, 1, 0) >= 0)
                covered += says
                if runs != (says, says):
                    wrong.append(((c1, c2), d, out, size, norm, says, runs))
    assert wrong == [], (len(wrong), wrong[:8])
    assert 0 < covered < len(SWEEP_D) * len(SWEEP_C1) * len(SWEEP_C2) * len(SWEEP_OUT) * len(SWEEP_SIZE) * len(SWEEP_NORM)


@pytest.mark.parametrize("out,size,covered", [(1, 28, True), (2, 28, True), (3, 32, True), (1, 32, False), (4, 28, False),
                                              (2, 32, False), (3, 28, False)])
def test_groupnorm_heads_the_kernels_serve(lib, out, size, covered):
    """GroupNorm has the matrix-core ConvT3 only: 16, 32 and 192 outputs.  Every other head is refused by the predicate
    and by make_route alike (the default 256-128-64 decoder, 32 groups per layer)."""
    from vqvae_amd.spatial_decoder import SpatialDecoder, hip_kernels_cover
    m = SpatialDecoder(out, (SWEEP_C0, 128, 64), 16, size, "group")
    assert hip_kernels_cover(m) is covered
    for graph in (0, 1):
        code = lib.geo_jvp_plan(module_descriptor(m), C.N_NODES, C.N_EDGES, 512, graph, 0)
        assert (code >= 0) is covered
        if not covered:
            assert b"GroupNorm needs 32 groups per layer" in lib.geo_last_error()


# ---------------------------------------------------------------- the reference itself

@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", ["c1-32-bn", "c2-16-bn"])
def test_the_autograd_reference_is_the_closed_form(name, training):
    """Two fp64 statements of the same lengths: the package's autograd route on the module, and oracle.metric.edge_lengths on
    the state dict (the bound test_gpu_fullsize uses between two fp64 statements).  The oracle returns no running statistics."""
    from oracle import metric as om
    case = C.CASES[name]
    zs, ze = C.edges(name)
    for bs in C.BATCH_SIZES:
        auto = C.reference(name, training, bs, torch.float64)[0]
        closed = om.edge_lengths(C.state_dict_of(name), case.norm, case.size, zs.numpy(), ze.numpy(), batch_size=bs,
                                 training=training, dtype=torch.float64).numpy()
        assert auto.dtype == np.float64 and auto.shape == closed.shape == (C.E,)
        np.testing.assert_allclose(auto, closed, rtol=2e-6, atol=0)


def test_the_reference_folds_running_statistics_per_chunk_and_side():
    """What the GPU tests compare the kernels' running statistics with: the copy's statistics moved, num_batches_tracked counts
    two decoder calls per chunk, and the module the case builds is left as it was."""
    name = "c1-32-bn"
    before = {k: v.clone() for k, v in C.build(name).state_dict().items()}
    for bs, calls in ((512, 8), (100, 42)):
        stats = C.reference(name, True, bs, torch.float64)[1]
        assert sorted(stats) == sorted(k for k in before if k.endswith(C.RUNNING_KEYS))
        for i in (1, 4):
            assert int(stats[f"deconv_layers.{i}.num_batches_tracked"]) == calls
            assert not np.allclose(stats[f"deconv_layers.{i}.running_mean"], before[f"deconv_layers.{i}.running_mean"].numpy())
    stats = C.reference(name, False, 512, torch.float64)[1]
    assert all(np.array_equal(stats[k], before[k].numpy()) for k in stats)
    assert C.reference("untracked-bn-train", True, 512, torch.float64)[1] == {}


# ---------------------------------------------------------------- admission

@pytest.mark.parametrize("name", list(C.CASES))
def test_every_case_is_admitted(name):
    """In every mode and batch size the case runs in, on the pairs and on the graph's gathered pairs: float32 torch leaves no
    edge outside 1e-5 of the fp64 reference, its 0.99-quantile is at most the figure the case's q99 gate is derived from, and
    with batch statistics no ReLU pre-activation of the fp64 reference lies within C.RELU_MARGIN of zero."""
    case = C.CASES[name]
    assert case.outside == 0
    assert case.q99_gate == (2e-6 if case.f32_q99 <= 1e-6 else 2 * case.f32_q99)
    for training, bs, which in itertools.product(case.modes, C.BATCH_SIZES, ("pairs", "graph")):
        want, _, margin = C.reference(name, training, bs, torch.float64, which)
        got = C.reference(name, training, bs, torch.float32, which)[0]
        rel = C.rel_error(got, want)
        within, q99, worst = C.figures(got, want)
        print(f"{name} train={training} bs={bs} {which}: float32 torch leaves {int((rel > C.TOL).sum())} outside {C.TOL}, "
              f"q99 {q99:.3e}, max {worst:.3e}; smallest |ReLU pre-activation| {margin.min():.2e}")
        assert int((rel > C.TOL).sum()) == 0, (training, bs, which, worst)
        assert q99 <= case.f32_q99, (training, bs, which, q99)
        assert margin.shape == want.shape and np.all(margin > 0)
        if C.descriptor(case, training).bn_train:
            assert margin.min() >= C.RELU_MARGIN, (training, bs, which, float(margin.min()), int(margin.argmin()) // bs)


# ---------------------------------------------------------------- routes

@pytest.mark.parametrize("name", list(C.CASES))
def test_every_case_takes_the_route_it_names(lib, name):
    case = C.CASES[name]
    for training in case.modes:
        desc = C.descriptor(case, training)
        for bs in C.BATCH_SIZES:
            assert C.route_of(lib, desc, 0, C.E, bs, False) == case.pairs_route[training]
            assert C.route_of(lib, desc, C.N_NODES, C.N_EDGES, bs, True) == case.graph_route[training]
            assert lib.geo_jvp_head_stream(desc, 0, C.E, bs, 0) == case.head_stream[training]


def test_the_descriptor_of_a_case_is_the_export_s(lib):
    """descriptor(case) -- what the route tests ask geo_jvp_plan about -- carries the integers DecoderExport reads off the
    module build() returns, in every mode."""
    from vqvae_amd.spatial_decoder import hip_kernels_cover
    fields = ("latent_dim", "c0", "c1", "c2", "out_channels", "out_size", "norm", "bn_train", "groups1", "groups2",
              "update_running")
    for name, case in C.CASES.items():
        for training in case.modes:
            m = C.build(name).train(training)
            assert hip_kernels_cover(m), name
            a, b = C.descriptor(case, training), module_descriptor(m)
            assert [getattr(a, f) for f in fields[:-1]] == [getattr(b, f) for f in fields[:-1]], (name, training)
            tracked = getattr(m.deconv_layers[1], "running_mean", None) is not None
            assert a.update_running == int(bool(a.bn_train) and tracked), (name, training)
