"""The decoder-JVP route on the host: geo_jvp_plan (the decision geo_decoder_jvp_edges / _pairs make, host arithmetic only) for
every decoder family the kernels serve or refuse, and the two workspace queries against the sizes recorded from the library
before the route was gathered into one function."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_plan_cases as C  # noqa: E402

E_ARG, E_WORKSPACE = -1, -2


@pytest.fixture()
def lib(request):
    from vqvae_amd import _lib
    L = _lib.load()
    defaults = {b"jvp_mid": 0, b"jvp_back_valu": 0, b"jvp_front_valu": 0, b"jvp_per_node": 1, b"jvp_node_jacobian": 1,
                b"jvp_start_dedup": 1}
    request.addfinalizer(lambda: [L.geo_set_option(k, v) for k, v in defaults.items()])
    return L


def plan(lib, decoder, size, graph, ws_bytes=0):
    n_nodes, n_edges, bs = C.SIZES[size]
    return lib.geo_jvp_plan(C.descriptor(decoder), n_nodes, n_edges, bs, int(graph), ws_bytes)


def route(lib, decoder, size, graph, ws_bytes=0):
    from vqvae_amd import _lib
    code = plan(lib, decoder, size, graph, ws_bytes)
    assert code >= 0, (decoder, size, lib.geo_last_error())
    r = _lib.decode_jvp_plan(code)
    flags = tuple(f for f in ("per_node", "node_jacobian", "dedup") if r[f])
    return (f"{r['front']}{r['dmax']}", r["mid"], r["back"]) + flags


def test_workspace_queries_answer_as_before_the_route_refactor(lib):
    """tests/golden/jvp_workspace_bytes.json: geo_jvp_workspace_bytes / geo_jvp_edges_workspace_bytes of commit f2f6d45 (the
    parent of the route refactor; its libgeo_hip.so loaded with ctypes, jvp_plan_cases.workspace_sizes) with default options.
    The workspace layout did not change: a difference here is a mistake in make_route, not a number to update."""
    want = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "jvp_workspace_bytes.json")))
    got = C.workspace_sizes(lib)
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if v != want[k]} == {}
    assert want["out_size_64/small"] == [0, 0] and min(want["c1_48/dense"]) > 0      # refused by the run, sized by the queries
    assert want["fm_bn_eval/dense"][1] > want["fm_bn_eval/sparse"][1] > want["fm_bn_eval/sparse"][0]


def test_header_constants_are_the_binding_s_names():
    import re
    from vqvae_amd import _lib
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "geo_hip.h")).read()
    defs = {k: int(v, 0) for k, v in re.findall(r"#define (GEO_JVP_[A-Z_]+) (0x[0-9a-f]+|\d+)\b", text)}
    for kind, names in (("FRONT", _lib.JVP_FRONT), ("MID", _lib.JVP_MID), ("BACK", _lib.JVP_BACK)):
        assert [defs[f"GEO_JVP_{kind}_{n.upper()}"] for n in names] == list(range(len(names)))
    assert (defs["GEO_JVP_PER_NODE"], defs["GEO_JVP_NODE_JACOBIAN"], defs["GEO_JVP_DEDUP"]) == (0x1000, 0x2000, 0x4000)
    assert _lib.decode_jvp_plan(1 | 2 << 2 | 3 << 4 | 1 << 8 | 0x1000 | 5 << 16) == {
        "front": "mfma", "dmax": 64, "mid": "all_tangent", "back": "per_node", "per_node": True, "node_jacobian": False,
        "dedup": False, "passes": 5}


def test_default_decoder_train_mode_batchnorm(lib):
    assert route(lib, "fm_bn_train", "small", graph=False) == ("valu16", "pipe", "mfma")
    assert route(lib, "fm_bn_train", "small", graph=True) == ("valu16", "pipe_dedup", "dedup", "dedup")
    assert route(lib, "cf32_bn_train", "dense", graph=True) == ("mfma32", "pipe_dedup", "dedup", "dedup")
    assert route(lib, "cf64_bn_train", "dense", graph=True) == ("mfma64", "pipe_dedup", "dedup", "dedup")
    assert route(lib, "cf64_bn_train", "dense", graph=False) == ("mfma64", "pipe", "mfma")
    lib.geo_set_option(b"jvp_start_dedup", 0)
    assert route(lib, "fm_bn_train", "small", graph=True) == ("valu16", "pipe", "mfma")
    lib.geo_set_option(b"jvp_start_dedup", 1)
    lib.geo_set_option(b"jvp_front_valu", 1)
    assert route(lib, "cf64_bn_train", "dense", graph=True) == ("valu64", "pipe_dedup", "dedup", "dedup")


def test_default_decoder_fixed_statistics(lib):
    from vqvae_amd import _lib
    for dec in ("fm_bn_eval", "fm_none"):
        assert route(lib, dec, "small", graph=False) == ("valu16", "pipe", "mfma")
        # 4 E >= 3 N d: the per-latent Jacobian; fewer edges per latent, or d > 16: the per-node primal alone
        assert route(lib, dec, "dense", graph=True) == ("valu16", "all_tangent", "per_node", "per_node", "node_jacobian")
        assert route(lib, dec, "sparse", graph=True) == ("valu16", "all_tangent", "per_node", "per_node")
        # more latents than a pass has slots: per edge end
        assert route(lib, dec, "few_edges", graph=True) == ("valu16", "pipe", "mfma")
    assert route(lib, "cf32_bn_eval", "small", graph=False) == ("mfma32", "pipe", "mfma")
    assert route(lib, "cf32_bn_eval", "dense", graph=True) == ("mfma32", "all_tangent", "per_node", "per_node")
    # a workspace of geo_jvp_workspace_bytes() only: the call works and takes the per-edge-end path
    n_nodes, n_edges, bs = C.SIZES["sparse"]
    small_ws = lib.geo_jvp_workspace_bytes(C.descriptor("fm_bn_eval"), n_edges, bs)
    assert route(lib, "fm_bn_eval", "sparse", graph=True, ws_bytes=small_ws) == ("valu16", "pipe", "mfma")
    assert plan(lib, "fm_bn_eval", "sparse", graph=True, ws_bytes=small_ws - 1) == E_WORKSPACE
    assert b"workspace" in lib.geo_last_error()
    # ... unless the Jacobian route (passes over N d / 2 pseudo-edges) needs less than the per-edge-end passes over E edges
    n_nodes, n_edges, bs = C.SIZES["dense"]
    small_ws = lib.geo_jvp_workspace_bytes(C.descriptor("fm_bn_eval"), n_edges, bs)
    assert route(lib, "fm_bn_eval", "dense", graph=True, ws_bytes=small_ws)[-1] == "node_jacobian"
    # room for the per-node buffers but not for the Jacobian's columns
    lib.geo_set_option(b"jvp_node_jacobian", 2)
    n_nodes, n_edges, bs = C.SIZES["sparse"]
    full_ws = lib.geo_jvp_edges_workspace_bytes(C.descriptor("fm_bn_eval"), n_nodes, n_edges, bs)
    assert route(lib, "fm_bn_eval", "sparse", graph=True, ws_bytes=full_ws)[-1] == "node_jacobian"
    assert route(lib, "fm_bn_eval", "sparse", graph=True, ws_bytes=full_ws - 1) == ("valu16", "all_tangent", "per_node", "per_node")
    # the options of the A/B tests
    lib.geo_set_option(b"jvp_node_jacobian", 2)
    assert route(lib, "fm_bn_eval", "sparse", graph=True) == ("valu16", "all_tangent", "per_node", "per_node", "node_jacobian")
    assert route(lib, "cf32_bn_eval", "dense", graph=True) == ("mfma32", "all_tangent", "per_node", "per_node")
    lib.geo_set_option(b"jvp_node_jacobian", 0)
    assert route(lib, "fm_bn_eval", "dense", graph=True) == ("valu16", "all_tangent", "per_node", "per_node")
    lib.geo_set_option(b"jvp_per_node", 0)
    assert route(lib, "fm_bn_eval", "dense", graph=True) == ("valu16", "pipe", "mfma")
    # the C2 graph: two passes over the edge ends per edge end, one over the Jacobian's pseudo-edges
    assert _lib.decode_jvp_plan(plan(lib, "fm_bn_train", "c2", graph=True))["passes"] == 2
    lib.geo_set_option(b"jvp_per_node", 1)
    lib.geo_set_option(b"jvp_node_jacobian", 1)
    assert _lib.decode_jvp_plan(plan(lib, "fm_bn_eval", "c2", graph=True))["passes"] == 1


def test_default_decoder_groupnorm(lib):
    assert route(lib, "fm_group", "small", graph=False) == ("valu16", "all", "mfma")
    assert route(lib, "cf32_group", "small", graph=False) == ("mfma32", "all", "mfma")
    assert route(lib, "fm_group", "dense", graph=True) == ("valu16", "all_tangent", "per_node", "per_node", "node_jacobian")
    assert route(lib, "fm_group", "sparse", graph=True) == ("valu16", "all_tangent", "per_node", "per_node")
    assert route(lib, "cf32_group", "dense", graph=True) == ("mfma32", "all_tangent", "per_node", "per_node")


def test_other_widths(lib):
    for dec in ("c1_64_bn_train", "c1_32_bn_train"):             # c2 = 64: one tile per workgroup; no dedup (not the pipeline)
        for graph in (False, True):
            assert route(lib, dec, "dense", graph) == ("valu16", "all", "mfma")
    for dec in ("c2_32_bn_train", "c2_32_bn_eval", "c2_128_bn_train", "small_bn_train"):
        for graph in (False, True):
            assert route(lib, dec, "dense", graph) == ("valu16", "chunk", "valu")
    for dec in ("px32_1ch_bn_train", "px32_1ch_bn_eval"):         # 64 outputs: the VALU ConvT3, hence no dedup and no per_node
        for graph in (False, True):
            assert route(lib, dec, "dense", graph) == ("valu16", "pipe", "valu")


def test_options_select_the_other_live_kernels(lib):
    lib.geo_set_option(b"jvp_mid", 2)
    assert route(lib, "fm_bn_train", "small", graph=True) == ("valu16", "chunk", "mfma")
    assert route(lib, "fm_bn_eval", "dense", graph=True) == ("valu16", "chunk", "mfma")
    lib.geo_set_option(b"jvp_mid", 3)
    assert route(lib, "fm_bn_train", "small", graph=True) == ("valu16", "all", "mfma")
    assert route(lib, "fm_bn_eval", "dense", graph=True) == ("valu16", "all_tangent", "per_node", "per_node", "node_jacobian")
    lib.geo_set_option(b"jvp_mid", 1)                             # the exact-f32 kernel is gone: selects nothing
    assert route(lib, "fm_bn_train", "small", graph=True) == ("valu16", "pipe_dedup", "dedup", "dedup")
    lib.geo_set_option(b"jvp_mid", 0)
    lib.geo_set_option(b"jvp_back_valu", 1)
    assert route(lib, "fm_bn_train", "small", graph=True) == ("valu16", "pipe", "valu")
    assert route(lib, "fm_bn_eval", "dense", graph=True) == ("valu16", "pipe", "valu")
    assert lib.geo_set_option(b"jvp_pipe_grid", 2) == E_ARG       # removed with the measurement that it changes nothing


@pytest.mark.parametrize("decoder,message", [
    ("c2_128_3ch32", b"decoder too wide for the back kernel"),
    ("px32_1ch_group", b"GroupNorm needs 32 groups per layer and dec_channels[2] == 64 (got 32/32 groups, c2=64)"),
    ("group_c2_32", b"GroupNorm needs 32 groups per layer and dec_channels[2] == 64 (got 32/32 groups, c2=32)"),
    ("group_16_groups", b"GroupNorm needs 32 groups per layer and dec_channels[2] == 64 (got 16/32 groups, c2=64)"),
    ("out_size_64", b"unsupported decoder (out_size 64, c2=64 must divide 128)"),
    ("c1_48", b"dec_channels[1]=48 not in {32,64,128}"),
])
def test_refused_decoders_report_the_run_s_verdict(lib, decoder, message):
    """`px32_1ch_group`: GroupNorm with a 64-output head has no matrix-core ConvT3.  spatial_decoder.hip_kernels_cover()
    refuses it as the library does (test_jvp_envelope_host.py sweeps the predicate against geo_jvp_plan)."""
    for graph in (False, True):
        assert plan(lib, decoder, "dense", graph) == E_ARG
        assert message in lib.geo_last_error()


# (n_nodes, E) of k = 20 union graphs over Gaussian latents (14 to 16 edges per latent; the last near the C2 graph), then a graph
# one edge below 0.75 d edges per latent (d = 16: 12) and one exactly on it
BUILD_GRAPHS = [(512, 7350), (2048, 30354), (60000, 948000), (512, 6143), (512, 6144)]
PART_BS = 512


def part_plan(lib, decoder, n_nodes, n_edges, build_edges):
    from vqvae_amd import _lib
    code = lib.geo_jvp_plan_part(C.descriptor(decoder), n_nodes, n_edges, build_edges, PART_BS, 1, 0)
    assert code >= 0, (decoder, n_nodes, n_edges, build_edges, lib.geo_last_error())
    return _lib.decode_jvp_plan(code)


def rank_slices(n_edges, world):
    from vqvae_amd import parallel
    out = [parallel.chunk_range(n_edges, PART_BS, rank, world) for rank in range(world)]
    assert out[0][0] == 0 and out[-1][1] == n_edges and all(a[1] == b[0] for a, b in zip(out, out[1:]))
    return [(e0, e1) for e0, e1 in out if e1 > e0]


@pytest.mark.parametrize("n_nodes,n_edges", BUILD_GRAPHS)
@pytest.mark.parametrize("decoder", ["fm_bn_eval", "fm_none", "fm_group"])
def test_every_part_of_a_build_takes_the_route_of_the_whole(lib, decoder, n_nodes, n_edges):
    """Fixed statistics, d = 16: a rank's share of the edges, told the build's edge count (geo_jvp_plan_part), carries the
    node_jacobian flag of the whole graph for every world size; asked about its own edges alone (geo_jvp_plan) at least one
    rank of two answers differently -- these graphs sit where a sharded build used to leave the single-process route."""
    from vqvae_amd import _lib
    desc = C.descriptor(decoder)
    whole = _lib.decode_jvp_plan(lib.geo_jvp_plan(desc, n_nodes, n_edges, PART_BS, 1, 0))
    assert whole["node_jacobian"] == (4 * n_edges >= 3 * n_nodes * 16) and whole["per_node"]
    assert part_plan(lib, decoder, n_nodes, n_edges, n_edges) == whole
    for world in (1, 2, 3, 8):
        alone = []
        for e0, e1 in rank_slices(n_edges, world):
            part = part_plan(lib, decoder, n_nodes, e1 - e0, n_edges)
            assert part["node_jacobian"] == whole["node_jacobian"], (world, e0, e1)
            assert part["per_node"] and (part["front"], part["mid"], part["back"]) == (whole["front"], whole["mid"], whole["back"])
            alone.append(_lib.decode_jvp_plan(lib.geo_jvp_plan(desc, n_nodes, e1 - e0, PART_BS, 1, 0))["node_jacobian"])
            # the workspace is the call's own: what the part query sizes is what the part plan assumes, and enough for the run
            ws = lib.geo_jvp_edges_part_workspace_bytes(desc, n_nodes, e1 - e0, n_edges, PART_BS)
            assert ws > 0 and _lib.decode_jvp_plan(lib.geo_jvp_plan_part(desc, n_nodes, e1 - e0, n_edges, PART_BS, 1, ws)) == part
        if world == 2 and whole["node_jacobian"]:
            assert not all(alone), alone
        if not whole["node_jacobian"]:
            assert not any(alone), alone
    e0, e1 = rank_slices(n_edges, 2)[0]
    assert lib.geo_jvp_plan_part(desc, n_nodes, e1 - e0, e1 - e0 - 1, PART_BS, 1, 0) == E_ARG
    assert b"build_edges" in lib.geo_last_error()
    assert lib.geo_jvp_edges_part_workspace_bytes(desc, n_nodes, e1 - e0, e1 - e0 - 1, PART_BS) == 0


@pytest.mark.parametrize("n_nodes,n_edges", BUILD_GRAPHS)
@pytest.mark.parametrize("decoder,want", [("cf32_bn_eval", ("all_tangent", "per_node", True, False, False)),
                                          ("fm_bn_train", ("pipe_dedup", "dedup", False, False, True))])
def test_build_edges_changes_nothing_where_the_jacobian_route_does_not_apply(lib, decoder, want, n_nodes, n_edges):
    """d = 32 and train-mode BatchNorm never take the per-latent Jacobian, whatever the build's edge count; train mode keeps
    its start-side dedup.  The plan of a part is the plan of the same call on its own."""
    from vqvae_amd import _lib
    desc = C.descriptor(decoder)
    for world in (1, 2, 3, 8):
        for e0, e1 in rank_slices(n_edges, world):
            part = part_plan(lib, decoder, n_nodes, e1 - e0, n_edges)
            assert (part["mid"], part["back"], part["per_node"], part["node_jacobian"], part["dedup"]) == want
            assert part == _lib.decode_jvp_plan(lib.geo_jvp_plan(desc, n_nodes, e1 - e0, PART_BS, 1, 0))
            assert (lib.geo_jvp_edges_part_workspace_bytes(desc, n_nodes, e1 - e0, n_edges, PART_BS)
                    == lib.geo_jvp_edges_workspace_bytes(desc, n_nodes, e1 - e0, PART_BS))
    assert lib.geo_jvp_plan_part(desc, n_nodes, n_edges, n_edges - 1, PART_BS, 1, 0) == E_ARG


def test_the_plain_queries_are_the_part_queries_with_the_call_s_own_count(lib):
    for dn in ("fm_bn_eval", "fm_group", "fm_bn_train", "cf32_bn_eval", "c1_48"):
        desc = C.descriptor(dn)
        for n_nodes, n_edges, bs in C.SIZES.values():
            assert (lib.geo_jvp_edges_part_workspace_bytes(desc, n_nodes, n_edges, n_edges, bs)
                    == lib.geo_jvp_edges_workspace_bytes(desc, n_nodes, n_edges, bs))
            for graph in (0, 1):
                assert (lib.geo_jvp_plan_part(desc, n_nodes, n_edges, n_edges, bs, graph, 0)
                        == lib.geo_jvp_plan(desc, n_nodes, n_edges, bs, graph, 0))


def test_the_run_entry_refuses_a_build_smaller_than_the_call_before_anything_else(lib):
    """geo_decoder_jvp_edges_part itself, not only its queries: build_edges < n_edges is GEO_E_ARG ahead of every other check --
    with null buffers the answer names build_edges, not the null pointers, and nothing is launched (no GPU here)."""
    desc = C.descriptor("fm_bn_eval")
    for n_edges, build_edges in ((7350, 7349), (512, 0), (1, -1)):
        assert lib.geo_decoder_jvp_edges_part(desc, None, 512, None, None, n_edges, build_edges, 512, None, None, 0, None) == E_ARG
        assert b"build_edges" in lib.geo_last_error(), lib.geo_last_error()
    # a valid count gets as far as the next check
    assert lib.geo_decoder_jvp_edges_part(desc, None, 512, None, None, 7350, 7350, 512, None, None, 0, None) == E_ARG
    assert b"null pointer" in lib.geo_last_error()
    assert lib.geo_decoder_jvp_edges(desc, None, 512, None, None, 7350, 512, None, None, 0, None) == E_ARG
    assert b"null pointer" in lib.geo_last_error()
