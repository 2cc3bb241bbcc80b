"""geo_jvp_head_stream on the host: which calls run ConvT3 with head_stream_kernel (host arithmetic only) for every decoder family
and call size of the route tests, the option behind it by name and by its default, and the symbol's declaration and binding."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_plan_cases as C  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
E_ARG = -1


@pytest.fixture()
def lib(request):
    from vqvae_amd import _lib
    L = _lib.load()
    defaults = {b"jvp_head_stream": 1, b"jvp_start_dedup": 1, b"jvp_back_valu": 0, b"jvp_per_node": 1}
    request.addfinalizer(lambda: [L.geo_set_option(k, v) for k, v in defaults.items()])
    return L


def _expected(lib, decoder, size, graph, option):
    """The rule of the header: the 16-output head (back_nt = 1) without GroupNorm on back route mfma or dedup, option != 0."""
    from vqvae_amd import _lib
    n_nodes, n_edges, bs = C.SIZES[size]
    code = lib.geo_jvp_plan(C.descriptor(decoder), n_nodes, n_edges, bs, int(graph), 0)
    if code < 0:
        return code
    d, _, cout, out_size, norm, _, _ = C.DECODERS[decoder]
    s_out = {28: 4, 32: 8}[out_size]
    outputs = cout * s_out * s_out
    back = _lib.decode_jvp_plan(code)["back"]
    return int(back in ("mfma", "dedup") and outputs <= 32 and norm != 2 and option != 0)


def test_query_follows_the_rule_for_every_decoder_and_size(lib):
    seen = set()
    for option in (1, 0):
        lib.geo_set_option(b"jvp_head_stream", option)
        for decoder in C.DECODERS:
            for size, (n_nodes, n_edges, bs) in C.SIZES.items():
                for graph in (0, 1):
                    want = _expected(lib, decoder, size, graph, option)
                    got = lib.geo_jvp_head_stream(C.descriptor(decoder), n_nodes, n_edges, bs, graph)
                    assert got == want, (decoder, size, graph, option, lib.geo_last_error())
                    seen.add(got)
    assert {0, 1, E_ARG} <= seen


def test_query_on_the_shipped_routes(lib):
    def q(decoder, size, graph):
        n_nodes, n_edges, bs = C.SIZES[size]
        return lib.geo_jvp_head_stream(C.descriptor(decoder), n_nodes, n_edges, bs, int(graph))
    assert q("fm_bn_train", "c2", True) == 1 and q("fm_bn_train", "small", False) == 1       # dedup, mfma
    assert q("fm_bn_eval", "small", False) == 1 and q("fm_none", "few_edges", True) == 1     # fixed statistics per slot
    assert q("fm_bn_eval", "dense", True) == 0 and q("fm_none", "sparse", True) == 0         # per latent
    assert q("fm_group", "small", False) == 0 and q("fm_group", "dense", True) == 0          # GroupNorm
    assert q("cf32_bn_train", "dense", True) == 0 and q("cf64_bn_train", "dense", False) == 0  # 192 outputs
    assert q("px32_1ch_bn_train", "small", True) == 0 and q("c2_32_bn_train", "small", True) == 0   # back_kernel
    assert q("c1_64_bn_train", "small", False) == 1                                          # narrower ConvT2, the same head
    assert q("out_size_64", "small", True) == E_ARG and b"unsupported decoder" in lib.geo_last_error()
    lib.geo_set_option(b"jvp_start_dedup", 0)
    assert q("fm_bn_train", "c2", True) == 1                                                 # route mfma over both sides
    lib.geo_set_option(b"jvp_back_valu", 1)
    assert q("fm_bn_train", "c2", True) == 0
    lib.geo_set_option(b"jvp_back_valu", 0)
    lib.geo_set_option(b"jvp_head_stream", 0)
    assert q("fm_bn_train", "c2", True) == 0 and q("fm_bn_train", "small", False) == 0


def test_option_does_not_change_plan_or_workspace(lib):
    lib.geo_set_option(b"jvp_head_stream", 1)
    on = C.workspace_sizes(lib)
    plans_on = {(d, s, g): lib.geo_jvp_plan(C.descriptor(d), *C.SIZES[s][:2], C.SIZES[s][2], g, 0)
                for d in C.DECODERS for s in C.SIZES for g in (0, 1)}
    lib.geo_set_option(b"jvp_head_stream", 0)
    assert C.workspace_sizes(lib) == on
    assert plans_on == {(d, s, g): lib.geo_jvp_plan(C.descriptor(d), *C.SIZES[s][:2], C.SIZES[s][2], g, 0)
                        for d in C.DECODERS for s in C.SIZES for g in (0, 1)}


def test_unknown_option_is_still_refused(lib):
    assert lib.geo_set_option(b"jvp_head_stream", 0) == 0
    assert lib.geo_set_option(b"jvp_head_streams", 0) == E_ARG
    assert b"unknown option" in lib.geo_last_error()
    assert lib.geo_set_option(b"jvp_head", 1) == E_ARG


_ENV_PROBE = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import jvp_plan_cases as C
from vqvae_amd import _lib
L = _lib.load()
n, e, bs = C.SIZES["c2"]
print(L.geo_jvp_head_stream(C.descriptor("fm_bn_train"), n, e, bs, 1))
"""


@pytest.mark.parametrize("env,want", [(None, 1), ("0", 0), ("1", 1)])
def test_environment_default(env, want):
    """The option is seeded once, when the library is first called: a fresh process per setting."""
    e = {k: v for k, v in os.environ.items() if k != "GEO_JVP_HEAD_STREAM"}
    if env is not None:
        e["GEO_JVP_HEAD_STREAM"] = env
    code = _ENV_PROBE.format(root=os.path.abspath(ROOT), tests=os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout
    assert int(out.strip().splitlines()[-1]) == want


def test_symbol_is_declared_bound_and_exported(lib):
    from vqvae_amd import _lib
    header = open(os.path.join(ROOT, "include", "geo_hip.h")).read()
    assert re.search(r"\bint geo_jvp_head_stream\(const geo_decoder_desc \*dec, int64_t n_nodes, int64_t n_edges, "
                     r"int32_t batch_size,\s*int32_t graph_edges\);", header)
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "geo_jvp_plan" in v and "geo_version" in v)
    restype, argtypes = table["geo_jvp_head_stream"]
    assert restype is ctypes.c_int and len(argtypes) == 5
    assert ctypes.CDLL(_lib.LIB_PATH).geo_jvp_head_stream is not None
    assert lib.geo_version() >= 113
