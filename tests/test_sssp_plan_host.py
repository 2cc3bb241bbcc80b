"""Host arithmetic of the multi-source shortest-path driver (no GPU): geo_sssp_plan and geo_sssp_workspace_bytes over a grid of
sizes, against the answers recorded from the commit before the driver was split into phases (one plan, one layout)."""
import pytest

NODES = [1, 2000, 12288, 12289, 60000, (1 << 25) - 1, 1 << 25]
SOURCES = [1, 16, 17, 40, 512, 1024]

# geo_sssp_workspace_bytes(n, 20 n, n_sources) of that commit, rows = NODES, columns = SOURCES: upper bounds from here on
WORKSPACE_BOUND = [
    [15872, 15872, 16128, 16640, 66048, 185856],
    [1868032, 1868032, 1949952, 2032640, 15205120, 30229760],
    [11404800, 11404800, 11908608, 12413184, 93126912, 184858880],
    [11407360, 11407360, 11911424, 12415744, 93135872, 184875008],
    [55634176, 55634176, 58093824, 60554752, 454497280, 901969920],
    [31105102592, 31105102592, 32480834304, 33856566784, 254141449472, 504323399168],
    [31105103872, 31105103872, 32480835584, 33856568064, 254141457152, 504323414784],
]
NEAREST_BOUND = [21248, 2402304, 14665472, 14669056, 71538176, 39997031424, 39997032704]

# geo_sssp_plan(n, n_sources) of that commit per option setting (name, value, default)
_SMALL, _ALL64 = [16, 16, 64, 64, 64, 64], [64] * 6
PLANS = {
    (None, 0, 0): [_SMALL] * 3 + [[16, 16, 64, 3016, 3016, 3016]] * 3 + [_SMALL],
    ("sssp_u32", 0, 1): [_SMALL] * 3 + [[16, 16, 64, 1016, 1016, 1016]] * 2 + [_SMALL] * 2,
    ("sssp_sb", 16, -1): [[16, 16, 1016, 3016, 3016, 3016]] * 6 + [[16] * 6],
    ("sssp_sb", 64, -1): [_ALL64] * 7,
}


def test_workspace_query_never_grows():
    from vqvae_amd import _lib
    lib = _lib.load()
    for i, n in enumerate(NODES):
        for j, s in enumerate(SOURCES):
            got = lib.geo_sssp_workspace_bytes(n, 20 * n, s)
            assert 0 < got <= WORKSPACE_BOUND[i][j], (n, s, got)
        assert 0 < lib.geo_sssp_nearest_workspace_bytes(n, 20 * n) <= NEAREST_BOUND[i], n


@pytest.mark.parametrize("option", list(PLANS), ids=lambda o: f"{o[0]}={o[1]}" if o[0] else "defaults")
def test_plan_answers_are_unchanged(option):
    from vqvae_amd import _lib
    lib = _lib.load()
    name, value, default = option
    if name:
        _lib.check(lib.geo_set_option(name.encode(), value), "geo_set_option")
    try:
        got = [[lib.geo_sssp_plan(n, s) for s in SOURCES] for n in NODES]
    finally:
        if name:
            lib.geo_set_option(name.encode(), default)
    assert got == PLANS[option]
