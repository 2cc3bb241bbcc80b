"""The workspace queries on the host: every *_workspace_bytes answer of the graph-build, clustering and shortest-path sources
against tests/golden/workspace_bytes.json, recorded (tools/gen_golden_workspace_bytes.py) from the library of the last commit
whose queries added their sizes by hand.  Since then each query measures the layout function its entry point carves
(geo::Arena, DESIGN.md "Workspaces") plus a named reserve; the answers did not change."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workspace_bytes_cases as W  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def flat(doc):
    out = {f"{q}({a})": v for q, by_args in doc["common"].items() for a, v in by_args.items()}
    for f, queries in doc["knn_filter"].items():
        out.update({f"knn_filter={f}: {q}({a})": v for q, by_args in queries.items() for a, v in by_args.items()})
    return out


def test_every_query_answers_what_the_hand_formulae_answered():
    from vqvae_amd import _lib
    want = flat(golden())
    got = flat(W.sizes(_lib.load()))
    assert sorted(got) == sorted(want)
    assert {k: (v, want[k]) for k, v in got.items() if v != want[k]} == {}


def test_the_grid_holds_what_it_is_meant_to():
    """Every query of the converted sources is in the file, with the degenerate sentinels and the filter's thresholds."""
    doc = golden()
    assert sorted(doc["common"]) == sorted({q for q, _ in W.common_cases()}) and len(doc["common"]) == 12
    assert sorted(doc["knn_filter"]) == ["0", "1", "2"]
    assert all(sorted(v) == sorted({q for q, _ in W.knn_cases()}) for v in doc["knn_filter"].values())
    c = doc["common"]
    assert c["geo_kpp_workspace_bytes"]["0"] == 4096 and c["geo_cc_workspace_bytes"]["-1"] == 1024
    assert c["geo_sssp_workspace_bytes"]["-1,16,32"] == 0 and c["geo_feature_workspace_bytes"]["256,4097"] == 0
    assert c["geo_cell_costs_workspace_bytes"][f"{W.I27},0,1,0"] > 0 and c["geo_kpp_workspace_bytes"][str(W.I31)] > 2 ** 35
    # the filter's arrays are in the answer from 16 384 rows (d = 64) / 40 000 rows (d = 16) with the option on, never with it off
    off, on = doc["knn_filter"]["0"]["geo_knn_workspace_bytes"], doc["knn_filter"]["1"]["geo_knn_workspace_bytes"]
    assert on["16383,64"] == off["16383,64"] and on["16384,64"] > off["16384,64"]
    assert on["39999,16"] == off["39999,16"] and on["40000,16"] > off["40000,16"]
    assert doc["knn_filter"]["2"] == doc["knn_filter"]["1"]
