"""The workspace queries on the host: every *_workspace_bytes answer of the graph-build, clustering, shortest-path and
model-side sources (decoder JVP and metric tensor, vanilla pull-back, k-means, vector quantizer, prior sampling) against
tests/golden/workspace_bytes.json, recorded (tools/gen_golden_workspace_bytes.py) from the library of the last commit whose
queries added their sizes by hand -- for the model side, "model", also the route or status geo_jvp_plan_part answers around
each queried size.  Since then each query measures the layout function its entry point carves (geo::Arena, DESIGN.md
"Workspaces") plus a named reserve; the answers did not change."""
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


def flat_model(doc):
    """{"setting: query(descriptor)": [answers]} and, where a list differs, the grid's arguments name the answer."""
    return {f"{setting}: {q}({d})": v for setting, queries in doc.items() for q, by_desc in queries.items()
            for d, v in by_desc.items()}


def model_arguments():
    """{"query(descriptor)": [args of each answer]} in the order model_answers() keeps."""
    out = {}
    for q, d, args in W.model_cases() + W.jvp_cases():
        out.setdefault(f"{q}({d})", []).append(args)
    return out


def test_every_query_answers_what_the_hand_formulae_answered():
    from vqvae_amd import _lib
    want = flat(golden())
    doc = W.sizes(_lib.load())
    got = flat(doc)
    assert sorted(got) == sorted(want)
    assert {k: (v, want[k]) for k, v in got.items() if v != want[k]} == {}
    # the model side: lists of answers in the grid's order; a difference is reported with its arguments
    want, got, args = flat_model(W.unpack_model(golden()["model"])), flat_model(doc["model"]), model_arguments()
    assert sorted(got) == sorted(want)
    moved = {}
    for k in got:
        assert len(got[k]) == len(want[k]), k
        where = args.get(k.split(": ", 1)[1], W.ROUTE_WS)
        moved.update({f"{k}{where[i]}": (g, w) for i, (g, w) in enumerate(zip(got[k], want[k])) if g != w})
    assert moved == {}


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


def test_the_model_grid_holds_what_it_is_meant_to():
    """Every model-side query is in the file under the defaults, the decoder JVP's under each route option changed alone, and the
    recorded route codes switch at the sizes geo_hip.h names: the edges query, and the pairs query as the least that runs."""
    m = W.unpack_model(golden()["model"])
    settings = ["defaults"] + [f"{o}={v}" for o, _, others in W.JVP_OPTIONS for v in others]
    assert sorted(m) == sorted(settings) and len(settings) == 7
    assert sorted(m["defaults"]) == sorted(W.model_queries()) and len(m["defaults"]) == 11
    jvp = sorted({q for q, _, _ in W.jvp_cases()} | {"geo_jvp_plan_part"})
    assert all(sorted(m[s]) == jvp for s in settings[1:])
    args = model_arguments()
    d = m["defaults"]
    for q, by_desc in d.items():
        if q != "geo_jvp_plan_part":
            assert all(len(v) == len(args[f"{q}({desc})"]) for desc, v in by_desc.items()), q
    assert all(v == 0 for q in d for v in d[q].get("null", [])) and sum("null" in d[q] for q in d) == 8
    at = lambda q, desc, a: d[q][desc][args[f"{q}({desc})"].index(a)]  # noqa: E731
    assert at("geo_jvp_workspace_bytes", "fm_bn_eval", (2048, 0)) == 0 and at("geo_kmeans_workspace_bytes", "", (0, 16, 16, 1, 1)) == 0
    assert at("geo_kmeans_workspace_bytes", "", (W.KM_N_END - 1, 16, 16, 1, 1)) > 2 ** 34
    assert at("geo_kmeans_workspace_bytes", "", (W.KM_N_END, 16, 16, 1, 1)) == 0
    assert at("geo_vq_workspace_bytes", "", (4096, W.KM_D_MAX + 1, 16)) == 0 and at("geo_vq_workspace_bytes", "", (4096, 16, W.KM_K_MAX)) > 0
    # one pass of 2^20 slots is the largest: one edge more adds a pass, not a byte
    full = W.jvp_edge_counts(512)[-2]
    assert at("geo_jvp_workspace_bytes", "fm_bn_train", (full, 512)) == at("geo_jvp_workspace_bytes", "fm_bn_train", (full + 1, 512))
    assert at("geo_jvp_workspace_bytes", "fm_bn_train", (full, 512)) > 12 * 10 ** 9
    # fixed statistics, few edges, the Jacobian route forced: it needs the edges query to the byte; one byte less leaves the
    # per-node route, the pairs query the per-edge-end route, one byte less GEO_E_WORKSPACE
    NODE_JACOBIAN, PER_NODE = 0x2000, 0x1000
    codes = dict(zip(W.ROUTE_WS, m["jvp_node_jacobian=2"]["geo_jvp_plan_part"]["fm_bn_eval/small/1"]))
    assert codes["0"] == codes["edges"] and codes["edges"] & NODE_JACOBIAN and codes["edges"] & PER_NODE
    assert not codes["edges-1"] & NODE_JACOBIAN and codes["edges-1"] & PER_NODE
    assert codes["pairs-1"] == -2 and codes["pairs"] == codes["pairs+1"] >= 0 and not codes["pairs"] & (NODE_JACOBIAN | PER_NODE)
    # by default the route needs enough edges per latent: the dense graph has them, and there the pairs query holds the columns too
    codes = dict(zip(W.ROUTE_WS, d["geo_jvp_plan_part"]["fm_bn_eval/dense/1"]))
    assert all(c & NODE_JACOBIAN for c in codes.values())
    assert not any(c & NODE_JACOBIAN for c in d["geo_jvp_plan_part"]["fm_bn_eval/small/1"] if c >= 0)
    assert not any(c & NODE_JACOBIAN for c in m["jvp_node_jacobian=0"]["geo_jvp_plan_part"]["fm_bn_eval/dense/1"] if c >= 0)
    assert not any(c & PER_NODE for c in m["jvp_per_node=0"]["geo_jvp_plan_part"]["fm_bn_eval/dense/1"] if c >= 0)
