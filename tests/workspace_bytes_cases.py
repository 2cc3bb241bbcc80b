"""The grid of arguments on which tests/golden/workspace_bytes.json pins the *_workspace_bytes answers of the graph-build,
clustering, shortest-path and model-side sources (tools/gen_golden_workspace_bytes.py records it,
test_workspace_bytes_host.py recomputes it): every alignment boundary of every layout, the kNN filter's size thresholds, the
largest n each signature admits and one zero and one negative argument per query; for the decoder JVP also the route or status
geo_jvp_plan_part answers around each queried size.  Host arithmetic only -- `lib` is any ctypes handle with the signatures
of vqvae_amd/_lib.py applied."""
import jvp_plan_cases as J
import prior_cases
from vqvae_amd import _lib

I31, I27 = 2 ** 31 - 1, 2 ** 27 - 1
N = (1, 2, 255, 256, 257, 4095, 4096, 12288, 12289, 16383, 16384, 19999, 20000, 39999, 40000, 79999, 80000, 199999, 200000,
     1000000)
D = (1, 7, 8, 9, 16, 17, 32, 33, 64, 65, 128)
M = (0, 1, 127, 128, 129, 5000, 1000000)
KNN = (1, 5, 15, 64)                     # k of the kNN graph
E = (0, 1, 7, 1000)
SOURCES = (1, 31, 32, 512)
K = (1, 2, 16, 64)                       # cells / codebook sizes, plus the largest admitted
FEATURE_K_MAX = 4096
KNN_FILTER = (0, 1, 2)                   # the option the knn queries read (filter_applies)


def nnz_of(n):
    return (0, 1, 16 * n)


def common_cases():
    """[(query, args)] of the queries that read no option."""
    out = []
    for n in N + (I31,):
        out += [("geo_kpp_workspace_bytes", (n,)), ("geo_cc_workspace_bytes", (n,)), ("geo_csr_compact_workspace_bytes", (n,))]
        out += [("geo_symmetrize_workspace_bytes", (n, k)) for k in KNN]
        out += [("geo_csr_insert_workspace_bytes", (n, e)) for e in E]
        out += [("geo_nearest_foreign_workspace_bytes", (n, d)) for d in D]
        out += [("geo_bridge_components_workspace_bytes", (n, d, c)) for d in D for c in (1, 2, 3, 1000, n)]
        out += [("geo_feature_workspace_bytes", (n, k)) for k in K + (FEATURE_K_MAX,)]
        for nnz in nnz_of(n):
            out.append(("geo_sssp_nearest_workspace_bytes", (n, nnz)))
            out += [("geo_sssp_workspace_bytes", (n, nnz, s)) for s in SOURCES]
    for n in N + (I27,):
        for nnz in nnz_of(n):
            for k in K + (n,):
                for max_cell in (0, 1, 4096, n):
                    out.append(("geo_cell_costs_workspace_bytes", (n, nnz, k, max_cell)))
                    out.append(("geo_cell_costs_min_workspace_bytes", (n, nnz, k, max_cell)))
    # degenerate: one zero and one negative argument per query
    out += [("geo_kpp_workspace_bytes", (0,)), ("geo_kpp_workspace_bytes", (-1,)),
            ("geo_cc_workspace_bytes", (0,)), ("geo_cc_workspace_bytes", (-1,)),
            ("geo_csr_compact_workspace_bytes", (0,)), ("geo_csr_compact_workspace_bytes", (-1,)),
            ("geo_symmetrize_workspace_bytes", (0, 5)), ("geo_symmetrize_workspace_bytes", (256, 0)),
            ("geo_symmetrize_workspace_bytes", (256, -1)), ("geo_symmetrize_workspace_bytes", (-1, 5)),
            ("geo_csr_insert_workspace_bytes", (0, 7)), ("geo_csr_insert_workspace_bytes", (256, -1)),
            ("geo_nearest_foreign_workspace_bytes", (0, 16)), ("geo_nearest_foreign_workspace_bytes", (256, -1)),
            ("geo_bridge_components_workspace_bytes", (256, 16, 0)), ("geo_bridge_components_workspace_bytes", (-1, 16, 2)),
            ("geo_bridge_components_workspace_bytes", (256, 0, 2)),
            ("geo_feature_workspace_bytes", (0, 16)), ("geo_feature_workspace_bytes", (256, -1)),
            ("geo_feature_workspace_bytes", (256, FEATURE_K_MAX + 1)), ("geo_feature_workspace_bytes", (I31 + 1, 16)),
            ("geo_sssp_nearest_workspace_bytes", (0, 16)), ("geo_sssp_nearest_workspace_bytes", (256, -1)),
            ("geo_sssp_workspace_bytes", (0, 16, 32)), ("geo_sssp_workspace_bytes", (256, 16, 0)),
            ("geo_sssp_workspace_bytes", (256, -1, 32)), ("geo_sssp_workspace_bytes", (-1, 16, 32)),
            ("geo_cell_costs_workspace_bytes", (0, 16, 2, 1)), ("geo_cell_costs_workspace_bytes", (256, -1, 2, 1)),
            ("geo_cell_costs_workspace_bytes", (256, 16, 0, 1)), ("geo_cell_costs_workspace_bytes", (256, 16, 2, -1)),
            ("geo_cell_costs_min_workspace_bytes", (0, 16, 2, 1)), ("geo_cell_costs_min_workspace_bytes", (256, -1, 2, 1))]
    return out


def knn_cases():
    """[(query, args)] of the queries that read the knn_filter option."""
    out = []
    for n in N + (I31,):
        for d in D:
            out += [("geo_knn_workspace_bytes", (n, d)), ("geo_knn_query_min_workspace_bytes", (n, d))]
            out += [("geo_knn_query_workspace_bytes", (n, m, d)) for m in (M if d in (7, 16) else (0, 129, 1000000))]
    out += [("geo_knn_workspace_bytes", (0, 16)), ("geo_knn_workspace_bytes", (256, -1)),
            ("geo_knn_query_min_workspace_bytes", (0, 16)), ("geo_knn_query_min_workspace_bytes", (256, -1)),
            ("geo_knn_query_workspace_bytes", (0, 5, 16)), ("geo_knn_query_workspace_bytes", (256, -1, 16)),
            ("geo_knn_query_workspace_bytes", (256, 5, 0))]
    return out


def answers(lib, cases):
    """{"query": {"a,b,c": bytes}}"""
    out = {}
    for name, args in cases:
        out.setdefault(name, {})[",".join(map(str, args))] = int(getattr(lib, name)(*args))
    return out


# ---- the model side: decoder JVP and metric tensor, vanilla pull-back, k-means, vector quantizer, prior sampling.  A case is
# (query, descriptor, args): the descriptor is a key of model_descriptors() and goes first in the call, "" for a query without one.
JVP_NODES = (0, 1, 127, 128, 129, 3000, 60000)
JVP_BATCH = (1, 100, 128, 512)
JVP_TILE, JVP_PASS_SLOTS = 32, 1 << 20   # jvp.hip's TS and MAX_SLOTS_PER_PASS
# the options that enter make_route's byte decisions: (name, default, the other settings), varied one at a time
JVP_OPTIONS = (("jvp_node_jacobian", 1, (0, 2)), ("jvp_per_node", 1, (0,)), ("jvp_mid", 0, (2, 3)), ("jvp_back_valu", 0, (1,)))
ROUTE_WS = ("0", "edges", "edges-1", "pairs", "pairs-1", "pairs+1")      # the ws_bytes geo_jvp_plan_part is asked about
VANILLA = {f"vanilla_c{c1}_{size}px_{co}ch": (16, c1, c1 // 2, co, size) for c1 in (128, 64) for size in (28, 32) for co in (1, 3)}
VANILLA_EDGES = (0, 1, 2047, 2048, 2049, 10 ** 6)
KM_N_END, KM_D_MAX, KM_K_MAX, KM_L_MAX = 2 ** 31 - 1024, 128, 4096, 64     # kmeans.hip: n < 2^31 - CHUNK, MAX_D, MAX_K, MAX_TRIALS
PRIOR_B = (1, 3, 100)


def model_descriptors():
    """{name: ctypes descriptor}: integers only -- no query reads device memory.  "null" is the null pointer."""
    out = {"null": None}
    out.update({name: J.descriptor(name) for name in J.DECODERS})
    for name, (d, c1, c2, co, size) in VANILLA.items():
        out[name] = _lib.VanillaDecoderDesc(latent_dim=d, c1=c1, c2=c2, out_channels=co, out_size=size)
    for name, cfg in prior_cases.DECODE_SHAPES.items():
        out["prior_" + name] = _lib.PriorDesc(**cfg)
    return out


def jvp_edge_counts(batch):
    """0, 1, around one chunk, and the count that fills exactly one pass of 2^20 slots, plus one."""
    full = JVP_PASS_SLOTS // (2 * -(-batch // JVP_TILE) * JVP_TILE) * batch
    return tuple(dict.fromkeys((0, 1, batch - 1, batch, batch + 1, full, full + 1)))


def jvp_cases():
    """The spatial decoder's size queries: the cases that are recorded once per setting of JVP_OPTIONS."""
    out = []
    for dn, dec in J.DECODERS.items():
        d = dec[0]
        for bs in JVP_BATCH:
            for e in jvp_edge_counts(bs):
                out.append(("geo_jvp_workspace_bytes", dn, (e, bs)))
                for n in JVP_NODES:
                    out.append(("geo_jvp_edges_workspace_bytes", dn, (n, e, bs)))
                    out.append(("geo_jvp_edges_part_workspace_bytes", dn, (n, e, e, bs)))
                    if 4 * e < 3 * n * d <= 16 * e:      # the edges-per-latent rule holds for the build, not for the part
                        out.append(("geo_jvp_edges_part_workspace_bytes", dn, (n, e, 4 * e, bs)))
        out += [("geo_metric_tensor_workspace_bytes", dn, (n,)) for n in JVP_NODES]
        out.append(("geo_metric_tensor_min_workspace_bytes", dn, ()))
    dn = "fm_bn_eval"
    out += [("geo_jvp_workspace_bytes", "null", (2048, 512)), ("geo_jvp_workspace_bytes", dn, (2048, 0)),
            ("geo_jvp_workspace_bytes", dn, (-1, 512)),
            ("geo_jvp_edges_workspace_bytes", "null", (3000, 2048, 512)), ("geo_jvp_edges_workspace_bytes", dn, (3000, 2048, 0)),
            ("geo_jvp_edges_workspace_bytes", dn, (-1, 2048, 512)),
            ("geo_jvp_edges_part_workspace_bytes", "null", (3000, 2048, 2048, 512)),
            ("geo_jvp_edges_part_workspace_bytes", dn, (3000, 2048, 2048, 0)),
            ("geo_jvp_edges_part_workspace_bytes", dn, (3000, 2048, 2047, 512)),
            ("geo_jvp_edges_part_workspace_bytes", dn, (3000, -1, 2048, 512)),
            ("geo_metric_tensor_workspace_bytes", "null", (3000,)), ("geo_metric_tensor_workspace_bytes", dn, (-1,)),
            ("geo_metric_tensor_min_workspace_bytes", "null", ())]
    return out


def model_cases():
    """The queries that read no option."""
    out = []
    for name in VANILLA:
        for e in VANILLA_EDGES:
            out.append(("geo_vanilla_jvp_workspace_bytes", name, (e,)))
            out += [("geo_vanilla_jvp_edges_workspace_bytes", name, (n, e)) for n in dict.fromkeys((0, 1, 2 * e, 2 * e + 1))]
    name = next(iter(VANILLA))
    out += [("geo_vanilla_jvp_workspace_bytes", "null", (2048,)), ("geo_vanilla_jvp_workspace_bytes", name, (-1,)),
            ("geo_vanilla_jvp_edges_workspace_bytes", "null", (100, 2048)), ("geo_vanilla_jvp_edges_workspace_bytes", name, (-1, 2048)),
            ("geo_vanilla_jvp_edges_workspace_bytes", name, (100, -1))]
    for n in N:
        for d in D:
            for k in K + (KM_K_MAX,):
                out.append(("geo_vq_workspace_bytes", "", (n, d, k)))
                out += [("geo_kmeans_workspace_bytes", "", (n, d, k, s, l)) for s in (1, 3) for l in (1, 2, KM_L_MAX)]
    for n, d, k in ((0, 16, 16), (KM_N_END - 1, 16, 16), (KM_N_END, 16, 16), (-1, 16, 16), (4096, 0, 16), (4096, KM_D_MAX + 1, 16),
                    (4096, -1, 16), (4096, 16, 0), (4096, 16, KM_K_MAX + 1), (4096, 16, -1)):
        out += [("geo_vq_workspace_bytes", "", (n, d, k)), ("geo_kmeans_workspace_bytes", "", (n, d, k, 1, 1))]
    out += [("geo_kmeans_workspace_bytes", "", (4096, 16, 16, s, l)) for s, l in ((0, 1), (2, 1), (-1, 1), (1, 0), (1, KM_L_MAX - 1),
                                                                                  (1, KM_L_MAX + 1), (1, -1))]
    for name, cfg in prior_cases.DECODE_SHAPES.items():
        out += [("geo_prior_sample_workspace_bytes", "prior_" + name, (b, s)) for b in PRIOR_B
                for s in dict.fromkeys((1, 63, 64, cfg["max_seq_len"]))]
    name = "prior_" + next(iter(prior_cases.DECODE_SHAPES))
    out += [("geo_prior_sample_workspace_bytes", "null", (3, 16)), ("geo_prior_sample_workspace_bytes", name, (0, 16)),
            ("geo_prior_sample_workspace_bytes", name, (3, 0)), ("geo_prior_sample_workspace_bytes", name, (-1, 16))]
    return out


def model_answers(lib, cases, descs):
    """{"query": {"descriptor": [answers in the order of `cases`]}}: the arguments are the grid's, not the file's."""
    out = {}
    for name, desc, args in cases:
        call = args if desc == "" else (descs[desc],) + args
        out.setdefault(name, {}).setdefault(desc, []).append(int(getattr(lib, name)(*call)))
    return out


def jvp_routes(lib, descs):
    """{"decoder/size/graph_edges": [geo_jvp_plan_part's route code or status for each ws_bytes of ROUTE_WS]}"""
    out = {}
    for dn in J.DECODERS:
        for sn, (n_nodes, n_edges, bs) in J.SIZES.items():
            edges = int(lib.geo_jvp_edges_workspace_bytes(descs[dn], n_nodes, n_edges, bs))
            pairs = int(lib.geo_jvp_workspace_bytes(descs[dn], n_edges, bs))
            ws = (0, edges, edges - 1, pairs, pairs - 1, pairs + 1)
            for graph in (0, 1):
                out[f"{dn}/{sn}/{graph}"] = [int(lib.geo_jvp_plan_part(descs[dn], n_nodes, n_edges, n_edges, bs, graph, max(w, 0)))
                                             for w in ws]
    return out


def model_sizes(lib):
    """{"defaults": every model-side answer, "option=value": the decoder JVP's under that one option changed}.  Restores the options."""
    descs = model_descriptors()
    jvp = lambda: dict(model_answers(lib, jvp_cases(), descs), geo_jvp_plan_part=jvp_routes(lib, descs))  # noqa: E731
    doc = {"defaults": dict(model_answers(lib, model_cases(), descs), **jvp())}
    for option, default, others in JVP_OPTIONS:
        try:
            for v in others:
                assert lib.geo_set_option(option.encode(), v) == 0
                doc[f"{option}={v}"] = jvp()
        finally:
            lib.geo_set_option(option.encode(), default)
    return doc


def pack_model(model):
    """How the golden file keeps model_sizes(): "defaults" whole, every other setting as what it changes,
    {"query": {"descriptor": {"position in the defaults' list": answer}}} -- an option moves few answers."""
    base = model["defaults"]
    out = {"defaults": base}
    for setting, queries in model.items():
        if setting != "defaults":
            changed = {q: {d: {str(i): a for i, (a, b) in enumerate(zip(v, base[q][d], strict=True)) if a != b}
                           for d, v in by_desc.items()} for q, by_desc in queries.items()}
            out[setting] = {q: {d: c for d, c in by_desc.items() if c} for q, by_desc in changed.items()}   # no entry: as the defaults
    return out


def unpack_model(packed):
    """pack_model() undone: every setting as whole lists."""
    base = packed["defaults"]
    out = {"defaults": base}
    for setting, queries in packed.items():
        if setting != "defaults":
            out[setting] = {q: {d: [by_desc.get(d, {}).get(str(i), b) for i, b in enumerate(v)] for d, v in base[q].items()}
                            for q, by_desc in queries.items()}
    return out


def model_queries():
    return {q for q, _, _ in model_cases() + jvp_cases()} | {"geo_jvp_plan_part"}


def sizes(lib):
    """The whole grid.  Sets and restores the knn_filter option (default 1) and the decoder JVP's."""
    doc = {"common": answers(lib, common_cases()), "knn_filter": {}}
    try:
        for f in KNN_FILTER:
            assert lib.geo_set_option(b"knn_filter", f) == 0
            doc["knn_filter"][str(f)] = answers(lib, knn_cases())
    finally:
        lib.geo_set_option(b"knn_filter", 1)
    doc["model"] = model_sizes(lib)
    return doc
