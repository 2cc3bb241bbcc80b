"""The grid of arguments on which tests/golden/workspace_bytes.json pins the *_workspace_bytes answers of the graph-build,
clustering and shortest-path sources (tools/gen_golden_workspace_bytes.py records it, test_workspace_bytes_host.py recomputes
it): every alignment boundary of every layout, the kNN filter's size thresholds, the largest n each signature admits and one
zero and one negative argument per query.  Host arithmetic only -- `lib` is any ctypes handle with the signatures of
vqvae_amd/_lib.py applied."""

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


def sizes(lib):
    """The whole grid.  Sets and restores the knn_filter option (default 1)."""
    doc = {"common": answers(lib, common_cases()), "knn_filter": {}}
    try:
        for f in KNN_FILTER:
            assert lib.geo_set_option(b"knn_filter", f) == 0
            doc["knn_filter"][str(f)] = answers(lib, knn_cases())
    finally:
        lib.geo_set_option(b"knn_filter", 1)
    return doc
