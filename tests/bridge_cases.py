"""CPU oracle and cases of the component-bridging tests (tests/test_bridge_host.py, tests/test_gpu_bridge.py).
TEST INFRASTRUCTURE ONLY: numpy, scipy and oracle.knn, nothing from vqvae_amd.

The contract (include/geo_hip.h): the pair key of nodes a != b is oracle.knn.knn_pair_keys(z, lo, hi, form) with
lo = min(a, b) the query row; pairs are ordered by (key, lo, hi); the bridges of a labelling are the edges Kruskal accepts
over all pairs whose ends carry different labels, joining labels -- C - 1 edges, sorted by that order."""
import functools

import numpy as np

from oracle import knn as ok


def key_form(d: int) -> int:
    return 1 if d > 15 else 0


# ------------------------------------------------------------------------------------------------ oracle
def all_cross_pairs(z, labels, form):
    """(key, lo, hi) of every pair lo < hi with different labels."""
    n = len(z)
    lo, hi = np.triu_indices(n, 1)
    m = labels[lo] != labels[hi]
    lo, hi = lo[m].astype(np.int64), hi[m].astype(np.int64)
    return ok.knn_pair_keys(z, lo, hi, form), lo, hi


def _find(par, a):
    while par[a] != a:
        par[a] = par[par[a]]
        a = par[a]
    return a


def kruskal(z, labels, form):
    """(edges int64 [C-1, 2], keys float64 [C-1]) sorted by (key, lo, hi): the contract itself."""
    labels = np.asarray(labels, dtype=np.int64)
    C = int(labels.max()) + 1
    if C == 1:
        return np.empty((0, 2), np.int64), np.empty(0, np.float64)
    key, lo, hi = all_cross_pairs(z, labels, form)
    order = np.lexsort((hi, lo, key))
    par = list(range(C))
    edges, keys = [], []
    for p in order:
        a, b = _find(par, labels[lo[p]]), _find(par, labels[hi[p]])
        if a != b:
            par[a] = b
            edges.append((int(lo[p]), int(hi[p])))
            keys.append(key[p])
            if len(edges) == C - 1:
                break
    assert len(edges) == C - 1
    return np.asarray(edges, np.int64).reshape(-1, 2), np.asarray(keys, np.float64)


def boruvka_skip_largest(z, labels, form):
    """The algorithm of geo_bridge_components restated: rounds in which every component but the currently largest (lowest
    label on ties) takes its (key, lo, hi)-minimum outgoing pair.  Returns (edges, keys) sorted like kruskal's, the rounds and
    the queries (nodes outside the largest component) per round."""
    labels = np.asarray(labels, dtype=np.int64)
    key, lo, hi = all_cross_pairs(z, labels, form)
    order = np.lexsort((hi, lo, key))
    key, lo, hi = key[order], lo[order], hi[order]
    cur = labels.copy()
    out = {}
    rounds, queries = 0, []
    while cur.max() > 0:
        rounds += 1
        C = int(cur.max()) + 1
        sizes = np.bincount(cur, minlength=C)
        big = int(np.argmax(sizes))
        queries.append(int(len(z) - sizes[big]))
        live = cur[lo] != cur[hi]
        best = {}
        for p in np.flatnonzero(live):                  # first hit per component in the total order = its minimum outgoing pair
            for c in (cur[lo[p]], cur[hi[p]]):
                if c != big and c not in best:
                    best[c] = p
            if len(best) == C - 1:
                break
        par = list(range(C))
        for p in sorted(set(best.values())):
            ra, rb = _find(par, cur[lo[p]]), _find(par, cur[hi[p]])
            assert ra != rb, "a round closed a cycle"
            par[max(ra, rb)] = min(ra, rb)
            out[(int(lo[p]), int(hi[p]))] = key[p]
        roots = np.array([_find(par, c) for c in range(C)])
        _, cur = np.unique(roots[cur], return_inverse=True)
    items = sorted(out.items(), key=lambda kv: (kv[1], kv[0][0], kv[0][1]))
    edges = np.asarray([e for e, _ in items], np.int64).reshape(-1, 2)
    keys = np.asarray([k for _, k in items], np.float64)
    return edges, keys, rounds, queries


def nearest_foreign(z, labels, rows, form):
    """(nbr int64 [m], key float64 [m]) by brute force: per query row the node of another label minimising (pair key, index);
    -1 and +inf where there is none."""
    labels = np.asarray(labels)
    rows = np.asarray(rows, dtype=np.int64)
    n = len(z)
    uniq, inv = np.unique(rows, return_inverse=True)
    nbr_u = np.full(len(uniq), -1, np.int64)
    key_u = np.full(len(uniq), np.inf, np.float64)
    allx = np.arange(n, dtype=np.int64)
    for i, q in enumerate(uniq):
        x = allx[labels != labels[q]]
        if x.size == 0:
            continue
        k = ok.knn_pair_keys(z, np.minimum(q, x), np.maximum(q, x), form)
        best = int(np.lexsort((x, k))[0])
        nbr_u[i], key_u[i] = x[best], k[best]
    return nbr_u[inv], key_u[inv]


# ------------------------------------------------------------------------------------------------ cases with a graph
@functools.lru_cache(maxsize=None)
def graph_latents():
    """name -> (z float32 [n, d], k, sym): the five latent sets, drawn in this order from one RandomState(0)."""
    r = np.random.RandomState(0)
    cases = {}
    for d in (5, 16, 32):
        ctr = r.randn(12, d).astype(np.float32) * 4
        z = (ctr[r.randint(0, 12, 600)] + 0.6 * r.randn(600, d)).astype(np.float32)
        cases[f"blobs_d{d}"] = (z, 3, "mutual")
    cases["grid_ties"] = (r.randint(0, 4, size=(300, 6)).astype(np.float32), 2, "mutual")     # equal keys everywhere
    z = np.concatenate([r.randn(900, 16), 30 + 25 * r.randn(40, 16)]).astype(np.float32)
    cases["giant_plus_outliers"] = (z, 5, "mutual")
    return cases


GRAPH_CASES = ("blobs_d5", "blobs_d16", "blobs_d32", "grid_ties", "giant_plus_outliers")
# observed with the oracle's graph builder: (components, largest component)
GRAPH_COMPONENTS = {"blobs_d5": (150, 49), "blobs_d16": (220, 39), "blobs_d32": (244, 36), "grid_ties": (127, 10),
                    "giant_plus_outliers": (243, 583)}


@functools.lru_cache(maxsize=None)
def graph_case(name):
    """dict: z, k, sym, form, W (the oracle's connectivity graph), C, labels, edges / keys (kruskal)."""
    z, k, sym = graph_latents()[name]
    W, _ = ok.build_knn_graph(z, k=k, mode="connectivity", sym=sym)
    C, labels = ok.connected_components(W)
    form = key_form(z.shape[1])
    edges, keys = kruskal(z, labels, form)
    return {"z": z, "k": k, "sym": sym, "form": form, "W": W, "C": C, "labels": np.asarray(labels, np.int32), "edges": edges,
            "keys": keys}


# ------------------------------------------------------------------------------------------------ cases with given labels
LABEL_CASES = ("random7_d16", "random7_d12", "halves_d16", "singletons_d7", "chunks_d40")


@functools.lru_cache(maxsize=None)
def label_case(name):
    """dict: z, labels int32, C, form, edges / keys (kruskal).
    random7_*: n = 1 037 (no multiple of 64), seven random labels; halves: two equal components (the largest is tied, label 0
    stays out of the queries); singletons: C = n = 200, the Euclidean minimum spanning tree, d = 7 (no multiple of 4);
    chunks_d40: two 32-wide chunks per row."""
    r = np.random.RandomState({"random7_d16": 1, "random7_d12": 2, "halves_d16": 3, "singletons_d7": 4, "chunks_d40": 5}[name])
    if name.startswith("random7"):
        d = int(name.split("_d")[1])
        z = r.randn(1037, d).astype(np.float32)
        labels = r.randint(0, 7, 1037)
        labels[:7] = np.arange(7)
    elif name == "halves_d16":
        z = r.randn(400, 16).astype(np.float32)
        labels = np.repeat([0, 1], 200)
    elif name == "singletons_d7":
        z = r.randn(200, 7).astype(np.float32)
        labels = np.arange(200)
    else:
        z = r.randn(300, 40).astype(np.float32)
        labels = r.randint(0, 5, 300)
        labels[:5] = np.arange(5)
    form = key_form(z.shape[1])
    labels = labels.astype(np.int32)
    edges, keys = kruskal(z, labels, form)
    return {"z": z, "labels": labels, "C": int(labels.max()) + 1, "form": form, "edges": edges, "keys": keys}


def query_rows(n, kind):
    """Query lists of geo_nearest_foreign: `strided` 207 rows (one query per wave; no multiple of 4, 8 or 64), `wrap4` 2 051
    rows with repeats (four queries per wave), `wrap8` 16 421 rows with repeats (eight per wave)."""
    if kind == "strided":
        return np.arange(2, n, 5, dtype=np.int32)[:207]
    m = {"wrap4": 2051, "wrap8": 16421}[kind]
    return ((np.arange(m, dtype=np.int64) * 5 + 2) % n).astype(np.int32)
