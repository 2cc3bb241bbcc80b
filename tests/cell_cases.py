"""Host-side restatement of the cell-restricted medoid update (DESIGN.md "Cell-restricted medoid update") for the tests of
csrc/cell.hip: the cut graph, the update through oracle/kmedoids.py on the all-pairs matrix of the cut graph, the selection
rule, and the host loop of fit_kmedoids_voronoi_graph.  Nothing here touches the GPU."""
import functools

import numpy as np
from scipy import sparse


def cut_graph(W, assign):
    """W without the entries whose two ends have different `assign`, or an end with assign < 0 (same shape, CSR)."""
    W = sparse.coo_matrix(W)
    a = np.asarray(assign)
    keep = (a[W.row] == a[W.col]) & (a[W.row] >= 0)
    return sparse.csr_matrix((W.data[keep], (W.row[keep], W.col[keep])), shape=W.shape)


def select_medoids(cost, assign, medoids):
    """Per cell the member with the smallest cost, lowest node index on ties; an empty cell and a cell whose costs are all
    +inf keep their medoid.  Returns (new medoids, number of all-inf cells)."""
    a = np.asarray(assign)
    new = np.array(medoids, dtype=np.int64).copy()
    kept = 0
    for c in range(len(new)):
        members = np.flatnonzero(a == c)
        if members.size == 0:
            continue
        if not np.isfinite(cost[members]).any():
            kept += 1
            continue
        new[c] = members[int(np.argmin(cost[members]))]
    return new, kept


def restated_update(W, assign, medoids, power):
    """(new medoids, cost f64 [n], all-inf cells): oracle.kmedoids.medoid_update over the all-pairs matrix of the cut graph,
    the selection rule of the definition, +inf for the nodes of no cell."""
    from oracle import kmedoids as okm
    a = np.asarray(assign)
    _, cost = okm.medoid_update(okm.all_pairs(cut_graph(W, a)), a, np.asarray(medoids), power)
    cost = np.where(a < 0, np.inf, cost)
    new, kept = select_medoids(cost, a, medoids)
    return new, cost, kept


def host_assign(W, medoids):
    """(dmin f32 [n], first argmin [n]) of the float32 distance rows of the medoids."""
    from oracle import sssp as osp
    D = osp.dijkstra_multi_source(W, np.asarray(medoids, dtype=int), dtype=np.float32)
    return D.min(axis=0), D.argmin(axis=0)


def objective(dmin, power):
    d = np.asarray(dmin).astype(np.float64)
    d = d[np.isfinite(d)]
    return float(np.sum(d * d if power == 2 else d))


def host_voronoi_graph(W, medoids0, max_iter, power=2):
    """The loop of fit_kmedoids_voronoi_graph on the host.  Returns (medoids, assign, history, rejected, all-inf cells seen)."""
    med = np.asarray(medoids0, dtype=np.int64)
    dmin, assign = host_assign(W, med)
    history, rejected, kept_seen = [objective(dmin, power)], False, 0
    for _ in range(max_iter):
        new, _, kept = restated_update(W, np.where(np.isfinite(dmin), assign, -1), med, power)
        kept_seen += kept
        if np.array_equal(new, med):
            break
        dmin_new, assign_new = host_assign(W, new)
        obj = objective(dmin_new, power)
        if not obj < history[-1]:
            rejected = True
            break
        med, dmin, assign = new, dmin_new, assign_new
        history.append(obj)
    return med, assign, history, rejected, kept_seen


def grow_cell(W, seed, size, taken):
    """`size` nodes not in `taken`, grown breadth-first from `seed` over W: connected in the induced subgraph."""
    W = W.tocsr()
    cell, queue, seen = [], [int(seed)], {int(seed)}
    while queue and len(cell) < size:
        v = queue.pop(0)
        cell.append(v)
        for u in W.indices[W.indptr[v]:W.indptr[v + 1]]:
            if int(u) not in seen and int(u) not in taken:
                seen.add(int(u))
                queue.append(int(u))
    assert len(cell) == size, (len(cell), size)
    return cell


def seven_node_example():
    """0 -1- 1 -2- 2 -1- 3 -1- 4 -3- 5 -1- 6 plus the chord 0 -4- 2.  Cells {0, 1, 2} and {3, 4, 5}, node 6 in no cell, cell 2
    empty.  The cut drops 2-3 and 5-6.  Inside cell 0: d(0,1) = 1, d(1,2) = 2, d(0,2) = 3 (the chord of 4 loses); inside cell 1:
    d(3,4) = 1, d(4,5) = 3, d(3,5) = 4.
    power 1: costs (4, 3, 5 | 5, 4, 7), power 2: (10, 5, 13 | 17, 10, 25); node 6: +inf.  New medoids (1, 4, kept 6)."""
    edges = [(0, 1, 1.0), (1, 2, 2.0), (2, 3, 1.0), (3, 4, 1.0), (4, 5, 3.0), (5, 6, 1.0), (0, 2, 4.0)]
    r = [e[0] for e in edges] + [e[1] for e in edges]
    c = [e[1] for e in edges] + [e[0] for e in edges]
    w = [e[2] for e in edges] * 2
    W = sparse.csr_matrix((np.array(w, dtype=np.float32), (r, c)), shape=(7, 7))
    assign = np.array([0, 0, 0, 1, 1, 1, -1])
    medoids = np.array([0, 5, 6])
    costs = {1: np.array([4.0, 3.0, 5.0, 5.0, 4.0, 7.0, np.inf]), 2: np.array([10.0, 5.0, 13.0, 17.0, 10.0, 25.0, np.inf])}
    return W, assign, medoids, costs, np.array([1, 4, 6])


@functools.lru_cache(maxsize=None)
def knn_graph(n, d, k, seed):
    """The graphs of tests/test_gpu_voronoi.py::_graph (largest component of a union kNN graph), built once per process."""
    from conftest import latents
    from oracle import knn as okn
    W, _ = okn.build_knn_graph(latents(n, d, seed), k=k, mode="distance", sym="union")
    mask = okn.largest_connected_component(W)
    return W[mask][:, mask].tocsr()
