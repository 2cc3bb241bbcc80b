"""numpy restatement of the geodesic-path entry points (include/geo_hip.h: geo_sssp_paths_count, geo_sssp_paths_fill,
geo_polyline_resample), shared by tests/test_paths_host.py, tests/test_gpu_paths.py and tools/exp_paths.py.  Plain loops, fp64,
one rounding per operation: every comparison against it is bit for bit."""
import numpy as np

SENTINEL = -9999


def walk(P_row: np.ndarray, source: int, target: int, n: int, max_hops=None):
    """(status, nodes source -> target): status 0 source reached, 1 unreachable (sentinel at a node other than the source),
    2 malformed (max_hops edges walked without reaching the source, or a predecessor outside [0, n)).  nodes is empty for
    status 1 and 2."""
    max_hops = n - 1 if max_hops is None else max_hops
    v, back = int(target), [int(target)]
    while True:
        if v == source:
            return 0, np.asarray(back[::-1], dtype=np.int32)
        if len(back) - 1 == max_hops:
            return 2, np.zeros(0, dtype=np.int32)
        p = int(P_row[v])
        if p == SENTINEL:
            return 1, np.zeros(0, dtype=np.int32)
        if p < 0 or p >= n:
            return 2, np.zeros(0, dtype=np.int32)
        v = p
        back.append(v)


def hop_weight(indptr, indices, weights, u: int, v: int) -> np.float32:
    """The weight of the hop u -> v on a pull CSR: the minimum over the entries of row v whose index is u (weights None:
    unit weights); +inf when there is none."""
    lo, hi = int(indptr[v]), int(indptr[v + 1])
    hit = np.flatnonzero(indices[lo:hi] == u)
    if hit.size == 0:
        return np.float32(np.inf)
    if weights is None:
        return np.float32(1.0)
    return np.float32(weights[lo:hi][hit].min())


def cumulative(indptr, indices, weights, nodes: np.ndarray) -> np.ndarray:
    """cum[0] = 0, cum[i] = cum[i - 1] + float64(w_i): fp64, source outward, one rounding per hop."""
    cum = np.zeros(len(nodes), dtype=np.float64)
    for i in range(1, len(nodes)):
        cum[i] = cum[i - 1] + np.float64(hop_weight(indptr, indices, weights, int(nodes[i - 1]), int(nodes[i])))
    return cum


def extract(P, sources, rows, targets, indptr, indices, weights, max_hops=None):
    """What paths_from_predecessors_device returns, on the host: (nodes i32 [T], offsets i64 [M + 1], cum f64 [T], hops i32 [M],
    status i32 [M])."""
    n = len(indptr) - 1
    M = len(rows)
    hops, status = np.full(M, -1, dtype=np.int32), np.zeros(M, dtype=np.int32)
    offsets = np.zeros(M + 1, dtype=np.int64)
    nodes, cum = [], []
    for m in range(M):
        r = int(rows[m])
        status[m], path = walk(P[r], int(sources[r]), int(targets[m]), n, max_hops)
        if status[m] == 0:
            hops[m] = len(path) - 1
            nodes.append(path)
            cum.append(cumulative(indptr, indices, weights, path))
        offsets[m + 1] = offsets[m] + (len(path) if status[m] == 0 else 0)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return cat(nodes, np.int32), offsets, cat(cum, np.float64), hops, status


def resample_one(z: np.ndarray, nodes: np.ndarray, cum: np.ndarray, F: int) -> np.ndarray:
    """F points at equal arc length along the polyline z[nodes] with running length cum: f32 [F, d].  Frame 0 is z[nodes[0]] and
    frame F - 1 is z[nodes[-1]]; frame f between them sits at s = cum[-1] * f / (F - 1) in the largest segment i <= hops - 1
    with cum[i] <= s, at u = (s - cum[i]) / (cum[i + 1] - cum[i]) (0 for a segment of length 0), and is a + u * (b - a) in
    fp64, rounded once to float32."""
    hops = len(nodes) - 1
    out = np.empty((F, z.shape[1]), dtype=np.float32)
    for f in range(F):
        i, u = 0, np.float64(0.0)
        if f == F - 1:
            i = hops
        elif f > 0 and hops > 0:
            s = np.float64(cum[hops]) * np.float64(f) / np.float64(F - 1)
            i = int(np.flatnonzero(cum[:hops] <= s).max())
            den = cum[i + 1] - cum[i]
            u = np.float64(0.0) if den == 0.0 else (s - cum[i]) / den
        a = z[nodes[i]].astype(np.float64)
        b = z[nodes[min(i + 1, hops)]].astype(np.float64)
        out[f] = (a + u * (b - a)).astype(np.float32)
    return out


def resample(z, nodes, offsets, cum, F: int) -> np.ndarray:
    """geo_polyline_resample after the wrapper's NaN fill: f32 [M, F, d], NaN for an empty slice."""
    M = len(offsets) - 1
    out = np.full((M, F, z.shape[1]), np.nan, dtype=np.float32)
    for m in range(M):
        lo, hi = int(offsets[m]), int(offsets[m + 1])
        if hi > lo:
            out[m] = resample_one(z, nodes[lo:hi], cum[lo:hi], F)
    return out


def chord(z, src, dst, F: int) -> np.ndarray:
    """The straight line between z[src[m]] and z[dst[m]]: the two-node polyline with cum = [0, 1]."""
    return np.stack([resample_one(z, np.array([a, b]), np.array([0.0, 1.0]), F) for a, b in zip(src, dst)])


def bits(x: np.ndarray) -> np.ndarray:
    """The array's bit pattern as integers of its width (NaN-safe equality)."""
    x = np.ascontiguousarray(x)
    return x.view({4: np.int32, 8: np.int64}[x.dtype.itemsize])
