"""Graph-based geodesic K-medoids on the MI355X -- same API as the reference's
src/geo/kmeans_optimized.py (kpp_initialization_graph :14, assign_points_to_medoids :77,
compute_quantization_error :109, fit_kmedoids_optimized :141, fit_kmedoids_with_connectivity_check :186).

The graph stays resident in HBM.  The whole k-means++ chain runs on the GPU (csrc/kpp.hip): pruned frontier
solves from each new centre, the running (min, first-argmin) update, and numpy's legacy RandomState.choice draw
restated bit for bit (float32 D^2 weights, float32 pairwise add.reduce, fp64 cdf, searchsorted); the host only
supplies the uniform deviates of the same RandomState stream and steps in for the rare draws the device declines
(u within rounding reach of a cdf step, degenerate weights).  GEO_KPP_HOST_DRAW=1 selects the reference's own
structure instead -- one device solve + one numpy draw on the downloaded d_min per centre (kmeans_optimized.py:47-69);
the tests compare both.
"""
import os
import time
from typing import List, Optional, Tuple

import numpy as np
import torch
from scipy import sparse

from .. import _lib
from .._device import DeviceCSR, device, ptr, ptr_or_stand_in, stream_ptr, workspace
from .._export import capped_workspace
from .geo_shortest_paths import nearest_source_device, _pull_structure, ensure_valid_graph, sssp_multi_device


def _to_device_graph(W) -> DeviceCSR:
    if isinstance(W, DeviceCSR):
        return W
    W = ensure_valid_graph(W)
    return DeviceCSR.from_scipy(_pull_structure(W, directed=False), device())


# Tuning switches of the chain, read ONCE at import (tests flip them through _KNOBS, bench leaves them alone).
_KNOBS = {"resident": os.environ.get("GEO_KPP_RESIDENT", "1") != "0",
          "resident_from": int(os.environ.get("GEO_KPP_RESIDENT_FROM", "0")),       # 0: by graph size, see _resident_from
          "log": os.environ.get("GEO_KPP_LOG", "0") == "1"}


def _resident_from(n: int) -> int:
    """First centre the resident workgroup takes over.  Centre t claims about n / t nodes; the workgroup's LDS table holds
    4096, and below ~1000 nodes per cell it beats the multi-workgroup step kernel (60 000 nodes: 64 gave 21.2 ms for the
    chain, 32 22.3 ms -- two early cells outgrew the table and were handed back -- 96 21.4 ms)."""
    return _KNOBS["resident_from"] or max(32, n // 1000)


class _Chain:
    """Running (min, first-argmin) over single-source solves: d_min of kmeans_optimized.py:36,44."""

    def __init__(self, G: DeviceCSR):
        self.G, self.lib = G, _lib.load()
        dev = G.indptr.device
        self.dmin = torch.full((G.n,), float("inf"), dtype=torch.float32, device=dev)
        self.arg = torch.zeros(G.n, dtype=torch.int32, device=dev)
        self.ws = workspace(self.lib.geo_sssp_workspace_bytes(G.n, G.nnz, 1), dev)
        self.host = torch.empty(G.n, dtype=torch.float32, pin_memory=True)
        self.sweeps = 0
        self.solves = 0

    def absorb(self, source: int, pos: int) -> np.ndarray:
        G = self.G
        sw = np.zeros(1, dtype=np.int32)
        with torch.cuda.device(G.indptr.device):
            _lib.check(self.lib.geo_sssp_single_update(
                ptr(G.indptr), ptr(G.indices), ptr(G.data), G.n, int(source), None, ptr(self.dmin),
                ptr(self.arg), int(pos), ptr(self.ws), self.ws.numel(), sw.ctypes.data, stream_ptr()),
                "geo_sssp_single_update")
            self.host.copy_(self.dmin, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        self.sweeps += int(sw[0])
        self.solves += 1
        return self.host.numpy()


def _next_center(rng, N: int, d_min: np.ndarray, centers: List[int]) -> Optional[int]:
    """One k-means++ draw, kmeans_optimized.py:47-69 (d_min is the float32 host copy)."""
    finite = np.isfinite(d_min)
    if finite.any():
        safe = np.where(finite, d_min, np.max(d_min[finite]) * 2.0)
    else:
        safe = np.ones_like(d_min)
    probs = safe ** 2
    probs[centers] = 0.0
    total = probs.sum()
    if total > 0:
        probs /= total
        return int(rng.choice(N, p=probs))
    taken = set(centers)
    rest = [i for i in range(N) if i not in taken]
    if rest:
        return int(rng.choice(rest))
    return None


def _draw_with_u(N: int, d_min: np.ndarray, centers: List[int], u: float):
    """The draw of kmeans_optimized.py:47-61 with the uniform deviate given: RandomState.choice(N, p=probs) is
    cdf = cumsum(float64(p)); cdf /= cdf[-1]; searchsorted(cdf, random_sample(), 'right').  Returns None when
    the weights are degenerate (sum == 0), which the caller resolves with the reference's fallback.
    Same values with fewer passes over the N entries (this runs when the device declines a draw, about once per chain
    at a million latents): no copy when every distance is finite, the cumulative sum taken in float64 directly, and
    the division by cdf[-1] -- monotone, so it cannot reorder the entries -- applied only around the answer."""
    finite = np.isfinite(d_min)
    if finite.all():
        safe = d_min
    elif finite.any():
        safe = np.where(finite, d_min, np.max(d_min[finite]) * 2.0)
    else:
        safe = np.ones_like(d_min)
    probs = safe * safe                                   # == safe ** 2 (numpy squares by multiplying)
    probs[centers] = 0.0
    total = probs.sum()
    if not total > 0:
        return None
    probs /= total
    cdf = np.cumsum(probs, dtype=np.float64)              # == probs.astype(float64).cumsum()
    last = cdf[-1]
    # searchsorted(cdf / last, u, 'right') = number of entries with cdf[j] / last <= u: start from the position in the
    # undivided array and settle it with the exact quotients of its neighbours
    j = int(cdf.searchsorted(u * last, side="right"))
    while j < N and cdf[j] / last <= u:
        j += 1
    while j > 0 and not (cdf[j - 1] / last <= u):
        j -= 1
    return j


def _snapshot(chain: _Chain, absorbed: int, snaps: Optional[dict]) -> None:
    """fit_kmedoids_path: keep (d_min, argmin) as they are once exactly `absorbed` centres are folded in (device copies)."""
    if snaps is not None and absorbed in snaps and snaps[absorbed] is None:
        snaps[absorbed] = (chain.dmin.clone(), chain.arg.clone())


def _kpp_chain_host(G: DeviceCSR, K: int, seed: int, absorb_last: bool, snaps: Optional[dict] = None):
    """Host-sampled chain: one device solve + one numpy draw per centre (reference structure)."""
    N = G.n
    rng = np.random.RandomState(seed)
    centers = [int(rng.randint(0, N))]
    chain = _Chain(G)
    complete = True
    for _ in range(1, K):
        d_min = chain.absorb(centers[-1], len(centers) - 1)
        _snapshot(chain, len(centers), snaps)
        nxt = _next_center(rng, N, d_min, centers)
        if nxt is None:
            print(f"Warning: Could not find {K} valid centers, stopping at {len(centers)}")
            complete = False
            break
        centers.append(nxt)
    if absorb_last and complete:
        chain.absorb(centers[-1], len(centers) - 1)     # the last centre gets no solve inside k++
    return centers, chain


class _SegmentPlan:
    """Which mode runs the chain's next segment, and up to which iteration (no torch, no library handle).
    While d_min still has unreachable (inf) entries the chain runs "budgeted": separate kernels per phase with a sweep
    budget per solve.  A solve exits early once converged, but every enqueued launch costs ~2 us, and a solve that needs
    more than were enqueued aborts and is redone.  The need is the hop radius of the new centre's (pruned) cell: the whole
    graph for the first centre, then shrinking -- segments of doubling length, each taking its budget from what the
    previous one needed.  Once d_min is finite everywhere (after the first centre on a connected graph) the rest of the
    chain is "step": ONE kernel launched over and over that always does "the next step" (csrc/kpp.hip, kpp_step_kernel),
    no budget, no launch spent on an empty frontier.  Later centres have small cells (~N/t nodes): from `resident_from` on
    the chain is "resident", ONE workgroup (kpp_resident_kernel) and a single launch for all remaining centres; a cell that
    outgrows its LDS table is run by the step kernel inside that same library call.
    `stops` (fit_kmedoids_path): no segment runs across one of these iterations."""
    CAP = 4094                                           # most sweeps per solve the device counts

    def __init__(self, K: int, N: int, it1: int, resident_ok: bool, resident_from: int, stops=()):
        self.K, self.N, self.it1, self.resident_ok, self.resident_from = K, N, it1, resident_ok, resident_from
        self.stops, self.budget, self.seg = sorted(stops), 16, 1

    def next(self, it: int, finite: bool) -> Tuple[str, int]:
        """(mode, seg_end) of the segment that starts at iteration it < it1; `finite`: d_min has no inf entry left."""
        if not (finite and self.K <= self.N):
            mode, seg_end = "budgeted", min(self.it1, it + self.seg)
        elif self.resident_ok and it >= min(self.resident_from, self.it1):
            mode, seg_end = "resident", self.it1
        else:
            mode, seg_end = "step", (min(self.it1, self.resident_from) if self.resident_ok else self.it1)
        return mode, min([seg_end] + [b for b in self.stops if b > it][:1])

    def library_args(self, mode: str, finite: bool) -> Tuple[int, int]:
        """(sweeps_per_solve, assume_finite) of geo_kpp_chain for `mode`."""
        return {"budgeted": self.budget, "step": 0, "resident": -1}[mode], 1 if finite else 0

    def clean_segment(self, used: int) -> None:
        """A budgeted segment ran through, its longest solve took `used` sweeps.  Cells shrink: the next needs no more."""
        self.seg, self.budget = min(2 * self.seg, 256), min(self.CAP, max(4, used + used // 8 + 1))

    def more_sweeps(self) -> bool:
        """A budgeted solve did not converge (reason 1): quadruple the budget.  False at the cap (the host solves)."""
        below = self.budget < self.CAP
        if below:
            self.budget, self.seg = min(self.CAP, 4 * self.budget), 1
        return below


class _Deviates:
    """One RandomState, advanced in lock-step with the committed draws: `first` is the first centre, u[t] the deviate the
    reference's rng.choice(N, p=probs) consumes for centre t+1.  The deviates are pre-drawn from `base_state` (the stream
    position before draw `base_t`); a uniform fallback (degenerate weights) consumes the stream differently, so it is
    replayed from base_state and the remaining deviates are drawn afresh from the position it leaves behind."""

    def __init__(self, seed: int, N: int, K: int):
        self.rng, self.K = np.random.RandomState(seed), K
        self.first = int(self.rng.randint(0, N))
        self.base_state, self.base_t = self.rng.get_state(), 0
        u = self.rng.random_sample(max(K - 1, 0)) if K > 1 else np.zeros(0)
        self.u = np.ascontiguousarray(u, dtype=np.float64)   # redrawn in place: the library reads it by address

    def __getitem__(self, t: int) -> float:
        return float(self.u[t])

    def uniform_fallback(self, t: int, rest: List[int]) -> int:
        """The reference's draw for degenerate weights at t, rng.choice(rest) (kmeans_optimized.py:66)."""
        self.rng.set_state(self.base_state)
        if t > self.base_t:
            self.rng.random_sample(t - self.base_t)      # the p-weighted draws committed since base_t
        nxt = int(self.rng.choice(rest))
        self.base_state, self.base_t = self.rng.get_state(), t + 1
        if self.K - 2 - t > 0:
            self.u[t + 1:] = self.rng.random_sample(self.K - 2 - t)
        return nxt


def _kpp_chain_device(G: DeviceCSR, K: int, seed: int, absorb_last: bool, snaps: Optional[dict] = None):
    """Device-resident chain (csrc/kpp.hip): the solves, the d_min update and numpy's draw all stay on the
    GPU; the host only supplies the uniform deviates of the same RandomState stream and steps in when the
    kernel declines a draw (u within rounding reach of a cdf boundary) or a solve needs more sweeps."""
    lib = _lib.load()
    N, dev = G.n, G.indptr.device
    draws = _Deviates(seed, N, K)
    chain = _Chain(G)           # chain.ws and `ws` below alias the same cached workspace buffer: geo_kpp_chain
    #                             re-initialises all of its workspace state on every call, and chain.absorb (which
    #                             overwrites it) only runs between two geo_kpp_chain calls, never during one
    centers_d = torch.zeros(max(K, 1), dtype=torch.int32, device=dev)
    centers_d[0] = draws.first
    is_center = torch.zeros(N, dtype=torch.uint8, device=dev)
    is_center[draws.first] = 1
    ws = workspace(lib.geo_kpp_workspace_bytes(N), dev)
    it, it1, n_valid = 0, (K if absorb_last else K - 1), K
    resident_ok = _KNOBS["resident"] and N <= lib.geo_kpp_resident_max_nodes()
    plan = _SegmentPlan(K, N, it1, resident_ok, _resident_from(N), snaps or ())
    finite, status = False, np.zeros(4, dtype=np.int32)
    while it < it1:
        _snapshot(chain, it, snaps)                      # here exactly centres 0 .. it-1 are folded into d_min
        mode, seg_end = plan.next(it, finite)
        sweeps_per_solve, assume_finite = plan.library_args(mode, finite)
        t_call = time.perf_counter()
        with torch.cuda.device(dev):
            _lib.check(lib.geo_kpp_chain(ptr(G.indptr), ptr(G.indices), ptr(G.data), N, ptr(centers_d),
                                         ptr(is_center), ptr(chain.dmin), ptr(chain.arg), draws.u.ctypes.data, it, seg_end,
                                         K, sweeps_per_solve, assume_finite, ptr(ws), ws.numel(), status.ctypes.data,
                                         stream_ptr()),
                       "geo_kpp_chain")
        # status[3]: budgeted = most sweeps of a solve, step = launches that did work, resident = centres handed back
        t, reason, used = int(status[0]), int(status[1]), int(status[3])
        if _KNOBS["log"]:
            import sys
            print(f"[kpp-log] it {it}..{seg_end} mode {plan.budget if mode == 'budgeted' else mode} -> "
                  f"abort {t} reason {reason} used {used} {1e3 * (time.perf_counter() - t_call):.2f} ms", file=sys.stderr)
        finite = finite or int(status[2]) == 0          # inf entries only ever disappear from d_min
        if reason == 4:
            raise _lib.GeoHipError(f"geo_kpp_chain: abort reason 4 at iteration {t}, which the library handles itself")
        if t < 0:                                        # clean segment
            chain.solves += seg_end - it
            it = seg_end
            if mode == "budgeted":
                plan.clean_segment(used)
            continue
        if reason == 1 and mode == "budgeted" and plan.more_sweeps():
            chain.solves += t - it                       # nothing of solve t was applied: redo it with more sweeps
            it = t
            continue
        chain.solves += t - it + 1
        centers_h = centers_d[: t + 1].cpu().numpy().astype(int).tolist()
        if reason == 1:                                  # beyond the device budget: host-driven solve
            chain.absorb(centers_h[t], t)
        if t + 1 >= K:
            break
        nxt = _draw_with_u(N, chain.dmin.cpu().numpy(), centers_h, draws[t])   # host draw: the device declined this one
        if nxt is None:                                  # degenerate weights: the reference's uniform fallback
            taken = set(centers_h)
            rest = [i for i in range(N) if i not in taken]
            if not rest:
                print(f"Warning: Could not find {K} valid centers, stopping at {len(centers_h)}")
                n_valid = t + 1
                break
            nxt = draws.uniform_fallback(t, rest)
        centers_d[t + 1] = nxt
        is_center[nxt] = 1
        it = t + 1
    centers = centers_d[:n_valid].cpu().numpy().astype(int).tolist()
    return centers, chain


def _kpp_chain(G: DeviceCSR, K: int, seed: int, absorb_last: bool, snaps: Optional[dict] = None):
    print(f"[kpp] Selecting {K} centers among {G.n} nodes")
    if os.environ.get("GEO_KPP_HOST_DRAW", "0") == "1":
        centers, chain = _kpp_chain_host(G, K, seed, absorb_last, snaps)
    else:
        centers, chain = _kpp_chain_device(G, K, seed, absorb_last, snaps)
    print(f"[kpp] Selected {len(centers)} centers")
    return centers, chain


def kpp_initialization_graph(W, K: int, seed: int = 42) -> List[int]:
    """K-means++ initialisation over graph distances (kmeans_optimized.py:14-74)."""
    centers, _ = _kpp_chain(_to_device_graph(W), K, seed, absorb_last=False)
    return centers


def _assign_device(G: DeviceCSR, medoids: np.ndarray):
    # nearest medoid + distance in ONE label-carrying solve (geo_sssp_nearest_source: exact fixed-point units), the K-source
    # solve only when the weights do not qualify
    src = torch.from_numpy(np.asarray(medoids, dtype=np.int32)).to(G.indptr.device)
    dmin, arg, _ = nearest_source_device(G, src)
    return dmin, arg


def _print_sizes(assign: np.ndarray, K: int) -> None:
    counts = np.bincount(assign, minlength=K)
    print(f"[assign] sizes min={counts.min()}, max={counts.max()}, mean={counts.mean():.1f}")


def assign_points_to_medoids(W, medoids: np.ndarray) -> np.ndarray:
    """Nearest medoid per node, first index on ties (kmeans_optimized.py:77-106)."""
    G = _to_device_graph(W)
    K = len(medoids)
    print(f"[assign] {G.n} points to {K} medoids")
    _, arg = _assign_device(G, medoids)
    assign = arg.cpu().numpy().astype(int)
    _print_sizes(assign, K)
    return assign


def _qe_from(dist_to_assigned: np.ndarray) -> float:
    finite = np.isfinite(dist_to_assigned)
    if finite.any():
        return float(np.sum(dist_to_assigned[finite] ** 2))
    return float("inf")


def compute_quantization_error(W, medoids: np.ndarray, assign: np.ndarray) -> float:
    """Sum of squared geodesic distances to the assigned medoid (kmeans_optimized.py:109-138)."""
    G = _to_device_graph(W)
    dev = G.indptr.device
    src = torch.from_numpy(np.asarray(medoids, dtype=np.int32)).to(dev)
    a = torch.from_numpy(np.asarray(assign, dtype=np.int64)).to(dev)
    # the usual call hands in the nearest-medoid assignment: then D[assign[v]][v] IS the column minimum, which one
    # label-carrying solve gives (geo_sssp_nearest_source) -- no K x N matrix; any other assignment takes the matrix
    dmin, amin, _ = nearest_source_device(G, src)
    if bool((amin.long() == a).all()):
        return _qe_from(dmin.cpu().numpy())
    D, _, _, _, _ = sssp_multi_device(G, src, want_D=True)
    picked = D.gather(0, a.view(1, -1)).view(-1)
    return _qe_from(picked.cpu().numpy())


def fit_kmedoids_optimized(W, K: int = 512, init: str = "kpp", seed: int = 42) -> Tuple[np.ndarray, np.ndarray, float]:
    """Graph-based geodesic K-medoids (kmeans_optimized.py:141-183).

    init="kpp" needs K solves instead of the reference's 3K-1: the running minimum / first-argmin
    kept during seeding plus one solve for the last centre IS the assignment and its distances."""
    if init not in ("kpp", "random"):
        raise ValueError("init must be 'kpp' or 'random'")
    G = _to_device_graph(W)
    N = G.n
    print(f"[kmedoids] N={N}, K={K}, edges={G.nnz}, avg_deg={G.nnz/max(1,N):.1f}")
    if init == "kpp":
        centers, chain = _kpp_chain(G, K, seed, absorb_last=True)
        medoids = np.array(centers, dtype=int)
        print(f"[assign] {N} points to {len(medoids)} medoids")
        assign = chain.arg.cpu().numpy().astype(int)
        d_assigned = chain.dmin.cpu().numpy()
    else:
        rng = np.random.RandomState(seed)
        medoids = rng.choice(N, size=min(K, N), replace=False).astype(int)
        print(f"[assign] {N} points to {len(medoids)} medoids")
        dmin, arg = _assign_device(G, medoids)
        assign = arg.cpu().numpy().astype(int)
        d_assigned = dmin.cpu().numpy()
    _print_sizes(assign, len(medoids))
    qe = _qe_from(d_assigned)
    print(f"[kmedoids] Done: clusters={len(medoids)}, qe={qe:.3f}")
    return medoids, assign, qe


def fit_kmedoids_path(W, K_values, init: str = "kpp", seed: int = 42, info: Optional[dict] = None):
    """fit_kmedoids_optimized for every K of K_values (any order, duplicates allowed) from ONE seeding chain.

    Extension: the reference's K sweep (demos/kmedoids_geodesic_analysis.py) fits every K from scratch.  For one seed the
    k-means++ centres of a smaller K are a prefix of those of a larger K (one randint, then one rng.choice per centre), and
    the assignment is the chain's running (d_min, argmin): the sweep is the chain of max(K_values), copied on the device each
    time exactly K_i centres are folded in -- max(K_values) solves instead of sum(K_values).  init="random" is nested the same
    way (RandomState.choice(N, K, replace=False) is a prefix of one permutation) but has no chain: one label-carrying solve
    per distinct K.  Entry i equals fit_kmedoids_optimized(W, K_values[i], init, seed) bit for bit.
    `info`, if given, receives solves (single-source solves of the chain, or label-carrying solves for "random") and, per
    entry, finite_fraction (share of nodes whose distance to their medoid is finite, from d_min)."""
    if init not in ("kpp", "random"):
        raise ValueError("init must be 'kpp' or 'random'")
    Ks = [int(K) for K in K_values]
    if not Ks or min(Ks) < 1:
        raise ValueError("K_values must be a non-empty sequence of positive integers")
    G = _to_device_graph(W)
    N, Kmax = G.n, max(Ks)
    print(f"[kmedoids] N={N}, K path={Ks}, edges={G.nnz}, avg_deg={G.nnz/max(1,N):.1f}")
    states = {}
    if init == "kpp":
        snaps = {K: None for K in set(Ks) if K < Kmax}
        centers, chain = _kpp_chain(G, Kmax, seed, absorb_last=True, snaps=snaps)
        for K in set(Ks):
            # a chain that ran out of nodes stopped with every centre folded in: that state answers every larger K
            dmin, arg = snaps[K] if K < len(centers) else (chain.dmin, chain.arg)
            states[K] = (np.array(centers[:K], dtype=int), dmin, arg)
        solves = chain.solves
    else:
        rng = np.random.RandomState(seed)
        full = rng.choice(N, size=min(Kmax, N), replace=False).astype(int)
        for K in set(Ks):
            dmin, arg = _assign_device(G, full[:K])
            states[K] = (full[:K].copy(), dmin, arg)
        solves = len(states)
    out, fractions = [], []
    for K in Ks:
        medoids, dmin, arg = states[K]
        assign = arg.cpu().numpy().astype(int)
        qe = _qe_from(dmin.cpu().numpy())
        fractions.append(int(torch.isfinite(dmin).sum()) / N)
        print(f"[kmedoids] K={K}: clusters={len(medoids)}, qe={qe:.3f}")
        out.append((medoids.copy(), assign, qe))
    if info is not None:
        info.update(solves=int(solves), finite_fraction=fractions)
    return out


def fit_kmedoids_with_connectivity_check(W, K: int = 512, init: str = "kpp", seed: int = 42):
    """K-medoids plus connectivity metadata (kmeans_optimized.py:186-227)."""
    from .knn_graph_optimized import connected_components_device
    G = _to_device_graph(W)
    n_components, labels = connected_components_device(G)
    sizes = np.bincount(labels.cpu().numpy())
    metadata = {"n_nodes": G.n, "n_edges": G.nnz, "n_components": n_components,
                "largest_component_size": sizes.max() if n_components > 0 else G.n}
    print(f"[graph] components={n_components}, largest={metadata['largest_component_size']}")
    medoids, assign, qe = fit_kmedoids_optimized(G, K=K, init=init, seed=seed)
    metadata.update({"n_medoids": len(medoids), "quantization_error": qe, "method": "optimized_kmedoids"})
    return medoids, assign, qe, metadata


# ---- extension: medoid update (Voronoi iteration) over the resident all-pairs matrix -------------------------------------
def medoid_update_device(D: torch.Tensor, assign: torch.Tensor, medoids: torch.Tensor, power: int = 2):
    """One medoid update: per cluster the member with the smallest sum of D[i][j]^power over the cluster's members
    (lowest node index on ties); a cluster without members keeps its medoid.  D f32 [n,n], assign i32/i64 [n],
    medoids i32 [K], all on the GPU.  Returns (new medoids i32 [K], cost f64 [n])."""
    lib = _lib.load()
    dev = D.device
    n, K = int(D.shape[0]), int(medoids.numel())
    a64 = assign.to(torch.int64)
    a32 = assign.to(torch.int32).contiguous()
    order = torch.argsort(a64, stable=True).to(torch.int32).contiguous()        # members ascending inside a cluster
    counts = torch.bincount(a64, minlength=K)
    offsets = torch.zeros(K + 1, dtype=torch.int32, device=dev)
    offsets[1:] = torch.cumsum(counts, 0).to(torch.int32)
    cost = torch.empty(n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.geo_cluster_costs(ptr(D), D.stride(0), ptr(a32), ptr(order), ptr(offsets), n, int(power),
                                         ptr(cost), stream_ptr()), "geo_cluster_costs")
    new, _ = _select_medoids(cost, a64, torch.arange(n, dtype=torch.int64, device=dev), medoids, n)
    return new, cost


def _select_medoids(cost: torch.Tensor, a64: torch.Tensor, nodes: torch.Tensor, medoids: torch.Tensor, n: int,
                    keep_all_inf: bool = False):
    """The medoid selection both updates share, two scatter-min passes: entry e is node nodes[e] of cluster a64[e] with cost
    cost[e]; per cluster the node with the smallest cost, lowest node index on ties; a cluster without an entry keeps its
    medoid.  keep_all_inf: a cluster whose costs are all +inf keeps its medoid too (otherwise its first node wins, as
    np.argmin has it).  Returns (new medoids i32 [K], smallest cost per cluster f64 [K], +inf for a cluster without an entry)."""
    dev, K = cost.device, int(medoids.numel())
    cmin = torch.full((K,), float("inf"), dtype=torch.float64, device=dev).scatter_reduce(0, a64, cost, "amin")
    hit = cost == cmin[a64]
    if keep_all_inf:
        hit = hit & torch.isfinite(cost)
    cand = torch.where(hit, nodes, torch.full_like(nodes, n))
    first = torch.full((K,), n, dtype=torch.int64, device=dev).scatter_reduce(0, a64, cand, "amin")
    new = torch.where(first < n, first, medoids.to(torch.int64)).to(torch.int32)
    return new, cmin


def assign_from_rows_device(D: torch.Tensor, medoids: torch.Tensor):
    """(dmin f32 [n], argmin i32 [n]): nearest medoid row of D per node, first medoid on ties."""
    lib = _lib.load()
    dev = D.device
    n = int(D.shape[1])
    rows = medoids.to(torch.int32).contiguous()
    dmin = torch.empty(n, dtype=torch.float32, device=dev)
    arg = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.geo_rows_argmin(ptr(D), D.stride(0), ptr(rows), int(rows.numel()), n, ptr(dmin), ptr(arg),
                                       stream_ptr()), "geo_rows_argmin")
    return dmin, arg


def fit_kmedoids_voronoi(W, K: int = 512, init: str = "kpp", seed: int = 42, max_iter: int = 10, power: int = 2,
                         D: Optional[torch.Tensor] = None):
    """fit_kmedoids_optimized followed by medoid updates until the medoids stop changing (at most max_iter updates).

    Extension of the reference (its k-medoids is seeding + one assignment, kmeans_optimized.py:141-183; SURVEY.md section 8
    f4): the all-pairs geodesic matrix is formed once on the GPU (all_pairs_geodesic_device) unless given, every
    iteration is one geo_cluster_costs + one geo_rows_argmin.  power=2 minimises the reference's quantisation error
    (sum of squared distances), which therefore never increases.  Returns (medoids, assign, qe, history) with
    history = [qe after the initial assignment, after update 1, ...]."""
    from .geo_shortest_paths import all_pairs_geodesic_device
    G = _to_device_graph(W)
    dev = G.indptr.device
    medoids0, assign0, qe0 = fit_kmedoids_optimized(W, K=K, init=init, seed=seed)
    if D is None:
        D = all_pairs_geodesic_device(G)
    med = torch.from_numpy(np.asarray(medoids0, dtype=np.int32)).to(dev)
    assign = torch.from_numpy(np.asarray(assign0, dtype=np.int32)).to(dev)
    history = [qe0]
    for _ in range(max_iter):
        new, _ = medoid_update_device(D, assign, med, power)
        if bool((new == med).all()):
            break
        med = new
        dmin, assign = assign_from_rows_device(D, med)
        history.append(_qe_from(dmin.cpu().numpy()))
    medoids = med.cpu().numpy().astype(int)
    assign_h = assign.cpu().numpy().astype(int)
    _print_sizes(assign_h, len(medoids))
    print(f"[kmedoids] Voronoi iterations: {len(history) - 1}, qe {history[0]:.3f} -> {history[-1]:.3f}")
    return medoids, assign_h, history[-1], history


# ---- extension: medoid update inside the cells, without any matrix (csrc/cell.hip) ----------------------------------------
def _as_i32(x, dev) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
    return t.to(device=dev, dtype=torch.int32).contiguous()


def cell_medoid_update_device(G, assign, medoids, power: int = 2, *, resident_nodes_max: Optional[int] = None,
                              max_workspace_bytes: Optional[int] = None, info: Optional[dict] = None):
    """One medoid update on the CUT graph (DESIGN.md "Cell-restricted medoid update"): G without the entries whose two ends
    have different `assign`; a node with assign < 0 is in no cell.  cost[i] = sum over the members j of i's cell of
    d_c(i, j)^power, d_c the shortest path inside the cell (geo_cell_costs: bit for bit geo_cluster_costs over the all-pairs
    matrix of the cut graph, which is never formed), +inf for assign[i] < 0.  Per cell the member with the smallest cost,
    lowest node index on ties; an empty cell and a cell whose costs are all +inf keep their medoid.
    G: symmetric weighted DeviceCSR (or a scipy matrix); assign i32 [n] in [-1, K); medoids i32 [K] in [0, n).
    resident_nodes_max: cells up to this size keep their distance rows in LDS (None: the library's bound); max_workspace_bytes
    caps the scratch (fewer large cells in flight); neither changes a bit of the result.
    Returns (new medoids i32 [K], cost f64 [n]).  `info`, if given, receives resident_cells, workspace_cells, max_sweeps,
    kept_cells (cells with members whose costs are all +inf) and tile (sources per unit of work)."""
    if power not in (1, 2):
        raise ValueError(f"power must be 1 or 2, got {power!r}")
    if resident_nodes_max is not None and int(resident_nodes_max) < 1:
        raise ValueError(f"resident_nodes_max must be at least 1, got {resident_nodes_max!r}")
    G = _to_device_graph(G)
    if G.data is None:
        raise ValueError("cell_medoid_update_device needs a weighted graph")
    dev, n = G.indptr.device, G.n
    a32, med = _as_i32(assign, dev), _as_i32(medoids, dev)
    K = int(med.numel())
    if a32.dim() != 1 or int(a32.numel()) != n:
        raise ValueError(f"assign must have one entry per node ({n}), got shape {tuple(a32.shape)}")
    if med.dim() != 1 or K < 1:
        raise ValueError("medoids must be a non-empty vector")
    if n and (int(a32.max()) >= K or int(a32.min()) < -1):
        raise ValueError(f"assign must lie in [-1, {K}), got [{int(a32.min())}, {int(a32.max())}]")
    if int(med.min()) < 0 or int(med.max()) >= n:
        raise ValueError(f"medoids must lie in [0, {n}), got [{int(med.min())}, {int(med.max())}]")
    lib = _lib.load()
    a64 = a32.to(torch.int64)
    keys = torch.where(a32 >= 0, a64, torch.full_like(a64, K))                  # nodes of no cell sort behind every cell
    order64 = torch.argsort(keys, stable=True)                                  # members ascending inside a cell
    counts = torch.bincount(keys, minlength=K + 1)[:K]
    offsets = torch.zeros(K + 1, dtype=torch.int32, device=dev)
    offsets[1:] = torch.cumsum(counts, 0).to(torch.int32)
    order = order64.to(torch.int32).contiguous()
    members, max_cell = int(offsets[K]), int(counts.max())
    ws = capped_workspace(lib.geo_cell_costs_workspace_bytes(n, G.nnz, K, max_cell), max_workspace_bytes, dev, "cell medoid update")
    cost = torch.empty(n, dtype=torch.float64, device=dev)
    status = np.zeros(4, dtype=np.int32)
    with torch.cuda.device(dev):
        _lib.check(lib.geo_cell_costs(ptr(G.indptr), ptr_or_stand_in(G.indices), ptr_or_stand_in(G.data), n, G.nnz, ptr(a32),
                                      ptr(order), ptr(offsets), K, int(power), int(resident_nodes_max or 0), ptr(cost), ptr(ws),
                                      ws.numel(), status.ctypes.data, stream_ptr()), "geo_cell_costs")
    nodes = order64[:members]
    new, cmin = _select_medoids(cost[nodes], a64[nodes], nodes, med, n, keep_all_inf=True)
    if info is not None:
        info.update(resident_cells=int(status[0]), workspace_cells=int(status[1]), max_sweeps=int(status[2]),
                    kept_cells=int(((counts > 0) & torch.isinf(cmin)).sum()), tile=int(lib.geo_cell_costs_tile()))
    return new, cost


def _objective(dmin: torch.Tensor, power: int) -> float:
    """sum of dmin^power over the finite entries, fp64 (numpy's sum of the host copy: the value a host loop computes)."""
    d = dmin.cpu().numpy().astype(np.float64)
    d = d[np.isfinite(d)]
    return float(np.sum(d * d if power == 2 else d))


def refine_voronoi_graph(G: DeviceCSR, medoids0, max_iter: int = 10, power: int = 2):
    """The rounds of fit_kmedoids_voronoi_graph from given medoids (the seeded state).  Returns (medoids i32 [K], dmin f32 [n],
    assign i32 [n] -- all on the GPU -- accepted objectives, one counter dict per update run, whether the guard fired)."""
    dev = G.indptr.device
    med = torch.from_numpy(np.asarray(medoids0, dtype=np.int32)).to(dev)
    dmin, assign = _assign_device(G, np.asarray(medoids0))
    history, updates, rejected = [_objective(dmin, power)], [], False
    for _ in range(max_iter):
        step = {}
        in_cell = torch.where(torch.isfinite(dmin), assign, torch.full_like(assign, -1))
        new, _ = cell_medoid_update_device(G, in_cell, med, power, info=step)
        updates.append(step)
        if bool((new == med).all()):
            break
        dmin_new, assign_new = _assign_device(G, new.cpu().numpy())
        objective = _objective(dmin_new, power)
        if not objective < history[-1]:
            rejected = True
            print(f"[kmedoids] update {len(updates)} not accepted: objective {objective:.3f} >= {history[-1]:.3f}")
            break
        med, dmin, assign = new, dmin_new, assign_new
        history.append(objective)
    return med, dmin, assign, history, updates, rejected


def fit_kmedoids_voronoi_graph(W, K: int = 512, init: str = "kpp", seed: int = 42, max_iter: int = 10, power: int = 2,
                               info: Optional[dict] = None):
    """fit_kmedoids_optimized followed by cell-restricted medoid updates (at most max_iter): refinement at any graph size,
    no all-pairs matrix (fit_kmedoids_voronoi needs one, about 230 000 nodes at most).

    Each round: the update inside the cells (cell_medoid_update_device; unreachable nodes, dmin = inf, belong to no cell);
    stop if no medoid moved; re-assign with one label-carrying solve (nearest_source_device); the objective is the sum of
    dmin^power over the finite entries in fp64.  A round is accepted only if the objective is strictly below the last
    accepted one, otherwise the previous state is kept and the fit stops: the cell-restricted cost of the old medoid equals
    its global cost except where float32 ties hand a path node to another medoid, so an update can, rarely, not pay off.
    Returns (medoids, assign, qe, history): history = the accepted objectives, the seeded state first; qe = the reference's
    quantisation error of the final distances.  `info`, if given, receives iterations, rejected (the guard fired) and
    updates (one dict of cell_medoid_update_device's counters per update run)."""
    if power not in (1, 2):
        raise ValueError(f"power must be 1 or 2, got {power!r}")
    G = _to_device_graph(W)
    medoids0, _, _ = fit_kmedoids_optimized(G, K=K, init=init, seed=seed)
    med, dmin, assign, history, updates, rejected = refine_voronoi_graph(G, medoids0, max_iter, power)
    medoids = med.cpu().numpy().astype(int)
    assign_h = assign.cpu().numpy().astype(int)
    _print_sizes(assign_h, len(medoids))
    print(f"[kmedoids] Voronoi iterations (cell-restricted): {len(history) - 1}, objective {history[0]:.3f} -> {history[-1]:.3f}")
    if info is not None:
        info.update(iterations=len(history) - 1, rejected=rejected, updates=updates)
    return medoids, assign_h, _qe_from(dmin.cpu().numpy()), history



# ---- extension: PAM swap over the resident all-pairs matrix ---------------------------------------------------------------
def pam_swap_deltas_device(D: torch.Tensor, medoids: torch.Tensor, power: int = 2):
    """PAM's SWAP evaluation for ALL (medoid, candidate) pairs in one pass over the resident matrix (csrc/medoid.hip:
    pam_swap_kernel, FastPAM1 form), per candidate: returns (best_delta f64 [n], best_medoid i32 [n], total).  best_delta[x]
    is the most negative change of the total cost sum_j D[nearest(j)][j]^power over the swaps medoids[i] -> x, best_medoid[x]
    the first i attaining it; the row of a medoid holds (+inf, 0).  total is the current total cost.
    D f32 [n, n] may be a row-strided view (D.stride(0) >= n, D.stride(1) == 1); K = len(medoids) >= 2.
    Every node needs a finite second-nearest medoid: the kernel's decomposition subtracts that cost, so where it is infinite (a
    connected component of the graph that holds exactly one medoid) the change would come out as inf - inf.  Such an input
    raises ValueError, naming the number of those nodes, before anything is launched."""
    lib = _lib.load()
    dev = D.device
    n, K = int(D.shape[0]), int(medoids.numel())
    if K < 2:
        raise ValueError(f"pam_swap_deltas_device needs at least 2 medoids, got {K}")
    med = medoids.to(torch.int64)
    dmin, near = assign_from_rows_device(D, medoids)                 # nearest medoid, first on ties
    near = near.to(torch.int64)
    c1 = dmin.double() ** power
    rows = D[med]                                                    # K x n float32 (a copy)
    rows.scatter_(0, near[None, :], float("inf"))
    d2 = rows.min(dim=0).values
    del rows
    no_second = int((d2 == float("inf")).sum())
    if no_second:
        raise ValueError(f"PAM swap: {no_second} of {n} nodes have no finite second-nearest medoid (a connected component "
                         f"with a single medoid); the swap evaluation is undefined there")
    # base[i] = sum over the nodes of medoid i of (c2 - c1), members in ascending node order, sequential fp64 sums
    # (segment sums through the sorted order: deterministic)
    gain = d2.double() ** power - c1
    order = torch.argsort(near, stable=True)
    counts = torch.bincount(near, minlength=K)
    base = torch.segment_reduce(gain[order], "sum", lengths=counts)
    is_med = torch.zeros(n, dtype=torch.uint8, device=dev)
    is_med[med] = 1
    near32, d1, d2 = near.to(torch.int32).contiguous(), dmin.contiguous(), d2.contiguous()
    best = torch.empty(n, dtype=torch.float64, device=dev)
    which = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.geo_pam_swap_deltas(ptr(D), D.stride(0), ptr(near32), ptr(d1), ptr(d2), ptr(base.contiguous()), ptr(is_med), n, K,
                                           int(power), ptr(best), ptr(which), stream_ptr()), "geo_pam_swap_deltas")
    return best, which, float(c1.sum())


def pam_swap_pass_device(D: torch.Tensor, medoids: torch.Tensor, power: int = 2):
    """The best single PAM swap over the resident matrix (pam_swap_deltas_device; K = 1 is handled here).  Returns
    (delta, i, x, total): the swap medoids[i] -> x with the most negative change of the total cost
    sum_j D[nearest(j)][j]^power (ties: lowest x, then first medoid), and the current total cost.
    With K >= 2 every node needs a finite second-nearest medoid: ValueError otherwise (see pam_swap_deltas_device)."""
    n, K = int(D.shape[0]), int(medoids.numel())
    if K == 1:                                                       # nothing to fall back on: the swap replaces the only medoid
        med = medoids.to(torch.int64)
        dmin, _ = assign_from_rows_device(D, medoids)
        c1 = dmin.double() ** power
        tot = torch.cat([(D[r0:r0 + 4096].double() ** power).sum(dim=1) for r0 in range(0, n, 4096)])
        tot[med] = float("inf")
        delta = tot.min() - c1.sum()
        x = int(torch.nonzero(tot == tot.min())[0])
        return float(delta), 0, x, float(c1.sum())
    best, which, total = pam_swap_deltas_device(D, medoids, power)
    delta = best.min()
    x = int(torch.nonzero(best == delta)[0])                         # lowest candidate among equal changes
    return float(delta), int(which[x]), x, total


def fit_kmedoids_pam(W, K: int = 512, init: str = "kpp", seed: int = 42, max_swaps: int = 50, power: int = 2,
                     D: Optional[torch.Tensor] = None, rel_tol: float = 1e-12):
    """fit_kmedoids_optimized followed by PAM swaps: the best (medoid -> non-medoid) exchange is applied while it lowers the
    total cost (power=2: the reference's quantisation error).  Extension (the reference's k-medoids
    is seeding + one assignment, kmeans_optimized.py:141-183).  Every swap evaluation reads the resident N x N matrix once.
    Returns (medoids, assign, qe, history of total costs).
    With K >= 2 every node must reach at least two medoids at every step (in a disconnected graph: no component with exactly
    one medoid); pam_swap_pass_device raises ValueError otherwise."""
    from .geo_shortest_paths import all_pairs_geodesic_device
    G = _to_device_graph(W)
    dev = G.indptr.device
    medoids0, _, _ = fit_kmedoids_optimized(W, K=K, init=init, seed=seed)
    if D is None:
        D = all_pairs_geodesic_device(G)
    med = torch.from_numpy(np.asarray(medoids0, dtype=np.int32)).to(dev)
    history = []
    for _ in range(max_swaps + 1):
        delta, i, x, total = pam_swap_pass_device(D, med, power)
        history.append(total)
        if len(history) > max_swaps or not delta < -rel_tol * total:
            break
        med[i] = x
    dmin, assign = assign_from_rows_device(D, med)
    medoids = med.cpu().numpy().astype(int)
    assign_h = assign.cpu().numpy().astype(int)
    _print_sizes(assign_h, len(medoids))
    print(f"[kmedoids] PAM swaps: {len(history) - 1}, total cost {history[0]:.3f} -> {history[-1]:.3f}")
    return medoids, assign_h, _qe_from(dmin.cpu().numpy()), history
