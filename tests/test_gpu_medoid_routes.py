"""The kernel variants of csrc/medoid.hip that the fits never select, on synthetic matrices (the kernels need no metric
property): pam_swap_kernel's scalar / vector loops, per-wave / shared LDS accumulators and per-candidate outputs;
attach_argmin_kernel beyond one 64-medoid round; cluster_cost_kernel and rows_argmin_kernel on padded rows.

PAM reference: the DEFINITION, not the FastPAM decomposition -- with Dp = D^power in fp64 and c1 <= c2 the two smallest medoid
costs of a node, delta[x][i] = sum_j min(Dp[x][j], c2[j] if nearest(j) == i else c1[j]) - sum_j c1[j], K passes over n x n in
torch float64 (`swap_deltas_by_definition`; one case ties it to oracle.kmedoids.pam_swap_pass, which recomputes the total
cost for every pair).

Matrices.  Integer-valued: every power and every fp64 sum is an integer below 2^53, exact in any order, LDS atomics
included -- best_delta must equal the reference's row minimum bit for bit and best_medoid must be the FIRST index attaining
it.  "int": float32 entries from {1, ..., 5}; these tie constantly, the sharp check of the tie rule.  "clustered": one group
per medoid, every other node in a random group, {1, ..., 5} inside a group and {50, ..., 99} across.  Only the row MINIMUM
over the medoids is returned, and with uniform entries and hundreds of medoids the few per-medoid terms of a row hardly ever
decide it (a kernel that added them to the wrong row passed "int" and "real" at K = 897); here a candidate takes over its own
group when that group's medoid goes, so the minimum sits at that medoid and consists of per-medoid terms.
Real-valued ("real", rand): |best_delta - row minimum| <= 1e-9 total, the bound of test_gpu_pam.py (fp64 sums of n terms:
~n 1e-16 relative).

The padding of every row-strided view is NaN: a lane that reads past n poisons its row.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INF = float("inf")
GEO_OK, GEO_E_ARG = 0, -1


def strided(a: np.ndarray, ld: int) -> torch.Tensor:
    """a f32 [r, n] as a device view [r, n] of a [r, ld] buffer whose padding is NaN."""
    r, n = a.shape
    buf = torch.full((r, ld), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[:, :n]
    view.copy_(torch.from_numpy(a))
    assert view.stride(0) == ld and view.stride(1) == 1
    return view


def matrix(n: int, family: str, seed: int, med=None) -> np.ndarray:
    r = np.random.RandomState(seed)
    if family == "real":
        D = r.rand(n, n).astype(np.float32)
    else:
        D = r.randint(1, 6, size=(n, n)).astype(np.float32)
    if family == "clustered":
        group = r.randint(0, len(med), size=n)
        group[med] = np.arange(len(med))
        far = r.randint(50, 100, size=(n, n)).astype(np.float32)
        D = np.where(group[:, None] == group[None, :], D, far)
    np.fill_diagonal(D, 0.0)
    return D


def medoid_set(n: int, K: int, seed: int, last: bool = True) -> np.ndarray:
    """K distinct rows in shuffled order: row 0, both rows of workgroup 5's pair, row n - 1 (`last`), the rest drawn."""
    r = np.random.RandomState(seed)
    if K == 2:
        return np.array([n - 1, 0] if last else [11, 10])
    fixed = [0, 10, 11] + ([n - 1] if last else [])
    pool = np.setdiff1d(np.arange(n - 1), fixed)               # never row n - 1 unless asked for
    med = np.concatenate([fixed, r.choice(pool, K - len(fixed), replace=False)])
    return med[r.permutation(K)]


def swap_deltas_by_definition(D: torch.Tensor, med: torch.Tensor, power: int):
    """(delta f64 [n, K], total): the change of the total cost for every (candidate x, medoid position i), rows of medoids
    +inf.  torch float64 on D's device."""
    Dp = D.double() ** power
    rows = Dp[med.long()]
    two = torch.topk(rows, 2, dim=0, largest=False).values
    c1, c2 = two[0], two[1]
    near = torch.min(rows, dim=0).indices                       # ties: c1 == c2 there, either choice gives the same costs
    total = c1.sum()
    delta = torch.empty(D.shape[0], med.numel(), dtype=torch.float64, device=D.device)
    for i in range(med.numel()):
        delta[:, i] = torch.minimum(Dp, torch.where(near == i, c2, c1)[None, :]).sum(dim=1) - total
    delta[med.long()] = INF
    return delta, float(total)


def first_argmin(delta: torch.Tensor):
    low = delta.min(dim=1).values
    hit = delta == low[:, None]
    return low, torch.argmax(hit.to(torch.uint8), dim=1).to(torch.int32)       # argmax: the first maximal index


def check_swap(D: torch.Tensor, med_h: np.ndarray, power: int, exact: bool):
    from vqvae_amd.geo.kmeans_optimized import pam_swap_deltas_device, pam_swap_pass_device
    med = torch.from_numpy(med_h.astype(np.int32)).cuda()
    n = D.shape[0]
    ref, total_ref = swap_deltas_by_definition(D, med, power)
    low, arg = first_argmin(ref)
    is_med = torch.zeros(n, dtype=torch.bool, device="cuda")
    is_med[med.long()] = True
    best, which, total = pam_swap_deltas_device(D, med, power)
    assert best.dtype == torch.float64 and which.dtype == torch.int32 and best.shape == which.shape == (n,)
    assert bool((best[is_med] == INF).all()) and not bool(which[is_med].any())          # a medoid is no candidate
    cand = ~is_med
    assert bool(torch.isfinite(low[cand]).all())
    delta, i, x, total_p = pam_swap_pass_device(D, med, power)
    assert total_p == total
    if exact:
        assert total == total_ref
        bad = torch.nonzero((best != low) & cand).flatten()
        assert bad.numel() == 0, (power, bad[:8].tolist(), best[bad[:8]].tolist(), low[bad[:8]].tolist())
        bad = torch.nonzero((which != arg) & cand).flatten()
        assert bad.numel() == 0, (power, "first medoid on ties", bad[:8].tolist(), which[bad[:8]].tolist(), arg[bad[:8]].tolist())
        x_ref = int(torch.nonzero(low == low.min())[0])
        assert (delta, i, x) == (float(low[x_ref]), int(arg[x_ref]), x_ref)
    else:
        bound = 1e-9 * total_ref
        assert abs(total - total_ref) <= 1e-9 * total_ref
        err = (best - low).abs()[cand].max().item()
        assert err <= bound, (power, err, bound)
        at = ref.gather(1, which.long()[:, None]).flatten()                           # the definition at the medoid returned
        gap = (at - low)[cand].max().item()
        assert gap <= bound, (power, gap, bound)
        assert not is_med[x] and 0 <= i < med.numel()
        assert delta == float(best[x]) and i == int(which[x]) and delta == float(best.min())
        assert abs(delta - float(low.min())) <= bound and float(ref[x, i]) - float(low.min()) <= bound


#    n, ld, K, families                               route
SWAP_SHAPES = [
    (259, 259, 7, ("int", "clustered", "real")),      # scalar by n; the last workgroup has one row, and it is a candidate
    (260, 261, 7, ("int", "clustered", "real")),      # scalar by ld (view of a wider buffer)
    (260, 264, 2, ("int", "clustered", "real")),      # vector with padding
    (260, 264, 7, ("int", "clustered", "real")),
    (4357, 4357, 7, ("int", "clustered", "real")),    # scalar, uneven wave shares
    (4360, 4360, 7, ("int", "clustered", "real")),    # vector, second trip of the four-steps-in-flight loop
    (1100, 1100, 896, ("int", "clustered", "real")),  # per-wave accumulators at the LDS limit (56 KB)
    (1100, 1100, 897, ("int", "clustered", "real")),  # shared accumulators
    (3788, 3788, 3584, ("int", "clustered")),         # the ABI's maximum
]
SWAP_CASES = [pytest.param(n, ld, K, fam, power, id=f"n{n}-ld{ld}-K{K}-{fam}-p{power}")
              for n, ld, K, fams in SWAP_SHAPES for fam in fams for power in (1, 2)]


@pytest.mark.parametrize("n,ld,K,family,power", SWAP_CASES)
def test_swap_deltas_of_every_candidate_equal_the_definition(n, ld, K, family, power):
    med = medoid_set(n, K, seed=K, last=n != 259)
    Dh = matrix(n, family, seed=n + K, med=med)
    D = strided(Dh, ld) if ld > n else torch.from_numpy(Dh).cuda()
    check_swap(D, med, power, exact=family != "real")


def test_the_definition_used_here_equals_the_oracle_on_a_small_case():
    """Ties swap_deltas_by_definition to oracle.kmedoids.pam_swap_pass (every pair tried, total cost recomputed)."""
    from oracle import kmedoids as ok
    for family in ("int", "clustered", "real"):
        med = np.array([40, 3, 60, 17])
        Dh = matrix(61, family, seed=9, med=med)
        for power in (1, 2):
            ref, total = swap_deltas_by_definition(torch.from_numpy(Dh).cuda(), torch.from_numpy(med).cuda(), power)
            low, arg = first_argmin(ref)
            d_o, i_o, x_o = ok.pam_swap_pass(Dh, med, power)
            x = int(torch.nonzero(low == low.min())[0])
            assert (x, int(arg[x])) == (x_o, i_o)
            assert abs(float(low[x]) - d_o) <= 1e-12 * total and abs(total - ok.total_cost(Dh, med, power)) <= 1e-12 * total


def two_components(seed: int) -> np.ndarray:
    """61 nodes, rows 40 and up a component of their own (integer-valued inside a component, +inf across)."""
    Dh = matrix(61, "int", seed)
    Dh[:40, 40:] = INF
    Dh[40:, :40] = INF
    return Dh


def test_a_component_with_a_single_medoid_is_refused():
    """Three medoids in the first component, one in the second: the 21 nodes of the second have no finite second-nearest
    medoid, base[i] = sum (c2 - c1) = inf meets max(c, c1) - c2 = -inf for every candidate of that component, and the kernel
    would return NaN where the definition is finite.  The wrapper refuses such an input and says how many nodes."""
    from vqvae_amd.geo.kmeans_optimized import pam_swap_pass_device
    D = torch.from_numpy(two_components(3)).cuda()
    med = torch.tensor([5, 50, 22, 31], dtype=torch.int32, device="cuda")
    ref, _ = swap_deltas_by_definition(D, med, 2)
    in_second = [x for x in range(40, 61) if x != 50]
    assert bool(torch.isfinite(ref[in_second, 1]).all()) and not bool(torch.isnan(ref).any())     # defined, and finite there
    for power in (1, 2):
        with pytest.raises(ValueError, match=r"\b21 of 61 nodes\b"):
            pam_swap_pass_device(D, med, power)


def test_a_disconnected_matrix_with_two_medoids_per_component_is_exact():
    """+inf entries by themselves are fine: a candidate of the other component takes nobody over (min(inf - c1, 0) = 0)."""
    D = torch.from_numpy(two_components(4)).cuda()
    for power in (1, 2):
        check_swap(D, np.array([5, 50, 22, 44]), power, exact=True)


def test_swap_abi_rejects_K_outside_its_range_before_any_launch():
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    lib = _lib.load()
    n = 3788
    D = torch.ones(n, n, dtype=torch.float32, device="cuda")
    near = torch.zeros(n, dtype=torch.int32, device="cuda")
    d1, d2 = torch.ones(n, device="cuda"), torch.ones(n, device="cuda")
    base = torch.zeros(3585, dtype=torch.float64, device="cuda")
    is_med = torch.zeros(n, dtype=torch.uint8, device="cuda")
    best = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    which = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    for K in (3585, 1):
        st = lib.geo_pam_swap_deltas(ptr(D), n, ptr(near), ptr(d1), ptr(d2), ptr(base), ptr(is_med), n, K, 2, ptr(best),
                                     ptr(which), stream_ptr())
        assert st == GEO_E_ARG, K
    torch.cuda.synchronize()
    assert bool((best == -7.0).all()) and bool((which == -7).all())


# ---- geo_attach_argmin ------------------------------------------------------------------------------------------------------
def attach_reference(Dt, nbr, length):
    """numpy float32: cand = len[v][u] + Dt[nbr[v][u]][m] (one float32 add), minimum over u, first argmin over m."""
    n_new, K = nbr.shape[0], Dt.shape[1]
    dist = np.full(n_new, np.inf, dtype=np.float32)
    arg = np.zeros(n_new, dtype=np.int32)
    for v in range(n_new):
        dm = np.full(K, np.inf, dtype=np.float32)
        for u in range(nbr.shape[1]):
            if nbr[v, u] >= 0:
                dm = np.minimum(dm, (length[v, u] + Dt[nbr[v, u]]).astype(np.float32))
        dist[v], arg[v] = dm.min(), int(np.argmin(dm))
    return dist, arg


@pytest.mark.parametrize("K", [1, 63, 64, 65, 130])
def test_attach_argmin_over_several_rounds_with_ties_and_missing_edges(K):
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    lib = _lib.load()
    nodes = 12
    for k in (1, 3):
        for n_new in (1, 5, 9):
            for ld in (K, K + 3):
                r = np.random.RandomState(1000 * K + 100 * k + 10 * n_new + ld)
                Dt = r.randint(1, 4, size=(nodes, K)).astype(np.float32)           # small integers: ties across lanes and rounds
                Dt[r.rand(nodes, K) < 0.2] = np.inf
                Dt[0] = np.inf                                                      # node 0 reaches no medoid
                length = r.randint(0, 3, size=(n_new, k)).astype(np.float32)
                nbr = r.randint(1, nodes, size=(n_new, k)).astype(np.int32)
                nbr[r.rand(n_new, k) < 0.25] = -1
                if n_new > 1:
                    nbr[n_new - 1] = -1                                             # no edge at all: (inf, 0)
                    nbr[1] = 0                                                      # edges, but no finite path: (inf, 0)
                    nbr[2, 0] = 3                                                   # at least one point with an edge
                want_d, want_a = attach_reference(Dt, nbr, length)
                if n_new > 1:
                    assert want_d[n_new - 1] == np.inf and want_a[n_new - 1] == 0 and want_d[1] == np.inf and want_a[1] == 0
                Dd = strided(Dt, ld) if ld > K else torch.from_numpy(Dt).cuda()
                nb, ln = torch.from_numpy(nbr).cuda(), torch.from_numpy(length).cuda()
                dist = torch.full((n_new + 4,), -7.0, dtype=torch.float32, device="cuda")
                arg = torch.full((n_new + 4,), -7, dtype=torch.int32, device="cuda")
                st = lib.geo_attach_argmin(ptr(Dd), ld, K, ptr(nb), ptr(ln), k, n_new, ptr(dist), ptr(arg), stream_ptr())
                assert st == GEO_OK
                what = (K, k, n_new, ld)
                np.testing.assert_array_equal(dist[:n_new].cpu().numpy(), want_d, err_msg=str(what))
                np.testing.assert_array_equal(arg[:n_new].cpu().numpy(), want_a, err_msg=str(what))
                assert bool((dist[n_new:] == -7.0).all()) and bool((arg[n_new:] == -7).all()), what
                # no point: GEO_OK and nothing written
                dist.fill_(-7.0)
                arg.fill_(-7)
                st = lib.geo_attach_argmin(ptr(Dd), ld, K, ptr(nb), ptr(ln), k, 0, ptr(dist), ptr(arg), stream_ptr())
                assert st == GEO_OK
                assert bool((dist == -7.0).all()) and bool((arg == -7).all()), what


# ---- geo_cluster_costs through medoid_update_device ------------------------------------------------------------------------
@pytest.mark.parametrize("power", [1, 2])
def test_cluster_costs_on_padded_rows_for_cluster_sizes_around_the_wave(power):
    from oracle import kmedoids as ok
    from vqvae_amd.geo.kmeans_optimized import medoid_update_device
    sizes = [0, 1, 63, 64, 65, 129]
    n = sum(sizes)
    assert n == 322 and n % 4 != 0
    r = np.random.RandomState(7)
    assign = r.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)
    np.testing.assert_array_equal(np.bincount(assign, minlength=len(sizes)), sizes)
    Dh = r.rand(n, n).astype(np.float32)
    med = np.array([int(np.flatnonzero(assign == c)[-1]) if s else 5 for c, s in enumerate(sizes)])   # cluster 0 is empty
    new_o, cost_o = ok.medoid_update(Dh, assign, med, power)
    assert (new_o[1:] != med[1:]).any() and new_o[0] == med[0]
    D = strided(Dh, n + 1)
    new_g, cost_g = medoid_update_device(D, torch.from_numpy(assign).cuda(), torch.from_numpy(med.astype(np.int32)).cuda(), power)
    np.testing.assert_array_equal(cost_g.cpu().numpy(), cost_o)             # same summation tree: bit-equal fp64
    np.testing.assert_array_equal(new_g.cpu().numpy(), new_o)


# ---- geo_rows_argmin --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 3])
def test_rows_argmin_on_padded_rows_with_either_output_alone(n_rows):
    from vqvae_amd import _lib
    from vqvae_amd._device import ptr, stream_ptr
    from vqvae_amd.geo.kmeans_optimized import assign_from_rows_device
    lib = _lib.load()
    n, ld = 257, 260
    r = np.random.RandomState(n_rows)
    Dh = r.randint(1, 4, size=(6, n)).astype(np.float32)
    Dh[r.rand(6, n) < 0.1] = np.inf
    Dh[4] = Dh[1]                                                            # two identical rows: the first listed wins
    Dh[:, 100] = np.inf                                                      # inf in every row: (inf, 0)
    Dh[:, 256] = np.inf
    rows_h = np.array([4, 1, 3][:n_rows], dtype=np.int32)
    want_d, want_a = Dh[rows_h].min(axis=0), np.argmin(Dh[rows_h], axis=0).astype(np.int32)
    assert want_d[100] == np.inf and want_a[100] == 0 and (n_rows == 1 or not (want_a == 1).any())
    D = strided(Dh, ld)
    rows = torch.from_numpy(rows_h).cuda()
    dmin, arg = assign_from_rows_device(D, rows)
    np.testing.assert_array_equal(dmin.cpu().numpy(), want_d)
    np.testing.assert_array_equal(arg.cpu().numpy(), want_a)
    only_d = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    only_a = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    assert lib.geo_rows_argmin(ptr(D), ld, ptr(rows), n_rows, n, ptr(only_d), None, stream_ptr()) == GEO_OK
    assert lib.geo_rows_argmin(ptr(D), ld, ptr(rows), n_rows, n, None, ptr(only_a), stream_ptr()) == GEO_OK
    assert torch.equal(only_d, dmin) and torch.equal(only_a, arg)
    assert lib.geo_rows_argmin(ptr(D), ld, ptr(rows), n_rows, n, None, None, stream_ptr()) == GEO_E_ARG
