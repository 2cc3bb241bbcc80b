"""The host side of the k-means++ chain (vqvae_amd/geo/kmeans_optimized.py) without a GPU: the segment planner against the
rule the chain's loop spelled out inline before the planner existed, its two budget transitions, and the RandomState
bookkeeping of the pre-drawn deviates against a RandomState driven the reference's way."""
import itertools

import numpy as np

from vqvae_amd.geo.kmeans_optimized import _Deviates, _SegmentPlan


def inline_rule(it, it1, K, N, finite, resident_ok, r_from, seg, stops, budget):
    """The three expressions of the former loop (no centre handed back, no fixed budget) and its library arguments."""
    one_step_at, fixed = -1, None
    step_mode = finite and not fixed and K <= N
    resident = step_mode and resident_ok and it >= min(r_from, it1) and it != one_step_at
    if resident:
        seg_end = it1
    elif step_mode:
        seg_end = it + 1 if it == one_step_at else (min(it1, r_from) if resident_ok and it < r_from else it1)
    else:
        seg_end = min(it1, it + seg)
    seg_end = min([seg_end] + [b for b in stops if b > it][:1])
    return seg_end, (-1 if resident else 0) if step_mode else budget, 1 if finite else 0


def test_planner_equals_the_inline_rule_on_the_grid():
    checked, modes = 0, set()
    for N in (40, 6000, 100000):
        for K, finite, resident_ok, r_from, absorb_last, seg in itertools.product(
                (1, 33, N, N + 3), (False, True), (False, True), (0, 1, 16), (False, True), (1, 2, 256)):
            it1 = K if absorb_last else K - 1
            for it in sorted({0, 1, 15, 16, 31, 32, it1 - 1}):
                if not 0 <= it < it1:
                    continue
                for stops in ((), (1,), (it + 1,), (it1 - 1,)):
                    plan = _SegmentPlan(K, N, it1, resident_ok, r_from, stops)
                    plan.seg, plan.budget = seg, 48
                    mode, seg_end = plan.next(it, finite)
                    want = inline_rule(it, it1, K, N, finite, resident_ok, r_from, seg, sorted(stops), 48)
                    assert (seg_end,) + plan.library_args(mode, finite) == want, (N, K, finite, resident_ok, r_from, it1, seg,
                                                                                  it, stops, mode)
                    assert it < seg_end <= it1
                    assert (plan.seg, plan.budget) == (seg, 48)             # planning changes nothing
                    modes.add(mode)
                    checked += 1
    assert modes == {"budgeted", "step", "resident"} and checked > 5000


def test_budget_transitions():
    for used in (0, 3, 16, 4000, 4094):
        for seg in (1, 2, 128, 256):
            plan = _SegmentPlan(64, 1000, 64, True, 32)
            plan.seg = seg
            plan.clean_segment(used)
            assert plan.seg == min(2 * seg, 256)
            assert plan.budget == min(4094, max(4, used + used // 8 + 1))
    assert [min(4094, max(4, u + u // 8 + 1)) for u in (0, 3, 16, 4000, 4094)] == [4, 4, 19, 4094, 4094]
    plan = _SegmentPlan(64, 1000, 64, True, 32)
    plan.seg, budgets = 64, [plan.budget]
    while plan.more_sweeps():                                               # reason 1, again and again
        assert plan.seg == 1
        budgets.append(plan.budget)
    assert budgets == [16, 64, 256, 1024, 4094]                             # min(cap, 4 * budget) up to the cap
    assert not plan.more_sweeps() and plan.budget == 4094                   # at the cap the solve is the host's


def test_deviates_follow_the_reference_stream():
    seed, N, K = 5, 50, 12
    dv = _Deviates(seed, N, K)
    ref = np.random.RandomState(seed)
    assert dv.first == int(ref.randint(0, N))
    np.testing.assert_array_equal(dv.u, ref.random_sample(K - 1))
    assert dv.u.dtype == np.float64 and dv.u.flags.c_contiguous and dv[3] == dv.u[3]
    address, before = dv.u.ctypes.data, dv.u.copy()

    # degenerate draw at t = 4: the reference has consumed one randint and four random_sample() by then
    rest = [i for i in range(N) if i % 3]
    ref = np.random.RandomState(seed)
    ref.randint(0, N)
    for _ in range(4):
        ref.random_sample()
    assert dv.uniform_fallback(4, rest) == int(ref.choice(rest))
    np.testing.assert_array_equal(dv.u[:5], before[:5])
    np.testing.assert_array_equal(dv.u[5:], ref.random_sample(K - 2 - 4))
    assert dv.u.ctypes.data == address                                     # redrawn in place: the library holds the address

    # a second one at t = 7 replays from the state the first one left: draws 5 and 6 were p-weighted
    ref = np.random.RandomState(seed)
    ref.randint(0, N)
    for _ in range(4):
        ref.random_sample()
    ref.choice(rest)
    for _ in range(2):
        ref.random_sample()
    rest2 = rest[3:]
    kept = dv.u.copy()
    assert dv.uniform_fallback(7, rest2) == int(ref.choice(rest2))
    np.testing.assert_array_equal(dv.u[:8], kept[:8])
    np.testing.assert_array_equal(dv.u[8:], ref.random_sample(K - 2 - 7))

    assert _Deviates(seed, N, 1).u.size == 0                                # K = 1: no draw at all
