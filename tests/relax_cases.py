"""Cases, curves and the numpy restatement shared by tests/test_relax_host.py and tests/test_gpu_relax.py.

Decoders come from tests/metric_tensor_cases.py: the five NATIVE cases (d of 1, 5 and 16, p_out of 16 and 192, BatchNorm-eval,
GroupNorm and no norm) and fm_small for the torch route.  The curves are zig-zags about a chord.  The restatement runs no code
of the project: Evaluate and the relax loop in numpy fp64 with explicit ascending sums (np.sum is pairwise), every product and
every sum an operation of its own."""
import numpy as np

from metric_tensor_cases import CASES, NATIVE, make_decoder, p_out_of  # noqa: F401  (re-exported to the tests)

FRAMES = (5, 9)
RELAX_ITERS = 20


def zigzag(d, F, index=0):
    """One curve f32 [F, d]: rs = RandomState(5 + F); a, b, zig = rs.randn(d) three times, zig normalised; the frames of the chord
    a -> b; odd interior frames + 0.5 zig, even interior frames - 0.5 zig.  index > 0: further curves, RandomState(5 + F + 1000 index)."""
    rs = np.random.RandomState(5 + F + 1000 * index)
    a, b, zig = rs.randn(d), rs.randn(d), rs.randn(d)
    zig = zig / np.linalg.norm(zig)
    t = (np.arange(F) / (F - 1))[:, None]
    x = a[None, :] + t * (b - a)[None, :]
    for f in range(1, F - 1):
        x[f] += 0.5 * zig if f % 2 == 1 else -0.5 * zig
    return x.astype(np.float32)


def zigzags(d, F, C):
    return np.stack([zigzag(d, F, i) for i in range(C)])


def evaluate(g, jac, x=None):
    """(energy [C], seg_sq [C, F-1], grad [C, F, d], tr [C, F]) fp64 from g f32 [C, F, p] and jac f32 [C, F, d, p]; with the
    frames x [C, F, d], energy = NaN for a curve with a NaN or an inf among its coordinates."""
    g64, J64 = np.asarray(g, dtype=np.float32).astype(np.float64), np.asarray(jac, dtype=np.float32).astype(np.float64)
    C, F, p = g64.shape
    d = J64.shape[2]
    with np.errstate(invalid="ignore", over="ignore"):
        dseg = g64[:, 1:] - g64[:, :-1]
        seg = np.zeros((C, F - 1))
        for o in range(p):
            seg = seg + dseg[:, :, o] * dseg[:, :, o]
        energy = np.zeros(C)
        for f in range(F - 1):
            energy = energy + seg[:, f]
        grad = np.zeros((C, F, d))
        if F > 2:
            r = (g64[:, 1:-1] - g64[:, :-2]) - (g64[:, 2:] - g64[:, 1:-1])
            s = np.zeros((C, F - 2, d))
            for o in range(p):
                s = s + J64[:, 1:-1, :, o] * r[:, :, None, o]
            grad[:, 1:-1] = 2.0 * s
        row = np.zeros((C, F, d))
        for o in range(p):
            row = row + J64[:, :, :, o] * J64[:, :, :, o]
        tr = np.zeros((C, F))
        for k in range(d):
            tr = tr + row[:, :, k]
    if x is not None:
        energy = np.where(np.isfinite(np.asarray(x)).all(axis=(1, 2)), energy, np.nan)
    return energy, seg, grad, tr


def step0(tr):
    """1 / (8 * max over interior f of tr[f]), 0 where that maximum is 0 (a NaN never becomes the maximum)."""
    m = np.zeros(tr.shape[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        for f in range(1, tr.shape[1] - 1):
            m = np.where(tr[:, f] > m, tr[:, f], m)
        return np.where(m > 0, 1.0 / (8.0 * np.where(m > 0, m, 1.0)), 0.0)


def trial(x, step, grad):
    """y[f] = (float)((double)x[f] - step * grad[f]) for interior f, the ends copied."""
    y = np.array(x, dtype=np.float32, copy=True)
    with np.errstate(invalid="ignore", over="ignore"):
        if y.shape[1] > 2:
            y[:, 1:-1] = (x[:, 1:-1].astype(np.float64) - step[:, None, None] * grad[:, 1:-1]).astype(np.float32)
    return y


def decide(E, Ey, step):
    """(take, new step): E_y < E strictly (False for a NaN), step * 2 or step / 4."""
    with np.errstate(invalid="ignore"):
        take = Ey < E
    return take, np.where(take, 2.0 * step, step / 4.0)


def relax(outputs_jac, x, n_iters, step=None):
    """The relax loop over outputs_jac(x f32 [C, F, d]) -> (g, jac): (x, energy0, energy, seg_sq, step, accepted)."""
    x = np.array(x, dtype=np.float32, copy=True)
    E, seg, grad, tr = evaluate(*outputs_jac(x), x)
    energy0 = E.copy()
    step = step0(tr) if step is None else np.where(np.asarray(step) < 0, step0(tr), np.asarray(step, dtype=np.float64))
    accepted = np.zeros(x.shape[0], dtype=np.int32)
    for _ in range(n_iters if x.shape[1] > 2 else 0):
        y = trial(x, step, grad)
        Ey, segy, grady, _ = evaluate(*outputs_jac(y), y)
        take, step = decide(E, Ey, step)
        x[take], grad[take], seg[take], E[take] = y[take], grady[take], segy[take], Ey[take]
        accepted += take.astype(np.int32)
    return x, energy0, E, seg, step, accepted


def bits(a):
    a = np.ascontiguousarray(a)
    return a.dtype.str, a.shape, a.tobytes()
