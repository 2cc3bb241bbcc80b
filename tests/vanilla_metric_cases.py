"""Shared by test_vanilla_metric_host.py, test_gpu_vanilla_metric.py and test_gpu_sym_spectrum.py: the cases of the vanilla
decoder's metric tensor (decoders from vanilla_curve_cases), their fp64 references by forward-mode autograd on the CPU (computed
once per case, read-only) and the symmetric matrices the eigenvalue kernel is tested on."""
import copy
import functools

import numpy as np
import torch

import vanilla_curve_cases as K

# the accuracy cases: every width, both sizes and channel counts, d from 1 to 128
CASES = ("wide-bn-28", "wide-bn-32x3", "narrow-none-28", "narrow-none-32x3-d5", "wide-none-28x3-d127", "narrow-bn-28x3-d33",
         "c0-192-bn-28-d65", "narrow-none-32x1-d1", "wide-bn-32x1-d2")
# cond(G64) <= 1e3 over the 33 latents (the table in DESIGN.md section 30; asserted where it is used): the cases that gate logvol.
# With 784 .. 3072 outputs for at most 128 latent dimensions every case is (cond <= 12).
WELL_CONDITIONED = CASES
EXACT_CASES = ("wide-bn-32x3", "narrow-none-28", "narrow-none-32x1-d1", "wide-none-28x3-d127")
N_LATENTS = 33                      # an odd count: the last latent is its own partner in the unit-tangent pass
DBL_EPS = float(np.finfo(np.float64).eps)
FLT_EPS = float(np.finfo(np.float32).eps)


def latent_dim(name):
    return K.spec(name)[1]


RELU_MARGIN = 1e-5                  # of a layer's rms pre-activation: 100 x what float32 arithmetic moves a pre-activation by


def relu_margin(dec, z) -> np.ndarray:
    """Per latent the smallest |pre-activation| of either ReLU layer relative to the layer's rms, on the fp64 module."""
    dd = copy.deepcopy(dec).cpu().double().eval()
    seen = []

    def hook(_module, args):
        x = args[0].detach().reshape(args[0].shape[0], -1)
        seen.append((x.abs().min(1).values / x.pow(2).mean(1).sqrt()).numpy())

    for m in dd.modules():
        if isinstance(m, torch.nn.ReLU):
            m.register_forward_pre_hook(hook)
    with torch.no_grad():
        dd(z.double())
    assert len(seen) == 2
    return np.minimum(*seen)


@functools.lru_cache(maxsize=None)
def _accuracy_rows(name, n):
    z = K.rows(name)[0][:8 * n]
    rows = np.flatnonzero(relu_margin(K.decoder(name), z) > RELU_MARGIN)[:n]
    assert rows.size == n
    return rows


def latents(name, n=N_LATENTS) -> torch.Tensor:
    """z f32 [n, d] of the accuracy gates: the first n rows of vanilla_curve_cases.rows that keep every ReLU input of the fp64
    module further than RELU_MARGIN from 0.  J is discontinuous where a ReLU input crosses 0: a latent that float32 arithmetic
    puts on the other side has a Jacobian no float32 route determines (a whole latent's d columns and its G at once, so the
    2085-row cap of vanilla_curve_cases for such rows does not scale down to 33 latents); the exactness tests use every row."""
    return K.rows(name)[0][torch.from_numpy(_accuracy_rows(name, n))].clone()


def columns(dec, z, dtype) -> np.ndarray:
    """J [n, d, nout] (float64 array): J[i][k] = d sigmoid(dec(z_i)) / dz_k by forward-mode autograd of unit vectors on a CPU
    copy of the eval-mode decoder in `dtype`."""
    n, d = z.shape
    eye = torch.eye(d).repeat(8, 1)
    out = []
    for lo in range(0, n, 8):
        zz = z[lo:lo + 8].repeat_interleave(d, dim=0)
        out.append(K.autograd_jvp(dec, zz, eye[:zz.shape[0]], dtype).reshape(zz.shape[0] // d, d, -1))
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(z f32 [33, d], J64 [33, d, nout], G64 [33, d, d]) of a case by fp64 autograd on the CPU; read-only."""
    z = latents(name)
    J64 = columns(K.decoder(name), z, torch.float64)
    G64 = np.einsum("nao,nbo->nab", J64, J64)
    J64.setflags(write=False)
    G64.setflags(write=False)
    return z, J64, G64


@functools.lru_cache(maxsize=None)
def reference32(name):
    """J32 [33, d, nout]: float32 autograd on the CPU at the same latents, the yardstick of the columns; read-only."""
    J32 = columns(K.decoder(name), latents(name), torch.float32)
    J32.setflags(write=False)
    return J32


def boundary_cap(rows: int) -> int:
    """vanilla_curve_cases.BOUNDARY_CAP (10 of 2085 rows above 1e-5: rows at a ReLU boundary) scaled to `rows`, rounded up."""
    return int(np.ceil(K.BOUNDARY_CAP * rows / K.N_ROWS))


# ------------------------------------------------------------------------------------------------ symmetric test matrices
SPECTRUM_DIMS = (1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128)
SPECTRUM_P_OUT = 3072               # the p_out of the rank rule in the eigenvalue kernel's tests
SPECTRA = ("geometric", "equal", "cluster", "rank1", "diagonal", "zero", "blocks")


def spectrum_values(kind, d):
    """The eigenvalues a matrix of `kind` is built from (None: rank1 and blocks state theirs through the matrix)."""
    if kind == "geometric":                                  # 12 decades, none within a factor 8 of the rank threshold
        s = np.geomspace(1e-12, 1.0, d) if d > 1 else np.ones(1)
        thr = (SPECTRUM_P_OUT * FLT_EPS) ** 2
        s[(s >= thr / 8) & (s < thr)] = thr / 8
        s[(s >= thr) & (s <= thr * 8)] = thr * 8
        return s
    if kind == "equal":
        return np.full(d, 3.0)
    if kind == "cluster":
        return np.concatenate([np.full(d // 2, 2.0), np.linspace(0.25, 7.0, d - d // 2)])
    if kind == "diagonal":
        return np.linspace(0.5, 9.0, d)[np.random.RandomState(d).permutation(d)]
    return None


def matrix(kind, d, seed=0) -> np.ndarray:
    """A symmetric fp64 [d, d] matrix: Q diag(s) Q^T with Q from a seeded QR (geometric over 12 decades, all equal, a repeated
    cluster plus a spread), v v^T (rank 1), a diagonal matrix, the zero matrix, or 2 x 2 blocks on the diagonal."""
    r = np.random.RandomState(1000 * d + seed)
    if kind == "zero":
        return np.zeros((d, d))
    if kind == "diagonal":
        return np.diag(spectrum_values(kind, d))
    if kind == "rank1":
        v = r.randn(d)
        return np.outer(v, v)
    if kind == "blocks":
        A = np.zeros((d, d))
        for i in range(0, d - 1, 2):
            a, b, c = 1.0 + r.rand(), 1.0 + r.rand(), 0.4 * (2.0 * r.rand() - 1.0)     # eigenvalues in [0.6, 2.4]
            A[i, i], A[i + 1, i + 1], A[i, i + 1], A[i + 1, i] = a, b, c, c
        if d % 2:
            A[d - 1, d - 1] = 1.5
        return A
    Q, _ = np.linalg.qr(r.randn(d, d))
    A = (Q * spectrum_values(kind, d)) @ Q.T
    return np.triu(A) + np.triu(A, 1).T
