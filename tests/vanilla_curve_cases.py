"""Shared by test_vanilla_vjp_host.py and test_gpu_vanilla_vjp.py: the rows and cotangents of the vector-Jacobian product of
the vanilla decoder (geo_vanilla_vjp), its fp64 / float32 autograd references (computed once per case, read-only) and the
kernels' algorithm restated in torch from the export's packed tensors.  Decoders come from vanilla_jvp_cases."""
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

import vanilla_jvp_cases as V

# The accuracy gate's cases: name -> how many of the 2085 rows float32 autograd on the CPU itself leaves outside 1e-5 of
# fp64 autograd (ReLU-boundary rows; the gate's cap is 10, check_against_fp64's own).  Counted on the CPU with the seeds
# below; count again after changing a name, a width or a seed (PYTHONPATH=. python tests/vanilla_curve_cases.py).  The count
# moves with the CPU's float32 kernels and thread count (wide-bn-32x1-d2: 5 on one machine, 13 on another), so it documents
# the inputs and gates nothing.  narrow-none-32x1-d1 has 38 and is left out of the accuracy gate (it stays in the exactness
# tests).
VJP_CASES = {
    "wide-bn-28": 3,
    "wide-bn-32x3": 3,
    "narrow-none-28": 0,
    "narrow-none-32x3-d5": 3,
    "wide-none-28x3-d127": 1,
    "narrow-bn-28x3-d33": 0,
    "c0-192-bn-28-d65": 2,
    "c0-48-none-32x3-d7": 2,
    "narrow-plainbn-28x1-d12": 2,
    "wide-bn-32x1-d2": 5,
}
EXACT_CASES = ("wide-bn-32x3", "narrow-none-28", "narrow-none-32x1-d1", "wide-bn-32x1-d2", "wide-none-28x3-d127")
N_ROWS = V.N_EDGES
BOUNDARY_CAP = 10                       # of 2085 rows: the 0.5 % of check_against_fp64


def spec(name):
    return V.CASES[name] if name in V.CASES else V.ENVELOPE_CASES[name]


@functools.lru_cache(maxsize=None)
def decoder(name):
    channels, d, C, size, norm = spec(name)
    return V.build(channels, d, C, size, norm, seed=len(name))


def n_out(name):
    _, _, C, size, _ = spec(name)
    return C * size * size


@functools.lru_cache(maxsize=None)
def rows(name):
    """(z f32 [2085, d], u f32 [2085, nout]); read-only."""
    d = spec(name)[1]
    z = V.make_edges(d)[0]
    u = torch.randn(N_ROWS, n_out(name), generator=torch.Generator().manual_seed(2))
    return z, u


def autograd_vjp(dec, z, u, dtype) -> np.ndarray:
    """J(z_i)^T u_i, J = d sigmoid(dec(z)) / dz, by torch autograd on a CPU copy of the eval-mode decoder in `dtype` (with fixed
    statistics a row's image depends on its own latent alone, so one backward pass of sum_i g_i . u_i gives every row)."""
    dd = copy.deepcopy(dec).cpu().to(dtype).eval()
    out = []
    for lo in range(0, z.shape[0], 512):
        zz = z[lo:lo + 512].cpu().to(dtype).clone().requires_grad_(True)
        g = torch.sigmoid(dd(zz)).reshape(zz.shape[0], -1)
        out.append(torch.autograd.grad((g * u[lo:lo + 512].cpu().to(dtype)).sum(), zz)[0])
    return torch.cat(out).double().numpy()


def autograd_jvp(dec, z, dz, dtype) -> np.ndarray:
    """J(z_i) dz_i [n, nout] by forward-mode autograd, same conventions."""
    dd = copy.deepcopy(dec).cpu().to(dtype).eval()
    _, t = torch.autograd.functional.jvp(lambda zz: torch.sigmoid(dd(zz)).reshape(zz.shape[0], -1), z.cpu().to(dtype),
                                         dz.cpu().to(dtype))
    return t.double().numpy()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(fp64 autograd VJP, float32 autograd VJP) of rows(name), float64 arrays [2085, d]; read-only."""
    z, u = rows(name)
    return autograd_vjp(decoder(name), z, u, torch.float64), autograd_vjp(decoder(name), z, u, torch.float32)


def row_error(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """Per row |got - want|_2 / |want|_2 in fp64."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)


def emulate_vjp(ex, z, u) -> torch.Tensor:
    """The kernels' passes in fp64 torch from the export's tensors alone: the point pass from `tensors` (as
    test_vanilla_jvp_host._emulate), the three layers backwards from `adjoint` (w3t by tap and channel, w2t and Atq unpacked
    from their K quads)."""
    T = {k: v.double().cpu() for k, v in {**ex.tensors, **ex.adjoint}.items()}
    d, c1, c2, C, S = ex.desc.latent_dim, ex.desc.c1, ex.desc.c2, ex.desc.out_channels, ex.desc.out_size
    s1, s2 = S // 4, S // 2
    w2 = T["w2p"].permute(0, 1, 2, 4, 3).reshape(4, 4, c1, c2)
    w3 = T["w3p"].permute(0, 1, 3, 2)

    def convt(x, w):                                                                 # x [B][s][s][cin] -> [B][2s][2s][cout]
        B, s = x.shape[0], x.shape[1]
        xp = F.pad(x, (0, 0, 1, 1, 1, 1))
        out = torch.zeros(B, 2 * s, 2 * s, w.shape[3], dtype=x.dtype)
        for py in (0, 1):
            for px in (0, 1):
                for a in (0, 1):
                    for b in (0, 1):
                        out[:, py::2, px::2] += xp[:, 1 + py - a:1 + py - a + s, 1 + px - b:1 + px - b + s] @ w[2 * py + px][2 * a + b]
        return out

    def pull(x, w):                                      # x [B][2s][2s][cout], w [16 taps][cout][cin] -> [B][s][s][cin]
        B, s = x.shape[0], x.shape[1] // 2
        xp = F.pad(x, (0, 0, 1, 1, 1, 1))                # padded index = pixel + 1: input (y, x) reads 2 y - 1 + ky -> 2 y + ky
        out = torch.zeros(B, s, s, w.shape[2], dtype=x.dtype)
        for ky in range(4):
            for kx in range(4):
                out += xp[:, ky:ky + 2 * s:2, kx:kx + 2 * s:2] @ w[4 * ky + kx]
        return out

    z, u = z.double().cpu(), u.double().cpu()
    n = z.shape[0]
    pre1 = (z @ T["At"][:d] + T["c"]).view(n, s1, s1, c1)
    pre2 = T["scale2"] * convt(pre1.clamp(min=0), w2) + T["shift2"]
    sig = torch.sigmoid(convt(pre2.clamp(min=0), w3) + T["b3"])                      # [n][S][S][C]
    u3 = sig * (1 - sig) * u.view(n, C, S, S).permute(0, 2, 3, 1)
    w3t = T["w3t"]                                                                   # [16][C][c2]
    u2 = pull(u3, w3t) * T["scale2"] * (pre2 > 0)
    w2t = T["w2t"].permute(0, 1, 3, 2).reshape(16, c2, c1)                           # K quads back to [tap][co][ci]
    u1 = (pull(u2, w2t) * (pre1 > 0)).reshape(n, s1 * s1 * c1)
    dn = T["Atq"].shape[1]
    Atn = T["Atq"].permute(0, 2, 1).reshape(s1 * s1 * c1, dn)                        # [n1][dn]
    out = u1 @ Atn
    assert not out[:, d:].any()
    return out[:, :d]


if __name__ == "__main__":                               # recount the boundary rows of float32 autograd
    for case_name in list(VJP_CASES) + ["narrow-none-32x1-d1"]:
        ref64, ref32 = reference(case_name)
        e = row_error(ref32, ref64)
        print(f"{case_name}: float32 autograd median {np.median(e):.2e}, q99 {np.quantile(e, 0.99):.2e}, "
              f"rows above 1e-5: {int((e > 1e-5).sum())}")
