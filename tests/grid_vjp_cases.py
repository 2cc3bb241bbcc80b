"""Shared by the grid VJP / grid relaxation tests: the decoders (decode_cases' spatial tables), the rows and
cotangents of geo_spatial_vjp with their fp64 / float32 autograd references (computed once per case, read-only), the kernels'
backward pass restated in fp64 torch from the export's `adjoint` packs, and numpy restatements of the curve rules that run no
project code."""
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

import decode_cases as D

ALL_CASES = {**D.SPATIAL_CASES, **D.SPATIAL_ENVELOPE_CASES}
CURVE_CASES = ("wide-bn-28-d16", "wide-bn-32x3-d32", "narrow-none-28-d5", "narrow-bn-28x3-d63")
CURVE_SHAPES = ((3, 5), (3, 9), (1, 3), (7, 5), (2, 2), (1, 64))
N_ROWS = 260
BOUNDARY_CAP = 4                        # of 260 rows: ReLU-boundary mask flips


def spec(name):
    return ALL_CASES[name]


@functools.lru_cache(maxsize=None)
def decoder(name):
    channels, d, C, size, norm = spec(name)
    return D.build_spatial(channels, d, C, size, norm, seed=len(name))


@functools.lru_cache(maxsize=None)
def rows(name):
    """(z f32 [260, d, 4, 4], u f32 [260, C, S, S]); read-only."""
    _, d, C, size, _ = spec(name)
    return D.grids(N_ROWS, d, seed=3), torch.randn(N_ROWS, C, size, size, generator=torch.Generator().manual_seed(5))


def autograd_vjp(dec, z, u, dtype):
    """(J(z_i)^T u_i [n, 16 d], g [n, nout]) as float64 arrays, J = d sigmoid(dec(z)) / dz, by torch autograd on a CPU copy of the
    eval-mode decoder in `dtype` (fixed statistics: one backward pass of sum_i g_i . u_i gives every row)."""
    dd = copy.deepcopy(dec).cpu().to(dtype).eval()
    zz = z.cpu().to(dtype).clone().requires_grad_(True)
    g = torch.sigmoid(dd(zz))
    out = torch.autograd.grad((g * u.cpu().to(dtype).reshape(g.shape)).sum(), zz)[0]
    return out.double().reshape(z.shape[0], -1).numpy(), g.detach().double().reshape(z.shape[0], -1).numpy()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(vjp64, g64, vjp32, g32) of rows(name); read-only."""
    z, u = rows(name)
    return autograd_vjp(decoder(name), z, u, torch.float64) + autograd_vjp(decoder(name), z, u, torch.float32)


def row_error(got, want):
    got, want = np.asarray(got, np.float64).reshape(len(want), -1), np.asarray(want, np.float64).reshape(len(want), -1)
    return np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)


def padding_one_twin(dec):
    """The same weights with the last layer's padding 1: a 28-px decoder's 32-px twin."""
    twin = copy.deepcopy(dec)
    twin.deconv_layers[6].padding = (1, 1)
    return twin


def emulate_backward(ex, dec, z, u) -> torch.Tensor:
    """J^T u [n, d, 4, 4] in fp64 torch: the masks and sigmoid' from the fp64 module, the three layers backwards from the export's
    `adjoint` packs alone (w3t by tap and channel, w2t and w1t unpacked from their K quads; scale1 sits inside w1t)."""
    T = {k: v.double().cpu() for k, v in {**ex.tensors, **ex.adjoint}.items()}
    d, c1, c2, C, S = ex.desc.latent_dim, ex.desc.c1, ex.desc.c2, ex.desc.out_channels, ex.desc.out_size
    crop = (32 - S) // 2
    dd = copy.deepcopy(dec).double().eval()
    seq = dd.deconv_layers
    with torch.no_grad():
        pre1 = seq[1](seq[0](dd.conv_in(z.double())))
        pre2 = seq[4](seq[3](pre1.clamp(min=0)))
        sig = torch.sigmoid(seq[6](pre2.clamp(min=0)))                               # [n][C][S][S]

    def pull(x, w):                                      # x [B][2s][2s][cout], w [16 taps][cout][cin] -> [B][s][s][cin]
        B, s = x.shape[0], x.shape[1] // 2
        xp = F.pad(x, (0, 0, 1, 1, 1, 1))
        out = torch.zeros(B, s, s, w.shape[2], dtype=x.dtype)
        for ky in range(4):
            for kx in range(4):
                out += xp[:, ky:ky + 2 * s:2, kx:kx + 2 * s:2] @ w[4 * ky + kx]
        return out

    u3 = F.pad(sig * (1 - sig) * u.double().view(sig.shape), (crop,) * 4).permute(0, 2, 3, 1)      # [n][32][32][C]
    u2 = pull(u3, T["w3t"]) * T["scale2"] * (pre2 > 0).permute(0, 2, 3, 1)
    w2t = T["w2t"].permute(0, 1, 3, 2).reshape(16, c2, c1)
    u1 = pull(u2, w2t) * (pre1 > 0).permute(0, 2, 3, 1)
    dn = T["w1t"].shape[2]
    w1t = T["w1t"].permute(0, 1, 3, 2).reshape(16, c1, dn)
    out = pull(u1, w1t)                                                              # [n][4][4][dn]
    assert not out[..., d:].any()
    return out[..., :d].permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------- the curve rules in numpy
def sign_probe(C, S):
    c, y, x = np.meshgrid(np.arange(C), np.arange(S), np.arange(S), indexing="ij")
    return np.where((c + y + x) % 2 == 0, 1.0, -1.0).astype(np.float32)


def fold_256(v):
    """Sum of v f64 [p] in the kernels' order: partial sum t adds entries t, t + 256, ... ascending from 0, then
    p[t] += p[t + s] for s = 128, 64, ..., 1."""
    part = np.zeros(256)
    for lo in range(0, v.shape[0], 256):
        chunk = v[lo:lo + 256]
        part[:chunk.shape[0]] = part[:chunk.shape[0]] + chunk
    s = 128
    while s >= 1:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def restate_energy(g, x):
    """(energy [C], seg_sq [C, F-1], r f32 [C, F, p]) from the outputs g f32 [C, F, p] and the frames x [C, F, ...]."""
    g64 = np.asarray(g, np.float32).astype(np.float64)
    C, Fr, p = g64.shape
    seg = np.zeros((C, Fr - 1))
    energy = np.zeros(C)
    r = np.zeros((C, Fr, p), np.float32)
    for c in range(C):
        for f in range(Fr - 1):
            ahead = g64[c, f + 1] - g64[c, f]
            seg[c, f] = fold_256(ahead * ahead)
            energy[c] = energy[c] + seg[c, f]
            if f > 0:
                r[c, f] = ((g64[c, f] - g64[c, f - 1]) - ahead).astype(np.float32)
        if not np.isfinite(np.asarray(x[c], np.float32)).all():
            energy[c] = np.nan
    return energy, seg, r


def restate_probe(v):
    """v f64 [n, 16 d] = J^T s per frame -> sum over the coordinates, ascending, of the squares."""
    t = np.zeros(v.shape[0])
    for k in range(v.shape[1]):
        t = t + v[:, k] * v[:, k]
    return t


def restate_first_step(probe):
    """probe f64 [C, F] -> 1 / (8 max over the interior frames), 0 where that maximum is 0; a NaN is ignored."""
    out = np.zeros(probe.shape[0])
    for c in range(probe.shape[0]):
        m = 0.0
        for f in range(1, probe.shape[1] - 1):
            if probe[c, f] > m:
                m = probe[c, f]
        out[c] = 1.0 / (8.0 * m) if m > 0 else 0.0
    return out


def restate_trial(x, step, grad):
    """y[f] = (float)((double)x[f] - step * grad[f]) for interior f; the ends are copied.  x [C, F, ...], grad the same shape."""
    y = np.array(x, np.float32)
    if x.shape[1] > 2:
        y[:, 1:-1] = (x[:, 1:-1].astype(np.float64) - step.reshape(-1, *([1] * (x.ndim - 1))) * grad[:, 1:-1]).astype(np.float32)
    return y


def curves(name, C, Fr, seed=11):
    """Random curves of grids f32 [C, F, d, 4, 4]."""
    d = spec(name)[1]
    return D.grids(C * Fr, d, seed=seed + 100 * Fr + C).view(C, Fr, d, 4, 4).contiguous()


def zigzag_grids(d, Fr, C, amplitude=4.0):
    """relax_cases.zigzag's recipe over the 16 d coordinates (RandomState(5 + F + 1000 i)) with the zig's amplitude `amplitude`
    instead of 0.5, reshaped to [C, F, d, 4, 4]."""
    out = []
    for i in range(C):
        rs = np.random.RandomState(5 + Fr + 1000 * i)
        a, b, zig = rs.randn(16 * d), rs.randn(16 * d), rs.randn(16 * d)
        zig = zig / np.linalg.norm(zig)
        x = a[None, :] + (np.arange(Fr) / (Fr - 1))[:, None] * (b - a)[None, :]
        for f in range(1, Fr - 1):
            x[f] += amplitude * zig if f % 2 == 1 else -amplitude * zig
        out.append(x.astype(np.float32))
    return torch.from_numpy(np.stack(out)).view(C, Fr, d, 4, 4).contiguous()
