"""The EMA vector quantizer's rules restated in numpy, for the tests: fp64 keys and sums, float32
wherever the rules name float32.  Written from the rules, independent of the project's code."""
import numpy as np

f32 = np.float32


def rows(z: np.ndarray) -> np.ndarray:
    """NCHW -> (B H W, C) float32."""
    return np.ascontiguousarray(z.transpose(0, 2, 3, 1).reshape(-1, z.shape[1])).astype(f32)


def keys(x: np.ndarray, e: np.ndarray) -> np.ndarray:
    """fp64 |x - e|^2 for every row and code."""
    x, e = np.asarray(x, np.float64), np.asarray(e, np.float64)
    return ((x[:, None, :] - e[None]) ** 2).sum(-1)


def labels(x: np.ndarray, e: np.ndarray) -> np.ndarray:
    return keys(x, e).argmin(1)   # first minimum: ties to the lowest code


def ema(cs, ea, counts, sums, decay, eps):
    """New (cluster_size, embed_avg, embed), float32."""
    K = len(cs)
    d32, omd = f32(decay), f32(1.0 - decay)
    cs = (cs.astype(f32) * d32 + counts.astype(f32) * omd).astype(f32)
    ea = (ea.astype(f32) * d32 + sums.astype(f32) * omd).astype(f32)
    n = f32(cs.astype(np.float64).sum())
    norm = np.maximum((cs + f32(eps)) / (n + f32(K * eps)) * n, f32(eps)).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        emb = ea / norm[:, None]
    emb = np.clip(np.nan_to_num(emb, nan=0.0, posinf=1.0, neginf=-1.0), -2, 2).astype(f32)
    return cs, ea, emb


def forward(z, embed, cs, ea, training, decay=0.99, eps=1e-5, beta=0.25, idx=None):
    """Outputs of one forward, and the buffers after it.  idx: use these labels instead of computing them."""
    B, C, H, W = z.shape
    x = rows(z)
    K = embed.shape[0]
    if idx is None:
        idx = labels(x, embed)
    idx = np.asarray(idx).reshape(-1)
    zq = embed[idx].reshape(B, H, W, C).transpose(0, 3, 1, 2).astype(f32)
    ze = z.astype(f32)
    st = (ze + (zq - ze)).astype(f32)
    counts = np.bincount(idx, minlength=K)
    out = {"idx": idx.reshape(B, H, W), "z_q": zq, "z_q_st": st,
           "loss": f32(f32(beta) * f32(((st.astype(np.float64) - ze) ** 2).mean())),
           "q_mse": f32(((zq.astype(np.float64) - ze) ** 2).mean())}
    p = counts / max(counts.sum(), 1)
    out["perplex"] = f32(np.exp(-(p * np.log(p + 1e-12)).sum()))
    out["usage"] = f32((counts > 0).mean())
    out["dead"] = f32(1) - out["usage"]
    out["counts"] = counts
    if training:
        sums = np.zeros((K, C), np.float64)
        np.add.at(sums, idx, x.astype(np.float64))
        out["cluster_size"], out["embed_avg"], out["embed"] = ema(cs, ea, counts, sums, decay, eps)
    else:
        out["cluster_size"], out["embed_avg"], out["embed"] = cs, ea, embed
    return out


def backward(g_st, g_loss, z, st, beta=0.25):
    """fp64 grad of z_e: g_st + g_loss beta 2 / numel (z_e - z_q_st)."""
    z64 = np.asarray(z, np.float64)
    return np.asarray(g_st, np.float64) + float(g_loss) * beta * 2.0 / z64.size * (z64 - np.asarray(st, np.float64))
