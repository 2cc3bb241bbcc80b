"""The reference's baseline VQ-VAE (baseline VQVAE/vqvae_cifar10_clean/models/vqvae.py) with the same constructor signatures,
forward tuples, module order and state_dict keys, so that `torch.manual_seed(s); VQVAE(**cfg)` draws the reference's initial
weights and checkpoints load both ways.

VectorQuantizerEMA runs on CUDA tensors through the HIP quantizer (csrc/kmeans.hip, geo_vq_forward / geo_vq_backward) inside an
autograd.Function; on CPU tensors the same rules run in torch with fp64 keys and sums:
  idx      argmin over codes of the fp64 key |x - e|^2, ties to the lowest code, a NaN key first (torch.argmin's rule): a
           row with a NaN or an infinite value gets code 0, its z_q_st and the loss come out NaN, as in the reference;
  z_q      embed[idx] before the update; z_q_st = z_e + (z_q - z_e) in float32;
  loss     beta * mean((z_q_st - z_e)^2), the mean an fp64 sum rounded once;
  EMA      (training only) cluster_size = cs decay + counts (1 - decay); embed_avg = ea decay + sums (1 - decay) with the
           per-code sums in fp64 rounded once; n = sum cs; norm = max((cs + eps) / (n + K eps) n, eps);
           embed = clamp(nan_to_num(embed_avg / norm, 0, 1, -1), -2, 2).
Every forward also leaves `last_stats`, a float32 tensor on z_e's device: (q_mse, perplexity, usage, dead) of the batch, the
per-batch codebook metrics of the reference's training loop, without a host sync.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib


class ResBlock(nn.Module):
    def __init__(self, ch):
        super().__init__()
        # the leading ReLU is in place, as in the reference: the skip connection adds relu(x), not x
        self.block = nn.Sequential(nn.ReLU(inplace=True), nn.Conv2d(ch, ch, 3, padding=1), nn.ReLU(inplace=True),
                                   nn.Conv2d(ch, ch, 1))

    def forward(self, x):
        return x + self.block(x)


class Encoder(nn.Module):
    def __init__(self, in_ch=3, hidden=256, z_ch=128, n_res=2):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(in_ch, hidden // 2, 4, 2, 1), nn.ReLU(True),
                                  nn.Conv2d(hidden // 2, hidden, 4, 2, 1), nn.ReLU(True),
                                  nn.Conv2d(hidden, z_ch, 3, 1, 1))
        self.res = nn.Sequential(*[ResBlock(z_ch) for _ in range(n_res)])
        self.out = nn.Conv2d(z_ch, z_ch, 1)

    def forward(self, x):
        return self.out(self.res(self.stem(x)))


class Decoder(nn.Module):
    def __init__(self, out_ch=3, hidden=256, z_ch=128, n_res=2):
        super().__init__()
        self.inp = nn.Conv2d(z_ch, z_ch, 1)
        self.res = nn.Sequential(*[ResBlock(z_ch) for _ in range(n_res)])
        self.head = nn.Sequential(nn.ReLU(True), nn.ConvTranspose2d(z_ch, hidden, 4, 2, 1), nn.ReLU(True),
                                  nn.ConvTranspose2d(hidden, hidden // 2, 4, 2, 1), nn.ReLU(True),
                                  nn.Conv2d(hidden // 2, out_ch, 1), nn.Tanh())

    def forward(self, z_q):
        return self.head(self.res(self.inp(z_q)))


def _ptr(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


def _workspace(nbytes: int, dev) -> torch.Tensor:
    """The quantizer's scratch: one exact-size allocation per call from the stream-ordered caching allocator (no device sync)."""
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


class _VQFunction(torch.autograd.Function):
    """HIP forward (labels, z_q, z_q_st, idx, loss, stats and, in training, the EMA update in place) and backward."""

    @staticmethod
    def forward(ctx, z_e, embed, cluster_size, embed_avg, training, decay, eps, beta):
        B, C, H, W = z_e.shape
        if z_e.dtype not in (torch.float32, torch.float16):
            raise TypeError(f"VectorQuantizerEMA on the GPU takes float32 or float16 z_e, not {z_e.dtype}")
        dev = z_e.device
        K = embed.shape[0] if embed.dim() == 2 else -1
        for name, t, shape in (("embed", embed, (K, C)), ("cluster_size", cluster_size, (K,)), ("embed_avg", embed_avg, (K, C))):
            if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
                raise ValueError(f"VectorQuantizerEMA: {name} must be a contiguous float32 tensor of shape {shape} on {dev} for "
                                 f"z_e of {C} channels; got {t.dtype} {tuple(t.shape)} on {t.device}")
        z = z_e.detach().contiguous()
        n = B * H * W
        L = _lib.load()
        nbytes = L.geo_vq_workspace_bytes(n, C, K)
        if nbytes == 0:
            raise _lib.GeoHipError(f"geo_vq_workspace_bytes rejected n={n} C={C} K={K} (C <= 128, K <= 4096)")
        ws = _workspace(nbytes, dev)
        z_q = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
        z_q_st = torch.empty_like(z_q)
        idx = torch.empty(B, H, W, dtype=torch.int64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        stats = torch.empty(4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(L.geo_vq_forward(_ptr(z), int(z.dtype == torch.float16), B, C, H * W, _ptr(embed), _ptr(cluster_size),
                                        _ptr(embed_avg), K, int(bool(training)), float(decay), float(eps), float(beta),
                                        _ptr(z_q), _ptr(z_q_st), _ptr(idx), _ptr(loss), _ptr(stats), None, _ptr(ws), nbytes,
                                        stream), "geo_vq_forward")
        ctx.save_for_backward(z, z_q_st)
        ctx.beta = float(beta)
        ctx.mark_non_differentiable(idx, z_q, stats)
        return z_q_st, loss, idx, z_q, stats

    @staticmethod
    def backward(ctx, g_st, g_loss, _g_idx, _g_zq, _g_stats):
        z, z_q_st = ctx.saved_tensors
        grad = torch.empty_like(z)
        g_st = None if g_st is None else g_st.float().contiguous()
        g_loss = None if g_loss is None else g_loss.float().contiguous()
        with torch.cuda.device(z.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(z.device).cuda_stream)
            _lib.check(_lib.load().geo_vq_backward(None if g_st is None else _ptr(g_st), None if g_loss is None else _ptr(g_loss),
                                                   ctx.beta, _ptr(z), int(z.dtype == torch.float16), _ptr(z_q_st), z.numel(),
                                                   _ptr(grad), stream), "geo_vq_backward")
        return grad, None, None, None, None, None, None, None


def nearest_codes(flat: torch.Tensor, embed: torch.Tensor) -> torch.Tensor:
    """Host rule: argmin over codes of the fp64 key sum_c (x_c - e_c)^2, first minimum (i64 [n])."""
    x, e = flat.double(), embed.double()
    step = max(1, (1 << 22) // max(1, e.numel()))
    out = [((x[i:i + step, None, :] - e[None]) ** 2).sum(-1).argmin(1) for i in range(0, x.shape[0], step)]
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.int64)


def batch_stats(counts: torch.Tensor, q_mse: torch.Tensor) -> torch.Tensor:
    """(q_mse, perplexity, usage, dead) from integer counts, in fp64, as float32 on the counts' device."""
    c = counts.double()
    p = c / max(float(c.sum()), 1.0)
    usage = ((c > 0).double().mean()).float()
    return torch.stack([q_mse.float(), torch.exp(-(p * (p + 1e-12).log()).sum()).float(), usage, 1.0 - usage])


class VectorQuantizerEMA(nn.Module):
    def __init__(self, n_codes=512, code_dim=128, decay=0.99, eps=1e-5, beta=0.25):
        super().__init__()
        self.n_codes = n_codes
        self.code_dim = code_dim
        self.beta = beta
        init = torch.randn(n_codes, code_dim)
        self.register_buffer("embed", init)
        self.register_buffer("cluster_size", torch.zeros(n_codes))
        self.register_buffer("embed_avg", init.clone())
        self.decay = decay
        self.eps = eps
        self.last_stats = None

    def forward(self, z_e):
        if z_e.is_cuda:
            z_q_st, loss, idx, z_q, stats = _VQFunction.apply(z_e, self.embed, self.cluster_size, self.embed_avg, self.training,
                                                              self.decay, self.eps, self.beta)
            self.last_stats = stats
            return z_q_st, loss, idx, z_q, z_e
        return self._forward_host(z_e)

    def _forward_host(self, z_e):
        B, C, H, W = z_e.shape
        flat = z_e.detach().permute(0, 2, 3, 1).reshape(-1, C).float()
        idx = nearest_codes(flat, self.embed)
        z_q = self.embed.index_select(0, idx).view(B, H, W, C).permute(0, 3, 1, 2).contiguous()
        counts = torch.bincount(idx, minlength=self.n_codes)
        if self.training:
            with torch.no_grad():
                sums = torch.zeros(self.n_codes, C, dtype=torch.float64).index_add_(0, idx, flat.double())
                self.ema_update(counts, sums)
        z_q_st = z_e + (z_q - z_e).detach()
        loss = self.beta * F.mse_loss(z_q_st.detach().double(), z_e.double()).float()
        q_mse = F.mse_loss(z_q.double(), z_e.detach().double())
        self.last_stats = batch_stats(counts, q_mse)
        return z_q_st, loss, idx.view(B, H, W), z_q, z_e

    @torch.no_grad()
    def ema_update(self, counts: torch.Tensor, sums: torch.Tensor) -> None:
        """The EMA step on the buffers from integer counts [K] and fp64 per-code sums [K][C] (host path)."""
        omd = 1.0 - self.decay
        self.cluster_size.mul_(self.decay).add_(counts.to(self.cluster_size.dtype), alpha=omd)
        self.embed_avg.mul_(self.decay).add_(sums.to(self.embed_avg.dtype), alpha=omd)
        n = self.cluster_size.double().sum().float()
        norm = ((self.cluster_size + self.eps) / (n + self.n_codes * self.eps) * n).clamp_min(self.eps)
        new = torch.nan_to_num(self.embed_avg / norm.unsqueeze(1), nan=0.0, posinf=1.0, neginf=-1.0).clamp_(-2.0, 2.0)
        self.embed.copy_(new)

    @torch.no_grad()
    def reseed_dead_codes(self, min_count: int = 5, sample_bank: torch.Tensor = None):
        """Codes whose EMA cluster size is below min_count take rows of sample_bank (N, C) drawn by torch.randperm on the
        bank's device; returns how many were reseeded (0 without a bank or on a dimension mismatch)."""
        if sample_bank is None or sample_bank.numel() == 0:
            return 0
        dead = self.cluster_size < float(min_count)
        n_dead = int(dead.sum().item())
        if n_dead == 0 or sample_bank.size(1) != self.code_dim:
            return 0
        take = min(n_dead, sample_bank.size(0))
        pick = torch.randperm(sample_bank.size(0), device=sample_bank.device)[:take]
        rows = sample_bank[pick]
        where = dead.nonzero(as_tuple=False).view(-1)[:take]
        self.embed[where] = rows.to(self.embed.dtype)
        self.embed_avg[where] = self.embed[where]
        self.cluster_size[where] = float(min_count)
        return int(take)


class VQVAE(nn.Module):
    def __init__(self, in_channels=3, z_channels=128, hidden=256, n_res_blocks=2, n_codes=512, beta=0.25, ema_decay=0.99,
                 ema_eps=1e-5):
        super().__init__()
        self.enc = Encoder(in_ch=in_channels, hidden=hidden, z_ch=z_channels, n_res=n_res_blocks)
        self.quant = VectorQuantizerEMA(n_codes=n_codes, code_dim=z_channels, decay=ema_decay, eps=ema_eps, beta=beta)
        self.dec = Decoder(out_ch=in_channels, hidden=hidden, z_ch=z_channels, n_res=n_res_blocks)

    def forward(self, x):
        z_q_st, loss_vq, idx, z_q, z_e = self.quant(self.enc(x))
        return self.dec(z_q_st), loss_vq, idx, z_q, z_e


def model_from_config(cfg: dict) -> VQVAE:
    """VQVAE(**) from the reference's config.yaml "model" section."""
    m = cfg["model"]
    return VQVAE(in_channels=m["in_channels"], z_channels=m["z_channels"], hidden=m["hidden"], n_res_blocks=m["n_res_blocks"],
                 n_codes=m["n_codes"], beta=m["beta"], ema_decay=m["ema_decay"], ema_eps=m["ema_eps"])
