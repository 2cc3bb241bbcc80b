"""Timing of the baseline VQ-VAE's quantizer and training step at the CIFAR config (B 128, 8 x 8, C 128, K 512): the HIP
quantizer (vqvae_amd.baseline) against a torch restatement of the reference module's forward (float32 expansion GEMM, one-hot
EMA, the training loop's per-batch metrics with their .item() syncs), AMP on and off.  Device events, warm-up, medians over
alternating blocks in one process.  Writes the JSON to the path given (default vqvae_exp.json).

    python tools/exp_vqvae.py [out.json] [--epoch]
    python tools/exp_vqvae.py --trace      # 40 HIP training steps only, for a kernel trace of its own
"""
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vqvae_amd.baseline import VQVAE  # noqa: E402

B, C, HW, K = 128, 128, 8, 512
CFG = dict(in_channels=3, z_channels=C, hidden=256, n_res_blocks=2, n_codes=K, beta=0.25, ema_decay=0.99, ema_eps=1e-5)


class TorchVQ(torch.nn.Module):
    """The reference quantizer's forward restated in torch ops (for timing only)."""

    def __init__(self, q):
        super().__init__()
        self.q = q

    def forward(self, z_e):
        q = self.q
        Bz, Cz, H, W = z_e.shape
        flat = z_e.permute(0, 2, 3, 1).contiguous().view(-1, Cz).float()
        emb = q.embed.float()
        d = (flat ** 2).sum(1, keepdim=True) - 2 * flat @ emb.t() + (emb ** 2).sum(1)
        idx = torch.argmin(d, dim=1)
        z_q = q.embed.index_select(0, idx).view(Bz, H, W, Cz).permute(0, 3, 1, 2).contiguous()
        if q.training:
            with torch.no_grad():
                oh = torch.zeros(idx.size(0), q.n_codes, device=z_e.device)
                oh.scatter_(1, idx.view(-1, 1), 1)
                q.cluster_size.mul_(q.decay).add_(oh.sum(0), alpha=1 - q.decay)
                q.embed_avg.mul_(q.decay).add_((flat.t() @ oh).t(), alpha=1 - q.decay)
                n = q.cluster_size.sum()
                cs = ((q.cluster_size + q.eps) / (n + q.n_codes * q.eps) * n).unsqueeze(1).clamp_min(q.eps)
                q.embed.copy_(torch.nan_to_num(q.embed_avg / cs, nan=0.0, posinf=1.0, neginf=-1.0).clamp_(-2.0, 2.0))
        z_q_st = z_e + (z_q - z_e).detach()
        loss = q.beta * F.mse_loss(z_q_st.detach().float(), z_e.float())
        return z_q_st, loss, idx.view(Bz, H, W), z_q, z_e


def torch_metrics(idx, z_q, z_e):
    quant_mse = F.mse_loss(z_q.detach(), z_e.detach())
    hist = torch.bincount(idx.view(-1), minlength=K).float()
    usage = (hist > 0).float().mean()
    p = hist / hist.sum().clamp_min(1.0)
    perplex = torch.exp(-(p * (p + 1e-12).log()).sum())
    return [quant_mse.item(), perplex.item(), usage.item(), (1.0 - usage).item()]


def hip_metrics(q):
    return q.last_stats   # stays on the device


def time_blocks(fns, reps=20, blocks=7, warm=5):
    """Median per-call ms of each fn, alternating blocks of reps calls, device events around each block."""
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(blocks):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            b.record()
            b.synchronize()
            res[k].append(a.elapsed_time(b) / reps)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in res.items()}


def quantizer_fns():
    torch.manual_seed(0)
    q_hip = VQVAE(**CFG).quant.cuda().train()
    torch.manual_seed(0)
    q_t = TorchVQ(VQVAE(**CFG).quant.cuda().train())
    z32 = (torch.randn(B, C, HW, HW, device="cuda") * 1.5).requires_grad_()
    z16 = z32.detach().half().requires_grad_()
    g = torch.randn(B, C, HW, HW, device="cuda")

    def run(q, z, amp, metrics):
        def f():
            with torch.autocast("cuda", enabled=amp):
                z_q_st, loss, idx, z_q, z_e = q(z)
            metrics(idx, z_q, z_e) if metrics is torch_metrics else hip_metrics(q)
            torch.autograd.backward([z_q_st, loss], [g, torch.ones((), device="cuda")])
        return f
    return {"hip_f32": run(q_hip, z32, False, None), "torch_f32": run(q_t, z32, False, torch_metrics),
            "hip_f16_input": run(q_hip, z16, True, None), "torch_amp_f16_input": run(q_t, z16, True, torch_metrics)}


def make_step(use_hip, data):
    torch.manual_seed(0)
    model = VQVAE(**CFG).cuda().train()
    if not use_hip:
        model.quant = TorchVQ(model.quant)
    opt = torch.optim.Adam(model.parameters(), lr=2e-4)
    scaler = torch.amp.GradScaler(enabled=True)
    acc = torch.zeros(7, dtype=torch.float64, device="cuda")
    it = [0]

    def step():
        x = data[(it[0] % (len(data) // B)) * B:(it[0] % (len(data) // B) + 1) * B]
        it[0] += 1
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", enabled=True):
            x_rec, loss_vq, idx, z_q, z_e = model(x)
            loss_rec = F.l1_loss(x_rec, x)
            loss = loss_rec + loss_vq
        with torch.no_grad():
            flat = z_e.detach().permute(0, 2, 3, 1).contiguous().view(-1, C)
            _ = flat[torch.randperm(flat.size(0), device=flat.device)[:256]]
        if use_hip:
            stats = torch.cat([torch.stack([loss.detach().float(), loss_rec.detach().float(), loss_vq.detach().float()]),
                               model.quant.last_stats]).double()
        else:
            m = torch_metrics(idx, z_q, z_e)
        if not torch.isfinite(loss):
            return
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        scaler.step(opt)
        scaler.update()
        if use_hip:
            acc.add_(stats * B)
        else:
            _ = [loss.item(), loss_rec.item(), loss_vq.item()] + m
    return step


def main():
    if "--trace" in sys.argv:
        step = make_step(True, torch.rand(B * 20, 3, 32, 32, device="cuda") * 2 - 1)
        for _ in range(40):
            step()
        torch.cuda.synchronize()
        return
    out = next((a for a in sys.argv[1:] if not a.startswith("--")), "vqvae_exp.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "shape": {"B": B, "C": C, "HW": HW, "K": K}}
    res["quantizer_fwd_ema_bwd"] = time_blocks(quantizer_fns(), reps=50, blocks=9)
    print(json.dumps(res["quantizer_fwd_ema_bwd"], indent=1), flush=True)
    data = torch.rand(B * 20, 3, 32, 32, device="cuda") * 2 - 1
    steps = {"hip_step_amp": make_step(True, data), "torch_step_amp": make_step(False, data)}
    res["train_step_amp"] = time_blocks(steps, reps=10, blocks=7, warm=10)
    print(json.dumps(res["train_step_amp"], indent=1), flush=True)
    if "--epoch" in sys.argv:
        res["epoch_390_steps_s"] = {}
        for name in ("hip_step_amp", "torch_step_amp", "hip_step_amp_2", "torch_step_amp_2"):
            f = steps[name.replace("_2", "")]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(390):
                f()
            torch.cuda.synchronize()
            res["epoch_390_steps_s"][name] = time.perf_counter() - t0
        print(json.dumps(res["epoch_390_steps_s"], indent=1), flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
