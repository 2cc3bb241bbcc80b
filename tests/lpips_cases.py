"""Shared by test_lpips_host.py and test_gpu_lpips.py: the seeded LPIPS network (no real AlexNet weights exist here; the
shapes are the real ones), the image pairs of the accuracy test, state dicts in the two key layouts the loader accepts, and
the fp64 / float32 CPU references (computed once per case, read-only).

Initialisation: convolution weights kaiming_normal_, biases N(0, 0.1), lin weights U(0, 2 / C).  With it the feature norms of
the pairs below stay well away from zero in every layer, so no normalisation is near its singular point."""
import copy
import functools

import torch

CASES = {"c1-28": (1, 28), "c3-32": (3, 32), "c3-64": (3, 64)}          # name -> (channels, size); 64 goes in directly
ALL_CASES = list(CASES)
N_PAIRS = 130        # 260 images: a multiple of the 4 images of a layer-2 workgroup, not of the 7 of layers 3 to 5; the
#                      sub-batches of 1 and 5 pairs (2 and 10 images) are ragged for both


def make_model(seed=0):
    """LPIPSAlex (float32, CPU, eval) with the seeded initialisation of the module docstring."""
    from vqvae_amd.eval.lpips import LPIPSAlex
    model = LPIPSAlex()
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        with torch.no_grad():
            for conv in model.convs:
                torch.nn.init.kaiming_normal_(conv.weight)
                conv.bias.normal_(0.0, 0.1)
            for lin in model.lins:
                lin.uniform_(0.0, 2.0 / lin.numel())
    return model.eval()


def dead_layer5(model):
    """A copy whose conv5 biases are -1e3: every f5 is zero."""
    dead = copy.deepcopy(model)
    with torch.no_grad():
        dead.convs[4].bias.fill_(-1e3)
    return dead


def state_dict_for_file(model, layout="lpips", with_extras=True) -> dict:
    """The module's weights under the lpips package's key names ("lpips") or torchvision's backbone names ("torchvision"),
    with the `lins.*` duplicates and the scaling layer's constants the package also writes."""
    from vqvae_amd.eval import lpips as L
    names = L._LPIPS_CONV_KEYS if layout == "lpips" else L._TORCHVISION_CONV_KEYS
    sd = {}
    for conv, name in zip(model.convs, names):
        sd[name + ".weight"] = conv.weight.detach().clone()
        sd[name + ".bias"] = conv.bias.detach().clone()
    for l, lin in enumerate(model.lins):
        sd[f"lin{l}.model.1.weight"] = lin.detach().clone().view(1, -1, 1, 1)
        if with_extras:
            sd[f"lins.{l}.model.1.weight"] = lin.detach().clone().view(1, -1, 1, 1)
    if with_extras:
        sd["scaling_layer.shift"] = torch.tensor(L.SHIFT).view(1, 3, 1, 1)
        sd["scaling_layer.scale"] = torch.tensor(L.SCALE).view(1, 3, 1, 1)
    return sd


def raw_pairs(n, channels, size, seed=1):
    """(a, b) in [0, 1]: the first half of b is a noisy copy of a (sigma 0.2, clamped), the second half unrelated images, so
    that the deep layers carry weight too."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand((n, channels, size, size), generator=g)
    b = torch.rand((n, channels, size, size), generator=g)
    noisy = (a + 0.2 * torch.randn(a.shape, generator=g)).clamp(0.0, 1.0)
    half = (n + 1) // 2
    b[:half] = noisy[:half]
    return a, b


def pairs(name, n=N_PAIRS):
    """(x0, x1) f32 [n, 3, 64, 64] in [-1, 1] of a case: through preprocess_for_lpips, or directly for 64 px."""
    from vqvae_amd.eval.lpips import preprocess_for_lpips
    channels, size = CASES[name]
    a, b = raw_pairs(n, channels, size, seed=len(name) + size)
    if size == 64:
        return (a * 2 - 1).contiguous(), (b * 2 - 1).contiguous()
    return preprocess_for_lpips(a).contiguous(), preprocess_for_lpips(b).contiguous()


@functools.lru_cache(maxsize=None)
def model():
    return make_model(0)


@functools.lru_cache(maxsize=None)
def case(name):
    """(x0, x1, fp64 values [n, 6], float32-torch maximum error per column [6]): columns 0 .. 4 are the layers, 5 the total."""
    x0, x1 = pairs(name)
    m = model()
    with torch.no_grad():
        m64 = copy.deepcopy(m).double()
        v64 = torch.cat([m64(x0, x1, per_layer=True), m64(x0, x1).view(-1, 1)], dim=1)
        v32 = torch.cat([m(x0, x1, per_layer=True), m(x0, x1).view(-1, 1)], dim=1)
    err32 = (v32.double() - v64).abs().max(dim=0).values
    return x0, x1, v64, err32
