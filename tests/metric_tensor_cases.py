"""Decoders, latents and the fp64 reference shared by tests/test_metric_tensor_host.py and tests/test_gpu_metric_tensor.py.

The reference runs no kernel of the project: the SpatialDecoder module with oracle.metric.make_decoder_state weights in
fp64 eval mode on the CPU, J64 by torch.autograd.functional.jacobian of sigmoid(decoder(z.view(1, d, 1, 1))).reshape(-1),
G64 = J64^T J64.  It is computed once per (case, latent count) and handed out read-only."""
import functools

import numpy as np
import torch

DEFAULT_CHANNELS = (256, 128, 64)
# name: (norm, d, out_channels, px, dec_channels, seed); BatchNorm cases run in eval mode
CASES = {
    "fm_batch": ("batch", 16, 1, 28, DEFAULT_CHANNELS, 21),
    "fm_none5": ("none", 5, 1, 28, DEFAULT_CHANNELS, 22),
    "cf_batch": ("batch", 16, 3, 32, DEFAULT_CHANNELS, 23),      # p_out = 192: the strided output loop and the np padding
    "fm_group": ("group", 16, 1, 28, DEFAULT_CHANNELS, 24),
    "fm_batch1": ("batch", 1, 1, 28, DEFAULT_CHANNELS, 25),
    "fm_small": ("batch", 16, 1, 28, (32, 32, 16), 26),           # dec_channels[2] = 16: no per-latent column pass, autograd route
}
NATIVE = ("fm_batch", "fm_none5", "cf_batch", "fm_group", "fm_batch1")
WELL_CONDITIONED = ("fm_none5", "cf_batch", "fm_batch1")          # cond(G64) <= 1e3: the cases that gate logvol
N_LATENTS = 33                                                    # one full 32-sample tile plus one latent, an odd count


def make_decoder(name, training=False):
    """(float32 module on the CPU, state dict) of a case."""
    from oracle import metric as om
    from vqvae_amd.spatial_decoder import SpatialDecoder
    norm, d, cout, px, channels, seed = CASES[name]
    sd = om.make_decoder_state(seed, d, cout, channels=channels, norm_type=norm)
    dec = SpatialDecoder(cout, channels, d, px, norm)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return dec.train(training), sd


def make_latents(name, n, salt=0):
    d, seed = CASES[name][1], CASES[name][5]
    return np.random.RandomState(1000 + 7 * seed + salt).randn(n, d).astype(np.float32)


def gram64_of(dec, z):
    """G64 [n, d, d] (numpy fp64) of a module's fp64 copy at float32 latents z [n, d], by autograd on the CPU."""
    import copy
    dec64 = copy.deepcopy(dec).cpu().double().eval()
    first = next(dec64.children())
    flat = hasattr(first, "in_features")

    def image(latent):
        x = latent.view(1, -1) if flat else latent.view(1, -1, 1, 1)
        return torch.sigmoid(dec64(x)).reshape(-1)

    out = []
    for row in torch.from_numpy(np.asarray(z)).double():
        J = torch.autograd.functional.jacobian(image, row, vectorize=True)       # [p_out, d]
        out.append((J.t() @ J).numpy())
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def reference(name, n=N_LATENTS, salt=0):
    """(z float32 [n, d], G64 [n, d, d]) of a case, both read-only."""
    dec, _ = make_decoder(name)
    z = make_latents(name, n, salt)
    G64 = gram64_of(dec, z)
    z.setflags(write=False)
    G64.setflags(write=False)
    return z, G64


def normalised_error(G, G64):
    """max |G - G64| / sqrt(G64_aa G64_bb) over every latent and entry."""
    diag = np.sqrt(np.einsum("naa->na", G64))
    return float(np.max(np.abs(np.asarray(G) - G64) / (diag[:, :, None] * diag[:, None, :])))


def rank_rule(eig, p_out):
    """numpy's matrix_rank rule on the float32 Jacobian's singular values sqrt(eig): the count above
    max(p_out, d) * FLT_EPSILON * sqrt(eig_max)."""
    eig = np.asarray(eig, dtype=np.float64)
    d = eig.shape[-1]
    sv = np.sqrt(np.maximum(eig, 0.0))
    tol = float(max(p_out, d)) * float(np.finfo(np.float32).eps) * sv.max(axis=-1, keepdims=True)
    return np.sum((eig > 0) & (sv > tol), axis=-1).astype(np.int32)


def p_out_of(name):
    _, _, cout, px, _, _ = CASES[name]
    return cout * (16 if px == 28 else 64)
