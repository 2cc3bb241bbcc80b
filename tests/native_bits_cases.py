"""Shared by tools/gen_golden_native_bits.py, test_gpu_native_bits.py and test_native_bits_host.py: the cases whose output bits
tests/golden/native_bits.json pins for the native encode, decode, pull-back and LPIPS (the code that shares csrc/mfma_conv.h
and geo::plan_passes), built from the seeded builders of encode_cases, decode_cases, vanilla_jvp_cases and lpips_cases.

A configuration is one network; `run(area, name, dev)` returns {case id: {"input": sha, "outputs": {array: sha}}} for its sizes
of n, and `workspace_answers(area, name)` the *_workspace_bytes answers for WORKSPACE_N (no device needed).  "input" hashes what
the seeded builders produced (the module's state and the images, latents or edges); the packed export tensors are hashed as
an output ("packed"), so a change of the host-side packing shows as a changed output, not as another generator.

Sizes, by what they reach: n = 1 is less than one tile; 5 images are a partial group of the 2 and 4 items of an encoder
workgroup, 5 pairs (10 images) of the 4 and 7 of an LPIPS group, 6 latents of the 4 (8 x 8) and 5 (7 x 7) items of a mid
workgroup; 37 cut by a 16-item workspace is passes of 16, 16, 5 (a partial 16-item first-stage workgroup of the spatial
decode); 9 pairs cut by a 4-pair workspace is 4, 4, 1; the graph's edges cut by the one-edge workspace run one edge per pass."""
import hashlib

import torch

import decode_cases as DC
import encode_cases as EC
import lpips_cases as LC
import vanilla_jvp_cases as V

WORKSPACE_N = (0, 1, 16, 63, 64, 65, 4095, 4096, 4097, 100000)
ENC_WIDE, ENC_NARROW = (64, 128, 256), (32, 64, 128)
DEC_WIDE, DEC_NARROW = (256, 128, 64), (128, 64, 32)

# name -> (kind, enc_channels, latent_dim, in_channels, size, norm): both width triples x both input pairings x both heads
ENCODE = {f"{kind}-{tag}-{C}x{size}": (kind, ch, d, C, size, norm)
          for kind, ds in (("vanilla", (40, 5)), ("spatial", (16, 5)))
          for (tag, ch, norm), d in zip((("wide", ENC_WIDE, "batch"), ("narrow", ENC_NARROW, "none")), ds)
          for C, size in ((1, 28), (3, 32))}
# name -> (kind, dec_channels, latent_dim, out_channels, size, norm): both width pairs x 28 and 32 px x 1 and 3 channels
DECODE = {f"{kind}-{tag}-{C}x{size}": (kind, ch, d, C, size, norm)
          for kind, ds in (("vanilla", (33, 5)), ("spatial", (16, 7)))
          for (tag, ch, norm), d in zip((("wide", DEC_WIDE, "batch"), ("narrow", DEC_NARROW, "none")), ds)
          for C in (1, 3) for size in (28, 32)}
JVP = dict(V.CASES)
LPIPS = {"alex": None}
AREAS = {"encode": ENCODE, "decode": DECODE, "jvp": JVP, "lpips": LPIPS}
ALL = [(area, name) for area, table in AREAS.items() for name in table]


def sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _state(module):
    return [t for _, t in sorted(module.state_dict().items())]


def _packed(export):
    return sha(*[t for _, t in sorted(export.tensors.items())])


def _build(area, name, dev):
    """(module, export on `dev`) of a configuration."""
    if area == "encode":
        from vqvae_amd.image_encoder import ImageEncoderExport
        kind, ch, d, C, size, norm = ENCODE[name]
        m = EC.build(kind, ch, d, C, norm, seed=len(name))
        return m, ImageEncoderExport(m, dev)
    if area == "decode":
        from vqvae_amd.spatial_decoder import SpatialImageDecoderExport
        from vqvae_amd.vanilla_decoder import VanillaDecoderExport
        kind, ch, d, C, size, norm = DECODE[name]
        if kind == "vanilla":
            m = V.build(ch, d, C, size, norm, seed=len(name))
            return m, VanillaDecoderExport(m, dev)
        m = DC.build_spatial(ch, d, C, size, norm, seed=len(name))
        return m, SpatialImageDecoderExport(m, dev)
    if area == "jvp":
        from vqvae_amd.vanilla_decoder import VanillaDecoderExport
        ch, d, C, size, norm = JVP[name]
        m = V.build(ch, d, C, size, norm, seed=len(name))
        return m, VanillaDecoderExport(m, dev)
    from vqvae_amd.eval.lpips import LPIPSExport
    m = LC.model()
    return m, LPIPSExport(m, dev)


def workspace_answers(area, name) -> dict:
    """{query: [answer for n in WORKSPACE_N]}; the edges query takes (n_nodes, n_edges) = (n, 4 n) and (n, n)."""
    from vqvae_amd import _lib
    lib = _lib.load()
    _, ex = _build(area, name, torch.device("cpu"))
    if area == "encode":
        return {"geo_image_encode_workspace_bytes": [int(lib.geo_image_encode_workspace_bytes(ex.desc, n)) for n in WORKSPACE_N]}
    if area == "decode":
        q = "geo_spatial_decode_workspace_bytes" if DECODE[name][0] == "spatial" else "geo_vanilla_decode_workspace_bytes"
        return {q: [int(getattr(lib, q)(ex.desc, n)) for n in WORKSPACE_N]}
    if area == "jvp":
        edges = lib.geo_vanilla_jvp_edges_workspace_bytes
        return {"geo_vanilla_jvp_workspace_bytes": [int(lib.geo_vanilla_jvp_workspace_bytes(ex.desc, n)) for n in WORKSPACE_N],
                "geo_vanilla_jvp_edges_workspace_bytes(n, 4 n)": [int(edges(ex.desc, n, 4 * n)) for n in WORKSPACE_N],
                "geo_vanilla_jvp_edges_workspace_bytes(n, n)": [int(edges(ex.desc, n, n)) for n in WORKSPACE_N]}
    return {"geo_lpips_alex_workspace_bytes": [int(lib.geo_lpips_alex_workspace_bytes(n)) for n in WORKSPACE_N]}


def _sizes(ns, capped_n, cap_bytes):
    """[(tag, n, max_workspace_bytes)]: every n uncapped, then `capped_n` under the cap."""
    return [(f"n{n}", n, None) for n in ns] + [(f"n{capped_n}-capped", capped_n, cap_bytes)]


def run(area, name, dev) -> dict:
    from vqvae_amd import _lib
    lib = _lib.load()
    m, ex = _build(area, name, dev)
    out = {}

    def put(tag, inputs, arrays):
        out[f"{area}/{name}/{tag}"] = {"input": sha(*_state(m), *inputs),
                                       "outputs": dict({k: sha(v) for k, v in arrays.items()}, packed=_packed(ex))}

    if area == "encode":
        from vqvae_amd.encode import encode_latents
        _, _, _, C, size, _ = ENCODE[name]
        x = EC.images(37, C, size)
        for tag, n, cap in _sizes((1, 5, 37), 37, int(lib.geo_image_encode_workspace_bytes(ex.desc, 16))):
            mu, logvar = encode_latents(ex, x[:n].to(dev), max_workspace_bytes=cap)
            put(tag, [x[:n]], {"mu": mu, "logvar": logvar})
    elif area == "decode":
        from vqvae_amd.decode import decode_logits
        kind, _, d, _, _, _ = DECODE[name]
        spatial = kind == "spatial"
        query = lib.geo_spatial_decode_workspace_bytes if spatial else lib.geo_vanilla_decode_workspace_bytes
        z = DC.grids(37, d) if spatial else DC.vectors(37, d)
        table = DC.vectors(50, d, seed=2)
        codes = torch.randint(0, 50, (37, 4, 4) if spatial else (37,), generator=torch.Generator().manual_seed(3))
        for tag, n, cap in _sizes((1, 6, 37), 37, int(query(ex.desc, 16))):
            put(tag + "-z", [z[:n]], {"logits": decode_logits(ex, z[:n].to(dev), max_workspace_bytes=cap)})
            put(tag + "-codes", [table, codes[:n]],
                {"logits": decode_logits(ex, table=table.to(dev), codes=codes[:n].to(dev), max_workspace_bytes=cap)})
    elif area == "jvp":
        from vqvae_amd.geo.riemannian_metric import edge_lengths_vanilla_device, edge_lengths_vanilla_graph_device
        d = JVP[name][1]
        zs, ze = V.make_edges(d, n_edges=37)
        for n in (1, 3, 37):
            got = edge_lengths_vanilla_device(ex, zs[:n].to(dev).contiguous(), ze[:n].to(dev).contiguous())
            put(f"pairs-n{n}", [zs[:n], ze[:n]], {"len": got})
        z, src, dst = V.small_graph(d)                     # the capped run takes a tenth of its edges
        zd, sd, dd = z.to(dev), src.to(dev), dst.to(dev)
        put("edges", [z, src, dst], {"len": edge_lengths_vanilla_graph_device(ex, zd, sd, dd)})
        least = int(lib.geo_vanilla_jvp_workspace_bytes(ex.desc, 1))
        put("edges-150-capped", [z, src[:150], dst[:150]],
            {"len": edge_lengths_vanilla_graph_device(ex, zd, sd[:150].contiguous(), dd[:150].contiguous(), max_workspace_bytes=least)})
    else:
        from vqvae_amd.eval.lpips import lpips_pairs
        x0, x1 = LC.pairs("c3-64", n=9)
        for tag, n, cap in _sizes((1, 5), 9, int(lib.geo_lpips_alex_workspace_bytes(4))):
            a, b = x0[:n].to(dev), x1[:n].to(dev)
            put(tag, [x0[:n], x1[:n]], {"total": lpips_pairs(ex, a, b, max_workspace_bytes=cap),
                                        "layers": lpips_pairs(ex, a, b, per_layer=True, max_workspace_bytes=cap)})
    return out
