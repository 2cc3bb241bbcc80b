"""Decoder descriptors and call sizes for the host-side JVP route tests (test_jvp_plan_host.py) -- no GPU, no weights: the
route and the workspace sizes depend on the descriptor's integers only."""
from vqvae_amd import _lib

# name: (latent_dim, (c0, c1, c2), out_channels, out_size, norm code [0 none, 1 batch, 2 group], bn_train, (groups1, groups2))
DECODERS = {
    "fm_bn_train": (16, (256, 128, 64), 1, 28, 1, 1, (0, 0)),
    "fm_bn_eval": (16, (256, 128, 64), 1, 28, 1, 0, (0, 0)),
    "fm_none": (16, (256, 128, 64), 1, 28, 0, 0, (0, 0)),
    "fm_group": (16, (256, 128, 64), 1, 28, 2, 0, (32, 32)),
    "cf32_bn_train": (32, (256, 128, 64), 3, 32, 1, 1, (0, 0)),
    "cf64_bn_train": (64, (256, 128, 64), 3, 32, 1, 1, (0, 0)),
    "cf32_bn_eval": (32, (256, 128, 64), 3, 32, 1, 0, (0, 0)),
    "cf32_group": (32, (256, 128, 64), 3, 32, 2, 0, (32, 32)),
    "c1_64_bn_train": (16, (256, 64, 64), 1, 28, 1, 1, (0, 0)),
    "c1_32_bn_train": (16, (256, 32, 64), 1, 28, 1, 1, (0, 0)),
    "c2_32_bn_train": (16, (256, 128, 32), 1, 28, 1, 1, (0, 0)),
    "c2_32_bn_eval": (16, (256, 128, 32), 1, 28, 1, 0, (0, 0)),
    "c2_128_bn_train": (16, (256, 128, 128), 1, 28, 1, 1, (0, 0)),
    "c2_128_3ch32": (16, (256, 128, 128), 3, 32, 1, 1, (0, 0)),          # back kernel's LDS budget: refused
    "small_bn_train": (16, (64, 32, 16), 1, 28, 1, 1, (0, 0)),
    "px32_1ch_bn_train": (16, (256, 128, 64), 1, 32, 1, 1, (0, 0)),       # 64 outputs: no matrix-core ConvT3
    "px32_1ch_bn_eval": (16, (256, 128, 64), 1, 32, 1, 0, (0, 0)),
    "px32_1ch_group": (16, (256, 128, 64), 1, 32, 2, 0, (32, 32)),        # GroupNorm needs the matrix-core ConvT3: refused
    "group_c2_32": (16, (256, 128, 32), 1, 28, 2, 0, (32, 32)),           # refused
    "group_16_groups": (16, (256, 128, 64), 1, 28, 2, 0, (16, 32)),       # refused
    "out_size_64": (16, (256, 128, 64), 1, 64, 1, 1, (0, 0)),             # refused, and no size
    "c1_48": (16, (256, 48, 64), 1, 28, 1, 0, (0, 0)),                    # refused by the run; the queries give a size
}

# (n_nodes, n_edges, batch_size): the pairs query / call ignores n_nodes
SIZES = {"small": (3000, 2048, 512), "ragged": (777, 5001, 100), "dense": (3000, 40000, 512), "sparse": (3000, 9000, 512),
         "few_edges": (5000, 100, 512), "c2": (60000, 946059, 512)}


def descriptor(name):
    d, (c0, c1, c2), cout, size, norm, bn_train, (g1, g2) = DECODERS[name]
    return _lib.DecoderDesc(latent_dim=d, c0=c0, c1=c1, c2=c2, out_channels=cout, out_size=size, norm=norm, bn_train=bn_train,
                            groups1=g1, groups2=g2, eps=1e-5, update_running=1, momentum=0.1)


def workspace_sizes(lib):
    """{"decoder/size": [geo_jvp_workspace_bytes, geo_jvp_edges_workspace_bytes]} for every decoder and size."""
    out = {}
    for dn in DECODERS:
        desc = descriptor(dn)
        for sn, (n_nodes, n_edges, bs) in SIZES.items():
            out[f"{dn}/{sn}"] = [int(lib.geo_jvp_workspace_bytes(desc, n_edges, bs)),
                                 int(lib.geo_jvp_edges_workspace_bytes(desc, n_nodes, n_edges, bs))]
    return out
