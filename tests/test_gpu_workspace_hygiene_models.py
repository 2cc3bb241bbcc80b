"""The model-side half of tests/test_gpu_workspace_hygiene.py: the entry points that cut their items into passes of a capped
workspace (image encode, both image decodes, LPIPS, the vanilla pull-back, the metric tensor, all through
_export.capped_workspace -> _device.workspace) and those that allocate their scratch per call behind a module-level
`_workspace` (k-means assign / seeding / Lloyd, the EMA quantizer, the ELBO, the prior's decode; ws_guard.SEAMS).

Same four runs per case (P production, Z zeros, O ones, S stale after a call on other data of the same shapes), every
documented output of Z, O and S equal to P's bit for bit, intact guards.  The library reports no route for these calls, so a
case passes a fixed label and instead asserts, by host arithmetic on the size queries alone, that the pass or slice structure
it names is the one the call takes: geo::plan_passes and vanilla_jvp.hip's `run` shrink a pass one item at a time (below 64
items) until its buffers fit, so a cap of query(k) with query(k) < query(k + 1) gives passes of exactly k items and a last one
of n mod k.  After the four runs P's outputs must be finite and not all zero; accuracy is tested elsewhere.

The last section calls five of the per-call entry points once each with a workspace one byte below the query: a refusal
before any launch, with the status DESIGN.md section 1 ("Workspaces") records for each (geo_prior_sample's is in
test_gpu_prior_envelope.py)."""
import ctypes

import numpy as np
import pytest
import torch

import decode_cases as D
import encode_cases as E
import lpips_cases as LC
import metric_tensor_cases as M
import prior_cases as PC
import vanilla_jvp_cases as V
from test_gpu_workspace_hygiene import _dev, _t
from ws_guard import GuardedWorkspace
from ws_guard import four_runs as _four_runs

pytestmark = pytest.mark.gpu

GEO_E_ARG, GEO_E_WORKSPACE = -1, -2


# ------------------------------------------------------------------------------------------------------------------ helpers
def _lib():
    from vqvae_amd import _lib as L
    return L.load()


def _cap(query, n, k):
    """max_workspace_bytes for passes of exactly k of the n items (None: no cap, one pass at exactly query(n)), after asserting
    on the query alone that this is what the library's shrink loop arrives at.  -> (cap, pass sizes)."""
    assert 1 <= n <= 64                                  # the shrink loop steps by one item below 64, and no pass limit is near
    if k is None:
        assert 0 < query(n - 1) < query(n)               # a pass of n items fits at query(n) and at nothing a smaller n asks for
        return None, [n]
    assert 1 <= k < n and 0 < query(k) < query(k + 1) <= query(n)
    return int(query(k)), [k] * (n // k) + ([n % k] if n % k else [])


def _live(out, *names):
    for name in names:
        t = out[name]
        t = t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))
        assert bool(torch.isfinite(t.double()).all()), name
        assert bool((t != 0).any()), name


def _g(seed):
    return torch.Generator().manual_seed(seed)


PASSES = [pytest.param(None, id="one_pass"), pytest.param(5, id="passes_of_5"), pytest.param(1, id="passes_of_1")]


# ------------------------------------------------------------------------------------------------------------ image encode
# Layers 2 and 3 take 1 or 2 and 2 or 4 items per workgroup, the head 32 rows: 11 items, and passes of 5, 5, 1 and of 1.
ENCODERS = [("vanilla", "narrow-none-28"), ("spatial", "wide-bn-32x3-d32")]        # 1x28x28 (32, 64, 128), 3x32x32 (64, 128, 256)


@pytest.mark.parametrize("k", PASSES)
@pytest.mark.parametrize("kind,name", ENCODERS)
def test_image_encode(kind, name, k, monkeypatch):
    from vqvae_amd.encode import encode_latents
    from vqvae_amd.image_encoder import ImageEncoderExport
    channels, d, C, size, norm = E.CASES[(kind, name)]
    export = ImageEncoderExport(E.build(kind, channels, d, C, norm, seed=len(name)), _dev())
    lib, n = _lib(), 11
    cap, passes = _cap(lambda m: lib.geo_image_encode_workspace_bytes(export.desc, m), n, k)
    assert passes == {None: [11], 5: [5, 5, 1], 1: [1] * 11}[k]

    def call(x):
        mu, logvar = encode_latents(export, x, max_workspace_bytes=cap)
        return {"mu": mu, "logvar": logvar}, "hip"

    out = _four_runs(monkeypatch, call, E.images(n, C, size, seed=2).to(_dev()), E.images(n, C, size, seed=1).to(_dev()), "hip")
    assert out["mu"].shape == ((n, d, 4, 4) if kind == "spatial" else (n, d))
    _live(out, "mu", "logvar")


# ---------------------------------------------------------------------------------------------------------- vanilla decode
# vj_mid_kernel takes 5 items at 7x7 (28 px) and 4 at 8x8 (32 px): 13 items, and passes of 6, 6, 1 and of 1.
@pytest.mark.parametrize("gather", [False, True], ids=["latents", "table_and_codes"])
@pytest.mark.parametrize("k", [pytest.param(None, id="one_pass"), pytest.param(6, id="passes_of_6"), pytest.param(1, id="passes_of_1")])
@pytest.mark.parametrize("name", ["wide-bn-28", "narrow-none-32x3-d5"])
def test_vanilla_decode(name, k, gather, monkeypatch):
    from vqvae_amd.decode import decode_logits
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    channels, d, C, size, norm = V.CASES[name]
    export = VanillaDecoderExport(V.build(channels, d, C, size, norm, seed=len(name)), _dev())
    lib, n = _lib(), 13
    cap, passes = _cap(lambda m: lib.geo_vanilla_decode_workspace_bytes(export.desc, m), n, k)
    assert passes == {None: [13], 6: [6, 6, 1], 1: [1] * 13}[k]

    def inputs(seed):
        if not gather:
            return (D.vectors(n, d, seed=seed).to(_dev()),)
        return D.vectors(9, d, seed=seed).to(_dev()), torch.randint(0, 9, (n,), generator=_g(seed), dtype=torch.int32).to(_dev())

    def call(inp):
        if gather:
            return {"logits": decode_logits(export, table=inp[0], codes=inp[1], max_workspace_bytes=cap)}, "hip"
        return {"logits": decode_logits(export, inp[0], max_workspace_bytes=cap)}, "hip"

    out = _four_runs(monkeypatch, call, inputs(2), inputs(1), "hip")
    assert out["logits"].shape == (n, C, size, size)
    _live(out, "logits")


# ---------------------------------------------------------------------------------------------------------- spatial decode
# sd_front_kernel takes 16 items: 17 uncapped is one past a full workgroup; 11 in passes of 5, 5, 1 and of 1.
@pytest.mark.parametrize("codes", [False, True], ids=["grids", "table_and_codes"])
@pytest.mark.parametrize("n,k", [(17, None), (11, 5), (11, 1)], ids=["17_one_pass", "11_passes_of_5", "11_passes_of_1"])
@pytest.mark.parametrize("name", ["wide-bn-32x3-d32", "narrow-none-28-d5"])          # (c1, c2) = (128, 64) and (64, 32)
def test_spatial_decode(name, n, k, codes, monkeypatch):
    from vqvae_amd.decode import decode_logits
    from vqvae_amd.spatial_decoder import SpatialImageDecoderExport
    channels, d, C, size, norm = D.SPATIAL_CASES[name]
    export = SpatialImageDecoderExport(D.build_spatial(channels, d, C, size, norm, seed=len(name)), _dev())
    lib = _lib()
    cap, passes = _cap(lambda m: lib.geo_spatial_decode_workspace_bytes(export.desc, m), n, k)
    assert passes == {(17, None): [17], (11, 5): [5, 5, 1], (11, 1): [1] * 11}[(n, k)]

    def inputs(seed):
        if not codes:
            return (D.grids(n, d, seed=seed).to(_dev()),)
        return D.vectors(9, d, seed=seed).to(_dev()), torch.randint(0, 9, (n, 4, 4), generator=_g(seed), dtype=torch.int32).to(_dev())

    def call(inp):
        if codes:
            return {"logits": decode_logits(export, table=inp[0], codes=inp[1], max_workspace_bytes=cap)}, "hip"
        return {"logits": decode_logits(export, inp[0], max_workspace_bytes=cap)}, "hip"

    out = _four_runs(monkeypatch, call, inputs(2), inputs(1), "hip")
    assert out["logits"].shape == (n, C, size, size)
    _live(out, "logits")


# ------------------------------------------------------------------------------------------------------------------- LPIPS
# The convolutions take groups of 4 and of 7 images: 11 pairs are 22 images; passes of 5 pairs are 10, 10 and 2 images.
_lpips_export = {}


def _lpips():
    from vqvae_amd.eval.lpips import LPIPSExport
    if "e" not in _lpips_export:
        _lpips_export["e"] = LPIPSExport(LC.model(), _dev())
    return _lpips_export["e"]


@pytest.mark.parametrize("per_layer", [False, True], ids=["total", "per_layer"])
@pytest.mark.parametrize("k", PASSES)
@pytest.mark.parametrize("name", ["c3-64", "c1-28"], ids=["enters_at_64", "resized_from_28"])
def test_lpips(name, k, per_layer, monkeypatch):
    from vqvae_amd.eval.lpips import last_lpips_path, lpips_pairs
    lib, n = _lib(), 11
    cap, passes = _cap(lambda m: lib.geo_lpips_alex_workspace_bytes(m), n, k)
    assert passes == {None: [11], 5: [5, 5, 1], 1: [1] * 11}[k]

    def inputs(seed):
        channels, size = LC.CASES[name]
        a, b = LC.raw_pairs(n, channels, size, seed=seed)
        if size == 64:
            return (a * 2 - 1).contiguous().to(_dev()), (b * 2 - 1).contiguous().to(_dev())
        from vqvae_amd.eval.lpips import preprocess_for_lpips
        return preprocess_for_lpips(a).contiguous().to(_dev()), preprocess_for_lpips(b).contiguous().to(_dev())

    def call(inp):
        out = lpips_pairs(_lpips(), inp[0], inp[1], per_layer=per_layer, max_workspace_bytes=cap)
        return {"lpips": out}, last_lpips_path()

    out = _four_runs(monkeypatch, call, inputs(4), inputs(3), "hip")
    assert out["lpips"].shape == ((n, 5) if per_layer else (n,)) and bool((out["lpips"] > 0).all())
    _live(out, "lpips")


# ------------------------------------------------------------------------------------------------------- vanilla pull-back
# vj_front_kernel takes 64 rows, vj_mid_kernel 5 (7x7) or 4 (8x8) items, two per edge in the tangent pass.
PULLBACK_DECODERS = ["wide-bn-28", "narrow-none-32x3-d5"]


def _vanilla_export(name):
    from vqvae_amd.vanilla_decoder import VanillaDecoderExport
    channels, d, C, size, norm = V.CASES[name]
    return VanillaDecoderExport(V.build(channels, d, C, size, norm, seed=len(name)), _dev()), d


@pytest.mark.parametrize("k", PASSES)
@pytest.mark.parametrize("name", PULLBACK_DECODERS)
def test_vanilla_jvp_pairs(name, k, monkeypatch):
    from vqvae_amd.geo.riemannian_metric import edge_lengths_vanilla_device
    export, d = _vanilla_export(name)
    lib, n_edges = _lib(), 11
    cap, passes = _cap(lambda m: lib.geo_vanilla_jvp_workspace_bytes(export.desc, m), n_edges, k)
    assert passes == {None: [11], 5: [5, 5, 1], 1: [1] * 11}[k]

    def inputs(seed):
        zs, ze = V.make_edges(d, n_edges=n_edges, seed=seed)
        return zs.to(_dev()).contiguous(), ze.to(_dev()).contiguous()

    def call(inp):
        return {"lengths": edge_lengths_vanilla_device(export, inp[0], inp[1], max_workspace_bytes=cap)}, "pairs"

    out = _four_runs(monkeypatch, call, inputs(2), inputs(1), "pairs")
    assert out["lengths"].shape == (n_edges,) and bool((out["lengths"] > 0).all())
    _live(out, "lengths")


@pytest.mark.parametrize("resident", [True, False], ids=["once_per_latent", "once_per_edge_end"])
@pytest.mark.parametrize("name", PULLBACK_DECODERS)
def test_vanilla_jvp_graph(name, resident, monkeypatch):
    """7 latents, 11 edges.  With the queried workspace n_nodes <= 2 n_edges and everything fits: the point pass runs once per
    latent.  Capped at geo_vanilla_jvp_workspace_bytes(desc, 1) the resident layout does not fit and every pass is one edge with
    a point pass over its own two ends."""
    from vqvae_amd.geo.riemannian_metric import edge_lengths_vanilla_graph_device
    export, d = _vanilla_export(name)
    lib, N, n_edges = _lib(), 7, 11

    def edges_query(n_nodes, m):
        return lib.geo_vanilla_jvp_edges_workspace_bytes(export.desc, n_nodes, m)

    def pairs_query(m):
        return lib.geo_vanilla_jvp_workspace_bytes(export.desc, m)

    assert N <= 2 * n_edges
    # the layout is (masks and images of `slots` points) + (two activation buffers of `eb` edges), each term aligned on its own:
    # edges_query(s, m) = points(s) + edges(m) for s <= 2 m, pairs_query(m) = points(2 m) + edges(m)
    assert edges_query(2 * n_edges, n_edges) == pairs_query(n_edges) and edges_query(8, 4) == pairs_query(4)
    if resident:
        cap = None
        assert edges_query(N, n_edges) < pairs_query(n_edges)                   # 7 point slots, not 22: the resident layout
    else:
        cap = int(pairs_query(1))
        resident_least = pairs_query(1) + edges_query(N, 4) - edges_query(2, 4)         # points(7) + edges(1)
        assert resident_least > cap                                             # so the call leaves the resident route,
        assert pairs_query(1) < pairs_query(2)                                  # and passes of two edges do not fit either

    def inputs(seed):
        g = _g(seed)
        z = torch.randn(N, d, generator=g)
        src = (torch.arange(n_edges, dtype=torch.int32) % N)[torch.randperm(n_edges, generator=g)]     # every latent has an edge
        dst = (src + 1 + torch.randint(0, N - 1, (n_edges,), generator=g, dtype=torch.int32)) % N      # never a self loop
        assert len(set(src.tolist()) | set(dst.tolist())) == N
        return z.to(_dev()), src.to(_dev()), dst.to(_dev())

    def call(inp):
        return {"lengths": edge_lengths_vanilla_graph_device(export, inp[0], inp[1], inp[2], max_workspace_bytes=cap)}, "graph"

    out = _four_runs(monkeypatch, call, inputs(2), inputs(1), "graph")
    assert out["lengths"].shape == (n_edges,) and bool((out["lengths"] > 0).all())
    _live(out, "lengths")


# ----------------------------------------------------------------------------------------------------------- metric tensor
@pytest.mark.parametrize("n,least", [(33, False), (65, True)], ids=["33_one_slice", "65_slices_32_32_1"])
@pytest.mark.parametrize("name", ["fm_batch", "cf_batch", "fm_group"])
def test_metric_tensor(name, n, least, monkeypatch):
    """33 latents are one past a 32-sample tile.  At geo_metric_tensor_min_workspace_bytes -- the bytes of one tile, less than
    two tiles take -- 65 latents run as slices of 32, 32 and 1."""
    from vqvae_amd.geo import pullback_metric_device
    from vqvae_amd.spatial_decoder import DecoderExport
    export = DecoderExport(M.make_decoder(name)[0].to(_dev()), _dev())
    lib = _lib()

    def query(m):
        return lib.geo_metric_tensor_workspace_bytes(export.desc, m)

    cap = None
    if least:
        cap = int(lib.geo_metric_tensor_min_workspace_bytes(export.desc))
        assert 0 < cap == query(32) < query(64) <= query(n) and n // 32 == 2 and n % 32 == 1
    else:
        assert 0 < query(32) < query(n)

    def call(z):
        res = pullback_metric_device(export, z, spectrum=True, max_workspace_bytes=cap)
        return {"G": res.G, "eig": res.eig, "logvol": res.logvol, "rank": res.rank}, res.route

    out = _four_runs(monkeypatch, call, _t(M.make_latents(name, n, salt=1)), _t(M.make_latents(name, n)), "native")
    d = M.CASES[name][1]
    assert out["G"].shape == (n, d, d) and out["eig"].shape == (n, d)
    _live(out, "G", "eig", "rank")
    assert not bool(torch.isnan(out["logvol"]).any()) and bool((out["logvol"] != 0).any())       # (-inf: a singular G)


# ----------------------------------------------------------------------------------------------------------------- k-means
def test_kmeans_assign(monkeypatch):
    """One row past a 128-row workgroup, ns_for(17) = 16, a second centre tile with one centre in it."""
    from vqvae_amd import cluster
    n, d, K = 129, 17, 33

    def inputs(seed):
        r = np.random.RandomState(seed)
        return _t((r.randn(n, d) * 3).astype(np.float32)), _t((r.randn(K, d) * 3).astype(np.float32))

    def call(inp):
        labels, keys, n_fallback = cluster.assign(inp[0], inp[1])
        return {"labels": labels, "keys": keys, "n_fallback": n_fallback}, "assign"

    out = _four_runs(monkeypatch, call, inputs(2), inputs(1), "assign")
    assert out["labels"].shape == (n,) and int(out["labels"].min()) >= 0 and int(out["labels"].max()) < K
    _live(out, "labels", "keys")


def test_kmeans_seeding(monkeypatch):
    """Two 1024-row segments, the second of one row; two starts, three local trials."""
    from vqvae_amd import cluster
    n, d, K, S, L = 1025, 3, 5, 2, 3

    def inputs(seed):
        r = np.random.RandomState(seed)
        X = (r.randn(n, d) * 3).astype(np.float32)
        first, u = cluster.seeding_draws(np.random.RandomState(seed + 10), n, K, S, L)
        first[1] = n - 1                                                         # the lone row of the second segment
        return _t(X), first, u

    def call(inp):
        centers, idx = cluster.plusplus_device(inp[0], K, inp[1], inp[2])
        return {"centers": centers, "indices": idx}, "seeding"

    B = inputs(1)
    out = _four_runs(monkeypatch, call, inputs(2), B, "seeding")
    idx = out["indices"].cpu().numpy()
    assert idx.shape == (S, K) and idx.min() >= 0 and idx.max() < n and all(len(set(row)) == K for row in idx.tolist())
    assert np.array_equal(idx[:, 0], B[1]) and torch.equal(out["centers"], B[0][out["indices"].long()])
    _live(out, "centers", "indices")


def test_kmeans_lloyd(monkeypatch):
    """Two starts; each starts with a centre far from every row, which is empty after the first assignment: the relocation
    kernel gives it the row farthest from its centre."""
    from vqvae_amd import cluster
    n, d, K, S = 1025, 17, 33, 2
    far = K - 1

    def inputs(seed):
        r = np.random.RandomState(seed)
        X = (r.randn(8, d)[r.randint(0, 8, n)] * 4 + r.randn(n, d)).astype(np.float32)            # eight blobs
        init = np.stack([X[r.choice(n, K, replace=False)] for _ in range(S)])
        init[:, far] = 1000.0
        return _t(X), _t(init)

    def call(inp):
        res = cluster.lloyd_device(inp[0], inp[1], 30, 0.0)
        return res, "lloyd"

    out = _four_runs(monkeypatch, call, inputs(2), inputs(1), "lloyd")
    assert out["labels"].shape == (S, n) and out["centers"].shape == (S, K, d)
    assert (out["n_iter"] >= 2).all(), out["n_iter"]
    for s in range(S):          # relocation happened: the far centre's cluster is populated and the centre came to the data
        assert bool((out["labels"][s] == far).any()) and float(out["centers"][s, far].abs().max()) < 100.0
    _live(out, "centers", "labels", "inertia", "n_iter")


# ------------------------------------------------------------------------------------------------------------ VQ forward
def _vq_inputs(case, seed):
    """(z_e, embed, cluster_size, embed_avg) on the device, built on the CPU from one seeded generator."""
    g = _g(seed)
    if case == "f32_train_ragged_tiles":             # HW = 35 and C = 33: two transpose tiles each, n = 105: two 64-position tiles
        K, z, dtype = 33, torch.randn(3, 33, 5, 7, generator=g), torch.float32
    elif case == "f16_eval_more_codes_than_rows":
        K, z, dtype = 4096, torch.randn(1, 32, 2, 3, generator=g) * 1.5, torch.float16
    else:                                            # test_training_step_skewed_cifar_shape's planting at n = 128 rows
        K, z, dtype = 512, torch.randn(2, 128, 8, 8, generator=g) * 0.05, torch.float32
    C = z.shape[1]
    embed = torch.randn(K, C, generator=g)
    if case == "f32_train_skewed":
        embed[5] = 0.0                               # nearly every row is next to code 5: its run spans both 64-position tiles
        pick = torch.randint(0, K, (8,), generator=g)
        z[0, :, 0, :] = (embed[pick] + 0.3 * torch.randn(8, C, generator=g)).t()
    cluster_size = torch.rand(K, generator=g) * 20
    embed_avg = embed * cluster_size[:, None]
    return tuple(t.to(_dev()) for t in (z.to(dtype), embed, cluster_size, embed_avg))


@pytest.mark.parametrize("case,training", [("f32_train_ragged_tiles", True), ("f16_eval_more_codes_than_rows", False),
                                           ("f32_train_skewed", True)])
def test_vq_forward(case, training, monkeypatch):
    from vqvae_amd.baseline import VectorQuantizerEMA

    def call(inp):
        z, embed, cluster_size, embed_avg = inp
        q = VectorQuantizerEMA(n_codes=embed.shape[0], code_dim=embed.shape[1]).to(_dev())       # a fresh one: training mutates it
        q.embed.copy_(embed), q.cluster_size.copy_(cluster_size), q.embed_avg.copy_(embed_avg)
        q.train(training)
        z_q_st, loss, idx, z_q, _ = q(z)
        out = {"z_q_st": z_q_st, "loss": loss, "idx": idx, "z_q": z_q, "last_stats": q.last_stats}
        if training:
            out.update(embed=q.embed.clone(), cluster_size=q.cluster_size.clone(), embed_avg=q.embed_avg.clone())
        return out, "hip"

    B = _vq_inputs(case, 1)
    out = _four_runs(monkeypatch, call, _vq_inputs(case, 2), B, "hip")
    K, n = B[1].shape[0], B[0].numel() // B[0].shape[1]
    counts = torch.bincount(out["idx"].reshape(-1), minlength=K)
    assert int(counts.sum()) == n
    if case == "f32_train_skewed":
        assert int(counts[5]) >= 115 and int((counts > 0).sum()) >= 3
        first, last = (out["idx"].reshape(-1) == 5).nonzero()[[0, -1], 0].tolist()
        assert first < 64 <= last
    if training:
        assert not torch.equal(out["embed"], B[1]) and not torch.equal(out["cluster_size"], B[2])
        _live(out, "embed", "cluster_size", "embed_avg")
    _live(out, "z_q_st", "loss", "z_q", "last_stats")


# -------------------------------------------------------------------------------------------------------------------- ELBO
# (B, P, d, recon mode, free bits, capacity mode): B P = 2355 is no multiple of 4 (the scalar route), 3136 is (float4)
ELBO_CASES = {
    "scalar_bce_free_bits_abs": (3, 785, 5, "bce", 0.5, "abs"),
    "scalar_mse_logits_clipped": (3, 785, 5, "mse_logits", None, "clipped"),
    "float4_mse_sigmoid_off": (4, 784, 16, "mse_sigmoid", 0.25, "off"),
}


@pytest.mark.parametrize("name", list(ELBO_CASES))
def test_elbo(name, monkeypatch):
    from vqvae_amd import vae
    B, P, d, recon, free_bits, capacity = ELBO_CASES[name]
    assert (B * P % 4 == 0) == name.startswith("float4")

    def inputs(seed):
        g = _g(seed)
        return tuple(t.to(_dev()) for t in (torch.randn(B, P, generator=g) * 2, torch.rand(B, P, generator=g),
                                            torch.randn(B, d, generator=g), torch.randn(B, d, generator=g) * 0.5))

    def call(inp):
        logits, x, mu, logvar = (t.clone() for t in inp)
        for t in (logits, mu, logvar):
            t.requires_grad_(True)
        out = vae.elbo_hip(logits, x, mu, logvar, vae.RECON_MODES[recon], free_bits, 0.7, 0.5, vae.CAPACITY_MODES[capacity])
        out[0].backward()
        return {"out": out.detach(), "d_logits": logits.grad, "d_mu": mu.grad, "d_logvar": logvar.grad}, "hip"

    out = _four_runs(monkeypatch, call, inputs(2), inputs(1), "hip")
    assert out["out"].shape == (4,) and out["out"].dtype == torch.float64
    _live(out, "out", "d_logits", "d_mu", "d_logvar")


# ------------------------------------------------------------------------------------------------------------ prior sample
# (DECODE_SHAPES model, top_k, labelled): 100 tokens are no multiple of 64; 192 / 3 and 448 / 7 are head dimension 64
PRIOR_CASES = {
    "v100_no_top_k": ("c320_h10_v100", None, False),
    "v100_top_k_7": ("c320_h10_v100", 7, False),
    "head_dim_64_v1024_top_k_50": ("c192_h3_v1024", 50, False),
    "head_dim_64_labelled_no_top_k": ("c448_h7_v2", None, True),
}


@pytest.mark.parametrize("name", list(PRIOR_CASES))
def test_prior_sample(name, monkeypatch):
    """17 rows are one past a 16-row linear tile; a prompt of one token and as many steps as the model has positions."""
    from vqvae_amd.prior.sampling import kernel_covers, sample_native
    shape, top_k, labelled = PRIOR_CASES[name]
    cfg = PC.DECODE_SHAPES[shape]
    assert (cfg["num_classes"] > 0) == labelled
    model = PC.seeded_model(cfg, 7, _dev())
    assert kernel_covers(model)
    rows, V_, steps = 17, cfg["num_tokens"], cfg["max_seq_len"]

    def inputs(seed):
        g = _g(seed)
        x = torch.randint(0, V_, (rows, 1), generator=g)
        u = torch.rand(rows, steps, generator=g)
        y = torch.randint(0, cfg["num_classes"], (rows,), generator=g) if labelled else None
        return x.to(_dev()), u.to(_dev()), None if y is None else y.to(_dev())

    def call(inp):
        tokens, logits = sample_native(model, inp[0], steps, 0.9, top_k, inp[2], inp[1], return_logits=True)
        return {"tokens": tokens, "logits": logits}, "hip"

    B = inputs(1)
    out = _four_runs(monkeypatch, call, inputs(2), B, "hip")
    assert out["tokens"].shape == (rows, 1 + steps) and out["logits"].shape == (rows, steps, V_)
    assert torch.equal(out["tokens"][:, :1], B[0]) and int(out["tokens"].min()) >= 0 and int(out["tokens"].max()) < V_
    _live(out, "tokens", "logits")


# --------------------------------------------------------------------------------------------------------------- refusals
SENTINEL = -7


def _refused(status, want, who, outputs, guard):
    """The call returned `want`, named itself in geo_last_error, wrote no output and left the guards alone."""
    lib = _lib()
    assert status == want, (status, lib.geo_last_error())
    text = lib.geo_last_error().decode()
    assert who in text and "workspace" in text, text
    torch.cuda.synchronize()
    for name, t in outputs.items():
        t = t if isinstance(t, torch.Tensor) else torch.from_numpy(t)
        assert bool((t == SENTINEL).all()), f"{who}: '{name}' was written"
    guard.check()


def _sentinels(dev, **shapes):
    return {name: torch.full(shape, SENTINEL, dtype=dtype, device=dev) for name, (shape, dtype) in shapes.items()}


def test_kmeans_calls_refuse_a_workspace_one_byte_short():
    from vqvae_amd._device import ptr, stream_ptr
    lib, dev = _lib(), _dev()
    n, d, K, S, L = 129, 17, 33, 2, 3
    r = np.random.RandomState(0)
    X, C = _t(r.randn(n, d).astype(np.float32)), _t(r.randn(S, K, d).astype(np.float32))
    g = GuardedWorkspace("ones32")
    with torch.cuda.device(dev):
        nbytes = lib.geo_kmeans_workspace_bytes(n, d, K, 1, 1)
        ws = g.workspace(nbytes, dev)
        out = _sentinels(dev, labels=((n,), torch.int32), keys=((n,), torch.float64))
        nfb = ctypes.c_int64(SENTINEL)
        status = lib.geo_kmeans_assign(ptr(X), n, d, ptr(C), K, ptr(out["labels"]), ptr(out["keys"]), ctypes.byref(nfb), ptr(ws),
                                       nbytes - 1, stream_ptr())
        _refused(status, GEO_E_WORKSPACE, "geo_kmeans_assign", out, g)
        assert nfb.value == SENTINEL

        out = _sentinels(dev, centers=((S, K, d), torch.float32), labels=((S, n), torch.int32))
        host = {"inertia": np.full(S, SENTINEL, np.float64), "n_iter": np.full(S, SENTINEL, np.int32),
                "strict": np.full(S, SENTINEL, np.int32)}
        status = lib.geo_kmeans_lloyd(ptr(X), n, d, K, S, ptr(C), 5, 0.0, ptr(out["centers"]), ptr(out["labels"]),
                                      *(host[k].ctypes.data_as(ctypes.c_void_p) for k in ("inertia", "n_iter", "strict")),
                                      ctypes.byref(nfb), ptr(ws), nbytes - 1, stream_ptr())
        _refused(status, GEO_E_WORKSPACE, "geo_kmeans_lloyd", dict(out, **host), g)
        assert nfb.value == SENTINEL

        nbytes = lib.geo_kmeans_workspace_bytes(n, d, K, S, L)
        ws = g.workspace(nbytes, dev)
        first = np.array([3, 100], dtype=np.int32)
        u = r.rand(S, K - 1, L)
        out = _sentinels(dev, indices=((S, K), torch.int32), centers=((S, K, d), torch.float32))
        status = lib.geo_kmeans_pp(ptr(X), n, d, K, S, L, first.ctypes.data_as(ctypes.c_void_p), u.ctypes.data_as(ctypes.c_void_p),
                                   ptr(out["indices"]), ptr(out["centers"]), ptr(ws), nbytes - 1, stream_ptr())
        _refused(status, GEO_E_WORKSPACE, "geo_kmeans_pp", out, g)


def test_vq_forward_refuses_a_workspace_one_byte_short():
    from vqvae_amd._device import ptr, stream_ptr
    lib, dev = _lib(), _dev()
    B, C, HW, K = 3, 33, 35, 33
    z = torch.randn(B, C, HW, generator=_g(0)).to(dev)
    state = _sentinels(dev, embed=((K, C), torch.float32), cluster_size=((K,), torch.float32), embed_avg=((K, C), torch.float32))
    out = _sentinels(dev, z_q=((B, C, HW), torch.float32), z_q_st=((B, C, HW), torch.float32), idx=((B, HW), torch.int64),
                     loss=((), torch.float32), stats=((4,), torch.float32), counts=((K,), torch.int32))
    g = GuardedWorkspace("ones32")
    with torch.cuda.device(dev):
        nbytes = lib.geo_vq_workspace_bytes(B * HW, C, K)
        ws = g.workspace(nbytes, dev)
        status = lib.geo_vq_forward(ptr(z), 0, B, C, HW, ptr(state["embed"]), ptr(state["cluster_size"]), ptr(state["embed_avg"]), K,
                                    1, 0.99, 1e-5, 0.25, ptr(out["z_q"]), ptr(out["z_q_st"]), ptr(out["idx"]), ptr(out["loss"]),
                                    ptr(out["stats"]), ptr(out["counts"]), ptr(ws), nbytes - 1, stream_ptr())
    _refused(status, GEO_E_WORKSPACE, "geo_vq_forward", dict(out, **state), g)


def test_elbo_forward_refuses_a_workspace_one_byte_short():
    """Through GEO_REQUIRE: GEO_E_ARG where the other calls answer GEO_E_WORKSPACE."""
    from vqvae_amd._device import ptr, stream_ptr
    lib, dev = _lib(), _dev()
    B, P, d = 3, 785, 5
    g0 = _g(0)
    logits, x, mu, logvar = (t.to(dev) for t in (torch.randn(B, P, generator=g0), torch.rand(B, P, generator=g0),
                                                 torch.randn(B, d, generator=g0), torch.randn(B, d, generator=g0)))
    out = _sentinels(dev, out=((4,), torch.float64))
    g = GuardedWorkspace("ones32")
    with torch.cuda.device(dev):
        nbytes = lib.geo_vae_elbo_workspace_bytes(B, P, d)
        ws = g.workspace(nbytes, dev)
        status = lib.geo_vae_elbo_forward(ptr(logits), ptr(x), ptr(mu), ptr(logvar), B, P, d, 0, 1, 0.5, 1.0, 2.0, 1, ptr(out["out"]),
                                          ptr(ws), nbytes - 1, stream_ptr())
    _refused(status, GEO_E_ARG, "geo_vae_elbo_forward", out, g)
