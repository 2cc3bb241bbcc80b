"""ctypes binding of libgeo_hip.so (include/geo_hip.h).  There is no fallback: importing a kernel
entry point without the built library raises, and every call checks the returned status."""
import ctypes
import os

import torch  # noqa: F401  -- must come first: libgeo_hip.so has to bind to the HIP runtime PyTorch-ROCm loads,
#                              so that device pointers and streams are shared (two runtimes = "no device")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgeo_hip.so")

c_p = ctypes.c_void_p
i32, i64, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t


class DecoderDesc(ctypes.Structure):
    """geo_decoder_desc of include/geo_hip.h."""
    _fields_ = ([(n, i32) for n in ("latent_dim", "c0", "c1", "c2", "out_channels", "out_size", "norm",
                                    "bn_train", "groups1", "groups2")]
                + [("eps", ctypes.c_float)]
                + [(n, c_p) for n in ("w_in", "b_in", "w1", "b1", "g1", "be1", "rm1", "rv1",
                                      "w2", "b2", "g2", "be2", "rm2", "rv2", "w3", "b3")]
                + [("update_running", i32), ("momentum", ctypes.c_float)])


class VanillaDecoderDesc(ctypes.Structure):
    """geo_vanilla_decoder_desc of include/geo_hip.h."""
    _fields_ = ([(n, i32) for n in ("latent_dim", "c1", "c2", "out_channels", "out_size")]
                + [(n, c_p) for n in ("At", "c", "w2p", "scale2", "shift2", "w3p", "b3", "w2t", "w3t", "Atq")])


class SpatialImageDecoderDesc(ctypes.Structure):
    """geo_spatial_image_decoder_desc of include/geo_hip.h."""
    _fields_ = ([(n, i32) for n in ("latent_dim", "c1", "c2", "out_channels", "out_size")]
                + [(n, c_p) for n in ("w1p", "scale1", "shift1", "w2p", "scale2", "shift2", "w3p", "b3", "w1t", "w2t",
                                         "w3t")])


class ImageEncoderDesc(ctypes.Structure):
    """geo_image_encoder_desc of include/geo_hip.h."""
    _fields_ = ([(n, i32) for n in ("in_channels", "in_size", "e1", "e2", "e3", "latent_dim", "spatial_head")]
                + [(n, c_p) for n in ("w1p", "scale1", "shift1", "w2p", "scale2", "shift2", "w3p", "scale3", "shift3", "whp", "bh")])


class LPIPSAlexDesc(ctypes.Structure):
    """geo_lpips_alex_desc of include/geo_hip.h."""
    _fields_ = [(n, c_p) for n in ("w1p", "b1", "w2p", "b2", "w3p", "b3", "w4p", "b4", "w5p", "b5",
                                   "lin1", "lin2", "lin3", "lin4", "lin5")]


class PriorDesc(ctypes.Structure):
    """geo_prior_desc of include/geo_hip.h."""
    _fields_ = ([(n, i32) for n in ("num_tokens", "embed_dim", "n_layers", "n_head", "max_seq_len", "num_classes")]
                + [("arena", c_p)]
                + [(n, i64) for n in ("pos_emb", "token_emb", "class_emb", "ln_f_w", "ln_f_b", "head_w")]
                + [("block", ctypes.POINTER(i64))])


_SIGNATURES = {
    "geo_version": (ctypes.c_int, []),
    "geo_last_error": (ctypes.c_char_p, []),
    "geo_set_option": (ctypes.c_int, [ctypes.c_char_p, i32]),
    "geo_sssp_workspace_bytes": (sz, [i32, i64, i32]),
    "geo_sssp_multi": (ctypes.c_int, [c_p, c_p, c_p, i32, i64, c_p, i32, c_p, c_p, c_p, c_p, c_p, sz, c_p, c_p]),
    "geo_sssp_nearest_workspace_bytes": (sz, [i32, i64]),
    "geo_sssp_nearest_source": (ctypes.c_int, [c_p, c_p, c_p, i32, i64, c_p, i32, c_p, c_p, c_p, sz, c_p, c_p]),
    "geo_sssp_last_profile": (ctypes.c_int, [c_p, c_p]),
    "geo_sssp_plan": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32]),
    "geo_prior_attention_fwd": (ctypes.c_int, [c_p, c_p, ctypes.c_float, i32, i32, i32, i32, c_p, c_p, c_p]),
    "geo_prior_attention_bwd": (ctypes.c_int, [c_p, c_p, c_p, ctypes.c_float, c_p, i32, i32, i32, i32, c_p, c_p]),
    "geo_prior_adamw": (ctypes.c_int, [c_p, c_p, c_p, c_p, i64, c_p, c_p, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_double, c_p]),
    "geo_sssp_single_update": (ctypes.c_int, [c_p, c_p, c_p, i32, i32, c_p, c_p, c_p, i32, c_p, sz, c_p, c_p]),
    "geo_kpp_workspace_bytes": (sz, [i32]),
    "geo_cluster_costs": (ctypes.c_int, [c_p, i64, c_p, c_p, c_p, i32, i32, c_p, c_p]),
    "geo_rows_argmin": (ctypes.c_int, [c_p, i64, c_p, i32, i32, c_p, c_p, c_p]),
    "geo_pam_swap_deltas": (ctypes.c_int, [c_p, i64, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, c_p, c_p, c_p]),
    "geo_attach_argmin": (ctypes.c_int, [c_p, i64, i32, c_p, c_p, i32, i64, c_p, c_p, c_p]),
    "geo_cell_costs_tile": (i32, []),
    "geo_cell_costs_resident_max_nodes": (i32, []),
    "geo_cell_costs_workspace_bytes": (sz, [i32, i64, i32, i32]),
    "geo_cell_costs_min_workspace_bytes": (sz, [i32, i64, i32, i32]),
    "geo_cell_costs": (ctypes.c_int, [c_p, c_p, c_p, i32, i64, c_p, c_p, c_p, i32, i32, i32, c_p, c_p, sz, c_p, c_p]),
    "geo_kpp_resident_max_nodes": (i32, []),
    "geo_kpp_chain": (ctypes.c_int, [c_p, c_p, c_p, i32, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, i32, i32, c_p, sz, c_p, c_p]),
    "geo_knn_workspace_bytes": (sz, [i64, i32]),
    "geo_knn_topk": (ctypes.c_int, [c_p, i64, i32, i32, i32, i64, i64, c_p, c_p, c_p, sz, c_p]),
    "geo_knn_query_workspace_bytes": (sz, [i64, i64, i32]),
    "geo_knn_query_min_workspace_bytes": (sz, [i64, i32]),
    "geo_knn_query": (ctypes.c_int, [c_p, i64, c_p, i64, i32, i32, i32, c_p, c_p, c_p, sz, c_p]),
    "geo_knn_last_path": (ctypes.c_int, []),
    "geo_knn_thresholds": (ctypes.c_int, [c_p, i64, i32, i32, i32, i64, i64, i32, c_p, c_p, sz, c_p]),
    "geo_nearest_foreign_workspace_bytes": (sz, [i64, i32]),
    "geo_nearest_foreign": (ctypes.c_int, [c_p, i64, i32, i32, c_p, c_p, i64, c_p, c_p, c_p, sz, c_p]),
    "geo_bridge_components_workspace_bytes": (sz, [i64, i32, i32]),
    "geo_bridge_components": (ctypes.c_int, [c_p, i64, i32, i32, c_p, i32, c_p, c_p, c_p, c_p, sz, c_p]),
    "geo_csr_insert_workspace_bytes": (sz, [i32, i64]),
    "geo_csr_insert_count": (ctypes.c_int, [c_p, c_p, i32, c_p, c_p, c_p, i64, c_p, c_p, c_p, sz, c_p]),
    "geo_csr_insert_fill": (ctypes.c_int, [c_p, c_p, c_p, i32, i64, c_p, c_p, c_p, c_p, sz, c_p]),
    "geo_symmetrize_workspace_bytes": (sz, [i32, i32]),
    "geo_symmetrize_count": (ctypes.c_int, [c_p, c_p, i32, i32, i32, c_p, c_p, c_p, sz, c_p]),
    "geo_symmetrize_fill": (ctypes.c_int, [c_p, c_p, i32, i32, i32, c_p, c_p, c_p, c_p, sz, c_p]),
    "geo_upper_edges_count": (ctypes.c_int, [c_p, c_p, i32, c_p, c_p, c_p, sz, c_p]),
    "geo_upper_edges_fill": (ctypes.c_int, [c_p, c_p, i32, c_p, c_p, c_p, c_p, c_p]),
    "geo_cc_workspace_bytes": (sz, [i32]),
    "geo_connected_components": (ctypes.c_int, [c_p, c_p, i32, c_p, c_p, c_p, sz, c_p]),
    "geo_csr_compact_workspace_bytes": (sz, [i32]),
    "geo_csr_compact_count": (ctypes.c_int, [c_p, c_p, c_p, i32, c_p, i32, c_p, c_p, c_p, c_p, c_p, sz, c_p]),
    "geo_csr_compact_fill": (ctypes.c_int, [c_p, c_p, c_p, i32, c_p, i32, c_p, c_p, c_p, c_p, c_p]),
    "geo_jvp_workspace_bytes": (sz, [ctypes.POINTER(DecoderDesc), i64, i32]),
    "geo_jvp_edges_workspace_bytes": (sz, [ctypes.POINTER(DecoderDesc), i64, i64, i32]),
    "geo_jvp_plan": (ctypes.c_int, [ctypes.POINTER(DecoderDesc), i64, i64, i32, i32, sz]),
    "geo_jvp_head_stream": (ctypes.c_int, [ctypes.POINTER(DecoderDesc), i64, i64, i32, i32]),
    "geo_decoder_jvp_edges": (ctypes.c_int, [ctypes.POINTER(DecoderDesc), c_p, i64, c_p, c_p, i64, i32, c_p, c_p, sz, c_p]),
    "geo_jvp_edges_part_workspace_bytes": (sz, [ctypes.POINTER(DecoderDesc), i64, i64, i64, i32]),
    "geo_jvp_plan_part": (ctypes.c_int, [ctypes.POINTER(DecoderDesc), i64, i64, i64, i32, i32, sz]),
    "geo_decoder_jvp_edges_part": (ctypes.c_int, [ctypes.POINTER(DecoderDesc), c_p, i64, c_p, c_p, i64, i64, i32, c_p, c_p, sz,
                                                  c_p]),
    "geo_decoder_jvp_pairs": (ctypes.c_int, [ctypes.POINTER(DecoderDesc), c_p, c_p, i64, i32, c_p, c_p, sz, c_p]),
    "geo_metric_tensor_workspace_bytes": (sz, [ctypes.POINTER(DecoderDesc), i64]),
    "geo_metric_tensor_min_workspace_bytes": (sz, [ctypes.POINTER(DecoderDesc)]),
    "geo_decoder_metric_tensor": (ctypes.c_int, [ctypes.POINTER(DecoderDesc), c_p, i64, c_p, c_p, c_p, c_p, c_p, sz, c_p]),
    "geo_curve_workspace_bytes": (sz, [ctypes.POINTER(DecoderDesc), i64, i32]),
    "geo_curve_min_workspace_bytes": (sz, [ctypes.POINTER(DecoderDesc), i32]),
    "geo_curve_energy": (ctypes.c_int, [ctypes.POINTER(DecoderDesc), c_p, i64, i32, c_p, c_p, c_p, c_p, c_p, c_p, sz, c_p]),
    "geo_curve_relax": (ctypes.c_int, [ctypes.POINTER(DecoderDesc), c_p, i64, i32, i32, c_p, c_p, c_p, c_p, c_p, c_p, sz, c_p]),
    "geo_vanilla_jvp_workspace_bytes": (sz, [ctypes.POINTER(VanillaDecoderDesc), i64]),
    "geo_vanilla_jvp_edges_workspace_bytes": (sz, [ctypes.POINTER(VanillaDecoderDesc), i64, i64]),
    "geo_vanilla_jvp_pairs": (ctypes.c_int, [ctypes.POINTER(VanillaDecoderDesc), c_p, c_p, i64, i32, c_p, c_p, sz, c_p]),
    "geo_vanilla_jvp_edges": (ctypes.c_int, [ctypes.POINTER(VanillaDecoderDesc), c_p, i64, c_p, c_p, i64, i32, c_p, c_p, sz, c_p]),
    "geo_vanilla_vjp_workspace_bytes": (sz, [ctypes.POINTER(VanillaDecoderDesc), i64]),
    "geo_vanilla_vjp_min_workspace_bytes": (sz, [ctypes.POINTER(VanillaDecoderDesc)]),
    "geo_vanilla_vjp": (ctypes.c_int, [ctypes.POINTER(VanillaDecoderDesc), c_p, c_p, i64, c_p, c_p, c_p, sz, c_p]),
    "geo_vanilla_curve_workspace_bytes": (sz, [ctypes.POINTER(VanillaDecoderDesc), i64, i32]),
    "geo_vanilla_curve_min_workspace_bytes": (sz, [ctypes.POINTER(VanillaDecoderDesc), i32]),
    "geo_vanilla_curve_energy": (ctypes.c_int, [ctypes.POINTER(VanillaDecoderDesc), c_p, i64, i32, c_p, c_p, c_p, c_p, c_p, c_p, sz, c_p]),
    "geo_vanilla_curve_relax": (ctypes.c_int, [ctypes.POINTER(VanillaDecoderDesc), c_p, i64, i32, i32, c_p, c_p, c_p, c_p, c_p, c_p, sz,
                                               c_p]),
    "geo_vanilla_metric_workspace_bytes": (sz, [ctypes.POINTER(VanillaDecoderDesc), i64]),
    "geo_vanilla_metric_min_workspace_bytes": (sz, [ctypes.POINTER(VanillaDecoderDesc)]),
    "geo_vanilla_metric_tensor": (ctypes.c_int, [ctypes.POINTER(VanillaDecoderDesc), c_p, c_p, i64, c_p, c_p, c_p, c_p, c_p, c_p, sz,
                                                 c_p]),
    "geo_sym_spectrum": (ctypes.c_int, [c_p, i64, i32, i32, c_p, c_p, c_p, c_p]),
    "geo_sym_spectrum_sweeps": (ctypes.c_int, [c_p, i64, i32, i32, c_p, c_p, c_p, c_p, c_p]),
    "geo_sym_spectrum_sweep_cap": (i32, []),
    "geo_vanilla_decode_workspace_bytes": (sz, [ctypes.POINTER(VanillaDecoderDesc), i64]),
    "geo_vanilla_decode": (ctypes.c_int, [ctypes.POINTER(VanillaDecoderDesc), c_p, c_p, i64, c_p, c_p, sz, c_p]),
    "geo_spatial_decode_workspace_bytes": (sz, [ctypes.POINTER(SpatialImageDecoderDesc), i64]),
    "geo_spatial_decode": (ctypes.c_int, [ctypes.POINTER(SpatialImageDecoderDesc), c_p, c_p, c_p, i64, c_p, c_p, sz, c_p]),
    "geo_spatial_vjp_workspace_bytes": (sz, [ctypes.POINTER(SpatialImageDecoderDesc), i64]),
    "geo_spatial_vjp_min_workspace_bytes": (sz, [ctypes.POINTER(SpatialImageDecoderDesc)]),
    "geo_spatial_vjp": (ctypes.c_int, [ctypes.POINTER(SpatialImageDecoderDesc), c_p, c_p, i64, c_p, c_p, c_p, sz, c_p]),
    "geo_spatial_curve_workspace_bytes": (sz, [ctypes.POINTER(SpatialImageDecoderDesc), i64, i32]),
    "geo_spatial_curve_min_workspace_bytes": (sz, [ctypes.POINTER(SpatialImageDecoderDesc), i32]),
    "geo_spatial_curve_energy": (ctypes.c_int, [ctypes.POINTER(SpatialImageDecoderDesc), c_p, i64, i32, c_p, c_p, c_p, c_p, c_p, c_p, sz,
                                                c_p]),
    "geo_spatial_curve_relax": (ctypes.c_int, [ctypes.POINTER(SpatialImageDecoderDesc), c_p, i64, i32, i32, c_p, c_p, c_p, c_p, c_p, c_p, sz,
                                               c_p]),
    "geo_image_encode_workspace_bytes": (sz, [ctypes.POINTER(ImageEncoderDesc), i64]),
    "geo_image_encode": (ctypes.c_int, [ctypes.POINTER(ImageEncoderDesc), c_p, i64, c_p, c_p, c_p, sz, c_p]),
    "geo_lpips_alex_workspace_bytes": (sz, [i64]),
    "geo_lpips_alex": (ctypes.c_int, [ctypes.POINTER(LPIPSAlexDesc), c_p, c_p, i64, c_p, c_p, c_p, sz, c_p]),
    "geo_gather_edge_weights":(ctypes.c_int, [c_p, c_p, i64, c_p, c_p]),
    "geo_prior_sample_workspace_bytes": (sz, [ctypes.POINTER(PriorDesc), i32, i32]),
    "geo_prior_sample": (ctypes.c_int, [ctypes.POINTER(PriorDesc), c_p, i32, i32, c_p, c_p, ctypes.c_float, i32, c_p, c_p, i32,
                                        c_p, sz, c_p]),
    "geo_kmeans_workspace_bytes": (sz, [i64, i32, i32, i32, i32]),
    "geo_kmeans_assign": (ctypes.c_int, [c_p, i64, i32, c_p, i32, c_p, c_p, c_p, c_p, sz, c_p]),
    "geo_kmeans_pp": (ctypes.c_int, [c_p, i64, i32, i32, i32, i32, c_p, c_p, c_p, c_p, c_p, sz, c_p]),
    "geo_kmeans_lloyd": (ctypes.c_int, [c_p, i64, i32, i32, i32, c_p, i32, ctypes.c_double, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                        sz, c_p]),
    "geo_image_pair_moments": (ctypes.c_int, [c_p, c_p, i64, i64, c_p, c_p]),
    "geo_cluster_label_scores": (ctypes.c_int, [c_p, c_p, i64, i32, i32, i32, c_p, c_p, c_p, c_p, c_p, c_p]),
    "geo_feature_workspace_bytes": (sz, [i64, i32]),
    "geo_feature_colstats": (ctypes.c_int, [c_p, i64, i32, i64, c_p, c_p, c_p, c_p, sz, c_p]),
    "geo_feature_gram": (ctypes.c_int, [c_p, i64, i32, i64, c_p, c_p, c_p, c_p, sz, c_p]),
    "geo_feature_project": (ctypes.c_int, [c_p, i64, i32, i64, c_p, c_p, c_p, i32, c_p, c_p]),
    "geo_path_stats": (ctypes.c_int, [c_p, i64, i32, i64, c_p, c_p, c_p, c_p, c_p]),
    "geo_sssp_paths_count": (ctypes.c_int, [c_p, i64, i32, c_p, c_p, c_p, i64, i32, i32, c_p, c_p, c_p]),
    "geo_sssp_paths_fill": (ctypes.c_int, [c_p, i64, i32, c_p, c_p, c_p, i64, i32, c_p, c_p, c_p, c_p, i64, c_p, c_p, c_p]),
    "geo_polyline_resample": (ctypes.c_int, [c_p, i64, i32, c_p, c_p, c_p, i64, i32, c_p, c_p]),
    "geo_csr_set_symmetric": (ctypes.c_int, [c_p, c_p, c_p, i32, c_p, c_p, c_p, i64, c_p, c_p]),
    "geo_vq_workspace_bytes": (sz, [i64, i32, i32]),
    "geo_vq_forward": (ctypes.c_int, [c_p, i32, i32, i32, i32, c_p, c_p, c_p, i32, i32, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_double, c_p, c_p, c_p, c_p, c_p, c_p, c_p, sz, c_p]),
    "geo_vq_backward": (ctypes.c_int, [c_p, c_p, ctypes.c_double, c_p, i32, c_p, i64, c_p, c_p]),
    "geo_vae_elbo_workspace_bytes": (sz, [i64, i64, i64]),
    "geo_vae_elbo_forward": (ctypes.c_int, [c_p, c_p, c_p, c_p, i64, i64, i64, i32, i32, ctypes.c_double, ctypes.c_double,
                                            ctypes.c_double, i32, c_p, c_p, sz, c_p]),
    "geo_vae_elbo_backward": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, i64, i64, i64, i32, i32, ctypes.c_double,
                                             ctypes.c_double, ctypes.c_double, i32, c_p, c_p, c_p, c_p]),
    "geo_batch_assemble": (ctypes.c_int, [c_p, i64, i32, i32, i32, c_p, i32, c_p, c_p, i32, c_p, c_p, c_p, c_p]),
    "geo_prdc_workspace_bytes": (sz, [i64, i64, i32]),
    "geo_prdc_min_workspace_bytes": (sz, [i32]),
    "geo_kth_radius": (ctypes.c_int, [c_p, i64, i32, i32, c_p, c_p, sz, c_p]),
    "geo_ball_count": (ctypes.c_int, [c_p, c_p, i64, c_p, i64, i32, c_p, c_p, c_p, c_p, sz, c_p]),
}

EXPORTS = tuple(_SIGNATURES)

# geo_jvp_plan's encoding (the GEO_JVP_* constants of include/geo_hip.h)
JVP_FRONT = ("valu", "mfma")
JVP_MID = ("pipe", "pipe_dedup", "all", "all_tangent", "chunk")
JVP_BACK = ("mfma", "per_node", "dedup", "valu")


def decode_jvp_plan(code: int) -> dict:
    """A non-negative geo_jvp_plan answer as names: front / mid / back kernels, the front's compiled width, flags, passes.
    `front_once` (GEO_JVP_FRONT_ONCE, library 1.0.5) is a key of the answer only where the flag is set: a code without it decodes
    to exactly the dictionary it always did -- read it with .get("front_once", False)."""
    assert code >= 0, code
    r = {"front": JVP_FRONT[code & 3], "dmax": 16 << ((code >> 2) & 3), "mid": JVP_MID[(code >> 4) & 15],
         "back": JVP_BACK[(code >> 8) & 15], "per_node": bool(code & 0x1000), "node_jacobian": bool(code & 0x2000),
         "dedup": bool(code & 0x4000), "passes": code >> 16}
    if code & 0x8000:
        r["front_once"] = True
    return r


_lib = None


class GeoHipError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load libgeo_hip.so (built by vqvae_amd/csrc/Makefile or __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GeoHipError(
                f"{LIB_PATH} is missing: build it with `make -C vqvae_amd/csrc` "
                "(the geodesic-codebook path has no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)           # AttributeError if the library lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        raise GeoHipError(f"{what} failed with status {status}: {load().geo_last_error().decode()}")
