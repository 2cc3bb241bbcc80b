// geo_common.h -- shared host-side helpers for libgeo_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "geo_hip.h"

namespace geo {

void set_error(const char *fmt, ...);

#define GEO_HIP_CHECK(expr)                                                                      \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            geo::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return GEO_E_HIP;                                                                    \
        }                                                                                        \
    } while (0)

#define GEO_REQUIRE(cond, ...)              \
    do {                                    \
        if (!(cond)) {                      \
            geo::set_error(__VA_ARGS__);    \
            return GEO_E_ARG;               \
        }                                   \
    } while (0)

#define GEO_LAUNCH_CHECK() GEO_HIP_CHECK(hipGetLastError())

// Experiment switches (DESIGN.md "Experiment switches").  Seeded ONCE from the environment when the library is
// loaded; afterwards only geo_set_option() changes them.  -1 = automatic / default behaviour.
struct Options {
    int sssp_sb = -1, sssp_act = 1, sssp_sparse_div = -1, sssp_map_div = -1, sssp_group = 1, sssp_grouped_cap = 256,
        sssp_trace = 0, sssp_u32 = 1, sssp_push = 1 /* near-far push solve for long geodesics; 2 = for every graph */,
        sssp_delta = 8 /* near-far bucket width in mean edge weights */, sssp_order = 0 /* sources ordered along 0: two exact landmark distances, 1: graph cells, 2: two landmark hop counts (1, 2: cheaper to compute, worse batches on the bench's swiss graph) */, sssp_push_blocks = 64, knn_filter = 1, kpp_grid = 256, kpp_profile = 0, jvp_mid = 0 /* ConvT2: 2 = per-chunk kernel, 3 = one tile per workgroup instead of the persistent kernel */,
        jvp_back_valu = 0, jvp_front_valu = 0, jvp_per_node = 1 /* fixed-statistics decoders: primal ConvT2 / ConvT3 once per latent */,
        jvp_node_jacobian = 1 /* fixed statistics, d <= 16: decoder Jacobian once per latent, edge ends from its columns (1: when the graph has enough edges per latent, 2: always, 0: never) */,
        jvp_start_dedup = 1 /* train-mode BatchNorm, graph edges: each chunk's start-side primal ConvT2 / ConvT3 rows once per run of equal src (0: once per slot) */,
        jvp_front_once = 1 /* on that route with the vector first layer: the tangent row once per edge, the start-side primal row once per run (0: every row of both sides) */,
        jvp_head_stream = 1 /* 16-output ConvT3 head without GroupNorm: head_stream_kernel, the next K block's rows in flight while one is converted and multiplied (0: back_mfma_kernel; same bits) */,
        curve_repack = 0 /* geo_curve_relax: 1 = pack the decoder's weights before every evaluation, as a run_jvp call per iteration would, instead of once per slice (a measurement switch; same bits) */,
        prdc_split = -1 /* geo_kth_radius / geo_ball_count: corpus ranges per query tile; -1 = enough to fill the chip, S >= 1 = S (cut to the corpus tiles, 32 and the workspace; same bits) */;
};
Options &options();

static inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// Bump allocator.  Over a caller's workspace it carves; default-constructed it measures: take() returns nullptr and only adds
// up sizes.  take() always advances `off`, past the end too (returning nullptr there): after a layout function ran, `off` is the
// bytes it needs and ok() whether it fitted.  One layout function per workspace, run by its query and its call.
struct Arena {
    char *base = nullptr;
    size_t size = SIZE_MAX, off = 0;
    bool measuring = true;
    Arena() {}
    Arena(void *p, size_t n) : base(static_cast<char *>(p)), size(n), measuring(false) {}
    bool ok() const { return measuring || (base && off <= size); }      // a carving arena over a null workspace never fits
    template <typename T>
    T *take(size_t count) {
        const size_t at = off;
        off += align_up(count * sizeof(T));
        return base && off <= size ? reinterpret_cast<T *>(base + at) : nullptr;
    }
    template <typename T>
    void take(T *&p, size_t count) { p = take<T>(count); }
    size_t mark() const { return off; }            // an optional group: m = mark(), take it, rewind(m) if !ok()
    void rewind(size_t m) { off = m; }
};
// The bytes of a layout function lay(Arena &, args...): what its *_workspace_bytes query answers, plus the query's named reserve.
template <typename F, typename... A>
size_t measure(F lay, A... args) { Arena ar; lay(ar, args...); return ar.off; }

// The ABI's rule (geo_hip.h): a workspace smaller than the size query that belongs to the call is refused before any launch.
// `ar` is the arena the call's layout was just carved from: the query measures that layout, so the carve fits once the size does.
#define GEO_REQUIRE_WORKSPACE(name, ar, need)                                                        \
    do {                                                                                             \
        if ((ar).size < (need) || !(ar).ok()) {                                                      \
            geo::set_error(name ": workspace %zu too small (%zu needed)", (ar).size, (size_t)(need)); \
            return GEO_E_WORKSPACE;                                                                  \
        }                                                                                            \
    } while (0)

// ---- passes over a caller's workspace.  An entry point that keeps per-item buffers of 4-byte elements in the workspace cuts its
// n items into passes of at most `cap`: the largest pass whose buffers fit, found by shrinking from min(n, cap).  The
// *_workspace_bytes query and the carve use the one byte formula, so they cannot drift apart.
static inline int64_t shrink_pass(int64_t items) { return items > 64 ? items - items / 8 : items - 1; }

// Bytes of the `nb` buffers of a pass of `items` items, buffer b holding per_item[b] 4-byte elements per item.
static inline size_t pass_bytes(const size_t *per_item, int nb, int64_t items) {
    size_t bytes = 0;
    for (int b = 0; b < nb; ++b) bytes += align_up((size_t)items * per_item[b] * 4);
    return bytes;
}

// What a *_workspace_bytes function answers for n >= 0 items: the buffers of one full pass (of one item for n = 0).
static inline size_t pass_query_bytes(const size_t *per_item, int nb, int64_t cap, int64_t n) {
    return pass_bytes(per_item, nb, n < 1 ? 1 : (n < cap ? n : cap));
}

// The pass size for n >= 1 items in a workspace of ws_bytes and the buffers carved from it, or GEO_E_WORKSPACE with the
// error text prefixed by the entry point's name `who`.
static inline int plan_passes(const char *who, const size_t *per_item, int nb, int64_t cap, int64_t n, void *ws, size_t ws_bytes,
                              int64_t *items, float **bufs) {
    int64_t pb = n < cap ? n : cap;
    while (pb >= 1 && pass_bytes(per_item, nb, pb) > ws_bytes) pb = shrink_pass(pb);
    if (pb < 1) {
        set_error("%s: workspace of %zu bytes is below the minimum of %zu", who, ws_bytes, pass_bytes(per_item, nb, 1));
        return GEO_E_WORKSPACE;
    }
    Arena ar(ws, ws_bytes);
    for (int b = 0; b < nb; ++b) ar.take(bufs[b], (size_t)pb * per_item[b]);
    if (!ar.ok()) {
        set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, ar.off);
        return GEO_E_WORKSPACE;
    }
    *items = pb;
    return GEO_OK;
}

// Exclusive prefix sum of int32 counts into int32 offsets (out[n] = total); returns total on host
// when total_host != nullptr (synchronises in that case).  tmp: >= scan_tmp_bytes(n).
size_t scan_tmp_bytes(int64_t n);
int exclusive_scan_i32(const int32_t *in, int32_t *out, int64_t n, void *tmp, size_t tmp_bytes,
                       int64_t *total_host, hipStream_t stream);

static inline int grid_for(int64_t work_items, int per_block, int cap = 8192) {
    int64_t g = (work_items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return static_cast<int>(g);
}

}  // namespace geo
