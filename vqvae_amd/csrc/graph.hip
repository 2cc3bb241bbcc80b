// graph.hip -- kNN-list symmetrisation, upper-triangle edge list, connected components and CSR
// compaction on the GPU (gfx950).  All of it is integer/byte work bound by HBM / L2 traffic.
//
// Replaces, in the reference:
//   csr_matrix + W.maximum/minimum(W.T) + setdiag(0) + eliminate_zeros   src/geo/knn_graph_optimized.py:54-66
//   W.nonzero() / rows < cols, U + U^T                                   src/scripts/build_codebook.py:43-45,53-54
//   scipy.sparse.csgraph.connected_components                            src/geo/knn_graph_optimized.py:175,187
//   W[mask][:, mask]                                                     src/scripts/build_codebook.py:59
#include "geo_common.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int WPB = 4;   // waves (= rows) per 256-thread block

// ------------------------------------------------------------------------------------ symmetrise
__global__ __launch_bounds__(256) void count_in_kernel(const int32_t *__restrict__ nbr, int64_t total, int32_t n,
                                                      int32_t *__restrict__ cnt_in) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t j = nbr[i];
        if (j >= 0 && j < n) atomicAdd(&cnt_in[j], 1);
    }
}

__global__ __launch_bounds__(256) void fill_in_kernel(const int32_t *__restrict__ nbr, const float *__restrict__ w,
                                                     int64_t total, int32_t n, int32_t k,
                                                     const int32_t *__restrict__ off_in, int32_t *__restrict__ cursor,
                                                     int32_t *__restrict__ in_src, float *__restrict__ in_w) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t j = nbr[i];
        if (j >= 0 && j < n) {
            const int32_t p = off_in[j] + atomicAdd(&cursor[j], 1);
            in_src[p] = (int32_t)(i / k);
            in_w[p] = w ? w[i] : 1.0f;
        }
    }
}

// weight of the directed entry a -> b in the kNN lists, 0 when absent (scipy: absent = 0)
__device__ __forceinline__ float directed_weight(const int32_t *__restrict__ nbr, const float *__restrict__ w,
                                                 int32_t k, int32_t a, int32_t b, bool *found) {
    const int32_t *row = nbr + (int64_t)a * k;
    for (int t = 0; t < k; ++t)
        if (row[t] == b) {
            *found = true;
            return w ? w[(int64_t)a * k + t] : 1.0f;
        }
    *found = false;
    return 0.0f;
}

// Element `t` of row r's candidate list: t < k -> out entry, else in entry.  Returns whether it is a
// kept primary of the symmetric matrix, with its column and value.
__device__ __forceinline__ bool sym_element(const int32_t *__restrict__ nbr, const float *__restrict__ w, int32_t n,
                                            int32_t k, int mode, const int32_t *__restrict__ off_in,
                                            const int32_t *__restrict__ in_src, const float *__restrict__ in_w,
                                            int32_t r, int32_t t, int32_t *col, float *val) {
    if (t < k) {
        const int32_t c = nbr[(int64_t)r * k + t];
        if (c < 0 || c >= n || c == r) return false;
        // a repeated column inside one list would be summed by scipy's COO->CSR; kNN lists have none
        const float wo = w ? w[(int64_t)r * k + t] : 1.0f;
        bool back;
        const float wb = directed_weight(nbr, w, k, c, r, &back);
        const float v = mode == 0 ? fmaxf(wo, wb) : fminf(wo, wb);
        *col = c;
        *val = v;
        return v != 0.0f;
    }
    if (mode != 0) return false;                       // mutual: an in-only entry has min(0, w) = 0
    const int32_t p = off_in[r] + (t - k);
    const int32_t c = in_src[p];
    if (c == r) return false;
    bool fwd;
    (void)directed_weight(nbr, w, k, r, c, &fwd);
    if (fwd) return false;                             // already produced by the out entry
    *col = c;
    *val = in_w[p];                                    // max(0, w)
    return *val != 0.0f;
}

// pass A: the kept primaries of row r, counted and left unsorted at a provisional position that needs no scan -- row r has at
// most k + in-degree(r) of them, so it starts at r k + off_in[r] (<= 2 n k in all).  Every element is evaluated once: the row
// offsets are known only after this pass, and sym_sort_kernel reads from the provisional position.
__global__ __launch_bounds__(256) void sym_count_kernel(const int32_t *__restrict__ nbr, const float *__restrict__ w,
                                                       int32_t n, int32_t k, int mode,
                                                       const int32_t *__restrict__ off_in,
                                                       const int32_t *__restrict__ in_src,
                                                       const float *__restrict__ in_w, int32_t *__restrict__ row_cnt,
                                                       int32_t *__restrict__ tmp_col, float *__restrict__ tmp_val) {
    const int lane = threadIdx.x & 63;
    const int32_t r = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (r >= n) return;
    const int32_t len = k + (off_in[r + 1] - off_in[r]);
    const int64_t base = (int64_t)r * k + off_in[r];
    int32_t cnt = 0;
    for (int32_t t0 = 0; t0 < len; t0 += 64) {
        const int32_t t = t0 + lane;
        int32_t c = 0;
        float v = 0.f;
        const bool keep = t < len && sym_element(nbr, w, n, k, mode, off_in, in_src, in_w, r, t, &c, &v);
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const int64_t p = base + cnt + __builtin_popcountll(m & ((1ull << lane) - 1ull));
            tmp_col[p] = c;
            tmp_val[p] = v;
        }
        cnt += __builtin_popcountll(m);
    }
    if (lane == 0) row_cnt[r] = cnt;
}

// pass B: rank sort of every row segment by column (columns inside a row are distinct)
// rows of the symmetrised graph, sorted by column (rank by counting inside the row).  The work item is a 64-entry SEGMENT
// of a row, not a row: kNN graphs of high-dimensional clouds have hubs (in-degrees in the thousands at d = 64), and one
// wave ranking a 7 000-entry row alone took 4 ms of the 50 000 x 64 configuration's step.
__global__ __launch_bounds__(256) void seg_count_kernel(const int32_t *__restrict__ indptr, int32_t n, int32_t *__restrict__ seg_cnt) {
    for (int32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x)
        seg_cnt[r] = (indptr[r + 1] - indptr[r] + 63) >> 6;
}

__global__ __launch_bounds__(256) void sym_sort_kernel(int32_t n, int32_t k, const int32_t *__restrict__ indptr,
                                                      const int32_t *__restrict__ seg_off,
                                                      const int32_t *__restrict__ off_in,
                                                      const int32_t *__restrict__ tmp_col,
                                                      const float *__restrict__ tmp_val, int32_t *__restrict__ indices,
                                                      float *__restrict__ data) {
    const int lane = threadIdx.x & 63;
    const int32_t w = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (w >= seg_off[n]) return;
    int32_t lo = 0, hi = n;                                    // the row r with seg_off[r] <= w < seg_off[r + 1]
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (seg_off[mid] <= w) lo = mid; else hi = mid;
    }
    const int32_t r = lo;
    const int32_t b = indptr[r], len = indptr[r + 1] - b;
    const int32_t *__restrict__ col = tmp_col + (int64_t)r * k + off_in[r];    // where sym_count_kernel left the row
    const float *__restrict__ val = tmp_val + (int64_t)r * k + off_in[r];
    const int32_t i = ((w - seg_off[r]) << 6) + lane;
    if (i < len) {
        const int32_t c = col[i];
        int32_t rank = 0;
        for (int32_t j = 0; j < len; ++j) rank += col[j] < c ? 1 : 0;
        indices[b + rank] = c;
        data[b + rank] = val[i];
    }
}

struct SymWs { int32_t *cnt_in, *off_in, *cursor, *in_src, *row_cnt, *tmp_col; float *in_w, *tmp_val; char *scan_tmp; size_t scan_bytes; };

// geo_symmetrize_count / _fill's layout: carved from the caller's workspace, measured by geo_symmetrize_workspace_bytes.
SymWs carve_sym(geo::Arena &ar, int32_t n, int32_t k) {
    const size_t n1 = (size_t)n + 1, nk = (size_t)n * k;
    SymWs o;
    ar.take(o.cnt_in, n1); ar.take(o.off_in, n1); ar.take(o.cursor, n1); ar.take(o.row_cnt, n1);
    ar.take(o.in_src, nk + 1); ar.take(o.in_w, nk + 1);
    ar.take(o.tmp_col, 2 * nk + 1); ar.take(o.tmp_val, 2 * nk + 1);
    o.scan_bytes = geo::scan_tmp_bytes((int64_t)n + 1);
    ar.take(o.scan_tmp, o.scan_bytes);
    return o;
}

// ------------------------------------------------------------------------------------ upper edges
__device__ __forceinline__ int32_t first_greater(const int32_t *__restrict__ idx, int32_t b, int32_t e, int32_t key) {
    while (b < e) {                       // first position with idx[pos] > key (sorted row)
        const int32_t m = (b + e) >> 1;
        if (idx[m] > key) e = m; else b = m + 1;
    }
    return b;
}

__global__ __launch_bounds__(256) void upper_count_kernel(const int32_t *__restrict__ indptr,
                                                         const int32_t *__restrict__ indices, int32_t n,
                                                         int32_t *__restrict__ cnt) {
    for (int32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x)
        cnt[r] = indptr[r + 1] - first_greater(indices, indptr[r], indptr[r + 1], r);
}

__global__ __launch_bounds__(256) void upper_fill_kernel(const int32_t *__restrict__ indptr,
                                                        const int32_t *__restrict__ indices, int32_t n,
                                                        const int32_t *__restrict__ upper_ptr,
                                                        int32_t *__restrict__ src, int32_t *__restrict__ dst,
                                                        int32_t *__restrict__ entry_edge) {
    const int lane = threadIdx.x & 63;
    const int32_t r = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (r >= n) return;
    const int32_t b = indptr[r], e = indptr[r + 1];
    const int32_t fu = e - (upper_ptr[r + 1] - upper_ptr[r]);        // first entry with col > r
    for (int32_t i = b + lane; i < e; i += 64) {
        const int32_t c = indices[i];
        int32_t eid = -1;
        if (c > r) {
            eid = upper_ptr[r] + (i - fu);
            src[eid] = r;
            dst[eid] = c;
        } else if (c < r) {
            const int32_t cb = indptr[c], ce = indptr[c + 1];
            const int32_t cfu = ce - (upper_ptr[c + 1] - upper_ptr[c]);
            const int32_t p = first_greater(indices, cfu, ce, r - 1);   // position of r in row c's upper part
            if (p < ce && indices[p] == r) eid = upper_ptr[c] + (p - cfu);
            (void)cb;
        }
        if (entry_edge) entry_edge[i] = eid;
    }
}

__global__ __launch_bounds__(256) void gather_weights_kernel(const float *__restrict__ len,
                                                            const int32_t *__restrict__ entry_edge, int64_t nnz,
                                                            float *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t e = entry_edge[i];
        out[i] = e >= 0 ? len[e] : 0.0f;
    }
}

// ------------------------------------------------------------------------------------ components
__global__ __launch_bounds__(256) void cc_init_kernel(int32_t *__restrict__ label, int32_t n) {
    for (int32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) label[v] = v;
}

// min-label hooking: a node takes the smallest label among itself and its neighbours and also
// pulls down the node its old label points to (so whole trees move at once).
__global__ __launch_bounds__(256) void cc_hook_kernel(const int32_t *__restrict__ indptr,
                                                     const int32_t *__restrict__ indices, int32_t n, int32_t *label,
                                                     int32_t *changed) {
    const int sub = threadIdx.x & 15;
    const int grp = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int ngrp = (gridDim.x * blockDim.x) >> 4;
    bool any = false;
    for (int32_t v = grp; v < n; v += ngrp) {
        const int32_t old = label[v];
        int32_t m = old;
        for (int32_t e = indptr[v] + sub; e < indptr[v + 1]; e += 16) m = min(m, label[indices[e]]);
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) m = min(m, __shfl_xor(m, off, 16));
        if (sub == 0 && m < old) {
            atomicMin(&label[v], m);
            atomicMin(&label[old], m);
            any = true;
        }
    }
    if (any) *changed = 1;
}

__global__ __launch_bounds__(256) void cc_jump_kernel(int32_t *label, int32_t n) {
    for (int32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        int32_t l = label[v];
        int32_t ll = label[l];
        while (ll < l) { l = ll; ll = label[l]; }
        label[v] = l;
    }
}

__global__ __launch_bounds__(256) void cc_roots_kernel(const int32_t *__restrict__ label, int32_t n,
                                                      int32_t *__restrict__ is_root) {
    for (int32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x)
        is_root[v] = label[v] == v ? 1 : 0;
}

__global__ __launch_bounds__(256) void cc_number_kernel(const int32_t *__restrict__ label,
                                                       const int32_t *__restrict__ root_rank, int32_t n,
                                                       int32_t *__restrict__ out) {
    for (int32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x)
        out[v] = root_rank[label[v]];
}

// ------------------------------------------------------------------------------------ compaction
__global__ __launch_bounds__(256) void keep_flags_kernel(const uint8_t *__restrict__ keep, int32_t n,
                                                        int32_t *__restrict__ flag) {
    for (int32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x)
        flag[v] = (!keep || keep[v]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void new_index_kernel(const int32_t *__restrict__ flag,
                                                       const int32_t *__restrict__ pos, int32_t n,
                                                       int32_t *__restrict__ new_index) {
    for (int32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x)
        new_index[v] = flag[v] ? pos[v] : -1;
}

__global__ __launch_bounds__(256) void compact_count_kernel(const int32_t *__restrict__ indptr,
                                                           const int32_t *__restrict__ indices,
                                                           const float *__restrict__ data, int32_t n,
                                                           const int32_t *__restrict__ new_index, int drop_zero,
                                                           int32_t *__restrict__ row_cnt_new) {
    const int lane = threadIdx.x & 63;
    const int32_t r = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (r >= n) return;
    const int32_t nr = new_index[r];
    if (nr < 0) return;
    int32_t cnt = 0;
    for (int32_t i = indptr[r] + lane; i < indptr[r + 1]; i += 64)
        cnt += (new_index[indices[i]] >= 0 && !(drop_zero && data && data[i] == 0.0f)) ? 1 : 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) row_cnt_new[nr] = cnt;
}

__global__ __launch_bounds__(256) void compact_fill_kernel(const int32_t *__restrict__ indptr,
                                                          const int32_t *__restrict__ indices,
                                                          const float *__restrict__ data, int32_t n,
                                                          const int32_t *__restrict__ new_index, int drop_zero,
                                                          const int32_t *__restrict__ indptr_new,
                                                          int32_t *__restrict__ indices_out,
                                                          float *__restrict__ data_out) {
    const int lane = threadIdx.x & 63;
    const int32_t r = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (r >= n) return;
    const int32_t nr = new_index[r];
    if (nr < 0) return;
    int32_t base = indptr_new[nr];
    const int32_t b = indptr[r], e = indptr[r + 1];
    for (int32_t i0 = b; i0 < e; i0 += 64) {
        const int32_t i = i0 + lane;
        int32_t nc = -1;
        bool keep = false;
        if (i < e) {
            nc = new_index[indices[i]];
            keep = nc >= 0 && !(drop_zero && data && data[i] == 0.0f);
        }
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const int32_t p = base + __builtin_popcountll(m & ((1ull << lane) - 1ull));
            indices_out[p] = nc;
            if (data_out) data_out[p] = data ? data[i] : 1.0f;
        }
        base += __builtin_popcountll(m);
    }
}

// ------------------------------------------------------------------------------------ insertion
// add_row / add_col / add_w [A]: the directed entries to merge, sorted by (row, col) and distinct, padded with row = n.
// The count leaves add_keep (the pair is not stored yet) and add_pre (kept entries before it in its row) for the fill.
__device__ __forceinline__ int32_t lower_bound_i32(const int32_t *__restrict__ a, int32_t lo, int32_t hi, int32_t x) {
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void insert_count_kernel(const int32_t *__restrict__ indptr,
                                                          const int32_t *__restrict__ indices, int32_t n,
                                                          const int32_t *__restrict__ add_row,
                                                          const int32_t *__restrict__ add_col, int32_t A,
                                                          int32_t *__restrict__ add_keep, int32_t *__restrict__ add_pre,
                                                          int32_t *__restrict__ row_cnt) {
    for (int32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const int32_t b = indptr[r], e = indptr[r + 1];
        const int32_t a0 = lower_bound_i32(add_row, 0, A, r), a1 = lower_bound_i32(add_row, a0, A, r + 1);
        int32_t kept = 0;
        for (int32_t a = a0; a < a1; ++a) {
            const int32_t p = lower_bound_i32(indices, b, e, add_col[a]);
            const int32_t keep = (p == e || indices[p] != add_col[a]) ? 1 : 0;
            add_keep[a] = keep;
            add_pre[a] = kept;
            kept += keep;
        }
        row_cnt[r] = e - b + kept;
    }
}

// one wave per row: a row without additions is a copy; otherwise every stored entry moves up by the kept additions
// left of it and every kept addition lands behind the stored entries left of it
__global__ __launch_bounds__(256) void insert_fill_kernel(const int32_t *__restrict__ indptr,
                                                         const int32_t *__restrict__ indices,
                                                         const float *__restrict__ data, int32_t n,
                                                         const int32_t *__restrict__ add_row,
                                                         const int32_t *__restrict__ add_col,
                                                         const float *__restrict__ add_w,
                                                         const int32_t *__restrict__ add_keep,
                                                         const int32_t *__restrict__ add_pre, int32_t A,
                                                         const int32_t *__restrict__ indptr_new,
                                                         int32_t *__restrict__ indices_out, float *__restrict__ data_out) {
    const int lane = threadIdx.x & 63;
    const int32_t r = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (r >= n) return;
    const int32_t b = indptr[r], e = indptr[r + 1], base = indptr_new[r];
    const int32_t kept_all = indptr_new[r + 1] - base - (e - b);
    const int32_t a0 = lower_bound_i32(add_row, 0, A, r), a1 = lower_bound_i32(add_row, a0, A, r + 1);
    for (int32_t i = b + lane; i < e; i += 64) {
        const int32_t c = indices[i];
        int32_t shift = 0;
        if (a1 > a0) {
            const int32_t a = lower_bound_i32(add_col, a0, a1, c);
            shift = a < a1 ? add_pre[a] : kept_all;
        }
        indices_out[base + (i - b) + shift] = c;
        data_out[base + (i - b) + shift] = data ? data[i] : 1.0f;
    }
    for (int32_t a = a0 + lane; a < a1; a += 64) {
        if (!add_keep[a]) continue;
        const int32_t p = lower_bound_i32(indices, b, e, add_col[a]);
        indices_out[base + (p - b) + add_pre[a]] = add_col[a];
        data_out[base + (p - b) + add_pre[a]] = add_w[a];
    }
}

unsigned rows_grid(int32_t n) { return (unsigned)((n + WPB - 1) / WPB); }

// The layouts of the other entry points, each measured by its query.  geo_upper_edges_count has no query of its own: it shares
// geo_connected_components' and counts into `label`.
struct CcWs { int32_t *label, *is_root, *rank, *changed; char *scan_tmp; size_t scan_bytes; };
CcWs carve_cc(geo::Arena &ar, int32_t n) {
    const size_t n1 = (size_t)n + 1;
    CcWs o;
    ar.take(o.label, n1); ar.take(o.is_root, n1); ar.take(o.rank, n1); ar.take(o.changed, 64);
    o.scan_bytes = geo::scan_tmp_bytes((int64_t)n + 1);
    ar.take(o.scan_tmp, o.scan_bytes);
    return o;
}

struct CompactWs { int32_t *flag, *pos, *row_cnt; char *scan_tmp; size_t scan_bytes; };
CompactWs carve_compact(geo::Arena &ar, int32_t n) {
    const size_t n1 = (size_t)n + 1;
    CompactWs o;
    ar.take(o.flag, n1); ar.take(o.pos, n1); ar.take(o.row_cnt, n1);
    o.scan_bytes = geo::scan_tmp_bytes((int64_t)n + 1);
    ar.take(o.scan_tmp, o.scan_bytes);
    return o;
}

struct InsertWs { int32_t *add_row, *add_col, *add_keep, *add_pre, *row_cnt; float *add_w; char *scan_tmp; size_t scan_bytes; };
InsertWs carve_insert(geo::Arena &ar, int32_t n, int64_t E) {
    const size_t A = (size_t)(2 * E + 1);
    InsertWs o;
    ar.take(o.add_row, A); ar.take(o.add_col, A); ar.take(o.add_w, A); ar.take(o.add_keep, A); ar.take(o.add_pre, A);
    ar.take(o.row_cnt, (size_t)n + 1);
    o.scan_bytes = geo::scan_tmp_bytes((int64_t)n + 1);
    ar.take(o.scan_tmp, o.scan_bytes);
    return o;
}

struct AddEntry { int32_t row, col; float w; };

// What each query answers beyond its measured layout (CC: 4096 less the `changed` block, which it used to leave to the slack).
constexpr size_t SYM_RESERVE = 4096, CC_RESERVE = 3840, COMPACT_RESERVE = 4096, INSERT_RESERVE = 4096;

}  // namespace

// ============================================================================================ ABI
extern "C" size_t geo_symmetrize_workspace_bytes(int32_t n, int32_t k) {
    if (n <= 0 || k <= 0) return 1024;
    return geo::measure(carve_sym, n, k) + SYM_RESERVE;
}

extern "C" int geo_symmetrize_count(const int32_t *nbr_idx, const float *nbr_w, int32_t n, int32_t k, int32_t mode,
                                    int32_t *indptr_out, int64_t *nnz_out, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GEO_REQUIRE(nbr_idx && indptr_out && nnz_out && ws, "geo_symmetrize_count: null pointer");
    GEO_REQUIRE(n > 0 && k > 0 && (int64_t)n * k < ((int64_t)1 << 30), "geo_symmetrize_count: bad n=%d k=%d", n, k);
    GEO_REQUIRE(mode == 0 || mode == 1, "geo_symmetrize_count: mode must be 0 (union) or 1 (mutual)");
    geo::Arena ar(ws, ws_bytes);
    const SymWs w = carve_sym(ar, n, k);
    GEO_REQUIRE_WORKSPACE("geo_symmetrize_count", ar, geo_symmetrize_workspace_bytes(n, k));
    const int64_t total = (int64_t)n * k;
    GEO_HIP_CHECK(hipMemsetAsync(w.cnt_in, 0, ((size_t)n + 1) * 4, s));
    GEO_HIP_CHECK(hipMemsetAsync(w.cursor, 0, ((size_t)n + 1) * 4, s));
    count_in_kernel<<<geo::grid_for(total, 256), 256, 0, s>>>(nbr_idx, total, n, w.cnt_in);
    GEO_LAUNCH_CHECK();
    int rc = geo::exclusive_scan_i32(w.cnt_in, w.off_in, n, w.scan_tmp, w.scan_bytes, nullptr, s);
    if (rc) return rc;
    fill_in_kernel<<<geo::grid_for(total, 256), 256, 0, s>>>(nbr_idx, nbr_w, total, n, k, w.off_in, w.cursor, w.in_src, w.in_w);
    GEO_LAUNCH_CHECK();
    sym_count_kernel<<<rows_grid(n), 256, 0, s>>>(nbr_idx, nbr_w, n, k, mode, w.off_in, w.in_src, w.in_w, w.row_cnt,
                                                  w.tmp_col, w.tmp_val);
    GEO_LAUNCH_CHECK();
    return geo::exclusive_scan_i32(w.row_cnt, indptr_out, n, w.scan_tmp, w.scan_bytes, nnz_out, s);
}

extern "C" int geo_symmetrize_fill(const int32_t *nbr_idx, const float *nbr_w, int32_t n, int32_t k, int32_t mode,
                                   const int32_t *indptr, int32_t *indices_out, float *data_out, void *ws,
                                   size_t ws_bytes, void *stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GEO_REQUIRE(nbr_idx && indptr && indices_out && data_out && ws, "geo_symmetrize_fill: null pointer");
    GEO_REQUIRE(n > 0 && k > 0 && (int64_t)n * k < ((int64_t)1 << 30), "geo_symmetrize_fill: bad n=%d k=%d", n, k);
    GEO_REQUIRE(mode == 0 || mode == 1, "geo_symmetrize_fill: mode must be 0 (union) or 1 (mutual)");
    geo::Arena ar(ws, ws_bytes);
    const SymWs w = carve_sym(ar, n, k);
    GEO_REQUIRE_WORKSPACE("geo_symmetrize_fill", ar, geo_symmetrize_workspace_bytes(n, k));
    // The workspace still holds what geo_symmetrize_count left: off_in and the rows' kept primaries at r k + off_in[r]
    // (tmp_col / tmp_val).  cnt_in and cursor are free: segment counts and their offsets.
    seg_count_kernel<<<geo::grid_for(n, 256, 1024), 256, 0, s>>>(indptr, n, w.cnt_in);
    GEO_LAUNCH_CHECK();
    if (int rc = geo::exclusive_scan_i32(w.cnt_in, w.cursor, n, w.scan_tmp, w.scan_bytes, nullptr, s)) return rc;
    const int64_t max_segs = (int64_t)n + (2 * (int64_t)n * k) / 64 + 1;          // nnz <= 2 n k (union)
    sym_sort_kernel<<<(unsigned)((max_segs + WPB - 1) / WPB), 256, 0, s>>>(n, k, indptr, w.cursor, w.off_in, w.tmp_col,
                                                                          w.tmp_val, indices_out, data_out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

extern "C" int geo_upper_edges_count(const int32_t *indptr, const int32_t *indices, int32_t n, int32_t *upper_ptr_out,
                                     int64_t *n_edges_out, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GEO_REQUIRE(indptr && indices && upper_ptr_out && n_edges_out && ws && n > 0, "geo_upper_edges_count: bad argument");
    geo::Arena ar(ws, ws_bytes);
    const CcWs w = carve_cc(ar, n);
    GEO_REQUIRE_WORKSPACE("geo_upper_edges_count", ar, geo_cc_workspace_bytes(n));
    int32_t *cnt = w.label;
    upper_count_kernel<<<geo::grid_for(n, 256), 256, 0, s>>>(indptr, indices, n, cnt);
    GEO_LAUNCH_CHECK();
    return geo::exclusive_scan_i32(cnt, upper_ptr_out, n, w.scan_tmp, w.scan_bytes, n_edges_out, s);
}

extern "C" int geo_upper_edges_fill(const int32_t *indptr, const int32_t *indices, int32_t n, const int32_t *upper_ptr,
                                    int32_t *src_out, int32_t *dst_out, int32_t *entry_edge_out, void *stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GEO_REQUIRE(indptr && indices && upper_ptr && src_out && dst_out && n > 0, "geo_upper_edges_fill: bad argument");
    upper_fill_kernel<<<rows_grid(n), 256, 0, s>>>(indptr, indices, n, upper_ptr, src_out, dst_out, entry_edge_out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

extern "C" int geo_gather_edge_weights(const float *len, const int32_t *entry_edge, int64_t nnz, float *data_out,
                                       void *stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GEO_REQUIRE(len && entry_edge && data_out && nnz >= 0, "geo_gather_edge_weights: bad argument");
    if (nnz == 0) return GEO_OK;
    gather_weights_kernel<<<geo::grid_for(nnz, 256), 256, 0, s>>>(len, entry_edge, nnz, data_out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

extern "C" size_t geo_cc_workspace_bytes(int32_t n) {
    if (n <= 0) return 1024;
    return geo::measure(carve_cc, n) + CC_RESERVE;
}

extern "C" int geo_connected_components(const int32_t *indptr, const int32_t *indices, int32_t n, int32_t *labels_out,
                                        int32_t *n_components_out, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GEO_REQUIRE(indptr && indices && labels_out && n_components_out && ws && n > 0,
                "geo_connected_components: bad argument");
    geo::Arena ar(ws, ws_bytes);
    const CcWs w = carve_cc(ar, n);
    GEO_REQUIRE_WORKSPACE("geo_connected_components", ar, geo_cc_workspace_bytes(n));
    int32_t *label = w.label, *is_root = w.is_root, *rank = w.rank, *changed = w.changed;
    const int g = geo::grid_for(n, 256, 2048);
    const int gh = geo::grid_for(n, 16, 2048);
    cc_init_kernel<<<g, 256, 0, s>>>(label, n);
    GEO_LAUNCH_CHECK();
    int32_t hchanged = 1;
    int64_t rounds = 0;
    while (hchanged) {
        GEO_HIP_CHECK(hipMemsetAsync(changed, 0, sizeof(int32_t), s));
        cc_hook_kernel<<<gh, 256, 0, s>>>(indptr, indices, n, label, changed);
        GEO_LAUNCH_CHECK();
        cc_jump_kernel<<<g, 256, 0, s>>>(label, n);
        GEO_LAUNCH_CHECK();
        GEO_HIP_CHECK(hipMemcpyAsync(&hchanged, changed, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        GEO_HIP_CHECK(hipStreamSynchronize(s));
        if (++rounds > (int64_t)n + 2) {
            geo::set_error("geo_connected_components: no fixed point after %lld rounds", (long long)rounds);
            return GEO_E_NOCONV;
        }
    }
    cc_roots_kernel<<<g, 256, 0, s>>>(label, n, is_root);
    GEO_LAUNCH_CHECK();
    int64_t ncomp = 0;
    int rc = geo::exclusive_scan_i32(is_root, rank, n, w.scan_tmp, w.scan_bytes, &ncomp, s);
    if (rc) return rc;
    cc_number_kernel<<<g, 256, 0, s>>>(label, rank, n, labels_out);
    GEO_LAUNCH_CHECK();
    GEO_HIP_CHECK(hipStreamSynchronize(s));
    *n_components_out = (int32_t)ncomp;
    return GEO_OK;
}

extern "C" size_t geo_csr_compact_workspace_bytes(int32_t n) {
    if (n <= 0) return 1024;
    return geo::measure(carve_compact, n) + COMPACT_RESERVE;
}

extern "C" int geo_csr_compact_count(const int32_t *indptr, const int32_t *indices, const float *data, int32_t n,
                                     const uint8_t *keep_node, int32_t drop_zero, int32_t *new_index_out,
                                     int32_t *indptr_out, int32_t *n_out, int64_t *nnz_out, void *ws, size_t ws_bytes,
                                     void *stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GEO_REQUIRE(indptr && indices && new_index_out && indptr_out && n_out && nnz_out && ws && n > 0,
                "geo_csr_compact_count: bad argument");
    geo::Arena ar(ws, ws_bytes);
    const CompactWs w = carve_compact(ar, n);
    GEO_REQUIRE_WORKSPACE("geo_csr_compact_count", ar, geo_csr_compact_workspace_bytes(n));
    int32_t *flag = w.flag, *pos = w.pos, *row_cnt = w.row_cnt;
    const int g = geo::grid_for(n, 256, 2048);
    keep_flags_kernel<<<g, 256, 0, s>>>(keep_node, n, flag);
    GEO_LAUNCH_CHECK();
    int64_t n_new = 0;
    int rc = geo::exclusive_scan_i32(flag, pos, n, w.scan_tmp, w.scan_bytes, &n_new, s);
    if (rc) return rc;
    new_index_kernel<<<g, 256, 0, s>>>(flag, pos, n, new_index_out);
    GEO_LAUNCH_CHECK();
    *n_out = (int32_t)n_new;
    if (n_new == 0) {
        *nnz_out = 0;
        GEO_HIP_CHECK(hipMemsetAsync(indptr_out, 0, sizeof(int32_t), s));
        return GEO_OK;
    }
    GEO_HIP_CHECK(hipMemsetAsync(row_cnt, 0, ((size_t)n + 1) * 4, s));
    compact_count_kernel<<<rows_grid(n), 256, 0, s>>>(indptr, indices, data, n, new_index_out, drop_zero, row_cnt);
    GEO_LAUNCH_CHECK();
    return geo::exclusive_scan_i32(row_cnt, indptr_out, n_new, w.scan_tmp, w.scan_bytes, nnz_out, s);
}

extern "C" int geo_csr_compact_fill(const int32_t *indptr, const int32_t *indices, const float *data, int32_t n,
                                    const uint8_t *keep_node, int32_t drop_zero, const int32_t *new_index,
                                    const int32_t *indptr_new, int32_t *indices_out, float *data_out, void *stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    (void)keep_node;
    GEO_REQUIRE(indptr && indices && new_index && indptr_new && indices_out && n > 0, "geo_csr_compact_fill: bad argument");
    compact_fill_kernel<<<rows_grid(n), 256, 0, s>>>(indptr, indices, data, n, new_index, drop_zero, indptr_new,
                                                     indices_out, data_out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

extern "C" size_t geo_csr_insert_workspace_bytes(int32_t n, int64_t E) {
    if (n <= 0 || E < 0) return 1024;
    return geo::measure(carve_insert, n, E) + INSERT_RESERVE;
}

extern "C" int geo_csr_insert_count(const int32_t *indptr, const int32_t *indices, int32_t n, const int32_t *src,
                                    const int32_t *dst, const float *w, int64_t E, int32_t *indptr_out, int64_t *nnz_out,
                                    void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GEO_REQUIRE(indptr && indices && src && dst && w && indptr_out && nnz_out && ws && n > 0, "geo_csr_insert_count: bad argument");
    GEO_REQUIRE(E >= 0 && E < ((int64_t)1 << 28), "geo_csr_insert_count: E=%lld out of range", (long long)E);
    geo::Arena ar(ws, ws_bytes);
    const InsertWs o = carve_insert(ar, n, E);
    GEO_REQUIRE_WORKSPACE("geo_csr_insert_count", ar, geo_csr_insert_workspace_bytes(n, E));
    // the edges are few: read them back, refuse a bad one before anything is launched, order both directions by (row, col)
    std::vector<int32_t> hs((size_t)E), hd((size_t)E);
    std::vector<float> hw((size_t)E);
    if (E > 0) {
        GEO_HIP_CHECK(hipMemcpyAsync(hs.data(), src, (size_t)E * 4, hipMemcpyDeviceToHost, s));
        GEO_HIP_CHECK(hipMemcpyAsync(hd.data(), dst, (size_t)E * 4, hipMemcpyDeviceToHost, s));
        GEO_HIP_CHECK(hipMemcpyAsync(hw.data(), w, (size_t)E * 4, hipMemcpyDeviceToHost, s));
        GEO_HIP_CHECK(hipStreamSynchronize(s));
    }
    for (int64_t e = 0; e < E; ++e) {
        GEO_REQUIRE(hs[e] >= 0 && hs[e] < n && hd[e] >= 0 && hd[e] < n, "geo_csr_insert_count: edge %lld (%d, %d) outside [0, %d)",
                    (long long)e, hs[e], hd[e], n);
        GEO_REQUIRE(hs[e] != hd[e], "geo_csr_insert_count: edge %lld is a self edge (%d)", (long long)e, hs[e]);
    }
    std::vector<AddEntry> add;
    add.reserve((size_t)(2 * E));
    for (int64_t e = 0; e < E; ++e) {
        add.push_back({hs[e], hd[e], hw[e]});
        add.push_back({hd[e], hs[e], hw[e]});
    }
    std::stable_sort(add.begin(), add.end(),
                     [](const AddEntry &a, const AddEntry &b) { return a.row != b.row ? a.row < b.row : a.col < b.col; });
    const size_t A = (size_t)(2 * E);
    std::vector<int32_t> hrow(A + 1, n), hcol(A + 1, 0);       // an edge listed twice counts once: the tail is padding (row n)
    std::vector<float> hww(A + 1, 0.0f);
    size_t u = 0;
    for (size_t a = 0; a < add.size(); ++a) {
        if (a > 0 && add[a].row == add[a - 1].row && add[a].col == add[a - 1].col) continue;
        hrow[u] = add[a].row; hcol[u] = add[a].col; hww[u] = add[a].w; ++u;
    }
    if (A > 0) {
        GEO_HIP_CHECK(hipMemcpyAsync(o.add_row, hrow.data(), A * 4, hipMemcpyHostToDevice, s));
        GEO_HIP_CHECK(hipMemcpyAsync(o.add_col, hcol.data(), A * 4, hipMemcpyHostToDevice, s));
        GEO_HIP_CHECK(hipMemcpyAsync(o.add_w, hww.data(), A * 4, hipMemcpyHostToDevice, s));
    }
    insert_count_kernel<<<geo::grid_for(n, 256, 2048), 256, 0, s>>>(indptr, indices, n, o.add_row, o.add_col, (int32_t)A, o.add_keep,
                                                                  o.add_pre, o.row_cnt);
    GEO_LAUNCH_CHECK();
    return geo::exclusive_scan_i32(o.row_cnt, indptr_out, n, o.scan_tmp, o.scan_bytes, nnz_out, s);   // synchronises: the host vectors may go
}

extern "C" int geo_csr_insert_fill(const int32_t *indptr, const int32_t *indices, const float *data, int32_t n, int64_t E,
                                   const int32_t *indptr_new, int32_t *indices_out, float *data_out, void *ws, size_t ws_bytes,
                                   void *stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    GEO_REQUIRE(indptr && indices && indptr_new && indices_out && data_out && ws && n > 0, "geo_csr_insert_fill: bad argument");
    GEO_REQUIRE(E >= 0 && E < ((int64_t)1 << 28), "geo_csr_insert_fill: E=%lld out of range", (long long)E);
    geo::Arena ar(ws, ws_bytes);
    const InsertWs o = carve_insert(ar, n, E);
    GEO_REQUIRE_WORKSPACE("geo_csr_insert_fill", ar, geo_csr_insert_workspace_bytes(n, E));
    insert_fill_kernel<<<rows_grid(n), 256, 0, s>>>(indptr, indices, data, n, o.add_row, o.add_col, o.add_w, o.add_keep, o.add_pre,
                                                    (int32_t)(2 * E), indptr_new, indices_out, data_out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}
