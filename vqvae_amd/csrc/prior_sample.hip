// prior_sample.hip -- KV-cached autoregressive sampling from the code prior (gfx950).
//
// The reference samples (src/scripts/generate_samples.py:19-31) by re-running the WHOLE forward on the growing prefix at
// every step: 15 forwards of the 4-layer model for a 16-token sequence, each ~70 torch launches, plus topk / softmax /
// multinomial / cat.  Here every position is computed once.  A "round" advances all B rows by one position t:
//
//   per layer  ps_linear<QKV>    LN1 + c_attn; q of position t to a scratch row, k and v into the KV cache at t
//              ps_attention      position t against cache positions <= t (one wave per (row, head))
//              ps_linear<RESID>  c_proj + bias + residual into x
//              ps_linear<GELU>   LN2 + mlp.0 + bias + exact erf GELU
//              ps_linear<RESID>  mlp.2 + bias + residual into x
//   then       ps_linear<PLAIN>  LN_f + head (no bias) -> logits [B][V]
//              ps_draw           one workgroup per row: temperature, top-k, softmax, inverse-CDF pick of token t+1 (or the
//                                prompt's token while t+1 is still prompt), and the embedding of position t+1 for the next round
//
// ps_linear tiles 16 rows x 64 output columns per workgroup: with B = 100 the work spreads over column slices, with B in the
// thousands over row tiles, and each weight matrix is read about once per round.  f32 throughout with fmaf accumulation
// (greedy parity with the reference needs f32 logits).  f32-input MFMA runs at the same per-clock rate as the f32 VALU on
// gfx950, and at B = 100 each projection is bound by the latency of its few workgroups' weight loads, not by arithmetic,
// so the projections use the VALU (DESIGN.md "Sampling from the prior" has the measured table).
//
// No inter-workgroup synchronisation, no allocation, no process-global state: concurrent calls on different streams with
// different workspaces are independent.
#include "geo_common.h"

#include <cfloat>
#include <climits>
#include <cmath>

namespace {

constexpr int PS_MAX_T = 16;      // positions (max_seq_len) covered
constexpr int PS_MAX_V = 1024;    // vocabulary covered: 4 logits per thread of a 256-thread draw workgroup
constexpr int PS_MAX_C = 512;
constexpr int LR = 16, LNC = 64;     // ps_linear tile: rows x output columns

enum { EPI_QKV = 0, EPI_RESID = 1, EPI_GELU = 2, EPI_PLAIN = 3 };

struct LinArgs {
    const float *in;                 // [B][K]
    const float *ln_w, *ln_b;        // LayerNorm over K applied to `in` first (both null: none)
    const float *W, *bias;           // W [N][K] (torch Linear), bias [N] or null
    float *out;                      // RESID: out[b][n] += ..., GELU / PLAIN: out [B][N]
    float *q, *kc, *vc;              // QKV: q [B][C]; kc / vc [B][S][C], position t
    int B, K, N, C, S, t;
};

__device__ inline float wave_sum(float v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ inline float wave_max(float v) {
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// out = epilogue(LN?(in) @ W^T + bias).  grid (ceil(B / LR), ceil(N / LNC)), 256 threads: thread (tx, ty) owns output column
// n0 + tx of rows r0 + 4 ty .. + 3.  K is a multiple of LK (embed_dim a multiple of 64, LK = 64 or 128 divides it; the host
// picks).  At B = 100 each launch is a few workgroups per CU's worth of latency-bound loads: the next k chunk is loaded into
// registers while the current one is multiplied out of LDS, and the LayerNorm statistics take one pass over the row.
template <int EPI, int LK>
__global__ __launch_bounds__(256) void ps_linear_kernel(LinArgs a) {
    constexpr int XQ = LR * LK / 4 / 256, WQ = LNC * LK / 4 / 256, KQ = LK / 4;    // float4 per thread per chunk
    __shared__ float xs[LR][LK + 4];
    __shared__ float wsm[LK][LNC + 1];
    __shared__ float s_mean[LR], s_rstd[LR];
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    const int r0 = blockIdx.x * LR, n0 = blockIdx.y * LNC;
    const int K = a.K;
    const bool ln = a.ln_w != nullptr;
    float4 px[XQ], pw[WQ];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < XQ; ++i) {
            const int idx = tid + i * 256, r = idx / KQ, kq = (idx % KQ) * 4, b = r0 + r;
            px[i] = b < a.B ? *reinterpret_cast<const float4 *>(a.in + (size_t)b * K + k0 + kq) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < WQ; ++i) {
            const int idx = tid + i * 256, n = idx / KQ, kq = (idx % KQ) * 4;
            pw[i] = n0 + n < a.N ? *reinterpret_cast<const float4 *>(a.W + (size_t)(n0 + n) * K + k0 + kq)
                                 : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    load(0);
    if (ln) {                                          // mean / biased variance per row, eps 1e-5 (F.layer_norm); K <= 512
        float v[4][PS_MAX_C / 64];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int b = r0 + ty * 4 + rr;
#pragma unroll
            for (int j = 0; j < PS_MAX_C / 64; ++j) {
                const int k = tx + 64 * j;
                v[rr][j] = (b < a.B && k < K) ? a.in[(size_t)b * K + k] : 0.f;
            }
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < PS_MAX_C / 64; ++j) s += v[rr][j];
            const float mean = wave_sum(s) / (float)K;
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < PS_MAX_C / 64; ++j) {
                const float d = tx + 64 * j < K ? v[rr][j] - mean : 0.f;
                ss = fmaf(d, d, ss);
            }
            const float rstd = rsqrtf(wave_sum(ss) / (float)K + 1e-5f);
            if (tx == 0) { s_mean[ty * 4 + rr] = mean; s_rstd[ty * 4 + rr] = rstd; }
        }
        __syncthreads();
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += LK) {
#pragma unroll
        for (int i = 0; i < XQ; ++i) {
            const int idx = tid + i * 256, r = idx / KQ, kq = (idx % KQ) * 4;
            float4 v = px[i];
            if (ln && r0 + r < a.B) {
                const float m = s_mean[r], rs = s_rstd[r];
                const float *g = a.ln_w + k0 + kq, *be = a.ln_b + k0 + kq;
                v.x = (v.x - m) * rs * g[0] + be[0];
                v.y = (v.y - m) * rs * g[1] + be[1];
                v.z = (v.z - m) * rs * g[2] + be[2];
                v.w = (v.w - m) * rs * g[3] + be[3];
            }
            *reinterpret_cast<float4 *>(&xs[r][kq]) = v;
        }
#pragma unroll
        for (int i = 0; i < WQ; ++i) {   // stored transposed: wsm[k][n]
            const int idx = tid + i * 256, n = idx / KQ, kq = (idx % KQ) * 4;
            wsm[kq][n] = pw[i].x;
            wsm[kq + 1][n] = pw[i].y;
            wsm[kq + 2][n] = pw[i].z;
            wsm[kq + 3][n] = pw[i].w;
        }
        __syncthreads();
        if (k0 + LK < K) load(k0 + LK);                 // in flight while this chunk is multiplied
#pragma unroll 4
        for (int k = 0; k < LK; k += 4) {
            const float w0 = wsm[k][tx], w1 = wsm[k + 1][tx], w2 = wsm[k + 2][tx], w3 = wsm[k + 3][tx];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const float4 xv = *reinterpret_cast<const float4 *>(&xs[ty * 4 + rr][k]);
                float s = acc[rr];
                s = fmaf(xv.x, w0, s);
                s = fmaf(xv.y, w1, s);
                s = fmaf(xv.z, w2, s);
                s = fmaf(xv.w, w3, s);
                acc[rr] = s;
            }
        }
        __syncthreads();
    }
    const int n = n0 + tx;
    if (n >= a.N) return;
    const float bias = a.bias ? a.bias[n] : 0.f;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int b = r0 + ty * 4 + rr;
        if (b >= a.B) break;
        const float v = acc[rr] + bias;
        if (EPI == EPI_QKV) {
            const int C = a.C;
            if (n < C) a.q[(size_t)b * C + n] = v;
            else if (n < 2 * C) a.kc[((size_t)b * a.S + a.t) * C + (n - C)] = v;
            else a.vc[((size_t)b * a.S + a.t) * C + (n - 2 * C)] = v;
        } else if (EPI == EPI_RESID) {
            float *o = a.out + (size_t)b * a.N + n;
            *o = *o + v;
        } else if (EPI == EPI_GELU) {
            a.out[(size_t)b * a.N + n] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
        } else {
            a.out[(size_t)b * a.N + n] = v;
        }
    }
}

// Context of position t: one wave per (row, head); lane j <= t scores key j, lane l < HD sums the values of column l.
template <int HD>
__global__ __launch_bounds__(256) void ps_attention_kernel(const float *__restrict__ q, const float *__restrict__ kc,
                                                           const float *__restrict__ vc, int B, int H, int S, int t, float scale,
                                                           float *__restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int bh = blockIdx.x * 4 + wave;
    if (bh >= B * H) return;
    const int b = bh / H, h = bh % H, C = H * HD;
    const float *qr = q + (size_t)b * C + h * HD;
    float s = -INFINITY;
    if (lane <= t) {
        const float *kr = kc + ((size_t)b * S + lane) * C + h * HD;
        float d = 0.f;
#pragma unroll 8
        for (int l = 0; l < HD; ++l) d = fmaf(qr[l], kr[l], d);
        s = d * scale;
    }
    const float m = wave_max(s);
    const float e = lane <= t ? expf(s - m) : 0.f;
    const float p = e * (1.0f / wave_sum(e));
    float acc = 0.f;
    for (int j = 0; j <= t; ++j) {
        const float pj = __shfl(p, j, 64);
        if (lane < HD) acc = fmaf(pj, vc[((size_t)b * S + j) * C + h * HD + lane], acc);
    }
    if (lane < HD) out[(size_t)b * C + h * HD + lane] = acc;
}

struct EmbArgs {
    const float *tok, *pos, *cls;    // token_emb [V][C], pos_emb [T][C], class_emb [num_classes][C] or null
    const int64_t *y;                // [B] or null
    int V, C, num_classes;
};

__device__ inline void embed_row(const EmbArgs &e, int b, int64_t token, int pos, float *x) {
    const int64_t tk = token < 0 ? 0 : (token >= e.V ? e.V - 1 : token);        // (the host validates; never index out of range)
    int64_t yc = 0;
    if (e.cls) { yc = e.y[b]; yc = yc < 0 ? 0 : (yc >= e.num_classes ? e.num_classes - 1 : yc); }
    for (int c = threadIdx.x; c < e.C; c += blockDim.x) {
        float v = e.tok[tk * e.C + c] + e.pos[(size_t)pos * e.C + c];             // (tok + pos) + cls, the reference's order
        if (e.cls) v = v + e.cls[yc * e.C + c];
        x[(size_t)b * e.C + c] = v;
    }
}

// Position 0: the prompt into tokens_out and the embedding of its first token into x.  Grid B.
__global__ __launch_bounds__(256) void ps_init_kernel(EmbArgs e, const int64_t *__restrict__ prompt, int T0, int T_total,
                                                      int64_t *__restrict__ tokens_out, float *__restrict__ x) {
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < T0; i += blockDim.x) tokens_out[(size_t)b * T_total + i] = prompt[(size_t)b * T0 + i];
    embed_row(e, b, prompt[(size_t)b * T0], 0, x);
}

struct DrawArgs {
    const float *logits;             // [B][V] (unused while t + 1 is prompt and no logits are requested)
    float *logits_out;               // [B][T_total - 1][V] or null
    const int64_t *prompt;           // [B][T0]
    const float *uniforms;           // [B][T_total - T0]
    int64_t *tokens_out;             // [B][T_total]
    float *x;                        // [B][C]: embedding of position t + 1 when build_next
    float temperature;
    int top_k, t, T0, T_total, build_next, have_logits;
    EmbArgs e;
};

__device__ inline uint32_t order_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Token t + 1 of row blockIdx.x.  Draw rule (shared with vqvae_amd/prior/sampling.py:draw_rule):
//   l = logits / temperature;  with top_k, keep every i with l_i >= (k-th largest l) -- ties at the k-th value all kept;
//   p_i = exp(l_i - max l) over kept i;  token = smallest i whose inclusive prefix sum exceeds u * sum(p), else the last
//   kept index.  Thread tid owns indices 4 tid .. 4 tid + 3, so the prefix runs in index order.
__global__ __launch_bounds__(256) void ps_draw_kernel(DrawArgs a, int V) {
    __shared__ float s_red[4];
    __shared__ unsigned s_hist[256];
    __shared__ uint32_t s_prefix;
    __shared__ int s_remaining;
    __shared__ int s_first, s_last;
    __shared__ int64_t s_tok;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool prompt_next = a.t + 1 < a.T0;
    if (a.have_logits && a.logits_out)
        for (int i = tid; i < V; i += 256)
            a.logits_out[((size_t)b * (a.T_total - 1) + a.t) * V + i] = a.logits[(size_t)b * V + i];
    if (prompt_next) {
        if (tid == 0) s_tok = a.prompt[(size_t)b * a.T0 + a.t + 1];
    } else {
        float l[4];
        bool valid[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = tid * 4 + e;
            valid[e] = i < V;
            l[e] = valid[e] ? a.logits[(size_t)b * V + i] / a.temperature : -INFINITY;
        }
        // max
        float m = wave_max(fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3])));
        if (lane == 0) s_red[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
        // k-th largest by radix select on order-preserving keys, 8 bits per pass
        float thr = -INFINITY;
        if (a.top_k > 0 && a.top_k < V) {
            uint32_t key[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) key[e] = order_key(l[e]);
            if (tid == 0) { s_prefix = 0u; s_remaining = a.top_k; }
            uint32_t mask = 0u;
            for (int shift = 24; shift >= 0; shift -= 8) {
                s_hist[tid] = 0u;
                __syncthreads();
                const uint32_t prefix = s_prefix;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (valid[e] && (key[e] & mask) == prefix) atomicAdd(&s_hist[(key[e] >> shift) & 255u], 1u);
                __syncthreads();
                if (wave == 0) {              // bins from the top: lane owns 4 lane .. 4 lane + 3, suffix counts across lanes
                    const int remaining = s_remaining;
                    unsigned h[4], own = 0u;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { h[j] = s_hist[4 * lane + j]; own += h[j]; }
                    unsigned suf = own;
                    for (int off = 1; off < 64; off <<= 1) {
                        const unsigned o = __shfl_down(suf, off, 64);
                        if (lane + off < 64) suf += o;
                    }
                    unsigned above = suf - own;          // keys in bins above this lane's four
                    for (int j = 3; j >= 0; --j) {
                        if (above < (unsigned)remaining && above + h[j] >= (unsigned)remaining) {
                            s_prefix = prefix | ((uint32_t)(4 * lane + j) << shift);
                            s_remaining = remaining - (int)above;
                        }
                        above += h[j];
                    }
                }
                mask |= 255u << shift;
                __syncthreads();
            }
            thr = key_float(s_prefix);
        }
        float p[4], c[4];
        float run = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool keep = valid[e] && l[e] >= thr;
            p[e] = keep ? expf(l[e] - m) : 0.f;
            run += p[e];
            c[e] = run;
        }
        // block exclusive scan of the per-thread sums
        float incl = run;
        for (int off = 1; off < 64; off <<= 1) {
            const float o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        __syncthreads();                                 // (s_red reused)
        if (lane == 63) s_red[wave] = incl;
        if (tid == 0) { s_first = INT_MAX; s_last = -1; }
        __syncthreads();
        float base = incl - run;
        for (int w = 0; w < wave; ++w) base += s_red[w];
        const float S = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
        const float u = a.uniforms[(size_t)b * (a.T_total - a.T0) + (a.t + 1 - a.T0)];
        const float target = u * S;
        int first = INT_MAX, last = -1;
#pragma unroll
        for (int e = 3; e >= 0; --e) {
            if (valid[e] && l[e] >= thr) {
                if (last < 0) last = tid * 4 + e;
                if (base + c[e] > target) first = tid * 4 + e;
            }
        }
        if (first != INT_MAX) atomicMin(&s_first, first);
        if (last >= 0) atomicMax(&s_last, last);
        __syncthreads();
        if (tid == 0) s_tok = s_first != INT_MAX ? s_first : s_last;
    }
    __syncthreads();
    const int64_t tok = s_tok;
    if (tid == 0) a.tokens_out[(size_t)b * a.T_total + a.t + 1] = tok;
    if (a.build_next) embed_row(a.e, b, tok, a.t + 1, a.x);
}

struct Plan { float *kv, *x, *q, *att, *hid, *logits; };

// geo_prior_sample's workspace for B rows and S cached positions: measured by geo_prior_sample_workspace_bytes.
Plan lay_out(geo::Arena &ar, const geo_prior_desc *d, int B, int S) {
    const size_t C = d->embed_dim;
    Plan p;
    ar.take(p.kv, (size_t)d->n_layers * 2 * B * S * C);
    ar.take(p.x, (size_t)B * C);
    ar.take(p.q, (size_t)B * C);
    ar.take(p.att, (size_t)B * C);
    ar.take(p.hid, (size_t)B * 4 * C);
    ar.take(p.logits, (size_t)B * d->num_tokens);
    return p;
}

template <int EPI>
void launch_linear(const LinArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.B + LR - 1) / LR), (unsigned)((a.N + LNC - 1) / LNC));
    if (a.K % 128 == 0) ps_linear_kernel<EPI, 128><<<grid, 256, 0, stream>>>(a);
    else ps_linear_kernel<EPI, 64><<<grid, 256, 0, stream>>>(a);
}

int check_desc(const geo_prior_desc *d, const char *fn) {
    GEO_REQUIRE(d && d->arena, "%s: null descriptor or arena", fn);
    GEO_REQUIRE(d->n_layers >= 1 && d->n_head >= 1 && d->embed_dim % d->n_head == 0, "%s: n_layers %d n_head %d embed_dim %d",
                fn, d->n_layers, d->n_head, d->embed_dim);
    const int hd = d->embed_dim / d->n_head;
    GEO_REQUIRE(hd == 16 || hd == 32 || hd == 64, "%s: head_dim %d not in {16, 32, 64}", fn, hd);
    GEO_REQUIRE(d->embed_dim % 64 == 0 && d->embed_dim <= PS_MAX_C, "%s: embed_dim %d (a multiple of 64, <= %d)", fn,
                d->embed_dim, PS_MAX_C);
    GEO_REQUIRE(d->num_tokens >= 1 && d->num_tokens <= PS_MAX_V, "%s: num_tokens %d (<= %d)", fn, d->num_tokens, PS_MAX_V);
    GEO_REQUIRE(d->max_seq_len >= 1 && d->max_seq_len <= PS_MAX_T, "%s: max_seq_len %d (<= %d)", fn, d->max_seq_len, PS_MAX_T);
    GEO_REQUIRE(d->num_classes >= 0 && (d->num_classes == 0 || d->class_emb >= 0), "%s: class embedding missing", fn);
    GEO_REQUIRE(d->block, "%s: null block offsets", fn);
    // every matrix row is read as float4: the tensors must start on 16 bytes
    GEO_REQUIRE(((uintptr_t)d->arena) % 16 == 0 && d->head_w % 4 == 0, "%s: arena or head not 16-byte aligned", fn);
    for (int i = 0; i < d->n_layers; ++i)
        for (int j : {4, 6, 8, 10})
            GEO_REQUIRE(d->block[i * 12 + j] % 4 == 0 && d->block[i * 12 + j] >= 0, "%s: block %d weight %d not 16-byte aligned",
                        fn, i, j);
    return GEO_OK;
}

}  // namespace

extern "C" size_t geo_prior_sample_workspace_bytes(const geo_prior_desc *d, int32_t B, int32_t n_positions) {
    if (!d || B < 1 || n_positions < 1) return 0;
    return geo::measure(lay_out, d, B, n_positions);
}

extern "C" int geo_prior_sample(const geo_prior_desc *d, const int64_t *prompt, int32_t T0, int32_t steps, const int64_t *y,
                                const float *uniforms, float temperature, int32_t top_k, int64_t *tokens_out, float *logits_out,
                                int32_t B, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int st = check_desc(d, "geo_prior_sample")) return st;
    GEO_REQUIRE(prompt && tokens_out, "geo_prior_sample: null prompt or tokens_out");
    GEO_REQUIRE(B >= 1 && B <= (1 << 24), "geo_prior_sample: B=%d", B);
    GEO_REQUIRE(T0 >= 1 && steps >= 0 && T0 + steps - 1 <= d->max_seq_len,
                "geo_prior_sample: T0=%d steps=%d (T0 + steps - 1 <= max_seq_len %d)", T0, steps, d->max_seq_len);
    GEO_REQUIRE(steps == 0 || uniforms, "geo_prior_sample: null uniforms");
    GEO_REQUIRE(std::isfinite(temperature) && temperature > 0.f, "geo_prior_sample: temperature %g", (double)temperature);
    GEO_REQUIRE(top_k >= 0 && top_k <= d->num_tokens, "geo_prior_sample: top_k %d (0..%d)", top_k, d->num_tokens);
    GEO_REQUIRE(!y || d->num_classes > 0, "geo_prior_sample: labels given to an unconditional model");
    const int T_total = T0 + steps, rounds = T_total - 1;
    const int C = d->embed_dim, H = d->n_head, V = d->num_tokens, hd = C / H;
    const int S = rounds > 0 ? rounds : 1;
    GEO_REQUIRE(ws && ((uintptr_t)ws) % 256 == 0, "geo_prior_sample: workspace null or not 256-byte aligned");
    geo::Arena ar(ws, ws_bytes);
    const Plan p = lay_out(ar, d, B, S);
    GEO_REQUIRE_WORKSPACE("geo_prior_sample", ar, ar.off);
    const float *A = d->arena;
    EmbArgs e{A + d->token_emb, A + d->pos_emb, y ? A + d->class_emb : nullptr, y, V, C, d->num_classes};
    ps_init_kernel<<<B, 256, 0, stream>>>(e, prompt, T0, T_total, tokens_out, p.x);
    GEO_LAUNCH_CHECK();
    const float scale = 1.0f / sqrtf((float)hd);
    const size_t layer_kv = (size_t)B * S * C;
    for (int t = 0; t < rounds; ++t) {
        for (int i = 0; i < d->n_layers; ++i) {
            const int64_t *o = d->block + i * 12;
            float *kc = p.kv + (size_t)i * 2 * layer_kv, *vc = kc + layer_kv;
            LinArgs a{};
            a.B = B; a.C = C; a.S = S; a.t = t;
            a.in = p.x; a.K = C; a.ln_w = A + o[0]; a.ln_b = A + o[1]; a.W = A + o[4]; a.bias = A + o[5]; a.N = 3 * C;
            a.q = p.q; a.kc = kc; a.vc = vc;
            launch_linear<EPI_QKV>(a, stream);
            const unsigned agrid = (unsigned)((B * H + 3) / 4);
            switch (hd) {
                case 16: ps_attention_kernel<16><<<agrid, 256, 0, stream>>>(p.q, kc, vc, B, H, S, t, scale, p.att); break;
                case 32: ps_attention_kernel<32><<<agrid, 256, 0, stream>>>(p.q, kc, vc, B, H, S, t, scale, p.att); break;
                default: ps_attention_kernel<64><<<agrid, 256, 0, stream>>>(p.q, kc, vc, B, H, S, t, scale, p.att); break;
            }
            a = LinArgs{};
            a.B = B; a.C = C;
            a.in = p.att; a.K = C; a.W = A + o[6]; a.bias = A + o[7]; a.N = C; a.out = p.x;
            launch_linear<EPI_RESID>(a, stream);
            a.in = p.x; a.K = C; a.ln_w = A + o[2]; a.ln_b = A + o[3]; a.W = A + o[8]; a.bias = A + o[9]; a.N = 4 * C; a.out = p.hid;
            launch_linear<EPI_GELU>(a, stream);
            a.in = p.hid; a.K = 4 * C; a.ln_w = a.ln_b = nullptr; a.W = A + o[10]; a.bias = A + o[11]; a.N = C; a.out = p.x;
            launch_linear<EPI_RESID>(a, stream);
        }
        const bool have_logits = t + 1 >= T0 || logits_out;
        if (have_logits) {
            LinArgs a{};
            a.B = B; a.C = C;
            a.in = p.x; a.K = C; a.ln_w = A + d->ln_f_w; a.ln_b = A + d->ln_f_b; a.W = A + d->head_w; a.N = V; a.out = p.logits;
            launch_linear<EPI_PLAIN>(a, stream);
        }
        DrawArgs da{};
        da.logits = p.logits; da.logits_out = logits_out; da.prompt = prompt; da.uniforms = uniforms; da.tokens_out = tokens_out;
        da.x = p.x; da.temperature = temperature; da.top_k = top_k; da.t = t; da.T0 = T0; da.T_total = T_total;
        da.build_next = t + 1 < rounds; da.have_logits = have_logits; da.e = e;
        ps_draw_kernel<<<B, 256, 0, stream>>>(da, V);
        GEO_LAUNCH_CHECK();
    }
    return GEO_OK;
}
