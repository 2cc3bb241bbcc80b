// sym_spectrum.hip -- eigenvalues of a batch of symmetric fp64 matrices, 1 <= d <= 128, on gfx950.
//
//   geo_sym_spectrum: per matrix the eigenvalues ascending, the numerical rank and logvol = 0.5 log det, by the rules of
//   metric_spectrum_kernel (csrc/jvp.hip), which stays what the spatial decoder's d <= 16 route runs.
//
// A matrix lives whole in its workgroup's LDS for the whole iteration ([D][D + 1] doubles: 132 096 bytes at D = 128, of the
// 160 KiB a gfx950 workgroup may hold), read once from HBM -- its upper triangle a <= b only, mirrored on the way in.  The kernel
// is instantiated for D = 16, 32 (four matrices per workgroup, 64 threads each), 64 (one, 256 threads) and 128 (one, 512).
//
// Parallel-order cyclic Jacobi.  m = d rounded up to even (the extra seat is a zero row and column, which no rotation
// touches: its off-diagonal entries are exactly 0 and stay so).  A sweep is m - 1 steps of the round-robin tournament on m seats:
// step r pairs seat m - 1 with r, and (r + i) mod (m - 1) with (r - i) mod (m - 1) for i = 1 .. m / 2 - 1 -- m / 2 disjoint pairs
// (p, q), p < q, every pair once per sweep.  A step has two phases with a barrier after each:
//   1. one thread per pair: the rotation from the values before the step (the smaller root t of t^2 + 2 theta t - 1,
//      theta = (a_qq - a_pp) / (2 a_pq)), kept as (s, tau = s / (1 + c)); it rewrites its own 2 x 2 diagonal block
//      (a_pp - t a_pq, a_qq + t a_pq, 0).  An entry that is exactly 0 is skipped (s = 0); from sweep FLUSH_SWEEP on an entry
//      with |a_pp| + 100 |a_pq| == |a_pp| and the same for a_qq is set to 0 instead of rotated.
//   2. one thread per pair of pairs P < Q: the 2 x 2 block B = A[{p,q}][{u,v}] becomes J_P^T (B J_Q) -- the column update, then
//      the row update, of that block alone, which reads nothing another thread of the step writes, so the barrier between the
//      two updates of a full-matrix sweep is not needed -- and is written to both triangles: the matrix stays symmetric bit
//      for bit.  Blocks whose two rotations are both skipped are left alone.
// The sweeps end when every off-diagonal entry is exactly 0, or after SWEEP_CAP sweeps.  Everything is a function of the
// matrix alone: a matrix that shares a workgroup with others takes the barriers of their sweeps but no rotation of its own
// once it has converged.  A matrix with a NaN or an inf among the entries read is never iterated: eig NaN, logvol NaN, rank 0;
// the same results for a matrix whose diagonal is not finite when the sweeps end.
#include "geo_common.h"

#include <cfloat>
#include <cmath>

namespace {

constexpr int SPEC_MAX_D = 128;
constexpr int SWEEP_CAP = 64;       // sweeps at most (the most any test matrix or decoder metric took: DESIGN.md section 30)
constexpr int FLUSH_SWEEP = 4;      // from this sweep on (0-based) a negligible entry is set to 0

__device__ __forceinline__ bool finite64(double v) {
    return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll;
}

template <int D, int M, int T>
__global__ __launch_bounds__(M * T) void sym_spectrum_kernel(const double *__restrict__ G, int64_t n, int d, int p_out,
                                                             double *__restrict__ eig_out, double *__restrict__ logvol_out,
                                                             int32_t *__restrict__ rank_out, int32_t *__restrict__ sweeps_out) {
    constexpr int LD = D + 1, NP = D / 2;
    __shared__ double A_s[M][D * LD];
    __shared__ double rs_s[M][NP], rt_s[M][NP];          // a step's rotations: sin and tau, s == 0: none
    __shared__ int pp_s[M][NP], qq_s[M][NP];             // and their seats p < q
    __shared__ double diag_s[M][D], sorted_s[M][D];
    __shared__ int bad_s[M], nz_s[M];
    const int g = threadIdx.x / T, t = threadIdx.x % T;
    const int64_t mat = (int64_t)blockIdx.x * M + g;
    const bool present = mat < n;
    double *A = A_s[g];
    const int m = (d + 1) & ~1, np = m / 2;

    if (t == 0) bad_s[g] = 0;
    __syncthreads();
    {
        const double *Gm = G + (size_t)(present ? mat : 0) * d * d;
        bool bad = false;
        for (int i = t; i < m * m; i += T) {
            const int r = i / m, c = i - r * m;
            double v = 0.0;
            if (present && r < d && c < d) v = r <= c ? Gm[(size_t)r * d + c] : Gm[(size_t)c * d + r];
            bad |= !finite64(v);
            A[r * LD + c] = v;
        }
        if (bad) bad_s[g] = 1;
    }
    __syncthreads();
    const bool live = present && !bad_s[g];

    int sweeps = 0;
    for (int sweep = 0; sweep < SWEEP_CAP; ++sweep) {
        if (t == 0) nz_s[g] = 0;
        __syncthreads();
        if (live) {
            bool nz = false;
            for (int i = t; i < m * m; i += T) {
                const int r = i / m, c = i - r * m;
                if (c > r) nz |= A[r * LD + c] != 0.0;
            }
            if (nz) nz_s[g] = 1;
        }
        __syncthreads();
        bool any = false;
#pragma unroll
        for (int k = 0; k < M; ++k) any |= nz_s[k] != 0;
        if (!any) break;                                   // (the same for every thread of the workgroup)
        const bool active = live && nz_s[g] != 0;
        if (active) ++sweeps;
        for (int r = 0; r < m - 1; ++r) {
            if (active && t < np) {
                int a = m - 1, b = r;
                if (t > 0) {
                    a = (r + t) % (m - 1);
                    b = (r - t + (m - 1)) % (m - 1);
                }
                const int p = a < b ? a : b, q = a < b ? b : a;
                const double apq = A[p * LD + q];
                double s = 0.0, tau = 0.0;
                if (apq != 0.0) {
                    const double app = A[p * LD + p], aqq = A[q * LD + q], gg = 100.0 * fabs(apq);
                    if (sweep >= FLUSH_SWEEP && fabs(app) + gg == fabs(app) && fabs(aqq) + gg == fabs(aqq)) {
                        A[p * LD + q] = 0.0;
                        A[q * LD + p] = 0.0;
                    } else {
                        const double h = aqq - app;
                        double tn;                          // tan of the rotation angle, the smaller root
                        if (fabs(h) + gg == fabs(h)) tn = apq / h;
                        else {
                            const double theta = 0.5 * h / apq;
                            tn = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                            if (theta < 0.0) tn = -tn;
                        }
                        const double c = 1.0 / sqrt(tn * tn + 1.0);
                        s = tn * c;
                        tau = s / (1.0 + c);
                        A[p * LD + p] = app - tn * apq;
                        A[q * LD + q] = aqq + tn * apq;
                        A[p * LD + q] = 0.0;
                        A[q * LD + p] = 0.0;
                    }
                }
                pp_s[g][t] = p;
                qq_s[g][t] = q;
                rs_s[g][t] = s;
                rt_s[g][t] = tau;
            }
            __syncthreads();
            if (active && np > 1) {
                // the pairs of pairs P < Q as a rectangle: row i holds row i of the strict upper triangle and then row np - 1 - i
                const int W = np - 1, H = (np + 1) / 2;
                for (int w = t; w < H * W; w += T) {
                    const int i = w / W, j = w - i * W;
                    int P, Q;
                    if (j < W - i) {
                        P = i;
                        Q = i + 1 + j;
                    } else {
                        if (W - i == i) continue;           // np odd: the middle row has no second half
                        P = W - i;
                        Q = P + 1 + (j - (W - i));
                    }
                    const double sP = rs_s[g][P], sQ = rs_s[g][Q];
                    if (sP == 0.0 && sQ == 0.0) continue;
                    const double tP = rt_s[g][P], tQ = rt_s[g][Q];
                    const int p = pp_s[g][P], q = qq_s[g][P], u = pp_s[g][Q], v = qq_s[g][Q];
                    const double b00 = A[p * LD + u], b01 = A[p * LD + v], b10 = A[q * LD + u], b11 = A[q * LD + v];
                    const double x00 = b00 - sQ * (b01 + b00 * tQ), x01 = b01 + sQ * (b00 - b01 * tQ);
                    const double x10 = b10 - sQ * (b11 + b10 * tQ), x11 = b11 + sQ * (b10 - b11 * tQ);
                    const double y00 = x00 - sP * (x10 + x00 * tP), y10 = x10 + sP * (x00 - x10 * tP);
                    const double y01 = x01 - sP * (x11 + x01 * tP), y11 = x11 + sP * (x01 - x11 * tP);
                    A[p * LD + u] = y00; A[u * LD + p] = y00;
                    A[p * LD + v] = y01; A[v * LD + p] = y01;
                    A[q * LD + u] = y10; A[u * LD + q] = y10;
                    A[q * LD + v] = y11; A[v * LD + q] = y11;
                }
            }
            __syncthreads();
        }
    }

    // the diagonal, sorted ascending by counting (ties in index order).  A value that is not finite here (finite entries near
    // DBL_MAX can overflow in a rotation) would leave slots of the sort unwritten: such a matrix takes the NaN / NaN / 0 exit too.
    if (live)
        for (int i = t; i < d; i += T) {
            const double v = A[i * LD + i];
            diag_s[g][i] = v;
            if (!finite64(v)) bad_s[g] = 1;
        }
    __syncthreads();
    const bool ok = live && !bad_s[g];
    if (ok)
        for (int i = t; i < d; i += T) {
            const double v = diag_s[g][i];
            int pos = 0;
            for (int j = 0; j < d; ++j) {
                const double e = diag_s[g][j];
                pos += (e < v || (e == v && j < i)) ? 1 : 0;
            }
            sorted_s[g][pos] = v;
        }
    __syncthreads();
    if (!present) return;
    for (int i = t; i < d; i += T) eig_out[(size_t)mat * d + i] = ok ? sorted_s[g][i] : (double)NAN;
    if (t != 0) return;
    if (sweeps_out) sweeps_out[mat] = sweeps;
    if (!ok) {
        logvol_out[mat] = (double)NAN;
        rank_out[mat] = 0;
        return;
    }
    const double emax = sorted_s[g][d - 1];
    const double tol = (double)(p_out > d ? p_out : d) * (double)FLT_EPSILON * (emax > 0.0 ? sqrt(emax) : 0.0);
    int rank = 0;
    bool positive = true;
    double logdet = 0.0;
    for (int i = 0; i < d; ++i) {
        const double e = sorted_s[g][i];
        if (e > 0.0) { logdet += log(e); if (sqrt(e) > tol) ++rank; }
        else positive = false;
    }
    rank_out[mat] = rank;
    logvol_out[mat] = positive ? 0.5 * logdet : -(double)INFINITY;
}

int spectrum(const char *who, const double *G, int64_t n, int d, int p_out, double *eig_out, double *logvol_out, int32_t *rank_out,
             int32_t *sweeps_out, hipStream_t st) {
    GEO_REQUIRE(d >= 1 && d <= SPEC_MAX_D, "%s: d %d not in [1,%d]", who, d, SPEC_MAX_D);
    GEO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "%s: n %lld", who, (long long)n);
    GEO_REQUIRE(p_out >= 1, "%s: p_out %d < 1", who, p_out);
    if (n == 0) return GEO_OK;
    GEO_REQUIRE(G && eig_out && logvol_out && rank_out, "%s: null pointer", who);
#define SPEC_LAUNCH(D_, M_, T_)                                                                                                \
    sym_spectrum_kernel<D_, M_, T_><<<(unsigned)((n + M_ - 1) / M_), M_ * T_, 0, st>>>(G, n, d, p_out, eig_out, logvol_out,      \
                                                                                      rank_out, sweeps_out)
    if (d <= 16) SPEC_LAUNCH(16, 4, 64);
    else if (d <= 32) SPEC_LAUNCH(32, 4, 64);
    else if (d <= 64) SPEC_LAUNCH(64, 1, 256);
    else SPEC_LAUNCH(128, 1, 512);
#undef SPEC_LAUNCH
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

}  // namespace

extern "C" int geo_sym_spectrum(const double *G, int64_t n, int32_t d, int32_t p_out, double *eig_out, double *logvol_out,
                                int32_t *rank_out, void *stream) {
    return spectrum("geo_sym_spectrum", G, n, d, p_out, eig_out, logvol_out, rank_out, nullptr, static_cast<hipStream_t>(stream));
}

extern "C" int geo_sym_spectrum_sweeps(const double *G, int64_t n, int32_t d, int32_t p_out, double *eig_out, double *logvol_out,
                                       int32_t *rank_out, int32_t *sweeps_out, void *stream) {
    GEO_REQUIRE(n == 0 || sweeps_out, "geo_sym_spectrum_sweeps: null pointer");
    return spectrum("geo_sym_spectrum_sweeps", G, n, d, p_out, eig_out, logvol_out, rank_out, sweeps_out,
                    static_cast<hipStream_t>(stream));
}

extern "C" int32_t geo_sym_spectrum_sweep_cap(void) { return SWEEP_CAP; }
