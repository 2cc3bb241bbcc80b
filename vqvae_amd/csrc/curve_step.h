// curve_step.h -- what the two curve relaxations (jvp.hip: the spatial decoder, vanilla_jvp.hip: the vanilla decoder) share: the
// state of a slice, its layout, and the accept / reject step per curve on the device.  Device code with
// internal linkage: each including file gets its own copy.
#pragma once
#include "geo_common.h"

namespace {

constexpr int CURVE_MAX_F = 64, CURVE_THREADS = 256;

// The state of a slice's relaxation, in the workspace: the trial y, and E / seg_sq / grad of the curve (cur) and of what was just
// evaluated (ev).  tr is read once, for a step the caller left to the call.
struct CurveState {
    float *y;
    double *e_ev, *e_cur, *seg_ev, *seg_cur, *grad_ev, *grad_cur, *tr;
};

// curve_step_kernel, one workgroup per curve: the decision about what was just evaluated, then the next trial.
//   first  x itself was evaluated: it becomes the state; energy0 = E; a step < 0 becomes 1 / (8 * max over interior f of tr[f]),
//          0 where that maximum is 0 (the maximum ignores a NaN, and 1 / inf is 0: such a curve never moves)
//   else   y was evaluated: E_y < E (false for a NaN on either side) accepts -- x, E, seg_sq, grad <- those of y, step *= 2,
//          accepted += 1 -- anything else rejects, step /= 4
//   last   no further trial: energy_out and seg_sq_out (may be null) take the state
//   else   y[f] = (float)((double)x[f] - step * grad[f]) for interior f, uncontracted; the ends are copied
// Every thread reads the decision's inputs before the barrier and the state is written after it.
__global__ __launch_bounds__(CURVE_THREADS) void curve_step_kernel(CurveState st, float *__restrict__ x, int F, int d, int first,
                                                                  int last, double *__restrict__ step, double *__restrict__ energy0,
                                                                  double *__restrict__ energy_out, double *__restrict__ seg_sq_out,
                                                                  int32_t *__restrict__ accepted) {
#pragma clang fp contract(off)
    const int64_t c = blockIdx.x;
    const int fd = F * d, t = threadIdx.x;
    const size_t at = (size_t)c * fd, seg_at = (size_t)c * (F - 1);
    const double e_ev = st.e_ev[c], e_cur = first ? e_ev : st.e_cur[c];
    double h = step[c];
    const bool take = first || e_ev < e_cur;
    if (first) {
        if (h < 0.0) {
            double m = 0.0;
            for (int f = 1; f < F - 1; ++f) {
                const double v = st.tr[(size_t)c * F + f];
                if (v > m) m = v;
            }
            h = m > 0.0 ? 1.0 / (8.0 * m) : 0.0;
        }
    } else {
        h = take ? 2.0 * h : h / 4.0;
    }
    __syncthreads();
    if (take) {
        for (int i = t; i < fd; i += CURVE_THREADS) {
            st.grad_cur[at + i] = st.grad_ev[at + i];
            if (!first) x[at + i] = st.y[at + i];
        }
        for (int f = t; f < F - 1; f += CURVE_THREADS) st.seg_cur[seg_at + f] = st.seg_ev[seg_at + f];
    }
    if (t == 0) {
        if (take) st.e_cur[c] = e_ev;
        step[c] = h;
        if (first) { accepted[c] = 0; if (energy0) energy0[c] = e_ev; }
        else if (take) accepted[c] += 1;
        if (last) energy_out[c] = take ? e_ev : e_cur;
    }
    __syncthreads();                                            // (the state below is this workgroup's own writes)
    if (last) {
        if (seg_sq_out)
            for (int f = t; f < F - 1; f += CURVE_THREADS) seg_sq_out[seg_at + f] = st.seg_cur[seg_at + f];
        return;
    }
    for (int i = t; i < fd; i += CURVE_THREADS) {
        const int f = i / d;
        const float xv = x[at + i];
        st.y[at + i] = f > 0 && f < F - 1 ? (float)((double)xv - h * st.grad_cur[at + i]) : xv;
    }
}

void lay_out_curves(geo::Arena &ar, CurveState *st, int64_t n_curves, int F, int d) {
    const size_t fd = (size_t)n_curves * F * d, segs = (size_t)n_curves * (F - 1);
    ar.take(st->y, fd);
    ar.take(st->e_ev, (size_t)n_curves); ar.take(st->e_cur, (size_t)n_curves);
    ar.take(st->seg_ev, segs); ar.take(st->seg_cur, segs);
    ar.take(st->grad_ev, fd); ar.take(st->grad_cur, fd);
    ar.take(st->tr, (size_t)n_curves * F);
}

}  // namespace
