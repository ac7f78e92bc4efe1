// The Langevin corrector of predictor-corrector sampling (pp_sample_corrected; the reference's
// SO2VESchedule.step_correct, schedule.py:238-273, with a step size per complex instead of one per batch).
//
// k_correct: ONE workgroup of 256 threads per segment of the context's segment table, one launch.  Thread t owns rows t, t + 256 ...
// counted from the segment's first row.
//   phase 1  the two fp64 sums s2 = sum (double)s^2 and n2 = sum (double)z^2 over the thread's movable entries in (row, k) order,
//            then a fixed binary tree over the 256 partials in LDS.  The order depends on (row within the complex, k) only: a
//            complex gets the same bits alone, padded or anywhere in a packed batch.  No atomics.
//   phase 2  every thread forms eps and amp from the two totals (the same operations on the same bits in every thread), draws the z
//            of its rows again with the same inline function -- the same bits -- and updates its own entries in place.
// Nothing crosses workgroups: no grid-wide hand-off, and a segment's result does not depend on the other segments.
#include "pp_internal.h"

struct CorrArgs {
    float *chi;                       // [N][4] corrected in place
    const float *score;               // [N][4] the network's score at chi
    const float *sc_mask;             // [N][4]
    const uint8_t *m1pi, *m2pi;       // [N][4]
    const uint8_t *fixed;             // [N] rows that are never moved and never counted, or nullptr
    const int32_t *off;               // the segment table [n_seg + 1]
    const pp_rng_row *tab;            // [N] (row within the complex, key of the complex)
    uint32_t seed_lo, seed_hi;
    int N;
    int step;                         // the counter's step: 2^20 + j
    float snr;
    double *trace;                    // this point's (s2, n2, eps, amp) of segment 0, or nullptr
    size_t trace_stride;              // doubles between two segments
};

// movable: in a periodic mask, SC_D_mask != 0, row not fixed, score finite
__device__ __forceinline__ bool corr_movable(const CorrArgs &A, int n, size_t e, float sc, float scm) {
    const bool periodic = (A.m1pi[e] | A.m2pi[e]) != 0;
    const bool pinned = A.fixed != nullptr && A.fixed[n] != 0;
    const bool finite = __builtin_fabsf(sc) <= 3.402823466e38f;          // false for NaN and the infinities
    return periodic && scm != 0.f && !pinned && finite;
}

// the corrector's draw of (row, k): words 0 and 1 of the counter at step 2^20 + j; words 2 and 3 stay unused
__device__ __forceinline__ float corr_draw(const CorrArgs &A, int n, int k) {
    const pp_rng_words w = pp_rng_draw(A.seed_lo, A.seed_hi, A.tab[n], k, A.step);
    return pp_rng_normal(w.o[0], w.o[1]);
}

__global__ void __launch_bounds__(256)
k_correct(CorrArgs A) {
#pragma clang fp contract(off)
    __shared__ double red_s[256], red_n[256];
    const int seg = blockIdx.x, tid = threadIdx.x;
    int a, b;
    pp_seg_rows(A.off, seg, A.N, a, b);
    double s2 = 0.0, n2 = 0.0;
    for (int n = a + tid; n < b; n += 256) {
        for (int k = 0; k < 4; k++) {
            const size_t e = (size_t)n * 4 + k;
            const float sc = A.score[e];
            if (!corr_movable(A, n, e, sc, A.sc_mask[e])) continue;
            const double sd = (double)sc, zd = (double)corr_draw(A, n, k);
            s2 += sd * sd;
            n2 += zd * zd;
        }
    }
    red_s[tid] = s2;
    red_n[tid] = n2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            red_s[tid] += red_s[tid + w];
            red_n[tid] += red_n[tid + w];
        }
        __syncthreads();
    }
    s2 = red_s[0];
    n2 = red_n[0];
    // a segment without a movable entry has s2 == 0 as well
    const double snr = (double)A.snr;
    const float eps = (float)(2.0 * snr * snr * n2 / s2);
    const float amp = (float)sqrt(2.0 * (double)eps);
    const bool on = s2 > 0.0 && __builtin_fabsf(eps) <= 3.402823466e38f && __builtin_fabsf(amp) <= 3.402823466e38f;
    if (!on) return;            // every entry keeps its bits, the trace row stays NaN
    if (tid == 0 && A.trace != nullptr) {
        double *t = A.trace + (size_t)seg * A.trace_stride;
        t[0] = s2; t[1] = n2; t[2] = (double)eps; t[3] = (double)amp;
    }
    for (int n = a + tid; n < b; n += 256) {
        for (int k = 0; k < 4; k++) {
            const size_t e = (size_t)n * 4 + k;
            const float sc = A.score[e], scm = A.sc_mask[e];
            if (!corr_movable(A, n, e, sc, scm)) continue;
            const float z = corr_draw(A, n, k);
            const float p = eps * sc;
            float y = A.chi[e] + p;
            const float q = amp * z;
            y = y + q;
            A.chi[e] = pp_wrap_pi(y) * scm;
        }
    }
}

// The corrector behind reverse step j on `chi`, in place, from the score the evaluation in front of it left in c->score.  trace
// (device [n_seg][n_steps][4] or null) receives (s2, n2, eps, amp) of every segment that has a corrector at row j.  One launch.
pp_status pp_launch_correct(pp_ctx *c, float *chi, const uint8_t *fixed, float snr, int j, int n_steps, const PPRng &rng,
                            double *trace, hipStream_t s) {
    CorrArgs A;
    A.chi = chi; A.score = c->score; A.sc_mask = c->b.SC_D_mask; A.m1pi = c->b.chi_1pi_periodic_mask; A.m2pi = c->b.chi_2pi_periodic_mask;
    A.fixed = fixed; A.off = c->seg_off; A.tab = rng.tab; A.seed_lo = rng.seed_lo; A.seed_hi = rng.seed_hi;
    A.N = c->N; A.step = c->max_steps + j; A.snr = snr;
    A.trace = trace ? trace + (size_t)j * 4 : nullptr;
    A.trace_stride = (size_t)n_steps * 4;
    PP_LAUNCH(c, k_correct, dim3(c->B), dim3(256), 0, s, A);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
