// Decoy ensembles (no reference counterpart): D decoys of every complex -> a consensus, a per-angle
// confidence, a score per decoy and a selected decoy, on the device.
//
// LAYOUT.  The B segments of the context are B / D groups of D consecutive segments of equal length: segment g * D + d is decoy d
// of group g (batch.replicate / replicate_many).  The consensus of a group has one row per residue of the complex; the consensus row
// of (group g, row r) is seg_off[g * D] / D + r, so the consensus rows of the groups lie back to back in [N / D][4] buffers exactly
// as the complexes would lie in a packed batch of one copy each.
//
// ARITHMETIC (everything below in fp64 on the fp32 inputs, every operation rounded on its own: fp contract off; PI is the double
// 3.14159265358979323846).  x_d is the angle of decoy d at one (consensus row, chi), p = 2 where chi_1pi_periodic_mask is set
// (the angle has period pi), else 1 (period 2 pi), m = SC_D_mask of decoy 0's entry (consensus) or of the entry itself (per decoy).
//   k_ens_consensus   one lane per (consensus row, chi), d = 0 .. D - 1 in that order:
//                        S = sum sin(p x_d), C = sum cos(p x_d)
//                        mean = (float)(atan2(S, C) / p), resultant = (float)(sqrt(S S + C C) / D);   m == 0: mean = resultant = 0
//                     resultant lies in [0, 1]: 1 = every decoy has this angle, 0 = the decoys cancel.
//   k_ens_per_decoy   one 256-thread workgroup per segment s; lane tid takes elements tid, tid + 256 ... of the segment's [rows][4]
//                     block, the 256 partial sums meet in a binary tree in LDS (the pattern of k_dsm_loss): every addition has a
//                     fixed place, two runs give the same bits, and the bits do not depend on what else the context holds.
//                        delta = (double)x - (double)mean, with the STORED fp32 mean; P = 2 PI / p;
//                        delta = delta - P floor((delta + P / 2) / P)                           -> [-P / 2, P / 2)
//                        dev[s] = sqrt(sum delta^2 m / max(sum m, 1)),    clash[s] = sum per_res / rows
//   k_ens_select      one workgroup per group: lane 0 walks d = 0 .. D - 1 over clash (select 1) or dev (select 2) and keeps the
//                     smallest; a later decoy replaces the holder only if it is smaller, or if the holder is NaN and it is not: the
//                     lowest index wins ties, a NaN loses to any number.  select 0: decoy 0.  Then the workgroup copies that
//                     decoy's rows to chi_best, bit for bit.
// No float atomics anywhere: every output word has one writer.
//
// A TABLE THAT BREAKS THE CONTRACT.  Rows come from pp_seg_rows, which clamps into the N rows of the batch.  A group is CONSISTENT
// when its D clamped segments have the same length len >= 1 and its consensus rows base .. base + len - 1 (base = first row / D) lie
// inside the N / D consensus rows (pp_group_rows, pp_segments.h: the one copy of this rule).  An inconsistent group reads nothing outside the batch and writes nothing outside the outputs:
// its best is -1, the dev of its segments NaN, its chi_best rows are not written, and a consensus row that maps into it gets 0, 0.
#include <cmath>

#include "pp_internal.h"

#define ENS_PI 3.14159265358979323846

__global__ void __launch_bounds__(256)
k_ens_consensus(int N, int G, int D, const int32_t *__restrict__ seg_off, const float *__restrict__ chi,
                const float *__restrict__ sc_mask, const uint8_t *__restrict__ m1pi, float *__restrict__ mean,
                float *__restrict__ resultant) {
#pragma clang fp contract(off)
    const int n_cons = N / D;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < 4 * n_cons; e += gridDim.x * 256) {
        const int crow = e >> 2, c = e & 3;
        const int g = pp_group_of_cons_row(seg_off, G, D, N, crow);
        int base, len, row0;
        const bool ok = pp_group_rows(seg_off, g, D, N, base, len, row0);
        const int r = crow - base;
        float mu = 0.f, R = 0.f;
        if (ok && r >= 0 && r < len) {
            const int e0 = 4 * (row0 + r) + c;
            if (sc_mask[e0] != 0.f) {
                const double p = m1pi[e0] ? 2.0 : 1.0;
                double S = 0.0, C = 0.0;
                for (int d = 0; d < D; d++) {
                    const double x = p * (double)chi[4 * (pp_decoy_row0(seg_off, g, D, N, d) + r) + c];
                    S += sin(x);
                    C += cos(x);
                }
                mu = (float)(atan2(S, C) / p);
                R = (float)(sqrt(S * S + C * C) / (double)D);
            }
        }
        mean[e] = mu;
        resultant[e] = R;
    }
}

__global__ void __launch_bounds__(256)
k_ens_per_decoy(int N, int D, const int32_t *__restrict__ seg_off, const float *__restrict__ chi, const float *__restrict__ sc_mask,
                const uint8_t *__restrict__ m1pi, const float *__restrict__ mean, const float *__restrict__ per_res,
                double *__restrict__ dev, double *__restrict__ clash) {
#pragma clang fp contract(off)
    __shared__ double red[3][256];
    const int s = blockIdx.x, tid = threadIdx.x;
    int a, b, base, len, row0;
    pp_seg_rows(seg_off, s, N, a, b);
    const bool ok = pp_group_rows(seg_off, s / D, D, N, base, len, row0);
    double sq = 0.0, sm = 0.0, sc = 0.0;
    if (ok) {
        for (int e = 4 * a + tid; e < 4 * b; e += 256) {
            const double P = m1pi[e] ? ENS_PI : 2.0 * ENS_PI;
            const double m = (double)sc_mask[e];
            double dl = (double)chi[e] - (double)mean[4 * (base - a) + e];
            dl = dl - P * floor((dl + P / 2.0) / P);
            sq += dl * dl * m;
            sm += m;
        }
    }
    if (per_res)
        for (int n = a + tid; n < b; n += 256) sc += (double)per_res[n];
    red[0][tid] = sq;
    red[1][tid] = sm;
    red[2][tid] = sc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            red[0][tid] += red[0][tid + w];
            red[1][tid] += red[1][tid + w];
            red[2][tid] += red[2][tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double den = red[1][0] > 1.0 ? red[1][0] : 1.0;
        dev[s] = ok ? sqrt(red[0][0] / den) : (double)NAN;
        if (per_res) clash[s] = red[2][0] / (double)(b - a > 0 ? b - a : 1);
    }
}

__global__ void __launch_bounds__(256)
k_ens_select(int N, int D, int select, const int32_t *__restrict__ seg_off, const float *__restrict__ chi,
             const double *__restrict__ dev, const double *__restrict__ clash, int32_t *__restrict__ best,
             float *__restrict__ chi_best) {
    __shared__ int pick;
    const int g = blockIdx.x, tid = threadIdx.x;
    int base, len, row0;
    const bool ok = pp_group_rows(seg_off, g, D, N, base, len, row0);
    if (tid == 0) {
        int k = -1;
        if (ok) {
            k = 0;
            const double *score = select == 1 ? clash : (select == 2 ? dev : nullptr);
            if (score)
                for (int d = 1; d < D; d++) {
                    const double v = score[g * D + d], cur = score[g * D + k];
                    if (v < cur || (cur != cur && v == v)) k = d;
                }
        }
        best[g] = k;
        pick = k;
    }
    __syncthreads();
    if (!chi_best || pick < 0) return;
    const int a = pp_decoy_row0(seg_off, g, D, N, pick);
    for (int e = tid; e < 4 * len; e += 256) chi_best[4 * base + e] = chi[4 * a + e];
}

pp_status pp_check_decoy_groups(const pp_ctx *c, int n_decoys, const char *who) {
    if (!c->packed && c->B != 1)
        FAIL(PP_ERR_INVALID, std::string(who) + ": needs a context from pp_complex_prepare_packed (or a B = 1 one), not a padded B > 1 batch");
    if (c->B % n_decoys != 0 || c->N % n_decoys != 0)
        FAIL(PP_ERR_INVALID, std::string(who) + ": the context's " + std::to_string(c->B) + " segments / " + std::to_string(c->N) +
                                 " rows are not groups of " + std::to_string(n_decoys) + " decoys");
    return PP_OK;
}

extern "C" pp_status pp_ensemble_reduce(pp_ctx *c, const float *chi, int n_decoys, const float *per_res, int select, float *mean,
                                        float *resultant, double *dev, double *clash, int32_t *best, float *chi_best, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !chi || !mean || !resultant || !dev || !best) FAIL(PP_ERR_INVALID, "pp_ensemble_reduce: null argument");
    if (per_res && !clash) FAIL(PP_ERR_INVALID, "pp_ensemble_reduce: per_res without clash");
    if (n_decoys < 1) FAIL(PP_ERR_INVALID, "pp_ensemble_reduce: n_decoys must be at least 1");
    if (select < 0 || select > 2) FAIL(PP_ERR_INVALID, "pp_ensemble_reduce: select must be 0 (none), 1 (clash) or 2 (medoid)");
    if (select == 1 && !per_res) FAIL(PP_ERR_INVALID, "pp_ensemble_reduce: select = 1 (clash) needs per_res");
    if (pp_status gs = pp_check_decoy_groups(c, n_decoys, "pp_ensemble_reduce"); gs != PP_OK) return gs;
    if (!c->b.SC_D_mask || !c->b.chi_1pi_periodic_mask)
        FAIL(PP_ERR_INVALID, "pp_ensemble_reduce: the batch of this ctx has no SC_D_mask / chi_1pi_periodic_mask");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int D = n_decoys, G = c->B / D, n_cons = c->N / D;
    const int blocks = (4 * n_cons + 255) / 256;
    hipLaunchKernelGGL(k_ens_consensus, dim3(blocks < 1 ? 1 : (blocks > 65536 ? 65536 : blocks)), dim3(256), 0, st, c->N, G, D,
                       c->seg_off, chi, c->b.SC_D_mask, c->b.chi_1pi_periodic_mask, mean, resultant);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ens_per_decoy, dim3(c->B), dim3(256), 0, st, c->N, D, c->seg_off, chi, c->b.SC_D_mask,
                       c->b.chi_1pi_periodic_mask, mean, per_res, dev, clash);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ens_select, dim3(G), dim3(256), 0, st, c->N, D, select, c->seg_off, chi, dev, clash, best, chi_best);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
