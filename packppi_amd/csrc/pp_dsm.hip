// Denoising score-matching loss (TorsionalDiffusion.py:126-154), the two pieces that are not the network:
//
//   k_so2_score : SO2Schedule.score(x, sigma) (schedule.py:66-75) WITHOUT its two 5001 x 5001 fp64 tables.  A table entry is a
//                 pure function of its two indices (schedule.py:8-20, 48-50), so the entry is computed instead of looked up:
//                 the quantisation to the index pair is the reference's, the grids x_j / sigma_i are the reference's (made by
//                 NumPy on the host, pp_so2_set_grids), the 201-term series runs in fp64 in the reference's order.
//   k_dsm_loss  : score_norm lookup (schedule.py:88-94), pred * sqrt(score_norm) * mask, and the masked sums per segment, in
//                 fp64 as the reference computes them (score_norm_ is float64, so everything behind it is promoted).
//
// PROMOTION DETAIL of the quantisation.  `np.log(np.abs(x) / PI + 1e-10)` runs on a float32 array and returns float32.  What
// follows, `(x - np.log(X_MIN)) / (0 - np.log(X_MIN)) * X_N`, mixes it with float64 SCALARS: under the reference's pinned
// NumPy 1.22 (value-based casting) the array stays float32 and the scaling is done in float32; under NumPy 2 (NEP 50) the
// float32 log is promoted and the scaling is done in float64.  The fixtures of this project are made under NumPy 2, so the
// kernels follow NumPy 2: fp32 wrap, fp32 division, fp32 logf, then fp64 arithmetic, clip, round half to even.
//
// Neither kernel is worth more than a clean loop: the score is ~200 fp64 exp per angle, the loss a few thousand elements.
#include <cmath>
#include <mutex>

#include "pp_internal.h"

#define SO2_N 5000                 // X_N = SIGMA_N: 5001 grid points each
#define SO2_TERMS 100              // series terms -100 .. 100 (schedule.py:48-49)
#define PP_MAX_DEVICES 64

struct So2Consts {
    float pi_f;                    // (float)PI: a float32 array op with a Python float casts the scalar to float32
    double pi, x_lo, x_span, s_lo, s_span;     // PI; ln X_MIN, 0 - ln X_MIN; ln SIGMA_MIN, ln SIGMA_MAX - ln SIGMA_MIN
};

static So2Consts so2_consts(int pi_periodic) {
    const double PI_D = 3.14159265358979323846;
    So2Consts k;
    k.pi = pi_periodic ? 0.5 * PI_D : PI_D;
    k.pi_f = (float)k.pi;
    k.x_lo = log(1e-5);
    k.x_span = 0.0 - log(1e-5);
    k.s_lo = log(3e-3);
    k.s_span = log(2.0) - log(3e-3);
    return k;
}

// np.round(np.clip(v, 0, 5000)).astype(int); a NaN (non-finite input) goes to index 0 so that no read leaves the grid
__device__ __forceinline__ int so2_index(double v) {
    v = v >= 0.0 ? (v > (double)SO2_N ? (double)SO2_N : v) : 0.0;
    return (int)rint(v);
}
__device__ __forceinline__ int so2_sigma_index(float sigma, const So2Consts &k) {
#pragma clang fp contract(off)
    const float l = logf(sigma / k.pi_f);
    return so2_index(((double)l - k.s_lo) / k.s_span * (double)SO2_N);
}

// grids: [2][5001] fp64 (schedule 1pi, then 2pi) of x_j and of sigma_i
__global__ void __launch_bounds__(256)
k_so2_score(const float *__restrict__ x, const float *__restrict__ sigma, size_t n, So2Consts k, const double *__restrict__ x_grid,
            const double *__restrict__ sigma_grid, float *__restrict__ score, int32_t *__restrict__ idx) {
#pragma clang fp contract(off)
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        // (x + PI) % (2 PI) - PI in fp32, np.remainder semantics (the result takes the divisor's sign)
        const float two_pi = 2.0f * k.pi_f;          // Python evaluates 2 * PI in double: (float)(2 PI) == 2 (float)PI exactly
        float r = fmodf(x[e] + k.pi_f, two_pi);
        if (r != 0.f && r < 0.f) r += two_pi;
        const float xw = r - k.pi_f;
        const float sign = xw > 0.f ? 1.f : (xw < 0.f ? -1.f : 0.f);
        const float lx = logf(fabsf(xw) / k.pi_f + 1e-10f);
        const int xi = so2_index(((double)lx - k.x_lo) / k.x_span * (double)SO2_N);
        const int si = so2_sigma_index(sigma[e], k);
        const double xv = x_grid[xi], sv = sigma_grid[si], s2 = sv * sv;
        double p = 0.0, g = 0.0;
        for (int i = -SO2_TERMS; i <= SO2_TERMS; i++) {
            const double y = xv + 2.0 * k.pi * (double)i;
            const double ex = exp(-(y * y) / 2.0 / s2);
            p += ex;
            g += y / s2 * ex;
        }
        const double entry = g / (p == 0.0 ? 1e-10 : p);
        score[e] = (float)(-(double)sign * entry);
        if (idx) {
            idx[2 * e] = si;
            idx[2 * e + 1] = xi;
        }
    }
}

// ---- the grids, per device ------------------------------------------------------------------------------------------------------
static std::mutex g_grid_mutex;
static double *g_grids[PP_MAX_DEVICES] = {};      // [2][2][5001]: x (1pi, 2pi), sigma (1pi, 2pi)

extern "C" pp_status pp_so2_set_grids(const double *x_grid, const double *sigma_grid, int device) {
    if (!x_grid || !sigma_grid) FAIL(PP_ERR_INVALID, "pp_so2_set_grids: null argument");
    if (device < 0 || device >= PP_MAX_DEVICES) FAIL(PP_ERR_INVALID, "pp_so2_set_grids: device index out of range");
    const size_t half = (size_t)2 * (SO2_N + 1);
    for (size_t i = 0; i < half; i++)
        if (!(x_grid[i] > 0.0) || !(sigma_grid[i] > 0.0) || std::isinf(x_grid[i]) || std::isinf(sigma_grid[i]))
            FAIL(PP_ERR_INVALID, "pp_so2_set_grids: grid entries must be positive and finite");
    std::lock_guard<std::mutex> lock(g_grid_mutex);
    PP_HIP_CHECK(hipSetDevice(device));
    if (!g_grids[device]) PP_HIP_CHECK(hipMalloc(&g_grids[device], 2 * half * sizeof(double)));
    PP_HIP_CHECK(hipMemcpy(g_grids[device], x_grid, half * sizeof(double), hipMemcpyHostToDevice));
    PP_HIP_CHECK(hipMemcpy(g_grids[device] + half, sigma_grid, half * sizeof(double), hipMemcpyHostToDevice));
    return PP_OK;
}

extern "C" pp_status pp_so2_score(const float *x, const float *sigma, size_t n, int pi_periodic, float *score, int32_t *idx,
                                  int device, void *stream) {
    if (!x || !sigma || !score) FAIL(PP_ERR_INVALID, "pp_so2_score: null argument");
    if (device < 0 || device >= PP_MAX_DEVICES) FAIL(PP_ERR_INVALID, "pp_so2_score: device index out of range");
    if (pi_periodic != 0 && pi_periodic != 1) FAIL(PP_ERR_INVALID, "pp_so2_score: pi_periodic must be 0 or 1");
    const double *grids;
    {
        std::lock_guard<std::mutex> lock(g_grid_mutex);
        grids = g_grids[device];
    }
    if (!grids) FAIL(PP_ERR_INVALID, "pp_so2_score: pp_so2_set_grids has not been called for this device");
    if (n == 0) return PP_OK;
    PP_HIP_CHECK(hipSetDevice(device));
    const size_t half = (size_t)2 * (SO2_N + 1), sel = pi_periodic ? 0 : (size_t)(SO2_N + 1);
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_so2_score, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x, sigma, n, so2_consts(pi_periodic), grids + sel, grids + half + sel, score, idx);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

// ---- the loss ---------------------------------------------------------------------------------------------------------------------
// One 256-thread workgroup per segment.  Thread t takes elements t, t + 256, ... of the segment's [rows][4] block, then the 256
// partial sums meet in a binary tree in LDS: the order of every addition is fixed, two runs give the same bits.
__global__ void __launch_bounds__(256)
k_dsm_loss(int N, const int32_t *__restrict__ seg_off, const float *__restrict__ pred, const float *__restrict__ target,
           const float *__restrict__ t_rows, const float *__restrict__ sc_mask, const uint8_t *__restrict__ m1pi,
           const double *__restrict__ score_norm, So2Consts k1, So2Consts k2, float sig_lo, float sig_span,
           double *__restrict__ num, double *__restrict__ den) {
#pragma clang fp contract(off)
    __shared__ double red[2][256];
    const int s = blockIdx.x, tid = threadIdx.x;
    int a, b;
    pp_seg_rows(seg_off, s, N, a, b);
    double sn_acc = 0.0, sd_acc = 0.0;
    for (int e = 4 * a + tid; e < 4 * b; e += 256) {
        const int n = e >> 2;
        const float sigma = expf(sig_lo + sig_span * t_rows[n]);          // t_to_sigma, fp32 (schedule.py:165-174)
        const double sn = m1pi[e] ? score_norm[so2_sigma_index(sigma, k1)] : score_norm[SO2_N + 1 + so2_sigma_index(sigma, k2)];
        const double m = (double)sc_mask[e];
        const double d = (double)target[e] - (double)pred[e] * sqrt(sn) * m;
        sn_acc += d * d / (sn + 1e-6);
        sd_acc += m;
    }
    red[0][tid] = sn_acc;
    red[1][tid] = sd_acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            red[0][tid] += red[0][tid + w];
            red[1][tid] += red[1][tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        num[s] = red[0][0];
        den[s] = red[1][0];
    }
}

extern "C" pp_status pp_dsm_loss(pp_ctx *c, const float *pred_score, const float *target_score, const float *t_rows,
                                 const double *score_norm, double *num, double *den, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !pred_score || !target_score || !t_rows || !score_norm || !num || !den) FAIL(PP_ERR_INVALID, "pp_dsm_loss: null argument");
    if (!c->b.SC_D_mask || !c->b.chi_1pi_periodic_mask) FAIL(PP_ERR_INVALID, "pp_dsm_loss: the batch of this ctx has no SC_D_mask / chi_1pi_periodic_mask");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    const double lo = pp_log_sigma_min(), hi = pp_log_sigma_max();
    hipLaunchKernelGGL(k_dsm_loss, dim3(c->B), dim3(256), 0, static_cast<hipStream_t>(stream), c->N, c->seg_off,
                       pred_score, target_score, t_rows, c->b.SC_D_mask, c->b.chi_1pi_periodic_mask, score_norm, so2_consts(1), so2_consts(0), (float)lo, (float)(hi - lo), num, den);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
