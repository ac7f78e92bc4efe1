// PackPPI-AP (src/models/AffinityPrediction.py): the head tensors and the ddG head.
//
//   pp_affinity_create / _destroy : mut_bias, seq_embedding, mutation_fusion, ddg_predictor on the device (:73-94)
//   k_affinity_head               : per segment max over rows of h_mt - h_wt and of h_wt - h_mt, then ddg_predictor
//                                   128 -> 128 ReLU -> 128 ReLU -> 1 on both (:186-187)
//
// The head is a few thousand FLOPs per segment over a [rows, 128] read: one 256-thread workgroup per segment, thread
// (f = tid & 127, half = tid >> 7) reduces feature f over every other row, the halves meet in LDS; then half 0 runs the
// MLP on the max of h_mt - h_wt and half 1 on that of h_wt - h_mt, one output feature per thread, plain fp32.
// k_affinity_embed, the part between the two networks, lives in pp_node.hip (it shares k_node_embed's helpers).
#include <string.h>
#include <cmath>

#include "pp_internal.h"

// torch.max semantics: a NaN wins and stays
__device__ __forceinline__ float max_nan(float m, float v) { return (v != v || v > m) ? v : m; }

__global__ void __launch_bounds__(256)
k_affinity_head(const float *__restrict__ h_wt, const float *__restrict__ h_mt, const int32_t *__restrict__ seg_off,
                int n_rows, const float *__restrict__ d0T, const float *__restrict__ d0_b, const float *__restrict__ d2T,
                const float *__restrict__ d2_b, const float *__restrict__ d4_w, const float *__restrict__ d4_b,
                float *__restrict__ ddg, float *__restrict__ ddg_inv) {
    __shared__ float red[2][2][128];     // [half][direction][feature]
    __shared__ float act[2][2][128];     // [direction][ping-pong][feature]
    const int s = blockIdx.x, t = threadIdx.x, f = t & 127, half = t >> 7;
    int a, b;
    pp_seg_rows(seg_off, s, n_rows, a, b);
    float m_fwd = -INFINITY, m_inv = -INFINITY;
    for (int r = a + half; r < b; r += 2) {
        const float w = h_wt[(size_t)r * 128 + f], m = h_mt[(size_t)r * 128 + f];
        m_fwd = max_nan(m_fwd, m - w);
        m_inv = max_nan(m_inv, w - m);
    }
    red[half][0][f] = m_fwd;
    red[half][1][f] = m_inv;
    __syncthreads();
    // half 0: ddg on max(h_mt - h_wt); half 1: ddg_inv on max(h_wt - h_mt).  Row order does not matter for a max except
    // where NaN meets NaN, and any NaN is NaN.
    const int dir = half;
    act[dir][0][f] = max_nan(red[0][dir][f], red[1][dir][f]);
    __syncthreads();
    float z = d0_b[f];
    for (int k = 0; k < 128; k++) z = fmaf(d0T[k * 128 + f], act[dir][0][k], z);
    act[dir][1][f] = z != z ? z : fmaxf(z, 0.f);      // ReLU that keeps a NaN, as torch.relu
    __syncthreads();
    z = d2_b[f];
    for (int k = 0; k < 128; k++) z = fmaf(d2T[k * 128 + f], act[dir][1][k], z);
    act[dir][0][f] = (z != z ? z : fmaxf(z, 0.f)) * d4_w[f];
    __syncthreads();
    if (f == 0) {
        float o = 0.f;
        for (int k = 0; k < 128; k++) o += act[dir][0][k];
        o += d4_b[0];
        (dir == 0 ? ddg : ddg_inv)[s] = o;
    }
}

extern "C" pp_status pp_affinity_create(const float *weights, size_t n_weights, int device, pp_affinity **out) {
    if (!weights || !out) FAIL(PP_ERR_INVALID, "pp_affinity_create: null argument");
    const bool network = n_weights == PP_AFF_N_WEIGHTS;
    if (!network && n_weights != PP_AFF_N_WEIGHTS_LINEAR)
        FAIL(PP_ERR_INVALID, "pp_affinity_create: expected " + std::to_string(PP_AFF_N_WEIGHTS) + " (network) or " +
                                 std::to_string(PP_AFF_N_WEIGHTS_LINEAR) + " (linear) weights, got " + std::to_string(n_weights));
    for (size_t i = 0; i < n_weights; i++)
        if (!std::isfinite(weights[i])) FAIL(PP_ERR_INVALID, "pp_affinity_create: weight " + std::to_string(i) + " is not finite");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FAIL(PP_ERR_NO_DEVICE, "pp_affinity_create: no HIP device visible");
    if (device < 0 || device >= ndev) FAIL(PP_ERR_INVALID, "pp_affinity_create: bad device index");
    PP_HIP_CHECK(hipSetDevice(device));

    // host image: the k_affinity_embed matrices k-quad interleaved ([in / 4][128][4], dense_slice), the head's transposed
    const float *w = weights;
    std::vector<float> img;
    auto take = [&](size_t n) { const float *p = w; w += n; return p; };
    auto put = [&](const float *src, size_t n) { size_t at = img.size(); img.insert(img.end(), src, src + n); return at; };
    auto put_T4 = [&](const float *W, int rows, int cols) {
        size_t at = img.size();
        img.resize(at + (size_t)rows * cols);
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++) img[at + ((size_t)(c >> 2) * rows + r) * 4 + (c & 3)] = W[(size_t)r * cols + c];
        return at;
    };
    auto put_T = [&](const float *W, int rows, int cols) {
        size_t at = img.size();
        img.resize(at + (size_t)rows * cols);
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++) img[at + (size_t)c * rows + r] = W[(size_t)r * cols + c];
        return at;
    };
    size_t o_mb = 0, o_se = 0, o_f0 = 0, o_f0b = 0, o_f2 = 0, o_f2b = 0;
    if (network) {
        o_mb = put(take(2 * 128), 2 * 128);
        o_se = put(take(21 * 128), 21 * 128);
        o_f0 = put_T4(take(128 * 384), 128, 384);
        o_f0b = put(take(128), 128);
        o_f2 = put_T4(take(128 * 128), 128, 128);
        o_f2b = put(take(128), 128);
    }
    const size_t o_d0 = put_T(take(128 * 128), 128, 128), o_d0b = put(take(128), 128);
    const size_t o_d2 = put_T(take(128 * 128), 128, 128), o_d2b = put(take(128), 128);
    const size_t o_d4 = put(take(128), 128), o_d4b = put(take(1), 1);

    pp_affinity *a = new (std::nothrow) pp_affinity();
    if (!a) FAIL(PP_ERR_INVALID, "out of host memory");
    a->device = device;
    a->network = network;
    if (hipMalloc(reinterpret_cast<void **>(&a->buf), img.size() * sizeof(float)) != hipSuccess) {
        delete a;
        FAIL(PP_ERR_HIP, "pp_affinity_create: hipMalloc failed");
    }
    if (hipMemcpy(a->buf, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(a->buf);
        delete a;
        FAIL(PP_ERR_HIP, "pp_affinity_create: hipMemcpy failed");
    }
    const float *d = a->buf;
    if (network) {
        a->mut_bias = d + o_mb; a->seq_emb = d + o_se;
        a->f0T = d + o_f0; a->f0_b = d + o_f0b; a->f2T = d + o_f2; a->f2_b = d + o_f2b;
    }
    a->d0T = d + o_d0; a->d0_b = d + o_d0b; a->d2T = d + o_d2; a->d2_b = d + o_d2b; a->d4_w = d + o_d4; a->d4_b = d + o_d4b;
    *out = a;
    return PP_OK;
}

extern "C" void pp_affinity_destroy(pp_affinity *a) {
    if (!a) return;
    if (a->buf) (void)hipFree(a->buf);
    delete a;
}

extern "C" pp_status pp_affinity_predict(const pp_affinity *a, const float *h_wt, const float *h_mt, const int32_t *seg_offsets,
                                         int n_seg, int n_rows, float *ddg, float *ddg_inv, void *stream) {
    if (!a || !h_wt || !h_mt || !seg_offsets || !ddg || !ddg_inv) FAIL(PP_ERR_INVALID, "pp_affinity_predict: null argument");
    if (n_seg < 1 || n_rows < 1) FAIL(PP_ERR_INVALID, "pp_affinity_predict: n_seg and n_rows must be positive");
    PP_HIP_CHECK(hipSetDevice(a->device));
    hipLaunchKernelGGL(k_affinity_head, dim3(n_seg), dim3(256), 0, static_cast<hipStream_t>(stream), h_wt, h_mt, seg_offsets,
                       n_rows, a->d0T, a->d0_b, a->d2T, a->d2_b, a->d4_w, a->d4_b, ddg, ddg_inv);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
