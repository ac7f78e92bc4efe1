// Tile helpers shared by the two edge translation units (pp_edge.hip: exact fp32, pp_edge_f16.hip: split f16).  Both keep an
// activation tile in the accumulator layout of the 32x32 MFMAs: lane l = (edge l & 31, half h = l >> 5), register r of tile t
// <-> feature 32 t + 8 (r >> 2) + 4 h + (r & 3).  Device-only header; what differs between the two files (EdgeArgs, the weight
// pipelines, the geometry, the stage macros, the launchers) stays with them.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

// one tile (16 registers) <-> 32 consecutive features of a row-major vector
__device__ __forceinline__ void load_tile(const float *__restrict__ row32, int h, f32x16 &d) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        f32x4v a = *reinterpret_cast<const f32x4v *>(row32 + 8 * q + 4 * h);
        d[4 * q] = a[0]; d[4 * q + 1] = a[1]; d[4 * q + 2] = a[2]; d[4 * q + 3] = a[3];
    }
}
__device__ __forceinline__ void add_tile(const float *__restrict__ row32, int h, f32x16 &d) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        f32x4v a = *reinterpret_cast<const f32x4v *>(row32 + 8 * q + 4 * h);
        d[4 * q] += a[0]; d[4 * q + 1] += a[1]; d[4 * q + 2] += a[2]; d[4 * q + 3] += a[3];
    }
}
__device__ __forceinline__ void store_tile(float *__restrict__ row32, int h, const f32x16 &d) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        f32x4v a = {d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]};
        *reinterpret_cast<f32x4v *>(row32 + 8 * q + 4 * h) = a;
    }
}
__device__ __forceinline__ void relu_tile(f32x16 &d) {
#pragma unroll
    for (int r = 0; r < 16; r++) d[r] = fmaxf(d[r], 0.f);
}

// exchange buffer: tile t, quad q, lane l -> float4
__device__ __forceinline__ void xbuf_put(float *xbuf, int t, int lane, const f32x16 &d) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        f32x4v a = {d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]};
        *reinterpret_cast<f32x4v *>(xbuf + ((t * 4 + q) * 64 + lane) * 4) = a;
    }
}
__device__ __forceinline__ void xbuf_get(const float *xbuf, int t, int lane, f32x16 &d) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        f32x4v a = *reinterpret_cast<const f32x4v *>(xbuf + ((t * 4 + q) * 64 + lane) * 4);
        d[4 * q] = a[0]; d[4 * q + 1] = a[1]; d[4 * q + 2] = a[2]; d[4 * q + 3] = a[3];
    }
}

// LayerNorm statistics over the 128 features of this lane's edge (64 here, 64 in lane ^ 32); v is centred in
// place; returns 1/std, writes the mean
__device__ __forceinline__ float ln_center(f32x16 (&v)[4], float &mean_out) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) s += v[t][r];
    s += __shfl_xor(s, 32);
    const float mean = s * (1.f / 128.f);
    mean_out = mean;
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            float d = v[t][r] - mean;
            v[t][r] = d;
            q = fmaf(d, d, q);
        }
    q += __shfl_xor(q, 32);
    return 1.f / sqrtf(q * (1.f / 128.f) + 1e-5f);
}
// centred tile -> tile * rstd * gamma + beta
__device__ __forceinline__ void ln_affine_tile(f32x16 &v, float rstd, const float *__restrict__ gamma32,
                                               const float *__restrict__ beta32, int h) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        f32x4v g = *reinterpret_cast<const f32x4v *>(gamma32 + 8 * q + 4 * h);
        f32x4v b = *reinterpret_cast<const f32x4v *>(beta32 + 8 * q + 4 * h);
#pragma unroll
        for (int p = 0; p < 4; p++) v[4 * q + p] = fmaf(v[4 * q + p] * rstd, g[p], b[p]);
    }
}
