// Ordered fp32 vector math of the geometry kernels (device only).  Every operation is rounded on its own (fp contract off) in the
// order written here, so a NumPy float32 restatement of a kernel that uses these gives the same words (the oracles under tests/).
// One copy: kernels that promise each other's bits (pp_hnet.hip and pp_hydrogens.hip) keep that promise by calling the same function.
#pragma once

// ((ax bx) + (ay by)) + (az bz)
__device__ __forceinline__ float pp_dot3(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    return ((ax * bx) + (ay * by)) + (az * bz);
}
// |p - q|^2 with d = p - q (pp_sasa, pp_shell; the pair kernels of pp_polar / pp_allatom.h subtract q - p and spell it out)
__device__ __forceinline__ float pp_d2(float px, float py, float pz, float qx, float qy, float qz) {
#pragma clang fp contract(off)
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return pp_dot3(dx, dy, dz, dx, dy, dz);
}
struct pp_v3 { float x, y, z; };
// v / sqrt(v . v) per component; a zero vector gives 0 / 0
__device__ __forceinline__ pp_v3 pp_unit(pp_v3 v) {
#pragma clang fp contract(off)
    const float n = sqrtf(pp_dot3(v.x, v.y, v.z, v.x, v.y, v.z));
    return {v.x / n, v.y / n, v.z / n};
}
// (a x b)_x = (ay bz) - (az by), cyclic
__device__ __forceinline__ pp_v3 pp_cross(pp_v3 a, pp_v3 b) {
#pragma clang fp contract(off)
    return {(a.y * b.z) - (a.z * b.y), (a.z * b.x) - (a.x * b.z), (a.x * b.y) - (a.y * b.x)};
}
// q - p
__device__ __forceinline__ pp_v3 pp_sub(const float *q, pp_v3 p) {
#pragma clang fp contract(off)
    return {q[0] - p.x, q[1] - p.y, q[2] - p.z};
}
__device__ __forceinline__ bool pp_finite(float v) { return __builtin_fabsf(v) <= 3.402823466e38f; }
// the larger of two; a NaN sticks
__device__ __forceinline__ float pp_nanmax(float m, float o) { return (m != m) ? m : ((o != o || o > m) ? o : m); }
