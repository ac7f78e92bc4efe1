// Disulfide bridges (no reference kernel): find the cysteine pairs whose sulfurs can meet, from the backbone
// alone, and close them by choosing the two chi1.  The reference's clash loss exempts every SG-SG pair (clash.py:198-210) and
// k_clash keeps that exemption; this is the only stage that knows the bond.
//
// DEFINITION, per segment of the context's segment table; fp32, every operation rounded on its own (fp contract off).
//   ELIGIBLE row: residue_type == PP_RESTYPE_CYS, residue_mask != 0, atom_mask slots 0, 1, 2, 5 (N, CA, C, SG) != 0.
//   GEOMETRY, relative to the row's CA (pp_shell.hip's habit: a structure far from the origin loses nothing).  The backbone frame is
//     pp_atom14's (e0 along C - CA, e1 from N - CA, 1e-8 inside both roots); with D the default frame of the slot's rigid group,
//     l its literature position and (s, c) the normalised sine and cosine of the angle,
//       v = (lx, c ly - s lz, s ly + c lz);  w = D.R v + D.t;  p = G.R w          (the chain G o (D Rx) applied to l, CA left out)
//     CB(n) = slot 4 at angle 0 of its group, SG(n, theta) = slot 5 with chi1 = theta.
//   GRID  theta_k = (float)(-pi + 2 pi k / 72) (the double expression, rounded once), k = 0 .. 71.
//   ENERGY of a pair a < b at (p, q), A = SG(a, theta_p), B = SG(b, theta_q), both taken relative to CA_a (B carries CA_b - CA_a):
//       E = ((|A-B| - 2.04) / 0.10)^2 + ((ang(CB_a, A, B) - 104) / 10)^2 + ((ang(CB_b, B, A) - 104) / 10)^2
//           + ((|dih(CB_a, A, B, CB_b)| - 90) / 30)^2                                   angles in degrees, summed left to right
//     ang(P, V, Q) = acos(clamp(u.v / (|u| |v|))), u = P - V, v = Q - V;  dih = atan2(|b2| b1.(b2 x b3), (b1 x b2).(b2 x b3)) with
//     b1 = A - CB_a, b2 = B - A, b3 = CB_b - B.  Emin(a, b) = min over the 72 x 72 grid, ties to the lowest 72 p + q.
//   CANDIDATES: a < b, same segment, both eligible, |CB_a - CB_b| <= cb_max, Emin <= max_energy.
//   BONDED SET: greedy in ascending (Emin, a, b); a pair is taken iff neither row is bonded yet.
//   CLOSURE of a bonded pair: a fixed row's table is its SG at its own chi1, 72 times.  With Emin_r the minimum of E over that
//     (restricted) grid and thr = min(max_energy, Emin_r + 4) -- raised to Emin_r if that is larger, so that the set is never empty --
//       F = {(p, q): E <= thr},   J = E + (wrap(theta_p - chi[a][0])^2 + wrap(theta_q - chi[b][0])^2) / sigma_chi^2,
//     wrap(x) = x - 2 pi rint(x / 2 pi); a fixed row's term is 0; without chi J = E.  The pick is the argmin of J over F, ties to the
//     lowest 72 p + q.  chi_out = chi bit for bit except chi_out[a][0] = theta_p, chi_out[b][0] = theta_q on rows that are not fixed.
//   EXPLICIT PAIRS replace the candidates: no cb_max, no max_energy (both thresholds are +inf).  A listed pair with a row out of
//     range, not eligible, or in another segment than its partner is dropped here; the Python layer refuses it by name first.
//
// LAUNCH, all on the caller's stream, no read-back:
//   k_ds_rows    one workgroup: the eligible rows in ascending order (a block scan per 256 rows) -> eidx[N], erow[E]
//   k_ds_tables  one workgroup per row (the others leave at once): 72 SG, CB, SG at the row's own chi1, CA -> tab[e][76] (float4)
//   k_ds_cand    one lane per eligible row walks the eligible rows behind it in its segment and appends the pairs within cb_max to
//                the candidate list (integer atomic; the list's order is never read: everything behind it orders by value and rows)
//     or k_ds_pairs: the caller's list, one lane per pair
//   k_ds_scan    one workgroup per candidate (grid-stride): both tables in LDS, 5184 energies over 256 lanes, argmin on (value, index)
//   k_ds_match   one workgroup per segment: repeatedly the smallest (Emin, a, b) among its candidates with two free rows
//   k_ds_close   one workgroup per candidate, the bonded ones stay: restricted minimum, then the argmin of J over F; one lane writes
// CAPACITY.  The candidate list holds min(N (N - 1) / 2, 64 N) pairs: every pair there is up to N = 129, 64 per row beyond.  A
// call that finds more sets count[s] = -1 for EVERY segment and bonds nothing (partner -1, report 0, chi_out = chi): the call has no
// read-back, so that is how it fails; packppi_amd.lib raises on it.  Never a silent cut.
#include "pp_internal.h"
#include "pp_vec.h"
#include <algorithm>
#pragma clang fp contract(off)

#define DS_T 256
#define DS_G 72
#define DS_PTS (DS_G * DS_G)
#define DS_PER ((DS_PTS + DS_T - 1) / DS_T)      // grid points a lane holds
#define DS_TAB 76                                // float4 per eligible row: 0..71 SG(theta_k) | 72 CB | 73 SG(own chi1) | 74 CA | 75 own chi1
#define DS_TWO_PI_F 6.28318530717958647692f
#define DS_RAD2DEG_F 57.29577951308232087680f

__host__ __device__ __forceinline__ float ds_theta(int k) { return (float)(-PP_PI_D + 2.0 * PP_PI_D * (double)k / 72.0); }

__device__ __forceinline__ float ds_dot(const float *a, const float *b) { return pp_dot3(a[0], a[1], a[2], b[0], b[1], b[2]); }
// pp_cross's operations on arrays: converting to pp_v3 and back at every call would be longer than these three lines
__device__ __forceinline__ void ds_cross(const float *a, const float *b, float *o) {
    o[0] = (a[1] * b[2]) - (a[2] * b[1]);
    o[1] = (a[2] * b[0]) - (a[0] * b[2]);
    o[2] = (a[0] * b[1]) - (a[1] * b[0]);
}
__device__ __forceinline__ float ds_wrap(float x) { return x - (rintf(x / DS_TWO_PI_F) * DS_TWO_PI_F); }
__device__ __forceinline__ float ds_sq(float x) { return x * x; }

// angle at V between P - V and Q - V, degrees
__device__ __forceinline__ float ds_angle(const float *P, const float *V, const float *Q) {
    float u[3], v[3];
    for (int k = 0; k < 3; k++) { u[k] = P[k] - V[k]; v[k] = Q[k] - V[k]; }
    float c = ds_dot(u, v) / (sqrtf(ds_dot(u, u)) * sqrtf(ds_dot(v, v)));
    c = c > 1.f ? 1.f : (c < -1.f ? -1.f : c);
    return acosf(c) * DS_RAD2DEG_F;
}

// E of one grid point; dist and chi3 (radians, signed) on request
__device__ __forceinline__ float ds_energy(const float *A, const float *B, const float *cba, const float *cbb, float *dist, float *chi3) {
    float b1[3], b2[3], b3[3], n1[3], n2[3];
    for (int k = 0; k < 3; k++) { b1[k] = A[k] - cba[k]; b2[k] = B[k] - A[k]; b3[k] = cbb[k] - B[k]; }
    const float d = sqrtf(ds_dot(b2, b2));
    ds_cross(b1, b2, n1);
    ds_cross(b2, b3, n2);
    const float dih = atan2f(d * ds_dot(b1, n2), ds_dot(n1, n2));
    if (dist) *dist = d;
    if (chi3) *chi3 = dih;
    float e = ds_sq((d - 2.04f) / 0.10f);
    e = e + ds_sq((ds_angle(cba, A, B) - 104.f) / 10.f);
    e = e + ds_sq((ds_angle(cbb, B, A) - 104.f) / 10.f);
    e = e + ds_sq(((fabsf(dih) * DS_RAD2DEG_F) - 90.f) / 30.f);
    return e;
}

// argmin on (value, index) over the workgroup: the smaller value, on equal values the smaller index, whatever the lane order.
// A lane without an entry brings (+inf, INT_MAX); a NaN value never wins against a number.
__device__ __forceinline__ void ds_argmin(float &v, int &i, float *rv, int *ri, int tid) {
    rv[tid] = v; ri[tid] = i;
    __syncthreads();
    for (int w = DS_T / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const float v2 = rv[tid + w];
            const int i2 = ri[tid + w];
            if (v2 < rv[tid] || (v2 == rv[tid] && i2 < ri[tid]) || (rv[tid] != rv[tid] && v2 == v2)) { rv[tid] = v2; ri[tid] = i2; }
        }
        __syncthreads();
    }
    v = rv[0]; i = ri[0];
    __syncthreads();
}

// head[0] = eligible rows, head[1] = candidate pairs found (may exceed the capacity: then nothing is bonded)
__global__ void __launch_bounds__(DS_T)
k_ds_rows(int N, const int64_t *__restrict__ rtype, const float *__restrict__ rmask, const float *__restrict__ amask,
          int32_t *__restrict__ eidx, int32_t *__restrict__ erow, int32_t *__restrict__ head) {
    __shared__ int sc[DS_T];
    __shared__ int s_base;
    const int tid = threadIdx.x;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int base = 0; base < N; base += DS_T) {
        const int n = base + tid;
        int f = 0;
        if (n < N) {
            const float *am = amask + (size_t)n * 14;
            f = (rtype[n] == PP_RESTYPE_CYS && rmask[n] != 0.f && am[0] != 0.f && am[1] != 0.f && am[2] != 0.f && am[5] != 0.f) ? 1 : 0;
        }
        sc[tid] = f;
        __syncthreads();
        for (int o = 1; o < DS_T; o <<= 1) {
            const int v = tid >= o ? sc[tid - o] : 0;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        const int b0 = s_base;
        if (n < N) {
            const int e = b0 + sc[tid] - 1;
            eidx[n] = f ? e : -1;
            if (f) erow[e] = n;
        }
        __syncthreads();
        if (tid == DS_T - 1) s_base = b0 + sc[DS_T - 1];
        __syncthreads();
    }
    if (tid == 0) { head[0] = s_base; head[1] = 0; head[2] = 0; head[3] = 0; }
}

__global__ void __launch_bounds__(128)
k_ds_tables(int N, const float *__restrict__ X, const int64_t *__restrict__ rtype, const float *__restrict__ chi,
            const int32_t *__restrict__ eidx, const float *__restrict__ default_frames, const int32_t *__restrict__ a2g,
            const float *__restrict__ lit, float4 *__restrict__ tab) {
    const int n = blockIdx.x, k = threadIdx.x;
    if (n >= N) return;
    const int e = eidx[n];
    if (e < 0 || k >= DS_TAB) return;
    float4 *o = tab + (size_t)e * DS_TAB;
    const float *x = X + (size_t)n * 42;
    const float own = chi ? chi[(size_t)n * 4] : 0.f;
    if (k == 74) { o[k] = make_float4(x[3], x[4], x[5], 0.f); return; }
    if (k == 75) { o[k] = make_float4(own, 0.f, 0.f, 0.f); return; }
    // backbone frame, columns e0 e1 e2 (pp_atom14's construction)
    float av[3], bv[3], cv[3];
    for (int q = 0; q < 3; q++) { av[q] = x[6 + q] - x[3 + q]; bv[q] = x[q] - x[3 + q]; }
    const float na = sqrtf(ds_dot(av, av) + 1e-8f);
    for (int q = 0; q < 3; q++) av[q] = av[q] / na;
    const float dt = ds_dot(av, bv);
    for (int q = 0; q < 3; q++) bv[q] = bv[q] - (av[q] * dt);
    const float nb = sqrtf(ds_dot(bv, bv) + 1e-8f);
    for (int q = 0; q < 3; q++) bv[q] = bv[q] / nb;
    ds_cross(av, bv, cv);
    const int S = (int)rtype[n];
    const int slot = k == 72 ? 4 : 5;
    const float ang = k < DS_G ? ds_theta(k) : (k == 72 ? 0.f : own);
    const float s0 = sinf(ang), c0 = cosf(ang);
    const float den = sqrtf(fmaxf((s0 * s0) + (c0 * c0), 1e-12f));
    const float sn = s0 / den, cs = c0 / den;
    const float *D = default_frames + ((size_t)S * 8 + a2g[S * 14 + slot]) * 16;
    const float *l = lit + ((size_t)S * 14 + slot) * 3;
    const float v[3] = {l[0], (cs * l[1]) - (sn * l[2]), (sn * l[1]) + (cs * l[2])};
    float w[3], p[3];
    for (int r = 0; r < 3; r++) w[r] = (((D[4 * r] * v[0]) + (D[4 * r + 1] * v[1])) + (D[4 * r + 2] * v[2])) + D[4 * r + 3];
    for (int r = 0; r < 3; r++) p[r] = ((av[r] * w[0]) + (bv[r] * w[1])) + (cv[r] * w[2]);
    o[k] = make_float4(p[0], p[1], p[2], 0.f);
}

__global__ void __launch_bounds__(DS_T)
k_ds_cand(int N, int n_seg, const int32_t *__restrict__ seg_off, const int32_t *__restrict__ erow, const float4 *__restrict__ tab,
          float cb_max, int cap, int32_t *__restrict__ head, int4 *__restrict__ candi) {
    const int e = blockIdx.x * DS_T + threadIdx.x;
    const int ne = head[0];
    if (e >= ne) return;
    const int a = erow[e];
    int lo, hi;
    pp_seg_rows(seg_off, pp_seg_of_row(seg_off, n_seg, a), N, lo, hi);
    if (a < lo || a >= hi) return;                           // a table that breaks the contract: the row is in no segment
    const float4 cba = tab[(size_t)e * DS_TAB + 72], caa = tab[(size_t)e * DS_TAB + 74];
    for (int e2 = e + 1; e2 < ne; e2++) {
        const int b = erow[e2];
        if (b >= hi) break;
        const float4 cbb = tab[(size_t)e2 * DS_TAB + 72], cab = tab[(size_t)e2 * DS_TAB + 74];
        const float d[3] = {(cbb.x - cba.x) + (cab.x - caa.x), (cbb.y - cba.y) + (cab.y - caa.y), (cbb.z - cba.z) + (cab.z - caa.z)};
        if (sqrtf(ds_dot(d, d)) <= cb_max) {
            const int i = atomicAdd(&head[1], 1);
            if (i < cap) candi[i] = make_int4(a, b, e, e2);
        }
    }
}

__global__ void __launch_bounds__(DS_T)
k_ds_pairs(int N, int n_seg, const int32_t *__restrict__ seg_off, const int32_t *__restrict__ eidx, const int32_t *__restrict__ pairs,
           int n_pairs, int32_t *__restrict__ head, int4 *__restrict__ candi) {
    const int i = blockIdx.x * DS_T + threadIdx.x;
    if (i == 0) head[1] = n_pairs;
    if (i >= n_pairs) return;
    int a = pairs[2 * i], b = pairs[2 * i + 1];
    if (a > b) { const int t = a; a = b; b = t; }
    int4 out = make_int4(-1, -1, -1, -1);
    if (a >= 0 && b < N && a != b && eidx[a] >= 0 && eidx[b] >= 0) {
        const int s = pp_seg_of_row(seg_off, n_seg, a);
        int lo, hi;
        pp_seg_rows(seg_off, s, N, lo, hi);
        if (a >= lo && b < hi) out = make_int4(a, b, eidx[a], eidx[b]);
    }
    candi[i] = out;
}

// both rows' tables relative to CA_a into LDS; a row with fix_a / fix_b gets its SG at its own chi1 in every entry
__device__ __forceinline__ void ds_load_pair(const float4 *__restrict__ tab, int ea, int eb, bool fix_a, bool fix_b, float4 *lA, float4 *lB,
                                             float (*lcb)[4], int tid) {
    const float4 *ta = tab + (size_t)ea * DS_TAB, *tb = tab + (size_t)eb * DS_TAB;
    const float4 caa = ta[74], cab = tb[74];
    const float sh[3] = {cab.x - caa.x, cab.y - caa.y, cab.z - caa.z};
    if (tid < DS_G) {
        lA[tid] = ta[fix_a ? 73 : tid];
    } else if (tid < 2 * DS_G) {
        const float4 q = tb[fix_b ? 73 : tid - DS_G];
        lB[tid - DS_G] = make_float4(q.x + sh[0], q.y + sh[1], q.z + sh[2], 0.f);
    } else if (tid == 2 * DS_G) {
        const float4 q = ta[72];
        lcb[0][0] = q.x; lcb[0][1] = q.y; lcb[0][2] = q.z;
    } else if (tid == 2 * DS_G + 1) {
        const float4 q = tb[72];
        lcb[1][0] = q.x + sh[0]; lcb[1][1] = q.y + sh[1]; lcb[1][2] = q.z + sh[2];
    }
}

__device__ __forceinline__ float ds_point(const float4 *lA, const float4 *lB, const float (*lcb)[4], int idx, float *dist, float *chi3) {
    const int p = idx / DS_G, q = idx - p * DS_G;
    const float4 a4 = lA[p], b4 = lB[q];
    const float A[3] = {a4.x, a4.y, a4.z}, B[3] = {b4.x, b4.y, b4.z};
    return ds_energy(A, B, lcb[0], lcb[1], dist, chi3);
}

__global__ void __launch_bounds__(DS_T)
k_ds_scan(int cap, const int32_t *__restrict__ head, const int4 *__restrict__ candi, const float4 *__restrict__ tab,
          float2 *__restrict__ cande) {
    __shared__ float4 lA[DS_G], lB[DS_G];
    __shared__ float lcb[2][4];
    __shared__ float rv[DS_T];
    __shared__ int ri[DS_T];
    const int tid = threadIdx.x;
    const int nc = head[1] < cap ? head[1] : cap;
    for (int c = blockIdx.x; c < nc; c += gridDim.x) {
        const int4 pr = candi[c];
        if (pr.x < 0) {                                      // a dropped explicit pair (uniform over the workgroup)
            if (tid == 0) cande[c] = make_float2(__builtin_inff(), __int_as_float(0));
            continue;
        }
        ds_load_pair(tab, pr.z, pr.w, false, false, lA, lB, lcb, tid);
        __syncthreads();
        float best = __builtin_inff();
        int bi = 0x7fffffff;
        for (int idx = tid; idx < DS_PTS; idx += DS_T) {
            const float e = ds_point(lA, lB, lcb, idx, nullptr, nullptr);
            if (e < best) { best = e; bi = idx; }
        }
        ds_argmin(best, bi, rv, ri, tid);
        if (tid == 0) cande[c] = make_float2(best, __int_as_float(bi));
    }
}

__global__ void __launch_bounds__(DS_T)
k_ds_match(int N, const int32_t *__restrict__ seg_off, int cap, const int32_t *__restrict__ head, const int4 *__restrict__ candi,
           const float2 *__restrict__ cande, float max_energy, int32_t *partner, int32_t *__restrict__ count) {
    __shared__ float rv[DS_T];
    __shared__ int ri[DS_T];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int found = head[1];
    if (found > cap) {                                       // more pairs within cb_max than the list holds: nothing is bonded
        if (tid == 0) count[s] = -1;
        return;
    }
    int lo, hi;
    pp_seg_rows(seg_off, s, N, lo, hi);
    volatile int32_t *pv = partner;
    int nb = 0;
    for (;;) {
        // the smallest (Emin, a, b) among the segment's candidates whose rows are both free: value first, then the rows
        float best = __builtin_inff();
        int bc = 0x7fffffff, ba = 0x7fffffff, bb = 0x7fffffff;
        for (int c = tid; c < found; c += DS_T) {
            const int4 pr = candi[c];
            if (pr.x < lo || pr.x >= hi) continue;
            const float e = cande[c].x;
            if (!(e <= max_energy) || pv[pr.x] >= 0 || pv[pr.y] >= 0) continue;
            if (bc == 0x7fffffff || e < best || (e == best && (pr.x < ba || (pr.x == ba && pr.y < bb)))) { best = e; bc = c; ba = pr.x; bb = pr.y; }
        }
        // two rounds: the value with the smaller first row, then, among the lanes that hold that (value, a), the smaller second row
        float v1 = bc == 0x7fffffff ? __builtin_inff() : best;
        int i1 = ba;
        ds_argmin(v1, i1, rv, ri, tid);
        if (i1 == 0x7fffffff) break;                         // no candidate left (uniform: every lane reads the same word)
        float v2 = (bc != 0x7fffffff && best == v1 && ba == i1) ? 0.f : __builtin_inff();
        int i2 = (bc != 0x7fffffff && best == v1 && ba == i1) ? bb : 0x7fffffff;
        ds_argmin(v2, i2, rv, ri, tid);
        if (tid == 0) { partner[i1] = i2; partner[i2] = i1; }
        nb++;
        __threadfence();
        __syncthreads();
    }
    if (tid == 0) count[s] = nb;
}

__global__ void __launch_bounds__(DS_T)
k_ds_close(int cap, const int32_t *__restrict__ head, const int4 *__restrict__ candi, const float2 *__restrict__ cande,
           const float4 *__restrict__ tab, const int32_t *__restrict__ partner, const float *__restrict__ chi,
           const uint8_t *__restrict__ fixed, float max_energy, float sigma2, float *__restrict__ chi_out, float *__restrict__ report) {
    __shared__ float4 lA[DS_G], lB[DS_G];
    __shared__ float lcb[2][4];
    __shared__ float rv[DS_T];
    __shared__ int ri[DS_T];
    const int tid = threadIdx.x;
    const int found = head[1];
    if (found > cap) return;
    for (int c = blockIdx.x; c < found; c += gridDim.x) {
        const int4 pr = candi[c];
        if (pr.x < 0) continue;
        const float emin = cande[c].x;
        if (!(emin <= max_energy) || partner[pr.x] != pr.y || partner[pr.y] != pr.x) continue;      // uniform over the workgroup
        const bool fa = fixed && fixed[pr.x] != 0, fb = fixed && fixed[pr.y] != 0;
        ds_load_pair(tab, pr.z, pr.w, fa, fb, lA, lB, lcb, tid);
        __syncthreads();
        float e[DS_PER];
        float best = __builtin_inff();
        int bi = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < DS_PER; u++) {
            const int idx = tid + DS_T * u;
            e[u] = __builtin_inff();
            if (idx < DS_PTS) {
                e[u] = ds_point(lA, lB, lcb, idx, nullptr, nullptr);
                if (e[u] < best) { best = e[u]; bi = idx; }
            }
        }
        ds_argmin(best, bi, rv, ri, tid);                    // best = Emin_r, the minimum over the restricted grid
        float thr = fminf(max_energy, best + 4.f);
        thr = thr < best ? best : thr;
        const float chia = tab[(size_t)pr.z * DS_TAB + 75].x, chib = tab[(size_t)pr.w * DS_TAB + 75].x;
        float jb = __builtin_inff();
        int ji = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < DS_PER; u++) {
            const int idx = tid + DS_T * u;
            if (idx < DS_PTS && e[u] <= thr) {
                float j = e[u];
                if (chi) {
                    const int p = idx / DS_G, q = idx - p * DS_G;
                    const float wa = fa ? 0.f : ds_wrap(ds_theta(p) - chia), wb = fb ? 0.f : ds_wrap(ds_theta(q) - chib);
                    j = e[u] + (((wa * wa) + (wb * wb)) / sigma2);
                }
                if (j < jb) { jb = j; ji = idx; }
            }
        }
        ds_argmin(jb, ji, rv, ri, tid);
        if (tid == 0) {
            float r1 = __builtin_inff(), r2 = 0.f, r3 = 0.f;
            if (ji < DS_PTS) {
                r1 = ds_point(lA, lB, lcb, ji, &r2, &r3);
                const int p = ji / DS_G, q = ji - p * DS_G;
                if (chi_out && !fa) chi_out[(size_t)pr.x * 4] = ds_theta(p);
                if (chi_out && !fb) chi_out[(size_t)pr.y * 4] = ds_theta(q);
            }
            float *ra = report + (size_t)pr.x * 4, *rb = report + (size_t)pr.y * 4;
            ra[0] = emin; ra[1] = r1; ra[2] = r2; ra[3] = r3;
            rb[0] = emin; rb[1] = r1; rb[2] = r2; rb[3] = r3;
        }
        __syncthreads();
    }
}

static size_t ds_align(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" pp_status pp_disulfide_close(pp_ctx *c, const float *chi, const uint8_t *fixed, const int32_t *pairs, int n_pairs,
                                        float cb_max, float max_energy, float sigma_chi, float *chi_out, int32_t *partner,
                                        float *report, int32_t *count, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !partner || !report || !count) FAIL(PP_ERR_INVALID, "pp_disulfide_close: null argument");
    if (!c->b.X || !c->b.atom_mask || !c->b.residue_type || !c->b.residue_mask)
        FAIL(PP_ERR_INVALID, "pp_disulfide_close: needs a batch with X, atom_mask, residue_type and residue_mask");
    if (!chi && (chi_out || fixed)) FAIL(PP_ERR_INVALID, "pp_disulfide_close: chi_out and fixed need chi");
    if (n_pairs < 0 || (n_pairs > 0 && !pairs)) FAIL(PP_ERR_INVALID, "pp_disulfide_close: n_pairs needs pairs");
    const bool listed = pairs != nullptr;
    if (!listed && (!std::isfinite(cb_max) || !(cb_max > 0.f) || std::isnan(max_energy)))
        FAIL(PP_ERR_INVALID, "pp_disulfide_close: cb_max must be finite and positive, max_energy a number");
    if (chi && (!std::isfinite(sigma_chi) || !(sigma_chi > 0.f)))
        FAIL(PP_ERR_INVALID, "pp_disulfide_close: sigma_chi must be finite and positive");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t N = (size_t)c->N;
    PP_HIP_CHECK(hipMemsetAsync(count, 0, (size_t)c->B * sizeof(int32_t), st));
    if (c->N < 1) return PP_OK;
    // the candidate list: every pair of rows up to N = 129, 64 per row beyond
    const unsigned long long all = (unsigned long long)N * (N - 1) / 2, lin = 64ull * N;
    const int cap = (int)std::max<unsigned long long>(1, std::min(all, std::min<unsigned long long>(lin, 0x7fffff00ull)));
    if (n_pairs > cap)
        FAIL(PP_ERR_INVALID, "pp_disulfide_close: " + std::to_string(n_pairs) + " pairs, the candidate list of this context holds " +
                                 std::to_string(cap));
    const size_t o_eidx = 0, o_erow = o_eidx + ds_align(N * 4), o_head = o_erow + ds_align(N * 4), o_tab = o_head + 256,
                 o_ci = o_tab + ds_align(N * DS_TAB * sizeof(float4)), o_ce = o_ci + ds_align((size_t)cap * sizeof(int4)),
                 total = o_ce + ds_align((size_t)cap * sizeof(float2));
    // total is a function of N alone (cap is), and N of a context never changes: the helper's size check never fires here
    void *wsp;
    if (pp_status rc = pp_ctx_workspace(c, PP_WS_DISULFIDE, total, &wsp)) return rc;
    char *ws = static_cast<char *>(wsp);
    int32_t *eidx = reinterpret_cast<int32_t *>(ws + o_eidx), *erow = reinterpret_cast<int32_t *>(ws + o_erow),
            *head = reinterpret_cast<int32_t *>(ws + o_head);
    float4 *tab = reinterpret_cast<float4 *>(ws + o_tab);
    int4 *candi = reinterpret_cast<int4 *>(ws + o_ci);
    float2 *cande = reinterpret_cast<float2 *>(ws + o_ce);

    PP_HIP_CHECK(hipMemsetAsync(partner, 0xff, N * sizeof(int32_t), st));
    PP_HIP_CHECK(hipMemsetAsync(report, 0, N * 4 * sizeof(float), st));
    if (chi_out && chi_out != chi) PP_HIP_CHECK(hipMemcpyAsync(chi_out, chi, N * 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
    const pp_plan *p = c->plan;
    const float me = listed ? INFINITY : max_energy;
    const int rows_grid = (c->N + DS_T - 1) / DS_T, pair_grid = cap < 2048 ? cap : 2048;
    hipLaunchKernelGGL(k_ds_rows, dim3(1), dim3(DS_T), 0, st, c->N, c->b.residue_type, c->b.residue_mask, c->b.atom_mask, eidx, erow, head);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ds_tables, dim3(c->N), dim3(128), 0, st, c->N, c->b.X, c->b.residue_type, chi, eidx, p->default_frames,
                       p->atom14_to_group, p->lit_positions, tab);
    PP_HIP_CHECK(hipGetLastError());
    if (listed)
        hipLaunchKernelGGL(k_ds_pairs, dim3(n_pairs / DS_T + 1), dim3(DS_T), 0, st, c->N, c->B, c->seg_off, eidx, pairs, n_pairs, head,
                           candi);
    else
        hipLaunchKernelGGL(k_ds_cand, dim3(rows_grid), dim3(DS_T), 0, st, c->N, c->B, c->seg_off, erow, tab, cb_max, cap, head, candi);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ds_scan, dim3(pair_grid), dim3(DS_T), 0, st, cap, head, candi, tab, cande);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ds_match, dim3(c->B), dim3(DS_T), 0, st, c->N, c->seg_off, cap, head, candi, cande, me, partner, count);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ds_close, dim3(pair_grid), dim3(DS_T), 0, st, cap, head, candi, cande, tab, partner, chi, fixed, me,
                       sigma_chi * sigma_chi, chi_out, report);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
