// Anchors (no reference kernel): distance restraints, optionally with an angle term, between a side-chain atom
// and a fixed point -- a metal ion, or the atom of a ligand the residue is covalently linked to.  pp_disulfide_close closes the one
// bond side chains make with each other; this closes the ones they make with everything else: one row, up to four chi, a fixed target.
//
// DEFINITION.  Arithmetic is fp32 with fp contract off.  Each row's result is a function of that row's data and its anchors only.
//   ANCHOR i has: row, the row it belongs to; slot, the donor atom14 slot, 5..13; ante, the slot of the same row the donor is bonded
//     to, 0..13; target, xyz in the batch's coordinates; d0 and sigma_d in A; theta0 and sigma_theta in degrees.  sigma_theta <= 0 means
//     no angle term.  A row may carry at most PP_ANCHOR_PER_ROW = 4 anchors.  They are taken in list order.
//   VALID means all of: row is in range and residue_mask != 0; atom_mask of N, CA, C, slot and ante is non-zero; the rigid group of
//     slot (a2g) is a chi group, 4..7 (CB never moves); ante != slot; target, d0, sigma_d > 0, theta0 and sigma_theta are finite.
//     An invalid entry, or a fifth anchor on a row, is dropped on the device and the row's status becomes -2.  The Python layer
//     refuses it by name before the call.  (Here: a residue_type outside 0..20 makes the entry invalid too -- it is never used as an
//     index --, an entry whose row is out of range marks no row, and "fifth" counts the VALID entries of the row in list order.)
//   GEOMETRY.  The row's atoms are built as pp_atom14 builds them: backbone frame, default frames of the rigid groups, rotation about x
//     by chi, literature positions.  They are built relative to the row's CA, and the target is taken as target - CA once (pp_shell's
//     and pp_disulfide's habit, so a structure far from the origin loses nothing).  With G the backbone frame (e0 along C - CA, e1
//     from N - CA, 1e-8 inside both roots, no translation), T_g(s, c) = D_g o Rx the torsion frame of group g at the normalised sine
//     and cosine of its angle:  F_4 = G o T_4,  F_g = F_(g-1) o T_g  (composed left to right),  atom = (F_g.R l + F_g.t) atom14_mask.
//     A backbone antecedent (slots 0..3) is X[ante] - CA; CB is group 0 at angle 0.  (The standard tables put no other side-chain
//     atom outside the groups 4..7; one that a caller's tables put there is built at angle 0 of its group.)
//   GRID.  n = the largest (group - 3) over the row's valid anchors: the number of chi the row's donors depend on, 1..4.
//     g(n) = 72, 72, 36, 24.  theta_k = (float)(-pi + 2 pi k / g).  A point is (k1..kn) with flat index ((k1 g + k2) g + k3) g + k4,
//     truncated to n digits.  Chi beyond n keep the caller's value (0 without chi).
//   ENERGY.  Sum over the row's valid anchors in list order of
//       ((|A - q| - d0) / sigma_d)^2 + ((ang(P, A, q) - theta0) / sigma_theta)^2
//     where A is the donor, P its antecedent and q the target.  ang is section 26's, in degrees.  A NaN never wins a minimum.
//   CLOSURE.  Emin = the minimum over the grid.  If Emin > max_energy, the row is open: status -1 and chi_out row = chi row bit for
//     bit.  Otherwise thr = max(Emin, min(max_energy, Emin + 4)) and F = {E <= thr}.
//     J = E + (sum over k <= n, left to right, of wrap(theta - chi[row][k])^2) / sigma_chi^2.  chi NULL means J = E.
//     The pick is the argmin of J over F, ties to the lowest flat index.  chi_out = chi bit for bit except the first n chi of closed
//     rows.  A fixed row is kept: status 2.  Its E, distance and angle at its own angles are reported and nothing is written.
//   OUTPUTS, on the device, one writer per word, no read-back, the call never waits for the stream:
//     status int32 [N]: 0 none, 1 closed, 2 kept, -1 open, -2 an entry of this row was dropped (the row is closed, kept or left open
//       by its other anchors all the same: chi_out and the reports say which).
//     report float [N][4] = (Emin, E at the pick, the first anchor's distance, the first anchor's angle); an open row has Emin alone,
//       a kept row its E twice.
//     anchor_report float [A][2] = distance and angle of every anchor at its row's pick; 0 for a dropped entry or an open row.
//     count int32 [n_seg] = rows of status 1 per segment of the context's segment table.
//     chi_out, which may be chi itself.
//
// LAUNCH, all on the caller's stream:
//   k_an_mark   one lane per anchor: valid or not; an invalid entry marks its row (integer atomic OR of one bit)
//   k_an_slots  one lane per valid anchor: its place among the row's valid anchors (a walk over the entries in front of it); the first
//               four go into the row's list, a later one marks the row
//   k_an_rows   one workgroup: the rows with a list or a mark in ascending order (a block scan per 256 rows)
//   k_an_close  one 256-lane workgroup per such row (the host launches min(N, A); the others leave at once).  The torsion frames of
//               the grid angles of all four groups lie in LDS (14 KB); a lane takes the points of one (k1, k2) at a time, composes
//               F_5 once and F_6 once per k3, so its inner loop is one composition and the anchors' atoms.  Two passes: Emin, then the
//               argmin of J over F with E computed again (nothing is stored per point).  Both reductions are the (value, index) LDS
//               tree: the result does not depend on the lane order.  No float atomics.
//   k_an_count  one workgroup per segment: the rows of status 1, an integer tree
// CAPACITY.  A <= 8 N (PP_ERR_INVALID beyond): the workspace, one allocation outside the arena made by the first call and freed with
// the context, is sized from N alone.
#include "pp_internal.h"
#include "pp_vec.h"
#include <algorithm>
#pragma clang fp contract(off)

#define AN_T 256
#define AN_GMAX 72
#define AN_RAD2DEG_F 57.29577951308232087680f
#define AN_TWO_PI_F 6.28318530717958647692f

struct AnF {                 // x -> r x + t, r row-major
    float r[9], t[3];
};
struct AnAnchor {            // one valid anchor of the row, as the grid reads it
    float la[3], lp[3];      // literature position of the donor; of the antecedent, or its fixed position relative to CA (gp < 0)
    float q[3];              // target - CA
    float d0, sd, th0, st, ama, amp;
    int ga, gp;              // donor's group 4..7; antecedent's group 4..7, or -1: lp is the position itself
    int idx;                 // the entry's index in the caller's list
};

__host__ __device__ __forceinline__ int an_grid(int n) { return n <= 2 ? 72 : (n == 3 ? 36 : 24); }
__device__ __forceinline__ float an_theta(int k, int g) { return (float)(-PP_PI_D + 2.0 * PP_PI_D * (double)k / (double)g); }
__device__ __forceinline__ float an_wrap(float x) { return x - (rintf(x / AN_TWO_PI_F) * AN_TWO_PI_F); }
__device__ __forceinline__ float an_sq(float x) { return x * x; }

__device__ __forceinline__ AnF an_compose(const AnF &a, const AnF &b) {
    AnF o;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) o.r[3 * i + j] = ((a.r[3 * i] * b.r[j]) + (a.r[3 * i + 1] * b.r[3 + j])) + (a.r[3 * i + 2] * b.r[6 + j]);
        o.t[i] = (((a.r[3 * i] * b.t[0]) + (a.r[3 * i + 1] * b.t[1])) + (a.r[3 * i + 2] * b.t[2])) + a.t[i];
    }
    return o;
}
// D o Rx(angle) for a default frame D (row-major 4 x 4) and the normalised (sin, cos)
__device__ __forceinline__ AnF an_torsion(const float *D, float sn, float cs) {
    AnF o;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        o.r[3 * i] = D[4 * i];
        o.r[3 * i + 1] = (D[4 * i + 1] * cs) + (D[4 * i + 2] * sn);
        o.r[3 * i + 2] = (D[4 * i + 2] * cs) - (D[4 * i + 1] * sn);
        o.t[i] = D[4 * i + 3];
    }
    return o;
}
__device__ __forceinline__ void an_sincos(float ang, float &sn, float &cs) {
    const float s0 = sinf(ang), c0 = cosf(ang);
    const float den = sqrtf(fmaxf((s0 * s0) + (c0 * c0), 1e-12f));
    sn = s0 / den; cs = c0 / den;
}
__device__ __forceinline__ AnF an_load(const float *p) {
    AnF o;
#pragma unroll
    for (int i = 0; i < 9; i++) o.r[i] = p[i];
#pragma unroll
    for (int i = 0; i < 3; i++) o.t[i] = p[9 + i];
    return o;
}
__device__ __forceinline__ void an_store(float *p, const AnF &f) {
#pragma unroll
    for (int i = 0; i < 9; i++) p[i] = f.r[i];
#pragma unroll
    for (int i = 0; i < 3; i++) p[9 + i] = f.t[i];
}
// (F_g.R l + F_g.t) am with the frame of group g chosen by selects (g is uniform over the workgroup)
__device__ __forceinline__ void an_atom(const AnF &f4, const AnF &f5, const AnF &f6, const AnF &f7, int g, const float *l, float am, float *p) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float r0 = g == 4 ? f4.r[3 * i] : g == 5 ? f5.r[3 * i] : g == 6 ? f6.r[3 * i] : f7.r[3 * i];
        const float r1 = g == 4 ? f4.r[3 * i + 1] : g == 5 ? f5.r[3 * i + 1] : g == 6 ? f6.r[3 * i + 1] : f7.r[3 * i + 1];
        const float r2 = g == 4 ? f4.r[3 * i + 2] : g == 5 ? f5.r[3 * i + 2] : g == 6 ? f6.r[3 * i + 2] : f7.r[3 * i + 2];
        const float t = g == 4 ? f4.t[i] : g == 5 ? f5.t[i] : g == 6 ? f6.t[i] : f7.t[i];
        p[i] = ((((r0 * l[0]) + (r1 * l[1])) + (r2 * l[2])) + t) * am;
    }
}
// angle at V between P - V and Q - V, degrees (pp_disulfide.hip's ds_angle)
__device__ __forceinline__ float an_angle(const float *P, const float *V, const float *Q) {
    float u[3], v[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { u[k] = P[k] - V[k]; v[k] = Q[k] - V[k]; }
    float c = pp_dot3(u[0], u[1], u[2], v[0], v[1], v[2]) /
              (sqrtf(pp_dot3(u[0], u[1], u[2], u[0], u[1], u[2])) * sqrtf(pp_dot3(v[0], v[1], v[2], v[0], v[1], v[2])));
    c = c > 1.f ? 1.f : (c < -1.f ? -1.f : c);
    return acosf(c) * AN_RAD2DEG_F;
}
// E of the row at the frames given; distance and angle of every anchor on request (the angle is computed there with or without a term)
__device__ __forceinline__ float an_energy(const AnF &f4, const AnF &f5, const AnF &f6, const AnF &f7, const AnAnchor *an, int na,
                                           float *dist, float *ang) {
    float e = 0.f;
    for (int i = 0; i < na; i++) {
        const AnAnchor &a = an[i];
        float A[3], P[3];
        an_atom(f4, f5, f6, f7, a.ga, a.la, a.ama, A);
        if (a.gp < 0) { P[0] = a.lp[0]; P[1] = a.lp[1]; P[2] = a.lp[2]; }
        else an_atom(f4, f5, f6, f7, a.gp, a.lp, a.amp, P);
        const float dx = A[0] - a.q[0], dy = A[1] - a.q[1], dz = A[2] - a.q[2];
        const float d = sqrtf(pp_dot3(dx, dy, dz, dx, dy, dz));
        float t = an_sq((d - a.d0) / a.sd);
        if (a.st > 0.f || ang) {
            const float th = an_angle(P, A, a.q);
            if (a.st > 0.f) t = t + an_sq((th - a.th0) / a.st);
            if (ang) ang[i] = th;
        }
        if (dist) dist[i] = d;
        e = i == 0 ? t : e + t;
    }
    return e;
}

// argmin on (value, index) over the workgroup (pp_disulfide.hip's ds_argmin): the smaller value, on equal values the smaller index,
// whatever the lane order; a lane without an entry brings (+inf, INT_MAX); a NaN never wins against a number
__device__ __forceinline__ void an_argmin(float &v, int &i, float *rv, int *ri, int tid) {
    rv[tid] = v; ri[tid] = i;
    __syncthreads();
    for (int w = AN_T / 2; w > 0; w >>= 1) {
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

__device__ __forceinline__ bool an_valid(int N, int4 e, float4 tg, float4 pr, const int64_t *__restrict__ rtype,
                                         const float *__restrict__ rmask, const float *__restrict__ amask, const int32_t *__restrict__ a2g) {
    if (e.x < 0 || e.x >= N || e.y < 5 || e.y > 13 || e.z < 0 || e.z > 13 || e.y == e.z) return false;
    const int64_t S = rtype[e.x];
    if (S < 0 || S > 20 || rmask[e.x] == 0.f) return false;
    const float *am = amask + (size_t)e.x * 14;
    if (am[0] == 0.f || am[1] == 0.f || am[2] == 0.f || am[e.y] == 0.f || am[e.z] == 0.f) return false;
    const int g = a2g[(int)S * 14 + e.y];
    if (g < 4 || g > 7) return false;
    return pp_finite(tg.x) && pp_finite(tg.y) && pp_finite(tg.z) && pp_finite(pr.x) && pp_finite(pr.y) && pr.y > 0.f && pp_finite(pr.z) &&
           pp_finite(pr.w);
}

__global__ void __launch_bounds__(AN_T)
k_an_mark(int N, int A, const int4 *__restrict__ ai, const float4 *__restrict__ at, const float4 *__restrict__ ap,
          const int64_t *__restrict__ rtype, const float *__restrict__ rmask, const float *__restrict__ amask,
          const int32_t *__restrict__ a2g, int32_t *__restrict__ vflag, int32_t *__restrict__ bad) {
    const int i = blockIdx.x * AN_T + threadIdx.x;
    if (i >= A) return;
    const int4 e = ai[i];
    const bool ok = an_valid(N, e, at[i], ap[i], rtype, rmask, amask, a2g);
    vflag[i] = ok ? 1 : 0;
    if (!ok && e.x >= 0 && e.x < N) atomicOr(&bad[e.x], 1);
}

__global__ void __launch_bounds__(AN_T)
k_an_slots(int A, const int4 *__restrict__ ai, const int32_t *__restrict__ vflag, int32_t *__restrict__ rowanch, int32_t *__restrict__ bad) {
    const int i = blockIdx.x * AN_T + threadIdx.x;
    if (i >= A || !vflag[i]) return;
    const int row = ai[i].x;                                  // in range: the entry is valid
    int k = 0;
    for (int j = 0; j < i; j++) k += (vflag[j] && ai[j].x == row) ? 1 : 0;
    if (k < PP_ANCHOR_PER_ROW) rowanch[(size_t)row * PP_ANCHOR_PER_ROW + k] = i;
    else atomicOr(&bad[row], 1);
}

__global__ void __launch_bounds__(AN_T)
k_an_rows(int N, const int32_t *__restrict__ rowanch, const int32_t *__restrict__ bad, int32_t *__restrict__ arow, int32_t *__restrict__ head) {
    __shared__ int sc[AN_T];
    __shared__ int s_base;
    const int tid = threadIdx.x;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int base = 0; base < N; base += AN_T) {
        const int n = base + tid;
        const int f = (n < N && (rowanch[(size_t)n * PP_ANCHOR_PER_ROW] >= 0 || bad[n] != 0)) ? 1 : 0;
        sc[tid] = f;
        __syncthreads();
        for (int o = 1; o < AN_T; o <<= 1) {
            const int v = tid >= o ? sc[tid - o] : 0;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        const int b0 = s_base;
        if (f) arow[b0 + sc[tid] - 1] = n;
        __syncthreads();
        if (tid == AN_T - 1) s_base = b0 + sc[AN_T - 1];
        __syncthreads();
    }
    if (tid == 0) head[0] = s_base;
}

// one pass over the row's grid: SECOND = false the minimum of E, true the minimum of J over {E <= thr}
template <bool SECOND>
__device__ __forceinline__ void an_scan(int n, int g, int gmax, const float (*sT)[AN_GMAX][12], const float (*sOwn)[12],
                                        const float (*sW)[AN_GMAX], const AnAnchor *an, int na, float thr, bool with_chi, float sigma2,
                                        int tid, float &best, int &bi) {
    const int no = n >= 2 ? g * g : g, n3 = n >= 3 ? g : 1, n4 = n == 4 ? g : 1;
    best = __builtin_inff();
    bi = 0x7fffffff;
    for (int o = tid; o < no; o += AN_T) {
        const int k1 = n >= 2 ? o / g : o, k2 = n >= 2 ? o - k1 * g : 0;
        const AnF f4 = an_load(sT[0][k1]);
        AnF f5 = f4, f6 = f4, f7 = f4;
        if (gmax >= 5) f5 = an_compose(f4, an_load(n >= 2 ? sT[1][k2] : sOwn[1]));
        const float w12 = n >= 2 ? sW[0][k1] + sW[1][k2] : sW[0][k1];
        for (int k3 = 0; k3 < n3; k3++) {
            if (gmax >= 6) f6 = an_compose(f5, an_load(n >= 3 ? sT[2][k3] : sOwn[2]));
            const float w123 = n >= 3 ? w12 + sW[2][k3] : w12;
            for (int k4 = 0; k4 < n4; k4++) {
                if (gmax >= 7) f7 = an_compose(f6, an_load(n == 4 ? sT[3][k4] : sOwn[3]));
                const int idx = (o * n3 + k3) * n4 + k4;
                const float e = an_energy(f4, f5, f6, f7, an, na, nullptr, nullptr);
                if (!SECOND) {
                    if (e < best) { best = e; bi = idx; }
                } else if (e <= thr) {
                    float j = e;
                    if (with_chi) j = e + ((n == 4 ? w123 + sW[3][k4] : w123) / sigma2);
                    if (j < best) { best = j; bi = idx; }
                }
            }
        }
    }
}

__global__ void __launch_bounds__(AN_T)
k_an_close(int N, const float *__restrict__ X, const int64_t *__restrict__ rtype, const float *chi /* may be chi_out */,
           const uint8_t *__restrict__ fixed, const int4 *__restrict__ ai, const float4 *__restrict__ at, const float4 *__restrict__ ap,
           const int32_t *__restrict__ head, const int32_t *__restrict__ arow, const int32_t *__restrict__ rowanch,
           const int32_t *__restrict__ bad, const float *__restrict__ default_frames, const int32_t *__restrict__ a2g,
           const float *__restrict__ amask14, const float *__restrict__ lit, float max_energy, float sigma2, float *chi_out,
           int32_t *__restrict__ status, float *__restrict__ report, float *__restrict__ areport) {
    __shared__ __attribute__((aligned(16))) float sT[4][AN_GMAX][12];      // torsion frames of the grid angles, group 4 composed with G
    __shared__ __attribute__((aligned(16))) float sOwn[4][12];             // the same at the row's own angles
    __shared__ float sW[4][AN_GMAX];                                       // wrap(theta_k - own chi)^2
    __shared__ float sG[12];
    __shared__ float sOwnChi[4];
    __shared__ AnAnchor sA[PP_ANCHOR_PER_ROW];
    __shared__ int s_na, s_n, s_gmax;
    __shared__ float rv[AN_T];
    __shared__ int ri[AN_T];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= head[0]) return;
    const int row = arow[blockIdx.x];
    const int S = (int)rtype[row];                            // 0..20 wherever the row has a valid anchor; not used otherwise
    const float *x = X + (size_t)row * 42;
    if (tid == 0) {
        // backbone frame, columns e0 e1 e2 (pp_atom14's construction), no translation: everything is relative to CA
        float av[3], bv[3], cv[3];
        for (int q = 0; q < 3; q++) { av[q] = x[6 + q] - x[3 + q]; bv[q] = x[q] - x[3 + q]; }
        const float na_ = sqrtf(pp_dot3(av[0], av[1], av[2], av[0], av[1], av[2]) + 1e-8f);
        for (int q = 0; q < 3; q++) av[q] = av[q] / na_;
        const float dt = pp_dot3(av[0], av[1], av[2], bv[0], bv[1], bv[2]);
        for (int q = 0; q < 3; q++) bv[q] = bv[q] - (av[q] * dt);
        const float nb = sqrtf(pp_dot3(bv[0], bv[1], bv[2], bv[0], bv[1], bv[2]) + 1e-8f);
        for (int q = 0; q < 3; q++) bv[q] = bv[q] / nb;
        cv[0] = (av[1] * bv[2]) - (av[2] * bv[1]);
        cv[1] = (av[2] * bv[0]) - (av[0] * bv[2]);
        cv[2] = (av[0] * bv[1]) - (av[1] * bv[0]);
        for (int q = 0; q < 3; q++) { sG[3 * q] = av[q]; sG[3 * q + 1] = bv[q]; sG[3 * q + 2] = cv[q]; sG[9 + q] = 0.f; }
        AnF G = an_load(sG);
        int na = 0, n = 0, gmax = 4;
        for (int k = 0; k < PP_ANCHOR_PER_ROW; k++) {
            const int i = rowanch[(size_t)row * PP_ANCHOR_PER_ROW + k];
            if (i < 0) break;
            const int4 e = ai[i];
            const float4 tg = at[i], pr = ap[i];
            AnAnchor &a = sA[na++];
            a.idx = i;
            a.ga = a2g[S * 14 + e.y];
            a.ama = amask14[S * 14 + e.y];
            a.amp = 1.f;
            for (int q = 0; q < 3; q++) a.la[q] = lit[((size_t)S * 14 + e.y) * 3 + q];
            a.q[0] = tg.x - x[3]; a.q[1] = tg.y - x[4]; a.q[2] = tg.z - x[5];
            a.d0 = pr.x; a.sd = pr.y; a.th0 = pr.z; a.st = pr.w;
            const int gp = a2g[S * 14 + e.z];
            if (e.z < 4) {
                a.gp = -1;
                for (int q = 0; q < 3; q++) a.lp[q] = x[3 * e.z + q] - x[3 + q];
            } else if (gp >= 4 && gp <= 7) {
                a.gp = gp;
                a.amp = amask14[S * 14 + e.z];
                for (int q = 0; q < 3; q++) a.lp[q] = lit[((size_t)S * 14 + e.z) * 3 + q];
            } else {
                // CB (group 0), or an atom a caller's tables put into another group below 4: built once, at angle 0 of its group
                a.gp = -1;
                const int gq = gp < 0 ? 0 : gp;
                const AnF F = an_compose(G, an_torsion(default_frames + ((size_t)S * 8 + gq) * 16, 0.f, 1.f));
                const float *l = lit + ((size_t)S * 14 + e.z) * 3;
                const float am = amask14[S * 14 + e.z];
                for (int q = 0; q < 3; q++) a.lp[q] = ((((F.r[3 * q] * l[0]) + (F.r[3 * q + 1] * l[1])) + (F.r[3 * q + 2] * l[2])) + F.t[q]) * am;
            }
            n = a.ga - 3 > n ? a.ga - 3 : n;
            gmax = a.ga > gmax ? a.ga : gmax;
            gmax = a.gp > gmax ? a.gp : gmax;
        }
        s_na = na; s_n = n; s_gmax = gmax;
    }
    if (tid < 4) sOwnChi[tid] = chi ? chi[(size_t)row * 4 + tid] : 0.f;
    __syncthreads();
    const int na = s_na, n = s_n, gmax = s_gmax;
    const bool dropped = bad[row] != 0;
    if (na == 0) {                                            // only dropped entries (uniform over the workgroup)
        if (tid == 0) status[row] = -2;
        return;
    }
    const int g = an_grid(n);
    {
        const AnF G = an_load(sG);
        for (int j = tid; j < 4 * g; j += AN_T) {
            const int grp = j / g, k = j - grp * g;
            const float th = an_theta(k, g);
            float sn, cs;
            an_sincos(th, sn, cs);
            AnF T = an_torsion(default_frames + ((size_t)S * 8 + 4 + grp) * 16, sn, cs);
            if (grp == 0) T = an_compose(G, T);
            an_store(sT[grp][k], T);
            sW[grp][k] = an_sq(an_wrap(th - sOwnChi[grp]));
        }
        if (tid < 4) {
            float sn, cs;
            an_sincos(sOwnChi[tid], sn, cs);
            AnF T = an_torsion(default_frames + ((size_t)S * 8 + 4 + tid) * 16, sn, cs);
            if (tid == 0) T = an_compose(G, T);
            an_store(sOwn[tid], T);
        }
    }
    __syncthreads();
    const bool kept = fixed && fixed[row] != 0;
    float emin = 0.f, jb = 0.f;
    int ei = 0, ji = 0x7fffffff;
    if (!kept) {
        an_scan<false>(n, g, gmax, sT, sOwn, sW, sA, na, 0.f, false, 1.f, tid, emin, ei);
        an_argmin(emin, ei, rv, ri, tid);
        if (!(emin > max_energy)) {
            float thr = fminf(max_energy, emin + 4.f);
            thr = thr < emin ? emin : thr;
            an_scan<true>(n, g, gmax, sT, sOwn, sW, sA, na, thr, chi != nullptr, sigma2, tid, jb, ji);
            an_argmin(jb, ji, rv, ri, tid);
        }
    }
    if (tid != 0) return;
    // one lane reports: the frames at the pick (a kept row: at its own angles) through the operations of the grid, so E is the grid's
    const bool closed = !kept && ji != 0x7fffffff;
    float dist[PP_ANCHOR_PER_ROW], ang[PP_ANCHOR_PER_ROW];
    float *rp = report + (size_t)row * 4;
    if (kept || closed) {
        int k[4] = {0, 0, 0, 0};
        if (closed) {
            int r = ji;
            for (int q = n - 1; q >= 0; q--) { k[q] = r % g; r /= g; }
        }
        const AnF f4 = an_load(closed ? sT[0][k[0]] : sOwn[0]);
        AnF f5 = f4, f6 = f4, f7 = f4;
        if (gmax >= 5) f5 = an_compose(f4, an_load(closed && n >= 2 ? sT[1][k[1]] : sOwn[1]));
        if (gmax >= 6) f6 = an_compose(f5, an_load(closed && n >= 3 ? sT[2][k[2]] : sOwn[2]));
        if (gmax >= 7) f7 = an_compose(f6, an_load(closed && n == 4 ? sT[3][k[3]] : sOwn[3]));
        const float e = an_energy(f4, f5, f6, f7, sA, na, dist, ang);
        rp[0] = kept ? e : emin; rp[1] = e; rp[2] = dist[0]; rp[3] = ang[0];
        for (int i = 0; i < na; i++) { areport[(size_t)sA[i].idx * 2] = dist[i]; areport[(size_t)sA[i].idx * 2 + 1] = ang[i]; }
        if (closed && chi_out)
            for (int q = 0; q < n; q++) chi_out[(size_t)row * 4 + q] = an_theta(k[q], g);
    } else {
        rp[0] = emin;
    }
    status[row] = dropped ? -2 : (kept ? 2 : (closed ? 1 : -1));
}

__global__ void __launch_bounds__(AN_T)
k_an_count(int N, const int32_t *__restrict__ seg_off, const int32_t *__restrict__ status, int32_t *__restrict__ count) {
    __shared__ int sc[AN_T];
    const int s = blockIdx.x, tid = threadIdx.x;
    int lo, hi;
    pp_seg_rows(seg_off, s, N, lo, hi);
    int c = 0;
    for (int r = lo + tid; r < hi; r += AN_T) c += status[r] == 1 ? 1 : 0;
    sc[tid] = c;
    __syncthreads();
    for (int w = AN_T / 2; w > 0; w >>= 1) {
        if (tid < w) sc[tid] += sc[tid + w];
        __syncthreads();
    }
    if (tid == 0) count[s] = sc[0];
}

static size_t an_align(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" pp_status pp_anchor_close(pp_ctx *c, const float *chi, const uint8_t *fixed, const int32_t *anchors_i,
                                     const float *anchors_target, const float *anchors_param, int A, float max_energy, float sigma_chi,
                                     float *chi_out, int32_t *status, float *report, float *anchor_report, int32_t *count, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !status || !report || !count) FAIL(PP_ERR_INVALID, "pp_anchor_close: null argument");
    if (!c->b.X || !c->b.atom_mask || !c->b.residue_type || !c->b.residue_mask)
        FAIL(PP_ERR_INVALID, "pp_anchor_close: needs a batch with X, atom_mask, residue_type and residue_mask");
    if (!chi && (chi_out || fixed)) FAIL(PP_ERR_INVALID, "pp_anchor_close: chi_out and fixed need chi");
    if (A < 0 || (A > 0 && (!anchors_i || !anchors_target || !anchors_param || !anchor_report)))
        FAIL(PP_ERR_INVALID, "pp_anchor_close: A needs anchors_i, anchors_target, anchors_param and anchor_report");
    if (std::isnan(max_energy)) FAIL(PP_ERR_INVALID, "pp_anchor_close: max_energy must be a number");
    if (chi && (!std::isfinite(sigma_chi) || !(sigma_chi > 0.f)))
        FAIL(PP_ERR_INVALID, "pp_anchor_close: sigma_chi must be finite and positive");
    const size_t N = (size_t)c->N;
    const unsigned long long cap = std::min<unsigned long long>(8ull * N, 0x7fffff00ull);
    if ((unsigned long long)A > cap)
        FAIL(PP_ERR_INVALID, "pp_anchor_close: " + std::to_string(A) + " anchors, a context of " + std::to_string(N) + " rows takes " +
                                 std::to_string(cap));
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PP_HIP_CHECK(hipMemsetAsync(count, 0, (size_t)c->B * sizeof(int32_t), st));
    if (c->N < 1) return PP_OK;
    PP_HIP_CHECK(hipMemsetAsync(status, 0, N * sizeof(int32_t), st));
    PP_HIP_CHECK(hipMemsetAsync(report, 0, N * 4 * sizeof(float), st));
    if (chi_out && chi_out != chi) PP_HIP_CHECK(hipMemcpyAsync(chi_out, chi, N * 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (A == 0) return PP_OK;
    PP_HIP_CHECK(hipMemsetAsync(anchor_report, 0, (size_t)A * 2 * sizeof(float), st));
    // sized from N alone (A <= 8 N), and N of a context never changes: the helper's size check never fires here
    const size_t o_rowanch = 0, o_bad = o_rowanch + an_align(N * PP_ANCHOR_PER_ROW * 4), o_arow = o_bad + an_align(N * 4),
                 o_head = o_arow + an_align(N * 4), o_vflag = o_head + 256, total = o_vflag + an_align((size_t)cap * 4);
    void *wsp;
    if (pp_status rc = pp_ctx_workspace(c, PP_WS_ANCHOR, total, &wsp)) return rc;
    char *ws = static_cast<char *>(wsp);
    int32_t *rowanch = reinterpret_cast<int32_t *>(ws + o_rowanch), *bad = reinterpret_cast<int32_t *>(ws + o_bad),
            *arow = reinterpret_cast<int32_t *>(ws + o_arow), *head = reinterpret_cast<int32_t *>(ws + o_head),
            *vflag = reinterpret_cast<int32_t *>(ws + o_vflag);
    PP_HIP_CHECK(hipMemsetAsync(rowanch, 0xff, N * PP_ANCHOR_PER_ROW * 4, st));
    PP_HIP_CHECK(hipMemsetAsync(bad, 0, N * 4, st));
    const pp_plan *p = c->plan;
    const int4 *ai = reinterpret_cast<const int4 *>(anchors_i);
    const float4 *at = reinterpret_cast<const float4 *>(anchors_target), *ap = reinterpret_cast<const float4 *>(anchors_param);
    const int a_grid = (A + AN_T - 1) / AN_T, row_grid = A < c->N ? A : c->N;
    hipLaunchKernelGGL(k_an_mark, dim3(a_grid), dim3(AN_T), 0, st, c->N, A, ai, at, ap, c->b.residue_type, c->b.residue_mask,
                       c->b.atom_mask, p->atom14_to_group, vflag, bad);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_an_slots, dim3(a_grid), dim3(AN_T), 0, st, A, ai, vflag, rowanch, bad);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_an_rows, dim3(1), dim3(AN_T), 0, st, c->N, rowanch, bad, arow, head);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_an_close, dim3(row_grid), dim3(AN_T), 0, st, c->N, c->b.X, c->b.residue_type, chi, fixed, ai, at, ap, head, arow,
                       rowanch, bad, p->default_frames, p->atom14_to_group, p->atom14_mask, p->lit_positions, max_energy,
                       sigma_chi * sigma_chi, chi_out, status, report, anchor_report);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_an_count, dim3(c->B), dim3(AN_T), 0, st, c->N, c->seg_off, status, count);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
