// Solvent-accessible surface (no reference kernel): Shrake-Rupley test points per atom, with four nested
// occluder levels counted in one pass, per segment of the context's segment table (the complexes of a packed ctx, the decoys of a
// group, the B rows of a padded batch).  The reference's interface (src/utils/interface.py: accessible area in the isolated chain
// above that in the complex) needs freesasa; this is the same definition made on the device from the batch itself.
//
// DEFINITION.  An atom (row n, slot a) is PRESENT iff radius[n][a] > 0 (residue_mask is not consulted).  For a present atom with
// centre p_a and test point k (unit vector u_k), the OCCLUDERS are every other present atom of the row's segment and the obstacle
// atoms of the segment with r_o > 0 (pp_ctx_set_obstacles), in four classes:
//   0  another present atom of the same row           2  a present atom of a row of the segment with another chain_indices
//   1  one of another row with the same chain_indices 3  an obstacle atom of the segment
// m(a, k) = the smallest class of an occluder that buries the point, 4 if none does; counts[n][a][L] = #{k : m(a, k) > L}: the
// points left exposed next to the own residue alone (L = 0), in the isolated chain (1), in the complex (2), with the obstacles (3).
// m is a minimum over a set: it depends on no list order, no chunking and no packing.
//
// ARITHMETIC (fp32, every operation rounded on its own: fp contract off), in this order:
//   R_a = r_a + probe;   q = p_a + (R_a u_k) per component;   occluder b: R_b = r_b + probe, d = q - p_b,
//   d2 = ((dx dx) + (dy dy)) + (dz dz);   buried iff d2 < R_b R_b (strict: a NaN buries nothing and is buried by nothing).
//   area[n][L] = sum over ascending present slots a of ((kf R_a) R_a) (float)counts[n][a][L],  kf = (float)(4 pi / P) from the host.
// A NumPy float32 restatement gives the same count bytes (tests/test_sasa_host.py).
//
// LAUNCH.  k_sasa_rows (one lane per row): the row's slot-1 position, the bounding radius of its present atoms around it -- from
// the coordinates given, as pp_shell's sh_row_atoms -- and its largest R.  k_sasa (one 256-thread workgroup per row i): lane t owns
// the (atom, point) items t, t + 256 ... of the 14 P, their points q and their m in registers; an item of an absent atom carries a
// NaN point, which nothing buries.  The workgroup walks the rows of its segment 256 at a time, keeps row j unless
//     d2(CA_i, CA_j) > ((rad_i + rad_j + Rmax_i + Rmax_j) 1.001 + 0.01)^2
// (a point of a can only be buried by b when |p_a - p_b| < R_a + R_b; the slack is pp_shell's, orders above fp32 rounding, so the
// test changes no output word; a NaN keeps the pair), and appends the present atoms of the kept rows to a list in LDS as
// (x, y, z, R_b^2, class); the segment's obstacles follow behind a sphere test against the row's sphere.  Whenever the list could
// overflow PP_SASA_LIST_CAP with the next batch it is DRAINED: every lane runs its items against the list -- all lanes of a wave
// read the same entry, an LDS broadcast -- and lowers its m; then the list refills.  The order of the list comes from an LDS
// atomic and does not matter.  At the end the counts are made with LDS integer atomics; every output word has one writer.
// k_sasa_seg (one workgroup per segment): the fp64 sums of area over the segment's rows in the fixed binary tree of
// k_ens_per_decoy.  No float atomics anywhere.
#include "pp_internal.h"
#include "pp_vec.h"

#define SA_T 256                       // threads of a workgroup
#define SA_STEP 16                     // kept rows whose atoms one append step takes: 16 lanes per row, 14 of them with an atom

// row[8 n + 0..2] = slot 1, [3] = bounding radius of the present atoms around it (-1: none present), [4] = the largest R
__global__ void __launch_bounds__(SA_T)
k_sasa_rows(int N, const float *__restrict__ xyz, const float *__restrict__ radius, float probe, float *__restrict__ row) {
#pragma clang fp contract(off)
    const int n = blockIdx.x * SA_T + threadIdx.x;
    if (n >= N) return;
    const float *p = xyz + (size_t)n * 42;
    float m2 = -1.f, rmax = 0.f;
    bool any = false;
    for (int a = 0; a < 14; a++) {
        const float r = radius[(size_t)n * 14 + a];
        if (r > 0.f) {
            any = true;
            const float d2 = pp_d2(p[3 * a], p[3 * a + 1], p[3 * a + 2], p[3], p[4], p[5]);
            // a NaN sticks: the row is then never pruned.  Not pp_nanmax: that tests the old value first, other instructions for the same value
            m2 = (d2 > m2 || d2 != d2) ? d2 : m2;
            const float R = r + probe;
            rmax = R > rmax ? R : rmax;
        }
    }
    float *o = row + (size_t)n * 8;
    o[0] = p[3]; o[1] = p[4]; o[2] = p[5];
    o[3] = any ? sqrtf(m2) : -1.f;
    o[4] = rmax;
}

// NU: (atom, point) items a lane holds, >= ceil(14 P / 256)
template <int NU>
__global__ void __launch_bounds__(SA_T)
k_sasa(int N, int n_seg, const int32_t *__restrict__ seg_off, const float *__restrict__ xyz, const float *__restrict__ radius,
       const int64_t *__restrict__ chain, const float *__restrict__ rowinfo, const float4 *__restrict__ oatoms,
       const int2 *__restrict__ oseg, const float *__restrict__ points, int P, float probe, float kf, int32_t *__restrict__ counts,
       float *__restrict__ area) {
#pragma clang fp contract(off)
    __shared__ float4 l_atom[PP_SASA_LIST_CAP];
    __shared__ uint8_t l_cls[PP_SASA_LIST_CAP];
    __shared__ float l_pts[PP_SASA_MAX_POINTS * 3];
    __shared__ float l_own[14][4];                           // x, y, z, R (0: the slot is absent)
    __shared__ int l_rows[SA_T];
    __shared__ int l_cnt[14 * 4];
    __shared__ int l_n, l_nrows;
    const int tid = threadIdx.x, i = blockIdx.x;
    if (i >= N) return;

    if (tid < 14) {
        const float r = radius[(size_t)i * 14 + tid];
        const float *p = xyz + (size_t)i * 42 + 3 * tid;
        l_own[tid][0] = p[0]; l_own[tid][1] = p[1]; l_own[tid][2] = p[2];
        l_own[tid][3] = r > 0.f ? r + probe : 0.f;
    }
    if (tid < 14 * 4) l_cnt[tid] = 0;
    if (tid == 0) { l_n = 0; l_nrows = 0; }
    for (int e = tid; e < 3 * P; e += SA_T) l_pts[e] = points[e];
    const int s = pp_seg_of_row(seg_off, n_seg, i);
    int lo, hi;
    pp_seg_rows(seg_off, s, N, lo, hi);
    const float *ri = rowinfo + (size_t)i * 8;
    const float cx = ri[0], cy = ri[1], cz = ri[2], rad_i = ri[3], rmax_i = ri[4];
    // a row without a present atom, or one outside its segment (a table that breaks the contract), has no surface
    if (rad_i < 0.f || i < lo || i >= hi) {
        if (counts && tid < 14 * 4) counts[(size_t)i * 56 + tid] = 0;
        if (tid < 4) area[(size_t)i * 4 + tid] = 0.f;
        return;
    }
    const long long ci = chain[i];
    __syncthreads();

    // this lane's items: point and class so far.  Class 0 -- the own row -- is settled here; the atom itself is left out
    const int n_items = 14 * P;
    const float qnan = __builtin_nanf("");
    float qx[NU], qy[NU], qz[NU];
    int m[NU];
#pragma unroll
    for (int u = 0; u < NU; u++) {
        const int it = tid + SA_T * u;
        qx[u] = qy[u] = qz[u] = qnan;
        m[u] = 0;
        if (it < n_items) {
            const int a = it / P, k = it - a * P;
            const float Ra = l_own[a][3];
            if (Ra > 0.f) {
                const float x = l_own[a][0] + (Ra * l_pts[3 * k]), y = l_own[a][1] + (Ra * l_pts[3 * k + 1]),
                            z = l_own[a][2] + (Ra * l_pts[3 * k + 2]);
                int mm = 4;
                for (int b = 0; b < 14; b++) {
                    const float Rb = l_own[b][3];
                    if (b != a && Rb > 0.f && pp_d2(x, y, z, l_own[b][0], l_own[b][1], l_own[b][2]) < Rb * Rb) mm = 0;
                }
                m[u] = mm;
                if (mm) { qx[u] = x; qy[u] = y; qz[u] = z; }     // a point at class 0 cannot sink further: it rides along as NaN
            }
        }
    }

    int cur = 0;                                             // entries in the list, the same number in every lane
    // run the items against the list and empty it (every lane has passed a barrier since the last append)
    auto drain = [&]() {
        for (int e = 0; e < cur; e++) {
            const float4 o = l_atom[e];
            const int c = l_cls[e];
#pragma unroll
            for (int u = 0; u < NU; u++) {
                const bool hit = pp_d2(qx[u], qy[u], qz[u], o.x, o.y, o.z) < o.w;
                m[u] = (hit && c < m[u]) ? c : m[u];
            }
        }
        __syncthreads();
        if (tid == 0) l_n = 0;
        __syncthreads();
        cur = 0;
    };

    for (int base = lo; base < hi; base += SA_T) {
        if (tid == 0) l_nrows = 0;
        __syncthreads();
        const int j = base + tid;
        bool keep = false;
        if (j < hi && j != i) {
            const float *rj = rowinfo + (size_t)j * 8;
            const float rad_j = rj[3];
            if (!(rad_j < 0.f)) {
                const float bound = (((rad_i + rad_j) + (rmax_i + rj[4])) * 1.001f) + 0.01f;
                keep = !(pp_d2(cx, cy, cz, rj[0], rj[1], rj[2]) > bound * bound);
            }
        }
        if (keep) l_rows[atomicAdd(&l_nrows, 1)] = j;
        const int nr = __syncthreads_count(keep ? 1 : 0);
        for (int r0 = 0; r0 < nr; r0 += SA_STEP) {
            if (cur + SA_STEP * 14 > PP_SASA_LIST_CAP) drain();
            const int r = r0 + (tid >> 4), a = tid & 15;
            bool will = false;
            if (r < nr && a < 14) {
                const int jj = l_rows[r];
                const float rb = radius[(size_t)jj * 14 + a];
                if (rb > 0.f) {
                    will = true;
                    const float *p = xyz + (size_t)jj * 42 + 3 * a;
                    const float Rb = rb + probe;
                    const int e = atomicAdd(&l_n, 1);
                    l_atom[e] = make_float4(p[0], p[1], p[2], Rb * Rb);
                    l_cls[e] = chain[jj] == ci ? 1 : 2;
                }
            }
            cur += __syncthreads_count(will ? 1 : 0);
        }
    }
    if (oatoms) {
        const int2 rg = oseg[s];
        for (int base = 0; base < rg.y; base += SA_T) {
            if (cur + SA_T > PP_SASA_LIST_CAP) drain();
            const int l = base + tid;
            bool will = false;
            if (l < rg.y) {
                const float4 o = oatoms[rg.x + l];
                if (o.w > 0.f) {
                    const float Ro = o.w + probe;
                    const float bound = (((rad_i + rmax_i) + Ro) * 1.001f) + 0.01f;
                    if (!(pp_d2(cx, cy, cz, o.x, o.y, o.z) > bound * bound)) {
                        will = true;
                        const int e = atomicAdd(&l_n, 1);
                        l_atom[e] = make_float4(o.x, o.y, o.z, Ro * Ro);
                        l_cls[e] = 3;
                    }
                }
            }
            cur += __syncthreads_count(will ? 1 : 0);
        }
    }
    drain();

#pragma unroll
    for (int u = 0; u < NU; u++) {
        const int it = tid + SA_T * u;
        if (it < n_items && m[u] > 0) {
            const int a = it / P;
            for (int L = 0; L < 4; L++)
                if (m[u] > L) atomicAdd(&l_cnt[a * 4 + L], 1);
        }
    }
    __syncthreads();
    if (counts && tid < 14 * 4) counts[(size_t)i * 56 + tid] = l_cnt[tid];
    if (tid < 4) {
        float sum = 0.f;
        for (int a = 0; a < 14; a++) {
            const float Ra = l_own[a][3];
            if (Ra > 0.f) sum = sum + (((kf * Ra) * Ra) * (float)l_cnt[a * 4 + tid]);
        }
        area[(size_t)i * 4 + tid] = sum;
    }
}

// seg_area[s][L] = the sum of area[n][L] over the rows of segment s, fp64, in the binary tree of k_ens_per_decoy
__global__ void __launch_bounds__(SA_T)
k_sasa_seg(int N, const int32_t *__restrict__ seg_off, const float *__restrict__ area, double *__restrict__ seg_area) {
#pragma clang fp contract(off)
    __shared__ double red[4][SA_T];
    const int s = blockIdx.x, tid = threadIdx.x;
    int a, b;
    pp_seg_rows(seg_off, s, N, a, b);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int n = a + tid; n < b; n += SA_T)
        for (int L = 0; L < 4; L++) acc[L] += (double)area[(size_t)n * 4 + L];
    for (int L = 0; L < 4; L++) red[L][tid] = acc[L];
    __syncthreads();
    for (int w = SA_T / 2; w > 0; w >>= 1) {
        if (tid < w)
            for (int L = 0; L < 4; L++) red[L][tid] += red[L][tid + w];
        __syncthreads();
    }
    if (tid < 4) seg_area[(size_t)s * 4 + tid] = red[tid][0];
}

extern "C" pp_status pp_sasa(pp_ctx *c, const float *xyz, const float *radius, const float *points, int n_points, float probe,
                             int32_t *counts, float *area, double *seg_area, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !radius || !points || !area) FAIL(PP_ERR_INVALID, "pp_sasa: null argument");
    if (n_points < 1 || n_points > PP_SASA_MAX_POINTS)
        FAIL(PP_ERR_INVALID, "pp_sasa: n_points must be 1 .. " + std::to_string(PP_SASA_MAX_POINTS));
    if (!std::isfinite(probe) || probe < 0.f) FAIL(PP_ERR_INVALID, "pp_sasa: probe must be finite and not negative");
    if (!c->b.chain_indices) FAIL(PP_ERR_INVALID, "pp_sasa: needs a batch with chain_indices");
    if (!xyz) xyz = c->b.X;
    if (!xyz) FAIL(PP_ERR_INVALID, "pp_sasa: no coordinates (xyz is null and the batch has no X)");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (c->N < 1) return PP_OK;
    const float kf = (float)(4.0 * PP_PI_D / (double)n_points);
    const bool obst = c->obst_M > 0;
    const float4 *oatoms = obst ? c->obst : nullptr;
    const int2 *oseg = obst ? c->obst_seg : nullptr;
    hipLaunchKernelGGL(k_sasa_rows, dim3((c->N + SA_T - 1) / SA_T), dim3(SA_T), 0, st, c->N, xyz, radius, probe, c->sasa_row);
    PP_HIP_CHECK(hipGetLastError());
    if (14 * n_points <= 6 * SA_T)
        hipLaunchKernelGGL(k_sasa<6>, dim3(c->N), dim3(SA_T), 0, st, c->N, c->B, c->seg_off, xyz, radius, c->b.chain_indices,
                           c->sasa_row, oatoms, oseg, points, n_points, probe, kf, counts, area);
    else
        hipLaunchKernelGGL(k_sasa<14>, dim3(c->N), dim3(SA_T), 0, st, c->N, c->B, c->seg_off, xyz, radius, c->b.chain_indices,
                           c->sasa_row, oatoms, oseg, points, n_points, probe, kf, counts, area);
    PP_HIP_CHECK(hipGetLastError());
    if (seg_area) {
        hipLaunchKernelGGL(k_sasa_seg, dim3(c->B), dim3(SA_T), 0, st, c->N, c->seg_off, area, seg_area);
        PP_HIP_CHECK(hipGetLastError());
    }
    return PP_OK;
}
