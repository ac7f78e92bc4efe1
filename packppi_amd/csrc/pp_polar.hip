// Polar contacts (no reference kernel): hydrogen bonds, salt bridges and polar obstacle contacts between the
// heavy atoms of every segment of the context's segment table (the complexes of a packed ctx, the decoys of a group, the B rows of a
// padded batch).  No pair crosses segments.  Chemistry is caller data, as pp_sasa takes `radius`:
//   cls  uint8 [N][14]     bit 0 donor, bit 1 acceptor, bit 2 cation, bit 3 anion; 0 = not polar or absent
//   ante int8 [N][14][2]   the slots of the same row the atom is bonded to, -1 = none; an entry outside -1 .. 13 makes the atom not
//                          polar and sets bit 2 of the context's sticky word
//
// ARITHMETIC (fp32, every operation rounded on its own: fp contract off), in this order:
//   1  atom x at p with antecedents at a1 (and a2): b = a1, or b = (a1 + a2) * 0.5f per component (no antecedent: u = 0)
//   2  u = b - p
//   3  pair (x at p, y at q):  d = q - p;  d2 = ((dx dx) + (dy dy)) + (dz dz);  sx = ((ux dx) + (uy dy)) + (uz dz);
//      e = p - q;  sy = ((uyx ex) + (uyy ey)) + (uyz ez) with y's own u
//   4  HYDROGEN BOND: x and y in different rows of one segment, (x donor and y acceptor) or (x acceptor and y donor),
//      d2 <= hb2 (hb2 = hb_max * hb_max, rounded once on the host), sx <= 0 and sy <= 0
//   5  the two sign tests say "both angles antecedent-atom...partner are at least 90 degrees" without a root or an arccosine; the
//      relation is symmetric by construction (e = -d exactly); a NaN makes a comparison false and gives no bond
//   6  SKIPPED: both atoms in backbone slots 0 or 3, rows adjacent (|n - j| = 1), equal chain_indices: the covalent neighbours
//   7  SALT BRIDGE between rows n != j of one segment: a cation atom of one and an anion atom of the other with d2 <= sb2
//   9  OBSTACLE PARTNER of an atom with cls != 0: an atom o of the segment's obstacle range with obst_polar[o] != 0 and d2 <= hb2
// Every test is an integer statement about fp32 numbers: a NumPy float32 restatement gives the same words (tests/polar_oracle.py).
//
// OUTPUTS: n_partners [N][14][2] (hydrogen-bond partners, polar obstacle atoms: true counts), partners [N][14][PP_POLAR_CAP] (the
// lowest codes (row - first row of the segment) * 14 + slot, ascending, then -1), res [N][8], seg [n_seg][8] (include/packppi_hip.h).
//
// LAUNCH.  k_polar_prep (16 lanes per row, 14 of them with an atom): checks the antecedents, writes (p, class) and u of every atom
// to the workspace and the row's sphere: slot 1 and the largest distance of a polar atom from it (-1: the row has no polar atom; a
// NaN sticks: the row is then never pruned).  k_polar (one wave per row i): the row's 14 atoms sit in LDS and are read as
// broadcasts.  The wave walks the rows of its segment 64 at a time in ascending order and keeps row j unless
//     d2(CA_i, CA_j) > ((rad_i + rad_j + reach) 1.001 + 0.01)^2,    reach = max(hb_max, sb_max)
// (two atoms within reach lie in spheres whose centres are at most rad_i + rad_j + reach apart; the slack is pp_shell's, orders above
// fp32 rounding, so the test changes no output word; a NaN keeps the pair).  The kept rows go to an LDS list in ascending order (a
// ballot and a bit count: no atomics), and their atoms are taken four rows at a time, 16 lanes per row: lane order is then code
// order.  For every own polar atom the hits are a ballot; a hit's place in the atom's partner list is the count so far plus the bits
// below the lane, so the lowest PP_POLAR_CAP codes come out ascending without a sort.  All counters are wave-uniform registers.  The
// segment sums are integer atomics on a zeroed array; each pair is counted from its lower row.  No float atomics anywhere.
#include "pp_internal.h"
#include "pp_vec.h"

#define PO_T 64                        // one wave per row

// P[n][a] = (x, y, z, class bits), U[n][a] = (u, 0), row[n] = (slot 1, radius of the polar atoms around it or -1)
__global__ void __launch_bounds__(256)
k_polar_prep(int N, const float *__restrict__ xyz, const uint8_t *__restrict__ cls, const int8_t *__restrict__ ante,
             float4 *__restrict__ P, float4 *__restrict__ U, float4 *__restrict__ row, unsigned *__restrict__ sat) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n = t >> 4, a = t & 15;
    const bool live = n < N && a < 14;
    float m2 = -1.f;
    bool any = false;
    if (live) {
        const float *pr = xyz + (size_t)n * 42;
        const float px = pr[3 * a], py = pr[3 * a + 1], pz = pr[3 * a + 2];
        int c = cls[(size_t)n * 14 + a];
        const int a1 = ante[((size_t)n * 14 + a) * 2], a2 = ante[((size_t)n * 14 + a) * 2 + 1];
        float ux = 0.f, uy = 0.f, uz = 0.f;
        if (c != 0) {
            if (a1 < -1 || a1 > 13 || a2 < -1 || a2 > 13) {
                c = 0;
                atomicOr(sat, 4u);
            } else if (a1 >= 0 || a2 >= 0) {
                float bx, by, bz;
                if (a1 >= 0 && a2 >= 0) {
                    bx = (pr[3 * a1] + pr[3 * a2]) * 0.5f;
                    by = (pr[3 * a1 + 1] + pr[3 * a2 + 1]) * 0.5f;
                    bz = (pr[3 * a1 + 2] + pr[3 * a2 + 2]) * 0.5f;
                } else {
                    const int b = a1 >= 0 ? a1 : a2;
                    bx = pr[3 * b]; by = pr[3 * b + 1]; bz = pr[3 * b + 2];
                }
                ux = bx - px; uy = by - py; uz = bz - pz;
            }
        }
        P[(size_t)n * 14 + a] = make_float4(px, py, pz, __int_as_float(c));
        U[(size_t)n * 14 + a] = make_float4(ux, uy, uz, 0.f);
        if (c != 0) {
            any = true;
            const float dx = px - pr[3], dy = py - pr[4], dz = pz - pr[5];
            m2 = pp_dot3(dx, dy, dz, dx, dy, dz);
        }
    }
    // the largest over the row's 16 lanes; a NaN sticks
    for (int w = 8; w > 0; w >>= 1) {
        const float o = __shfl_xor(m2, w, 16);
        const int oa = __shfl_xor(any ? 1 : 0, w, 16);
        m2 = pp_nanmax(m2, o);
        any = any || oa != 0;
    }
    if (n < N && a == 0) {
        const float *pr = xyz + (size_t)n * 42;
        row[n] = make_float4(pr[3], pr[4], pr[5], any ? sqrtf(m2) : -1.f);
    }
}

__global__ void __launch_bounds__(PO_T)
k_polar(int N, int n_seg, const int32_t *__restrict__ seg_off, const float4 *__restrict__ P, const float4 *__restrict__ U,
        const float4 *__restrict__ rowinfo, const int64_t *__restrict__ chain, const float4 *__restrict__ oatoms,
        const int2 *__restrict__ oseg, const uint8_t *__restrict__ opolar, float hb2, float sb2, float reach,
        int32_t *__restrict__ partners, int32_t *__restrict__ n_partners, int32_t *__restrict__ res, int32_t *__restrict__ seg_out) {
#pragma clang fp contract(off)
    __shared__ float4 l_p[14], l_u[14];
    __shared__ int l_rows[PO_T];
    __shared__ int l_part[14 * PP_POLAR_CAP];
    const int lane = threadIdx.x, i = blockIdx.x;
    if (i >= N) return;
    const unsigned long long below = (1ull << lane) - 1ull;

    if (lane < 14) {
        l_p[lane] = P[(size_t)i * 14 + lane];
        l_u[lane] = U[(size_t)i * 14 + lane];
    }
    if (lane < 14 * PP_POLAR_CAP) l_part[lane] = -1;
    const int s = pp_seg_of_row(seg_off, n_seg, i);
    int lo, hi;
    pp_seg_rows(seg_off, s, N, lo, hi);
    const float4 ri = rowinfo[i];
    __syncthreads();

    int n_hb[14], n_same[14], n_ob[14];
#pragma unroll
    for (int x = 0; x < 14; x++) n_hb[x] = n_same[x] = n_ob[x] = 0;
    int sb_same = 0, sb_other = 0;
    int up_all = 0, up_inter = 0, up_sc = 0, up_sc_inter = 0, up_sb = 0, up_sb_inter = 0;

    // a row without a polar atom, or one outside its segment (a table that breaks the contract), has no partner: zeros below
    const bool active = !(ri.w < 0.f) && i >= lo && i < hi;
    if (active) {
        const long long ci = chain[i];
        for (int base = lo; base < hi; base += PO_T) {
            const int j = base + lane;
            bool keep = false;
            if (j < hi && j != i) {
                const float4 rj = rowinfo[j];
                if (!(rj.w < 0.f)) {
                    const float bound = (((ri.w + rj.w) + reach) * 1.001f) + 0.01f;
                    const float dx = rj.x - ri.x, dy = rj.y - ri.y, dz = rj.z - ri.z;
                    keep = !(pp_dot3(dx, dy, dz, dx, dy, dz) > bound * bound);
                }
            }
            const unsigned long long kept = __ballot(keep);
            if (kept == 0ull) continue;                       // the same in every lane
            if (keep) l_rows[__popcll(kept & below)] = j;     // ascending rows
            __syncthreads();
            const int nr = __popcll(kept);
            for (int r0 = 0; r0 < nr; r0 += 4) {
                const int r = r0 + (lane >> 4), a = lane & 15;
                const bool valid = r < nr && a < 14;
                int jj = i, yc = 0;
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f), uq = q;
                bool same = false;
                if (valid) {
                    jj = l_rows[r];
                    q = P[(size_t)jj * 14 + a];
                    uq = U[(size_t)jj * 14 + a];
                    yc = __float_as_int(q.w);
                    same = chain[jj] == ci;
                }
                if (__ballot(yc != 0) == 0ull) continue;
                const bool up = jj > i, ysc = a >= 4;
                const bool adj = same && (jj - i == 1 || i - jj == 1) && (a == 0 || a == 3);
                const int code = (jj - lo) * 14 + a;
                bool sb_any = false;
#pragma unroll
                for (int x = 0; x < 14; x++) {
                    const float4 p = l_p[x];
                    const int xc = __float_as_int(p.w);
                    if (xc == 0) continue;                    // the same in every lane
                    const float4 u = l_u[x];
                    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
                    const float d2 = pp_dot3(dx, dy, dz, dx, dy, dz);
                    const float sx = pp_dot3(u.x, u.y, u.z, dx, dy, dz);
                    const float ex = p.x - q.x, ey = p.y - q.y, ez = p.z - q.z;
                    const float sy = pp_dot3(uq.x, uq.y, uq.z, ex, ey, ez);
                    const bool da = ((xc & 1) && (yc & 2)) || ((xc & 2) && (yc & 1));
                    const bool skip = adj && (x == 0 || x == 3);
                    const bool hb = da && !skip && d2 <= hb2 && sx <= 0.f && sy <= 0.f;
                    const bool sb = (((xc & 4) && (yc & 8)) || ((xc & 8) && (yc & 4))) && d2 <= sb2;
                    sb_any = sb_any || sb;
                    const unsigned long long m = __ballot(hb);
                    if (m != 0ull) {
                        const unsigned long long ms = __ballot(hb && same), mu = __ballot(hb && up);
                        const unsigned long long msc = __ballot(hb && up && (x >= 4 || ysc));
                        if (hb) {
                            const int pos = n_hb[x] + __popcll(m & below);
                            if (pos < PP_POLAR_CAP) l_part[x * PP_POLAR_CAP + pos] = code;
                        }
                        n_hb[x] += __popcll(m);
                        n_same[x] += __popcll(ms);
                        up_all += __popcll(mu);
                        up_inter += __popcll(mu & ~ms);
                        up_sc += __popcll(msc);
                        up_sc_inter += __popcll(msc & ~ms);
                    }
                }
                // salt bridges count partner ROWS: a row of the step is 16 lanes
                const unsigned long long mb = __ballot(sb_any);
                if (mb != 0ull) {
                    const unsigned long long mbs = __ballot(sb_any && same), mbu = __ballot(sb_any && up);
                    for (int k = 0; k < 4; k++) {
                        const unsigned g = (unsigned)(mb >> (16 * k)) & 0xffffu;
                        if (g == 0u) continue;
                        const bool gs = ((mbs >> (16 * k)) & 0xffffull) != 0ull, gu = ((mbu >> (16 * k)) & 0xffffull) != 0ull;
                        sb_same += gs ? 1 : 0;
                        sb_other += gs ? 0 : 1;
                        up_sb += gu ? 1 : 0;
                        up_sb_inter += (gu && !gs) ? 1 : 0;
                    }
                }
            }
            __syncthreads();                                  // the list is rewritten by the next 64 rows
        }
        if (oatoms) {
            const int2 rg = oseg[s];
            for (int base = 0; base < rg.y; base += PO_T) {
                const int l = base + lane;
                bool pol = false;
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                if (l < rg.y) {
                    o = oatoms[rg.x + l];
                    pol = opolar[rg.x + l] != 0;
                }
                if (__ballot(pol) == 0ull) continue;
#pragma unroll
                for (int x = 0; x < 14; x++) {
                    const float4 p = l_p[x];
                    if (__float_as_int(p.w) == 0) continue;
                    const float dx = o.x - p.x, dy = o.y - p.y, dz = o.z - p.z;
                    n_ob[x] += __popcll(__ballot(pol && pp_dot3(dx, dy, dz, dx, dy, dz) <= hb2));
                }
            }
        }
    }
    __syncthreads();

    int r_out[8] = {0, 0, 0, 0, sb_same, sb_other, 0, 0};
    int my_hb = 0, my_ob = 0;
#pragma unroll
    for (int x = 0; x < 14; x++) {
        const bool polar = active && __float_as_int(l_p[x].w) != 0;
        if (x >= 4) { r_out[0] += n_same[x]; r_out[1] += n_hb[x] - n_same[x]; }
        if (x == 0 || x == 3) { r_out[2] += n_same[x]; r_out[3] += n_hb[x] - n_same[x]; }
        r_out[6] += n_ob[x];
        r_out[7] += (polar && n_hb[x] == 0 && n_ob[x] == 0) ? 1 : 0;
        if (lane == x) { my_hb = n_hb[x]; my_ob = n_ob[x]; }
    }
    const int s_out[8] = {up_all, up_inter, up_sc, up_sc_inter, up_sb, up_sb_inter, r_out[6], r_out[7]};
    if (lane < 14) {
        n_partners[((size_t)i * 14 + lane) * 2] = my_hb;
        n_partners[((size_t)i * 14 + lane) * 2 + 1] = my_ob;
    }
    if (partners && lane < 14 * PP_POLAR_CAP) partners[(size_t)i * 14 * PP_POLAR_CAP + lane] = l_part[lane];
    int my_r = 0, my_s = 0;
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (lane == k) { my_r = r_out[k]; my_s = s_out[k]; }
    if (lane < 8) {
        res[(size_t)i * 8 + lane] = my_r;
        if (active && my_s != 0) atomicAdd(&seg_out[(size_t)s * 8 + lane], my_s);
    }
}

extern "C" pp_status pp_polar(pp_ctx *c, const float *xyz, const uint8_t *cls, const int8_t *ante, const uint8_t *obst_polar,
                              float hb_max, float sb_max, int32_t *partners, int32_t *n_partners, int32_t *res, int32_t *seg,
                              void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !cls || !ante || !n_partners || !res || !seg) FAIL(PP_ERR_INVALID, "pp_polar: null argument");
    if (!std::isfinite(hb_max) || !(hb_max > 0.f) || !std::isfinite(sb_max) || !(sb_max > 0.f))
        FAIL(PP_ERR_INVALID, "pp_polar: hb_max and sb_max must be finite and positive");
    if (!c->b.chain_indices) FAIL(PP_ERR_INVALID, "pp_polar: needs a batch with chain_indices");
    if (obst_polar && c->obst_M <= 0) FAIL(PP_ERR_INVALID, "pp_polar: obst_polar on a context without obstacle atoms");
    if (!xyz) xyz = c->b.X;
    if (!xyz) FAIL(PP_ERR_INVALID, "pp_polar: no coordinates (xyz is null and the batch has no X)");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (c->N < 1) return PP_OK;
    const size_t n_atoms = (size_t)c->N * 14;
    const size_t total = (2 * n_atoms + (size_t)c->N) * sizeof(float4);
    void *ws;
    if (pp_status rc = pp_ctx_workspace(c, PP_WS_POLAR, total, &ws)) return rc;
    float4 *P = static_cast<float4 *>(ws), *U = P + n_atoms, *row = U + n_atoms;
    const float hb2 = hb_max * hb_max, sb2 = sb_max * sb_max;
    const float reach = hb_max > sb_max ? hb_max : sb_max;
    const bool obst = obst_polar != nullptr;
    PP_HIP_CHECK(hipMemsetAsync(seg, 0, (size_t)c->B * 8 * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_polar_prep, dim3((unsigned)((n_atoms / 14 * 16 + 255) / 256)), dim3(256), 0, st, c->N, xyz, cls, ante, P, U, row,
                       c->sat);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_polar, dim3(c->N), dim3(PO_T), 0, st, c->N, c->B, c->seg_off, P, U, row, c->b.chain_indices,
                       obst ? c->obst : nullptr, obst ? c->obst_seg : nullptr, obst_polar, hb2, sb2, reach, partners, n_partners, res,
                       seg);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
