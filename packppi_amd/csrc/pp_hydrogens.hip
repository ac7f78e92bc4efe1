// Explicit hydrogens and the all-atom clashscore (no reference kernel).  Both entries work per segment of the
// context's segment table (the complexes of a packed ctx, the decoys of a group, the B rows of a padded batch); nothing crosses
// segments.  Chemistry is caller data, as pp_sasa takes `radius` and pp_polar `cls`: the kernels know slots, not residues.
//
// pp_hydrogens.  An all-atom row has PP_AA_SLOTS = 27 slots: 0 .. 13 atom14, 14 + k the k-th hydrogen (PP_H_MAX = 13).
//   place int8  [21][13][5]  per residue type and hydrogen: (kind, parent slot p, n1, n2, n3).  kind & 15: 0 none, 1 SUM, 2 T2,
//                            3 NERF; kind & 16: the hydrogen is dropped on a row with link[n] >= 0.  SUM: n1 .. n3 are the parent's
//                            heavy neighbours, -1 = none, 14 = the C of row n - 1 (needs link_prev[n]).  T2: n1 < n2 its two
//                            neighbours.  NERF: n1 = a, the parent's one neighbour, n2 = b, a neighbour of a.
//   param float [21][13][5]  (L, c1, s1, c2, s2): T2: c1 = cos alpha, s1 = +-sin alpha; NERF: cos / sin of the angle H-p-a and of
//                            the dihedral H-p-a-b, rounded to float once on the host
// An entry outside its range (a kind that is none of these, a slot outside 0 .. 13, a neighbour outside -1 .. 14), or a
// residue_type outside 0 .. 20, is found on the device: the hydrogen is dropped and bit 3 of the context's sticky word is set.  It
// is never used as an index.
//
// ARITHMETIC (fp32, every operation rounded on its own: fp contract off).  Every vector is a difference to the parent p, so the
// only error of the size of the coordinates is the final add.  unit(v) = v / sqrt(((vx vx) + (vy vy)) + (vz vz)) per component.
//   link_prev[n] = row n - 1 lies in the same segment and has the same chain_indices, atom_mask of its slot 2 (C) and of slot 0 (N)
//                  of row n are not 0, and d = C - N has ((dx dx) + (dy dy)) + (dz dz) <= 4.0f
//   SUM    u_i = unit(q_i - p) for the neighbours in table order;  s = unit((u_1 + u_2) + u_3) (absent ones left out);
//          H = p - (L s)
//   T2     u_1, u_2 as above;  b = -unit(u_1 + u_2);  n = unit(u_1 x u_2);  H = p + L ((c1 b) + (s1 n))
//   NERF   H = p + pp_nerf(...) (pp_allatom.h: the definition, shared with the rotor states of pp_hnet.hip)
//   dot and cross products, unit: pp_vec.h
// A hydrogen EXISTS iff atom_mask is not 0 for its parent and for every atom it reads, link_prev[n] holds if it reads the previous
// C, it is not dropped for link, and all three results are finite (atoms exactly in line give 0 / 0: the hydrogen is dropped).
// hmask says so; hxyz of a hydrogen that does not exist is 0.
//
// pp_clashscore.  Which atoms are COUNTED, the acls bits and the pair rules, steps 1 - 6 (serious overlap, excluded pairs, obstacle
// atoms): pp_allatom.h.  A pair is a hit iff it overlaps (steps 1 - 4) and is not excluded (step 5); obstacle atoms by step 6.
// Every test is an integer statement about fp32 numbers: a NumPy float32 restatement gives the same words (tests/allatom_oracle.py).
//
// OUTPUTS (int32): n_clash [N][27][2] (partner atoms, obstacle atoms: true counts), partners [N][27][PP_CLASH_CAP] (the lowest codes
// (row - first row of the segment) * 27 + slot, ascending, then -1), res [N][4], seg [n_seg][8] (include/packppi_hip.h).
//
// LAUNCH.  k_aa_prep (32 lanes per row, 27 of them with an atom): writes (p, radius or 0) and one word (class, separations from
// slots 0, 2, 5) per atom, and the row's sphere: slot 1 and the largest (distance from it + radius) of a counted atom (-1: none; a
// NaN sticks: the row is then never pruned).  k_clashscore (one wave per row i): the row's 27 atoms and its 27 x 27 separations sit
// in LDS and are read as broadcasts.  The wave walks the rows of its segment 64 at a time in ascending order, its own included, and
// keeps row j unless
//     d2(CA_i, CA_j) > ((R_i + R_j - cut) 1.001 + 0.01)^2
// (two overlapping atoms have d <= rx + ry - cut and lie in spheres whose centres are then at most R_i + R_j - cut apart; the slack
// is pp_polar's, orders above fp32 rounding, so the test changes no output word; a NaN keeps the pair).  The kept rows go to an LDS
// list in ascending order (a ballot and a bit count), and their atoms are taken two rows at a time, 32 lanes per row: a row of 27
// atoms fills 27 of 32 lanes, where 16-lane groups would fill 27 of 32 as well and need two steps per row; lane order is code order.
// For every counted atom of the own row the hits are a ballot; a hit's place in the partner list is the count so far plus the bits
// below the lane.  Per-atom counts live in the lane of the atom's slot, row and segment counts in wave-uniform registers.  The
// segment sums are integer atomics on a zeroed array; a pair is counted from its lower (row, slot).  No float atomics anywhere.
#include "pp_internal.h"
#include "pp_allatom.h"

#define AA_T 64                        // one wave per row

// 16 lanes per row: lane k < 13 places hydrogen k, lane 13 writes link_prev
__global__ void __launch_bounds__(256)
k_hydrogens(int N, int n_seg, const int32_t *__restrict__ seg_off, const float *__restrict__ xyz, const float *__restrict__ amask,
            const int64_t *__restrict__ rtype, const int64_t *__restrict__ chain, const int8_t *__restrict__ place,
            const float *__restrict__ param, const int32_t *__restrict__ link, float *__restrict__ hxyz,
            uint8_t *__restrict__ hmask, uint8_t *__restrict__ link_prev, unsigned *__restrict__ sat) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n = t >> 4, k = t & 15;
    if (n >= N || k > PP_H_MAX) return;
    const int s = pp_seg_of_row(seg_off, n_seg, n);
    int lo, hi;
    pp_seg_rows(seg_off, s, N, lo, hi);
    const float *pr = xyz + (size_t)n * 42;
    const float *am = amask + (size_t)n * 14;
    bool lp = false;
    if (n > lo && n < hi && chain[n] == chain[n - 1] && amask[(size_t)(n - 1) * 14 + 2] != 0.f && am[0] != 0.f) {
        const float *pc = pr - 42 + 6;
        const float dx = pc[0] - pr[0], dy = pc[1] - pr[1], dz = pc[2] - pr[2];
        lp = pp_dot3(dx, dy, dz, dx, dy, dz) <= 4.0f;
    }
    if (k == PP_H_MAX) {
        link_prev[n] = lp ? 1 : 0;
        return;
    }
    const long long ty = rtype[n];
    bool ok = false;
    float hx = 0.f, hy = 0.f, hz = 0.f;
    if (ty < 0 || ty > 20) {
        atomicOr(sat, AA_SAT);
    } else {
        const int8_t *pl = place + ((size_t)ty * PP_H_MAX + k) * 5;
        const float *pa = param + ((size_t)ty * PP_H_MAX + k) * 5;
        const int kind = pl[0], p = pl[1], n1 = pl[2], n2 = pl[3], n3 = pl[4];
        const int how = kind & 15;
        if (kind != 0) {
            bool bad = kind < 0 || kind > 31 || how < 1 || how > 3 || p < 0 || p > 13;
            if (how == 1) bad = bad || n1 < -1 || n1 > 14 || n2 < -1 || n2 > 14 || n3 < -1 || n3 > 14;
            else bad = bad || n1 < 0 || n1 > 13 || n2 < 0 || n2 > 13;
            if (bad) {
                atomicOr(sat, AA_SAT);
            } else {
                ok = am[p] != 0.f && !((kind & 16) && link && link[n] >= 0);
                const pp_v3 P = {pr[3 * p], pr[3 * p + 1], pr[3 * p + 2]};
                const float L = pa[0];
                pp_v3 d = {0.f, 0.f, 0.f};
                if (how == 1) {
                    pp_v3 sum = {0.f, 0.f, 0.f};
                    bool first = true;
                    const int nb[3] = {n1, n2, n3};
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        const int a = nb[q];
                        if (a < 0) continue;
                        const float *src = pr + 3 * a;
                        if (a == 14) {
                            ok = ok && lp;
                            src = lp ? pr - 42 + 6 : pr;           // without link_prev there may be no previous row to read
                        } else {
                            ok = ok && am[a] != 0.f;
                        }
                        const pp_v3 u = pp_unit(pp_sub(src, P));
                        if (first) sum = u;
                        else sum = {sum.x + u.x, sum.y + u.y, sum.z + u.z};
                        first = false;
                    }
                    ok = ok && !first;
                    const pp_v3 sdir = pp_unit(sum);
                    d = {-(L * sdir.x), -(L * sdir.y), -(L * sdir.z)};
                } else if (how == 2) {
                    ok = ok && am[n1] != 0.f && am[n2] != 0.f;
                    const pp_v3 u1 = pp_unit(pp_sub(pr + 3 * n1, P)), u2 = pp_unit(pp_sub(pr + 3 * n2, P));
                    const pp_v3 b = pp_unit({u1.x + u2.x, u1.y + u2.y, u1.z + u2.z});
                    const pp_v3 nn = pp_unit(pp_cross(u1, u2));
                    const float c1 = pa[1], s1 = pa[2];
                    d = {L * ((c1 * -b.x) + (s1 * nn.x)), L * ((c1 * -b.y) + (s1 * nn.y)), L * ((c1 * -b.z) + (s1 * nn.z))};
                } else {
                    ok = ok && am[n1] != 0.f && am[n2] != 0.f;
                    d = pp_nerf(P, pr + 3 * n1, pr + 3 * n2, L, pa[1], pa[2], pa[3], pa[4]);
                }
                hx = P.x + d.x; hy = P.y + d.y; hz = P.z + d.z;
                ok = ok && pp_finite(hx) && pp_finite(hy) && pp_finite(hz);
            }
        }
    }
    const size_t o = (size_t)n * PP_H_MAX + k;
    hmask[o] = ok ? 1 : 0;
    hxyz[o * 3] = ok ? hx : 0.f;
    hxyz[o * 3 + 1] = ok ? hy : 0.f;
    hxyz[o * 3 + 2] = ok ? hz : 0.f;
}

extern "C" pp_status pp_hydrogens(pp_ctx *c, const float *xyz, const int8_t *place, const float *param, const int32_t *link,
                                  float *hxyz, uint8_t *hmask, uint8_t *link_prev, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !place || !param || !hxyz || !hmask || !link_prev) FAIL(PP_ERR_INVALID, "pp_hydrogens: null argument");
    if (!c->b.chain_indices || !c->b.residue_type || !c->b.atom_mask)
        FAIL(PP_ERR_INVALID, "pp_hydrogens: needs a batch with chain_indices, residue_type and atom_mask");
    if (!xyz) xyz = c->b.X;
    if (!xyz) FAIL(PP_ERR_INVALID, "pp_hydrogens: no coordinates (xyz is null and the batch has no X)");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (c->N < 1) return PP_OK;
    hipLaunchKernelGGL(k_hydrogens, dim3((unsigned)(((size_t)c->N * 16 + 255) / 256)), dim3(256), 0, st, c->N, c->B, c->seg_off, xyz,
                       c->b.atom_mask, c->b.residue_type, c->b.chain_indices, place, param, link, hxyz, hmask, link_prev, c->sat);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

// P[n][a] = (x, y, z, radius of a counted atom or 0), I[n][a] = class | sep(a, 0) << 4 | sep(a, 2) << 8 | sep(a, 5) << 12,
// row[n] = (slot 1, the largest distance from it + radius of a counted atom or -1)
__global__ void __launch_bounds__(256)
k_aa_prep(int N, const float *__restrict__ xyz, const float *__restrict__ hxyz, const uint8_t *__restrict__ hmask,
          const float *__restrict__ radius, const uint8_t *__restrict__ acls, const uint8_t *__restrict__ aa_sep,
          const int64_t *__restrict__ rtype, float4 *__restrict__ P, int32_t *__restrict__ I, float4 *__restrict__ row,
          unsigned *__restrict__ sat) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n = t >> 5, a = t & 31;
    const bool live = n < N && a < AA_S;
    float m = -1.f;
    bool any = false;
    if (live) {
        float4 p = pp_aa_atom(xyz, hxyz, hmask, radius, n, a);
        I[(size_t)n * AA_S + a] = pp_aa_word(p, acls, aa_sep, rtype[n], n, a, sat);
        P[(size_t)n * AA_S + a] = p;
        if (p.w > 0.f) {
            any = true;
            m = pp_aa_extent(p, xyz + (size_t)n * 42 + 3);
        }
    }
    pp_aa_row_sphere(m, any);
    if (n < N && a == 0) {
        const float *ca = xyz + (size_t)n * 42 + 3;
        row[n] = make_float4(ca[0], ca[1], ca[2], any ? m : -1.f);
    }
}

__global__ void __launch_bounds__(AA_T)
k_clashscore(int N, int n_seg, const int32_t *__restrict__ seg_off, const float4 *__restrict__ P, const int32_t *__restrict__ I,
             const float4 *__restrict__ rowinfo, const int64_t *__restrict__ chain, const int64_t *__restrict__ rtype,
             const uint8_t *__restrict__ aa_sep, const uint8_t *__restrict__ link_prev, const int32_t *__restrict__ link,
             const float4 *__restrict__ oatoms, const int2 *__restrict__ oseg, const uint8_t *__restrict__ opolar, float cut,
             float hb_allow, int32_t *__restrict__ partners, int32_t *__restrict__ n_clash, int32_t *__restrict__ res,
             int32_t *__restrict__ seg_out) {
#pragma clang fp contract(off)
    __shared__ float4 l_p[AA_S];
    __shared__ int l_i[AA_S];
    __shared__ uint8_t l_sep[AA_S * AA_S + 7];
    __shared__ int l_rows[AA_T];
    __shared__ int l_part[AA_S * PP_CLASH_CAP];
    const int lane = threadIdx.x, i = blockIdx.x;
    if (i >= N) return;
    const unsigned long long below = (1ull << lane) - 1ull;

    if (lane < AA_S) {
        l_p[lane] = P[(size_t)i * AA_S + lane];
        l_i[lane] = I[(size_t)i * AA_S + lane];
    }
    for (int q = lane; q < AA_S * PP_CLASH_CAP; q += AA_T) l_part[q] = -1;
    {
        const long long ty = rtype[i];
        const bool tok = ty >= 0 && ty <= 20;                 // otherwise the row has no counted atom (k_aa_prep)
        for (int q = lane; q < AA_S * AA_S; q += AA_T) l_sep[q] = tok ? aa_sep[(size_t)ty * AA_S * AA_S + q] : 9;
    }
    const int s = pp_seg_of_row(seg_off, n_seg, i);
    int lo, hi;
    pp_seg_rows(seg_off, s, N, lo, hi);
    const float4 ri = rowinfo[i];
    __syncthreads();

    int my_at = 0, my_ob = 0;                                  // lane x: the counts of the own atom in slot x
    int r_same = 0, r_other = 0, r_ob = 0, r_atoms = 0;
    int up_all = 0, up_inter = 0, up_h = 0, up_nbb = 0, up_row = 0;

    // a row without a counted atom, or one outside its segment (a table that breaks the contract), has no partner: zeros below
    const bool active = !(ri.w < 0.f) && i >= lo && i < hi;
    if (active) {
        const long long ci = chain[i];
        const int lpi = link_prev[i];
        const int lki = link ? link[i] : -1;
        for (int x = 0; x < AA_S; x++) r_atoms += l_p[x].w > 0.f ? 1 : 0;
        for (int base = lo; base < hi; base += AA_T) {
            const int j = base + lane;
            bool keep = false;
            if (j < hi) {
                const float4 rj = rowinfo[j];
                if (j == i) {
                    keep = true;
                } else if (!(rj.w < 0.f)) {
                    const float bound = (((ri.w + rj.w) - cut) * 1.001f) + 0.01f;
                    const float dx = rj.x - ri.x, dy = rj.y - ri.y, dz = rj.z - ri.z;
                    keep = !(pp_dot3(dx, dy, dz, dx, dy, dz) > bound * bound);
                }
            }
            const unsigned long long kept = __ballot(keep);
            if (kept == 0ull) continue;                       // the same in every lane
            if (keep) l_rows[__popcll(kept & below)] = j;     // ascending rows
            __syncthreads();
            const int nr = __popcll(kept);
            for (int r0 = 0; r0 < nr; r0 += 2) {
                const int r = r0 + (lane >> 5), a = lane & 31;
                const bool valid = r < nr && a < AA_S;
                int jj = i, yi = 0;
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                bool same = false, rel_next = false, rel_prev = false, rel_ss = false;
                if (valid) {
                    jj = l_rows[r];
                    q = P[(size_t)jj * AA_S + a];
                    yi = I[(size_t)jj * AA_S + a];
                    same = chain[jj] == ci;
                    rel_next = jj == i + 1 && link_prev[jj] != 0;
                    rel_prev = jj == i - 1 && lpi != 0;
                    rel_ss = jj != i && lki == jj && link[jj] == i;       // lki >= 0 only with link
                }
                const bool yok = valid && q.w > 0.f;
                if (__ballot(yok) == 0ull) continue;
                const bool own = jj == i;
                const int code = (jj - lo) * AA_S + a;
                const int y0 = (yi >> 4) & 15, y2 = (yi >> 8) & 15, y5 = (yi >> 12) & 15;
#pragma nounroll
                for (int x = 0; x < AA_S; x++) {
                    const float4 p = l_p[x];
                    if (!(p.w > 0.f)) continue;               // the same in every lane
                    const int xi = l_i[x];
                    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
                    const float d2 = pp_dot3(dx, dy, dz, dx, dy, dz);
                    float t = (p.w + q.w) - cut;                  // steps 2 - 4; hn_term (pp_hnet.hip) is the other copy
                    if (((xi & 1) && (yi & 2)) || ((xi & 2) && (yi & 1))) t = t - hb_allow;
                    const int sep = pp_aa_sep(own, rel_next, rel_prev, rel_ss, xi, y0, y2, y5, &l_sep[x * AA_S + (valid ? a : 0)]);
                    const bool hyd = ((xi | yi) & 4) != 0;
                    const bool hit = yok && !(own && a == x) && sep > pp_aa_excl(hyd) && t > 0.f && d2 <= t * t;
                    const unsigned long long m = __ballot(hit);
                    if (m != 0ull) {
                        const bool up = jj > i || (own && a > x);
                        const unsigned long long ms = __ballot(hit && same), mu = __ballot(hit && up);
                        const unsigned long long mr = __ballot(hit && own), mh = __ballot(hit && up && hyd);
                        const unsigned long long mn = __ballot(hit && up && !((xi & 8) && (yi & 8)));
                        const int before = __shfl(my_at, x);
                        if (hit) {
                            const int pos = before + __popcll(m & below);
                            if (pos < PP_CLASH_CAP) l_part[x * PP_CLASH_CAP + pos] = code;
                        }
                        if (lane == x) my_at += __popcll(m);
                        r_same += __popcll(ms & ~mr) + __popcll(mr & mu);
                        r_other += __popcll(m & ~ms);
                        up_all += __popcll(mu);
                        up_inter += __popcll(mu & ~ms);
                        up_h += __popcll(mh);
                        up_nbb += __popcll(mn);
                        up_row += __popcll(mu & mr);
                    }
                }
            }
            __syncthreads();                                  // the list is rewritten by the next 64 rows
        }
        if (oatoms) {
            const int2 rg = oseg[s];
            for (int base = 0; base < rg.y; base += AA_T) {
                const int l = base + lane;
                bool pol = false;
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                if (l < rg.y) {
                    o = oatoms[rg.x + l];
                    pol = opolar && opolar[rg.x + l] != 0;
                }
                const bool ook = l < rg.y && o.w > 0.f;
                if (__ballot(ook) == 0ull) continue;
#pragma nounroll
                for (int x = 0; x < AA_S; x++) {
                    const float4 p = l_p[x];
                    if (!(p.w > 0.f)) continue;
                    const float dx = o.x - p.x, dy = o.y - p.y, dz = o.z - p.z;
                    const float d2 = pp_dot3(dx, dy, dz, dx, dy, dz);
                    float t = (p.w + o.w) - cut;
                    if ((l_i[x] & 1) && pol) t = t - hb_allow;
                    const int cnt = __popcll(__ballot(ook && t > 0.f && d2 <= t * t));
                    if (lane == x) my_ob += cnt;
                    r_ob += cnt;
                }
            }
        }
    }
    __syncthreads();

    if (lane < AA_S) {
        n_clash[((size_t)i * AA_S + lane) * 2] = my_at;
        n_clash[((size_t)i * AA_S + lane) * 2 + 1] = my_ob;
    }
    if (partners)
        for (int q = lane; q < AA_S * PP_CLASH_CAP; q += AA_T) partners[(size_t)i * AA_S * PP_CLASH_CAP + q] = l_part[q];
    const int r_out[4] = {r_same, r_other, r_ob, r_atoms};
    const int s_out[8] = {r_atoms, up_all, up_inter, up_h, up_nbb, up_row, r_ob, up_all - up_nbb};
    int my_r = 0, my_s = 0;
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (lane == k) { my_r = k < 4 ? r_out[k & 3] : 0; my_s = s_out[k]; }
    if (lane < 4) res[(size_t)i * 4 + lane] = my_r;
    if (lane < 8 && active && my_s != 0) atomicAdd(&seg_out[(size_t)s * 8 + lane], my_s);
}

extern "C" pp_status pp_clashscore(pp_ctx *c, const float *xyz, const float *hxyz, const uint8_t *hmask, const float *radius,
                                   const uint8_t *acls, const uint8_t *aa_sep, const uint8_t *link_prev, const int32_t *link,
                                   const uint8_t *obst_polar, float cut, float hb_allow, int32_t *partners, int32_t *n_clash,
                                   int32_t *res, int32_t *seg, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !hxyz || !hmask || !radius || !acls || !aa_sep || !link_prev || !n_clash || !res || !seg)
        FAIL(PP_ERR_INVALID, "pp_clashscore: null argument");
    if (!std::isfinite(cut) || !std::isfinite(hb_allow) || hb_allow < 0.f)
        FAIL(PP_ERR_INVALID, "pp_clashscore: cut must be finite, hb_allow finite and not negative");
    if (!c->b.chain_indices || !c->b.residue_type)
        FAIL(PP_ERR_INVALID, "pp_clashscore: needs a batch with chain_indices and residue_type");
    if (obst_polar && c->obst_M <= 0) FAIL(PP_ERR_INVALID, "pp_clashscore: obst_polar on a context without obstacle atoms");
    if (!xyz) xyz = c->b.X;
    if (!xyz) FAIL(PP_ERR_INVALID, "pp_clashscore: no coordinates (xyz is null and the batch has no X)");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (c->N < 1) return PP_OK;
    const size_t n_atoms = (size_t)c->N * AA_S;
    const size_t total = n_atoms * (sizeof(float4) + sizeof(int32_t)) + (size_t)c->N * sizeof(float4);
    void *ws;
    if (pp_status rc = pp_ctx_workspace(c, PP_WS_ALLATOM, total, &ws)) return rc;
    float4 *P = static_cast<float4 *>(ws), *row = P + n_atoms;
    int32_t *I = reinterpret_cast<int32_t *>(row + c->N);
    const bool obst = c->obst_M > 0;
    PP_HIP_CHECK(hipMemsetAsync(seg, 0, (size_t)c->B * 8 * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_aa_prep, dim3((unsigned)(((size_t)c->N * 32 + 255) / 256)), dim3(256), 0, st, c->N, xyz, hxyz, hmask, radius,
                       acls, aa_sep, c->b.residue_type, P, I, row, c->sat);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_clashscore, dim3(c->N), dim3(AA_T), 0, st, c->N, c->B, c->seg_off, P, I, row, c->b.chain_indices,
                       c->b.residue_type, aa_sep, link_prev, link, obst ? c->obst : nullptr, obst ? c->obst_seg : nullptr, obst_polar,
                       cut, hb_allow, partners, n_clash, res, seg);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
