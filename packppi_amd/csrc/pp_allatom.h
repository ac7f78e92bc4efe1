// The all-atom rules that pp_hydrogens.hip (pp_hydrogens, pp_clashscore) and pp_hnet.hip (pp_hnet_optimize)
// both compile: NERF, the per-atom record with the row sphere, and of the pair rules below the bond separation and the exclusion
// threshold of step 5.  Steps 1 - 4 and 6 and the bonded-row flags of step 5 are DEFINED here and WRITTEN twice, in k_clashscore and
// in hn_term / k_hn_propose: no helper shape tried left k_clashscore's instructions alone (profiles/r31_rowsweep_isa.txt), so those
// two copies agree by their text and the byte-exact suites, and each names the other.
// fp32, every operation rounded on its own (fp contract off; pp_vec.h).
//
// An all-atom row has PP_AA_SLOTS = 27 slots: 0 .. 13 atom14, 14 + k the k-th hydrogen (PP_H_MAX = 13).  Atom (row n, slot a) is COUNTED
// iff radius[n][a] > 0 and, for a >= 14, hmask[n][a - 14] != 0.  acls bits: 0 polar hydrogen, 1 acceptor, 2 hydrogen, 3 backbone.
// PAIR RULES for (x at p, y at q) of counted atoms of one segment:
//   1  d = q - p;  d2 = ((dx dx) + (dy dy)) + (dz dz)
//   2  t = (rx + ry) - cut
//   3  one a polar hydrogen and the other an acceptor:  t = t - hb_allow
//   4  SERIOUS OVERLAP iff t > 0 and d2 <= t t   (no root; a NaN makes a comparison false: none)
//   5  EXCLUDED iff the bond separation is <= 3, or <= 4 when either atom is a hydrogen.  Same row: aa_sep[type][x][y].  Rows i and
//      i + 1 with link_prev[i + 1]: sep(x, slot 2) + 1 + sep(y, slot 0).  Rows with link[i] == j and link[j] == i: sep(x, slot 5) + 1 +
//      sep(y, slot 5).  The smallest of those that apply; any other pair of rows is never excluded.
//   6  OBSTACLE atom o (r_o > 0) of the segment's range against every counted atom: steps 1 - 4 with t = (rx + r_o) - cut, step 3's
//      condition being that x is a polar hydrogen and obst_polar[o] != 0; no exclusions
#pragma once
#include "pp_vec.h"

#define AA_S PP_AA_SLOTS
#define AA_SAT 8u                      // sticky bit 3: a table entry or residue type out of range

// NERF: H - p of a hydrogen on parent p with a the parent's one neighbour and b a neighbour of a, from the bond length L, cos / sin
// (c1, s1) of the angle H-p-a and (c2, s2) of the dihedral H-p-a-b:
//   qa = a - p, qb = b - p;  e = unit(-qa);  n = unit((qa - qb) x e);  m = n x e;
//   H - p = ((k0 e) + (k1 m)) + (k2 n),  k0 = -(L c1), k1 = (L s1) c2, k2 = (L s1) s2
// Every vector is a difference to p, so the caller's H = p + (H - p) is the only operation with an error of the size of the coordinates.
__device__ __forceinline__ pp_v3 pp_nerf(pp_v3 P, const float *a, const float *b, float L, float c1, float s1, float c2, float s2) {
#pragma clang fp contract(off)
    const pp_v3 qa = pp_sub(a, P), qb = pp_sub(b, P);
    const pp_v3 e = pp_unit({-qa.x, -qa.y, -qa.z});
    const pp_v3 nn = pp_unit(pp_cross({qa.x - qb.x, qa.y - qb.y, qa.z - qb.z}, e));
    const pp_v3 m = pp_cross(nn, e);
    const float k0 = -(L * c1), k1 = (L * s1) * c2, k2 = (L * s1) * s2;
    return {((k0 * e.x) + (k1 * m.x)) + (k2 * nn.x), ((k0 * e.y) + (k1 * m.y)) + (k2 * nn.y), ((k0 * e.z) + (k1 * m.z)) + (k2 * nn.z)};
}

// (position, radius of a counted atom or 0) of slot `slot` of row n
__device__ __forceinline__ float4 pp_aa_atom(const float *xyz, const float *hxyz, const uint8_t *hmask, const float *radius, int n,
                                             int slot) {
    const float *src = slot < 14 ? xyz + (size_t)n * 42 + 3 * slot : hxyz + ((size_t)n * PP_H_MAX + (slot - 14)) * 3;
    float r = radius[(size_t)n * AA_S + slot];
    if (!(r > 0.f) || (slot >= 14 && hmask[(size_t)n * PP_H_MAX + (slot - 14)] == 0)) r = 0.f;
    return make_float4(src[0], src[1], src[2], r);
}
// the atom's word: class | sep(a, 0) << 4 | sep(a, 2) << 8 | sep(a, 5) << 12, separations capped at 15.  A residue type outside
// 0 .. 20 is never used as an index: the atom is not counted (p.w = 0, word 0) and, if it was, the sticky bit is set
__device__ __forceinline__ int pp_aa_word(float4 &p, const uint8_t *acls, const uint8_t *aa_sep, long long ty, int n, int slot,
                                          unsigned *sat) {
    if (ty < 0 || ty > 20) {
        if (p.w > 0.f) atomicOr(sat, AA_SAT);
        p.w = 0.f;
        return 0;
    }
    const uint8_t *sp = aa_sep + ((size_t)ty * AA_S + slot) * AA_S;
    const int s0 = sp[0] > 15 ? 15 : sp[0], s2 = sp[2] > 15 ? 15 : sp[2], s5 = sp[5] > 15 ? 15 : sp[5];
    return (acls[(size_t)n * AA_S + slot] & 15) | (s0 << 4) | (s2 << 8) | (s5 << 12);
}
// what atom p adds to the row sphere around ca: its distance from ca plus its radius
__device__ __forceinline__ float pp_aa_extent(const float4 p, const float *ca) {
#pragma clang fp contract(off)
    const float dx = p.x - ca[0], dy = p.y - ca[1], dz = p.z - ca[2];
    return sqrtf(pp_dot3(dx, dy, dz, dx, dy, dz)) + p.w;
}

// the row sphere: pp_nanmax of m, and the OR of any, over the 32 lanes of a row
__device__ __forceinline__ void pp_aa_row_sphere(float &m, bool &any) {
    for (int w = 16; w > 0; w >>= 1) {
        const float o = __shfl_xor(m, w, 32);
        const int oa = __shfl_xor(any ? 1 : 0, w, 32);
        m = pp_nanmax(m, o);
        any = any || oa != 0;
    }
}

// step 5: the bond separation of x (word xi) and y, whose word holds y0 = sep(y, slot 0) at bits 4 .. 7, y2 at 8 .. 11, y5 at 12 .. 15;
// own: the same row, *own_sep = aa_sep[type][x][y]; rel_next / rel_prev / rel_ss: the partner's row is i + 1 with link_prev, i - 1 with
// link_prev[i], or the row's disulfide partner; 99: not bonded
__device__ __forceinline__ int pp_aa_sep(bool own, bool rel_next, bool rel_prev, bool rel_ss, int xi, int y0, int y2, int y5,
                                         const uint8_t *own_sep) {
    int sep = 99;
    if (own) sep = *own_sep;
    if (rel_next) sep = min(sep, ((xi >> 8) & 15) + 1 + y0);
    if (rel_prev) sep = min(sep, ((xi >> 4) & 15) + 1 + y2);
    if (rel_ss) sep = min(sep, ((xi >> 12) & 15) + 1 + y5);
    return sep;
}
// step 5: a pair is excluded iff its separation is not above this; hyd: either atom is a hydrogen (class bit 2)
__device__ __forceinline__ int pp_aa_excl(bool hyd) { return hyd ? 4 : 3; }
