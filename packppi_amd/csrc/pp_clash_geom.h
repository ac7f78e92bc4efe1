// The backbone-only geometry behind every STATIC clash list (device only; pp_clash.hip: k_clash_cand, k_obst_cand; pp_recombine.hip:
// rc_row), written once so that the lists keep resting on one bound.
//
// The Adam loop and the recombination move side chains, never the backbone.  Let e_n be how far an atom of row n can be from its CA
// for ANY chi (cl_extent).  Atoms of rows i and j can only ever overlap if |CA_i - CA_j| < e_i + e_j + cl_reach(tol), and an atom of
// row i can only ever overlap obstacle o if |CA_i - q_o| < e_i + r_o + cl_obst_reach(tol): outside of that the hinge
// max(r_a + r_b - tol - dist, 0) is zero at every angle.  A list made with these limits is a superset of every pair whose hinge can
// be non-zero at any angles, so a kernel that reads the list instead of scanning adds the same numbers.
//
// The CA-distance comparisons themselves stay with their kernels: rc_near must be symmetric and is compiled with contraction off,
// k_clash_cand's is not, and merging them would change which marginal pairs enter k_clash_cand's lists.
#pragma once

#define CL_RA_MAX 1.8f            // the largest between-residue radius of a protein atom (S)
// largest r_a + r_b - tol of two protein atoms: 3.6 = 2 x 1.8, S against S
__device__ __forceinline__ float cl_reach(float tol) { return 2.f * CL_RA_MAX - tol; }
// largest r_a - tol of a protein atom against an obstacle, whose own radius the caller adds
__device__ __forceinline__ float cl_obst_reach(float tol) { return CL_RA_MAX - tol; }

// Row n of the batch: its CA into ca, and its extent e = the side-chain bound of the residue type (side_extent, pp_plan::side_extent:
// over all chi) or the actual distance of its N / C / O from CA, times 1.0001 plus 1e-3 (a margin over the rounding), whichever is
// larger.  X [.][14][3] holds N, CA, C, O first; amask [.][14] says which atoms exist.
__device__ __forceinline__ float cl_extent(const float *__restrict__ X, const float *__restrict__ amask, const int64_t *__restrict__ rtype,
                                           const float *__restrict__ side_extent, int n, float (&ca)[3]) {
    const float *x = X + (size_t)n * 42;
    ca[0] = x[3]; ca[1] = x[4]; ca[2] = x[5];
    float e = side_extent[(int)rtype[n]];
    const float *m = amask + (size_t)n * 14;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        if (a == 1 || m[a] == 0.f) continue;
        const float dx = x[3 * a] - ca[0], dy = x[3 * a + 1] - ca[1], dz = x[3 * a + 2] - ca[2];
        e = fmaxf(e, sqrtf(dx * dx + dy * dy + dz * dz) * 1.0001f + 1e-3f);
    }
    return e;
}
