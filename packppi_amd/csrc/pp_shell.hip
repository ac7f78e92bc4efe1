// Shell masks (no reference kernel): "which rows lie near these rows", per complex, on the device.  CA mode is
// the local mask of AffinityPrediction.get_local_subgraph (AffinityPrediction.py:124-145); ATOM mode with PP_SHELL_OTHER_CHAIN and
// every row a seed is the interface selection.  The result is the `fixed` byte array of pp_sample_partial / pp_proximal_pinned
// inverted, made without a read-back.
//
// DEFINITION, per segment of the context's segment table (the complexes of a packed ctx, the B rows of a padded one, padding rows
// included).  shell[n] = 1 iff a row j of the SAME segment exists with seeds[j] != 0, (PP_SHELL_OTHER_CHAIN) chain_indices[j] !=
// chain_indices[n], and
//   PP_SHELL_CA     d2(xyz[n][1], xyz[j][1]) < r2                                        (atom14 slot 1 = CA; atom_mask not read)
//   PP_SHELL_ATOM   atoms a of n, b of j with atom_mask[n][a] != 0, atom_mask[j][b] != 0 and d2(xyz[n][a], xyz[j][b]) < r2.
// j = n counts: a seed row is in its own shell (CA mode; ATOM mode if it has an atom; never under PP_SHELL_OTHER_CHAIN).
// residue_mask is not consulted.  count[s] = the number of shell rows of segment s.
//
// ARITHMETIC (fp32, every operation rounded on its own: fp contract off).  d = p - q per component,
// d2 = ((dx dx) + (dy dy)) + (dz dz), r2 = radius radius computed once on the host in fp32, the comparison is the strict d2 < r2.
// A NaN coordinate gives a NaN d2, which is not < r2.  A NumPy float32 restatement gives the same bytes.
//
// LAUNCH.  One kernel (behind one memset of count): workgroup w owns rows 256 w .. 256 w + 255; thread t decides row n = 256 w + t
// and is the only writer of shell[n].  The rows that can be partners of the workgroup's rows are the rows of the segments its first
// and last row lie in, lo .. hi - 1.  The workgroup walks them 256 at a time: thread t looks at row lo + 256 k + t and, if it is a
// seed, appends it to a list in LDS (row, segment, chain, CA, and in ATOM mode its atom bits and bounding radius); then every thread
// tests its row against the list.  Few seeds x all rows -- a mutation scan -- costs one pass over the seed bytes and a handful of
// distance tests per row; all x all -- an interface -- costs the full pair loop.  The list order comes from an LDS atomic and does
// not matter: the result is an OR over it.
//
// PRUNING, ATOM mode.  A row's bounding radius is rad = max over its present atoms of |atom - xyz[row][1]|, computed in this launch
// from the coordinates given (never from the plan's per-type extents: xyz is caller data).  By the triangle inequality no atom pair
// of (n, j) is closer than |CA_n - CA_j| - rad_n - rad_j, so the pair is skipped when
//     d2(CA_n, CA_j) > ((radius + rad_n + rad_j) 1.001 + 0.01)^2.
// Every fp32 quantity here is within a few 2^-24 of its real value (a difference of two floats is correctly rounded, so d, d2 and
// the square roots carry relative errors only); the 0.1 % + 0.01 slack is four orders above that, so a skipped pair has no atom pair
// with a computed d2 < r2: not one output byte changes.  A NaN or infinite radius or CA makes the comparison false and the pair is
// tested in full.  A row without a present atom is in no ATOM shell and seeds none; it is dropped where the list is made.
#include "pp_internal.h"
#include "pp_vec.h"

#define SH_T 256        // threads of a workgroup = rows it decides = seed candidates it looks at per pass

// present-atom bits of a row and its bounding radius around slot 1 (-1: no atom present)
__device__ __forceinline__ unsigned sh_row_atoms(const float *__restrict__ xyz, const float *__restrict__ amask, int n, float &rad) {
    const float *p = xyz + (size_t)n * 42;
    unsigned bits = 0;
    float m2 = -1.f;
    for (int a = 0; a < 14; a++)
        if (amask[(size_t)n * 14 + a] != 0.f) {
            bits |= 1u << a;
            const float d2 = pp_d2(p[3 * a], p[3 * a + 1], p[3 * a + 2], p[3], p[4], p[5]);
            m2 = (d2 > m2 || d2 != d2) ? d2 : m2;           // a NaN sticks: the pair is then never pruned
        }
    rad = bits ? sqrtf(m2) : -1.f;
    return bits;
}

template <bool ATOM>
__global__ void __launch_bounds__(SH_T)
k_shell(int N, int n_seg, const int32_t *__restrict__ seg_off, const uint8_t *__restrict__ seeds, const float *__restrict__ xyz,
        const float *__restrict__ amask, const int64_t *__restrict__ chain, float radius, float r2, uint8_t *__restrict__ shell,
        int32_t *__restrict__ count) {
#pragma clang fp contract(off)
    __shared__ int l_row[SH_T], l_seg[SH_T];
    __shared__ long long l_chain[SH_T];
    __shared__ float l_ca[SH_T][3], l_rad[SH_T];
    __shared__ unsigned l_bits[SH_T];
    __shared__ int l_n;
    const int tid = threadIdx.x;
    const long long first = (long long)blockIdx.x * SH_T;
    if (first >= N) return;
    const int n = (int)first + tid;
    const bool live = n < N;
    const int last = (int)(first + SH_T - 1 < N ? first + SH_T - 1 : N - 1);
    // the partner rows of this workgroup: the segments of its first and last row (clamped into the batch by pp_seg_rows)
    const int s_first = pp_seg_of_row(seg_off, n_seg, (int)first), s_last = pp_seg_of_row(seg_off, n_seg, last);
    int lo, hi, t0, t1;
    pp_seg_rows(seg_off, s_first, N, lo, t0);
    pp_seg_rows(seg_off, s_last, N, t1, hi);
    if (hi < lo) hi = lo;

    int my_seg = -1;
    long long my_chain = 0;
    float cx = 0.f, cy = 0.f, cz = 0.f, my_rad = -1.f;
    unsigned my_bits = 0;
    float ax[ATOM ? 14 : 1][3];
    if (live) {
        my_seg = pp_seg_of_row(seg_off, n_seg, n);
        int a, b;
        pp_seg_rows(seg_off, my_seg, N, a, b);
        if (n < a || n >= b) my_seg = -1;                   // a table that breaks the contract: the row is in no segment
        if (chain) my_chain = chain[n];
        const float *p = xyz + (size_t)n * 42;
        cx = p[3]; cy = p[4]; cz = p[5];
        if (ATOM) {
            my_bits = sh_row_atoms(xyz, amask, n, my_rad);
            for (int a2 = 0; a2 < 14; a2++)
                for (int k = 0; k < 3; k++) ax[a2][k] = p[3 * a2 + k];
        }
    }
    bool hit = false;
    const bool can = live && my_seg >= 0 && (!ATOM || my_bits != 0);

    for (int base = lo; base < hi; base += SH_T) {
        if (tid == 0) l_n = 0;
        __syncthreads();
        const int j = base + tid;
        if (j < hi && seeds[j] != 0) {
            float rad = 0.f;
            unsigned bits = 1;
            if (ATOM) bits = sh_row_atoms(xyz, amask, j, rad);
            if (bits) {
                const int e = atomicAdd(&l_n, 1);
                const float *q = xyz + (size_t)j * 42;
                l_row[e] = j;
                l_seg[e] = pp_seg_of_row(seg_off, n_seg, j);
                l_chain[e] = chain ? chain[j] : 0;
                l_ca[e][0] = q[3]; l_ca[e][1] = q[4]; l_ca[e][2] = q[5];
                l_rad[e] = rad;
                l_bits[e] = bits;
            }
        }
        __syncthreads();
        const int cnt = l_n;
        if (can && !hit) {
            for (int e = 0; e < cnt; e++) {
                if (l_seg[e] != my_seg) continue;
                if (chain && l_chain[e] == my_chain) continue;
                const float dca2 = pp_d2(cx, cy, cz, l_ca[e][0], l_ca[e][1], l_ca[e][2]);
                if (!ATOM) {
                    if (dca2 < r2) { hit = true; break; }
                    continue;
                }
                const float bound = (radius + my_rad + l_rad[e]) * 1.001f + 0.01f;
                if (dca2 > bound * bound) continue;
                const float *q = xyz + (size_t)l_row[e] * 42;
                const unsigned jb = l_bits[e];
                for (int b2 = 0; b2 < 14 && !hit; b2++) {
                    if (!((jb >> b2) & 1u)) continue;
                    const float qx = q[3 * b2], qy = q[3 * b2 + 1], qz = q[3 * b2 + 2];
#pragma unroll
                    for (int a2 = 0; a2 < (ATOM ? 14 : 1); a2++)
                        if (((my_bits >> a2) & 1u) && pp_d2(ax[a2][0], ax[a2][1], ax[a2][2], qx, qy, qz) < r2) hit = true;
                }
                if (hit) break;
            }
        }
        __syncthreads();
    }
    if (live) shell[n] = hit ? 1 : 0;
    if (count) {
        if (s_first == s_last) {                             // the usual case: one integer atomic per workgroup
            const int c = __syncthreads_count(hit ? 1 : 0);
            if (tid == 0 && c) atomicAdd(&count[s_first], c);
        } else if (hit) {
            atomicAdd(&count[my_seg], 1);
        }
    }
}

extern "C" pp_status pp_ctx_shell(pp_ctx *c, const uint8_t *seeds, int mode, float radius, int flags, const float *xyz,
                                  uint8_t *shell, int32_t *count, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !seeds || !shell) FAIL(PP_ERR_INVALID, "pp_ctx_shell: null argument");
    if (mode != PP_SHELL_CA && mode != PP_SHELL_ATOM) FAIL(PP_ERR_INVALID, "pp_ctx_shell: mode must be PP_SHELL_CA or PP_SHELL_ATOM");
    if (flags & ~PP_SHELL_OTHER_CHAIN) FAIL(PP_ERR_INVALID, "pp_ctx_shell: unknown flag bit");
    if (!std::isfinite(radius) || !(radius > 0.f)) FAIL(PP_ERR_INVALID, "pp_ctx_shell: radius must be finite and positive");
    if (mode == PP_SHELL_ATOM && !c->b.atom_mask) FAIL(PP_ERR_INVALID, "pp_ctx_shell: PP_SHELL_ATOM needs a batch with atom_mask");
    if ((flags & PP_SHELL_OTHER_CHAIN) && !c->b.chain_indices)
        FAIL(PP_ERR_INVALID, "pp_ctx_shell: PP_SHELL_OTHER_CHAIN needs a batch with chain_indices");
    if (!xyz) xyz = c->b.X;
    if (!xyz) FAIL(PP_ERR_INVALID, "pp_ctx_shell: no coordinates (xyz is null and the batch has no X)");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (count) PP_HIP_CHECK(hipMemsetAsync(count, 0, (size_t)c->B * sizeof(int32_t), st));
    if (c->N < 1) return PP_OK;
    const float r2 = radius * radius;
    const int64_t *chain = (flags & PP_SHELL_OTHER_CHAIN) ? c->b.chain_indices : nullptr;
    const dim3 grid((unsigned)((c->N + SH_T - 1) / SH_T)), block(SH_T);
    if (mode == PP_SHELL_ATOM)
        hipLaunchKernelGGL(k_shell<true>, grid, block, 0, st, c->N, c->B, c->seg_off, seeds, xyz, c->b.atom_mask, chain, radius, r2,
                           shell, count);
    else
        hipLaunchKernelGGL(k_shell<false>, grid, block, 0, st, c->N, c->B, c->seg_off, seeds, xyz, (const float *)nullptr, chain,
                           radius, r2, shell, count);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
