// All-atom chi refinement: a conservative descent in chi space on the explicit-hydrogen overlap energy (no reference kernel;
// DESIGN.md section 32).  One entry, pp_chi_refine, per segment of the context's segment table; nothing crosses segments.  Chemistry
// is caller data, as for pp_clashscore / pp_hnet_optimize, whose slots, class bits, separations and atom record are pp_allatom.h's
// here as there; the overlap test is written out in rf_term as hn_term (pp_hnet.hip) and k_clashscore (pp_hydrogens.hip) write it.
//
// MOVERS.  A row is a MOVER iff residue_mask != 0, one of its SC_D_mask entries != 0, it is not in `fixed`, and its residue_type lies
// in 0 .. 20.  Its state is steps int8 [4]; angle j of the state is
//     steps[j] == 0:  chi0[j], the caller's bits
//     else:           a = chi0[j] + ((float)steps[j] delta);  a >= PI: a - 2PI;  a < -PI: a + 2PI    (PI = 3.14159274f, 2PI = 6.28318548f)
// always from chi0: nothing drifts.  CANDIDATES of a sweep: 0 the current state, 1 + 2j / 2 + 2j the current state with steps[j] + 1 /
// - 1; candidate c > 0 EXISTS iff SC_D_mask[j] != 0 and |steps[j] +- 1| <= max_steps.  The coordinates of a candidate are what
// pp_atom14 and pp_hydrogens compute at its angles: the entry runs those two over a buffer of candidate angles, once per candidate
// and sweep, so they are the project's own bits by construction (pp_launch_atom14, pp_hydrogens: the launches of the public entries).
// MOVED atoms of a mover: the atom14 slots 5 .. 13 and every hydrogen of the type whose parent or one of whose neighbours in `place`
// is such a slot (the hydrogens on CB are built from CG: they turn with chi1).  At most 9 + 13 = PP_REFINE_MOVED.
//
// ENERGY (int32).  A pair term exists for a moved atom x of mover r against any other counted atom y of the segment that is not a
// moved atom of r, and against every obstacle atom (r_o > 0) of the segment's range.  fp32, contract off:
//   excluded  step 5 of the pair rules of pp_allatom.h (never for an obstacle)
//   t         their steps 2 - 3 (6 for an obstacle);  d2 of step 1
//   level     the number of k in 0 .. bands - 1 with  t_k > 0 and d2 <= t_k t_k,  t_k = t - ((float)k band);  0 for an excluded pair.
//             Level >= 1 is pp_clashscore's serious overlap; a NaN makes every comparison false.
//   bond      pp_hnet.hip's: 2 good, 1 weak, else 0
//   term      64 level - bond
// E_r(c | s) = the sum of the terms of r at candidate c, everything else at its state in s;  F(s) = every term once.
//
// SWEEP (DESIGN.md sections 18 and 30).  Propose: a mover WITH a term of level >= 1 at its current state takes the existing candidate
// of smallest E, the lowest index on ties, its own on a tie with it; gain = E(own) - E(proposed).  A mover without such a term has
// gain 0: a clean residue is never moved.  Apply: r moves iff gain_r > 0 and every partner with a positive gain has a smaller gain, or
// an equal one and a higher row.  Partners: pp_hnet.hip's predicate with ext = the caller's refine extents.  Two movers whose MOVED
// atoms can share a term in any states are partners, two accepted movers never are, so F drops by the sum of the accepted gains, in
// integers.  A segment without a positive gain is converged: its propose / apply launches return at once (the candidate builders are
// the entries' own launches over all rows; they rewrite the same bits).
//
// LAUNCH.  Per sweep k = 0 .. max_sweeps: k_rf_angles (the 9 candidate angle sets), 9 x (atom14, hydrogens), k_rf_prep (32 lanes per
// row: P / I of candidate 0 as k_hn_prep writes them, the row sphere over every existing candidate), k_rf_propose (one wave per mover,
// k_hn_propose's shape: the CA-sphere row filter through a ballot into LDS, the candidates' moved atoms and their parents in LDS, at
// most 9 x 22 x 16 B each, read as broadcasts; the per-candidate sums are compile-time indexed registers), and for k < max_sweeps
// k_rf_apply (one wave per mover: the accept rule, then steps[j] += +-1).  After sweep 0's prep: k_rf_compact and k_rf_partners (the
// backbone does not move: the lists hold for the call); a list beyond PP_REFINE_PCAP is scanned again in apply with the same
// predicate.  Candidate 0 of the last sweep is the result.  F of a sweep: every mover adds E(own) minus the terms against moved atoms
// of movers in lower rows to trace[segment][sweep] (integer atomics; the count of positive gains per segment and sweep is the only
// other one).  No read-back, no persistent kernel, no spin-wait, no float atomics.
// k_rf_compact, k_rf_partners and k_rf_finish_seg restate k_hn_compact, k_hn_partners and k_hn_finish_seg: kernels are not shared
// across translation units here, and pp_hnet.hip's instructions stay as they are.
#include "pp_internal.h"
#include "pp_allatom.h"

#define RF_T 64
#define RF_C PP_REFINE_CAND
#define RF_M PP_REFINE_MOVED
#define RF_NP (PP_REFINE_MAX_SWEEPS + 1)
#define RF_PI 3.14159274f
#define RF_2PI 6.28318548f

struct RfSets {                        // the candidate coordinate sets of the sweep: [RF_C][N] rows each
    const float *xyz, *hxyz;
    const uint8_t *hmask;
    size_t N;
};
__device__ __forceinline__ float4 rf_atom(const RfSets &S, const float *radius, int n, int slot, int c) {
    return pp_aa_atom(S.xyz + (size_t)c * S.N * 42, S.hxyz + (size_t)c * S.N * PP_H_MAX * 3, S.hmask + (size_t)c * S.N * PP_H_MAX, radius,
                      n, slot);
}

// angle j of a state: see the header of this file
__device__ __forceinline__ float rf_angle(float chi0, int st, float delta) {
#pragma clang fp contract(off)
    if (st == 0) return chi0;
    float a = chi0 + ((float)st * delta);
    if (a >= RF_PI) a = a - RF_2PI;
    if (a < -RF_PI) a = a + RF_2PI;
    return a;
}

// 16 lanes per row: lane c < 9 writes the angles of candidate c, lane 0 the candidate mask (0: no mover)
__global__ void __launch_bounds__(256)
k_rf_angles(int N, const float *__restrict__ chi0, const int8_t *__restrict__ steps, const float *__restrict__ rmask,
            const float *__restrict__ scd_mask, const uint8_t *__restrict__ fixed, const int64_t *__restrict__ rtype, float delta,
            int max_steps, float *__restrict__ chiC, int32_t *__restrict__ cmask) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n = t >> 4, c = t & 15;
    if (n >= N) return;
    const float *sm = scd_mask + (size_t)n * 4;
    const long long ty = rtype[n];
    const bool mover = rmask[n] != 0.f && (sm[0] != 0.f || sm[1] != 0.f || sm[2] != 0.f || sm[3] != 0.f) && !(fixed && fixed[n] != 0) &&
                       ty >= 0 && ty <= 20;
    int st[4];
    for (int j = 0; j < 4; j++) st[j] = mover ? steps[(size_t)n * 4 + j] : 0;
    bool exists = mover;
    if (c > 0 && c < RF_C) {
        const int j = (c - 1) >> 1, v = st[j] + ((c & 1) ? 1 : -1);
        exists = mover && sm[j] != 0.f && v <= max_steps && v >= -max_steps;
        if (exists) st[j] = v;
    }
    if (c < RF_C)
        for (int j = 0; j < 4; j++) chiC[((size_t)c * N + n) * 4 + j] = rf_angle(chi0[(size_t)n * 4 + j], st[j], delta);
    int bits = (exists && c < RF_C) ? (1 << c) : 0;
    for (int w = 8; w > 0; w >>= 1) bits |= __shfl_xor(bits, w, 16);
    if (c == 0) cmask[n] = bits;
}

// the moved slots of residue type ty (0 .. 20): see the header of this file.  A `place` entry is compared, never used as an index
__device__ __forceinline__ unsigned rf_moved_mask(const int8_t *place, long long ty) {
    unsigned mask = 0x3fe0u;                                   // slots 5 .. 13
    for (int k = 0; k < PP_H_MAX; k++) {
        const int8_t *pl = place + ((size_t)ty * PP_H_MAX + k) * 5;
        if (pl[0] == 0) continue;
        bool mv = false;
        for (int q = 1; q < 5; q++) mv = mv || (pl[q] >= 5 && pl[q] <= 13);
        if (mv) mask |= 1u << (14 + k);
    }
    return mask;
}

// 32 lanes per row: P / I of candidate 0, the row sphere over every existing candidate, the moved mask of a mover
__global__ void __launch_bounds__(256)
k_rf_prep(int N, RfSets S, const float *__restrict__ radius, const uint8_t *__restrict__ acls, const uint8_t *__restrict__ aa_sep,
          const int64_t *__restrict__ rtype, const int8_t *__restrict__ place, const int32_t *__restrict__ cmask,
          float4 *__restrict__ P, int32_t *__restrict__ I, float4 *__restrict__ row, int32_t *__restrict__ mmask,
          unsigned *__restrict__ sat) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n = t >> 5, a = t & 31;
    const bool rowok = n < N;
    const long long ty = rowok ? rtype[n] : 0;
    const bool tyok = ty >= 0 && ty <= 20;
    const int cm = rowok ? cmask[n] : 0;
    const unsigned mask = (cm != 0 && tyok) ? rf_moved_mask(place, ty) : 0u;      // the same in the 32 lanes of a row
    const float *ca = S.xyz + (size_t)(rowok ? n : 0) * 42 + 3;
    float m = -1.f;
    bool any = false;
    const bool live = rowok && a < AA_S;
    if (live) {
        float4 at = rf_atom(S, radius, n, a, 0);
        int word = pp_aa_word(at, acls, aa_sep, ty, n, a, sat);
        if (tyok && a >= 14) {
            const int par = place[((size_t)ty * PP_H_MAX + (a - 14)) * 5 + 1];
            word |= ((par < 0 || par > 13) ? 0 : par) << 16;    // such a hydrogen was dropped by pp_hydrogens: it is not counted
        }
        const bool mine = ((mask >> a) & 1u) != 0u;
        if (at.w > 0.f) {
            any = true;
            m = pp_aa_extent(at, ca);
        }
        if (mine) {
            for (int c = 1; c < RF_C; c++) {
                if (!((cm >> c) & 1)) continue;
                const float4 q = rf_atom(S, radius, n, a, c);
                if (q.w > 0.f) {
                    any = true;
                    m = pp_nanmax(m, pp_aa_extent(q, ca));
                }
            }
        }
        P[(size_t)n * AA_S + a] = at;
        I[(size_t)n * AA_S + a] = word | (mine ? (1 << 20) : 0);
    }
    pp_aa_row_sphere(m, any);
    if (rowok && a == 0) {
        row[n] = make_float4(ca[0], ca[1], ca[2], any ? m : -1.f);
        mmask[n] = (int32_t)mask;
    }
}

// the movers in ascending row order (k_hn_compact)
__global__ void __launch_bounds__(1024)
k_rf_compact(int N, const int32_t *__restrict__ mmask, int32_t *__restrict__ movers, int32_t *__restrict__ n_movers) {
    __shared__ int l_cnt[16];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    int base = 0;
    for (int start = 0; start < N; start += 1024) {
        const int n = start + tid;
        const bool f = n < N && mmask[n] != 0;
        const unsigned long long b = __ballot(f);
        if (lane == 0) l_cnt[w] = __popcll(b);
        __syncthreads();
        int off = base, total = 0;
        for (int q = 0; q < 16; q++) {
            if (q < w) off += l_cnt[q];
            total += l_cnt[q];
        }
        if (f) movers[off + __popcll(b & ((1ull << lane) - 1ull))] = n;
        base += total;
        __syncthreads();
    }
    if (tid == 0) n_movers[0] = base;
}

// P(r): pp_hnet.hip's hn_partner.  Both rows are movers, so their types are in range.
__device__ __forceinline__ bool rf_partner(const float4 ci, const float4 cj, float ei, float ej, float reach) {
#pragma clang fp contract(off)
    const float b = (ei + ej) + reach;
    const float dx = cj.x - ci.x, dy = cj.y - ci.y, dz = cj.z - ci.z;
    return pp_dot3(dx, dy, dz, dx, dy, dz) <= b * b;
}

__global__ void __launch_bounds__(RF_T)
k_rf_partners(int N, int n_seg, const int32_t *__restrict__ seg_off, const int32_t *__restrict__ movers,
              const int32_t *__restrict__ n_movers, const int32_t *__restrict__ mmask, const float4 *__restrict__ rowinfo,
              const int64_t *__restrict__ rtype, const float *__restrict__ ext, float reach, int32_t *__restrict__ plist,
              int32_t *__restrict__ pcount) {
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n_movers[0]) return;
    const int i = movers[blockIdx.x];
    const int s = pp_seg_of_row(seg_off, n_seg, i);
    int lo, hi;
    pp_seg_rows(seg_off, s, N, lo, hi);
    const float4 ci = rowinfo[i];
    const float ei = ext[rtype[i]];
    int cnt = 0;
    for (int base = lo; base < hi; base += RF_T) {
        const int j = base + lane;
        bool f = false;
        if (j < hi && j != i && mmask[j] != 0) f = rf_partner(ci, rowinfo[j], ei, ext[rtype[j]], reach);
        const unsigned long long b = __ballot(f);
        if (f) {
            const int pos = cnt + __popcll(b & ((1ull << lane) - 1ull));
            if (pos < PP_REFINE_PCAP) plist[(size_t)i * PP_REFINE_PCAP + pos] = j;
        }
        cnt += __popcll(b);
    }
    if (lane == 0) pcount[i] = cnt;
}

struct RfPhys {
    float cut, hb_allow, hb_weak, hb_weak2, hb_good2, band;
    int bands;
};

// the term of moved atom (p, class word xi, parent at dp) against atom (q, yi, parent at dq) whose exclusion is settled: ok = a pair
// that is not excluded; far = the atoms are in different rows (or y is an obstacle).  hn_term with the graded overlap
__device__ __forceinline__ int rf_term(const float4 p, int xi, const float4 dp, const float4 q, int yi, const float4 dq, bool ok,
                                       bool far, const RfPhys &ph) {
#pragma clang fp contract(off)
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    const float d2 = pp_dot3(dx, dy, dz, dx, dy, dz);
    float t = (p.w + q.w) - ph.cut;
    const bool xh = (xi & 1) && (yi & 2), yh = (xi & 2) && (yi & 1);
    if (xh || yh) t = t - ph.hb_allow;
    int level = 0;
    for (int k = 0; k < ph.bands; k++) {
        const float tk = t - ((float)k * ph.band);
        level += (tk > 0.f && d2 <= tk * tk) ? 1 : 0;
    }
    int v = ok ? 64 * level : 0;
    if (ok && far && (xh || yh)) {
        // v = A - h, w = D - h
        const float vx = xh ? dx : -dx, vy = xh ? dy : -dy, vz = xh ? dz : -dz;
        const float wx = xh ? dp.x - p.x : dq.x - q.x, wy = xh ? dp.y - p.y : dq.y - q.y, wz = xh ? dp.z - p.z : dq.z - q.z;
        const float s = pp_dot3(vx, vy, vz, wx, wy, wz), ww = pp_dot3(wx, wy, wz, wx, wy, wz);
        const bool weak = d2 <= ph.hb_weak2 && s <= 0.f;
        const bool good = weak && d2 <= ph.hb_good2 && (s * s) >= 0.25f * (ww * d2);
        v -= good ? 2 : (weak ? 1 : 0);
    }
    return v;
}

__global__ void __launch_bounds__(RF_T)
k_rf_propose(int N, int n_seg, const int32_t *__restrict__ seg_off, int sweep, const int32_t *__restrict__ movers,
             const int32_t *__restrict__ n_movers, const float4 *__restrict__ P, const int32_t *__restrict__ I,
             const float4 *__restrict__ rowinfo, RfSets S, const float *__restrict__ radius, const int64_t *__restrict__ rtype,
             const uint8_t *__restrict__ aa_sep, const uint8_t *__restrict__ link_prev, const int32_t *__restrict__ link,
             const float4 *__restrict__ oatoms, const int2 *__restrict__ oseg, const uint8_t *__restrict__ opolar, RfPhys ph,
             const int32_t *__restrict__ cmask, const int32_t *__restrict__ mmask, int32_t *__restrict__ prop,
             int32_t *__restrict__ gain, int32_t *__restrict__ npos, int32_t *__restrict__ e_out, int32_t *__restrict__ trace,
             int tr_stride, int32_t *__restrict__ energy) {
#pragma clang fp contract(off)
    __shared__ float4 l_own[RF_C * RF_M];                      // [candidate][moved atom]: position, radius of a counted atom or 0
    __shared__ float4 l_par[RF_C * RF_M];                      // its parent at that candidate (hydrogens)
    __shared__ int l_slot[RF_M], l_xi[RF_M];
    __shared__ uint8_t l_sep[AA_S * AA_S + 7];
    __shared__ int l_rows[RF_T];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n_movers[0]) return;
    const int i = movers[blockIdx.x];
    const int s = pp_seg_of_row(seg_off, n_seg, i);
    if (sweep > 0 && npos[(size_t)s * RF_NP + sweep - 1] == 0) return;      // the segment converged in an earlier sweep
    int lo, hi;
    pp_seg_rows(seg_off, s, N, lo, hi);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int cm = cmask[i];
    const unsigned mask = (unsigned)mmask[i];
    const int nx = min(__popc(mask), RF_M);
    {
        const long long ty = rtype[i];                         // a mover: in range
        for (int q = lane; q < AA_S * AA_S; q += RF_T) l_sep[q] = aa_sep[(size_t)ty * AA_S * AA_S + q];
    }
    if (lane < nx) {
        unsigned mm = mask;
        for (int q = 0; q < lane; q++) mm &= mm - 1u;
        const int slot = __ffs((int)mm) - 1;
        l_slot[lane] = slot;
        l_xi[lane] = I[(size_t)i * AA_S + slot];
    }
    __syncthreads();
    for (int q = lane; q < RF_C * nx; q += RF_T) {
        const int c = q / nx, xk = q - c * nx, slot = l_slot[xk];
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f), d = p;
        if ((cm >> c) & 1) {
            p = rf_atom(S, radius, i, slot, c);
            if (slot >= 14) {
                const float *src = S.xyz + ((size_t)c * S.N + i) * 42 + 3 * ((l_xi[xk] >> 16) & 15);
                d = make_float4(src[0], src[1], src[2], 0.f);
            }
        }
        l_own[c * RF_M + xk] = p;
        l_par[c * RF_M + xk] = d;
    }
    const float4 ri = rowinfo[i];
    __syncthreads();

    int e[RF_C];
#pragma unroll
    for (int c = 0; c < RF_C; c++) e[c] = 0;
    int dup = 0;                                               // terms of candidate 0 against moved atoms of movers in lower rows
    int hot = 0;                                               // candidate 0 has a term of level >= 1
    const int lpi = link_prev[i];
    const int lki = link ? link[i] : -1;
    const float g = fmaxf(-ph.cut, ph.hb_weak);
    for (int base = lo; base < hi; base += RF_T) {
        const int j = base + lane;
        bool keep = false;
        if (j < hi) {
            const float4 rj = rowinfo[j];
            if (j == i) {
                keep = true;
            } else if (!(rj.w < 0.f)) {
                const float bound = (((ri.w + rj.w) + g) * 1.001f) + 0.01f;
                const float dx = rj.x - ri.x, dy = rj.y - ri.y, dz = rj.z - ri.z;
                keep = !(pp_dot3(dx, dy, dz, dx, dy, dz) > bound * bound);
            }
        }
        const unsigned long long kept = __ballot(keep);
        if (kept == 0ull) continue;                           // the same in every lane
        if (keep) l_rows[__popcll(kept & below)] = j;         // ascending rows
        __syncthreads();
        const int nr = __popcll(kept);
        for (int r0 = 0; r0 < nr; r0 += 2) {
            const int r = r0 + (lane >> 5), a = lane & 31;
            const bool valid = r < nr && a < AA_S;
            int jj = i, yi = 0;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f), dq = q;
            bool rel_next = false, rel_prev = false, rel_ss = false;
            if (valid) {
                jj = l_rows[r];
                q = P[(size_t)jj * AA_S + a];
                yi = I[(size_t)jj * AA_S + a];
                rel_next = jj == i + 1 && link_prev[jj] != 0;
                rel_prev = jj == i - 1 && lpi != 0;
                rel_ss = jj != i && lki == jj && link[jj] == i;       // lki >= 0 only with link
            }
            const bool own = jj == i;
            const bool yok = valid && q.w > 0.f && !(own && ((mask >> a) & 1u));
            if (__ballot(yok) == 0ull) continue;
            if (yok && (yi & 1)) dq = P[(size_t)jj * AA_S + ((yi >> 16) & 15)];
            const bool lower = ((yi >> 20) & 1) && jj < i;
            const int y0 = (yi >> 4) & 15, y2 = (yi >> 8) & 15, y5 = (yi >> 12) & 15;
            const bool yhyd = (yi & 4) != 0;
#pragma unroll
            for (int c = 0; c < RF_C; c++) {
                if ((cm >> c) & 1) {                          // the same in every lane
                    int acc = 0;
#pragma nounroll
                    for (int xk = 0; xk < nx; xk++) {
                        const float4 p = l_own[c * RF_M + xk];
                        if (!(p.w > 0.f)) continue;           // the same in every lane
                        const int xi = l_xi[xk], x = l_slot[xk];
                        const int sep = pp_aa_sep(own, rel_next, rel_prev, rel_ss, xi, y0, y2, y5, &l_sep[x * AA_S + (valid ? a : 0)]);
                        const bool ok = yok && sep > pp_aa_excl((xi & 4) || yhyd);
                        const int v = rf_term(p, xi, l_par[c * RF_M + xk], q, yi, dq, ok, !own, ph);
                        acc += v;
                        if (c == 0 && v > 32) hot = 1;
                    }
                    e[c] += acc;
                    if (c == 0 && lower) dup += acc;
                }
            }
        }
        __syncthreads();                                      // the list is rewritten by the next 64 rows
    }
    if (oatoms) {
        const int2 rg = oseg[s];
        const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int base = 0; base < rg.y; base += RF_T) {
            const int l = base + lane;
            bool pol = false;
            float4 o = none;
            if (l < rg.y) {
                o = oatoms[rg.x + l];
                pol = opolar && opolar[rg.x + l] != 0;
            }
            const bool ook = l < rg.y && o.w > 0.f;
            if (__ballot(ook) == 0ull) continue;
            const int oi = pol ? 2 : 0;                       // an obstacle is an acceptor or nothing
#pragma unroll
            for (int c = 0; c < RF_C; c++) {
                if ((cm >> c) & 1) {
                    int acc = 0;
#pragma nounroll
                    for (int xk = 0; xk < nx; xk++) {
                        const float4 p = l_own[c * RF_M + xk];
                        if (!(p.w > 0.f)) continue;
                        const int v = rf_term(p, l_xi[xk] & 1, l_par[c * RF_M + xk], o, oi, none, ook, true, ph);
                        acc += v;
                        if (c == 0 && v > 32) hot = 1;
                    }
                    e[c] += acc;
                }
            }
        }
    }
    // the wave's sums, the same in every lane afterwards
#pragma unroll
    for (int c = 0; c < RF_C; c++)
        for (int w = 32; w > 0; w >>= 1) e[c] += __shfl_xor(e[c], w);
    for (int w = 32; w > 0; w >>= 1) dup += __shfl_xor(dup, w);
    const bool is_hot = __ballot(hot != 0) != 0ull;
    const int e_cur = e[0];
    int best = 0, e_best = e_cur;
    if (is_hot) {
#pragma unroll
        for (int c = 1; c < RF_C; c++)
            if (((cm >> c) & 1) && e[c] < e_best) { best = c; e_best = e[c]; }
    }
    if (energy && sweep == 0) {
        int mine = 0;
#pragma unroll
        for (int c = 0; c < RF_C; c++) mine = (c == lane && ((cm >> c) & 1)) ? e[c] : mine;
        if (lane < RF_C) energy[(size_t)i * RF_C + lane] = mine;
    }
    if (lane == 0) {
        prop[i] = best;
        gain[i] = e_cur - e_best;
        if (sweep == 0) e_out[(size_t)i * 2] = e_cur;
        e_out[(size_t)i * 2 + 1] = e_cur;
        if (e_cur - dup != 0) atomicAdd(&trace[(size_t)s * tr_stride + sweep], e_cur - dup);
        if (e_cur - e_best > 0) atomicAdd(&npos[(size_t)s * RF_NP + sweep], 1);
    }
}

__global__ void __launch_bounds__(RF_T)
k_rf_apply(int N, int n_seg, const int32_t *__restrict__ seg_off, int sweep, const int32_t *__restrict__ movers,
           const int32_t *__restrict__ n_movers, const float4 *__restrict__ rowinfo, const int64_t *__restrict__ rtype,
           const float *__restrict__ ext, float reach, const int32_t *__restrict__ mmask, const int32_t *__restrict__ prop,
           const int32_t *__restrict__ gain, const int32_t *__restrict__ npos, const int32_t *__restrict__ plist,
           const int32_t *__restrict__ pcount, int8_t *__restrict__ steps) {
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n_movers[0]) return;
    const int i = movers[blockIdx.x];
    const int s = pp_seg_of_row(seg_off, n_seg, i);
    if (npos[(size_t)s * RF_NP + sweep] == 0) return;         // converged: nobody in the segment wants to move
    const int gi = gain[i];
    if (gi <= 0) return;
    const int cnt = pcount[i];
    bool blocked = false;
    if (cnt <= PP_REFINE_PCAP) {
        if (lane < cnt) {
            const int j = plist[(size_t)i * PP_REFINE_PCAP + lane];
            const int gj = gain[j];
            blocked = gj > 0 && !(gj < gi || (gj == gi && j > i));
        }
    } else {                                                  // the list did not hold them all: the same predicate over the segment
        int lo, hi;
        pp_seg_rows(seg_off, s, N, lo, hi);
        const float4 ci = rowinfo[i];
        const float ei = ext[rtype[i]];
        for (int base = lo; base < hi; base += RF_T) {
            const int j = base + lane;
            if (j < hi && j != i && mmask[j] != 0 && rf_partner(ci, rowinfo[j], ei, ext[rtype[j]], reach)) {
                const int gj = gain[j];
                blocked = blocked || (gj > 0 && !(gj < gi || (gj == gi && j > i)));
            }
        }
    }
    if (__ballot(blocked) != 0ull) return;
    if (lane == 0) {
        const int c = prop[i];                                // gain > 0: c is 1 .. 8
        if (c >= 1 && c < RF_C) {
            const size_t o = (size_t)i * 4 + ((c - 1) >> 1);
            steps[o] = (int8_t)(steps[o] + ((c & 1) ? 1 : -1));
        }
    }
}

// per segment: sweeps taken, converged, and F carried behind the sweep that converged (k_hn_finish_seg)
__global__ void __launch_bounds__(64)
k_rf_finish_seg(int n_seg, int max_sweeps, const int32_t *__restrict__ npos, int32_t *__restrict__ trace,
                int32_t *__restrict__ sweeps, int32_t *__restrict__ converged) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_seg) return;
    const int32_t *np = npos + (size_t)s * RF_NP;
    int32_t *tr = trace + (size_t)s * (max_sweeps + 1);
    int k = 0;
    while (k < max_sweeps && np[k] != 0) k++;                 // sweep k + 1 moved somebody iff propose k found a positive gain
    sweeps[s] = k;
    converged[s] = np[k] == 0 ? 1 : 0;
    for (int q = k + 1; q <= max_sweeps; q++) tr[q] = tr[k];
}

extern "C" pp_status pp_chi_refine(pp_ctx *c, const float *chi0, const uint8_t *fixed, const int8_t *place, const float *param,
                                   const float *ext, const float *radius, const uint8_t *acls, const uint8_t *aa_sep,
                                   const int32_t *link, const uint8_t *obst_polar, float delta, int max_steps, int bands, float band,
                                   float cut, float hb_allow, float hb_weak, float hb_weak2, float hb_good2, float reach,
                                   int max_sweeps, float *chi_out, int8_t *steps, float *xyz_out, float *hxyz_out, uint8_t *hmask_out,
                                   uint8_t *link_prev, int32_t *e, int32_t *trace, int32_t *sweeps, int32_t *converged,
                                   float *cand_xyz, float *cand_hxyz, uint8_t *cand_hmask, int32_t *cand_mask, int32_t *energy,
                                   void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !chi0 || !place || !param || !ext || !radius || !acls || !aa_sep || !chi_out || !steps || !xyz_out || !hxyz_out ||
        !hmask_out || !link_prev || !e || !trace || !sweeps || !converged)
        FAIL(PP_ERR_INVALID, "pp_chi_refine: null argument");
    if ((cand_xyz != nullptr) != (cand_hxyz != nullptr) || (cand_xyz != nullptr) != (cand_hmask != nullptr) ||
        (cand_xyz != nullptr) != (cand_mask != nullptr))
        FAIL(PP_ERR_INVALID, "pp_chi_refine: cand_xyz, cand_hxyz, cand_hmask and cand_mask go together");
    if (!std::isfinite(delta) || !(delta > 0.f) || max_steps < 1 || max_steps > PP_REFINE_MAX_STEPS ||
        !((float)max_steps * delta < RF_PI))
        FAIL(PP_ERR_INVALID, "pp_chi_refine: delta must be finite and positive, max_steps in 1 .. PP_REFINE_MAX_STEPS, max_steps delta < pi");
    if (bands < 1 || bands > PP_REFINE_MAX_BANDS || !std::isfinite(band) || !(band > 0.f))
        FAIL(PP_ERR_INVALID, "pp_chi_refine: bands must lie in 1 .. PP_REFINE_MAX_BANDS, band must be finite and positive");
    if (!std::isfinite(cut) || !std::isfinite(hb_allow) || hb_allow < 0.f)
        FAIL(PP_ERR_INVALID, "pp_chi_refine: cut must be finite, hb_allow finite and not negative");
    if (!std::isfinite(hb_weak) || !std::isfinite(hb_weak2) || !std::isfinite(hb_good2) || !(hb_weak > 0.f) || !(hb_weak2 > 0.f) ||
        !(hb_good2 > 0.f) || hb_good2 > hb_weak2)
        FAIL(PP_ERR_INVALID, "pp_chi_refine: hb_weak, hb_weak2 and hb_good2 must be finite and positive, hb_good2 <= hb_weak2");
    if (!std::isfinite(reach) || reach < hb_weak) FAIL(PP_ERR_INVALID, "pp_chi_refine: reach must be finite and at least hb_weak");
    if (max_sweeps < 0 || max_sweeps > PP_REFINE_MAX_SWEEPS)
        FAIL(PP_ERR_INVALID, "pp_chi_refine: max_sweeps must lie in 0 .. PP_REFINE_MAX_SWEEPS");
    if (!c->b.X || !c->b.BB_D || !c->b.chain_indices || !c->b.residue_type || !c->b.atom_mask || !c->b.residue_mask || !c->b.SC_D_mask)
        FAIL(PP_ERR_INVALID,
             "pp_chi_refine: needs a batch with X, BB_D, chain_indices, residue_type, atom_mask, residue_mask and SC_D_mask");
    if (obst_polar && c->obst_M <= 0) FAIL(PP_ERR_INVALID, "pp_chi_refine: obst_polar on a context without obstacle atoms");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (c->N < 1) return PP_OK;
    const size_t N = (size_t)c->N, n_atoms = N * AA_S;
    // float4: P [N][27], row [N];  float: chiC [9][N][4], xyzC [9][N][42], hxC [9][N][39];  int32: I [N][27], then [N] each of cmask,
    // mmask, prop, gain, movers, pcount, plist [N][PCAP], npos [n_seg][RF_NP], n_movers [4];  uint8: hmC [9][N][13]
    const size_t n_f4 = n_atoms + N;
    const size_t n_f = (size_t)RF_C * N * (4 + 42 + PP_H_MAX * 3);
    const size_t n_i32 = n_atoms + 6 * N + N * PP_REFINE_PCAP + (size_t)c->B * RF_NP + 4;
    const size_t total = n_f4 * sizeof(float4) + n_f * sizeof(float) + n_i32 * sizeof(int32_t) + (size_t)RF_C * N * PP_H_MAX;
    void *ws;
    if (pp_status rc = pp_ctx_workspace(c, PP_WS_REFINE, total, &ws)) return rc;
    float4 *P = static_cast<float4 *>(ws), *row = P + n_atoms;
    float *chiC = reinterpret_cast<float *>(row + N), *xyzC = chiC + (size_t)RF_C * N * 4, *hxC = xyzC + (size_t)RF_C * N * 42;
    int32_t *I = reinterpret_cast<int32_t *>(hxC + (size_t)RF_C * N * PP_H_MAX * 3);
    int32_t *cmask = I + n_atoms, *mmask = cmask + N, *prop = mmask + N, *gain = prop + N, *movers = gain + N;
    int32_t *pcount = movers + N, *plist = pcount + N, *npos = plist + N * PP_REFINE_PCAP, *n_movers = npos + (size_t)c->B * RF_NP;
    uint8_t *hmC = reinterpret_cast<uint8_t *>(n_movers + 4);
    const bool obst = c->obst_M > 0;
    const RfSets S = {xyzC, hxC, hmC, N};
    const RfPhys ph = {cut, hb_allow, hb_weak, hb_weak2, hb_good2, band, bands};
    const int tr_stride = max_sweeps + 1;
    PP_HIP_CHECK(hipMemsetAsync(npos, 0, ((size_t)c->B * RF_NP + 4) * sizeof(int32_t), st));
    PP_HIP_CHECK(hipMemsetAsync(trace, 0, (size_t)c->B * tr_stride * sizeof(int32_t), st));
    PP_HIP_CHECK(hipMemsetAsync(e, 0, N * 2 * sizeof(int32_t), st));
    PP_HIP_CHECK(hipMemsetAsync(steps, 0, N * 4, st));
    if (energy) PP_HIP_CHECK(hipMemsetAsync(energy, 0, N * RF_C * sizeof(int32_t), st));
    const dim3 rows16((unsigned)((N * 16 + 255) / 256)), rows32((unsigned)((N * 32 + 255) / 256));
    for (int k = 0; k <= max_sweeps; k++) {
        hipLaunchKernelGGL(k_rf_angles, rows16, dim3(256), 0, st, c->N, chi0, steps, c->b.residue_mask, c->b.SC_D_mask, fixed,
                           c->b.residue_type, delta, max_steps, chiC, cmask);
        PP_HIP_CHECK(hipGetLastError());
        for (int q = 0; q < RF_C; q++) {
            if (pp_status rc = pp_launch_atom14(c, chiC + (size_t)q * N * 4, xyzC + (size_t)q * N * 42, st)) return rc;
            if (pp_status rc = pp_hydrogens(c, xyzC + (size_t)q * N * 42, place, param, link, hxC + (size_t)q * N * PP_H_MAX * 3,
                                            hmC + (size_t)q * N * PP_H_MAX, link_prev, stream))
                return rc;
        }
        hipLaunchKernelGGL(k_rf_prep, rows32, dim3(256), 0, st, c->N, S, radius, acls, aa_sep, c->b.residue_type, place, cmask, P, I, row,
                           mmask, c->sat);
        PP_HIP_CHECK(hipGetLastError());
        if (k == 0) {
            hipLaunchKernelGGL(k_rf_compact, dim3(1), dim3(1024), 0, st, c->N, mmask, movers, n_movers);
            PP_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_rf_partners, dim3(c->N), dim3(RF_T), 0, st, c->N, c->B, c->seg_off, movers, n_movers, mmask, row,
                               c->b.residue_type, ext, reach, plist, pcount);
            PP_HIP_CHECK(hipGetLastError());
            if (cand_xyz) {
                PP_HIP_CHECK(hipMemcpyAsync(cand_xyz, xyzC, (size_t)RF_C * N * 42 * sizeof(float), hipMemcpyDeviceToDevice, st));
                PP_HIP_CHECK(hipMemcpyAsync(cand_hxyz, hxC, (size_t)RF_C * N * PP_H_MAX * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
                PP_HIP_CHECK(hipMemcpyAsync(cand_hmask, hmC, (size_t)RF_C * N * PP_H_MAX, hipMemcpyDeviceToDevice, st));
                PP_HIP_CHECK(hipMemcpyAsync(cand_mask, cmask, N * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
            }
        }
        hipLaunchKernelGGL(k_rf_propose, dim3(c->N), dim3(RF_T), 0, st, c->N, c->B, c->seg_off, k, movers, n_movers, P, I, row, S, radius,
                           c->b.residue_type, aa_sep, link_prev, link, obst ? c->obst : nullptr, obst ? c->obst_seg : nullptr, obst_polar,
                           ph, cmask, mmask, prop, gain, npos, e, trace, tr_stride, energy);
        PP_HIP_CHECK(hipGetLastError());
        if (k == max_sweeps) break;
        hipLaunchKernelGGL(k_rf_apply, dim3(c->N), dim3(RF_T), 0, st, c->N, c->B, c->seg_off, k, movers, n_movers, row, c->b.residue_type,
                           ext, reach, mmask, prop, gain, npos, plist, pcount, steps);
        PP_HIP_CHECK(hipGetLastError());
    }
    // candidate 0 of the last sweep is the state after the last apply
    PP_HIP_CHECK(hipMemcpyAsync(chi_out, chiC, N * 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
    PP_HIP_CHECK(hipMemcpyAsync(xyz_out, xyzC, N * 42 * sizeof(float), hipMemcpyDeviceToDevice, st));
    PP_HIP_CHECK(hipMemcpyAsync(hxyz_out, hxC, N * PP_H_MAX * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    PP_HIP_CHECK(hipMemcpyAsync(hmask_out, hmC, N * PP_H_MAX, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_rf_finish_seg, dim3((unsigned)((c->B + 63) / 64)), dim3(64), 0, st, c->B, max_sweeps, npos, trace, sweeps,
                       converged);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
