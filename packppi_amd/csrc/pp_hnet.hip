// Hydrogen-bond network optimisation: Asn / Gln / His flips and rotatable hydrogens (no reference kernel).
// One entry, pp_hnet_optimize, per segment of the context's segment table; nothing crosses segments.  Chemistry is caller data, as
// for pp_hydrogens / pp_clashscore, whose slots, class bits, separations and NERF are pp_allatom.h's here as there; the overlap test
// is written out in hn_term as k_clashscore writes it.
//
// MOVERS.  mover int32 [21][4] per residue type: (kind, states, bit mask over the 27 all-atom slots of the atoms that move, 0).
//   kind 1 ROTOR: 1 .. 12 states, at most 3 moved slots, all hydrogens with a NERF entry in `place`.  The j-th moved hydrogen in state c
//                 is pp_hydrogens' NERF (the same pp_nerf) with (c2, s2) = rot [21][12][3][2] at (type, c, j) in place of param's.
//                 State 0 holds param's own values, so it reproduces pp_hydrogens' bits.
//   kind 2 FLIP:  2 states, at most 7 moved slots.  State c takes the moved slots from (xyz_c, hxyz_c, hmask_c): the caller's two
//                 coordinate sets, the second at chi + pi.  Without a second set no flip row is a mover.
// An entry outside these ranges, or a residue_type outside 0 .. 20, is found on the device: the row is no mover and bit 3 of the
// context's sticky word is set; it is never used as an index.  Atom (n, a) is COUNTED in state c iff radius[n][a] > 0 and, for a >= 14,
// hmask_c[n][a - 14] != 0 (a rotor's hmask is hmask0 in every state).  A row is a MOVER iff its type has one and at least one moved
// slot is counted in state 0.  ext float [21]: no moved atom of the type is ever farther from CA than this.
//
// ENERGY (int32).  A pair term exists for a moved atom x of mover r at its state against any other counted atom y of the segment that
// is not a moved atom of r, and against every obstacle atom (r_o > 0) of the segment's range.  fp32, contract off:
//   excluded  step 5 of the pair rules of pp_allatom.h (never for an obstacle)
//   overlap   their steps 1 - 4 (6 for an obstacle), and not excluded
//   bond      not excluded, x and y in different rows, one a polar hydrogen h (class bit 0) with its parent D (place[..][1]; of a
//             moved hydrogen: the parent at the same state), the other an acceptor A (class bit 1; an obstacle: obst_polar != 0):
//             v = A - h, w = D - h, d2 = ((vx vx) + (vy vy)) + (vz vz), s = ((vx wx) + (vy wy)) + (vz wz), ww the same sum of w and w;
//             weak iff d2 <= hb_weak2 and s <= 0;  good iff weak and d2 <= hb_good2 and (s s) >= 0.25f (ww d2);  2 good, 1 weak, else 0
//   term      64 [overlap] - bond.  A NaN makes every comparison false: 0.
// hb [N][2] counts the terms with a bond (weak or good) of a row's moved atoms at the start and at the end, a bond between two movers
// in the higher row only: the sum over a segment is the number of explicit-hydrogen bonds its movers make, each once.
// E_r(c | s) = the sum of the terms of r at state c, everything else at its state in s;  F(s) = every term once.
//
// SWEEP (DESIGN.md section 18's scheme).  s = 0.  Propose: every mover takes the state of smallest E, the lowest on ties, its own on
// a tie with it; gain = E(own) - E(proposed).  Apply: r moves iff gain_r > 0 and every partner with a positive gain has a smaller
// gain, or an equal one and a higher row.  Partners P(r): movers r' != r of the segment with
//     d2(CA_r, CA_r') <= b b,  b = (ext[type_r] + ext[type_r']) + reach,  d = CA_r' - CA_r, d2 = ((dx dx) + (dy dy)) + (dz dz)
// (CA = slot 1 of xyz0).  Two movers with a pair term in any states are partners, two accepted movers never are, so F drops by the
// sum of the accepted gains, in integers.  A segment without a positive gain is converged: its later launches return at once.
//
// LAUNCH.  k_hn_prep (32 lanes per row): the current atoms P [N][27] (position, radius of a counted atom or 0) and I [N][27] (class |
// sep to slots 0, 2, 5 << 4, 8, 12 | parent slot << 16 | moved atom of a mover << 20) at state 0, the rotor candidates, and the row
// sphere: slot 1 and the largest (distance + radius) of a counted atom over ALL states.  k_hn_compact (one workgroup): the movers in
// ascending row order.  k_hn_partners (one wave per mover): the partner rows, ascending, the first PP_HNET_PCAP of them; a longer
// list is scanned again in k_hn_apply with the same predicate in the same order.  k_hn_propose (one wave per mover, k_clashscore's
// shape): rows of the segment kept unless
//     d2(CA_i, CA_j) > ((R_i + R_j + max(-cut, hb_weak)) 1.001 + 0.01)^2
// (two atoms with a term lie within max(rx + ry - cut, hb_weak) <= rx + ry + max(-cut, hb_weak); the slack is pp_clashscore's; the
// spheres hold every state, so the test changes no output word), taken two rows at a time, 32 lanes per row, from P / I; the own side,
// at most 7 moved atoms x states, sits in LDS and is read as broadcasts; every state, the current one included, runs the same
// instructions; the per-state sums are compile-time indexed registers, reduced across the wave once.  F of the sweep: every mover
// adds E(own) minus the terms against moved atoms of movers in lower rows to trace[segment][sweep] (integer atomics; the count of
// positive gains per segment and sweep is the only other one).  k_hn_apply (one wave per mover) rewrites the accepted movers' atoms
// in P.  k_hn_finish writes the selection.  Launches: prep, compact, partners, propose x (max_sweeps + 1), apply x max_sweeps, finish;
// no read-back, no persistent kernel, no spin-wait, no float atomics.
#include "pp_internal.h"
#include "pp_allatom.h"

#define HN_T 64
#define HN_NP (PP_HNET_MAX_SWEEPS + 1)
#define HN_CAND (PP_HNET_STATES * PP_HNET_ROT_H)

// slot of the j-th set bit of mask (j below its bit count)
__device__ __forceinline__ int hn_nth_bit(unsigned mask, int j) {
    for (int q = 0; q < j; q++) mask &= mask - 1u;
    return __ffs((int)mask) - 1;
}

struct HnSets {                        // the caller's two coordinate sets; set 1 is null on a call without flips
    const float *xyz[2], *hxyz[2];
    const uint8_t *hmask[2];
};

// position and radius-or-0 of moved slot `slot` of flip row n in state c
__device__ __forceinline__ float4 hn_flip_atom(const HnSets &S, const float *radius, int n, int slot, int c) {
    return pp_aa_atom(S.xyz[c], S.hxyz[c], S.hmask[c], radius, n, slot);
}

__global__ void __launch_bounds__(256)
k_hn_prep(int N, HnSets S, const float *__restrict__ radius, const uint8_t *__restrict__ acls, const uint8_t *__restrict__ aa_sep,
          const int64_t *__restrict__ rtype, const int8_t *__restrict__ place, const float *__restrict__ param,
          const int32_t *__restrict__ mover, const float *__restrict__ rot, float4 *__restrict__ P, int32_t *__restrict__ I,
          float4 *__restrict__ row, float4 *__restrict__ candb, float *__restrict__ cand_out, int32_t *__restrict__ meta,
          int32_t *__restrict__ mmask, int32_t *__restrict__ st, unsigned *__restrict__ sat) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n = t >> 5, a = t & 31;
    const bool rowok = n < N;
    const long long ty = rowok ? rtype[n] : 0;
    const bool tyok = ty >= 0 && ty <= 20;
    int kind = 0, ns = 0;
    unsigned mask = 0u;
    if (rowok && tyok) {                                       // the same in the 32 lanes of a row
        const int32_t *mt = mover + (size_t)ty * 4;
        kind = mt[0]; ns = mt[1]; mask = (unsigned)mt[2];
        if (kind != 0) {
            bool bad = kind < 0 || kind > 2 || (mask >> AA_S) != 0u || mask == 0u;
            if (kind == 1) bad = bad || ns < 1 || ns > PP_HNET_STATES || (mask & 0x3fffu) != 0u || __popc(mask) > PP_HNET_ROT_H;
            if (kind == 2) bad = bad || ns != 2 || __popc(mask) > PP_HNET_MOVED;
            if (!bad && kind == 1) {
                for (unsigned hm = mask >> 14; hm != 0u; hm &= hm - 1u) {
                    const int8_t *pl = place + ((size_t)ty * PP_H_MAX + (__ffs((int)hm) - 1)) * 5;
                    bad = bad || pl[0] < 0 || pl[0] > 31 || (pl[0] & 15) != 3 || pl[1] < 0 || pl[1] > 13 || pl[2] < 0 || pl[2] > 13 ||
                          pl[3] < 0 || pl[3] > 13;
                }
            }
            if (bad) {
                if (a == 0) atomicOr(sat, AA_SAT);
                kind = 0;
            }
        }
        if (kind == 2 && !S.xyz[1]) kind = 0;
        if (kind == 0) { ns = 0; mask = 0u; }
    }
    const float *ca = S.xyz[0] + (size_t)(rowok ? n : 0) * 42 + 3;
    float m = -1.f;
    float4 at = make_float4(0.f, 0.f, 0.f, 0.f);                // the lane's atom at state 0
    bool any = false;
    int word = 0;
    const bool live = rowok && a < AA_S;
    const bool mine = live && ((mask >> a) & 1u) != 0u;        // a moved slot of the row's type
    if (live) {
        at = hn_flip_atom(S, radius, n, a, 0);
        word = pp_aa_word(at, acls, aa_sep, ty, n, a, sat);
        if (tyok && a >= 14) {
            const int par = place[((size_t)ty * PP_H_MAX + (a - 14)) * 5 + 1];
            word |= ((par < 0 || par > 13) ? 0 : par) << 16;    // such a hydrogen was dropped by pp_hydrogens: it is not counted
        }
        if (at.w > 0.f) {
            any = true;
            m = pp_aa_extent(at, ca);
        }
    }
    // a mover iff a moved slot is counted in state 0
    int mv = (mine && at.w > 0.f) ? 1 : 0;
    for (int w = 16; w > 0; w >>= 1) mv |= __shfl_xor(mv, w, 32);
    const bool is_mover = mv != 0;
    if (is_mover && kind == 2 && mine) {                        // the other state of a flip
        const float4 q = hn_flip_atom(S, radius, n, a, 1);
        if (q.w > 0.f) {
            any = true;
            m = pp_nanmax(m, pp_aa_extent(q, ca));
        }
    }
    if (is_mover && kind == 1) {                                // every state of a rotor: candidate (c, j) at c * 3 + j
        const int nh = __popc(mask);
        for (int q = a; q < HN_CAND; q += 32) {
            const int c = q / PP_HNET_ROT_H, j = q - c * PP_HNET_ROT_H;
            if (c >= ns || j >= nh) continue;
            const int k = hn_nth_bit(mask >> 14, j);
            if (S.hmask[0][(size_t)n * PP_H_MAX + k] == 0) continue;
            const int8_t *pl = place + ((size_t)ty * PP_H_MAX + k) * 5;
            const float *pa = param + ((size_t)ty * PP_H_MAX + k) * 5;
            const float *cs = rot + (((size_t)ty * PP_HNET_STATES + c) * PP_HNET_ROT_H + j) * 2;
            const float *pr = S.xyz[0] + (size_t)n * 42;
            const int p = pl[1], n1 = pl[2], n2 = pl[3];
            const pp_v3 Pp = {pr[3 * p], pr[3 * p + 1], pr[3 * p + 2]};
            const pp_v3 d = pp_nerf(Pp, pr + 3 * n1, pr + 3 * n2, pa[0], pa[1], pa[2], cs[0], cs[1]);
            const float hx = Pp.x + d.x, hy = Pp.y + d.y, hz = Pp.z + d.z;
            candb[(size_t)n * HN_CAND + q] = make_float4(hx, hy, hz, 0.f);
            if (cand_out) {
                float *o = cand_out + ((size_t)n * HN_CAND + q) * 3;
                o[0] = hx; o[1] = hy; o[2] = hz;
            }
            const float rr = radius[(size_t)n * AA_S + 14 + k];
            if (rr > 0.f) m = pp_nanmax(m, pp_aa_extent(make_float4(hx, hy, hz, rr), ca));
        }
    }
    if (live) {
        P[(size_t)n * AA_S + a] = at;
        I[(size_t)n * AA_S + a] = word | ((is_mover && mine) ? (1 << 20) : 0);
    }
    pp_aa_row_sphere(m, any);
    if (rowok && a == 0) {
        row[n] = make_float4(ca[0], ca[1], ca[2], any ? m : -1.f);
        meta[n] = is_mover ? (kind | (ns << 4)) : 0;
        mmask[n] = is_mover ? (int32_t)mask : 0;
        st[n] = is_mover ? 0 : -1;
    }
}

// the movers in ascending row order
__global__ void __launch_bounds__(1024)
k_hn_compact(int N, const int32_t *__restrict__ mmask, int32_t *__restrict__ movers, int32_t *__restrict__ n_movers) {
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

// P(r): see the header of this file.  Both rows are movers, so their types are in range.
__device__ __forceinline__ bool hn_partner(const float4 ci, const float4 cj, float ei, float ej, float reach) {
#pragma clang fp contract(off)
    const float b = (ei + ej) + reach;
    const float dx = cj.x - ci.x, dy = cj.y - ci.y, dz = cj.z - ci.z;
    return pp_dot3(dx, dy, dz, dx, dy, dz) <= b * b;
}

__global__ void __launch_bounds__(HN_T)
k_hn_partners(int N, int n_seg, const int32_t *__restrict__ seg_off, const int32_t *__restrict__ movers,
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
    for (int base = lo; base < hi; base += HN_T) {
        const int j = base + lane;
        bool f = false;
        if (j < hi && j != i && mmask[j] != 0) f = hn_partner(ci, rowinfo[j], ei, ext[rtype[j]], reach);
        const unsigned long long b = __ballot(f);
        if (f) {
            const int pos = cnt + __popcll(b & ((1ull << lane) - 1ull));
            if (pos < PP_HNET_PCAP) plist[(size_t)i * PP_HNET_PCAP + pos] = j;
        }
        cnt += __popcll(b);
    }
    if (lane == 0) pcount[i] = cnt;
}

struct HnPhys {
    float cut, hb_allow, hb_weak, hb_weak2, hb_good2;
};

// the term of moved atom (p, class word xi, parent at dp) against atom (q, yi, parent at dq) whose exclusion is settled: ok = a pair
// that is not excluded; far = the atoms are in different rows (or y is an obstacle)
__device__ __forceinline__ int hn_term(const float4 p, int xi, const float4 dp, const float4 q, int yi, const float4 dq, bool ok,
                                       bool far, const HnPhys &ph) {
#pragma clang fp contract(off)
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    const float d2 = pp_dot3(dx, dy, dz, dx, dy, dz);
    float t = (p.w + q.w) - ph.cut;                           // steps 2 - 4 as k_clashscore (pp_hydrogens.hip) writes them
    const bool xh = (xi & 1) && (yi & 2), yh = (xi & 2) && (yi & 1);
    if (xh || yh) t = t - ph.hb_allow;
    int v = (ok && t > 0.f && d2 <= t * t) ? 64 : 0;
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

__global__ void __launch_bounds__(HN_T)
k_hn_propose(int N, int n_seg, const int32_t *__restrict__ seg_off, int sweep, const int32_t *__restrict__ movers,
             const int32_t *__restrict__ n_movers, const float4 *__restrict__ P, const int32_t *__restrict__ I,
             const float4 *__restrict__ rowinfo, const float4 *__restrict__ candb, HnSets S, const float *__restrict__ radius,
             const int64_t *__restrict__ chain, const int64_t *__restrict__ rtype, const uint8_t *__restrict__ aa_sep,
             const uint8_t *__restrict__ link_prev, const int32_t *__restrict__ link, const float4 *__restrict__ oatoms,
             const int2 *__restrict__ oseg, const uint8_t *__restrict__ opolar, HnPhys ph, const int32_t *__restrict__ meta,
             const int32_t *__restrict__ mmask, const int32_t *__restrict__ st, int32_t *__restrict__ prop, int32_t *__restrict__ gain,
             int32_t *__restrict__ npos, int32_t *__restrict__ e_out, int32_t *__restrict__ hb_out, int32_t *__restrict__ trace,
             int tr_stride, int32_t *__restrict__ energy) {
#pragma clang fp contract(off)
    __shared__ float4 l_own[PP_HNET_STATES * PP_HNET_MOVED];   // [state][moved atom]: position, radius of a counted atom or 0
    __shared__ float4 l_par[PP_HNET_STATES * PP_HNET_MOVED];   // its parent at that state (hydrogens)
    __shared__ int l_slot[8], l_xi[8];
    __shared__ uint8_t l_sep[AA_S * AA_S + 7];
    __shared__ int l_rows[HN_T];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n_movers[0]) return;
    const int i = movers[blockIdx.x];
    const int s = pp_seg_of_row(seg_off, n_seg, i);
    if (sweep > 0 && npos[(size_t)s * HN_NP + sweep - 1] == 0) return;      // the segment converged in an earlier sweep
    int lo, hi;
    pp_seg_rows(seg_off, s, N, lo, hi);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int mt = meta[i], kind = mt & 15, ns = (mt >> 4) & 15, cur = st[i];
    const unsigned mask = (unsigned)mmask[i];
    const int nx = __popc(mask);
    {
        const long long ty = rtype[i];                         // a mover: in range
        for (int q = lane; q < AA_S * AA_S; q += HN_T) l_sep[q] = aa_sep[(size_t)ty * AA_S * AA_S + q];
    }
    if (lane < nx) {
        const int slot = hn_nth_bit(mask, lane);
        l_slot[lane] = slot;
        l_xi[lane] = I[(size_t)i * AA_S + slot];
    }
    __syncthreads();
    if (lane < ns * nx) {
        const int c = lane / nx, xk = lane - c * nx, slot = l_slot[xk];
        float4 p, d = make_float4(0.f, 0.f, 0.f, 0.f);
        const int par = (l_xi[xk] >> 16) & 15;
        if (kind == 1) {
            p = candb[(size_t)i * HN_CAND + c * PP_HNET_ROT_H + xk];
            const float r = radius[(size_t)i * AA_S + slot];
            const bool have = S.hmask[0][(size_t)i * PP_H_MAX + (slot - 14)] != 0;
            p.w = (r > 0.f && have) ? r : 0.f;
            if (!have) p = make_float4(0.f, 0.f, 0.f, 0.f);
            d = P[(size_t)i * AA_S + par];
        } else {
            p = hn_flip_atom(S, radius, i, slot, c);
            if (slot >= 14) d = ((mask >> par) & 1u) ? hn_flip_atom(S, radius, i, par, c) : P[(size_t)i * AA_S + par];
        }
        l_own[c * PP_HNET_MOVED + xk] = p;
        l_par[c * PP_HNET_MOVED + xk] = d;
    }
    const float4 ri = rowinfo[i];
    __syncthreads();

    int e[PP_HNET_STATES];
#pragma unroll
    for (int c = 0; c < PP_HNET_STATES; c++) e[c] = 0;
    int dup = 0;                                               // terms of the current state against moved atoms of movers in lower rows
    int nb = 0;                                                // bonds of the current state, those against such atoms left out
    const long long ci = chain[i];
    const int lpi = link_prev[i];
    const int lki = link ? link[i] : -1;
    const float g = fmaxf(-ph.cut, ph.hb_weak);
    for (int base = lo; base < hi; base += HN_T) {
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
            for (int c = 0; c < PP_HNET_STATES; c++) {
                if (c < ns) {                                 // the same in every lane
                    int acc = 0;
#pragma nounroll
                    for (int xk = 0; xk < nx; xk++) {
                        const float4 p = l_own[c * PP_HNET_MOVED + xk];
                        if (!(p.w > 0.f)) continue;           // the same in every lane
                        const int xi = l_xi[xk], x = l_slot[xk];
                        const int sep = pp_aa_sep(own, rel_next, rel_prev, rel_ss, xi, y0, y2, y5, &l_sep[x * AA_S + (valid ? a : 0)]);
                        const bool ok = yok && sep > pp_aa_excl((xi & 4) || yhyd);
                        const int v = hn_term(p, xi, l_par[c * PP_HNET_MOVED + xk], q, yi, dq, ok, !own, ph);
                        acc += v;
                        if (c == cur && !lower && (v > 32 ? 64 - v : -v) > 0) nb++;       // v is 64 [overlap] - bond
                    }
                    e[c] += acc;
                    if (c == cur && lower) dup += acc;
                }
            }
        }
        __syncthreads();                                      // the list is rewritten by the next 64 rows
    }
    if (oatoms) {
        const int2 rg = oseg[s];
        const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int base = 0; base < rg.y; base += HN_T) {
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
            for (int c = 0; c < PP_HNET_STATES; c++) {
                if (c < ns) {
                    int acc = 0;
#pragma nounroll
                    for (int xk = 0; xk < nx; xk++) {
                        const float4 p = l_own[c * PP_HNET_MOVED + xk];
                        if (!(p.w > 0.f)) continue;
                        const int v = hn_term(p, l_xi[xk] & 1, l_par[c * PP_HNET_MOVED + xk], o, oi, none, ook, true, ph);
                        acc += v;
                        if (c == cur && (v > 32 ? 64 - v : -v) > 0) nb++;
                    }
                    e[c] += acc;
                }
            }
        }
    }
    // the wave's sums, the same in every lane afterwards
#pragma unroll
    for (int c = 0; c < PP_HNET_STATES; c++)
        for (int w = 32; w > 0; w >>= 1) e[c] += __shfl_xor(e[c], w);
    for (int w = 32; w > 0; w >>= 1) dup += __shfl_xor(dup, w);
    for (int w = 32; w > 0; w >>= 1) nb += __shfl_xor(nb, w);
    int e_cur = 0;
#pragma unroll
    for (int c = 0; c < PP_HNET_STATES; c++) e_cur = (c == cur) ? e[c] : e_cur;
    int best = cur, e_best = e_cur;
#pragma unroll
    for (int c = 0; c < PP_HNET_STATES; c++)
        if (c < ns && e[c] < e_best) { best = c; e_best = e[c]; }
    if (energy && sweep == 0) {
        int mine = 0;
#pragma unroll
        for (int c = 0; c < PP_HNET_STATES; c++) mine = (c == lane && c < ns) ? e[c] : mine;
        if (lane < PP_HNET_STATES) energy[(size_t)i * PP_HNET_STATES + lane] = mine;
    }
    if (lane == 0) {
        prop[i] = best;
        gain[i] = e_cur - e_best;
        if (sweep == 0) e_out[(size_t)i * 2] = e_cur;
        e_out[(size_t)i * 2 + 1] = e_cur;
        if (hb_out) {
            if (sweep == 0) hb_out[(size_t)i * 2] = nb;
            hb_out[(size_t)i * 2 + 1] = nb;
        }
        if (e_cur - dup != 0) atomicAdd(&trace[(size_t)s * tr_stride + sweep], e_cur - dup);
        if (e_cur - e_best > 0) atomicAdd(&npos[(size_t)s * HN_NP + sweep], 1);
    }
}

__global__ void __launch_bounds__(HN_T)
k_hn_apply(int N, int n_seg, const int32_t *__restrict__ seg_off, int sweep, const int32_t *__restrict__ movers,
           const int32_t *__restrict__ n_movers, HnSets S, const float *__restrict__ radius, const float4 *__restrict__ candb,
           const float4 *__restrict__ rowinfo, const int64_t *__restrict__ rtype, const float *__restrict__ ext, float reach,
           const int32_t *__restrict__ meta, const int32_t *__restrict__ mmask, const int32_t *__restrict__ prop,
           const int32_t *__restrict__ gain, const int32_t *__restrict__ npos, const int32_t *__restrict__ plist,
           const int32_t *__restrict__ pcount, int32_t *__restrict__ st, float4 *__restrict__ P) {
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n_movers[0]) return;
    const int i = movers[blockIdx.x];
    const int s = pp_seg_of_row(seg_off, n_seg, i);
    if (npos[(size_t)s * HN_NP + sweep] == 0) return;         // converged: nobody in the segment wants to move
    const int gi = gain[i];
    if (gi <= 0) return;
    const int cnt = pcount[i];
    bool blocked = false;
    if (cnt <= PP_HNET_PCAP) {
        if (lane < cnt) {
            const int j = plist[(size_t)i * PP_HNET_PCAP + lane];
            const int gj = gain[j];
            blocked = gj > 0 && !(gj < gi || (gj == gi && j > i));
        }
    } else {                                                  // the list did not hold them all: the same predicate over the segment
        int lo, hi;
        pp_seg_rows(seg_off, s, N, lo, hi);
        const float4 ci = rowinfo[i];
        const float ei = ext[rtype[i]];
        for (int base = lo; base < hi; base += HN_T) {
            const int j = base + lane;
            if (j < hi && j != i && mmask[j] != 0 && hn_partner(ci, rowinfo[j], ei, ext[rtype[j]], reach)) {
                const int gj = gain[j];
                blocked = blocked || (gj > 0 && !(gj < gi || (gj == gi && j > i)));
            }
        }
    }
    if (__ballot(blocked) != 0ull) return;
    const unsigned mask = (unsigned)mmask[i];
    const int kind = meta[i] & 15, c = prop[i];
    if (lane < AA_S && ((mask >> lane) & 1u)) {
        float4 p;
        if (kind == 1) {
            const int j = __popc(mask & ((1u << lane) - 1u));
            const float r = radius[(size_t)i * AA_S + lane];
            const bool have = S.hmask[0][(size_t)i * PP_H_MAX + (lane - 14)] != 0;
            p = have ? candb[(size_t)i * HN_CAND + c * PP_HNET_ROT_H + j] : make_float4(0.f, 0.f, 0.f, 0.f);
            p.w = (r > 0.f && have) ? r : 0.f;
        } else {
            p = hn_flip_atom(S, radius, i, lane, c);
        }
        P[(size_t)i * AA_S + lane] = p;
    }
    if (lane == 0) st[i] = c;
}

// the selection: 32 lanes per row
__global__ void __launch_bounds__(256)
k_hn_finish(int N, HnSets S, const float *__restrict__ chi0, const float *__restrict__ chi1, const float4 *__restrict__ candb,
            const int32_t *__restrict__ meta, const int32_t *__restrict__ mmask, const int32_t *__restrict__ st,
            int32_t *__restrict__ state, float *__restrict__ xyz_out, float *__restrict__ hxyz_out, uint8_t *__restrict__ hmask_out,
            float *__restrict__ chi_out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n = t >> 5, a = t & 31;
    if (n >= N) return;
    const int c = st[n], kind = meta[n] & 15;
    const unsigned mask = (unsigned)mmask[n];
    const int set = (kind == 2 && c == 1) ? 1 : 0;
    if (a == 0) state[n] = c;
    if (a < 14) {
        for (int k = 0; k < 3; k++) xyz_out[(size_t)n * 42 + 3 * a + k] = S.xyz[set][(size_t)n * 42 + 3 * a + k];
    }
    if (a < PP_H_MAX) {
        const size_t o = (size_t)n * PP_H_MAX + a;
        const uint8_t have = S.hmask[set][o];
        float hx = S.hxyz[set][o * 3], hy = S.hxyz[set][o * 3 + 1], hz = S.hxyz[set][o * 3 + 2];
        if (kind == 1 && ((mask >> (14 + a)) & 1u) && have != 0) {
            const float4 p = candb[(size_t)n * HN_CAND + c * PP_HNET_ROT_H + __popc((mask >> 14) & ((1u << a) - 1u))];
            hx = p.x; hy = p.y; hz = p.z;
        }
        hmask_out[o] = have;
        hxyz_out[o * 3] = hx; hxyz_out[o * 3 + 1] = hy; hxyz_out[o * 3 + 2] = hz;
    }
    if (chi_out && a >= 16 && a < 20) chi_out[(size_t)n * 4 + (a - 16)] = (set ? chi1 : chi0)[(size_t)n * 4 + (a - 16)];
}

// per segment: sweeps taken, converged, and F carried behind the sweep that converged
__global__ void __launch_bounds__(64)
k_hn_finish_seg(int n_seg, int max_sweeps, const int32_t *__restrict__ npos, int32_t *__restrict__ trace,
                int32_t *__restrict__ sweeps, int32_t *__restrict__ converged) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_seg) return;
    const int32_t *np = npos + (size_t)s * HN_NP;
    int32_t *tr = trace + (size_t)s * (max_sweeps + 1);
    int k = 0;
    while (k < max_sweeps && np[k] != 0) k++;                 // sweep k + 1 moved somebody iff propose k found a positive gain
    sweeps[s] = k;
    converged[s] = np[k] == 0 ? 1 : 0;
    for (int q = k + 1; q <= max_sweeps; q++) tr[q] = tr[k];
}

extern "C" pp_status pp_hnet_optimize(pp_ctx *c, const float *xyz0, const float *hxyz0, const uint8_t *hmask0, const float *xyz1,
                                      const float *hxyz1, const uint8_t *hmask1, const float *chi0, const float *chi1,
                                      const int8_t *place, const float *param, const int32_t *mover, const float *rot,
                                      const float *ext, const float *radius, const uint8_t *acls, const uint8_t *aa_sep,
                                      const uint8_t *link_prev, const int32_t *link, const uint8_t *obst_polar, float cut,
                                      float hb_allow, float hb_weak, float hb_weak2, float hb_good2, float reach, int max_sweeps,
                                      int32_t *state, float *xyz_out, float *hxyz_out, uint8_t *hmask_out, float *chi_out, int32_t *e,
                                      int32_t *hb, int32_t *trace, int32_t *sweeps, int32_t *converged, float *cand, int32_t *energy, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !xyz0 || !hxyz0 || !hmask0 || !place || !param || !mover || !rot || !ext || !radius || !acls || !aa_sep || !link_prev ||
        !state || !xyz_out || !hxyz_out || !hmask_out || !e || !trace || !sweeps || !converged)
        FAIL(PP_ERR_INVALID, "pp_hnet_optimize: null argument");
    if ((xyz1 != nullptr) != (hxyz1 != nullptr) || (xyz1 != nullptr) != (hmask1 != nullptr))
        FAIL(PP_ERR_INVALID, "pp_hnet_optimize: xyz1, hxyz1 and hmask1 go together");
    if ((chi0 != nullptr) != (chi1 != nullptr) || (chi0 != nullptr) != (chi_out != nullptr))
        FAIL(PP_ERR_INVALID, "pp_hnet_optimize: chi0, chi1 and chi_out go together");
    if (chi0 && !xyz1) FAIL(PP_ERR_INVALID, "pp_hnet_optimize: chi1 without the second coordinate set");
    if (!std::isfinite(cut) || !std::isfinite(hb_allow) || hb_allow < 0.f)
        FAIL(PP_ERR_INVALID, "pp_hnet_optimize: cut must be finite, hb_allow finite and not negative");
    if (!std::isfinite(hb_weak) || !std::isfinite(hb_weak2) || !std::isfinite(hb_good2) || !(hb_weak > 0.f) || !(hb_weak2 > 0.f) ||
        !(hb_good2 > 0.f) || hb_good2 > hb_weak2)
        FAIL(PP_ERR_INVALID, "pp_hnet_optimize: hb_weak, hb_weak2 and hb_good2 must be finite and positive, hb_good2 <= hb_weak2");
    if (!std::isfinite(reach) || reach < hb_weak) FAIL(PP_ERR_INVALID, "pp_hnet_optimize: reach must be finite and at least hb_weak");
    if (max_sweeps < 0 || max_sweeps > PP_HNET_MAX_SWEEPS)
        FAIL(PP_ERR_INVALID, "pp_hnet_optimize: max_sweeps must lie in 0 .. PP_HNET_MAX_SWEEPS");
    if (!c->b.chain_indices || !c->b.residue_type)
        FAIL(PP_ERR_INVALID, "pp_hnet_optimize: needs a batch with chain_indices and residue_type");
    if (obst_polar && c->obst_M <= 0) FAIL(PP_ERR_INVALID, "pp_hnet_optimize: obst_polar on a context without obstacle atoms");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (c->N < 1) return PP_OK;
    const size_t N = (size_t)c->N, n_atoms = N * AA_S;
    // float4: P [N][27], row [N], candb [N][36];  int32: I [N][27], then [N] each of meta, mmask, st, prop, gain, movers, pcount,
    // plist [N][PCAP], npos [n_seg][HN_NP], n_movers [4]
    const size_t n_f4 = n_atoms + N + N * HN_CAND;
    const size_t n_i32 = n_atoms + 7 * N + N * PP_HNET_PCAP + (size_t)c->B * HN_NP + 4;
    const size_t total = n_f4 * sizeof(float4) + n_i32 * sizeof(int32_t);
    void *ws;
    if (pp_status rc = pp_ctx_workspace(c, PP_WS_HNET, total, &ws)) return rc;
    float4 *P = static_cast<float4 *>(ws), *row = P + n_atoms, *candb = row + N;
    int32_t *I = reinterpret_cast<int32_t *>(candb + N * HN_CAND);
    int32_t *meta = I + n_atoms, *mmask = meta + N, *cur = mmask + N, *prop = cur + N, *gain = prop + N, *movers = gain + N;
    int32_t *pcount = movers + N, *plist = pcount + N, *npos = plist + N * PP_HNET_PCAP, *n_movers = npos + (size_t)c->B * HN_NP;
    const bool obst = c->obst_M > 0;
    const HnSets S = {{xyz0, xyz1}, {hxyz0, hxyz1}, {hmask0, hmask1}};
    const HnPhys ph = {cut, hb_allow, hb_weak, hb_weak2, hb_good2};
    const int tr_stride = max_sweeps + 1;
    PP_HIP_CHECK(hipMemsetAsync(npos, 0, ((size_t)c->B * HN_NP + 4) * sizeof(int32_t), st));
    PP_HIP_CHECK(hipMemsetAsync(trace, 0, (size_t)c->B * tr_stride * sizeof(int32_t), st));
    PP_HIP_CHECK(hipMemsetAsync(e, 0, N * 2 * sizeof(int32_t), st));
    if (hb) PP_HIP_CHECK(hipMemsetAsync(hb, 0, N * 2 * sizeof(int32_t), st));
    if (cand) PP_HIP_CHECK(hipMemsetAsync(cand, 0, N * HN_CAND * 3 * sizeof(float), st));
    if (energy) PP_HIP_CHECK(hipMemsetAsync(energy, 0, N * PP_HNET_STATES * sizeof(int32_t), st));
    const dim3 rows32((unsigned)((N * 32 + 255) / 256));
    hipLaunchKernelGGL(k_hn_prep, rows32, dim3(256), 0, st, c->N, S, radius, acls, aa_sep, c->b.residue_type, place, param, mover, rot,
                       P, I, row, candb, cand, meta, mmask, cur, c->sat);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_hn_compact, dim3(1), dim3(1024), 0, st, c->N, mmask, movers, n_movers);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_hn_partners, dim3(c->N), dim3(HN_T), 0, st, c->N, c->B, c->seg_off, movers, n_movers, mmask, row,
                       c->b.residue_type, ext, reach, plist, pcount);
    PP_HIP_CHECK(hipGetLastError());
    for (int k = 0; k <= max_sweeps; k++) {
        hipLaunchKernelGGL(k_hn_propose, dim3(c->N), dim3(HN_T), 0, st, c->N, c->B, c->seg_off, k, movers, n_movers, P, I, row, candb, S,
                           radius, c->b.chain_indices, c->b.residue_type, aa_sep, link_prev, link, obst ? c->obst : nullptr,
                           obst ? c->obst_seg : nullptr, obst_polar, ph, meta, mmask, cur, prop, gain, npos, e, hb, trace, tr_stride, energy);
        PP_HIP_CHECK(hipGetLastError());
        if (k == max_sweeps) break;
        hipLaunchKernelGGL(k_hn_apply, dim3(c->N), dim3(HN_T), 0, st, c->N, c->B, c->seg_off, k, movers, n_movers, S, radius, candb, row,
                           c->b.residue_type, ext, reach, meta, mmask, prop, gain, npos, plist, pcount, cur, P);
        PP_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_hn_finish, rows32, dim3(256), 0, st, c->N, S, chi0, chi1, candb, meta, mmask, cur, state, xyz_out, hxyz_out,
                       hmask_out, chi_out);
    PP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_hn_finish_seg, dim3((unsigned)((c->B + 63) / 64)), dim3(64), 0, st, c->B, max_sweeps, npos, trace, sweeps,
                       converged);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
