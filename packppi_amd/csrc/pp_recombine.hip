// Recombination of a decoy ensemble per residue (no reference counterpart): the D sampled states of every
// residue are that residue's rotamer candidates, and a conflict-free parallel descent on the clash objective picks one per residue.
//
// LAYOUT.  That of pp_ensemble.hip: segment g * D + d of the context is decoy d of group g, all decoys of a group have the same
// length, backbone, types and masks; consensus row (g, r) has buffer index seg_off[g * D] / D + r.  An assignment s gives every
// consensus row a decoy; the recombined structure takes row r's angles from decoy s[r].
//
// OBJECTIVE.  sum over the rows of a complex of pp_clash's per_res splits exactly into
//   U(r, d)            the within-residue term of row r at decoy d's angles,
//   W(r, d; r', d')    sum over the allowed atom pairs (a of r at d, b of r' at d') of
//                      err * ([a >= 4] / (nsc_r + 1e-10) + [b >= 4] / (nsc_r' + 1e-10)),   err = max(rad_a + rad_b - tol - dist, 0),
//   F(s) = sum_r U(r, s_r) + 1/2 sum_r sum_{r' != r} W(r, s_r; r', s_r'),     clash(s) = F(s) / L_g,
// with k_clash's masks and exclusions, in fp32.  E_r(d | s) = U(r, d) + sum_{r'} W(r, d; r', s_r'): moving row r alone from s_r
// to d changes F by E_r(d | s) - E_r(s_r | s).
//
// PARTNERS.  P(r) = the rows r' != r of the group with another residue_index and |CA_r - CA_r'| < e_r + e_r' + cl_reach(tol), e =
// cl_extent (pp_clash_geom.h): symmetric, a function of the backbone and the types only, and a superset of every pair whose W can
// be non-zero at any angles.  k_rc_setup lists them per consensus row, ascending, up to RC_LCAP; a row with more scans the rows of
// its group with the same predicate, in the same order, wherever the list would be read: same partners, same order, same bits.
//
// ONE SWEEP = two launches.
//   k_rc_propose  one 256-thread workgroup per consensus row; wave w evaluates the candidates d = w, w + 4, ...  Inside a wave
//                 k_clash's layout: lane = 16 * stripe + own atom, four partner stripes.  The partners that pass the exact
//                 bounding-sphere test at (d, s_r') are compacted in order into LDS; partner number q of that sequence goes to
//                 stripe q mod 4 whatever the LDS window holds, every lane adds its terms in ascending q, then stripes and atoms
//                 fold in butterflies: every E has one fixed summation order, the same for every d.  prop_r = the d with the
//                 smallest E (lowest d on ties, a NaN loses to any number), gain_r = E_r(s_r) - E_r(prop_r).
//   k_rc_apply    one wave per consensus row: s_r <- prop_r iff gain_r > 0 and every partner with a positive gain has a smaller
//                 one (or an equal one and a higher row).  Accepted rows are pairwise non-partners, so their gains add up.  The same
//                 launch carries one more workgroup per group, which sums this sweep's row terms into trace[g][k] (fp64, fixed
//                 order) and keeps the group's counters.
// A group without a positive gain is converged: its later launches return at once.  Everything that crosses workgroups (s, prop,
// gain, the counters) crosses a kernel boundary; the only atomics are integer counters.  No float atomics: bit-reproducible.
#include "pp_internal.h"
#include "pp_clash_geom.h"      // cl_extent, cl_reach: the bound the static partner lists rest on

#define RC_LCAP (2 * PP_CL_CAP)      // static partners listed per consensus row (more: the row scans its group instead)
#define RC_WCAP 256                  // partners one wave holds in LDS before it works them off (>= RC_LCAP, a multiple of 64)

struct RcArgs {
    int N, G, D, M, K;               // rows, groups, decoys, consensus rows (N / D), max_sweeps
    const int32_t *seg_off;
    const float *chi;
    const float4 *rec;               // k_atom14's records at chi
    const float *X, *amask, *side_extent, *lower, *upper;
    const int64_t *rtype, *rindex;
    float tol;
    // obstacle atoms of the context (pp_ctx_set_obstacles), or oatoms == nullptr: none.  They belong to the group: U(r, d) gains the
    // obstacle term of row r at decoy d's angles, so F(s) stays the sum of pp_clash's per_res at the recombined angles
    const float4 *oatoms;            // [.] (x, y, z, radius)
    const int2 *oseg;                // [B] (first, count) of every segment's range
    // workspace (rc_workspace: carved from the context's proximal buffers, the two never run at once on one context)
    int2 *info;                      // [M] (group, row within it), (-1, .) = not a row of a group that is recombined
    int32_t *s, *prop;               // [M] the assignment; this sweep's proposals
    float *gain, *rowU, *rowW;       // [M] this sweep's gains; U(r, s_r) and sum_r' W(r, s_r; r', s_r') at the sweep's start
    int4 *ginfo;                     // [G] (first consensus row, length, recombined?, 0)
    int32_t *cnt;                    // [G][2] rows with a positive gain in sweep k, at [k & 1]
    int32_t *plist, *pcnt;           // [M][RC_LCAP] static partners (rows within the group, ascending); [M] their number or -1
    // outputs
    const int32_t *start;
    int32_t *pick, *sweeps, *converged;
    float *chi_out, *energy;
    double *trace;
};

// obstacles belong to the group: its decoys must point at one range (a group that does not is left alone like a ragged one)
__device__ __forceinline__ bool rc_obst_same(const RcArgs &A, int g) {
    if (!A.oatoms) return true;
    const int2 r0 = A.oseg[g * A.D];
    bool ok = true;
    for (int d = 1; d < A.D; d++) {
        const int2 r = A.oseg[g * A.D + d];
        ok = ok && r.x == r0.x && r.y == r0.y;
    }
    return ok;
}
// what the static partner predicate reads of a row: CA, the extent e (cl_extent), residue_index
struct RcRow {
    float ca[3], e;
    int ri;
};
__device__ __forceinline__ RcRow rc_row(const RcArgs &A, int n) {
    RcRow o;
    o.e = cl_extent(A.X, A.amask, A.rtype, A.side_extent, n, o.ca);
    o.ri = (int)A.rindex[n];
    return o;
}
// symmetric in its two rows: squares of differences, a commutative sum of the extents.  Not k_clash_cand's comparison, which is
// compiled with contraction on (pp_clash_geom.h)
__device__ __forceinline__ bool rc_near(const RcRow &p, const RcRow &q, float reach) {
#pragma clang fp contract(off)
    const float dx = q.ca[0] - p.ca[0], dy = q.ca[1] - p.ca[1], dz = q.ca[2] - p.ca[2];
    const float lim = p.e + q.e + reach;
    return p.ri != q.ri && lim > 0.f && (dx * dx + dy * dy) + dz * dz < lim * lim;
}

// ---------------------------------------------------------------------------------------------
// front pass: which rows are recombined, the start assignment, the static partner lists, the groups' counters
// ---------------------------------------------------------------------------------------------
// Workgroups 0 .. ceil(M / 4) - 1: one wave per consensus row.  The G workgroups behind them: one per group.
__global__ void __launch_bounds__(256)
k_rc_setup(RcArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nrb = (A.M + 3) / 4;
    if ((int)blockIdx.x >= nrb) {
        const int g = blockIdx.x - nrb;
        int base, len, row0;
        bool ok = pp_group_rows(A.seg_off, g, A.D, A.N, base, len, row0);
        const int st = A.start ? A.start[g] : 0;
        ok = ok && st >= 0 && st < A.D && rc_obst_same(A, g);
        if (threadIdx.x == 0) {
            A.ginfo[g] = make_int4(base, len, ok ? 1 : 0, 0);
            A.cnt[2 * g] = 0;
            A.cnt[2 * g + 1] = 0;
            A.sweeps[g] = 0;
            A.converged[g] = (ok && A.D == 1) ? 1 : 0;          // one candidate per row: nothing to decide
        }
        if (!ok)
            for (int k = threadIdx.x; k <= A.K; k += 256) A.trace[(size_t)g * (A.K + 1) + k] = (double)NAN;
        return;
    }
    const int cr = blockIdx.x * 4 + wave;
    if (cr >= A.M) return;
    const int g = pp_group_of_cons_row(A.seg_off, A.G, A.D, A.N, cr);
    int base, len, row0;
    bool ok = pp_group_rows(A.seg_off, g, A.D, A.N, base, len, row0);
    const int r = cr - base;
    const int st = A.start ? A.start[g] : 0;
    ok = ok && st >= 0 && st < A.D && r >= 0 && r < len && rc_obst_same(A, g);
    if (!ok) {
        if (lane == 0) A.info[cr] = make_int2(-1, 0);
        return;
    }
    if (lane == 0) {
        A.info[cr] = make_int2(g, r);
        A.s[cr] = st;
    }
    // static partners: the backbone and the types are those of every decoy, read from decoy 0
    const RcRow me = rc_row(A, row0 + r);
    const float reach = cl_reach(A.tol);
    int32_t *out = A.plist + (size_t)cr * RC_LCAP;
    int cnt = 0;
    for (int j0 = 0; j0 < len; j0 += 64) {
        const int jl = j0 + lane;
        bool keep = false;
        if (jl < len && jl != r) keep = rc_near(me, rc_row(A, row0 + jl), reach);
        const unsigned long long bal = __ballot(keep);
        const int at = cnt + __popcll(bal & ((1ull << lane) - 1ull));
        if (keep && at < RC_LCAP) out[at] = jl;
        cnt += __popcll(bal);
    }
    if (lane == 0) A.pcnt[cr] = cnt <= RC_LCAP ? cnt : -1;
}

// ---------------------------------------------------------------------------------------------
// propose
// ---------------------------------------------------------------------------------------------
// full: every candidate d (else only d = s_r: the row terms of the trace); count: write prop / gain and count the positive gains
__global__ void __launch_bounds__(256)
k_rc_propose(RcArgs A, int k, int full, int count) {
    __shared__ int s_list[4][RC_WCAP];
    __shared__ float s_best[4][2];
    __shared__ float s_cur[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cr = blockIdx.x;
    const int2 inf = A.info[cr];
    if (inf.x < 0) return;
    const int g = inf.x, r = inf.y;
    if (k > 0 && A.converged[g]) return;
    const int4 gi = A.ginfo[g];
    const int base = gi.x, len = gi.y, D = A.D;
    const int sr = A.s[cr];
    const int a = lane & 15, slot = lane >> 4;
    const bool own = a < 14;
    const float4 *__restrict__ rec = A.rec;
    const float tol = A.tol, reach = cl_reach(tol);
    const int nst = A.pcnt[cr];
    const int32_t *pl = A.plist + (size_t)cr * RC_LCAP;
    const int row00 = pp_decoy_row0(A.seg_off, g, A.D, A.N, 0);
    RcRow me0 = {};
    if (nst < 0) me0 = rc_row(A, row00 + r);
    const int nslots = nst >= 0 ? nst : len;
    int *list = s_list[wave];

    float bestE = 0.f;
    int bestD = -1;
    const int dfirst = full ? wave : (wave == 0 ? sr : D), dstep = full ? 4 : D;
    for (int d = dfirst; d < D; d += dstep) {
        const int ig = pp_decoy_row0(A.seg_off, g, A.D, A.N, d) + r;
        const float4 me = rec[(size_t)ig * 16 + 15];
        const int S = __float_as_int(me.z);
        const int ri = __float_as_int(me.y);
        const float nsc = me.x;
        float pa[3] = {0.f, 0.f, 0.f}, ea = 0.f, ra = 0.f;
        if (own) {
            const float4 q = rec[(size_t)ig * 16 + a];
            pa[0] = q.x; pa[1] = q.y; pa[2] = q.z;
            ra = q.w;
            ea = q.w != 0.f ? 1.f : 0.f;
        }
        const float4 cme = rec[(size_t)ig * 16 + 14];
        float wa = 0.f, wb = 0.f;           // sum of err over this lane's pairs; the same weighted with the partner's 1 / nsc
        int ord = 0, cnt = 0;               // partners worked off so far; partners waiting in LDS
        for (int c0 = 0; c0 < nslots; c0 += 64) {
            const int ci = c0 + lane;
            bool keep = false;
            int jg = 0;
            if (ci < nslots) {
                const int jl = nst >= 0 ? pl[ci] : ci;
                const bool partner = nst >= 0 ? true : (jl != r && rc_near(me0, rc_row(A, row00 + jl), reach));
                if (partner) {
                    jg = pp_decoy_row0(A.seg_off, g, A.D, A.N, A.s[base + jl]) + jl;          // the partner's records at ITS current decoy
                    const float4 cj = rec[(size_t)jg * 16 + 14];
                    const float dx = cj.x - cme.x, dy = cj.y - cme.y, dz = cj.z - cme.z;
                    const float lim = cme.w + cj.w + reach;
                    keep = (lim > 0.f) && (dx * dx + dy * dy + dz * dz < lim * lim);
                }
            }
            const unsigned long long bal = __ballot(keep);
            if (keep) list[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = jg;
            cnt += __popcll(bal);
            if (cnt + 64 <= RC_WCAP && c0 + 64 < nslots) continue;
            __builtin_amdgcn_wave_barrier();
            // partner number ord + c of the sequence belongs to stripe (ord + c) mod 4
            for (int c = (slot - ord) & 3; c < cnt; c += 4) {
                const int jp = list[c];
                // (k_clash's atom-pair loop without the gradient, pp_clash.hip: change both or neither)
                float4 pbr[14];
#pragma unroll
                for (int bb = 0; bb < 14; bb++) pbr[bb] = rec[(size_t)jp * 16 + bb];
                const float4 mj = rec[(size_t)jp * 16 + 15];
                const int rj = __float_as_int(mj.y);
                const bool i_low = ri < rj;
                const bool adjacent = i_low ? (ri + 1 == rj) : (rj + 1 == ri);
                if (own && ea != 0.f && rj != ri) {
                    float eb = 0.f;
#pragma unroll
                    for (int bb = 0; bb < 14; bb++) {
                        const float4 pb = pbr[bb];
                        bool ok = pb.w != 0.f && !(a < 4 && bb < 4) && !(a == 5 && bb == 5);
                        if (adjacent) {
                            if (i_low ? (a == 2 && bb == 0) : (a == 0 && bb == 2)) ok = false;      // peptide bond C(lower) - N(higher)
                        }
                        if (ok) {
                            const float dx = pa[0] - pb.x, dy = pa[1] - pb.y, dz = pa[2] - pb.z;
                            const float d2 = 1e-10f + dx * dx + dy * dy + dz * dz;
                            const float thr = (ra + pb.w) - tol;
                            if (!(thr > 0.f && d2 < thr * thr)) continue;
                            const float err = thr - sqrtf(d2);
                            if (err > 0.f) {
                                wa += err;
                                if (bb >= 4) eb += err;
                            }
                        }
                    }
                    wb += eb / (mj.x + 1e-10f);
                }
            }
            __builtin_amdgcn_wave_barrier();
            ord += cnt;
            cnt = 0;
        }
        // the within-residue bounds (k_clash's tail, a copy: change both or neither): stripes of partner atoms b = slot, slot + 4, ...
        float ua = 0.f;
        if (own && ea != 0.f) {
            for (int bb = slot; bb < 14; bb += 4) {
                if (bb == a || (a < 4 && bb < 4)) continue;
                const float4 pb = rec[(size_t)ig * 16 + bb];
                if (pb.w == 0.f) continue;
                const float dx = pa[0] - pb.x, dy = pa[1] - pb.y, dz = pa[2] - pb.z;
                const float dd = sqrtf(1e-10f + dx * dx + dy * dy + dz * dz);
                const float lo = A.lower[(S * 14 + a) * 14 + bb], up = A.upper[(S * 14 + a) * 14 + bb];
                ua += 2.f * (fmaxf(lo - dd, 0.f) + fmaxf(dd - up, 0.f));          // row sum + column sum of a symmetric table
            }
        }
        // the obstacle term of k_clash<., ., true> (a copy of its hinge: change both or neither): obstacle l of the group's range goes to
        // stripe l mod 4, ascending l per lane; the residue's bounding sphere drops obstacles whose hinge is zero on every atom
        if (A.oatoms) {
            const int2 orng = A.oseg[g * D];
            const float oreach = cl_obst_reach(tol);
            const bool act = own && a >= 4 && ea != 0.f;
            for (int c0 = 0; c0 < orng.y; c0 += 64) {
                bool keep = false;
                if (c0 + lane < orng.y) {
                    const float4 q = A.oatoms[orng.x + c0 + lane];
                    const float dx = q.x - cme.x, dy = q.y - cme.y, dz = q.z - cme.z;
                    const float lim = cme.w + q.w + oreach;
                    keep = q.w > 0.f && lim > 0.f && (dx * dx + dy * dy + dz * dz < lim * lim);
                }
                unsigned long long bal = __ballot(keep);
                while (bal) {
                    const int l = c0 + __builtin_ctzll(bal);
                    bal &= bal - 1ull;
                    const float4 q = A.oatoms[orng.x + l];
                    if (act && (l & 3) == slot) {
                        const float dx = pa[0] - q.x, dy = pa[1] - q.y, dz = pa[2] - q.z;
                        const float d2 = 1e-10f + dx * dx + dy * dy + dz * dz;
                        const float thr = (ra + q.w) - tol;
                        if (thr > 0.f && d2 < thr * thr) {
                            const float err = thr - sqrtf(d2);
                            if (err > 0.f) ua += err;
                        }
                    }
                }
            }
        }
        // fold the 4 stripes, then the 16 atoms (fixed order)
        for (int o = 16; o <= 32; o <<= 1) {
            wa += __shfl_xor(wa, o);
            wb += __shfl_xor(wb, o);
            ua += __shfl_xor(ua, o);
        }
        float lw = (own && a >= 4) ? wa : 0.f, lb = own ? wb : 0.f, lu = (own && a >= 4) ? ua : 0.f;
        for (int o = 8; o > 0; o >>= 1) {
            lw += __shfl_xor(lw, o);
            lb += __shfl_xor(lb, o);
            lu += __shfl_xor(lu, o);
        }
        const float U = lu / (nsc + 1e-10f);
        const float W = lw / (nsc + 1e-10f) + lb;
        const float E = U + W;
        if (A.energy && k == 0 && lane == 0) A.energy[(size_t)cr * D + d] = E;
        if (d == sr && lane == 0) { s_cur[0] = U; s_cur[1] = W; s_cur[2] = E; }
        if (bestD < 0 || E < bestE || (bestE != bestE && E == E)) { bestE = E; bestD = d; }     // ascending d: the lowest wins ties
    }
    if (lane == 0) { s_best[wave][0] = bestE; s_best[wave][1] = __int_as_float(bestD); }
    __syncthreads();
    if (threadIdx.x != 0) return;
    A.rowU[cr] = s_cur[0];
    A.rowW[cr] = s_cur[1];
    if (!count) return;
    float pE = 0.f;
    int pd = -1;
    for (int w = 0; w < 4; w++) {
        const float E = s_best[w][0];
        const int d = __float_as_int(s_best[w][1]);
        if (d < 0) continue;
        const bool en = E != E, pn = pE != pE;
        if (pd < 0 || E < pE || (pn && !en) || ((E == pE || (en && pn)) && d < pd)) { pE = E; pd = d; }
    }
    const float Es = s_cur[2];
    float gain = 0.f;
    if (pd != sr) gain = (Es != Es && pE == pE) ? INFINITY : Es - pE;
    A.prop[cr] = pd;
    A.gain[cr] = gain;
    if (gain > 0.f) atomicAdd(&A.cnt[2 * g + (k & 1)], 1);
}

// ---------------------------------------------------------------------------------------------
// trace[g][k] from the row terms of sweep k's propose launch; with `update` the group's counters (apply launch of sweep k)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void rc_trace_block(const RcArgs &A, int g, int k, bool update) {
#pragma clang fp contract(off)
    __shared__ double red[2][256];
    const int tid = threadIdx.x;
    const int4 gi = A.ginfo[g];
    if (!gi.z) return;                                  // not recombined: k_rc_setup wrote its NaN trace
    double *tr = A.trace + (size_t)g * (A.K + 1);
    int32_t *cnt = A.cnt + 2 * g;
    if (k > 0 && A.converged[g]) {                      // converged before this sweep: nothing was evaluated, nothing moved
        if (tid == 0) {
            tr[k] = tr[k - 1];
            if (update) cnt[(k + 1) & 1] = 0;
        }
        return;
    }
    double su = 0.0, sw = 0.0;
    for (int r = tid; r < gi.y; r += 256) {
        su += (double)A.rowU[gi.x + r];
        sw += (double)A.rowW[gi.x + r];
    }
    red[0][tid] = su;
    red[1][tid] = sw;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            red[0][tid] += red[0][tid + w];
            red[1][tid] += red[1][tid + w];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    tr[k] = (red[0][0] + 0.5 * red[1][0]) / (double)gi.y;
    if (update) {
        if (cnt[k & 1] > 0) A.sweeps[g] += 1;           // some gain is positive: the largest of them is accepted, a row moves
        else A.converged[g] = 1;
        cnt[(k + 1) & 1] = 0;
    }
}

// ---------------------------------------------------------------------------------------------
// apply: one wave per consensus row (workgroups 0 .. ceil(M / 4) - 1), then one workgroup per group for the trace
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_rc_apply(RcArgs A, int k) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nrb = (A.M + 3) / 4;
    if ((int)blockIdx.x >= nrb) {
        rc_trace_block(A, blockIdx.x - nrb, k, true);
        return;
    }
    const int cr = blockIdx.x * 4 + wave;
    if (cr >= A.M) return;
    const int2 inf = A.info[cr];
    if (inf.x < 0) return;
    const int g = inf.x, r = inf.y;
    if (A.cnt[2 * g + (k & 1)] == 0) return;            // no positive gain in this group (or the group had converged before)
    const float gain = A.gain[cr];
    if (!(gain > 0.f)) return;
    const int4 gi = A.ginfo[g];
    const int base = gi.x, len = gi.y;
    const int nst = A.pcnt[cr];
    const int32_t *pl = A.plist + (size_t)cr * RC_LCAP;
    const int row00 = pp_decoy_row0(A.seg_off, g, A.D, A.N, 0);
    RcRow me0 = {};
    if (nst < 0) me0 = rc_row(A, row00 + r);
    const float reach = cl_reach(A.tol);
    const int nslots = nst >= 0 ? nst : len;
    bool blocked = false;
    for (int c0 = 0; c0 < nslots; c0 += 64) {
        const int ci = c0 + lane;
        if (ci >= nslots) continue;
        const int jl = nst >= 0 ? pl[ci] : ci;
        if (nst < 0 && !(jl != r && rc_near(me0, rc_row(A, row00 + jl), reach))) continue;
        const float gj = A.gain[base + jl];
        if (gj > 0.f && !(gain > gj || (gain == gj && r < jl))) blocked = true;
    }
    if (__ballot(blocked) != 0ull) return;
    if (lane == 0) A.s[cr] = A.prop[cr];
}

// ---------------------------------------------------------------------------------------------
// behind the last sweep: pick, chi_out (one lane per consensus angle), then one workgroup per group for trace[g][K]
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_rc_finish(RcArgs A) {
    const int neb = (4 * A.M + 255) / 256;
    if ((int)blockIdx.x >= neb) {
        rc_trace_block(A, blockIdx.x - neb, A.K, false);
        return;
    }
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 4 * A.M) return;
    const int cr = e >> 2, c = e & 3;
    const int2 inf = A.info[cr];
    if (inf.x < 0) return;                              // pick stays -1, chi_out is not written
    const int sr = A.s[cr];
    const int row = pp_decoy_row0(A.seg_off, inf.x, A.D, A.N, sr) + inf.y;
    A.chi_out[e] = A.chi[(size_t)row * 4 + c];
    if (c == 0) A.pick[cr] = sr;
}

// The workspace of A (A.M, A.G set) out of the proximal buffers of the context: no allocation.  pm, pv, pz, pxeff and cand_cnt hold
// 4 N four-byte words each, cand 4 N PP_CL_CAP (pp_api.hip); every line below says how many words of which donor it takes.
static pp_status rc_workspace(const pp_ctx *c, RcArgs &A) {
    const size_t M = A.M, G = A.G, w = 4 * (size_t)c->N;
    const size_t fit[][2] = {{4 * M, w},                         // pm:       info [M] int2 | s [M] | prop [M]
                             {3 * M, w},                         // pv:       gain [M] | rowU [M] | rowW [M]
                             {4 * G, w},                         // pz:       ginfo [G] int4
                             {2 * G, w},                         // pxeff:    cnt [G][2]
                             {M * RC_LCAP, w * PP_CL_CAP},       // cand:     plist [M][RC_LCAP]
                             {M, w}};                            // cand_cnt: pcnt [M]
    bool ok = c->cand != nullptr;
    for (const auto &f : fit) ok = ok && f[0] <= f[1];
    if (!ok)
        FAIL(PP_ERR_INVALID, "pp_ensemble_recombine: " + std::to_string(M) + " consensus rows / " + std::to_string(G) +
                                 " groups do not fit the proximal workspace of this " + std::to_string(c->N) + "-row context");
    int32_t *pm = reinterpret_cast<int32_t *>(c->pm);
    A.info = reinterpret_cast<int2 *>(pm); A.s = pm + 2 * M; A.prop = pm + 3 * M;
    A.gain = c->pv; A.rowU = c->pv + M; A.rowW = c->pv + 2 * M;
    A.ginfo = reinterpret_cast<int4 *>(c->pz);
    A.cnt = reinterpret_cast<int32_t *>(c->pxeff);
    A.plist = c->cand; A.pcnt = c->cand_cnt;
    return PP_OK;
}

extern "C" pp_status pp_ensemble_recombine(pp_ctx *c, const float *chi, int n_decoys, const int32_t *start, int max_sweeps,
                                           int32_t *pick, float *chi_out, double *trace, int32_t *sweeps, int32_t *converged,
                                           float *energy, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !chi || !pick || !chi_out || !trace || !sweeps || !converged) FAIL(PP_ERR_INVALID, "pp_ensemble_recombine: null argument");
    if (n_decoys < 1) FAIL(PP_ERR_INVALID, "pp_ensemble_recombine: n_decoys must be at least 1");
    if (max_sweeps < 0) FAIL(PP_ERR_INVALID, "pp_ensemble_recombine: max_sweeps must not be negative");
    pp_status st;
    if ((st = pp_check_decoy_groups(c, n_decoys, "pp_ensemble_recombine")) != PP_OK) return st;
    if (!c->plan->clash_params_set) FAIL(PP_ERR_INVALID, "pp_ensemble_recombine: call pp_plan_set_clash_params first");
    if (!c->b.atom_mask || !c->b.residue_index) FAIL(PP_ERR_INVALID, "pp_ensemble_recombine: batch lacks atom_mask / residue_index");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const pp_plan *p = c->plan;
    RcArgs A;
    A.N = c->N; A.D = n_decoys; A.G = c->B / n_decoys; A.M = c->N / n_decoys; A.K = max_sweeps;
    A.seg_off = c->seg_off; A.chi = chi; A.rec = reinterpret_cast<const float4 *>(c->rec);
    A.X = c->b.X; A.amask = c->b.atom_mask; A.side_extent = p->side_extent; A.lower = p->bounds_lower; A.upper = p->bounds_upper;
    A.rtype = c->b.residue_type; A.rindex = c->b.residue_index; A.tol = p->clash_tol;
    A.oatoms = c->obst_M > 0 ? c->obst : nullptr; A.oseg = c->obst_seg;
    if ((st = rc_workspace(c, A)) != PP_OK) return st;
    A.start = start; A.pick = pick; A.sweeps = sweeps; A.converged = converged; A.chi_out = chi_out; A.energy = energy; A.trace = trace;
    PP_HIP_CHECK(hipMemsetAsync(pick, 0xff, (size_t)A.M * sizeof(int32_t), s));          // -1: rows of groups that are left alone
    const int nrb = (A.M + 3) / 4;
    hipLaunchKernelGGL(k_rc_setup, dim3(nrb + A.G), dim3(256), 0, s, A);
    PP_HIP_CHECK(hipGetLastError());
    if ((st = pp_launch_atom14(c, chi, c->xyz, s)) != PP_OK) return st;                 // the records of every decoy at chi
    for (int k = 0; k < max_sweeps; k++) {
        hipLaunchKernelGGL(k_rc_propose, dim3(A.M), dim3(256), 0, s, A, k, 1, 1);
        hipLaunchKernelGGL(k_rc_apply, dim3(nrb + A.G), dim3(256), 0, s, A, k);
    }
    // the row terms at the final assignment (max_sweeps = 0: also the place where `energy` is written)
    hipLaunchKernelGGL(k_rc_propose, dim3(A.M), dim3(256), 0, s, A, max_sweeps, (max_sweeps == 0 && energy) ? 1 : 0, 0);
    hipLaunchKernelGGL(k_rc_finish, dim3((4 * A.M + 255) / 256 + A.G), dim3(256), 0, s, A);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
