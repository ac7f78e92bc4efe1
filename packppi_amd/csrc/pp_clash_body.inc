// Body of the clash kernels of pp_clash.hip, k_clash<CAND, FUSE> and k_clash_seg<CAND> (included inside both; not a header).  It reads
// the kernel's parameters by name and two macros: PP_CLASH_INV_N, the 1 / n of the mean in the gradient weights (k_clash: its argument
// inv_ntot; k_clash_seg: inv_row[i], the residue's own complex), and PP_CLASH_STEP_INV_N, the 1 / n of the Adam step's anchor term
// (k_clash: U.inv_n; k_clash_seg: inv_row[i]).  Kept as text rather than as an inlined device function: that way k_clash compiles to
// exactly the instructions it did before k_clash_seg existed (an inlined body schedules differently).
    __shared__ int s_list[CL_WAVES][CL_MAXC];
    __shared__ float s_red[CL_WAVES][16][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x;              // one workgroup per residue; its waves take interleaved 64-partner windows
    if (i >= N) return;
    const int row0 = seg[i].x, L = seg[i].y;      // partner residues: the rows of this residue's own complex
    const int a = lane & 15, slot = lane >> 4;
    const bool own = a < 14;
    // rec[n] (written by k_atom14): 14 x (x, y, z, exists * radius) | (CA, bounding radius) | (n side-chain atoms,
    // residue_index, residue type): every partner needs 15 coalesced 16-byte reads instead of ~85 scattered ones
    const float4 me = rec[(size_t)i * 16 + 15];
    const int S = __float_as_int(me.z);
    const int ri = __float_as_int(me.y);
    float pa[3] = {0.f, 0.f, 0.f}, ea = 0.f, ra = 0.f;
    if (own) {
        const float4 q = rec[(size_t)i * 16 + a];
        pa[0] = q.x; pa[1] = q.y; pa[2] = q.z;
        ra = q.w;
        ea = q.w != 0.f ? 1.f : 0.f;
    }
    const float nsc = me.x;                          // number of side-chain atoms -> this residue's weight in the mean
    const float wi = PP_CLASH_INV_N / (nsc + 1e-10f);
    const float4 cme = rec[(size_t)i * 16 + 14];          // bounding sphere (centroid, radius)
    const float cai[3] = {cme.x, cme.y, cme.z};
    const float radi = cme.w;
    const float reach = 3.6f - tol;                 // largest r_a + r_b - tol (S-S)

    float loss_a = 0.f, ga[3] = {0.f, 0.f, 0.f};
    int *list = s_list[wave];
    int n_static = -1;
    if constexpr (CAND) n_static = cand_cnt[(size_t)i * CL_WAVES + wave];
    const int32_t *my_cand = CAND ? cand + ((size_t)i * CL_WAVES + wave) * PP_CL_CAP : nullptr;
    // partner residues of the same complex: from the static candidates (one pass), or in windows that fit the candidate list
    const bool use_static = CAND && n_static >= 0;
    bool more = true;
    for (int base = 64 * wave; use_static ? more : base < L; ) {
        int cnt = 0;
        int jscan = base;
        if (use_static) {
            // the static candidates of this wave (ascending, at most PP_CL_CAP <= CL_MAXC): the exact sphere test on each, compacted in order
            for (int c0 = 0; c0 < n_static; c0 += 64) {
                const int ci = c0 + lane;
                bool keep = false;
                int jg = 0;
                if (ci < n_static) {
                    jg = my_cand[ci];
                    const float4 cj = rec[(size_t)jg * 16 + 14];
                    float dx = cj.x - cai[0], dy = cj.y - cai[1], dz = cj.z - cai[2];
                    float lim = radi + cj.w + reach;
                    keep = (lim > 0.f) && (dx * dx + dy * dy + dz * dz < lim * lim);
                }
                unsigned long long bal = __ballot(keep);
                if (keep) list[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = jg;
                cnt += __popcll(bal);
            }
            more = false;
        } else {
            for (; jscan < L && cnt + 64 <= CL_MAXC; jscan += 64 * CL_WAVES) {
                int jl = jscan + lane;
                bool keep = false;
                if (jl < L) {
                    int jg = row0 + jl;
                    if (jg != i) {
                        const float4 cj = rec[(size_t)jg * 16 + 14];
                        const float4 mj = rec[(size_t)jg * 16 + 15];
                        float dx = cj.x - cai[0], dy = cj.y - cai[1], dz = cj.z - cai[2];
                        float lim = radi + cj.w + reach;
                        keep = (lim > 0.f) && (dx * dx + dy * dy + dz * dz < lim * lim) && (__float_as_int(mj.y) != ri);
                    }
                }
                unsigned long long bal = __ballot(keep);
                if (keep) list[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = row0 + jl;
                cnt += __popcll(bal);
            }
        }
        base = jscan;
        __builtin_amdgcn_wave_barrier();
        for (int c = slot; c < cnt; c += 4) {
            const int jg = list[c];
            // all of the partner's records first, unconditionally: inside the branches below the compiler may not hoist them,
            // and fourteen dependent round trips per candidate were 13 of this kernel's 20 us at T1124 (fetching the next
            // candidate's records one iteration ahead on top of this gains nothing)
            float4 pbr[14];
#pragma unroll
            for (int bb = 0; bb < 14; bb++) pbr[bb] = rec[(size_t)jg * 16 + bb];
            const float4 mj = rec[(size_t)jg * 16 + 15];
            const int rj = __float_as_int(mj.y);
            const bool i_low = ri < rj;
            const bool adjacent = i_low ? (ri + 1 == rj) : (rj + 1 == ri);
            const float wj = PP_CLASH_INV_N / (mj.x + 1e-10f);
            if (own && ea != 0.f) {
#pragma unroll
                for (int bb = 0; bb < 14; bb++) {
                    const float4 pb = pbr[bb];
                    bool ok = pb.w != 0.f && !(a < 4 && bb < 4) && !(a == 5 && bb == 5);
                    if (adjacent) {
                        // peptide bond C(lower) - N(higher)
                        if (i_low ? (a == 2 && bb == 0) : (a == 0 && bb == 2)) ok = false;
                    }
                    if (ok) {
                        float dx = pa[0] - pb.x, dy = pa[1] - pb.y, dz = pa[2] - pb.z;
                        // squared test first: the IEEE sqrt and the division below are ~50 instructions, and only a few
                        // per cent of the surviving atom pairs overlap (most trips skip the branch for the whole wave)
                        const float d2 = 1e-10f + dx * dx + dy * dy + dz * dz;
                        const float thr = (ra + pb.w) - tol;
                        if (!(thr > 0.f && d2 < thr * thr)) continue;
                        float d = sqrtf(d2);
                        float err = thr - d;
                        if (err > 0.f) {
                            loss_a += err;
                            float cw = (a >= 4 ? wi : 0.f) + (bb >= 4 ? wj : 0.f);
                            float sc = -cw / d;
                            ga[0] = fmaf(sc, dx, ga[0]); ga[1] = fmaf(sc, dy, ga[1]); ga[2] = fmaf(sc, dz, ga[2]);
                        }
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    // fold the 4 partner stripes, then the 4 waves (fixed order: reproducible)
    for (int o = 16; o <= 32; o <<= 1) {
        loss_a += __shfl_xor(loss_a, o);
        ga[0] += __shfl_xor(ga[0], o); ga[1] += __shfl_xor(ga[1], o); ga[2] += __shfl_xor(ga[2], o);
    }
    if (lane < 16) {
        s_red[wave][lane][0] = loss_a; s_red[wave][lane][1] = ga[0]; s_red[wave][lane][2] = ga[1]; s_red[wave][lane][3] = ga[2];
    }
    __syncthreads();
    if (wave != 0) return;
    if (slot == 0) {
#pragma unroll
        for (int w = 1; w < CL_WAVES; w++) {
            loss_a += s_red[w][a][0]; ga[0] += s_red[w][a][1]; ga[1] += s_red[w][a][2]; ga[2] += s_red[w][a][3];
        }
    } else {
        loss_a = 0.f; ga[0] = ga[1] = ga[2] = 0.f;
    }
    // within-residue bounds: stripes of partner atoms b = slot, slot+4, ...
    if (own && ea != 0.f) {
        for (int bb = slot; bb < 14; bb += 4) {
            if (bb == a || (a < 4 && bb < 4)) continue;
            const float4 pb = rec[(size_t)i * 16 + bb];
            if (pb.w == 0.f) continue;
            float dx = pa[0] - pb.x, dy = pa[1] - pb.y, dz = pa[2] - pb.z;
            float d = sqrtf(1e-10f + dx * dx + dy * dy + dz * dz);
            float lo = lower[(S * 14 + a) * 14 + bb], up = upper[(S * 14 + a) * 14 + bb];
            float e_lo = lo - d, e_up = d - up;
            float l = fmaxf(e_lo, 0.f) + fmaxf(e_up, 0.f);
            loss_a += 2.f * l;                                  // row sum + column sum of a symmetric table
            float dl = (e_up > 0.f ? 1.f : 0.f) - (e_lo > 0.f ? 1.f : 0.f);
            float cw = 2.f * ((a >= 4 ? wi : 0.f) + (bb >= 4 ? wi : 0.f));
            float sc = cw * dl / d;
            ga[0] = fmaf(sc, dx, ga[0]); ga[1] = fmaf(sc, dy, ga[1]); ga[2] = fmaf(sc, dz, ga[2]);
        }
    }
    // fold the 4 partner stripes
    for (int o = 16; o <= 32; o <<= 1) {
        loss_a += __shfl_xor(loss_a, o);
        ga[0] += __shfl_xor(ga[0], o); ga[1] += __shfl_xor(ga[1], o); ga[2] += __shfl_xor(ga[2], o);
    }
    float lres = (own && a >= 4) ? loss_a : 0.f;
    for (int o = 8; o > 0; o >>= 1) lres += __shfl_xor(lres, o);
    const float pres = lres / (nsc + 1e-10f);
    if (lane == 0) per_res[i] = pres;
    float dk[4] = {0.f, 0.f, 0.f, 0.f};
    if (dchi || FUSE) {
        if (own && a >= 5) {
            const int g = a2g[S * 14 + a];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (g >= 4 + k) {
                    const float *ax = axes + ((size_t)i * 4 + k) * 6;
                    float rx = pa[0] - ax[3], ry = pa[1] - ax[4], rz = pa[2] - ax[5];
                    float cx = ax[1] * rz - ax[2] * ry, cy = ax[2] * rx - ax[0] * rz, cz = ax[0] * ry - ax[1] * rx;
                    dk[k] = ga[0] * cx + ga[1] * cy + ga[2] * cz;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            for (int o = 8; o > 0; o >>= 1) dk[k] += __shfl_xor(dk[k], o);
        }
        if (dchi && lane < 4) dchi[(size_t)i * 4 + lane] = lane == 0 ? dk[0] : (lane == 1 ? dk[1] : (lane == 2 ? dk[2] : dk[3]));
    }
    if constexpr (FUSE) {
        const ProxUpd &U = F.U;
        const bool st = slot == 0;                  // the stripe that stores
        // everything the tail reads, in one batch: the reconstruction's inputs and the Adam operands of chi_k, k = a < 4
        const A14In I = a14_load(i, a, S, F.X, F.BB_D, F.default_frames, a2g, F.amask14, F.lit, F.atom_exists, F.between_radius);
        const int k = a < 4 ? a : 0;
        const size_t e = (size_t)i * 4 + k;
        const float xe = U.xeff[e], ze = U.z[e], xo = U.x[e], mo = U.m[e], vo = U.v[e], c0v = U.chi0[e];
        const bool mk = U.mask[i] != 0;
        // loss_t = mean_n [sum_k (xeff - z)^2 + lamda per_res] at the incoming iterate; then torch.optim.Adam defaults (lr 1e-2,
        // betas (0.9, 0.999), eps 1e-8, bias-corrected; step_size = lr / (1 - beta1^t) and bc2s = sqrt(1 - beta2^t) come from the
        // host in double); outputs as optimize.py:66-71
        const float dch = k == 0 ? dk[0] : (k == 1 ? dk[1] : (k == 2 ? dk[2] : dk[3]));
        float q = 0.f, outv = 0.f;
        if (a < 4) {
            const float d = xe - ze;
            q = fabsf(d) * fabsf(d);
            const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
            float g = 0.f;
            if (mk) g = 2.f * (xo - ze) * PP_CLASH_STEP_INV_N + U.lamda * dch;
            const float mm = mo + (g - mo) * (1.f - b1);             // exp_avg.lerp_(grad, 1 - beta1)
            const float vv = vo * b2 + (1.f - b2) * (g * g);
            const float denom = sqrtf(vv) / U.bc2s + eps;
            const float xn = xo - U.step_size * (mm / denom);
            outv = mk ? xn : c0v;
            if (st) {
                U.m[e] = mm; U.v[e] = vv; U.x[e] = xn;
                U.xeff[e] = outv;
                if (U.traj) U.traj[(size_t)U.t * N * 4 + e] = outv;
                if (U.last) U.last[e] = outv;
            }
        }
        q += __shfl_xor(q, 1, 16);
        q += __shfl_xor(q, 2, 16);
        if (lane == 0) U.loss_part[(size_t)U.t * N + i] = q + U.lamda * pres;
        // the reconstruction at the new angles: lane a in 3..6 evaluates chi_(a-3), which lane a - 3 has just stepped
        const float chi_new = __shfl(outv, (a - 3) & 15, 16);
        a14_finish(I, i, a, st, a < 3 ? I.bbd_t : chi_new, F.rindex, F.xyz, F.axes_out, F.brad, F.rec_out);
    }
