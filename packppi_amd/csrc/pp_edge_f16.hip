// The edge-level stages of InvariantPointMessagePassing (layers.py:65-148) on the F16 matrix pipe with fp32-level
// accuracy: the DEFAULT edge kernels (PACKPPI_EDGE=f32 builds the exact-fp32 ones of pp_edge.hip instead; same launchers,
// results equal to ~1e-6).
//
// Same decomposition as pp_edge.hip: a workgroup of 4 waves owns R residues (R = 1 or 2, template) and their K<=32 edges
// each, activations live in the 32x32 MFMA accumulator layout (lane = (edge, half h); register r of tile t <-> feature
// 32 t + 8 (r >> 2) + 4 h + (r & 3)) so that a layer's outputs are the next layer's B operands, wave w computes output
// tile w of every layer (N-split) and publishes it through a 16 KB LDS exchange buffer per residue, the 456-wide first
// layer is split by linearity, the edge update goes straight on to the next layer's node message.  What differs:
//   * arithmetic: every fp32 product is three v_mfma_f32_32x32x16_f16 on two-way f16 splits (below);
//   * weights go global memory -> registers (no LDS-DMA ring), three stages ahead of their use;
//   * a layer's input is read from LDS tile by tile, a stage ahead of its use, never held as a whole vector in registers;
//     LayerNorm statistics are reduced per wave and merged across the four waves (Chan): ~140 VGPRs, 38.4 KB of LDS ->
//     three workgroups per CU;
//   * f32 -> f16 conversions go through v_cvt_pkrtz_f16_f32 (see cvt2 below: with gfx950's v_cvt_pk_f16_f32 the kernels
//     were only correct with one wave per SIMD).
// Measured (MI355X, T1124, 100 steps): 45.5 k residues/s against 26.6 k for pp_edge.hip.
#include "pp_internal.h"

PP_RANGE_COUNTER
PP_RANGE_READER(pp_edge_range_hits)

#include "pp_edge_tile.h"      // f32x16 / f32x4v and the tile helpers shared by the two edge translation units
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

// ---- split-f16 arithmetic -------------------------------------------------------------------------------------
// Every fp32 operand x of the dense layers is carried as two f16 numbers, hi = f16(x) and lo = f16(x - hi)
// (x = hi + lo to 2^-22 relative; f16 subnormals are honoured by the MFMA, measured), and a product W x is three
// v_mfma_f32_32x32x16_f16 with fp32 accumulation: Wh xh + Wh xl + Wl xh (the dropped Wl xl term is 2^-22 relative).
// Measured (tools/debug/ubench/mfma_f16_probe.hip): K = 128 dot products come out as close to fp64 as a sequential fp32
// FMA chain does (2.7e-6 vs 4.1e-6 max abs error), at 3 x 32 cycles per 16-deep step against 8 x 64 cycles for
// v_mfma_f32_32x32x2_f32: 5.3x the FP32-matrix rate, with the same bytes per weight (2 x 2) and per activation.
// Range: |x| must stay below 65504 (LayerNorm-bounded activations and O(1) weights do by orders of magnitude).
//
// One tile (32 features of this lane's edge) as MFMA operands: k-step s in {0,1} carries accumulator registers
// 8s..8s+7 of the tile, i.e. features 32 t + 8 (2 s + (i >> 2)) + 4 h + (i & 3), i = 0..7, for lane half h.
struct HT {
    h8 hi[2], lo[2];
};
// RELU: the tile is max(v, 0) (hidden activations: also saturated at the f16 maximum, one v_med3 for both); otherwise v
// is a LayerNorm output or an h_E row (|v| far below 65504 by construction) and is split as it is.  Two values at a time
// so that hipcc emits v_cvt_pk_f16_f32 / v_pk_add_f32: 2.5 VALU instructions per value (3.5 with RELU).
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
// f32 pair -> packed f16 by v_cvt_pkrtz_f16_f32 (round toward zero), NOT by gfx950's new v_cvt_pk_f16_f32 (round to nearest
// even; what __builtin_convertvector and plain casts of a pair compile to).  A build with the packed round-to-nearest form
// everywhere (-DPP_X_CVT_PK) is not reproducible from run to run with two or more waves per SIMD.  Round 5 took that apart
// (profiles/r05_cvt_pk_hazard.txt): the instruction itself is clean -- in a micro-repro of 100 configurations and at every
// activation split of these kernels (bit-reproducible, 4.3e-6 rad at T1124) --; the failure is confined to geometry_put's four
// point pairs written as convertvector TOGETHER (each alone is clean, wait states do not cure it, the barrier protocol holds under
// injected skew): an interaction inside that one instruction sequence that no reduced form reproduces.  pkrtz stays, everywhere:
// one rounding rule for every operand.  The split does not care which way hi is rounded: lo = x - hi is exact either way and
// hi + lo still carries 21 bits of x; pkrtz is one instruction per pair.
typedef __fp16 fp16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h2v cvt2(f32x2v x) {
    const fp16x2_t r = __builtin_amdgcn_cvt_pkrtz(x[0], x[1]);
    return __builtin_bit_cast(h2v, r);
}
// x - (float)hh for a packed pair: one v_fma_mix_f32 per value (the f16 half is an operand of the fp32 FMA; exact, like the
// v_cvt_f32_f16 + v_sub_f32 pair it replaces -- a quarter of the split's VALU instructions)
__device__ __forceinline__ f32x2v split_residual(h2v hh, f32x2v x) {
    const unsigned hp = __builtin_bit_cast(unsigned, hh);
    float d0, d1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d0) : "v"(hp), "v"(x[0]));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d1) : "v"(hp), "v"(x[1]));
    return f32x2v{d0, d1};
}
typedef unsigned short us2v __attribute__((ext_vector_type(2)));
template <bool RELU>
__device__ __forceinline__ void split_tile(const f32x16 &v, HT &o, unsigned &sat) {
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int i = 0; i < 8; i += 2) {
            f32x2v x = {v[8 * s + i], v[8 * s + i + 1]};
            PP_RANGE(RELU ? fmaxf(x[0], 0.f) : x[0]) PP_RANGE(RELU ? fmaxf(x[1], 0.f) : x[1])
            if (RELU) {
                x[0] = __builtin_amdgcn_fmed3f(x[0], 0.f, 65504.f);
                x[1] = __builtin_amdgcn_fmed3f(x[1], 0.f, 65504.f);
            }
            const h2v hh = cvt2(x);
#ifndef PP_X_NOSAT     /* A/B aid: build without the sticky-flag bookkeeping */
            if (RELU)      // sticky saturation flag: running maximum of the clamped halves (v_pk_max_u16), see pp_internal.h
#else
            if (false)
#endif
                sat = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(us2v, sat), __builtin_bit_cast(us2v, hh)));
            const f32x2v d = split_residual(hh, x);
            const h2v ll = cvt2(d);
            o.hi[s][i] = hh[0]; o.hi[s][i + 1] = hh[1];
            o.lo[s][i] = ll[0]; o.lo[s][i + 1] = ll[1];
        }
}
__device__ __forceinline__ void join_tile(const HT &t, f32x16 &v) {
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int i = 0; i < 8; i++) v[8 * s + i] = (float)t.hi[s][i] + (float)t.lo[s][i];
}

#define ET 256
#define CH32 (128 * 32)                 // floats per packed weight chunk (16 KB); a wave's quarter is 1024 floats
#define XBUF_FLOATS (4 * 4 * 64 * 4)    // exchange buffer: [tile][quad][lane] float4
#define PARAM_FLOATS 1152               // edge kernel: small per-layer vectors, packed by pp_pack.h put_edge_params
#define PARAM_LDS 640                   // ... of which b_mid | b_out | ffn_out_b | g2 | be2 are staged to LDS (ffn_in_b is read in place), then g3 | be3 (256)

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

struct EdgeArgs {
    int N, K;
    float inv_K;
    union {                    // one slot, so that the argument block of every instance is laid out as it always was:
        const float *rmask;        // [N]
        const int32_t *live_rows;  // LIVE instances (they never read rmask: the list holds no masked row): [N + 2] the rows that get a
                                   // workgroup, ascending, then -1 (pp_prepare.hip k_live_rows)
        const int2 *live_mix;      // ... k_edge_update_mix: [N] the rows of workgroup b
    };
    const int32_t *eidx;       // [N][K]
    const float *mask_att;     // [N][32]
    const float *frames;       // [N][12]
    const float *pts;          // [N][48]   p_loc | p_glob of the message being computed
    const float *PA, *PC;      // [N][128]
    const float *hE_in;        // [N][K][128]
    float *hE_out;             // [N][K][128]   (edge kernel)
    float *S, *msum;           // node kernel outputs
    const float *wstream;      // this kernel's weight chunks, packed in consumption order (pp_pack.h put_chunk)
    const float *params;       // edge kernel: b_mid | b_out | ffn_out_b | g2 | be2 | ffn_in_b[512]
    const float *g3, *be3;     // edge kernel: last LayerNorm (read in the epilogue)
    const float *b_mid;        // node kernel (per-lane read)
    const float *Z;            // layer 0: precomputed W_B h_E0 of this message function [N][K][128]
    const float *pts2, *PA2, *PC2, *b_mid2;   // fused edge update: node-level inputs / bias of the NEXT node message
    float *Znm, *Zem;          // k_edge_static outputs
    const float *ls_in, *ls_x1, *ls_out;   // LNS kernels: power-of-two operand scales [128] of the h_E read, of x1, of the h_E written
    unsigned *sat;             // the context's sticky saturation word (bit 0: edge kernels)
    float *dbg;                // diagnostics: [N][4 waves][64 lanes][8] or null
    int n_pairs;               // k_edge_update_mix: workgroups with two residues (the rest have one)
    int mix_mode;
};
enum { P_BMID = 0, P_BOUT = 128, P_FOB = 256, P_G2 = 384, P_BE2 = 512, P_FIB = 640 };

// ---- weight pipeline: global memory -> registers, private to each wave -------------------------------------------
// Wave w only ever needs rows 32w..32w+31 of a weight chunk (its output tile), so its quarter of every chunk is packed
// (pp_plan_create, put_chunk_f16) as [quad q][lane][8 halves] = exactly the A-operand registers of the stage's MFMAs
// (q = k-step 0 hi, lo, k-step 1 hi, lo): four coalesced global_load_dwordx4 (1 KB each) per wave per stage, straight
// into one of PP_WDEPTH + 1 rotating operand sets, PP_WDEPTH stages ahead of their use.  The stream (0.9 MB per launch)
// is L2-resident; every fetch is amortised over the R residues of the workgroup.  No LDS hop, no M0, no hand-counted
// waits: these are ordinary loads, hipcc counts them (vmcnt) itself.  The earlier LDS-DMA ring (pp_edge.hip's scheme)
// needs M0 and a scalar base rewritten for every copy while earlier copies are still queued, which the hardware does not
// interlock ("Split-f16"); with a wave alone on its SIMD there are registers to spare instead.
// The chunk offset is made opaque and every stage starts with a scheduling barrier, so each fetch is issued where it is
// written (as read-only kernel arguments the compiler would otherwise hoist all of them to the top of the kernel).
#ifndef PP_WDEPTH
#define PP_WDEPTH 2        // stages a weight fetch runs ahead of its use, two-residue workgroups (a stage = 384 cycles of MFMAs)
#endif
#ifndef PP_WDEPTH_R1
#define PP_WDEPTH_R1 2     // ... one-residue workgroups (4 and 6 measured: no change, profiles/r04_ab_experiments.txt)
#endif
// ring depth of the instance in scope: every kernel body defines R (residues per workgroup)
#define WDEPTH_ (R == 1 ? PP_WDEPTH_R1 : PP_WDEPTH)
// -DPP_X_TS -DPP_X_TS_FINE=k0: wave 0's clock after each of the 16 stages k0 .. k0 + 15 of the edge update (measurement aid)
#if defined(PP_X_TS) && defined(PP_X_TS_FINE)
#define TSF(k) if constexpr ((k) >= PP_X_TS_FINE && (k) < PP_X_TS_FINE + 16) tsf[(k) - PP_X_TS_FINE] = (int)(__builtin_readcyclecounter() - ts0f);
#else
#define TSF(k)
#endif
// (PP_WGS2, the same for the two-residue instances: pp_internal.h, next to the launch-shape rule that counts in it)
#ifndef PP_WGS
#define PP_WGS 3           // register budget = 512 / PP_WGS per lane: three workgroups per CU (the kernels need ~140 VGPRs, 38.4 KB of LDS)
#endif
#define NRING (WDEPTH_ + 1)
#ifdef PP_X_NOWLOAD      /* timing experiment (results are wrong): no weight fetches after the prologue */
#define PP_X_NOWLOAD_ true
#else
#define PP_X_NOWLOAD_ false
#endif

#ifdef PP_X_E_NOMFMA     /* timing experiment (results are wrong): the matrix instructions are left out */
#define MFMA16(a, b, c) (c)
#else
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)
#endif

// A operands of one stage in registers: [s0 hi, s0 lo, s1 hi, s1 lo]
struct AOp {
    h8 r[4];
};
__device__ __forceinline__ void gload_A(const h8 *__restrict__ wq, int chunk, AOp &a) {
    int off = chunk * 1024;                  // h8 units per 16 KB chunk
    asm volatile("" : "+s"(off));
    const h8 *p = wq + off;
    a.r[0] = p[0]; a.r[1] = p[64]; a.r[2] = p[128]; a.r[3] = p[192];
}
// R residues share the A operands (weights) of a stage: R independent accumulator chains, issued interleaved so that a
// wave alone on its SIMD never waits on its own previous MFMA.  x[r][T] = input tile T of residue r.
template <int R, int T, bool SWAP>
__device__ __forceinline__ void mfma_x(const AOp &a, const HT (&x)[R][4], f32x16 (&acc)[R]) {
#pragma unroll
    for (int s = 0; s < 2; s++) {
        if (SWAP) {
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = MFMA16(x[r][T].hi[s], a.r[2 * s], acc[r]);
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = MFMA16(x[r][T].lo[s], a.r[2 * s], acc[r]);
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = MFMA16(x[r][T].hi[s], a.r[2 * s + 1], acc[r]);
        } else {
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = MFMA16(a.r[2 * s], x[r][T].hi[s], acc[r]);
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = MFMA16(a.r[2 * s], x[r][T].lo[s], acc[r]);
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = MFMA16(a.r[2 * s + 1], x[r][T].hi[s], acc[r]);
        }
    }
}
// one k-step S of a stage (3 R MFMAs) on one tile per residue; a stage = k-steps 0 and 1 of its weight chunk
template <int R, bool SWAP, int S>
__device__ __forceinline__ void mfma_hs(const AOp &a, const HT (&x)[R], f32x16 (&acc)[R]) {
    if (SWAP) {
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = MFMA16(x[r].hi[S], a.r[2 * S], acc[r]);
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = MFMA16(x[r].lo[S], a.r[2 * S], acc[r]);
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = MFMA16(x[r].hi[S], a.r[2 * S + 1], acc[r]);
    } else {
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = MFMA16(a.r[2 * S], x[r].hi[S], acc[r]);
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = MFMA16(a.r[2 * S], x[r].lo[S], acc[r]);
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = MFMA16(a.r[2 * S + 1], x[r].hi[S], acc[r]);
    }
}
// the 72 invariant-point features as operands: lane half h carries the features of points 4h .. 4h+3, one point per
// k-step S5 = 0..3 and the four distances in k-step 4 (geometry_put below); geometry chunk C holds k-steps 2C and 2C+1
// (the last one is all padding and skipped).  The operands live in a 10 KB LDS block per residue, [k-step][hi | lo][lane] h8.
#define GBUF_FLOATS (5 * 2 * 64 * 4)
template <int R, int C>
__device__ __forceinline__ void mfma_geo(const AOp &a, const float *gbuf, int lane, f32x16 (&acc)[R]) {
#pragma unroll
    for (int s = 0; s < 2; s++) {
        if (2 * C + s < 5) {
            h8 ghi[R], glo[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const h8 *gp = reinterpret_cast<const h8 *>(gbuf + r * GBUF_FLOATS) + (2 * (2 * C + s)) * 64 + lane;
                ghi[r] = gp[0];
                glo[r] = gp[64];
            }
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = MFMA16(a.r[2 * s], ghi[r], acc[r]);
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = MFMA16(a.r[2 * s], glo[r], acc[r]);
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = MFMA16(a.r[2 * s + 1], ghi[r], acc[r]);
        }
    }
}
// a tile that is only ever ADDED to another one travels as four independent 16-byte pieces: a 16-register tuple for it would
// fragment the register file where many tiles are in flight at once (the batched prologue loads)
struct TileQ {
    f32x4v q[4];
};
__device__ __forceinline__ void load_tile_q(const float *__restrict__ row32, int h, TileQ &t) {
#pragma unroll
    for (int q = 0; q < 4; q++) t.q[q] = *reinterpret_cast<const f32x4v *>(row32 + 8 * q + 4 * h);
}
__device__ __forceinline__ void add_tile_q(const TileQ &t, f32x16 &d) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        d[4 * q] += t.q[q][0]; d[4 * q + 1] += t.q[q][1]; d[4 * q + 2] += t.q[q][2]; d[4 * q + 3] += t.q[q][3];
    }
}
// LNS instances: dst = src * s, s a per-feature power of two (exact) -- the operand copy that gets split when a LayerNorm gain is
// far from 1 (pp_rebalance.h ln_operand_scales); the tile itself, which also feeds a residual path, stays as it is
__device__ __forceinline__ void scale_tile(const float *__restrict__ s32, int h, const f32x16 &src, f32x16 &dst) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const f32x4v a = *reinterpret_cast<const f32x4v *>(s32 + 8 * q + 4 * h);
        dst[4 * q] = src[4 * q] * a[0]; dst[4 * q + 1] = src[4 * q + 1] * a[1]; dst[4 * q + 2] = src[4 * q + 2] * a[2]; dst[4 * q + 3] = src[4 * q + 3] * a[3];
    }
}
// publish SRC as operands: as it is, or (LNS) times the scale vector SV
#define PUBLISH_OPERAND(SRC, BUF, SV)                                                     \
    if constexpr (LNS) {                                                                  \
        f32x16 sc_[R];                                                                    \
        _Pragma("unroll") for (int r = 0; r < R; r++) scale_tile((SV) + 32 * wave, h, SRC[r], sc_[r]);   \
        PUBLISH_OWN(false, sc_, BUF)                                                      \
    } else {                                                                              \
        PUBLISH_OWN(false, SRC, BUF)                                                      \
    }
// split tiles through the exchange buffer (xbuf_put / xbuf_get of pp_edge_tile.h), the same 4 KB per tile:
// [hi s0 | hi s1 | lo s0 | lo s1][lane] h8
__device__ __forceinline__ void xbuf_put_h(float *xbuf, int t, int lane, const HT &d) {
    h8 *xb = reinterpret_cast<h8 *>(xbuf) + (t * 4) * 64 + lane;
    xb[0] = d.hi[0]; xb[64] = d.hi[1]; xb[128] = d.lo[0]; xb[192] = d.lo[1];
}
__device__ __forceinline__ void xbuf_get_h(const float *xbuf, int t, int lane, HT &d) {
    const h8 *xb = reinterpret_cast<const h8 *>(xbuf) + (t * 4) * 64 + lane;
    d.hi[0] = xb[0]; d.hi[1] = xb[64]; d.lo[0] = xb[128]; d.lo[1] = xb[192];
}

// 72 invariant point features of edge (i, j) as split-f16 MFMA operands in LDS.  Lane half h carries the features of
// points 4h .. 4h+3 (pp_pack.h put_geo_chunk permutes W_G's columns to match), point-major: k-step q = 0..3 holds point
// 4h + q as  p_loc xyz | |p_loc| | R_i^T (p_glob_j - t_i) xyz | its norm;  k-step 4 holds |p_glob_i - p_glob_j| of the four
// points | 0 x4.  All four waves need all of it as B operand, so they SHARE the work: wave w computes point 4h + w of its
// lanes, splits its eight values into ONE operand vector (hi, lo: two lane-linear 16-byte LDS writes) and drops its
// distance into k-step 4; a workgroup barrier follows at the call site.
// The inputs come in two levels: geo_load_i needs only the residue index (the residue's own point 4h + q, local and global,
// and its frame), geo_load_j the neighbour index (the neighbour's global point); geometry_put is arithmetic + LDS writes.
struct GeoI {
    float lx, ly, lz, gx, gy, gz;
    float fr[12];
};
__device__ __forceinline__ void geo_load_i(const float *__restrict__ pts_i, const float *__restrict__ fr, int h, int q, GeoI &g) {
    const float *pl = pts_i + 12 * h + 3 * q, *pg = pts_i + 24 + 12 * h + 3 * q;
    g.lx = pl[0]; g.ly = pl[1]; g.lz = pl[2];
    g.gx = pg[0]; g.gy = pg[1]; g.gz = pg[2];
#pragma unroll
    for (int k = 0; k < 12; k++) g.fr[k] = fr[k];
}
__device__ __forceinline__ void geo_load_j(const float *__restrict__ pts_j, int h, int q, float (&pj)[3]) {
    const float *p = pts_j + 24 + 12 * h + 3 * q;
    pj[0] = p[0]; pj[1] = p[1]; pj[2] = p[2];
}
__device__ __forceinline__ void geometry_put(const GeoI &g, const float (&pj)[3], int wave, int lane, float *gbuf) {
    const int q = wave;
    const float *fr = g.fr;
    const float lx = g.lx, ly = g.ly, lz = g.lz;
    const float gx = g.gx, gy = g.gy, gz = g.gz;
    const float jx = pj[0], jy = pj[1], jz = pj[2];
    float v[10];
    v[0] = lx; v[1] = ly; v[2] = lz;
    v[3] = sqrtf(lx * lx + ly * ly + lz * lz + 1e-8f);
    const float dx = jx - fr[9], dy = jy - fr[10], dz = jz - fr[11];
    const float nx = fr[0] * dx + fr[3] * dy + fr[6] * dz;
    const float ny = fr[1] * dx + fr[4] * dy + fr[7] * dz;
    const float nz = fr[2] * dx + fr[5] * dy + fr[8] * dz;
    v[4] = nx; v[5] = ny; v[6] = nz;
    v[7] = sqrtf(nx * nx + ny * ny + nz * nz + 1e-8f);
    const float ex = gx - jx, ey = gy - jy, ez = gz - jz;
    v[8] = sqrtf(ex * ex + ey * ey + ez * ez + 1e-8f);
    v[9] = 0.f;
    h8 vh, vl;
    h2v dh, dl;
#pragma unroll
    for (int i = 0; i < 10; i += 2) {
        const f32x2v x = {v[i], v[i + 1]};
        PP_RANGE(x[0]) PP_RANGE(x[1])
        const h2v hh = cvt2(x);
        const f32x2v d = split_residual(hh, x);
        const h2v ll = cvt2(d);
        if (i < 8) { vh[i] = hh[0]; vh[i + 1] = hh[1]; vl[i] = ll[0]; vl[i + 1] = ll[1]; }
        else { dh = hh; dl = ll; }
    }
    h8 *gv = reinterpret_cast<h8 *>(gbuf);
    gv[(2 * q) * 64 + lane] = vh;                       // k-step q, hi
    gv[(2 * q + 1) * 64 + lane] = vl;                   // k-step q, lo
    _Float16 *gh = reinterpret_cast<_Float16 *>(gbuf);
    gh[((2 * 4) * 64 + lane) * 8 + q] = dh[0];          // k-step 4, element q: this point's distance
    gh[((2 * 4 + 1) * 64 + lane) * 8 + q] = dl[0];
    if (wave == 0) {          // padding elements 4..7 of k-step 4, hi and lo
        const f32x2v z = {0.f, 0.f};
        *reinterpret_cast<f32x2v *>(gh + ((2 * 4) * 64 + lane) * 8 + 4) = z;
        *reinterpret_cast<f32x2v *>(gh + ((2 * 4 + 1) * 64 + lane) * 8 + 4) = z;
    }
}

// ACC names the accumulator array the stage's MFMAs chain on: the empty asm at the end uses one element of every chain,
// which keeps the MFMAs inside their stage (they are pure, and instruction selection would otherwise let them sink past
// the following stages' fetches, keeping every operand set alive).
#define WSTAGE(k, NCH, ACC, BODY)                                                                              \
    {                                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        if constexpr ((k) + WDEPTH_ < (NCH) && !PP_X_NOWLOAD_)                                                 \
            gload_A(wq, (k) + WDEPTH_, AR[((k) + WDEPTH_) % NRING]);                                           \
        const AOp &AK = AR[(k) % NRING];                                                                       \
        BODY;                                                                                                  \
        _Pragma("unroll") for (int r_ = 0; r_ < R; r_++) asm volatile("" ::"v"(ACC[r_][0]));                   \
        TSF(k)                                                                                                 \
    }

// ---- activations between layers -----------------------------------------------------------------------------------
// A layer's input (B operands) is read from LDS tile by tile, one stage ahead of its use, into two rotating operand sets
// `bt` -- never as a whole 128-feature vector in registers (64 VGPRs): that is what lets two two-residue workgroups share a
// CU.  Buffers per residue: xbuf (the exchange buffer every layer publishes into) and, in the edge update, x1buf (the
// LayerNorm-2 output, which all four FFN blocks and nobody else read) -- 16 KB each, split-f16 tiles.
//
// ROTATED TILE ORDER (round 4).  Wave w owns output tile w of every layer, so after a layer it holds tile w of the next
// layer's input in registers -- the one tile it does not have to wait for.  The stages of a layer therefore visit the input
// tiles in the order w, w+1, w+2, w+3 (mod 4): position 0 takes its B operands straight from the split (registers), and the
// two workgroup barriers of a hand-over move INSIDE matrix stages, where the wave's own MFMAs (and the other workgroup's)
// cover them:
//   barrier B ("every wave has published its tile") sits between the two k-steps of position 0; the LDS reads of the second
//             tile are issued right behind it and land under the second k-step;
//   barrier A ("every wave has read the buffer the next publication overwrites") sits between the two k-steps of a later
//             stage whose operands have arrived -- position 3 of the layer, or of the W1 block in front of the publication.
// A hand-over used to be: barrier, ReLU + split, LDS write, barrier, LDS read latency, all exposed (~1 300 cycles of a lone
// workgroup, x10 per launch: profiles/r03_edge_stage_stamps.txt); what stays exposed is the split itself.  The weight stream
// is private to each wave, so the rotation costs nothing: pp_pack.h put_chunk_rot packs wave w's quarter of the chunk at
// position p from input tile (w + p) & 3.  (Accumulation order per output feature changes with the wave: results differ
// from round 3 by fp32 rounding, deterministically.)
#define ROT(p) ((wave + (p)) & 3)        // input tile at position p of a rotated layer (wave-uniform)
#define BT_FETCH(BUF, t, set)                                                     \
    _Pragma("unroll") for (int r = 0; r < R; r++) xbuf_get_h((BUF) + r * XBUF_FLOATS, t, lane, bt[set][r]);
// every accumulator chain reaches this point before anything behind it is issued (MFMAs are pure: without a use the
// instruction selection would let them sink past a barrier)
#define ACC_FENCE(ACC) _Pragma("unroll") for (int r_ = 0; r_ < R; r_++) asm volatile("" ::"v"(ACC[r_][0]));
// stage k = position P of a rotated layer reading BUF: B operand = bt[P & 1] (tile ROT(P)); the next tile is requested first,
// or -- FETCH_LATE -- behind the barrier in the middle of the stage (position 0: the tile was published by another wave).
// BAR: a workgroup barrier between the two k-steps.
#define RSTAGE(k, NCH, ACC, BUF, P, SWAP, BAR, FETCH_LATE)                                                  \
    WSTAGE(k, NCH, ACC, {                                                                                   \
        if constexpr ((P) < 3 && !(FETCH_LATE)) { BT_FETCH(BUF, ROT((P) + 1), ((P) + 1) & 1) }   \
        (mfma_hs<R, SWAP, 0>(AK, bt[(P) & 1], ACC));                                                        \
        if constexpr (BAR) { ACC_FENCE(ACC) __syncthreads(); }                                              \
        if constexpr ((P) < 3 && (FETCH_LATE)) { BT_FETCH(BUF, ROT((P) + 1), ((P) + 1) & 1) }    \
        (mfma_hs<R, SWAP, 1>(AK, bt[(P) & 1], ACC));                                                        \
    })
// a layer whose first B operands (the wave's own tile) are in bt[0] already -- PUBLISH_OWN() put them there and into BUF.
// BAR_A: barrier A in position 3 (the next publication overwrites BUF and no other barrier lies in between).
#define RLAYER_OWN(k0, NCH, ACC, BUF, SWAP, BAR_A)                                \
    RSTAGE((k0) + 0, NCH, ACC, BUF, 0, SWAP, true, true)                          \
    RSTAGE((k0) + 1, NCH, ACC, BUF, 1, SWAP, false, false)                        \
    RSTAGE((k0) + 2, NCH, ACC, BUF, 2, SWAP, false, false)                        \
    RSTAGE((k0) + 3, NCH, ACC, BUF, 3, SWAP, BAR_A, false)
// a layer reading a buffer that was published long ago (x1buf in the FFN blocks 1..3): every tile comes from LDS
#define RLAYER_BUF(k0, NCH, ACC, BUF, SWAP, BAR_A)                                \
    BT_FETCH(BUF, ROT(0), 0)                                                      \
    RSTAGE((k0) + 0, NCH, ACC, BUF, 0, SWAP, false, false)                        \
    RSTAGE((k0) + 1, NCH, ACC, BUF, 1, SWAP, false, false)                        \
    RSTAGE((k0) + 2, NCH, ACC, BUF, 2, SWAP, false, false)                        \
    RSTAGE((k0) + 3, NCH, ACC, BUF, 3, SWAP, BAR_A, false)
// publish this wave's tile of every residue (split, RELU or not) into BUF and keep it as the B operands of position 0.  No
// barrier here: B follows inside position 0 of the consuming layer, A was passed inside an earlier stage.
#define PUBLISH_OWN(RELU, SRC, BUF)                                               \
    _Pragma("unroll") for (int r = 0; r < R; r++) {                               \
        split_tile<RELU>(SRC[r], bt[0][r], sat);                                  \
        xbuf_put_h((BUF) + r * XBUF_FLOATS, wave, lane, bt[0][r]);                \
    }

// shared first layer: acc (tile `wave`) = PA_i + PC_j + W_B h_E + W_G geom, ReLU.  Chunks W_B x4 (absent when ST0: layer 0's
// W_B h_E0 is timestep-invariant and arrives precomputed in acc), then W_G x3.  C0 = number of W_B chunks.  The h_E tiles
// were published by the caller (PUBLISH_OWN: each wave its own tile; position 0's barrier also publishes the geometry
// operands); with ST0 the caller's barrier did.  Barrier A for the publication that follows sits in front of the last
// geometry stage (!ST0 only: with ST0 nothing has read xbuf yet).
#define FIRST_LAYER(K0, NCH)                                                      \
    if constexpr (!ST0) {                                                         \
        RLAYER_OWN((K0) + 0, NCH, acc, xbuf, false, false)                        \
    }                                                                             \
    WSTAGE((K0) + C0 + 0, NCH, acc, (mfma_geo<R, 0>(AK, gbuf, lane, acc)))        \
    WSTAGE((K0) + C0 + 1, NCH, acc, (mfma_geo<R, 1>(AK, gbuf, lane, acc)))        \
    if constexpr (!ST0) { __syncthreads(); }                                      \
    WSTAGE((K0) + C0 + 2, NCH, acc, (mfma_geo<R, 2>(AK, gbuf, lane, acc)))        \
    PUBLISH_OWN(true, acc, xbuf)

#define PROLOGUE_PIPE(NCH)                                                                                     \
    const h8 *wq = reinterpret_cast<const h8 *>(A.wstream) + wave * 256 + lane;    /* this wave's quarter, this lane */ \
    AOp AR[NRING];                                                                                             \
    _Pragma("unroll") for (int pk = 0; pk < WDEPTH_ && pk < (NCH); pk++) gload_A(wq, pk, AR[pk]);

// The R residues of a workgroup are rows res0 .. res0 + R - 1.  `live` = in range and not masked; a dead slot computes on
// a live residue's inputs (no garbage enters the pipes) and stores nothing.  All of it is wave-uniform.
#define GROUP_SETUP()                                                                          \
    int n[R];                                                                                  \
    bool live[R], inr[R];                                                                      \
    int first = -1;                                                                            \
    GROUP_SETUP_ROWS()
#define GROUP_SETUP_ROWS()                                                                     \
    float rm_[R];                                                                              \
    _Pragma("unroll") for (int r = 0; r < R; r++) {                                            \
        const int nr = res0 + r;                                                               \
        inr[r] = nr < A.N;                                                                     \
        n[r] = inr[r] ? nr : A.N - 1;                                                          \
        rm_[r] = A.rmask[n[r]];                                                                \
    }                                                                                          \
    _Pragma("unroll") for (int r = 0; r < R; r++) {                                            \
        live[r] = inr[r] && rm_[r] != 0.f;                                                     \
        if (live[r] && first < 0) first = n[r];                                                \
    }

// LayerNorm over the 128 features of an edge whose four 32-feature tiles sit in four different waves: every wave
// reduces its own tile (mean and centred sum of squares of 32 values: 16 here, 16 in lane ^ 32), the four partials meet
// in a 1 KB LDS block `st` ([wave][edge] float2) and are merged with the pairwise update of Chan et al. (equal counts),
// which is as stable as the reference's two-pass variance.  ln_partial: before the barrier; ln_merge: after it.
__device__ __forceinline__ void ln_partial(const f32x16 &v, float *st, int wave, int j, int h) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 16; q++) s += v[q];
    s += __shfl_xor(s, 32);
    const float m = s * (1.f / 32.f);
    float q2 = 0.f;
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const float d = v[q] - m;
        q2 = fmaf(d, d, q2);
    }
    q2 += __shfl_xor(q2, 32);
    if (h == 0) {
        f32x2v o = {m, q2};
        *reinterpret_cast<f32x2v *>(st + (wave * 32 + j) * 2) = o;
    }
}
__device__ __forceinline__ float ln_merge(const float *st, int j, float &mean_out) {
    f32x2v p[4];
#pragma unroll
    for (int w = 0; w < 4; w++) p[w] = *reinterpret_cast<const f32x2v *>(st + (w * 32 + j) * 2);
    const float mean = 0.25f * ((p[0][0] + p[1][0]) + (p[2][0] + p[3][0]));
    float m2 = (p[0][1] + p[1][1]) + (p[2][1] + p[3][1]);
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const float d = p[w][0] - mean;
        m2 = fmaf(32.f * d, d, m2);
    }
    mean_out = mean;
    return 1.f / sqrtf(m2 * (1.f / 128.f) + 1e-5f);
}
#define STAT_FLOATS 256

// ---------------------------------------------------------------------------------------------
// node message: S[i] = (1/K) sum_j mask_ij relu(W_mid relu(W_in [..]) + b), msum[i] = (1/K) sum_j mask_ij
// ---------------------------------------------------------------------------------------------
template <int R, bool ST0>
__device__ __forceinline__ void node_message_body(const EdgeArgs &A, const int res0, float *smem) {
    float *const xbuf = smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int K = A.K;
    unsigned sat = 0;
    GROUP_SETUP()
#pragma unroll
    for (int r = 0; r < R; r++)
        if (inr[r] && !live[r]) {         // masked / padded residue
            if (tid < 128) A.S[(size_t)n[r] * 128 + tid] = 0.f;
            if (tid == 0) A.msum[n[r]] = 0.f;
        }
    if (first < 0) return;
#pragma unroll
    for (int r = 0; r < R; r++)
        if (!live[r]) n[r] = first;
    constexpr int C0 = ST0 ? 0 : 4;
    constexpr int NCH = C0 + 7;           // chunks: [W_B x4,] W_G x3, W_mid x4
#if defined(PP_X_TS) && defined(PP_X_TS_FINE)
    const unsigned long long ts0f = __builtin_readcyclecounter();
    int tsf[16] = {0};
#endif
    HT bt[2][R];
    f32x16 acc[R];
    float *gbuf = smem + R * XBUF_FLOATS;
    const int jj = j < K ? j : K - 1;
    // loads in two levels, each for every residue at once (as in edge_update_body): what needs only the row index, then the
    // neighbour-dependent gathers together with the accumulator tiles
    int nbr[R];
#pragma unroll
    for (int r = 0; r < R; r++) nbr[r] = A.eidx[(size_t)n[r] * K + jj];
    GeoI gi0[R];
    float pj[R][3];
    f32x16 hin[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        geo_load_i(A.pts + (size_t)n[r] * 48, A.frames + (size_t)n[r] * 12, h, wave, gi0[r]);
        if constexpr (!ST0) load_tile(A.hE_in + ((size_t)n[r] * K + jj) * 128 + 32 * wave, h, hin[r]);   // this wave's tile of h_E
    }
    const float bmid = A.b_mid[32 * wave + j];            // SWAP form: feature on the lane
    PROLOGUE_PIPE(NCH)
    TileQ pc[R], zt[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        geo_load_j(A.pts + (size_t)nbr[r] * 48, h, wave, pj[r]);
        load_tile(A.PA + (size_t)n[r] * 128 + 32 * wave, h, acc[r]);
        load_tile_q(A.PC + (size_t)nbr[r] * 128 + 32 * wave, h, pc[r]);
        if constexpr (ST0) load_tile_q(A.Z + ((size_t)n[r] * K + jj) * 128 + 32 * wave, h, zt[r]);
    }
    if constexpr (!ST0) { PUBLISH_OWN(false, hin, xbuf) }
#pragma unroll
    for (int r = 0; r < R; r++) {
        geometry_put(gi0[r], pj[r], wave, lane, gbuf + r * GBUF_FLOATS);
        add_tile_q(pc[r], acc[r]);
        if constexpr (ST0) add_tile_q(zt[r], acc[r]);
    }
    if constexpr (ST0) __syncthreads();   // geometry operands are in LDS (otherwise the first W_B stage's barrier says so)
    FIRST_LAYER(0, NCH)
    // the edge masks of the final reduction are requested before the last layer (read where they are used, their round trip
    // followed the last MFMA)
    f32x4v mmv[R][4];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const float *mrow = A.mask_att + (size_t)n[r] * 32 + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; q++) mmv[r][q] = *reinterpret_cast<const f32x4v *>(mrow + 8 * q);
    }
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int q = 0; q < 16; q++) acc[r][q] = bmid;
    RLAYER_OWN(C0 + 3, NCH, acc, xbuf, true, false)
#pragma unroll
    for (int r = 0; r < R; r++) {
        // rows (registers) are edges e = 8 (r>>2) + 4 h + (r&3); mask and reduce over them
        float s = 0.f, ms = 0.f;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const f32x4v mm = mmv[r][q];
#pragma unroll
            for (int pq = 0; pq < 4; pq++) {
                s = fmaf(fmaxf(acc[r][4 * q + pq], 0.f), mm[pq], s);
                ms += mm[pq];
            }
        }
        s += __shfl_xor(s, 32);
        ms += __shfl_xor(ms, 32);
        if (live[r]) {
            if (h == 0) A.S[(size_t)n[r] * 128 + 32 * wave + j] = s * A.inv_K;
            if (tid == 0) A.msum[n[r]] = ms * A.inv_K;
        }
    }
    if (pp_sat_hit(sat)) atomicOr(A.sat, 1u);
}

// three workgroups per CU for both instances: the stand-alone node message is a chain of gathers with 84 MFMAs per wave behind
// it (52 KB of LDS and <= 168 registers at R = 2), so a third resident workgroup is cover, not contention
#ifndef PP_NM_WGS2
#define PP_NM_WGS2 3       // workgroups per CU of the two-residue node message (2 = the edge update's budget: round-4 behaviour)
#endif
template <int R, bool ST0>
__global__ void __launch_bounds__(ET, R == 1 ? PP_WGS : PP_NM_WGS2)
k_node_message(EdgeArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    node_message_body<R, ST0>(A, blockIdx.x * R, smem);
}

// ---------------------------------------------------------------------------------------------
// edge update: h_E <- mask * LN3(x1 + FFN(x1)),  x1 = LN2(h_E + mask * MLP3([..]))
// ---------------------------------------------------------------------------------------------
// FFN hidden block c (chunks 15 + 8c ..): W1 s=0..3 (input: the x1 tiles) -> hidden tile 4c+wave -> exchange ->
// W2 s'=0..3 accumulate into out
// The block's bias tile (global memory: LDS has no room for the 512 values in the one-residue instances) is requested a layer
// ahead into `fib` -- under the W2 stages of the block before, block 0's before the second LayerNorm: read where it is
// needed, its L2 round trip (~470 cycles, stage stamps: -DPP_X_TS_FINE) sat on the critical path of every block.
#define FFN_BIAS_FETCH(c) load_tile(A.params + P_FIB + 128 * (c) + 32 * wave, h, fib);
// hidden block c: W1 (input x1buf: block 0 right behind its publication -- own tile first --, blocks 1..3 from LDS, with
// barrier A for the publication of the hidden tile in their last position: every wave is done with the previous block's W2
// reads of xbuf by then), ReLU + split + publish into xbuf, W2 (own hidden tile first) accumulating into `out`
#define FFN_BLOCK(c)                                                                                         \
    _Pragma("unroll") for (int r = 0; r < R; r++) acc[r] = fib;                                              \
    if constexpr ((c) == 0) { RLAYER_OWN(C0 + 11 + 8 * (c), NCH, acc, x1buf, false, false) }                 \
    else { RLAYER_BUF(C0 + 11 + 8 * (c), NCH, acc, x1buf, false, true) }                                     \
    PUBLISH_OWN(true, acc, xbuf)                                                                             \
    if constexpr ((c) < 3) { FFN_BIAS_FETCH((c) + 1) }                                                       \
    RLAYER_OWN(C0 + 11 + 8 * (c) + 4, NCH, out, xbuf, false, false)

// -DPP_X_TS: phase timestamps (s_memtime, core-clock cycles since kernel start) of wave 0 to dbg[n][24]
// (tools/debug/phase_times.py)
#ifdef PP_X_TS
#define TS(i) { tsv[i] = (int)(__builtin_readcyclecounter() - ts0); }
#else
#define TS(i)
#endif
// FUSE: the workgroup goes straight on to the NEXT layer's node message of its residues (same edges, whose new h_E it
// holds; the node-level inputs PA2 / PC2 / pts2 were written by the node update that ran before this kernel): one
// launch, one prologue and one read of h_E less per layer.
// LNS: the plan carries operand scales behind small LayerNorm gains (A.ls_*): the three LayerNorm outputs that become f16 operands
// are multiplied by their power-of-two scale vector before the split (the default instances contain none of it).
// WB: the new h_E is written back to A.hE_out (masked rows as zeros).  Without it (the layer-1 launch of a fused evaluation,
// whose only consumer of h_E is the fused message below, fed from registers through xbuf) neither store is issued.
// LIVE (the layer-1 launch of a sampling run): the workgroup's rows are lrow.x and, R = 2, lrow.y -- entries of the context's
// live-row list, -1 for an empty second slot -- instead of res0 .. res0 + R - 1.  The list holds no masked row, so its lookup at
// the kernel's entry stands where the other instances read residue_mask: the prologue keeps its four dependent round trips.  A
// row that is not listed gets no workgroup: its S / msum keep what layer 0's launch wrote (pp_api.hip run_network).
template <int R, bool ST0, bool FUSE, bool LNS = false, bool WB = true, bool LIVE = false>
__device__ __forceinline__ void edge_update_body(const EdgeArgs &A, const int res0, float *smem, const int2 lrow = {-1, -1}) {
    float *const xbuf = smem, *const x1buf = smem + R * XBUF_FLOATS, *const stat = x1buf + R * XBUF_FLOATS,
                 *const prm = stat + R * STAT_FLOATS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int K = A.K;
    const int jj = j < K ? j : K - 1;
    unsigned sat = 0;
    int n[R];
    bool live[R], inr[R];
    int first = -1;
    if constexpr (LIVE) {
        static_assert(!WB, "a launch over the live rows alone leaves the other rows' h_E unwritten");
#pragma unroll
        for (int r = 0; r < R; r++) {
            n[r] = r == 0 ? lrow.x : lrow.y;
            inr[r] = live[r] = n[r] >= 0;
        }
        first = lrow.x;                   // (the caller left if the workgroup has no row)
    } else {
        GROUP_SETUP_ROWS()
    }
#pragma unroll
    for (int r = 0; r < R; r++)
        if (!LIVE && inr[r] && !live[r]) {         // masked / padded residue: its edges are zero
            if (WB && j < K) {
                f32x4v z = {0.f, 0.f, 0.f, 0.f};
                float *orow = A.hE_out + ((size_t)n[r] * K + j) * 128 + 32 * wave;
#pragma unroll
                for (int q = 0; q < 4; q++) *reinterpret_cast<f32x4v *>(orow + 8 * q + 4 * h) = z;
            }
            if constexpr (FUSE) {
                if (tid < 128) A.S[(size_t)n[r] * 128 + tid] = 0.f;
                if (tid == 0) A.msum[n[r]] = 0.f;
            }
        }
    if (first < 0) return;
#pragma unroll
    for (int r = 0; r < R; r++)
        if (!live[r]) n[r] = first;
    // chunks: [W_B x4,] W_G x3, W_mid x4, W_out x4, then per hidden block c: W1 x4, W2 x4
    constexpr int C0 = ST0 ? 0 : 4;
    constexpr int NEU = C0 + 43;                       // chunks of the edge update itself
    constexpr int NCH = NEU + (FUSE ? 11 : 0);         // + W_B x4, W_G x3, W_mid x4 of the next node message
#ifdef PP_X_TS
    const unsigned long long ts0 = __builtin_readcyclecounter();
    int tsv[24];
#endif
#if defined(PP_X_TS) && defined(PP_X_TS_FINE)
    const unsigned long long ts0f = __builtin_readcyclecounter();
    int tsf[16] = {0};
#endif
    HT bt[2][R];
    f32x16 acc[R], out[R];
    float *gbuf = x1buf;      // the geometry operands borrow the x1 buffer: dead until LayerNorm 2 and again after the FFN
    int nbr[R];
    float me[R];
    GeoI gi0[R];
    float pj[R][3];
#pragma unroll
    for (int r = 0; r < R; r++) {
        nbr[r] = A.eidx[(size_t)n[r] * K + jj];
        me[r] = A.mask_att[(size_t)n[r] * 32 + jj];            // (lanes j >= K mirror edge K - 1 throughout)
    }
    // the small per-layer vectors go to LDS once (published by the first barrier)
    constexpr int PRM_IT = (PARAM_LDS / 4 + ET - 1) / ET;
    f32x4v prv[PRM_IT], prg;
#pragma unroll
    for (int it = 0; it < PRM_IT; it++) prv[it] = *reinterpret_cast<const f32x4v *>(A.params + 4 * min(tid + it * ET, PARAM_LDS / 4 - 1));
    {
        const int t64 = min(tid, 63);
        prg = *reinterpret_cast<const f32x4v *>((t64 < 32 ? A.g3 + 4 * t64 : A.be3 + 4 * (t64 - 32)));
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        geo_load_i(A.pts + (size_t)n[r] * 48, A.frames + (size_t)n[r] * 12, h, wave, gi0[r]);
        load_tile(A.hE_in + ((size_t)n[r] * K + jj) * 128 + 32 * wave, h, out[r]);
    }
    PROLOGUE_PIPE(NCH)
#pragma unroll
    for (int r = 0; r < R; r++) geo_load_j(A.pts + (size_t)nbr[r] * 48, h, wave, pj[r]);
    TileQ pc[R], zt[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        load_tile(A.PA + (size_t)n[r] * 128 + 32 * wave, h, acc[r]);
        load_tile_q(A.PC + (size_t)nbr[r] * 128 + 32 * wave, h, pc[r]);
        if constexpr (ST0) load_tile_q(A.Z + ((size_t)n[r] * K + jj) * 128 + 32 * wave, h, zt[r]);
    }
#pragma unroll
    for (int it = 0; it < PRM_IT; it++) *reinterpret_cast<f32x4v *>(prm + 4 * min(tid + it * ET, PARAM_LDS / 4 - 1)) = prv[it];
    if (tid < 64) *reinterpret_cast<f32x4v *>(prm + PARAM_LDS + 4 * tid) = prg;
#pragma unroll
    for (int r = 0; r < R; r++) geometry_put(gi0[r], pj[r], wave, lane, gbuf + r * GBUF_FLOATS);
    if constexpr (!ST0) { PUBLISH_OPERAND(out, xbuf, A.ls_in) }
#pragma unroll
    for (int r = 0; r < R; r++) {
        add_tile_q(pc[r], acc[r]);
        if constexpr (ST0) add_tile_q(zt[r], acc[r]);
    }
    if constexpr (ST0) __syncthreads();   // geometry operands and parameters are in LDS (otherwise the first W_B stage's barrier says so)
    TS(0)
    FIRST_LAYER(0, NCH)
    TS(1)
    // ---- second layer (chunks C0 + 3 ..): barrier A in its last position, the third layer's input overwrites xbuf --------
#pragma unroll
    for (int r = 0; r < R; r++) load_tile(prm + P_BMID + 32 * wave, h, acc[r]);
    RLAYER_OWN(C0 + 3, NCH, acc, xbuf, false, true)
    TS(2)
    PUBLISH_OWN(true, acc, xbuf)
    TS(3)
    // ---- third layer (chunks C0 + 7 ..) -----------------------------------------------------------
#pragma unroll
    for (int r = 0; r < R; r++) load_tile(prm + P_BOUT + 32 * wave, h, acc[r]);
    RLAYER_OWN(C0 + 7, NCH, acc, xbuf, false, false)
    TS(4)
    // ---- x1 = LN2(h_E + mask * m): own tile only, statistics merged across the four waves ---------------
    f32x16 fib;
    FFN_BIAS_FETCH(0)
#pragma unroll
    for (int r = 0; r < R; r++) {
#pragma unroll
        for (int q = 0; q < 16; q++) out[r][q] = fmaf(acc[r][q], me[r], out[r][q]);
        ln_partial(out[r], stat + r * STAT_FLOATS, wave, j, h);
    }
    __syncthreads();
    TS(5)
#pragma unroll
    for (int r = 0; r < R; r++) {
        float mean;
        const float rstd = ln_merge(stat + r * STAT_FLOATS, j, mean);
#pragma unroll
        for (int q = 0; q < 16; q++) out[r][q] -= mean;
        ln_affine_tile(out[r], rstd, prm + P_G2 + 32 * wave, prm + P_BE2 + 32 * wave, h);
    }
    PUBLISH_OPERAND(out, x1buf, A.ls_x1)  // (x1buf last held the geometry operands: read before the barriers above)
    // `out` keeps x1 (this wave's tile, fp32) as the residual of the second LayerNorm and collects the FFN output
    // on top of it: out = x1 + b + W2 relu(W1 x1 + b1)
#pragma unroll
    for (int r = 0; r < R; r++) add_tile(prm + P_FOB + 32 * wave, h, out[r]);
    TS(6)
    // ---- FFN 128 -> 512 -> 128 in four hidden blocks of 128 ------------------------------------------
    FFN_BLOCK(0)
    TS(7)
    FFN_BLOCK(1)
    TS(8)
    FFN_BLOCK(2)
    TS(9)
    FFN_BLOCK(3)
    TS(10)
    // ---- h_E = mask * LN3(x1 + ffn) ---------------------------------------------------------------------
#pragma unroll
    for (int r = 0; r < R; r++) ln_partial(out[r], stat + r * STAT_FLOATS, wave, j, h);
    __syncthreads();
    TS(11)
#pragma unroll
    for (int r = 0; r < R; r++) {
        float mean3;
        const float rstd = ln_merge(stat + r * STAT_FLOATS, j, mean3);
#pragma unroll
        for (int q = 0; q < 16; q++) out[r][q] -= mean3;
        ln_affine_tile(out[r], rstd, prm + PARAM_LDS + 32 * wave, prm + PARAM_LDS + 128 + 32 * wave, h);
#pragma unroll
        for (int q = 0; q < 16; q++) out[r][q] *= me[r];
        // lanes j >= K mirror edge K - 1 (same inputs, same value): they store it again rather than being masked off
        if (WB && live[r]) store_tile(A.hE_out + ((size_t)n[r] * K + jj) * 128 + 32 * wave, h, out[r]);
    }
    TS(12)
    if constexpr (FUSE) {
        // ---- next layer's node message on the fresh edges ------------------------------------------------
        // (xbuf was last read by the W2 stages of FFN block 3, the geometry block = x1buf by its W1 stages: every wave
        //  has passed the LayerNorm barrier since)
        GeoI gi_[R];
        float pj2[R][3];
#pragma unroll
        for (int r = 0; r < R; r++) {
            asm volatile("" : "+v"(nbr[r]));      // the gather addresses are formed HERE, not hoisted to the prologue
            geo_load_i(A.pts2 + (size_t)n[r] * 48, A.frames + (size_t)n[r] * 12, h, wave, gi_[r]);
            geo_load_j(A.pts2 + (size_t)nbr[r] * 48, h, wave, pj2[r]);
            load_tile(A.PA2 + (size_t)n[r] * 128 + 32 * wave, h, acc[r]);
        }
        __builtin_amdgcn_sched_barrier(0);
        PUBLISH_OPERAND(out, xbuf, A.ls_out)
        __builtin_amdgcn_sched_barrier(0);
        TileQ pc2[R];
#pragma unroll
        for (int r = 0; r < R; r++) load_tile_q(A.PC2 + (size_t)nbr[r] * 128 + 32 * wave, h, pc2[r]);
#pragma unroll
        for (int r = 0; r < R; r++) geometry_put(gi_[r], pj2[r], wave, lane, gbuf + r * GBUF_FLOATS);
        const float bmid = A.b_mid2[32 * wave + j];           // SWAP form: feature on the lane
        TS(13)
        // the next message's first layer always has its W_B stages (the edges are fresh)
        RLAYER_OWN(NEU + 0, NCH, acc, xbuf, false, false)
        WSTAGE(NEU + 4, NCH, acc, (mfma_geo<R, 0>(AK, gbuf, lane, acc)))
        WSTAGE(NEU + 5, NCH, acc, (mfma_geo<R, 1>(AK, gbuf, lane, acc)))
        __syncthreads();                  // barrier A of the publication below
        WSTAGE(NEU + 6, NCH, acc, (mfma_geo<R, 2>(AK, gbuf, lane, acc)))
#pragma unroll
        for (int r = 0; r < R; r++) add_tile_q(pc2[r], acc[r]);
        TS(14)
        PUBLISH_OWN(true, acc, xbuf)
        f32x4v mmv[R][4];          // edge masks of the final reduction, requested a layer ahead (as in node_message_body)
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float *mrow = A.mask_att + (size_t)n[r] * 32 + 4 * h;
#pragma unroll
            for (int q = 0; q < 4; q++) mmv[r][q] = *reinterpret_cast<const f32x4v *>(mrow + 8 * q);
        }
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int q = 0; q < 16; q++) acc[r][q] = bmid;
        TS(15)
        RLAYER_OWN(NEU + 7, NCH, acc, xbuf, true, false)
        TS(16)
#pragma unroll
        for (int r = 0; r < R; r++) {
            // rows (registers) are edges e = 8 (r>>2) + 4 h + (r&3); mask and reduce over them
            float sacc = 0.f, ms = 0.f;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const f32x4v mm = mmv[r][q];
#pragma unroll
                for (int pq = 0; pq < 4; pq++) {
                    sacc = fmaf(fmaxf(acc[r][4 * q + pq], 0.f), mm[pq], sacc);
                    ms += mm[pq];
                }
            }
            sacc += __shfl_xor(sacc, 32);
            ms += __shfl_xor(ms, 32);
            if (live[r]) {
                if (h == 0) A.S[(size_t)n[r] * 128 + 32 * wave + j] = sacc * A.inv_K;
                if (tid == 0) A.msum[n[r]] = ms * A.inv_K;
            }
        }
    }
    if (pp_sat_hit(sat)) atomicOr(A.sat, 1u);
#ifdef PP_X_TS
    TS(17)
    if (A.dbg && tid == 0)
        for (int q = 0; q < 18; q++) A.dbg[(size_t)n[0] * 24 + q] = (float)tsv[q];
    if (A.dbg && tid == 0) A.dbg[(size_t)n[0] * 24 + 18] = (float)((ts0 >> 6) & 0xFFFFF);      // when the workgroup started, units of 64 cycles
#ifdef PP_X_TS_FINE
    if (A.dbg && tid == 0)
        for (int q = 0; q < 16; q++) A.dbg[(size_t)n[0] * 24 + q] = (float)tsf[q];
#endif
#endif
}

template <int R, bool ST0, bool FUSE, bool LNS = false, bool WB = true, bool LIVE = false>
__global__ void __launch_bounds__(ET, R == 1 ? PP_WGS : PP_WGS2)
k_edge_update(EdgeArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if constexpr (LIVE) {
        int2 lrow = {-1, -1};
        if constexpr (R == 2) lrow = *reinterpret_cast<const int2 *>(A.live_rows + 2 * blockIdx.x);
        else lrow.x = A.live_rows[blockIdx.x];
        if (lrow.x < 0) return;           // behind the end of the list (the launch is sized for all rows)
        edge_update_body<R, ST0, FUSE, LNS, WB, true>(A, 0, smem, lrow);
    } else {
        edge_update_body<R, ST0, FUSE, LNS, WB>(A, blockIdx.x * R, smem);
    }
}

// MIXED launch for one complex that fills the chip once (2 < residues per CU <= 3).  Every workgroup streams the layer's
// whole weight set through its CU's vector memory path (64 B/clk): with three one-residue workgroups per CU that is 2.8 MB
// per CU and launch, ~20 us -- longer than the matrix work (16 us).  Here a CU hosts TWO workgroups, one with two residues
// (each weight fetch feeds two accumulator chains) and one with one: the same three residues and the same MFMA work per CU
// for two passes of the stream instead of three.  Workgroups 0 .. n_pairs - 1 take residues (2 b, 2 b + 1), the others one
// residue each; in dispatch order the first half lands on distinct CUs, so a CU mostly gets one of each kind (placement is
// the hardware's choice: it only affects speed).  A residue's kind is a function of (index, N): results are reproducible.
// LIVE: workgroup b takes the one or two rows of A.live_mix[b] (k_live_rows deals the live rows out: the split between pair and
// one-row workgroups and their dispatch order are the table's).
template <bool ST0, bool FUSE, bool LNS = false, bool WB = true, bool LIVE = false>
__global__ void __launch_bounds__(ET, 2)
k_edge_update_mix(EdgeArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x;
    if constexpr (LIVE) {
        const int2 lrow = A.live_mix[b];
        if (lrow.x < 0) return;
        if (lrow.y >= 0) edge_update_body<2, ST0, FUSE, LNS, WB, true>(A, 0, smem, lrow);
        else edge_update_body<1, ST0, FUSE, LNS, WB, true>(A, 0, smem, lrow);
        return;
    }
    int pair = -1, single = -1;
    if (A.mix_mode == 2) {               // experiment: kinds interleaved in dispatch order
        const int ns = gridDim.x - A.n_pairs;
        if (b < 2 * ns) { if (b & 1) single = b >> 1; else pair = b >> 1; }
        else pair = b - ns;
    } else if (A.mix_mode == 3) {        // experiment: the one-residue workgroups first in dispatch order
        const int ns = gridDim.x - A.n_pairs;
        if (b < ns) single = b; else pair = b - ns;
    } else {
        if (b < A.n_pairs) pair = b; else single = b - A.n_pairs;
    }
    if (pair >= 0) edge_update_body<2, ST0, FUSE, LNS, WB>(A, 2 * pair, smem);
    else edge_update_body<1, ST0, FUSE, LNS, WB>(A, 2 * A.n_pairs + single, smem);
}

// the stand-alone node message (layer 0) with the same split of a CU's three residues: two weight passes instead of three
template <bool ST0>
__global__ void __launch_bounds__(ET, 2)
k_node_message_mix(EdgeArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x;
    const int ns = gridDim.x - A.n_pairs;
    if (A.mix_mode == 3) {               // the one-residue workgroups first in dispatch order
        if (b < ns) node_message_body<1, ST0>(A, 2 * A.n_pairs + b, smem);
        else node_message_body<2, ST0>(A, 2 * (b - ns), smem);
    } else {                             // the pairs first, as in k_edge_update_mix
        if (b < A.n_pairs) node_message_body<2, ST0>(A, 2 * b, smem);
        else node_message_body<1, ST0>(A, 2 * A.n_pairs + (b - A.n_pairs), smem);
    }
}

// ---------------------------------------------------------------------------------------------
// once per complex: Z_nm = W_B(node message, layer 0) h_E0 and Z_em = W_B(edge message, layer 0) h_E0.  h_E0 never
// changes during sampling, so the layer-0 kernels skip four of their stages and start from these tiles.
// ---------------------------------------------------------------------------------------------
template <bool LNS>
__global__ void __launch_bounds__(ET, 1)
k_edge_static(EdgeArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = 1;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int n = blockIdx.x;
    const int K = A.K;
    if (A.rmask[n] == 0.f) return;        // never read: the layer kernels leave masked residues early as well
    constexpr int NCH = 8;                // chunks: W_B(node message) x4, W_B(edge message) x4
#if defined(PP_X_TS) && defined(PP_X_TS_FINE)
    const unsigned long long ts0f = __builtin_readcyclecounter();
    int tsf[16] = {0};
#endif
    PROLOGUE_PIPE(NCH)
    HT x[1][4];
    f32x16 acc[1];
    const int jj = j < K ? j : K - 1;
    const float *hrow = A.hE_in + ((size_t)n * K + jj) * 128;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        load_tile(hrow + 32 * t, h, acc[0]);
        if constexpr (LNS) scale_tile(A.ls_in + 32 * t, h, acc[0], acc[0]);      // h_E0 times its operand scale (pp_rebalance.h)
        unsigned nosat = 0;
        split_tile<false>(acc[0], x[0][t], nosat);
    }
#pragma unroll
    for (int r = 0; r < 16; r++) acc[0][r] = 0.f;
    WSTAGE(0, NCH, acc, (mfma_x<1, 0, false>(AK, x, acc)))
    WSTAGE(1, NCH, acc, (mfma_x<1, 1, false>(AK, x, acc)))
    WSTAGE(2, NCH, acc, (mfma_x<1, 2, false>(AK, x, acc)))
    WSTAGE(3, NCH, acc, (mfma_x<1, 3, false>(AK, x, acc)))
    store_tile(A.Znm + ((size_t)n * K + jj) * 128 + 32 * wave, h, acc[0]);      // lanes j >= K mirror edge K - 1
#pragma unroll
    for (int r = 0; r < 16; r++) acc[0][r] = 0.f;
    WSTAGE(4, NCH, acc, (mfma_x<1, 0, false>(AK, x, acc)))
    WSTAGE(5, NCH, acc, (mfma_x<1, 1, false>(AK, x, acc)))
    WSTAGE(6, NCH, acc, (mfma_x<1, 2, false>(AK, x, acc)))
    WSTAGE(7, NCH, acc, (mfma_x<1, 3, false>(AK, x, acc)))
    store_tile(A.Zem + ((size_t)n * K + jj) * 128 + 32 * wave, h, acc[0]);
}

// ---------------------------------------------------------------------------------------------
// once per complex: edge features + embedding, h_E0 = LayerNorm(Linear(468 -> 128)(e_ij))  (encoder.py:105-246) -- the MFMA
// form of pp_prepare.hip's k_edge_embed (which the exact-fp32 build keeps): 0.25 ms -> see DESIGN.md.  One workgroup per
// residue.  The 400 RBF inputs (25 backbone atom pairs x 16 Gaussians) are written to LDS directly as split-f16 B operands
// -- k-step S = atom pair S, lane half h = Gaussians 8h .. 8h+7 -- and contracted on the matrix pipe against the packed RBF
// block of the weight (plan->embed_stream); the other 68 inputs (one-hot relative position = a column select, chain flag,
// two pair dihedrals) and the bias initialise the accumulator; LayerNorm as in the edge update.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float dist_eps_nc(const float *a, const float *b, float eps) {
#pragma clang fp contract(off)      // rounds like the reference's separate mul / add / sqrt (as in pp_prepare.hip)
    float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    float s = dx * dx;
    s = s + dy * dy;
    s = s + dz * dz;
    return sqrtf(s + eps);
}
// chunk C of the RBF block: k-steps (atom pairs) 2C and 2C+1 (the 26th is padding and skipped)
template <int C>
__device__ __forceinline__ void emb_step(const AOp &a, const float *gb, int lane, f32x16 &acc) {
#pragma unroll
    for (int s2 = 0; s2 < 2; s2++) {
        if (2 * C + s2 < 25) {
            const h8 *gp = reinterpret_cast<const h8 *>(gb) + (2 * (2 * C + s2)) * 64 + lane;
            const h8 bh = gp[0];
            const h8 bl = gp[64];
            acc = MFMA16(a.r[2 * s2], bh, acc);
            acc = MFMA16(a.r[2 * s2], bl, acc);
            acc = MFMA16(a.r[2 * s2 + 1], bh, acc);
        }
    }
}

struct EmbedArgs {
    int N, K;
    const float *bbpos;            // [N][15]  N, CA, C, O, virtual CB
    const int32_t *eidx;           // [N][K]
    const int64_t *res_index, *chain;
    const float *WT;               // [468][128] transposed weight (one-hot / flag / dihedral columns)
    const float *bias, *ln_g, *ln_b;
    const float *wstream;          // packed RBF block, 13 chunks
    float *hE0;                    // [N][K][128]
};
#define EMB_GB_FLOATS (25 * 2 * 64 * 4)      // 50 KB: [pair][hi | lo][lane] h8
__global__ void __launch_bounds__(ET, 2)
k_edge_embed_f16(EmbedArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *gb = smem, *stat = smem + EMB_GB_FLOATS;
    __shared__ float s_pos[33][15];                             // slot 32 = centre residue
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int n = blockIdx.x, K = A.K;
    const int jj = j < K ? j : K - 1;
    constexpr int R = 1;
    constexpr int NCH = 13;
#if defined(PP_X_TS) && defined(PP_X_TS_FINE)
    const unsigned long long ts0f = __builtin_readcyclecounter();
    int tsf[16] = {0};
#endif
    PROLOGUE_PIPE(NCH)
    for (int t = tid; t < 15; t += ET) s_pos[32][t] = A.bbpos[(size_t)n * 15 + t];
    for (int t = tid; t < 32 * 15; t += ET) {
        int e = t / 15, c = t - e * 15;
        int ee = e < K ? e : K - 1;                              // slots >= K mirror edge K - 1
        s_pos[e][c] = A.bbpos[(size_t)A.eidx[(size_t)n * K + ee] * 15 + c];
    }
    __syncthreads();
    // 25 atom-pair distances -> 16 Gaussians each (centre atom a major, neighbour atom b minor), as operands
    for (int item = tid; item < 32 * 25 * 2; item += ET) {
        const int hh = item & 1, e = (item >> 1) & 31, pr = item >> 6;
        const int a = pr / 5, bq = pr - a * 5;
        const float dd = dist_eps_nc(&s_pos[32][3 * a], &s_pos[e][3 * bq], 1e-6f);
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            // torch.linspace(0, 20, 16): ascending from the start below the midpoint, descending from the end above it
            const float step = 20.0f / 15.0f;
            const int r = 8 * hh + i;
            const float mu = (r < 8) ? step * (float)r : 20.0f - step * (float)(15 - r);
            const float z = (dd - mu) / 1.25f;
            v[i] = expf(-(z * z));
        }
        h8 vh, vl;
#pragma unroll
        for (int i = 0; i < 8; i += 2) {
            const f32x2v x = {v[i], v[i + 1]};
            const h2v hi2 = cvt2(x);
            const f32x2v d = {fmaf((float)hi2[0], -1.0f, x[0]), fmaf((float)hi2[1], -1.0f, x[1])};
            const h2v lo2 = cvt2(d);
            vh[i] = hi2[0]; vh[i + 1] = hi2[1];
            vl[i] = lo2[0]; vl[i + 1] = lo2[1];
        }
        h8 *gp = reinterpret_cast<h8 *>(gb) + (2 * pr) * 64 + e + 32 * hh;
        gp[0] = vh;
        gp[64] = vl;
    }
    // accumulator init: bias + the 68 non-RBF inputs of this lane's edge
    f32x16 acc[1];
    {
        const int jn = A.eidx[(size_t)n * K + jj];
        long off = (long)(A.res_index[n] - A.res_index[jn]) + 32;
        off = off < 0 ? 0 : (off > 64 ? 64 : off);
        const float etype = (A.chain[n] == A.chain[jn]) ? 2.f : 1.f;
        // phi_ij = dih(C_i, N_j, CA_j, C_j), psi_ij = dih(N_i, CA_i, C_i, N_j), rounded as the reference rounds them
        // (pp_internal.h); the j == i edge included: its values are the reference's own arccos rounding noise
        const float phi = pp_pair_dihedral_t(&s_pos[32][6], &s_pos[j][0], &s_pos[j][3], &s_pos[j][6]);
        const float psi = pp_pair_dihedral_t(&s_pos[32][0], &s_pos[32][3], &s_pos[32][6], &s_pos[j][0]);
        load_tile(A.bias + 32 * wave, h, acc[0]);
        add_tile(A.WT + (size_t)off * 128 + 32 * wave, h, acc[0]);
        f32x16 w;
        load_tile(A.WT + (size_t)465 * 128 + 32 * wave, h, w);
#pragma unroll
        for (int q = 0; q < 16; q++) acc[0][q] = fmaf(w[q], etype, acc[0][q]);
        load_tile(A.WT + (size_t)466 * 128 + 32 * wave, h, w);
#pragma unroll
        for (int q = 0; q < 16; q++) acc[0][q] = fmaf(w[q], phi, acc[0][q]);
        load_tile(A.WT + (size_t)467 * 128 + 32 * wave, h, w);
#pragma unroll
        for (int q = 0; q < 16; q++) acc[0][q] = fmaf(w[q], psi, acc[0][q]);
    }
    __syncthreads();
#define EMB_STAGE(c) WSTAGE(c, NCH, acc, (emb_step<c>(AK, gb, lane, acc[0])))
    EMB_STAGE(0) EMB_STAGE(1) EMB_STAGE(2) EMB_STAGE(3) EMB_STAGE(4) EMB_STAGE(5) EMB_STAGE(6)
    EMB_STAGE(7) EMB_STAGE(8) EMB_STAGE(9) EMB_STAGE(10) EMB_STAGE(11) EMB_STAGE(12)
#undef EMB_STAGE
    ln_partial(acc[0], stat, wave, j, h);
    __syncthreads();
    float mean;
    const float rstd = ln_merge(stat, j, mean);
#pragma unroll
    for (int q = 0; q < 16; q++) acc[0][q] -= mean;
    ln_affine_tile(acc[0], rstd, A.ln_g + 32 * wave, A.ln_b + 32 * wave, h);
    store_tile(A.hE0 + ((size_t)n * K + jj) * 128 + 32 * wave, h, acc[0]);       // lanes j >= K mirror edge K - 1
}
static const size_t EMB_SMEM = (EMB_GB_FLOATS + STAT_FLOATS) * sizeof(float);
pp_status pp_launch_edge_embed_f16(pp_ctx *c, hipStream_t s) {
    static bool attr_done = false;
    if (!attr_done) {
        PP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_edge_embed_f16),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)EMB_SMEM));
        attr_done = true;
    }
    const pp_plan *p = c->plan;
    EmbedArgs A;
    A.N = c->N; A.K = c->K;
    A.bbpos = c->bbpos; A.eidx = c->eidx; A.res_index = c->b.residue_index; A.chain = c->b.chain_indices;
    A.WT = p->edge_emb_T; A.bias = p->w + p->off.edge_emb_b;
    A.ln_g = p->w + p->off.norm_edges_g; A.ln_b = p->w + p->off.norm_edges_b;
    A.wstream = p->embed_stream; A.hE0 = c->hE0;
    hipLaunchKernelGGL(k_edge_embed_f16, dim3(c->N), dim3(ET), EMB_SMEM, s, A);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

static float *g_dbg = nullptr;
#ifdef PP_DIAG
extern "C" void pp_debug_set_dbg(float *p) { g_dbg = p; }
#endif
static EdgeArgs edge_args(pp_ctx *c, int layer, bool edge) {
    const pp_plan *p = c->plan;
    const LayerOff &o = p->off.layer[layer];
    EdgeArgs A;
    A.N = c->N; A.K = c->K; A.inv_K = 1.0f / (float)c->K;
    A.n_pairs = 0;
    A.mix_mode = 0;
    A.rmask = c->b.residue_mask;
    A.eidx = c->eidx; A.mask_att = c->mask_att; A.frames = c->frames;
    A.pts = edge ? c->ptsE : c->ptsN;
    A.PA = edge ? c->PAe : c->PAn;
    A.PC = edge ? c->PCe : c->PCn;
    A.hE_in = layer == 0 ? c->hE0 : c->hE;
    A.hE_out = c->hE;
    A.S = c->S; A.msum = c->msum;
    A.wstream = edge ? p->lt[layer].em_stream : p->lt[layer].nm_stream;
    A.params = p->lt[layer].em_params;
    A.g3 = p->w + o.norm_g[3]; A.be3 = p->w + o.norm_b[3];
    A.b_mid = p->w + o.nm_mid_b;
    A.Z = edge ? c->Zem : c->Znm;
    A.Znm = c->Znm; A.Zem = c->Zem;
    A.pts2 = c->ptsN; A.PA2 = c->PAn; A.PC2 = c->PCn;
    A.b_mid2 = p->w + p->off.layer[layer < 2 ? layer + 1 : 2].nm_mid_b;
    A.dbg = g_dbg;
    A.sat = c->sat;
    // operand scales behind small LayerNorm gains (null: the plan has none and the default instances run)
    const float *ls = p->ln_scale;
    A.ls_in = ls ? ls + 128 * (layer == 0 ? PP_LN_E0 : PP_LN_E(layer - 1)) : nullptr;
    A.ls_x1 = ls ? ls + 128 * PP_LN_X1(layer < 2 ? layer : 1) : nullptr;
    A.ls_out = ls ? ls + 128 * PP_LN_E(layer < 2 ? layer : 1) : nullptr;
    return A;
}

#ifdef PP_NO_FUSE_NM
#define PP_FUSED false
#else
#define PP_FUSED true
#endif
#define PP_RMAX 2

// one workgroup per CU: the request is padded beyond half of the CU's 160 KB (the kernels need R x 16 KB + 4.5 KB)
#ifndef PP_LDS_PAD
#define PP_LDS_PAD 0           // > 80 KB forces one workgroup per CU (occupancy experiments)
#endif
static size_t g_lds_pad = PP_LDS_PAD;     // pp_debug_set_lds_pad(): occupancy experiments
#ifdef PP_DIAG
extern "C" void pp_debug_set_lds_pad(int bytes) { g_lds_pad = (size_t)bytes; }
#endif
static size_t pad_smem(size_t b) { return b > g_lds_pad ? b : g_lds_pad; }
static size_t nm_smem(int R) { return pad_smem((R * XBUF_FLOATS + R * GBUF_FLOATS) * sizeof(float)); }
static size_t eu_smem(int R) {
    return pad_smem((2 * R * XBUF_FLOATS + R * STAT_FLOATS + PARAM_LDS + 256) * sizeof(float));
}
#define ST_SMEM pad_smem(0)
#define MAX_SMEM (160 * 1024)

typedef void (*edge_kernel_t)(EdgeArgs);
template <int R> static edge_kernel_t nm_kernel(bool st0) {
    return st0 ? k_node_message<R, true> : k_node_message<R, false>;
}
// wb = false selects the instances without the h_E write-back.  They exist for layer 1 only (ST0 = false): layer 0's h_E is
// the next layer's input, so its launch always stores.
// live = true (with wb = false, layer 1) selects the instances that take their rows from the live-row list.
template <int R> static edge_kernel_t eu_kernel(bool st0, bool lns, bool wb, bool live = false) {
    if (live) return lns ? k_edge_update<R, false, PP_FUSED, true, false, true> : k_edge_update<R, false, PP_FUSED, false, false, true>;
    if (!wb && !st0) return lns ? k_edge_update<R, false, PP_FUSED, true, false> : k_edge_update<R, false, PP_FUSED, false, false>;
    if (lns) return st0 ? k_edge_update<R, true, PP_FUSED, true> : k_edge_update<R, false, PP_FUSED, true>;
    return st0 ? k_edge_update<R, true, PP_FUSED> : k_edge_update<R, false, PP_FUSED>;
}
static edge_kernel_t mix_kernel(bool st0, bool lns, bool wb, bool live = false) {
    if (live) return lns ? k_edge_update_mix<false, PP_FUSED, true, false, true> : k_edge_update_mix<false, PP_FUSED, false, false, true>;
    if (!wb && !st0) return lns ? k_edge_update_mix<false, PP_FUSED, true, false> : k_edge_update_mix<false, PP_FUSED, false, false>;
    if (lns) return st0 ? k_edge_update_mix<true, PP_FUSED, true> : k_edge_update_mix<false, PP_FUSED, true>;
    return st0 ? k_edge_update_mix<true, PP_FUSED> : k_edge_update_mix<false, PP_FUSED>;
}

static edge_kernel_t nm_kernel_r(int R, bool st0) {
    return R == 1 ? nm_kernel<1>(st0) : nm_kernel<2>(st0);
}
static edge_kernel_t eu_kernel_r(int R, bool st0, bool lns = false, bool wb = true, bool live = false) {
    return R == 1 ? eu_kernel<1>(st0, lns, wb, live) : eu_kernel<2>(st0, lns, wb, live);
}


static int g_num_cu = 0;
static bool edge_attrs() {
    static bool done = false, ok = false;
    if (!done) {
        done = true;
        auto set = [](const void *f, size_t bytes) {
            return hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
        };
        ok = set(reinterpret_cast<const void *>(k_edge_static<false>), MAX_SMEM) && set(reinterpret_cast<const void *>(k_edge_static<true>), MAX_SMEM);
        for (int R = 1; R <= PP_RMAX && ok; R++)
            for (int st0 = 0; st0 < 2 && ok; st0++)
                ok = set(reinterpret_cast<const void *>(nm_kernel_r(R, st0)), MAX_SMEM) &&
                     set(reinterpret_cast<const void *>(eu_kernel_r(R, st0, false, true)), MAX_SMEM) &&
                     set(reinterpret_cast<const void *>(eu_kernel_r(R, st0, true, true)), MAX_SMEM) &&
                     set(reinterpret_cast<const void *>(eu_kernel_r(R, st0, false, false)), MAX_SMEM) &&
                     set(reinterpret_cast<const void *>(eu_kernel_r(R, st0, true, false)), MAX_SMEM);
        for (int R = 1; R <= PP_RMAX && ok; R++)
            for (int lns = 0; lns < 2 && ok; lns++)
                ok = set(reinterpret_cast<const void *>(eu_kernel_r(R, false, lns, false, true)), MAX_SMEM);
        for (int lns = 0; lns < 2 && ok; lns++) ok = set(reinterpret_cast<const void *>(mix_kernel(false, lns, false, true)), MAX_SMEM);
        for (int st0 = 0; st0 < 2 && ok; st0++)
            for (int lns = 0; lns < 2 && ok; lns++)
                ok = set(reinterpret_cast<const void *>(mix_kernel(st0, lns, true)), MAX_SMEM) &&
                     set(reinterpret_cast<const void *>(mix_kernel(st0, lns, false)), MAX_SMEM);
        ok = ok && set(reinterpret_cast<const void *>(k_node_message_mix<true>), MAX_SMEM) &&
             set(reinterpret_cast<const void *>(k_node_message_mix<false>), MAX_SMEM);
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            g_num_cu = prop.multiProcessorCount;
        if (g_num_cu <= 0) g_num_cu = 256;
    }
    return ok;
}

// Residues per workgroup: 1 (two such workgroups share a CU: 223 VGPRs).  R = 2 -- two interleaved accumulator chains per
// weight fetch, 458 registers, one workgroup per CU -- is kept for the structural test (tests/test_hip_parity.py) and
// measurements (PP_EDGE_R=2 / pp_debug_set_edge_R): it was the better choice for multi-round sizes while the kernels were
// confined to one wave per SIMD, and lost to two co-resident R = 1 workgroups on every workload once they were not
// (T1124 32.8 vs 42.4 k residues/s, S1500 41.5 vs 46.6, C5 shard 43.5 vs 51.0).
static int g_forced_R = -1;
#ifdef PP_DIAG
extern "C" void pp_debug_set_edge_R(int R) { g_forced_R = R; }
#endif
static int pick_R(int N) {
    if (g_forced_R < 0) {
        const char *e = PP_GETENV("PP_EDGE_R");
        g_forced_R = e ? atoi(e) : 0;
    }
    if (g_forced_R >= 1 && g_forced_R <= PP_RMAX) return g_forced_R;
    return N > PP_WGS * g_num_cu ? 2 : 1;
}

// mixed launch (k_edge_update_mix): when one-residue workgroups would sit three to a CU in a single round
static int g_mix = -1;
static bool use_mix(int N) {
    if (g_mix < 0) {
        const char *e = PP_GETENV("PP_EDGE_MIX");
        // 1: the pairs first in dispatch order, in the edge update and in the node message (re-measured behind the live rows: 1.3 % of
        // a T1124 pass over 3, the one-residue workgroups first, which round 4 had found better by 0.5-1 %)
        g_mix = e ? atoi(e) : 1;
    }
    if (g_forced_R >= 1 || !g_mix) return false;
    return N > 2 * g_num_cu && N <= 3 * g_num_cu;
}
// its two-residue workgroups: residues (2 b, 2 b + 1) for b < mix_pairs(N), the remaining N - 2 mix_pairs(N) get one workgroup each
// (the launch-shape rule's count for this regime, pp_internal.h pp_edge_shape: (N + 2) / 3)
static int mix_pairs(int N) { return pp_edge_shape(N, g_num_cu, PP_WGS2).pairs; }
// the live-row launch is the mixed one in both mixed regimes of the rule: the one above and 2 slots < N <= 3 slots rows, where the
// all-rows launches stay two-row launches
static bool use_live_mix(int N) {
    (void)use_mix(N);      // (reads PP_EDGE_MIX once)
    return g_forced_R < 1 && g_mix && pp_live_mix_size(N, g_num_cu, PP_WGS2);
}

// resident workgroups per CU the runtime predicts for the two kernels (measurement aid)
void pp_edge_occupancy(int *node_msg, int *edge_upd) {
    edge_attrs();
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(node_msg, reinterpret_cast<const void *>(nm_kernel_r(1, false)), ET, nm_smem(1));
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(edge_upd, reinterpret_cast<const void *>(eu_kernel_r(1, false)), ET, eu_smem(1));
}

#define EDGE_ATTR_CHECK()                                                                                   \
    if (!edge_attrs()) {                                                                                    \
        pp_set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for the edge kernels");        \
        return PP_ERR_HIP;                                                                                  \
    }

pp_status pp_launch_edge_static(pp_ctx *c, hipStream_t s) {
    EDGE_ATTR_CHECK()
    EdgeArgs A = edge_args(c, 0, false);
    A.wstream = c->plan->static_stream;
    if (c->plan->ln_scale) hipLaunchKernelGGL(k_edge_static<true>, dim3(c->N), dim3(ET), ST_SMEM, s, A);
    else hipLaunchKernelGGL(k_edge_static<false>, dim3(c->N), dim3(ET), ST_SMEM, s, A);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

pp_status pp_launch_node_message(pp_ctx *c, int layer, hipStream_t s) {
    EDGE_ATTR_CHECK()
    EdgeArgs A = edge_args(c, layer, false);
    static const char *nm_env = PP_GETENV("PP_NM_R");
    static const int nm_R = nm_env ? atoi(nm_env) : 0;       // measurement aid: residues per workgroup of this kernel only
    const int R = (nm_R >= 1 && nm_R <= PP_RMAX) ? nm_R : pick_R(c->N);
    static const char *nmix_env = PP_GETENV("PP_NM_MIX");
    static const bool nmix = !(nmix_env && atoi(nmix_env) == 0);
    if (nmix && !(nm_R >= 1 && nm_R <= PP_RMAX) && use_mix(c->N)) {
        A.n_pairs = mix_pairs(c->N);
        A.mix_mode = g_mix;
        const int singles = c->N - 2 * A.n_pairs > 0 ? c->N - 2 * A.n_pairs : 0;
        PP_LAUNCH(c, (layer == 0 ? k_node_message_mix<true> : k_node_message_mix<false>), dim3(A.n_pairs + singles), dim3(ET),
                  nm_smem(2), s, A);
        PP_HIP_CHECK(hipGetLastError());
        return PP_OK;
    }
    PP_LAUNCH(c, nm_kernel_r(R, layer == 0), dim3((c->N + R - 1) / R), dim3(ET), nm_smem(R), s, A);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

#ifdef PP_DIAG
// pp_debug_launch_plan: what the edge update and the node message of N rows would launch
pp_status pp_edge_launch_plan(int N, int *R, int *mixed, int *n_pairs) {
    EDGE_ATTR_CHECK()
    *mixed = use_mix(N) ? 1 : 0;
    *R = pick_R(N);
    *n_pairs = *mixed ? mix_pairs(N) : 0;
    return PP_OK;
}
#endif

// true when k_edge_update also computes the next layer's node message
extern "C" int pp_edge_variant(void) { return 1; }
bool pp_edge_fused() { return PP_FUSED; }

// layers 0 and 1 only (the reference's layer-2 edge update is dead code); keep_hE = false skips the h_E write-back of a
// layer-1 launch (layer 0 always stores: layer 1 reads it)
pp_status pp_launch_edge_update(pp_ctx *c, int layer, bool keep_hE, hipStream_t s, const PPLive *live) {
    EDGE_ATTR_CHECK()
    if (layer < 0 || layer > 1) { pp_set_error("pp_launch_edge_update: layer must be 0 or 1"); return PP_ERR_INVALID; }
    if (live && (layer != 1 || keep_hE || !PP_FUSED)) { pp_set_error("pp_launch_edge_update: the live-row launch is layer 1's, without write-back"); return PP_ERR_INVALID; }
    EdgeArgs A = edge_args(c, layer, true);
    const int R = pick_R(c->N);
    const bool mixed = live ? use_live_mix(c->N) : use_mix(c->N);
    if (live) {                     // (the slot of rmask)
        // the table is filled by pp_launch_live_rows for the sizes it expects the mixed launch at: never launch on one it did not fill
        if (mixed && !live->mix) { pp_set_error("pp_launch_edge_update: the mixed launch has no live-row work table for this context"); return PP_ERR_INVALID; }
        if (mixed) A.live_mix = live->mix;
        else A.live_rows = live->rows;
    }
    const bool lns = c->plan->ln_scale != nullptr;      // operand scales behind small LayerNorm gains: the LNS instances
    if (lns && !PP_FUSED) { pp_set_error("pp_launch_edge_update: a plan with LayerNorm operand scales needs the fused build"); return PP_ERR_UNSUPPORTED; }
    if (mixed) {
        // three residues per CU as one two-residue and one one-residue workgroup
        A.n_pairs = live ? 0 : mix_pairs(c->N);      // (the live instances read the table, not n_pairs)
        A.mix_mode = g_mix;
        const int singles = c->N - 2 * A.n_pairs > 0 ? c->N - 2 * A.n_pairs : 0;
        // live rows: the table deals the M <= N live rows out by the launch-shape rule (k_live_rows); the grid is the rule's worst
        // case over M, the surplus workgroups read (-1, -1) and leave
        const int wgs = live ? pp_live_mix_grid(c->N, g_num_cu, PP_WGS2) : A.n_pairs + singles;
        PP_LAUNCH(c, mix_kernel(layer == 0, lns, keep_hE, live != nullptr), dim3(wgs), dim3(ET), eu_smem(2) > eu_smem(1) ? eu_smem(2) : eu_smem(1), s, A);
        PP_HIP_CHECK(hipGetLastError());
        return PP_OK;
    }
    PP_LAUNCH(c, eu_kernel_r(R, layer == 0, lns, keep_hE, live != nullptr), dim3((c->N + R - 1) / R), dim3(ET), eu_smem(R), s, A);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
