// Internal declarations shared by the HIP translation units of libpackppi_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cmath>
#include <vector>
#include <mutex>
#include <stdint.h>
#include <string>

#include "../../include/packppi_hip.h"

// ---- product vs laboratory ------------------------------------------------------------------------------------------
// Five measurement switches are left in the sources, all in pp_edge_f16.hip, all behind -DPP_LAB and a TAGGED library:
//   -DPP_X_TS [-DPP_X_TS_FINE=k0]  phase / stage clocks of wave 0 into the dbg buffer (tools/debug/phase_*.py, stage_times.py);
//   -DPP_X_NOWLOAD, -DPP_X_E_NOMFMA  ablations (WRONG RESULTS): no weight fetches / no matrix instructions -- what the launch time
//                                    is made of (profiles/r02_edge_ablation.txt);
//   -DPP_X_NOSAT                   no sticky-flag bookkeeping (A/B of its price, tools/debug/ab_sat.sh).
// The switches of experiments that are settled (node-update stop points and ablations, wave priorities, conversion variants,
// the clash ablations ...) were removed from the sources in round 5 -- the device code of all four libraries is the same to the
// instruction (profiles/r05_switch_cleanup.txt); the builds behind the older records are in the history (up to 5cba218).
//   -DPP_LAB   is required by every PP_X_* switch and by the tuning parameters below;
//   -DPP_DIAG  (implied by PP_LAB; the libpackppi_hip.dbg.so build) compiles the pp_debug_* exports and the getenv switches
//              of the launchers (PP_NU_SPLIT, PP_EDGE_MIX, PP_EDGE_R, PP_NM_R, PP_NM_MIX, PP_NODE_F16, PP_DEBUG): same kernels, same
//              results, forced launch shapes -- the default / .f32 / .chk libraries have neither.
// packppi_amd/build.py refuses these flags for the three product libraries and lib.load() refuses a library whose flag
// stamp is not one of the known sets.
#if defined(PP_LAB) && !defined(PP_DIAG)
#define PP_DIAG
#endif
#if !defined(PP_LAB) &&                                                                                                       \
    (defined(PP_X_TS) || defined(PP_X_TS_FINE) || defined(PP_X_NOWLOAD) || defined(PP_X_E_NOMFMA) || defined(PP_X_NOSAT) ||      \
     defined(PP_WDEPTH) || defined(PP_WDEPTH_R1) || defined(PP_NXB_R1) || defined(PP_WGS2) || defined(PP_WGS) ||                 \
     defined(PP_NM_WGS2) ||                                                                                                  \
     defined(PP_LDS_PAD) || defined(PP_NO_FUSE_NM) || defined(PP_NU_DEPTH))
#error "PP_X_* / tuning switches compile laboratory variants (most give wrong results): add -DPP_LAB and build a TAGGED library (python -m packppi_amd.build --tag NAME -DPP_LAB -DPP_X_...)"
#endif
#ifdef PP_DIAG
#define PP_GETENV(name) getenv(name)
#else
#define PP_GETENV(name) ((const char *)nullptr)      /* product builds read no environment switches */
#endif

#define PP_H 128          // hidden width
#define PP_MSG_IN 456     // message MLP input width
#define PP_NPTS 8         // invariant points per node
#define PP_PROX_CHUNK 64   // proximal steps whose loss terms are parked before one reduction
#define PP_CL_CAP 96       // static clash-partner candidates kept per (residue, wave) -- k_clash_cand / k_clash<true>
#define PP_OB_CAP PP_OBSTACLE_CAP      // static obstacle candidates kept per residue -- k_obst_cand / k_clash<CAND, FUSE, true> (include/packppi_hip.h)

#include "pp_weights.h"      // LayerOff / WeightOff / pp_weight_offsets(): offsets into the concatenated weight buffer
#include "pp_rng.h"          // Philox4x32-10 and the normal transform of the seeded sampling noise (counter layout there)
#include "pp_segments.h"     // pp_seg_of_row / pp_seg_rows / pp_group_rows: the arithmetic of the context's segment table (pp_ctx::seg_off)

// Transposed ([in][out]) copies used by the node-level (VALU) kernels, per layer.
struct LayerT {
    const float *pts_node_wT, *pts_edge_wT;          // [128][24]
    const float *nm_A_T, *nm_C_T, *em_A_T, *em_C_T;  // W_in[:, 0:128]^T, W_in[:, 256:384]^T  -> [128][128]
    const float *nm_out_T;                           // [128][128]
    const float *nd_in_T;                            // [128][512]
    const float *nd_out_T;                           // [512][128]
    const float *nm_stream, *em_stream;              // MFMA weight chunks packed in consumption order (pp_pack.h put_stream)
    const float *em_params;                          // edge kernel small vectors, one block
    const float *nu_stream;                          // k_node_update: split-f16 weight slots, [wave][slot] (pp_pack.h put_node_stream)
    const float *nu_params;                          // k_node_update: small per-layer vectors, one block (NU_P_* offsets)
};

// ---- k_node_update (pp_node.hip): packed weight stream and parameter block ---------------------------------------
// One slot = the A operand of one (16-feature tile, 32-deep k-step) of v_mfma_f32_16x16x32_f16 as split f16:
// [hi | lo * 2^11][lane 64][8 halves] = 2 KB; a wave's slots are contiguous in the order it consumes them.
// Layers 0 and 1 use the MID list (next = this layer's edge message + the next layer's node message), layer 2 the LAST
// list (decoder + the layer-0 node-message inputs of the next step).
#define PP_NU_WAVES 8
#define PP_NU_SLOT_FLOATS 512
#define PP_NU_SLOTS_MID 56     // W_out 4 | FFN-in 16 | FFN-out 16 | PAe 4 | PCe 4 | PAn 4 | PCn 4 | pts 4 (waves 0-2)
#define PP_NU_SLOTS_LAST 59    // W_out 4 | FFN-in 16 | FFN-out 16 | D1 4 (waves 0-3) | D2 4, D3 1, D4 1 (wave 0) | embed 1 | PAn 4 | PCn 4 | pts 4 (waves 0-1)
#define PP_NU_LO_SCALE 2048.0f
enum {
    NU_P_OUTB = 0, NU_P_G0 = 128, NU_P_B0 = 256, NU_P_FIB = 384, NU_P_FOB = 896, NU_P_G1 = 1024, NU_P_B1 = 1152,
    // MID
    NU_P_PAE_B = 1280, NU_P_PAN_B = 1408, NU_P_PTS_B = 1536, NU_P_MID_TOTAL = 1600,
    // LAST
    NU_P_DB0 = 1280, NU_P_DB1 = 1344, NU_P_DB2 = 1376, NU_P_DB3 = 1392, NU_P_PAN0_B = 1408, NU_P_PTS0_B = 1536,
    NU_P_EMB_B = 1568, NU_P_EMB_G = 1696, NU_P_EMB_BETA = 1824, NU_P_LAST_TOTAL = 1952
};

struct ArenaSlot {
    void *p;
    size_t bytes;
    hipStream_t stream;      // work on this stream may still be using the memory
};
struct pp_plan {
    int device;
    std::vector<ArenaSlot> arena_pool;   // workspaces of destroyed contexts, reused by the next pp_complex_prepare
    std::mutex pool_mutex;
    bool has_network;         // false: geometry-only plan (atom14 / clash / proximal)
    int knn_ties;             // PP_KNN_TIES_*: what the neighbour search does on exactly equal distances
    float annealed_temp;      // sample_cfg.annealed_temp (the T of schedule.py:205-208), default 3
    int rebalanced_chains;    // split-f16 build: ReLU chains whose layers were rescaled by a power of two (pp_rebalance.h rebalance_relu_chains)
    float *ln_scale = nullptr;       // split-f16 build: [5][128] power-of-two operand scales behind small LayerNorm gains (pp_rebalance.h), or null
    int ln_scaled_features = 0;      // ... how many of them differ from 1
    float *w;                 // device copy of all weights, original layouts
    WeightOff off;
    float *wT;                // device arena of transposed copies
    LayerT lt[3];
    const float *node_emb_T;  // [51][128]
    const float *edge_emb_T;  // [468][128]
    const float *d0_in_T, *d0_out_T, *d2_in_T, *d2_out_T;   // [128][64] [64][32] [32][16] [16][4]
    const float *static_stream;                             // k_edge_static: W_B chunks of layer 0 (node, edge message)
    const float *embed_stream;                              // split-f16 build: the 400 RBF columns of the edge embedding, 13 chunks
    // chemistry tables (device)
    float *default_frames;    // [21][8][16]
    int32_t *atom14_to_group; // [21][14]
    float *atom14_mask;       // [21][14]
    float *lit_positions;     // [21][14][3]
    float *between_radius;    // [21][14]
    float *side_extent;       // [21] upper bound of |side-chain atom - CA| over all chi, per residue type (pp_api.hip side_chain_extents)
    float *bounds_lower, *bounds_upper;   // [21][14][14]
    float clash_tol;
    bool clash_params_set;
    int num_cu = 0;           // compute units of the device (which context sizes take the mixed edge launch and its live-row table)
};

// log sigma_min, log sigma_max of t_to_sigma (schedule.py:165-174; sigma from 0.01 pi to pi) in fp64: sigma(t), the step scalars
// and the loss round them to fp32 the same way, (float)lo + (float)(hi - lo) * t
#define PP_PI_D 3.14159265358979323846
static inline double pp_log_sigma_min() { return log(0.01 * PP_PI_D); }
static inline double pp_log_sigma_max() { return log(PP_PI_D); }

// Per-step scalars of the reverse process, computed on the host (schedule.py:198-235) and handed to the kernels as arguments.
struct StepParams {
    float temb[16];     // sinusoidal embedding of t
    float c_ode;        // 0.5 * g^2 * dt
    float w;            // annealed weight
    float c_drift;      // g^2 * dt        (sde)
    float c_diff;       // g * sqrt(dt)    (sde)
    float pad[12];
};

// Lazy workspaces: ONE allocation each outside the arena, made by the first call of its entry on a context (hipMalloc may wait for
// the device: no other call pays for it), kept for the later ones, freed with the context.  Each is sized from N (pp_hnet_optimize:
// and the segment count), which never change on a context, so the first call's allocation fits every later one.
enum {
    PP_WS_DISULFIDE,          // pp_disulfide_close: tables of the eligible rows, candidate list
    PP_WS_POLAR,              // pp_polar: [N][14] position + class, [N][14] direction, [N] row sphere
    PP_WS_ALLATOM,            // pp_clashscore: [N][27] position + radius, [N] row sphere, [N][27] class + separations
    PP_WS_HNET,               // pp_hnet_optimize: current atoms, rotor candidates, mover and partner lists, per-sweep counters
    PP_WS_REFINE,             // pp_chi_refine: the candidate angle and coordinate sets, current atoms, mover and partner lists, counters
    PP_WS_ANCHOR,             // pp_anchor_close: the rows' anchor lists, marks, the list of anchored rows, validity of the entries
    PP_WS_COUNT
};
struct pp_workspace {
    void *p = nullptr;
    size_t bytes = 0;
};

struct pp_ctx {
    pp_plan *plan;
    pp_batch b;               // caller-owned device pointers
    int B, L, K, N;           // B complexes, L = the longest, N rows: a padded batch [B][L] (N = B*L) or, packed, the sum of lengths
    bool packed = false;      // rows of the complexes back to back, no padding rows (pp_complex_prepare_packed).  Read only for what
                              // differs by creation: which contexts the proximal exports take and what their workspaces hold
    int shortest = 0;         // the shortest complex: the caller's min_len (padded: L)
    int32_t *seg_off;         // [B + 1] THE segment table: the first row of every complex, then N (pp_segments.h).  Packed: a copy
                              // of the caller's; padded: 0, L, 2L ...  Everything per complex reads it; no consumer forks on `packed`
    int2 *seg;                // [N] (first row, length) of the complex each row belongs to, made from seg_off (k_fill_seg)
    // static per complex
    int32_t *eidx;            // [N][K] global node index of each neighbour
    float *mask_att;          // [N][32] mask_i*mask_j (0 for slots >= K)
    float *frames;            // [N][12]  R (row-major 9) | t (3)
    float *bbpos;             // [N][5][3] N CA C O CB*
    float *hE0;               // [N][K][128]
    float *Znm, *Zem;         // [N][K][128] W_B h_E0 of layer 0's node / edge message (k_edge_static)
    // per-evaluation state
    float *hE;                // [N][K][128]
    float *hV;                // [N][128]
    float *hV_alt;            // [N][128] the split node-update launches write the new h_V here, then the two pointers swap
    float *S;                 // [N][128]  masked mean of the node-message hidden layer
    float *msum;              // [N]
    float *ptsN, *PAn, *PCn;  // node-message inputs [N][48] [N][128] [N][128]
    float *ptsE, *PAe, *PCe;  // edge-message inputs
    float *score;             // [N][4]
    float *chi_tmp;           // [N][4]
    void *arena = nullptr;          // ONE device allocation behind every workspace pointer above (one hipMalloc / hipFree per ctx)
    size_t arena_bytes = 0;
    hipStream_t last_stream = nullptr;   // the stream of the most recent call on this context (arena hand-over)
    int max_steps;
    // clash / proximal workspaces
    float *xyz;               // [N][14][3]
    float *rec;               // [N][16][4] packed per-residue records for k_clash (positions + radii, CA + reach, ids)
    float *axes;              // [N][4][6]  chi-frame x-axis (3) | origin (3)
    float *rec2, *axes2;      // the other buffers of the proximal loop: step t reads rec / axes of step t and writes those of step t + 1
    float *brad;              // [N] bounding radius around CA
    float *per_res;           // [N]
    float *dchi;              // [N][4]
    float *px, *pm, *pv, *pz, *pxeff;   // proximal: param, Adam moments, anchor, effective chi  [N][4]
    uint8_t *pmask;           // [N]
    int32_t *cand;            // [N][4][PP_CL_CAP] proximal: static clash-partner candidates of every (residue, wave of its workgroup)
    int32_t *cand_cnt;        // [N][4] their number, -1 = more than PP_CL_CAP (that wave scans all partners as before)
    float *prox_part;         // [PP_PROX_CHUNK][N] per-residue loss terms of the proximal steps parked before one reduction (k_prox_losses)
    // the proximal loop (packed contexts and B = 1) runs per complex of seg_off, all complexes in the same launches
    int32_t *prox_nrows;      // [B] the caller's norm_rows (the row count each complex's means divide by)
    float2 *prox_seg;         // [B] per complex: (mean divisor, 1 / divisor), written by k_prox_init
    float *prox_inv;          // [N] 1 / divisor of the row's complex: the gradient and anchor weight of k_clash<CAND, true>
    float *scal;              // small scalar scratch
    // obstacle atoms (pp_ctx_set_obstacles): fixed spheres the side chains of a segment must not overlap
    float4 *obst = nullptr;   // [obst_M] (x, y, z, radius): the context's own copy, ONE allocation outside the arena, freed with the ctx
    int obst_M = 0;           // 0 = the context holds no obstacles: every launcher takes the instances it has always taken
    int obst_cap = 0;         // atoms the allocation holds
    int2 *obst_seg;           // [B] (first, count) of every segment's range in obst
    int2 *obst_row;           // [N] the range of the row's segment (k_obst_rows)
    int32_t *obst_cand;       // [N][PP_OB_CAP] proximal: static obstacle candidates of every residue, ascending (k_obst_cand)
    int32_t *obst_cnt;        // [N] their number, -1 = more than PP_OB_CAP (the residue scans its segment's range)
    float *sasa_row;          // [N][8] pp_sasa: slot 1 (3), bounding radius of the present atoms around it, largest R (k_sasa_rows)
    pp_workspace ws[PP_WS_COUNT];   // the lazy workspaces of the analysis entries (pp_ctx_workspace)
    // seeded sampling noise (pp_rng.h): the per-row table of the seeded kernels and the complexes' keys
    pp_rng_row *rng_tab;      // [N] (row within the complex, key of the complex); filled by pp_launch_rng_table
    uint64_t *rng_keys;       // [B] the caller's keys (pp_ctx_set_rng_keys), staged for the table kernel
    bool rng_tab_set = false; // the table holds the default keys (segment ordinals) or the caller's
    // live rows (pp_prepare.hip k_live_rows): the rows whose side chain a sampling run can move.  Set 0 is made
    // when the context is prepared, set 1 by every pp_sample_partial (it also drops the call's fixed rows)
    int32_t *live_rows[2];    // [N + 2] the rows in ascending order, then -1 up to the end
    int2 *live_mix[2];        // [N] k_edge_update_mix: the one or two rows of every workgroup in dispatch order ((-1, -1): none; (r, -1): one)
    int32_t *live_cnt[2];     // [1] number of live rows
    bool live_mix_set[2] = {false, false};   // pp_launch_live_rows filled live_mix of this set (only contexts of the mixed launch's size)
    unsigned *sat;            // sticky word: bit 0 = an edge kernel, bit 1 = a node kernel clamped a hidden activation at 65504
    // in-situ kernel timing (pp_profile_kernel): every launch of one hot kernel carries a start / stop event pair
    // (hipExtLaunchKernelGGL: the dispatch's own begin / end timestamps, what rocprofv3's kernel trace reports)
    int prof_which = -1;       // -1 off, 0 node message, 1 edge update, 2 node update
    bool prof_armed = false;   // the next PP_LAUNCH on this ctx is one of the profiled kernel
    std::vector<hipEvent_t> prof_ev;
    size_t prof_n = 0;         // events used (2 per launch)
};

void pp_set_error(const std::string &msg);
#define PP_HIP_CHECK(expr)                                                                   \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            pp_set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                 \
            return PP_ERR_HIP;                                                               \
        }                                                                                    \
    } while (0)
// refuse a call: leave the message for pp_last_error, return the status
#define FAIL(code, msg)          \
    do {                         \
        pp_set_error(msg);       \
        return code;             \
    } while (0)
// workspace `which` (PP_WS_*) of the context at exactly `bytes`: the existing allocation if its size matches; one of another size (it
// cannot arise today) is replaced, not trusted.  Here, not in pp_api.hip, so that tests/native/workspace_sanitize.cpp can compile the
// two functions against stand-ins for hipMalloc / hipFree
inline pp_status pp_ctx_workspace(pp_ctx *c, int which, size_t bytes, void **out) {
    pp_workspace &w = c->ws[which];
    if (w.p && w.bytes != bytes) {
        PP_HIP_CHECK(hipFree(w.p));
        w = {};
    }
    if (!w.p) {
        PP_HIP_CHECK(hipMalloc(&w.p, bytes));
        w.bytes = bytes;
    }
    *out = w.p;
    return PP_OK;
}
// pp_ctx_destroy: hipFree waits for the device, so only a context that ever ran one of these entries pays it
inline void pp_ctx_free_workspaces(pp_ctx *c) {
    for (pp_workspace &w : c->ws) {
        if (w.p) (void)hipFree(w.p);
        w = {};
    }
}
// what the ensemble calls (`who`: pp_ensemble_reduce, pp_ensemble_recombine) ask of the context: packed or B = 1, and its segments
// and rows groups of n_decoys (pp_ensemble.hip)
pp_status pp_check_decoy_groups(const pp_ctx *c, int n_decoys, const char *who);

// ---- f16 operand range check (-DPP_CHECK_RANGE: the libpackppi_hip.chk.so build; packppi_amd/rangecheck.py) -----------------
// The split-f16 kernels saturate hidden activations at the f16 maximum (65504) and assume every other operand is far below it.
// That holds by orders of magnitude for the seeded fixtures; a trained checkpoint is checked, not trusted: in this build every
// fp32 value that is about to be split into f16 operands is compared with the limit and counted (per translation unit; atomics:
// this build is for checking, not for timing).  The default build compiles none of it.
#ifdef PP_CHECK_RANGE
#define PP_RANGE_COUNTER static __device__ unsigned int g_range_hits;
#define PP_RANGE(x)                                                                                    \
    {                                                                                                  \
        const float rx_ = (x);                                                                         \
        if (!(__builtin_fabsf(rx_) < 65504.f)) atomicAdd(&g_range_hits, 1u);                           \
    }
#define PP_RANGE_READER(name)                                                                          \
    unsigned int name(int reset) {                                                                     \
        unsigned int v = 0, z = 0;                                                                     \
        (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_range_hits), sizeof(v));                            \
        if (reset) (void)hipMemcpyToSymbol(HIP_SYMBOL(g_range_hits), &z, sizeof(z));                   \
        return v;                                                                                      \
    }
#else
#define PP_RANGE_COUNTER
#define PP_RANGE(x)
#define PP_RANGE_READER(name) \
    unsigned int name(int) { return 0; }
#endif
// ---- sticky f16 saturation flag of the DEFAULT kernels ------------------------------------------------------------------
// Hidden activations are clamped at the f16 maximum before they are split (one v_med3).  Every build remembers when that
// happened: the clamped halves are folded into a per-lane running maximum (v_pk_max_u16 on the packed pair: non-negative
// f16 bit patterns order like integers), and a lane that saw 0x7BFF ORs a bit into the
// context's sticky word when the kernel ends.  pp_ctx_saturated reads it.  NaN activations are not flagged (v_med3 turns
// them into a finite value first): they cannot arise from finite inputs here, see relu_sat in pp_node.hip.
__device__ __forceinline__ bool pp_sat_hit(unsigned packed_max) {
    return (packed_max & 0xffffu) >= 0x7bffu || (packed_max >> 16) >= 0x7bffu;
}
unsigned int pp_edge_range_hits(int reset);
unsigned int pp_node_range_hits(int reset);

// next (start, stop) event pair of an armed profiling run; false when profiling is off for this launch
bool pp_prof_take(pp_ctx *c, hipEvent_t *e0, hipEvent_t *e1);
#define PP_LAUNCH(c, kernel, grid, block, shmem, s, ...)                                              \
    do {                                                                                               \
        hipEvent_t e0_ = nullptr, e1_ = nullptr;                                                       \
        if ((c)->prof_armed && pp_prof_take((c), &e0_, &e1_))                                          \
            hipExtLaunchKernelGGL(kernel, grid, block, shmem, s, e0_, e1_, 0, __VA_ARGS__);            \
        else                                                                                           \
            hipLaunchKernelGGL(kernel, grid, block, shmem, s, __VA_ARGS__);                            \
    } while (0)

// ---- inter-residue dihedral, rounded like the reference's ATen CPU ops (encoder.py:164-174) ------------------------------
// sgn * arccos(n1 . n2) has no clamp: where four atoms are coplanar (every j == i edge; on ideal-geometry backbones also a few
// trans pairs with |psi| within 3e-4 of pi) the argument is 1 or -1 up to rounding, and one ulp decides between NaN -> 0,
// exactly pi and pi - 5e-4: the feature is rounding noise of size pi.  The only way to agree with the reference there is to
// round as it does.  Measured against torch 2.10 CPU (tools/debug/aten_rounding_probe.py, 76 864 dihedrals of four C5
// complexes, argument and sign bit-equal):  torch.cross  c = fma(a1, b2, -(a2 * b1))  (second product rounded first);
// torch.norm  sqrt(fma(z, z, fma(y, y, x * x)));  (a * b).sum(-1)  ((p0 + p1) + p2) on separately rounded products; IEEE
// division.  arccos itself differs from ATen's by at most an ulp, which is smooth.
#ifdef __HIPCC__
__device__ __forceinline__ void pp_cross_t(const float *a, const float *b, float *o) {
#pragma clang fp contract(off)
    const float q0 = a[2] * b[1], q1 = a[0] * b[2], q2 = a[1] * b[0];
    o[0] = __builtin_fmaf(a[1], b[2], -q0);
    o[1] = __builtin_fmaf(a[2], b[0], -q1);
    o[2] = __builtin_fmaf(a[0], b[1], -q2);
}
__device__ __forceinline__ float pp_dot_t(const float *a, const float *b) {
#pragma clang fp contract(off)
    const float p0 = a[0] * b[0], p1 = a[1] * b[1], p2 = a[2] * b[2];
    return (p0 + p1) + p2;
}
__device__ __forceinline__ void pp_unit_t(float *v) {
#pragma clang fp contract(off)
    const float x2 = v[0] * v[0];
    const float n = sqrtf(__builtin_fmaf(v[2], v[2], __builtin_fmaf(v[1], v[1], x2)));
    for (int k = 0; k < 3; k++) {
        const float q = v[k] / n;
        v[k] = (q != q) ? 0.f : q;           // nan_to_num of 0 / 0; +-inf cannot occur for finite input
    }
}
__device__ __forceinline__ float pp_pair_dihedral_t(const float *p0, const float *p1, const float *p2, const float *p3) {
#pragma clang fp contract(off)
    float u0[3], u1[3], u2[3], n1[3], n2[3], c12[3];
    for (int k = 0; k < 3; k++) { u0[k] = p2[k] - p1[k]; u1[k] = p0[k] - p1[k]; u2[k] = p3[k] - p2[k]; }
    pp_cross_t(u0, u1, n1); pp_unit_t(n1);
    pp_cross_t(u0, u2, n2); pp_unit_t(n2);
    pp_cross_t(u1, u2, c12);
    const float sg = pp_dot_t(c12, u0);
    const float sgn = (sg > 0.f) ? 1.f : ((sg < 0.f) ? -1.f : 0.f);
    const float ang = sgn * acosf(pp_dot_t(n1, n2));
    return (ang != ang) ? 0.f : ang;
}
#endif

// PackPPI-AP head tensors (pp_affinity.hip): one device allocation; matrices read by k_affinity_embed in the k-quad
// interleaved layout of dense_slice ([in / 4][128][4]), those of k_affinity_head transposed ([in][out])
struct pp_affinity {
    int device;
    bool network;                                              // has mut_bias / seq_embedding / mutation_fusion (mode network)
    float *buf;
    const float *mut_bias, *seq_emb;                           // [2][128], [21][128]
    const float *f0T, *f0_b, *f2T, *f2_b;                      // mutation_fusion.0 [96][128][4], .2 [32][128][4]
    const float *d0T, *d0_b, *d2T, *d2_b, *d4_w, *d4_b;        // ddg_predictor.0 / .2 [128][128], .4 [128], [1]
};

// Seeded sampling noise as a kernel argument: the LAST parameter of k_node_update / k_node_update_valu, read by the seeded
// instances only (tab == nullptr: the noise, if any, comes from the caller's tensor)
struct PPRng {
    const pp_rng_row *tab;
    uint32_t seed_lo, seed_hi;
};

// Partial repacking (pp_sample_partial) as a kernel argument: the LAST parameter of k_node_update / k_node_update_valu, behind
// PPRng, read by the PINNED instances only.  One per reverse step: the host sets sigma, renoise and traj for step j.
struct PPPin {
    const uint8_t *fixed;     // [N] 1 = the row keeps chi_ref, 0 = the row steps
    const float *chi_ref;     // [N][4]
    float *traj;              // this step's [N][4] slice of chi_traj, or null
    float sigma;              // sigma(schedule[j + 1]) in fp32 as fill_step computes it: the noise level the step arrives at
    int renoise;              // 1: a fixed row gets chi_ref re-noised to sigma with this step's draws; 0: chi_ref itself
};                            //    (PP_FIX_HOLD, and the last step of PP_FIX_RENOISE)

// The live rows of a sampling run as the layer-1 edge update takes them (pp_ctx::live_*): rows for the one- and two-row instances
// (workgroup b reads rows[R b .. R b + R - 1]), mix for the mixed launch (workgroup b reads mix[b])
struct PPLive {
    const int32_t *rows;
    const int2 *mix;
};

// ---- the shape of an edge-level launch over M rows ------------------------------------------------------
// ONE rule for the host's launchers (M = the context's rows) and for k_live_rows (M = the live rows, known only on the device).  A CU
// hosts `slots` (PP_WGS2) workgroups of the two-row instances, S = slots * CUs in one round, and every workgroup streams the layer's
// whole weight set:
//   M <= S            one row per workgroup: one round, no CU streams the weights more than `slots` times
//   S < M <= 3 S / 2  three rows on a CU in one round as one pair and one one-row workgroup: (M + 2) / 3 pairs (section 4.8)
//   3 S / 2 < M <= 2 S  pairs: one round of co-resident pairs
//   2 S < M <= 3 S    a full round of S pairs, then the other M - 2 S rows as one-row workgroups: the tail of a second round of
//                     pairs lasts as long as a pair running alone, a one-row workgroup is done sooner (section 4.9)
//   3 S < M           pairs: the length follows the number of weight passes
// Pairs are dispatched first, in the table of k_live_rows and in the all-rows mixed launches (pp_edge_f16.hip use_mix; the
// diagnostics library's PP_EDGE_MIX=3 restores their earlier order).  An odd M leaves the last pair with one row: one_row is never
// negative.
#ifndef PP_WGS2
#define PP_WGS2 2          // workgroups per CU of the two-row edge instances (pp_edge_f16.hip)
#endif
struct PPEdgeShape {
    int pairs, one_row;
    bool pairs_first;
};
__host__ __device__ inline PPEdgeShape pp_edge_shape(int M, int num_cu, int slots) {
    const int S = slots * num_cu;
    PPEdgeShape sh = {(M + 1) / 2, 0, true};
    if (M <= S) sh.pairs = 0;
    else if (2 * M <= 3 * S) sh.pairs = (M + 2) / 3;
    else if (M > 2 * S && M <= 3 * S) sh.pairs = S;
    sh.one_row = M > 2 * sh.pairs ? M - 2 * sh.pairs : 0;
    return sh;
}
// entry b of the work table of a mixed launch (pp_ctx::live_mix) with this shape: rows [>= M + 1] holds the M rows, then -1
__host__ __device__ inline int2 pp_live_mix_entry(const int32_t *rows, const PPEdgeShape &sh, int b) {
    int2 e = make_int2(-1, -1);
    const int p = sh.pairs_first ? b : b - sh.one_row, q = sh.pairs_first ? b - sh.pairs : b;      // index among the pairs / the one-row
    if (p >= 0 && p < sh.pairs) e = make_int2(rows[2 * p], rows[2 * p + 1]);
    else if (q >= 0 && q < sh.one_row) e.x = rows[2 * sh.pairs + q];
    return e;
}
// the context sizes whose live-row launch is the mixed one and takes its rows from the work table (both mixed regimes above)
inline bool pp_live_mix_size(int N, int num_cu, int slots) {
    const int S = slots * num_cu;
    return (N > S && 2 * N <= 3 * S) || (N > 2 * S && N <= 3 * S);
}
// its workgroups for the worst case over M <= N live rows (the host never learns M; surplus workgroups read (-1, -1) and leave):
// no shape of M <= 3 S / 2 rows has more than S workgroups, one of 2 S < M rows has M - S
inline int pp_live_mix_grid(int N, int num_cu, int slots) {
    const int S = slots * num_cu;
    return N > 2 * S ? N - S : S;
}

// ---- launchers implemented in the kernel translation units ----------------------------------
// live-row set `set` of the context (0: every row with an angle to move; 1: those that are not `fixed` either), on the stream
pp_status pp_launch_live_rows(pp_ctx *c, int set, const uint8_t *fixed, hipStream_t s);
// seeded noise (pp_node.hip): the per-row table from the context's segment table (keys_set: c->rng_keys holds the caller's keys,
// else a complex's key is its ordinal), the draws of one step, the initial noising
pp_status pp_launch_rng_table(pp_ctx *c, bool keys_set, hipStream_t s);
pp_status pp_launch_noise_seeded(pp_ctx *c, uint64_t seed, int step, float *noise, uint32_t *words, hipStream_t s);
pp_status pp_launch_add_noise_seeded(pp_ctx *c, const float *chi0, float sigma, uint64_t seed, float *chi, hipStream_t s);
// k_affinity_embed (pp_node.hip): the mutation branch's node embedding + fusion -> ctx h_V and layer 0's node-message inputs
pp_status pp_launch_affinity_embed(pp_ctx *c, const pp_affinity *a, const int64_t *rtype, const float *sc_sincos,
                                   const int64_t *mut_mask, const float *hV_pret, hipStream_t s);
pp_status pp_launch_prepare(pp_ctx *c, hipStream_t s, const int64_t *E_idx = nullptr);   // E_idx: given neighbour lists instead of the kNN search
pp_status pp_launch_node_embed(pp_ctx *c, const float *chi, const StepParams &sp, hipStream_t s);
pp_status pp_launch_node_embed_rows(pp_ctx *c, const float *chi, const float *t_rows, hipStream_t s);   // a time per row (DEVICE [N])
// What one network evaluation is given besides the context (host side; a single evaluation leaves all but `cur` zero).  The middle
// layers read none of it but chi, step, mode and noise, which they hand to their kernel unread.
struct NodeEval {
    float *chi;                 // the angles the reverse step moves, or null
    int step, mode;             // the step's index; PP_MODE_ODE / PP_MODE_SDE
    const float *noise;         // pp_sample's sde noise tensor, or null
    const StepParams *cur;      // layer 2: this step's scalars
    const StepParams *next;     // layer 2 inside sampling: the next step, if its node embedding is to follow (else null)
    const PPRng *rng;           // layer 2 inside seeded sampling, else null: the reverse step draws its own noise, `noise` is not read
    const PPPin *pin;           // layer 2 inside pp_sample_partial, else null (needs rng in either mode): the PINNED reverse step
};
pp_status pp_launch_node_update(pp_ctx *c, int layer, int last_mode, const NodeEval &ev, hipStream_t s);
pp_status pp_launch_edge_static(pp_ctx *c, hipStream_t s);
#ifdef PP_EDGE_F16
pp_status pp_launch_edge_embed_f16(pp_ctx *c, hipStream_t s);   // pp_edge_f16.hip: MFMA form of k_edge_embed
#endif
pp_status pp_launch_node_message(pp_ctx *c, int layer, hipStream_t s);
bool pp_edge_fused();            // does pp_launch_edge_update also compute the next layer's node message?
// + node message of layer + 1.  keep_hE: write the new h_E back to c->hE.  A fused evaluation passes false for layer 1, where
// the fused message takes h_E from registers and the next evaluation's layer 0 overwrites c->hE before anything reads it;
// the unfused build (whose layer-2 node message reads c->hE) and the diagnostics pass true.  Layer 0 always stores.
// live (layer 1 of a sampling run without write-back, else null): only the listed rows get a workgroup; S / msum of the others keep
// what layer 0's launch wrote (see pp_api.hip run_network)
pp_status pp_launch_edge_update(pp_ctx *c, int layer, bool keep_hE, hipStream_t s, const PPLive *live = nullptr);
pp_status pp_launch_atom14(pp_ctx *c, const float *chi, float *xyz, hipStream_t s);
pp_status pp_launch_clash(pp_ctx *c, const float *xyz, float *per_res, float *dchi, hipStream_t s, bool use_candidates = false);
// One loop for both: pp_launch_proximal is the single-complex call (means over the complex's own rows, losses [nsteps]) without the
// accept rule; the packed one takes per-complex divisors from c->prox_nrows if norm_given, fills losses [B][nsteps] and chi_accepted.
// fixed (pp_proximal_pinned, else null; device [N]): rows taken out of the clash mask where it is made; moved (device [N] or null)
// receives the mask that was optimised.
pp_status pp_launch_proximal(pp_ctx *c, const float *chi, float lamda, int nsteps, float *traj,
                             float *chi_last, float *losses, hipStream_t s);
pp_status pp_launch_proximal_packed(pp_ctx *c, const float *chi, float lamda, int nsteps, bool norm_given, float *traj,
                                    float *chi_last, float *chi_accepted, float *losses, hipStream_t s,
                                    const uint8_t *fixed = nullptr, uint8_t *moved = nullptr);

// pp_sample_guided (pp_clash.hip).  begin: the static partner lists and obstacle candidates, once per call.
// nudge: chi stepped in place against the clash gradient at chi (rows of `fixed`, device [N] or null, are left alone); trace
// (device [B][n_schedule] or null) receives every segment's mean clash before the step at column j.  They use the proximal loop's
// workspaces (cand, obst_cand, xyz, rec, axes, per_res).
pp_status pp_launch_guide_begin(pp_ctx *c, hipStream_t s);
pp_status pp_launch_guide_nudge(pp_ctx *c, float *chi, const uint8_t *fixed, float eta, float cap, double *trace, int n_schedule,
                                int j, hipStream_t s);

// pp_sample_corrected (pp_correct.hip): the Langevin corrector behind reverse step j on chi, in place, from the
// score in c->score; per segment of the context's table, one workgroup each.  snr = snr[j]; the draws are those of counter step
// 2^20 + j.  trace (device [n_seg][n_steps][4] or null) receives (s2, n2, eps, amp) at row j of every segment that has a corrector.
pp_status pp_launch_correct(pp_ctx *c, float *chi, const uint8_t *fixed, float snr, int j, int n_steps, const PPRng &rng,
                            double *trace, hipStream_t s);

void pp_edge_occupancy(int *node_msg, int *edge_upd);
#if defined(PP_DIAG) && defined(PP_EDGE_F16)
// pp_debug_launch_plan: the launchers' own choices for a context of N rows (pp_edge_f16.hip pick_R / use_mix / mix_pairs, pp_node.hip nu_shape)
pp_status pp_edge_launch_plan(int N, int *R, int *mixed, int *n_pairs);
pp_status pp_node_launch_plan(int N, int *cl, int *multi);
#endif

// last_mode values for pp_launch_node_update
#define PP_NU_MID 0        // layers 0,1: update + edge-message inputs + next layer's node-message inputs
#define PP_NU_SCORE 1      // layer 2, single evaluation: update + decoder
#define PP_NU_STEP 2       // layer 2 inside sampling: update + decoder + reverse step + next embed
