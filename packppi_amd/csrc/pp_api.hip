// C ABI of libpackppi_hip.so: plan / ctx lifetime and the per-call kernel schedules.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "pp_internal.h"
#include "pp_pack.h"           // the packed weight layouts and pack_network() (host-only header)
#ifdef PP_EDGE_F16
#include "pp_rebalance.h"      // rebalance_relu_chains(): power-of-two rebalancing of the ReLU chains (host-only header)
#endif
#include "pp_topk_aten.h"

static thread_local std::string g_err;
void pp_set_error(const std::string &msg) { g_err = msg; }

extern "C" const char *pp_last_error(void) { return g_err.c_str(); }
extern "C" int pp_version(void) { return 101; }
// build stamp (packppi_amd/build.py passes -DPP_BUILD_ID="<sources>-<flags>"); the marker prefix lets build.py read it from
// the file without loading the library
#ifndef PP_BUILD_ID
#define PP_BUILD_ID "unstamped-unstamped"
#endif
static const char g_build_id[] = "PP_BUILD_ID=" PP_BUILD_ID;
extern "C" const char *pp_build_id(void) { return g_build_id + 12; }

template <typename T>
static pp_status upload(T **dst, const T *src, size_t n) {
    PP_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(dst), n * sizeof(T)));
    PP_HIP_CHECK(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return PP_OK;
}

// f16 operand range check (pp_internal.h): events counted since the last reset by the kernels of a -DPP_CHECK_RANGE build
extern "C" int pp_has_range_check(void) {
#ifdef PP_CHECK_RANGE
    return 1;
#else
    return 0;
#endif
}
// `who`: the export the message names
static pp_status range_check(const char *who, unsigned long long *edge_events, unsigned long long *node_events, int reset) {
#ifdef PP_CHECK_RANGE
    (void)who;
    PP_HIP_CHECK(hipDeviceSynchronize());
    *edge_events = (unsigned long long)pp_edge_range_hits(reset);
    *node_events = (unsigned long long)pp_node_range_hits(reset);
    return PP_OK;
#else
    (void)reset;
    *edge_events = *node_events = 0;
    FAIL(PP_ERR_UNSUPPORTED, std::string(who) + ": this library was built without -DPP_CHECK_RANGE (use libpackppi_hip.chk.so: "
                                                "python -m packppi_amd.rangecheck)");
#endif
}
extern "C" pp_status pp_range_check_parts(unsigned long long *edge_events, unsigned long long *node_events, int reset) {
    if (!edge_events || !node_events) FAIL(PP_ERR_INVALID, "pp_range_check_parts: null argument");
    return range_check("pp_range_check_parts", edge_events, node_events, reset);
}
extern "C" pp_status pp_range_check(unsigned long long *events, int reset) {
    if (!events) FAIL(PP_ERR_INVALID, "pp_range_check: null argument");
    unsigned long long edge = 0, node = 0;
    const pp_status st = range_check("pp_range_check", &edge, &node, reset);
    *events = edge + node;
    return st;
}
// Non-finite INPUTS.  The kernels clamp hidden activations with v_med3 / v_max, which turn a NaN into a finite number: a NaN that
// enters with the caller's tensors would come out as finite angles that mean nothing, where the reference returns NaN
// (layers.py:22-33 has no such clamp).  From finite inputs no NaN can arise inside (every weight is checked finite at plan
// creation, every LayerNorm has its eps, every hidden activation is bounded), so the inputs are what is checked: the backbone
// coordinates of unmasked rows when a context is prepared, the angles at every pp_score / pp_sample.  Bit 2 of the sticky word.
__global__ void k_flag_nonfinite(const float *__restrict__ v, int rows, int row_stride, int per_row, const float *__restrict__ rmask,
                                 unsigned *__restrict__ sat) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * per_row) return;
    const int r = i / per_row, k = i - r * per_row;
    if (rmask && rmask[r] == 0.f) return;
    const float x = v[(size_t)r * row_stride + k];
    if (!(__builtin_fabsf(x) <= 3.402823466e38f)) atomicOr(sat, 4u);
}
static void flag_nonfinite(pp_ctx *c, const float *v, int row_stride, int per_row, hipStream_t s) {
    const int n = c->N * per_row;
    hipLaunchKernelGGL(k_flag_nonfinite, dim3((n + 255) / 256), dim3(256), 0, s, v, c->N, row_stride, per_row, c->b.residue_mask, c->sat);
}

// sticky saturation word of the context (every build): waits for `stream`
extern "C" pp_status pp_ctx_saturated(pp_ctx *c, int *flags, void *stream) {
    if (!c || !flags) FAIL(PP_ERR_INVALID, "pp_ctx_saturated: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned v = 0;
    PP_HIP_CHECK(hipMemcpyAsync(&v, c->sat, sizeof(v), hipMemcpyDeviceToHost, s));
    PP_HIP_CHECK(hipStreamSynchronize(s));
    *flags = (int)v;
    return PP_OK;
}

// The context's live rows (the rows a sampling run can move: residue_mask != 0 and a non-zero SC_D_mask entry), ascending:
// rows is a DEVICE array [N] (entries behind the count are -1), *count their number.  Waits for `stream`.
extern "C" pp_status pp_ctx_live_rows(pp_ctx *c, int32_t *rows, int *count, void *stream) {
    if (!c || !rows || !count) FAIL(PP_ERR_INVALID, "pp_ctx_live_rows: null argument");
    if (!c->plan->has_network) FAIL(PP_ERR_INVALID, "pp_ctx_live_rows: plan was created without network weights");
    hipStream_t s = static_cast<hipStream_t>(stream);
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    int32_t cnt = 0;
    PP_HIP_CHECK(hipMemcpyAsync(rows, c->live_rows[0], (size_t)c->N * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    PP_HIP_CHECK(hipMemcpyAsync(&cnt, c->live_cnt[0], sizeof(cnt), hipMemcpyDeviceToHost, s));
    PP_HIP_CHECK(hipStreamSynchronize(s));
    *count = (int)cnt;
    return PP_OK;
}

// The work table of the context's mixed live-row launch, read-only: mix is a HOST array [N][2], entry b the
// one or two rows of workgroup b in dispatch order ((r, -1): one row; (-1, -1): none).  *workgroups is the launch's grid -- every live
// row must sit in front of it -- or 0 for a context whose size does not take the mixed launch (mix is left alone).  Takes no stream:
// a read-back for tests and tools, it waits for the whole device (whatever stream prepared the context, the table is complete).
extern "C" pp_status pp_ctx_live_mix(pp_ctx *c, int32_t *mix, int *workgroups) {
    if (!c || !mix || !workgroups) FAIL(PP_ERR_INVALID, "pp_ctx_live_mix: null argument");
    if (!c->plan->has_network) FAIL(PP_ERR_INVALID, "pp_ctx_live_mix: plan was created without network weights");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    *workgroups = 0;
    if (!c->live_mix_set[0]) return PP_OK;
    PP_HIP_CHECK(hipDeviceSynchronize());
    PP_HIP_CHECK(hipMemcpy(mix, c->live_mix[0], (size_t)c->N * sizeof(int2), hipMemcpyDeviceToHost));
    *workgroups = pp_live_mix_grid(c->N, c->plan->num_cu, PP_WGS2);
    return PP_OK;
}

// The same table on the HOST, for a device of num_cu compute units (no device call; the rule and the entries are the functions
// k_live_rows calls, pp_internal.h): rows [N + 2] holds M rows and then -1, mix is [N][2].  *workgroups as above.
extern "C" pp_status pp_live_mix_host(const int32_t *rows, int M, int N, int num_cu, int32_t *mix, int *workgroups) {
    if (!rows || !mix || !workgroups || M < 0 || M > N || num_cu < 1) FAIL(PP_ERR_INVALID, "pp_live_mix_host: null argument, M outside 0 .. N or no compute unit");
    const PPEdgeShape sh = pp_edge_shape(M, num_cu, PP_WGS2);
    for (int b = 0; b < N; b++) {
        const int2 e = pp_live_mix_entry(rows, sh, b);
        mix[2 * b] = e.x;
        mix[2 * b + 1] = e.y;
    }
    *workgroups = pp_live_mix_size(N, num_cu, PP_WGS2) ? pp_live_mix_grid(N, num_cu, PP_WGS2) : 0;
    return PP_OK;
}

// How far a side-chain atom can get from its CA whatever the chi angles are, per residue type: the atom sits at chain(lit) in the
// backbone frame (origin CA), the chain composes default frames and rotations about x, a rotation keeps the norm and a frame adds at
// most the length of its translation: |atom - CA| <= |lit| + sum of |t_k| over the frames of its chain (features.py:95-194).
// Rigorous, about 15 % above the true maximum; the proximal loop's static partner lists are built from it (pp_clash.hip).
static void side_chain_extents(const pp_tables *tables, float (&ext)[21]) {
    for (int S = 0; S < 21; S++) {
        float m = 0.f;
        for (int a = 4; a < 14; a++) {
            if (tables->atom14_mask[S * 14 + a] == 0.f) continue;
            const float *lp = tables->lit_positions + (S * 14 + a) * 3;
            float b = std::sqrt(lp[0] * lp[0] + lp[1] * lp[1] + lp[2] * lp[2]);
            const int g = tables->atom14_to_group[S * 14 + a];
            auto tlen = [&](int k) { const float *f = tables->default_frames + ((size_t)S * 8 + k) * 16; return std::sqrt(f[3] * f[3] + f[7] * f[7] + f[11] * f[11]); };
            if (g >= 4) for (int k = 4; k <= g; k++) b += tlen(k);
            else b += tlen(g);
            m = std::max(m, b);
        }
        ext[S] = m * 1.0001f + 1e-3f;
    }
}

// owners for objects under construction: an early return releases what was allocated so far through the public destroy call
struct PlanDeleter { void operator()(pp_plan *p) const { pp_plan_destroy(p); } };
struct CtxDeleter { void operator()(pp_ctx *c) const { pp_ctx_destroy(c); } };

extern "C" pp_status pp_plan_create(const float *weights, size_t n_weights, const pp_tables *tables, int device,
                                    pp_plan **out) {
    if (!tables || !out) FAIL(PP_ERR_INVALID, "pp_plan_create: null argument");
    WeightOff off = pp_weight_offsets();
    const bool has_net = weights != nullptr;
    if (has_net && (n_weights != off.total || off.total != PP_N_WEIGHTS))
        FAIL(PP_ERR_INVALID, "pp_plan_create: expected " + std::to_string(off.total) + " weights, got " +
                                 std::to_string(n_weights));
    if (has_net)      // the dense layers run on two-way f16 splits of the weights: every weight must be finite and inside the f16 range
        for (size_t i = 0; i < n_weights; i++)
            if (!(std::fabs(weights[i]) < 65504.f))
                FAIL(PP_ERR_INVALID, "pp_plan_create: weight " + std::to_string(i) + " is not finite or outside the f16 range (" +
                                         std::to_string(weights[i]) + ")");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FAIL(PP_ERR_NO_DEVICE, "pp_plan_create: no HIP device visible");
    if (device < 0 || device >= ndev) FAIL(PP_ERR_INVALID, "pp_plan_create: bad device index");
    PP_HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    PP_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        FAIL(PP_ERR_NO_DEVICE, std::string("pp_plan_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);

    // value-initialised: every device pointer is null until its upload, and pp_plan_destroy skips nulls -- every return below
    // frees the plan and what it holds so far
    std::unique_ptr<pp_plan, PlanDeleter> p(new (std::nothrow) pp_plan());
    if (!p) FAIL(PP_ERR_INVALID, "out of host memory");
    p->device = device;
    p->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    p->off = off;
    p->has_network = has_net;
    p->knn_ties = PP_KNN_TIES_ATEN_CPU;
    p->annealed_temp = 3.0f;      // configs/model/sample_cfg/Sampling.yaml:4
    p->rebalanced_chains = 0;
    pp_status st;
    const float *wpack = weights;          // what the edge-level MFMA streams are packed from
#ifdef PP_EDGE_F16
    std::vector<float> rebalanced, ln_packed;
    if (has_net) {
        LnScales sc;
        p->rebalanced_chains = rewrite_checkpoint(weights, off, rebalanced, ln_packed, sc);
        p->ln_scaled_features = sc.n_scaled;
        for (size_t i = 0; i < off.total; i++)
            if (!(std::fabs(rebalanced[i]) < 65504.f) || !(std::fabs(ln_packed[i]) < 65504.f))
                FAIL(PP_ERR_INVALID, "pp_plan_create: weight " + std::to_string(i) + " leaves the f16 range when its ReLU chain is "
                                     "rebalanced (run this checkpoint on libpackppi_hip.f32.so)");
        weights = rebalanced.data();       // everything below -- device copy, node-level streams, transposed copies -- is made from it
        wpack = ln_packed.data();          // ... and the edge-level streams from the copy with the operand scales in its columns
        if (sc.n_scaled > 0 && (st = upload(&p->ln_scale, &sc.v[0][0], (size_t)5 * 128)) != PP_OK) return st;
    }
#endif
    if (has_net) {
        if ((st = upload(&p->w, weights, off.total)) != PP_OK) return st;
        std::vector<float> arena;
        const PackOff o = pack_network(arena, weights, wpack, off);
        if ((st = upload(&p->wT, arena.data(), arena.size())) != PP_OK) return st;
        const float *wT = p->wT;
        p->node_emb_T = wT + o.node_emb_T;
        p->edge_emb_T = wT + o.edge_emb_T;
        for (int l = 0; l < 3; l++) {
            const LayerPackOff &ol = o.lt[l];
            LayerT &t = p->lt[l];
            t.pts_node_wT = wT + ol.pts_node_wT; t.pts_edge_wT = wT + ol.pts_edge_wT;
            t.nm_A_T = wT + ol.nm_A_T; t.nm_C_T = wT + ol.nm_C_T;
            t.em_A_T = wT + ol.em_A_T; t.em_C_T = wT + ol.em_C_T;
            t.nm_out_T = wT + ol.nm_out_T;
            t.nd_in_T = wT + ol.nd_in_T; t.nd_out_T = wT + ol.nd_out_T;
            t.nm_stream = wT + ol.nm_stream; t.em_stream = wT + ol.em_stream;
            t.em_params = wT + ol.em_params;
            t.nu_stream = wT + ol.nu_stream; t.nu_params = wT + ol.nu_params;
        }
        p->static_stream = wT + o.static_stream;
#ifdef PP_EDGE_F16
        p->embed_stream = wT + o.embed_stream;
#endif
        p->d0_in_T = wT + o.d0_in_T; p->d0_out_T = wT + o.d0_out_T;
        p->d2_in_T = wT + o.d2_in_T; p->d2_out_T = wT + o.d2_out_T;
    }

    if ((st = upload(&p->default_frames, tables->default_frames, 21 * 8 * 16)) != PP_OK) return st;
    if ((st = upload(&p->atom14_to_group, tables->atom14_to_group, 21 * 14)) != PP_OK) return st;
    if ((st = upload(&p->atom14_mask, tables->atom14_mask, 21 * 14)) != PP_OK) return st;
    if ((st = upload(&p->lit_positions, tables->lit_positions, 21 * 14 * 3)) != PP_OK) return st;
    if ((st = upload(&p->between_radius, tables->between_radius, 21 * 14)) != PP_OK) return st;
    float ext[21];
    side_chain_extents(tables, ext);
    if ((st = upload(&p->side_extent, ext, 21)) != PP_OK) return st;
    PP_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&p->bounds_lower), 21 * 14 * 14 * sizeof(float)));
    PP_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&p->bounds_upper), 21 * 14 * 14 * sizeof(float)));
    p->clash_params_set = false;
    *out = p.release();
    return PP_OK;
}

extern "C" void pp_plan_destroy(pp_plan *p) {
    if (!p) return;
    void *ptrs[] = {p->w, p->wT, p->default_frames, p->atom14_to_group, p->atom14_mask, p->lit_positions,
                    p->between_radius, p->bounds_lower, p->bounds_upper, p->ln_scale, p->side_extent};
    for (void *q : ptrs) if (q) (void)hipFree(q);
    for (const ArenaSlot &sl : p->arena_pool) {
        (void)hipFree(sl.p);
    }
    delete p;
}

extern "C" pp_status pp_plan_set_knn_ties(pp_plan *p, int mode) {
    if (!p) FAIL(PP_ERR_INVALID, "pp_plan_set_knn_ties: null plan");
    if (mode != PP_KNN_TIES_LOWER_INDEX && mode != PP_KNN_TIES_ATEN_CPU && mode != PP_KNN_TIES_ATEN_MEMBER)
        FAIL(PP_ERR_INVALID, "pp_plan_set_knn_ties: unknown mode " + std::to_string(mode));
    p->knn_ties = mode;
    return PP_OK;
}

extern "C" int pp_plan_rebalanced_chains(const pp_plan *p) { return p ? p->rebalanced_chains : -1; }
extern "C" int pp_plan_ln_scaled_features(const pp_plan *p) { return p ? p->ln_scaled_features : -1; }
// HOST helper, no device call: the five operand-scale vectors pp_plan_create would choose for these weights (after the ReLU-chain
// rebalancing), [h_E0 | h_E after layer 0 | after layer 1 | x1 of layer 0 | of layer 1] x 128; the exact-fp32 build returns ones
extern "C" pp_status pp_ln_operand_scales_host(const float *weights, size_t n_weights, float *out, int *n_scaled) {
    const WeightOff off = pp_weight_offsets();
    if (!weights || !out || n_weights != off.total) FAIL(PP_ERR_INVALID, "pp_ln_operand_scales_host: bad argument");
    int n = 0;
#ifdef PP_EDGE_F16
    const LnScales sc = ln_operand_scales(weights, off);
    std::memcpy(out, &sc.v[0][0], sizeof(sc.v));
    n = sc.n_scaled;
#else
    for (int i = 0; i < 5 * 128; i++) out[i] = 1.f;
#endif
    if (n_scaled) *n_scaled = n;
    return PP_OK;
}

// HOST helper, no device call: the weight vector as pp_plan_create packs it (split-f16 build: ReLU chains rebalanced by powers of
// two; exact-fp32 build: a copy).  Lets a CPU test hold the rebalanced network to the original one through the oracle.
extern "C" pp_status pp_rebalance_weights_host(const float *weights, size_t n_weights, float *out, int *chains) {
    const WeightOff off = pp_weight_offsets();
    if (!weights || !out || n_weights != off.total) FAIL(PP_ERR_INVALID, "pp_rebalance_weights_host: bad argument");
    memcpy(out, weights, n_weights * sizeof(float));
    int c = 0;
#ifdef PP_EDGE_F16
    {
        std::vector<float> plain, packed;
        LnScales sc;
        c = rewrite_checkpoint(weights, off, plain, packed, sc);      // (`plain`: the rebalanced network with the operand scales multiplied back)
        memcpy(out, plain.data(), n_weights * sizeof(float));
    }
#endif
    if (chains) *chains = c;
    return PP_OK;
}

// sample_cfg.annealed_temp (TorsionalDiffusion.py:70-75 -> SO2VESchedule(annealed_temp=...), schedule.py:205-208)
extern "C" pp_status pp_plan_set_annealed_temp(pp_plan *p, float T) {
    if (!p) FAIL(PP_ERR_INVALID, "pp_plan_set_annealed_temp: null plan");
    // schedule.py:216-217 tests `if self.annealed_temp`: 0 (and None, which the host side maps to 0) switch the annealing off
    if (!std::isfinite(T)) FAIL(PP_ERR_INVALID, "pp_plan_set_annealed_temp: annealed_temp must be finite (0 = no annealing)");
    p->annealed_temp = T;
    return PP_OK;
}

// torch.topk(values, k, largest=False) indices of ATen's CPU kernel (pp_topk_aten.h), on the host
extern "C" pp_status pp_topk_aten_host(const float *values, int n, int k, int32_t *idx_out) {
    if (!values || !idx_out || n < 1 || k < 1 || k > n) FAIL(PP_ERR_INVALID, "pp_topk_aten_host: bad argument");
    std::vector<pp_tk_pair> q((size_t)n);
    for (int j = 0; j < n; j++) { q[j].v = values[j]; q[j].i = j; }
    pp_tk_topk_smallest(q.data(), n, k);
    for (int j = 0; j < k; j++) idx_out[j] = q[j].i;
    return PP_OK;
}

extern "C" pp_status pp_plan_set_clash_params(pp_plan *p, float tol, const float *lower, const float *upper, void *stream) {
    if (!p || !lower || !upper) FAIL(PP_ERR_INVALID, "pp_plan_set_clash_params: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the host tables are caller-owned and may be freed on return: blocking copies
    PP_HIP_CHECK(hipStreamSynchronize(s));
    PP_HIP_CHECK(hipMemcpy(p->bounds_lower, lower, 21 * 14 * 14 * sizeof(float), hipMemcpyHostToDevice));
    PP_HIP_CHECK(hipMemcpy(p->bounds_upper, upper, 21 * 14 * 14 * sizeof(float), hipMemcpyHostToDevice));
    p->clash_tol = tol;
    p->clash_params_set = true;
    return PP_OK;
}

// ---------------------------------------------------------------------------------------------
extern "C" void pp_ctx_destroy(pp_ctx *c) {
    if (!c) return;
    if (c->arena) {                                   // every workspace pointer lives in this one allocation
        // hand it to the plan's pool instead of hipFree (which synchronises the device): a context per batch is created
        // and destroyed on the sampling path.  Work already enqueued on last_stream may still be using the memory; the
        // next owner either runs on the same stream (ordered after it) or waits for that stream first.
        pp_plan *p = c->plan;
        std::lock_guard<std::mutex> g(p->pool_mutex);
        if (p->arena_pool.size() < 4) {
            p->arena_pool.push_back({c->arena, c->arena_bytes, c->last_stream});
        } else {
            (void)hipFree(c->arena);
        }
    }
    for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
    if (c->obst) (void)hipFree(c->obst);              // waits for the device: only a context that ever held obstacles pays it
    pp_ctx_free_workspaces(c);                        // likewise: only a context that ever ran one of their entries
    delete c;
}

// the table of a padded batch [B][L]: complex s is rows s * L .. s * L + L - 1
__global__ void k_seg_uniform(int32_t *__restrict__ off, int n_seg, int L) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s <= n_seg) off[s] = s * L;
}
// (first row, length) of the complex every row belongs to, from the context's table (pp_segments.h pp_seg_fill: on the uniform
// table of a padded batch its clamps are no-ops and this is ((n / L) * L, L))
__global__ void k_fill_seg(int2 *__restrict__ seg, int N, const int32_t *__restrict__ off, int n_seg, int max_len) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int start, len;
    pp_seg_fill(off, n_seg, N, max_len, n, start, len);
    seg[n] = make_int2(start, len);
}

static pp_status prepare_impl(pp_plan *plan, const pp_batch *b, const int32_t *seg_offsets, int n_seg, int min_len,
                              int max_len, void *stream, pp_ctx **out) {
    const bool packed = seg_offsets != nullptr;
    if (!plan || !b || !out) FAIL(PP_ERR_INVALID, "pp_complex_prepare: null argument");
    if (b->B <= 0 || b->L <= 0) FAIL(PP_ERR_INVALID, "pp_complex_prepare: B and L must be positive");
    if ((packed ? max_len : b->L) > 16384) FAIL(PP_ERR_UNSUPPORTED, "pp_complex_prepare: L > 16384 residues per complex is not supported");
    if (packed) {
        if (b->B != 1) FAIL(PP_ERR_INVALID, "pp_complex_prepare_packed: the batch tensors are [1, sum of lengths, ...]");
        if (n_seg < 1 || min_len < 1 || max_len < min_len || (long long)n_seg * min_len > b->L || (long long)n_seg * max_len < b->L)
            FAIL(PP_ERR_INVALID, "pp_complex_prepare_packed: segment count / lengths do not fit the batch");
        // K = min(32, L) is a per-batch constant of the reference (encoder.py:115): complexes shorter than 32 residues
        // cannot share a context with longer ones.  A plan without network weights builds no graph and has no K: its structure
        // stages (shell, SASA, disulfides, polar, hydrogens, clashscore, hnet, refine) take segments of any lengths
        if (plan->has_network && min_len < PP_TOP_K && min_len != max_len)
            FAIL(PP_ERR_UNSUPPORTED, "pp_complex_prepare_packed: complexes shorter than 32 residues must be prepared on their own");
    }
    if (!b->X || !b->residue_type || !b->BB_D)
        FAIL(PP_ERR_INVALID, "pp_complex_prepare: batch needs at least X, residue_type and BB_D");
    const bool net = plan->has_network;
    if (net && (!b->atom_mask || !b->residue_mask || !b->residue_index || !b->chain_indices || !b->BB_D_sincos ||
                !b->SC_D_mask || !b->chi_1pi_periodic_mask || !b->chi_2pi_periodic_mask))
        FAIL(PP_ERR_INVALID, "pp_complex_prepare: batch has a null tensor pointer");
    PP_HIP_CHECK(hipSetDevice(plan->device));
    // value-initialised: every pointer null, prof_which = -1.  Every return below goes through pp_ctx_destroy.
    std::unique_ptr<pp_ctx, CtxDeleter> owner(new (std::nothrow) pp_ctx());
    if (!owner) FAIL(PP_ERR_INVALID, "out of host memory");
    pp_ctx *c = owner.get();
    c->plan = plan;
    c->b = *b;
    c->packed = packed;
    c->B = packed ? n_seg : b->B;
    c->L = packed ? max_len : b->L;
    c->N = b->B * b->L;
    const int shortest = packed ? min_len : b->L;
    c->K = shortest < PP_TOP_K ? shortest : PP_TOP_K;
    c->shortest = shortest;
    const size_t N = c->N, K = c->K;
    // one arena for all workspaces (a context per batch is created and destroyed on the sampling path: ~35 hipMalloc /
    // hipFree pairs cost 1.5 ms per context, one pair 0.1 ms): sizes first, then one hipMalloc, then the pointers
    struct Slot { void **p; size_t bytes; };
    std::vector<Slot> slots;
    size_t total = 0;
#define ALLOC(field, n) { const size_t bytes_ = (((n) ? (n) : 1) * sizeof(*c->field) + 255) & ~size_t(255);          \
                          slots.push_back({reinterpret_cast<void **>(&c->field), bytes_}); total += bytes_; }
    if (net) {
        ALLOC(eidx, N * K); ALLOC(mask_att, N * 32); ALLOC(frames, N * 12); ALLOC(bbpos, N * 15);
        ALLOC(hE0, N * K * 128); ALLOC(hE, N * K * 128); ALLOC(Znm, N * K * 128); ALLOC(Zem, N * K * 128); ALLOC(hV, N * 128); ALLOC(hV_alt, N * 128); ALLOC(S, N * 128); ALLOC(msum, N);
        ALLOC(ptsN, N * 48); ALLOC(PAn, N * 128); ALLOC(PCn, N * 128);
        ALLOC(ptsE, N * 48); ALLOC(PAe, N * 128); ALLOC(PCe, N * 128);
        ALLOC(score, N * 4); ALLOC(chi_tmp, N * 4);
        for (int k = 0; k < 2; k++) { ALLOC(live_rows[k], N + 2); ALLOC(live_mix[k], N); ALLOC(live_cnt[k], 1); }
    }
    ALLOC(xyz, N * 42); ALLOC(rec, N * 64); ALLOC(axes, N * 24); ALLOC(rec2, N * 64); ALLOC(axes2, N * 24); ALLOC(brad, N); ALLOC(per_res, N); ALLOC(dchi, N * 4);
    ALLOC(px, N * 4); ALLOC(pm, N * 4); ALLOC(pv, N * 4); ALLOC(pz, N * 4); ALLOC(pxeff, N * 4); ALLOC(pmask, N);
    // the proximal loop is defined for one complex (optimize.py:27): a B = 1 context, or every complex of a packed one (pp_proximal_packed)
    const bool prox = c->B == 1 || packed;
    if (prox) { ALLOC(cand, (size_t)N * 4 * PP_CL_CAP); ALLOC(cand_cnt, N * 4); }
    ALLOC(scal, 64);
    ALLOC(sat, 4);
    ALLOC(seg, N);
    ALLOC(prox_part, (size_t)PP_PROX_CHUNK * N);
    if (prox) { ALLOC(prox_nrows, c->B); ALLOC(prox_seg, c->B); ALLOC(prox_inv, N); }
    if (prox) { ALLOC(obst_seg, c->B); ALLOC(obst_row, N); ALLOC(obst_cand, (size_t)N * PP_OB_CAP); ALLOC(obst_cnt, N); }
    ALLOC(sasa_row, N * 8);
    ALLOC(seg_off, (size_t)c->B + 1);
    ALLOC(rng_tab, N); ALLOC(rng_keys, c->B);
    c->max_steps = 1 << 20;
#undef ALLOC
    c->last_stream = static_cast<hipStream_t>(stream);
    {
        std::lock_guard<std::mutex> g(plan->pool_mutex);
        int best = -1;
        for (int i = 0; i < (int)plan->arena_pool.size(); i++)
            if (plan->arena_pool[i].bytes >= total && (best < 0 || plan->arena_pool[i].bytes < plan->arena_pool[best].bytes)) best = i;
        if (best >= 0) {
            const ArenaSlot sl = plan->arena_pool[best];
            plan->arena_pool.erase(plan->arena_pool.begin() + best);
            if (sl.stream != c->last_stream) (void)hipStreamSynchronize(sl.stream);
            c->arena = sl.p;
            c->arena_bytes = sl.bytes;
        }
    }
    if (!c->arena && hipMalloc(&c->arena, total) != hipSuccess) {
        c->arena = nullptr;
        FAIL(PP_ERR_HIP, "hipMalloc of the context workspace failed");
    }
    if (!c->arena_bytes) c->arena_bytes = total;
    char *base = static_cast<char *>(c->arena);
    for (const Slot &sl : slots) { *sl.p = base; base += sl.bytes; }
    hipStream_t s_ = static_cast<hipStream_t>(stream);
    // the context's segment table, before anything reads it: a copy of the caller's (which need not outlive this call's stream
    // work), or 0, L, 2L ... written on the device -- nothing is staged, nothing waits
    if (packed) {
        if (hipMemcpyAsync(c->seg_off, seg_offsets, ((size_t)n_seg + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s_) != hipSuccess)
            FAIL(PP_ERR_HIP, "copying the segment offsets failed");
    } else {
        hipLaunchKernelGGL(k_seg_uniform, dim3((c->B + 256) / 256), dim3(256), 0, s_, c->seg_off, c->B, c->L);
    }
    hipLaunchKernelGGL(k_fill_seg, dim3((c->N + 255) / 256), dim3(256), 0, s_, c->seg, c->N, c->seg_off, c->B, c->L);
    if (hipGetLastError() != hipSuccess) FAIL(PP_ERR_HIP, "segment table launch failed");
    if (hipMemsetAsync(c->sat, 0, 4 * sizeof(unsigned), s_) != hipSuccess) FAIL(PP_ERR_HIP, "clearing the saturation word failed");
    if (net) {
        pp_status st;
        flag_nonfinite(c, c->b.X, 42, 12, s_);      // N, CA, C, O of the unmasked rows
        if ((st = pp_launch_prepare(c, s_)) != PP_OK) return st;
        if ((st = pp_launch_edge_static(c, s_)) != PP_OK) return st;
        if ((st = pp_launch_live_rows(c, 0, nullptr, s_)) != PP_OK) return st;
    }
    *out = owner.release();
    return PP_OK;
}

extern "C" pp_status pp_complex_prepare(pp_plan *plan, const pp_batch *b, void *stream, pp_ctx **out) {
    return prepare_impl(plan, b, nullptr, 0, 0, 0, stream, out);
}

extern "C" pp_status pp_complex_prepare_packed(pp_plan *plan, const pp_batch *b, const int32_t *seg_offsets, int n_seg,
                                               int min_len, int max_len, void *stream, pp_ctx **out) {
    if (!seg_offsets) FAIL(PP_ERR_INVALID, "pp_complex_prepare_packed: null segment offsets");
    return prepare_impl(plan, b, seg_offsets, n_seg, min_len, max_len, stream, out);
}

__global__ void k_widen_idx(const int32_t *__restrict__ src, int64_t *__restrict__ dst, size_t n, const int2 *__restrict__ seg, int K) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        size_t node = i / K;
        dst[i] = (int64_t)src[i] - (int64_t)seg[node].x;      // back to the per-complex residue numbering of the reference
    }
}

extern "C" pp_status pp_ctx_get_graph(pp_ctx *c, int64_t *E_idx, float *hE0, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);      // the copies below read the arena on `stream`
    if (!c) FAIL(PP_ERR_INVALID, "pp_ctx_get_graph: null ctx");
    if (!c->plan->has_network) FAIL(PP_ERR_INVALID, "pp_ctx_get_graph: plan was created without network weights");
    hipStream_t s = static_cast<hipStream_t>(stream);
    size_t n = (size_t)c->N * c->K;
    if (E_idx) hipLaunchKernelGGL(k_widen_idx, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c->eidx, E_idx, n, c->seg, c->K);
    if (hE0) PP_HIP_CHECK(hipMemcpyAsync(hE0, c->hE0, n * 128 * sizeof(float), hipMemcpyDeviceToDevice, s));
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}

extern "C" pp_status pp_ctx_set_graph(pp_ctx *c, const int64_t *E_idx, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !E_idx) FAIL(PP_ERR_INVALID, "pp_ctx_set_graph: null argument");
    if (!c->plan->has_network) FAIL(PP_ERR_INVALID, "pp_ctx_set_graph: plan was created without network weights");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    pp_status st = pp_launch_prepare(c, s, E_idx);
    if (st == PP_OK) st = pp_launch_edge_static(c, s);
    if (st != PP_OK) return st;
    int bad = 0;          // inspection-grade call: it validates the indices, which needs one read-back
    PP_HIP_CHECK(hipMemcpyAsync(&bad, c->scal, sizeof(int), hipMemcpyDeviceToHost, s));
    PP_HIP_CHECK(hipStreamSynchronize(s));
    if (bad) FAIL(PP_ERR_INVALID, "pp_ctx_set_graph: " + std::to_string(bad) + " neighbour indices outside their complex");
    return PP_OK;
}

// ---------------------------------------------------------------------------------------------
// per-step scalars (schedule.py:165-174,198-235; layers.py:257-268), fp32 like the reference's tensors
// sigma(t) in fp32 (TorsionalDiffusion.py:84-88): fill_step, the initial noising and the re-noising of pp_sample_partial share it
static float sigma_f32(float t) {
    const double lo = pp_log_sigma_min(), hi = pp_log_sigma_max();
    return expf((float)lo + (float)(hi - lo) * t);
}

static void fill_step(StepParams *sp, float t, float dt, float T) {
    const double PI_D = PP_PI_D, hi = pp_log_sigma_max();
    memset(sp, 0, sizeof(*sp));
    // sinusoidal embedding of t * 10000
    const float ts = t * 10000.0f;
    const float nemb = (float)(-(log(10000.0) / 7.0));
    for (int i = 0; i < 8; i++) {
        float freq = expf((float)i * nemb);
        float arg = ts * freq;
        sp->temb[i] = (float)sin((double)arg);
        sp->temb[8 + i] = (float)cos((double)arg);
    }
    float sigma = sigma_f32(t);
    float g = sigma * (float)sqrt(2.0 * log(PI_D / (0.01 * PI_D)));
    float ratio = sigma / (float)exp(hi);
    float alpha = 1.0f - ratio * ratio;
    sp->w = T != 0.f ? T / (alpha + (1.0f - alpha) * T) : 1.0f;      // schedule.py:216-217: a falsy annealed_temp means weight 1
    sp->c_ode = (0.5f * (g * g)) * dt;
    sp->c_drift = (g * g) * dt;
    sp->c_diff = g * sqrtf(dt);
}

// pp_profile_kernel: arm the launch of kernel class `which` that follows (the launcher's PP_LAUNCH takes the event pair)
static inline void prof_arm(pp_ctx *c, int which) { c->prof_armed = c->prof_which == which; }
static inline void prof_disarm(pp_ctx *c) { c->prof_armed = false; }
bool pp_prof_take(pp_ctx *c, hipEvent_t *e0, hipEvent_t *e1) {
    c->prof_armed = false;
    while (c->prof_ev.size() < c->prof_n + 2) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return false;
        c->prof_ev.push_back(e);
    }
    *e0 = c->prof_ev[c->prof_n++];
    *e1 = c->prof_ev[c->prof_n++];
    return true;
}

// The layer-1 edge update of a sampling run takes only the context's live rows.  PP_EDGE_LIVE=0 in the
// environment restores the launch over all rows -- read by every build: it is the A/B switch of the tests and the benchmark.
static bool edge_live_on() {
    static const char *e = getenv("PP_EDGE_LIVE");
    static const bool on = !(e && atoi(e) == 0);
    return on;
}

// ev: what the evaluation is given (pp_internal.h NodeEval)
// live (sampling runs, else null): the rows whose layer-1 edge update has a reader.  That launch makes h_E (not stored) and the
// layer-2 message S / msum of row i, which feed only the layer-2 node update of row i, whose h_V feeds only the decoder and the
// reverse step of row i: nothing of it reaches the returned angles of a row that cannot move (y = wrap(..) * SC_D_mask = 0, or
// the pinned value), and the next evaluation starts from a fresh embedding.  S / msum of a skipped row keep what THIS evaluation's
// layer-0 launch wrote there -- the row's layer-1 message, or the zeros of a masked row: finite values of the same run, never
// uninitialised memory -- and the layer-2 node update computes on them as on any other message.  What it computes for such a row is
// read by nobody, and it must not be reported either: k_node_update<PP_NU_STEP> leaves the rows that cannot move out of the sticky
// saturation word (pp_node.hip, `satrow`), so the word does not depend on which message a skipped row was given.
static pp_status run_network(pp_ctx *c, hipStream_t s, int last_mode, const NodeEval &ev, const PPLive *live) {
    pp_status st;
    for (int l = 0; l < 3; l++) {
        if (l == 0 || !pp_edge_fused()) {   // fused build: layers 1 and 2 come from the tail of the previous edge update
            prof_arm(c, 0);
            st = pp_launch_node_message(c, l, s);
            prof_disarm(c);
            if (st != PP_OK) return st;
        }
        prof_arm(c, 2);
        st = pp_launch_node_update(c, l, l < 2 ? PP_NU_MID : last_mode, ev, s);
        prof_disarm(c);
        if (st != PP_OK) return st;
        if (l < 2) {
            prof_arm(c, 1);
            st = pp_launch_edge_update(c, l, l == 0 || !pp_edge_fused(), s, l == 1 ? live : nullptr);   // layer 1's h_E has no reader here
            prof_disarm(c);
            if (st != PP_OK) return st;
        }
    }
    return PP_OK;
}

// the tail the single evaluations share: the three layers with the decoder (PP_NU_SCORE) on the embedded h_V, then the results out
// (`score` or `hV` may be null).  `sp`: PP_NU_SCORE reads no per-step scalar and no time embedding from it
static pp_status evaluate_and_copy(pp_ctx *c, const StepParams &sp, float *score, float *hV, hipStream_t s) {
    pp_status st;
    const NodeEval ev = {nullptr, 0, PP_MODE_ODE, nullptr, &sp, nullptr, nullptr, nullptr};
    if ((st = run_network(c, s, PP_NU_SCORE, ev, nullptr)) != PP_OK) return st;
    if (score) PP_HIP_CHECK(hipMemcpyAsync(score, c->score, (size_t)c->N * 4 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (hV) PP_HIP_CHECK(hipMemcpyAsync(hV, c->hV, (size_t)c->N * 128 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return PP_OK;
}

extern "C" pp_status pp_score(pp_ctx *c, const float *chi, float t, float *score, float *hV, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !chi || !score) FAIL(PP_ERR_INVALID, "pp_score: null argument");
    if (!c->plan->has_network) FAIL(PP_ERR_INVALID, "pp_score: plan was created without network weights");
    hipStream_t s = static_cast<hipStream_t>(stream);
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    StepParams sp;
    fill_step(&sp, t, 0.f, c->plan->annealed_temp);
    pp_status st;
    flag_nonfinite(c, chi, 4, 4, s);
    if ((st = pp_launch_node_embed(c, chi, sp, s)) != PP_OK) return st;
    return evaluate_and_copy(c, sp, score, hV, s);
}

// pp_score with a time per row: only the node embedding sees the time (columns 35..50 of encoder.node_embedding), so the
// sibling embedding kernel is the one difference; the MPNN, the decoder and every edge kernel are pp_score's.
extern "C" pp_status pp_score_rows(pp_ctx *c, const float *chi, const float *t_rows, float *score, float *hV, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !chi || !t_rows || !score) FAIL(PP_ERR_INVALID, "pp_score_rows: null argument");
    if (!c->plan->has_network) FAIL(PP_ERR_INVALID, "pp_score_rows: plan was created without network weights");
    hipStream_t s = static_cast<hipStream_t>(stream);
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    StepParams sp;
    fill_step(&sp, 0.f, 0.f, c->plan->annealed_temp);     // PP_NU_SCORE reads no per-step scalar and no time embedding
    pp_status st;
    flag_nonfinite(c, chi, 4, 4, s);
    flag_nonfinite(c, t_rows, 1, 1, s);
    if ((st = pp_launch_node_embed_rows(c, chi, t_rows, s)) != PP_OK) return st;
    return evaluate_and_copy(c, sp, score, hV, s);
}

extern "C" pp_status pp_affinity_encode(const pp_affinity *a, pp_ctx *c, const int64_t *residue_type, const float *sc_sincos,
                                        const int64_t *mut_mask, const float *hV_pret, float *hV, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!a || !c || !residue_type || !sc_sincos || !mut_mask || !hV_pret || !hV) FAIL(PP_ERR_INVALID, "pp_affinity_encode: null argument");
    if (!a->network) FAIL(PP_ERR_INVALID, "pp_affinity_encode: the affinity head was created for mode linear (no mutation branch)");
    if (!c->plan->has_network) FAIL(PP_ERR_INVALID, "pp_affinity_encode: plan was created without network weights");
    if (a->device != c->plan->device) FAIL(PP_ERR_INVALID, "pp_affinity_encode: affinity head and ctx are on different devices");
    hipStream_t s = static_cast<hipStream_t>(stream);
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    StepParams sp;
    fill_step(&sp, 0.f, 0.f, c->plan->annealed_temp);     // not read by the network: its time-embedding columns are zero
    pp_status st;
    if ((st = pp_launch_affinity_embed(c, a, residue_type, sc_sincos, mut_mask, hV_pret, s)) != PP_OK) return st;
    return evaluate_and_copy(c, sp, nullptr, hV, s);
}

// ---- seeded sampling noise (pp_rng.h) -----------------------------------------------------------------------------------------
// the per-row table with the default keys, if the context has none yet: one small launch, nothing waits
static pp_status rng_table_ready(pp_ctx *c, hipStream_t s) {
    return c->rng_tab_set ? PP_OK : pp_launch_rng_table(c, false, s);
}

extern "C" pp_status pp_ctx_set_rng_keys(pp_ctx *c, const uint64_t *keys, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c) FAIL(PP_ERR_INVALID, "pp_ctx_set_rng_keys: null ctx");
    hipStream_t s = static_cast<hipStream_t>(stream);
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    // the host table is caller-owned: from pageable memory, hipMemcpyAsync has taken the data when it returns (it may block)
    if (keys) PP_HIP_CHECK(hipMemcpyAsync(c->rng_keys, keys, (size_t)c->B * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    return pp_launch_rng_table(c, keys != nullptr, s);
}

extern "C" pp_status pp_noise_seeded(pp_ctx *c, uint64_t seed, int step, float *noise, uint32_t *words, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !noise) FAIL(PP_ERR_INVALID, "pp_noise_seeded: null argument");
    if (step < -1 || step >= c->max_steps) FAIL(PP_ERR_INVALID, "pp_noise_seeded: step must be -1 (initial noising) .. 2^20 - 1");
    hipStream_t s = static_cast<hipStream_t>(stream);
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    pp_status st;
    if ((st = rng_table_ready(c, s)) != PP_OK) return st;
    return pp_launch_noise_seeded(c, seed, step, noise, words, s);
}

extern "C" pp_status pp_add_noise_seeded(pp_ctx *c, const float *chi0, float t, uint64_t seed, float *chi, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !chi0 || !chi) FAIL(PP_ERR_INVALID, "pp_add_noise_seeded: null argument");
    if (!c->b.chi_1pi_periodic_mask || !c->b.chi_2pi_periodic_mask) FAIL(PP_ERR_INVALID, "pp_add_noise_seeded: batch lacks the periodic masks");
    hipStream_t s = static_cast<hipStream_t>(stream);
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    pp_status st;
    if ((st = rng_table_ready(c, s)) != PP_OK) return st;
    return pp_launch_add_noise_seeded(c, chi0, sigma_f32(t), seed, chi, s);
}

// What one sampling run is: the five exports fill one and call sample_impl.
struct SampleRun {
    const char *who;                    // the export, for messages
    const float *sde_noise = nullptr;   // pp_sample: the per-step noise tensor, or
    bool seeded = false;                // the reverse steps draw their own noise
    uint64_t seed = 0;                  //   from this seed
    const float *chi_ref = nullptr;     // the pin (partial repacking), or null: [N][4]
    const uint8_t *fixed = nullptr;     //   [N]: fixed rows are pinned inside the reverse step
    int fix_mode = PP_FIX_RENOISE;      //   PP_FIX_HOLD / PP_FIX_RENOISE
    const float *eta = nullptr;         // the guide, or null: HOST [n_schedule], the step size of nudge point j, 0 = none
    float cap = 0.f;                    //   largest |step| of one angle at one nudge
    double *trace = nullptr;            //   [B][n_schedule] or null
    float *chi_traj = nullptr;          // [n_schedule - 1][N][4] or null: written by the pinned step's lanes, copied in a run without a pin
    const float *snr = nullptr;         // the corrector, or null: HOST [n_schedule - 1], 0 = none behind reverse step j
    double *corr_trace = nullptr;       //   [B][n_schedule - 1][4] = (s2, n2, eps, amp) or null
};
static pp_status sample_impl(pp_ctx *c, float *chi, const float *schedule, int n_schedule, int mode, const SampleRun &run, hipStream_t s);

extern "C" pp_status pp_sample(pp_ctx *c, float *chi, const float *schedule, int n_schedule, int mode,
                               const float *sde_noise, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (c && mode == PP_MODE_SDE && !sde_noise) FAIL(PP_ERR_INVALID, "pp_sample: sde mode needs the per-step noise tensor");
    SampleRun run = {"pp_sample"};
    run.sde_noise = sde_noise;
    return sample_impl(c, chi, schedule, n_schedule, mode, run, static_cast<hipStream_t>(stream));
}

extern "C" pp_status pp_sample_seeded(pp_ctx *c, float *chi, const float *schedule, int n_schedule, int mode, uint64_t seed,
                                      void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    SampleRun run = {"pp_sample_seeded"};
    run.seeded = mode == PP_MODE_SDE;       // ode draws nothing: pp_sample
    run.seed = seed;
    return sample_impl(c, chi, schedule, n_schedule, mode, run, static_cast<hipStream_t>(stream));
}

extern "C" pp_status pp_sample_partial(pp_ctx *c, float *chi, const float *chi_ref, const uint8_t *fixed, int fix_mode,
                                       const float *schedule, int n_schedule, int mode, uint64_t seed, float *chi_traj,
                                       void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!chi_ref || !fixed) FAIL(PP_ERR_INVALID, "pp_sample_partial: null argument");
    SampleRun run = {"pp_sample_partial"};
    run.seeded = true;
    run.seed = seed;
    run.chi_ref = chi_ref; run.fixed = fixed; run.fix_mode = fix_mode;
    run.chi_traj = chi_traj;
    return sample_impl(c, chi, schedule, n_schedule, mode, run, static_cast<hipStream_t>(stream));
}

// ---- clash-guided sampling -----------------------------------------------------------------------------------
extern "C" pp_status pp_sample_guided(pp_ctx *c, float *chi, const float *chi_ref, const uint8_t *fixed, int fix_mode,
                                      const float *schedule, int n_schedule, int mode, uint64_t seed, const float *eta, float cap,
                                      float *chi_traj, double *clash_trace, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c) FAIL(PP_ERR_INVALID, "pp_sample_guided: null ctx");
    if (!chi) FAIL(PP_ERR_INVALID, "pp_sample_guided: null chi");
    if (!schedule) FAIL(PP_ERR_INVALID, "pp_sample_guided: null schedule");
    if (!eta) FAIL(PP_ERR_INVALID, "pp_sample_guided: null eta");
    if ((chi_ref == nullptr) != (fixed == nullptr))
        FAIL(PP_ERR_INVALID, "pp_sample_guided: chi_ref and fixed must be given together (both, or neither for a run without a pin)");
    SampleRun run = {"pp_sample_guided"};
    run.seeded = fixed != nullptr || mode == PP_MODE_SDE;          // ode without a pin draws nothing: pp_sample's instances
    run.seed = seed;
    run.chi_ref = chi_ref; run.fixed = fixed; run.fix_mode = fix_mode;
    run.eta = eta; run.cap = cap; run.trace = clash_trace;
    run.chi_traj = chi_traj;
    return sample_impl(c, chi, schedule, n_schedule, mode, run, static_cast<hipStream_t>(stream));
}

// ---- predictor-corrector sampling ----------------------------------------------------------------------------
extern "C" pp_status pp_sample_corrected(pp_ctx *c, float *chi, const float *chi_ref, const uint8_t *fixed, int fix_mode,
                                         const float *schedule, int n_schedule, int mode, uint64_t seed, const float *snr,
                                         const float *eta, float cap, float *chi_traj, double *clash_trace, double *corr_trace,
                                         void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c) FAIL(PP_ERR_INVALID, "pp_sample_corrected: null ctx");
    if (!chi) FAIL(PP_ERR_INVALID, "pp_sample_corrected: null chi");
    if (!schedule) FAIL(PP_ERR_INVALID, "pp_sample_corrected: null schedule");
    if (!snr) FAIL(PP_ERR_INVALID, "pp_sample_corrected: null snr");
    if ((chi_ref == nullptr) != (fixed == nullptr))
        FAIL(PP_ERR_INVALID, "pp_sample_corrected: chi_ref and fixed must be given together (both, or neither for a run without a pin)");
    SampleRun run = {"pp_sample_corrected"};
    run.seeded = fixed != nullptr || mode == PP_MODE_SDE;          // the reverse steps of ode without a pin draw nothing; the corrector draws
    run.seed = seed;
    run.chi_ref = chi_ref; run.fixed = fixed; run.fix_mode = fix_mode;
    run.eta = eta; run.cap = cap; run.trace = eta ? clash_trace : nullptr;
    run.chi_traj = chi_traj;
    run.snr = snr; run.corr_trace = corr_trace;
    return sample_impl(c, chi, schedule, n_schedule, mode, run, static_cast<hipStream_t>(stream));
}

// The argument checks of a run, each written once, in the one order that reports a call with several faults as every export always
// has: the exports with a pin or a guide name an unknown mode in front of the plan's and the schedule's faults, the other two behind.
static pp_status check_run(const pp_ctx *c, const float *chi, const float *schedule, int n_schedule, int mode, const SampleRun &run) {
    const std::string w(run.who);
    const bool pinned = run.fixed != nullptr, guided = run.eta != nullptr, corrected = run.snr != nullptr;
    const bool bad_mode = mode != PP_MODE_ODE && mode != PP_MODE_SDE;
    if (!c || !chi || !schedule) FAIL(PP_ERR_INVALID, w + ": null argument");
    if (pinned && run.chi_ref == chi) FAIL(PP_ERR_INVALID, w + ": chi_ref and chi must be distinct buffers");
    if (pinned && run.fix_mode != PP_FIX_HOLD && run.fix_mode != PP_FIX_RENOISE) FAIL(PP_ERR_INVALID, w + ": unknown fix_mode");
    if ((pinned || guided || corrected) && bad_mode) FAIL(PP_ERR_INVALID, w + ": unknown mode");
    if (pinned && !guided && (!c->b.chi_1pi_periodic_mask || !c->b.chi_2pi_periodic_mask))
        FAIL(PP_ERR_INVALID, w + ": batch lacks the periodic masks");
    if (!guided && !c->plan->has_network) FAIL(PP_ERR_INVALID, w + ": plan was created without network weights");
    if (n_schedule < 2) FAIL(PP_ERR_INVALID, w + ": schedule needs at least 2 times");
    if (corrected) {
        for (int j = 0; j < n_schedule - 1; j++)
            if (!(run.snr[j] >= 0.f) || std::isinf(run.snr[j]))
                FAIL(PP_ERR_INVALID, w + ": snr[" + std::to_string(j) + "] must be finite and not negative");
        if (!c->plan->has_network) FAIL(PP_ERR_INVALID, w + ": plan was created without network weights (a geometry-only plan)");
        if (!c->b.SC_D_mask || !c->b.chi_1pi_periodic_mask || !c->b.chi_2pi_periodic_mask)
            FAIL(PP_ERR_INVALID, w + ": batch lacks SC_D_mask / the periodic masks");
    }
    if (guided) {
        for (int j = 0; j < n_schedule; j++)
            if (!(run.eta[j] >= 0.f) || std::isinf(run.eta[j]))
                FAIL(PP_ERR_INVALID, w + ": eta[" + std::to_string(j) + "] must be finite and not negative");
        if (!(run.cap > 0.f)) FAIL(PP_ERR_INVALID, w + ": cap must be positive (INFINITY = no clamp)");
        if (!c->plan->has_network) FAIL(PP_ERR_INVALID, w + ": plan was created without network weights (a geometry-only plan)");
        if (!c->plan->clash_params_set) FAIL(PP_ERR_INVALID, w + ": call pp_plan_set_clash_params first");
        if (!c->b.atom_mask || !c->b.residue_index) FAIL(PP_ERR_INVALID, w + ": batch lacks atom_mask / residue_index");
        if (!c->b.SC_D_mask || !c->b.chi_1pi_periodic_mask || !c->b.chi_2pi_periodic_mask)
            FAIL(PP_ERR_INVALID, w + ": batch lacks SC_D_mask / the periodic masks");
        if (!c->packed && c->B != 1)
            FAIL(PP_ERR_INVALID, w + ": needs a context from pp_complex_prepare_packed (or a B = 1 one), not a padded B > 1 batch");
    }
    if (n_schedule - 1 > c->max_steps) FAIL(PP_ERR_UNSUPPORTED, w + ": more than 2^20 steps");
    if (bad_mode) FAIL(PP_ERR_INVALID, w + ": unknown mode");
    return PP_OK;
}

// the pin of reverse step j: a fixed row arrives at the noise level of schedule[j + 1] like the free rows; after the last step it
// holds chi_ref itself (sigma(0) = 0.01 pi is not 0)
static PPPin step_pin(const SampleRun &run, const float *schedule, int j, int nsteps, int N) {
    return {run.fixed, run.chi_ref, run.chi_traj ? run.chi_traj + (size_t)j * N * 4 : nullptr, sigma_f32(schedule[j + 1]),
            run.fix_mode == PP_FIX_RENOISE && j + 1 < nsteps ? 1 : 0};
}

// pp_sample, pp_sample_seeded, pp_sample_partial, pp_sample_guided and pp_sample_corrected
static pp_status sample_impl(pp_ctx *c, float *chi, const float *schedule, int n_schedule, int mode, const SampleRun &run, hipStream_t s) {
    pp_status st;
    if ((st = check_run(c, chi, schedule, n_schedule, mode, run)) != PP_OK) return st;
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    const bool pinned = run.fixed != nullptr, guided = run.eta != nullptr;
    const int nsteps = n_schedule - 1;
    // Corrected run: the corrector of reverse step j sits behind it (and its pin), in front of nudge point j + 1.  snr[j] == 0
    // enqueues nothing.  The corrector always draws, in ode mode too
    auto corr_at = [&](int j) { return run.snr != nullptr && run.snr[j] != 0.f; };
    bool corrected = false;
    for (int j = 0; j < nsteps; j++) corrected = corrected || corr_at(j);
    if ((run.seeded || corrected) && (st = rng_table_ready(c, s)) != PP_OK) return st;
    const PPRng rng = {c->rng_tab, (uint32_t)run.seed, (uint32_t)(run.seed >> 32)};
    // per-step scalars are kernel arguments: nothing is staged, nothing waits for the stream
    std::vector<StepParams> steps((size_t)nsteps);
    for (int j = 0; j < nsteps; j++) fill_step(&steps[j], schedule[j], schedule[j] - schedule[j + 1], c->plan->annealed_temp);
    // (A hipGraph replay of the loop was measured and dropped: with no stray event records in the stream the kernel
    // trace shows back-to-back dispatches, and capture + replay was 2 % slower than plain launches.)
    flag_nonfinite(c, chi, 4, 4, s);
    // Guided run: nudge point j < nsteps sits in front of evaluation j, nudge point nsteps behind the last reverse step.  A point with
    // eta == 0 enqueues nothing: the evaluation in front of it keeps its fused next-step embedding.  An evaluation followed by a nudge
    // drops it (next = nullptr): the angles the next evaluation embeds exist only behind the nudge, which the embedding launch follows.
    auto nudge_at = [&](int j) { return guided && run.eta[j] != 0.f; };
    auto nudge = [&](int j) { return pp_launch_guide_nudge(c, chi, run.fixed, run.eta[j], run.cap, run.trace, n_schedule, j, s); };
    if (guided) {
        if (run.trace) PP_HIP_CHECK(hipMemsetAsync(run.trace, 0xff, (size_t)c->B * n_schedule * sizeof(double), s));   // NaN
        bool any = false;
        for (int j = 0; j <= nsteps; j++) any = any || run.eta[j] != 0.f;
        if (any && (st = pp_launch_guide_begin(c, s)) != PP_OK) return st;
        if (nudge_at(0) && (st = nudge(0)) != PP_OK) return st;
    }
    if (run.corr_trace) PP_HIP_CHECK(hipMemsetAsync(run.corr_trace, 0xff, (size_t)c->B * nsteps * 4 * sizeof(double), s));   // NaN
    StepParams sp_end;                        // the corrector behind the last reverse step embeds at schedule[nsteps]
    if (corrected && corr_at(nsteps - 1)) fill_step(&sp_end, schedule[nsteps], 0.f, c->plan->annealed_temp);
    if (nudge_at(0)) prof_arm(c, 6);          // pp_profile_kernel(6): the embedding launch behind a nudge
    st = pp_launch_node_embed(c, chi, steps[0], s);
    prof_disarm(c);
    if (st != PP_OK) return st;
    static const bool dbg = PP_GETENV("PP_DEBUG") != nullptr;
    const auto h0 = std::chrono::steady_clock::now();
    // the live rows of this run: the context's, or without the call's fixed rows (made here, on the stream).  The in-situ timing
    // runs of pp_profile_kernel launch all rows (their rates are quoted per row of the context)
    PPLive live = {nullptr, nullptr};
    const bool use_live = edge_live_on() && pp_edge_fused() && c->prof_which < 0;
    if (use_live) {
        const int set = pinned ? 1 : 0;
        if (pinned && (st = pp_launch_live_rows(c, 1, run.fixed, s)) != PP_OK) return st;
        live.rows = c->live_rows[set];
        live.mix = c->live_mix_set[set] ? c->live_mix[set] : nullptr;      // null: not filled, the mixed launch refuses it
    }
    for (int j = 0; j < nsteps; j++) {
        const PPPin pin = pinned ? step_pin(run, schedule, j, nsteps, c->N) : PPPin{nullptr, nullptr, nullptr, 0.f, 0};
        const bool then_corr = corr_at(j), then_nudge = nudge_at(j + 1);
        // an evaluation followed by a corrector or a nudge drops its fused embedding: the angles evaluation j + 1 embeds exist only
        // behind them, and the corrector's own evaluation starts from pp_score's embedding launch (below)
        const NodeEval ev = {chi, j, mode, run.sde_noise, &steps[j], j + 1 < nsteps && !then_corr && !then_nudge ? &steps[j + 1] : nullptr,
                             run.seeded ? &rng : nullptr, pinned ? &pin : nullptr};
        if ((st = run_network(c, s, PP_NU_STEP, ev, use_live ? &live : nullptr)) != PP_OK) return st;
        if (run.chi_traj && !pinned)
            PP_HIP_CHECK(hipMemcpyAsync(run.chi_traj + (size_t)j * c->N * 4, chi, (size_t)c->N * 4 * sizeof(float),
                                        hipMemcpyDeviceToDevice, s));
        if (then_corr) {
            // the score at the new state and time: pp_score's launch sequence, the embedding launch included (all rows, no fused
            // embedding behind it) -- the bits of pp_score(ctx, chi, schedule[j + 1]) behind any step.  The embedding the reverse step
            // could fuse is the same function in the matrix pipe's arithmetic, not the same bits.  Then the update in one launch
            const StepParams &sp = j + 1 < nsteps ? steps[j + 1] : sp_end;
            if ((st = pp_launch_node_embed(c, chi, sp, s)) != PP_OK) return st;
            const NodeEval evs = {nullptr, 0, PP_MODE_ODE, nullptr, &sp, nullptr, nullptr, nullptr};
            if ((st = run_network(c, s, PP_NU_SCORE, evs, nullptr)) != PP_OK) return st;
            prof_arm(c, 7);                   // pp_profile_kernel(7): k_correct
            st = pp_launch_correct(c, chi, run.fixed, run.snr[j], j, nsteps, rng, run.corr_trace, s);
            prof_disarm(c);
            if (st != PP_OK) return st;
        }
        if (then_nudge && (st = nudge(j + 1)) != PP_OK) return st;
        if ((then_corr || then_nudge) && j + 1 < nsteps) {      // the angles evaluation j + 1 embeds exist only now
            if (then_nudge) prof_arm(c, 6);
            st = pp_launch_node_embed(c, chi, steps[j + 1], s);
            prof_disarm(c);
            if (st != PP_OK) return st;
        }
    }
    if (dbg) {
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - h0).count();
        fprintf(stderr, "[pp] pp_sample: host enqueue of %d steps took %.0f us (%.1f us per step)\n", nsteps, us, us / nsteps);
    }
    return PP_OK;
}

extern "C" pp_status pp_atom14(pp_ctx *c, const float *chi, float *xyz, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !chi || !xyz) FAIL(PP_ERR_INVALID, "pp_atom14: null argument");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    return pp_launch_atom14(c, chi, xyz, static_cast<hipStream_t>(stream));
}

extern "C" pp_status pp_clash(pp_ctx *c, const float *chi, float *per_res, float *dchi, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !chi || !per_res) FAIL(PP_ERR_INVALID, "pp_clash: null argument");
    if (!c->plan->clash_params_set) FAIL(PP_ERR_INVALID, "pp_clash: call pp_plan_set_clash_params first");
    if (!c->b.atom_mask || !c->b.residue_index) FAIL(PP_ERR_INVALID, "pp_clash: batch lacks atom_mask / residue_index");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    pp_status st;
    if ((st = pp_launch_atom14(c, chi, c->xyz, s)) != PP_OK) return st;
    return pp_launch_clash(c, c->xyz, per_res, dchi, s);
}

extern "C" pp_status pp_proximal(pp_ctx *c, const float *chi, float lamda, int num_steps, float *chi_traj,
                                 float *chi_last, float *losses, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !chi || !losses) FAIL(PP_ERR_INVALID, "pp_proximal: null argument");
    if (c->B != 1) FAIL(PP_ERR_INVALID, "pp_proximal: batch.num_proteins must be 1 (optimize.py:27); optimise the complexes of a packed or padded batch one by one");
    if (num_steps < 1) FAIL(PP_ERR_INVALID, "pp_proximal: num_steps must be >= 1");
    if (!c->plan->clash_params_set) FAIL(PP_ERR_INVALID, "pp_proximal: call pp_plan_set_clash_params first");
    if (!c->b.atom_mask || !c->b.residue_index) FAIL(PP_ERR_INVALID, "pp_proximal: batch lacks atom_mask / residue_index");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    return pp_launch_proximal(c, chi, lamda, num_steps, chi_traj, chi_last, losses, static_cast<hipStream_t>(stream));
}

// ---- obstacle atoms ----------------------------------------------------------------------------------------
// the context's copy of the caller's atoms; a non-finite coordinate or radius, or a negative radius, sets bit 2 of the sticky word
__global__ void k_obst_copy(const float4 *__restrict__ src, float4 *__restrict__ dst, int M, unsigned *__restrict__ sat) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= M) return;
    const float4 q = src[o];
    dst[o] = q;
    const float big = 3.402823466e38f;
    const bool fin = __builtin_fabsf(q.x) <= big && __builtin_fabsf(q.y) <= big && __builtin_fabsf(q.z) <= big && __builtin_fabsf(q.w) <= big;
    if (!fin || q.w < 0.f) atomicOr(sat, 4u);
}
// obst_row[n] = the range of the segment row n belongs to
__global__ void k_obst_rows(int N, const int32_t *__restrict__ off, int n_seg, const int2 *__restrict__ oseg, int2 *__restrict__ orow) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < N) orow[n] = oseg[pp_seg_of_row(off, n_seg, n)];
}

extern "C" pp_status pp_ctx_set_obstacles(pp_ctx *c, const float *xyzr, const int32_t *seg_range, int M, void *stream) {
    if (!c) FAIL(PP_ERR_INVALID, "pp_ctx_set_obstacles: null ctx");
    c->last_stream = static_cast<hipStream_t>(stream);
    if (!c->packed && c->B != 1)
        FAIL(PP_ERR_INVALID, "pp_ctx_set_obstacles: needs a context from pp_complex_prepare_packed (or a B = 1 one), not a padded B > 1 batch");
    if (M < 0) FAIL(PP_ERR_INVALID, "pp_ctx_set_obstacles: M must not be negative");
    if (M == 0 || !xyzr) {          // clear: the launchers go back to the instances without obstacles; the allocation stays for the next set
        c->obst_M = 0;
        return PP_OK;
    }
    if (!seg_range) FAIL(PP_ERR_INVALID, "pp_ctx_set_obstacles: null seg_range");
    for (int s = 0; s < c->B; s++) {
        const long long first = seg_range[2 * s], count = seg_range[2 * s + 1];
        if (first < 0 || count < 0 || first + count > M)
            FAIL(PP_ERR_INVALID, "pp_ctx_set_obstacles: the range of segment " + std::to_string(s) + " (" + std::to_string(first) + ", " +
                                     std::to_string(count) + ") lies outside the " + std::to_string(M) + " atoms");
    }
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (M > c->obst_cap) {
        // a larger copy: hipFree waits for the device, so nothing enqueued can still read the old one (the only wait of this call, and
        // only when the set grows)
        if (c->obst) (void)hipFree(c->obst);
        c->obst = nullptr;
        c->obst_cap = 0;
        c->obst_M = 0;
        PP_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&c->obst), (size_t)M * sizeof(float4)));
        c->obst_cap = M;
    }
    // the host table is caller-owned: from pageable memory, hipMemcpyAsync has taken the data when it returns
    PP_HIP_CHECK(hipMemcpyAsync(c->obst_seg, seg_range, (size_t)c->B * sizeof(int2), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_obst_copy, dim3((M + 255) / 256), dim3(256), 0, s, reinterpret_cast<const float4 *>(xyzr), c->obst, M, c->sat);
    hipLaunchKernelGGL(k_obst_rows, dim3((c->N + 255) / 256), dim3(256), 0, s, c->N, c->seg_off, c->B, c->obst_seg, c->obst_row);
    PP_HIP_CHECK(hipGetLastError());
    c->obst_M = M;
    return PP_OK;
}

// pp_proximal_packed and pp_proximal_pinned (`who` names the export in messages; fixed == nullptr: no pin)
static pp_status proximal_packed_impl(const char *who, pp_ctx *c, const float *chi, const uint8_t *fixed, float lamda, int num_steps,
                                      const int32_t *norm_rows, float *chi_traj, float *chi_last, float *chi_accepted, float *losses,
                                      uint8_t *moved, void *stream) {
    const std::string w(who);
    if (!c->packed && c->B != 1)
        FAIL(PP_ERR_INVALID, w + ": needs a context from pp_complex_prepare_packed (or a B = 1 one), not a padded B > 1 batch");
    if (num_steps < 1) FAIL(PP_ERR_INVALID, w + ": num_steps must be >= 1");
    if (!c->plan->clash_params_set) FAIL(PP_ERR_INVALID, w + ": call pp_plan_set_clash_params first");
    if (!c->b.atom_mask || !c->b.residue_index) FAIL(PP_ERR_INVALID, w + ": batch lacks atom_mask / residue_index");
    // every complex is at least c->shortest rows long (min_len; for an unpacked B = 1 context: N): an entry below that is shorter
    // than its complex for sure (the exact lengths are on the device only; the kernels take max(entry, length))
    const int shortest = c->shortest;
    if (norm_rows)
        for (int s = 0; s < c->B; s++)
            if (norm_rows[s] < shortest)
                FAIL(PP_ERR_INVALID, w + ": norm_rows[" + std::to_string(s) + "] = " + std::to_string(norm_rows[s]) +
                                         " is below the shortest complex (" + std::to_string(shortest) + " rows)");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the host table is caller-owned: from pageable memory, hipMemcpyAsync has taken the data when it returns
    if (norm_rows) PP_HIP_CHECK(hipMemcpyAsync(c->prox_nrows, norm_rows, (size_t)c->B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    return pp_launch_proximal_packed(c, chi, lamda, num_steps, norm_rows != nullptr, chi_traj, chi_last, chi_accepted, losses, s, fixed,
                                     moved);
}

extern "C" pp_status pp_proximal_packed(pp_ctx *c, const float *chi, float lamda, int num_steps, const int32_t *norm_rows,
                                        float *chi_traj, float *chi_last, float *chi_accepted, float *losses, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !chi || !chi_last || !chi_accepted || !losses) FAIL(PP_ERR_INVALID, "pp_proximal_packed: null argument");
    return proximal_packed_impl("pp_proximal_packed", c, chi, nullptr, lamda, num_steps, norm_rows, chi_traj, chi_last, chi_accepted,
                                losses, nullptr, stream);
}

extern "C" pp_status pp_proximal_pinned(pp_ctx *c, const float *chi, const uint8_t *fixed, float lamda, int num_steps,
                                        const int32_t *norm_rows, float *chi_traj, float *chi_last, float *chi_accepted,
                                        float *losses, uint8_t *moved, void *stream) {
    if (c) c->last_stream = static_cast<hipStream_t>(stream);
    if (!c || !chi || !fixed || !chi_last || !chi_accepted || !losses) FAIL(PP_ERR_INVALID, "pp_proximal_pinned: null argument");
    return proximal_packed_impl("pp_proximal_pinned", c, chi, fixed, lamda, num_steps, norm_rows, chi_traj, chi_last, chi_accepted,
                                losses, moved, stream);
}

// Measurement aid (bench.py): average duration of one launch of a hot kernel, timed with HIP events on
// `stream` around `iters` back-to-back launches.  which: 0 = node message, 1 = edge update (layer 1 weights; the instance
// that sampling runs, which does not write h_E back in the fused build).
// The ctx must have been through pp_score / pp_sample so that its state buffers hold real activations.
extern "C" pp_status pp_time_kernel(pp_ctx *c, int which, int iters, float *avg_ms, void *stream) {
    if (!c || !avg_ms || iters < 1) FAIL(PP_ERR_INVALID, "pp_time_kernel: bad argument");
    if (!c->plan->has_network) FAIL(PP_ERR_INVALID, "pp_time_kernel: plan was created without network weights");
    hipStream_t s = static_cast<hipStream_t>(stream);
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    if (PP_GETENV("PP_DEBUG")) {
        int a = 0, b = 0;
        pp_edge_occupancy(&a, &b);
        fprintf(stderr, "[pp] resident workgroups/CU: k_node_message %d, k_edge_update %d\n", a, b);
    }
    hipEvent_t e0, e1;
    PP_HIP_CHECK(hipEventCreate(&e0));
    PP_HIP_CHECK(hipEventCreate(&e1));
    pp_status st = PP_OK;
    for (int w = 0; w < 2 && st == PP_OK; w++) st = which == 0 ? pp_launch_node_message(c, 0, s) : pp_launch_edge_update(c, 1, !pp_edge_fused(), s);
    PP_HIP_CHECK(hipEventRecord(e0, s));
    for (int i = 0; i < iters && st == PP_OK; i++) st = which == 0 ? pp_launch_node_message(c, 0, s) : pp_launch_edge_update(c, 1, !pp_edge_fused(), s);
    PP_HIP_CHECK(hipEventRecord(e1, s));
    PP_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    PP_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *avg_ms = ms / (float)iters;
    return st;
}

// Diagnostics -- libpackppi_hip.dbg.so only (-DPP_DIAG; tools/debug and the per-layer parity test): run single launches or a
// prefix of one network evaluation, read or restore an internal buffer.  Declared in include/packppi_hip.h under PP_DIAG.
#ifdef PP_DIAG
extern "C" pp_status pp_debug_edge(pp_ctx *c, int layer, void *stream) {
    if (!c || !c->plan->has_network) FAIL(PP_ERR_INVALID, "pp_debug_edge: bad ctx");
    return pp_launch_edge_update(c, layer, true, static_cast<hipStream_t>(stream));
}
extern "C" pp_status pp_debug_nm(pp_ctx *c, int layer, void *stream) {
    if (!c || !c->plan->has_network) FAIL(PP_ERR_INVALID, "pp_debug_nm: bad ctx");
    return pp_launch_node_message(c, layer, static_cast<hipStream_t>(stream));
}
extern "C" pp_status pp_debug_set_hE(pp_ctx *c, const float *src, size_t n) {
    if (!c || !src) FAIL(PP_ERR_INVALID, "pp_debug_set_hE: null");
    PP_HIP_CHECK(hipMemcpy(c->hE, src, n * sizeof(float), hipMemcpyDeviceToDevice));
    return PP_OK;
}
// which: 0 h_E, 1 S, 2 msum, 3 h_E0, 4 Z_em, 5 h_V, 6 score, 7 cand_cnt [N][4] (the int32 bits in the 4-byte slots: what the last
// proximal call's k_clash_cand left), 8 the plan's side_extent [21], 9 obst_cnt [N] (int32 bits: what its k_obst_cand left)
extern "C" pp_status pp_debug_buffer(pp_ctx *c, int which, float *dst, size_t n) {
    if (!c || !dst) FAIL(PP_ERR_INVALID, "pp_debug_buffer: null");
    const float *src = which == 0 ? c->hE : which == 1 ? c->S : which == 2 ? c->msum : which == 3 ? c->hE0 : which == 4 ? c->Zem :
                       which == 6 ? c->score : c->hV;
    if (which == 7 || which == 8 || which == 9) {
        src = which == 7 ? reinterpret_cast<const float *>(c->cand_cnt) : which == 9 ? reinterpret_cast<const float *>(c->obst_cnt) : c->plan->side_extent;
        if (!src) FAIL(PP_ERR_INVALID, "pp_debug_buffer: this context has no candidate lists");
        if (n > (which == 7 ? (size_t)c->N * 4 : which == 9 ? (size_t)c->N : (size_t)21)) FAIL(PP_ERR_INVALID, "pp_debug_buffer: n is larger than the table");
    }
    PP_HIP_CHECK(hipDeviceSynchronize());
    PP_HIP_CHECK(hipMemcpy(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice));
    return PP_OK;
}
// The first `n_launches` kernel launches of one network evaluation at time t (pp_score's schedule: node embedding, then
// NM0, NU0, EU0(+NM1), NU1, EU1(+NM2), NU2): after 1 + 2 the layer-0 h_V is in place, after 1 + 3 the layer-0 h_E, after
// 1 + 4 / 1 + 5 the same of layer 1, after 1 + 6 the final h_V (mpnn.py:47-62, layers.py:119-148).
extern "C" pp_status pp_debug_score_prefix(pp_ctx *c, const float *chi, float t, int n_launches, void *stream) {
    if (!c || !chi || !c->plan->has_network) FAIL(PP_ERR_INVALID, "pp_debug_score_prefix: bad argument");
    if (!pp_edge_fused()) FAIL(PP_ERR_UNSUPPORTED, "pp_debug_score_prefix: needs the fused edge update");
    hipStream_t s = static_cast<hipStream_t>(stream);
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    StepParams sp;
    fill_step(&sp, t, 0.f, c->plan->annealed_temp);
    pp_status st = PP_OK;
    int k = 0;
    auto more = [&]() { return st == PP_OK && k++ < n_launches; };
    const NodeEval ev = {nullptr, 0, PP_MODE_ODE, nullptr, &sp, nullptr, nullptr, nullptr};
    if (more()) st = pp_launch_node_embed(c, chi, sp, s);
    if (more()) st = pp_launch_node_message(c, 0, s);
    for (int l = 0; l < 3; l++) {
        if (more()) st = pp_launch_node_update(c, l, l < 2 ? PP_NU_MID : PP_NU_SCORE, ev, s);
        if (l < 2 && more()) st = pp_launch_edge_update(c, l, true, s);     // every h_E stays readable
    }
    return st;
}
// Which kernel instances the launches of a network evaluation run for this context's row count, from the launchers' own
// predicates: out = {R, mixed, n_pairs, cl, multi} -- residues per edge / node-message workgroup, the mixed pair + single launch and
// its pair count (0 when not mixed), workgroups per tile of a middle-layer node update, the node update's more-tiles-than-CUs instance.
extern "C" pp_status pp_debug_launch_plan(pp_ctx *c, int32_t out[5]) {
    if (!c || !out) FAIL(PP_ERR_INVALID, "pp_debug_launch_plan: null");
#ifdef PP_EDGE_F16
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    int R = 0, mixed = 0, n_pairs = 0, cl = 0, multi = 0;
    pp_status st = pp_edge_launch_plan(c->N, &R, &mixed, &n_pairs);
    if (st == PP_OK) st = pp_node_launch_plan(c->N, &cl, &multi);
    if (st != PP_OK) return st;
    out[0] = R; out[1] = mixed; out[2] = n_pairs; out[3] = cl; out[4] = multi;
    return PP_OK;
#else
    FAIL(PP_ERR_UNSUPPORTED, "pp_debug_launch_plan: the split-f16 edge kernels only");
#endif
}
#endif

// Measurement aid (bench.py): in-situ duration of one hot kernel.  After pp_profile_kernel(ctx, which) every launch of
// that kernel inside pp_score / pp_sample carries a start / stop HIP event pair (hipExtLaunchKernelGGL: the
// dispatch's own begin and end timestamps);
// pp_profile_read synchronises, sums the pair intervals, reports (total ms, launches) and switches profiling off.
extern "C" pp_status pp_profile_kernel(pp_ctx *c, int which) {
    if (!c || which < 0 || which > 7)
        FAIL(PP_ERR_INVALID, "pp_profile_kernel: which must be 0 (node message), 1 (edge update), 2 (node update), 3 (the Adam-step launch of pp_proximal / pp_proximal_packed / pp_proximal_pinned: clash + gradient + step + reconstruction), 4, 5, 6 (the launches of a nudge of pp_sample_guided: reconstruction, clash + gradient + step, node embedding) or 7 (the corrector launch of pp_sample_corrected)");
    c->prof_which = which;
    c->prof_n = 0;
    return PP_OK;
}

extern "C" pp_status pp_profile_read(pp_ctx *c, float *total_ms, int *launches) {
    if (!c || !total_ms || !launches) FAIL(PP_ERR_INVALID, "pp_profile_read: null argument");
    PP_HIP_CHECK(hipSetDevice(c->plan->device));
    double tot = 0.0;
    size_t pairs = c->prof_n / 2;
    if (pairs) PP_HIP_CHECK(hipEventSynchronize(c->prof_ev[2 * pairs - 1]));
    for (size_t i = 0; i < pairs; i++) {
        float ms = 0.f;
        PP_HIP_CHECK(hipEventElapsedTime(&ms, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
        tot += ms;
    }
    *total_ms = (float)tot;
    *launches = (int)pairs;
    c->prof_which = -1;
    c->prof_n = 0;
    return PP_OK;
}
