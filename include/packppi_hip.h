/*
 * packppi_hip.h -- C ABI of the MI355X (gfx950) side-chain sampling path.
 *
 * The reference (Jackz915/PackPPI) is pure Python/PyTorch and has no FFI; the entry points
 * below are what a binding for its hot path binds.  Each one names the
 * reference call it replaces (paths relative to the upstream repo root).
 *
 * Conventions
 *   - every `const float*` / `int64_t*` argument that is not marked HOST is a caller-owned,
 *     contiguous DEVICE pointer (e.g. torch.Tensor.data_ptr() of a ROCm tensor);
 *   - all floating data is fp32, indices are int64 (as in the reference batch object);
 *   - `stream` is a hipStream_t passed as void*; work is enqueued asynchronously on it and the
 *     library never synchronises the device, except where stated;
 *   - no exceptions cross the ABI: calls return pp_status, pp_last_error() gives the message
 *     of the calling thread's most recent failure;
 *   - a pp_ctx is not thread-safe; different ctxs may be driven from different threads;
 *   - a pp_ctx may be driven on one stream now and on another later, but the library orders nothing between two streams: a call
 *     on stream B sees what an earlier call on stream A left in the ctx only if the caller has ordered B behind A (an event
 *     wait, a synchronisation).  The one ordering the library does itself is the workspace hand-over of pp_ctx_destroy.
 *     tests/test_streams_gpu.py runs every stream-taking entry on a busy non-default stream.
 */
#ifndef PACKPPI_HIP_H
#define PACKPPI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pp_status {
    PP_OK = 0,
    PP_ERR_INVALID = 1,     /* bad argument / shape */
    PP_ERR_HIP = 2,         /* a HIP runtime call failed */
    PP_ERR_UNSUPPORTED = 3, /* valid request this build does not implement */
    PP_ERR_NO_DEVICE = 4    /* no gfx950 device visible */
} pp_status;

typedef struct pp_plan pp_plan; /* weights + chemistry tables resident on one GPU */
typedef struct pp_ctx pp_ctx;   /* one batch of complexes: cached graph, frames, workspaces */

#define PP_N_WEIGHTS 1439172u /* fp32 parameters of the score network (112 tensors) */
#define PP_HIDDEN 128
#define PP_TOP_K 32
#define PP_MODE_ODE 0
#define PP_MODE_SDE 1
/* What the neighbour search does where two CA distances of a row are exactly equal (pp_plan_set_knn_ties). */
#define PP_KNN_TIES_LOWER_INDEX 0 /* the residue with the lower index first                                          */
#define PP_KNN_TIES_ATEN_CPU 1    /* default: the choice AND order of torch.topk on CPU (the reference CPU path)       */
#define PP_KNN_TIES_ATEN_MEMBER 2 /* that choice only where it decides membership (rank K == rank K+1), else lower index */

/* Residue-chemistry tables (HOST pointers; values of src/utils/residue_constants.py:595-677). */
typedef struct pp_tables {
    const float *default_frames;   /* [21,8,4,4] restype_rigid_group_default_frame           */
    const int32_t *atom14_to_group;/* [21,14]    restype_atom14_to_rigid_group               */
    const float *atom14_mask;      /* [21,14]    restype_atom14_mask                         */
    const float *lit_positions;    /* [21,14,3]  restype_atom14_rigid_group_positions        */
    const float *between_radius;   /* [21,14]    vdW radius table of clash.py:263-287        */
} pp_tables;

/* The reference `batch` object (complex_dataset.py:123-139, complex_datamodule.py:205-224). */
typedef struct pp_batch {
    int32_t B, L;
    const float *X;                /* [B,L,14,3] */
    const float *atom_mask;        /* [B,L,14]   */
    const int64_t *residue_type;   /* [B,L]      */
    const float *residue_mask;     /* [B,L]      */
    const int64_t *residue_index;  /* [B,L]      */
    const int64_t *chain_indices;  /* [B,L]      */
    const float *BB_D;             /* [B,L,3]    */
    const float *BB_D_sincos;      /* [B,L,3,2]  */
    const float *SC_D;             /* [B,L,4]    */
    const float *SC_D_mask;        /* [B,L,4]    */
    const uint8_t *chi_1pi_periodic_mask; /* [B,L,4] bool */
    const uint8_t *chi_2pi_periodic_mask; /* [B,L,4] bool */
} pp_batch;

int pp_version(void);
const char *pp_last_error(void);

/* Build stamp: "<sources>-<flags>", two 16-digit hex prefixes of the SHA-256 of (a) every .hip / .h file of packppi_amd/csrc
 * plus this header, (b) the compiler flags, as computed by packppi_amd/build.py when the library was compiled.  The Python
 * binding refuses a library whose <sources> part differs from the sources on disk (a stale prebuilt .so). */
const char *pp_build_id(void);

/* Replaces TDiffusionModule.__init__ + load_from_checkpoint (TorsionalDiffusion.py:22-82,
 * eval_diffusion.py:29-41).  `weights` is a HOST buffer holding the 112 state_dict tensors
 * concatenated in the order of packppi_amd/weights.py::weight_spec(), nn.Linear [out,in].
 * weights == NULL gives a geometry-only plan (pp_atom14 / pp_clash / pp_proximal, the
 * checkpoint-free path of src/proximal_optimize.py); its batches need only X, residue_type,
 * BB_D and, for the clash calls, atom_mask and residue_index. */
pp_status pp_plan_create(const float *weights, size_t n_weights, const pp_tables *tables, int device,
                         pp_plan **plan);
void pp_plan_destroy(pp_plan *plan);

/* Replaces rc.make_atom14_dists_bounds(tol, vtf) as consumed by find_sc_violations
 * (clash.py:299-308): `lower`/`upper` are HOST [21,14,14] tables for these parameters.  The tables are
 * caller-owned and may be freed on return, so this call waits for `stream` and copies them synchronously
 * (the one blocking call besides the measurement aids; it runs once per parameter set, not per batch). */
pp_status pp_plan_set_clash_params(pp_plan *plan, float overlap_tolerance, const float *lower,
                                   const float *upper, void *stream);

/* ProteinEncoder._dist takes torch.topk(D_adjust, K, largest=False) (encoder.py:105-118), which leaves the choice between
 * exactly equal distances to the implementation -- and on ideal-geometry or 0.001-Angstrom-grid coordinates equal distances
 * do occur (about one row in five of the synthetic complexes has an order tie, one complex in thirty a membership tie at rank
 * K / K+1, which changes the graph).  PP_KNN_TIES_ATEN_CPU (the default) reproduces the reference CPU path: rows that hold a
 * tie among their K+1 smallest values are redone on the device with the selection ATen's CPU topk makes (std::nth_element +
 * std::sort, or std::partial_sort when 64 K <= L, of libstdc++ over (value, index) pairs with a value-only comparator;
 * csrc/pp_topk_aten.h).  Applies to contexts prepared afterwards. */
pp_status pp_plan_set_knn_ties(pp_plan *plan, int mode);

/* Replaces sample_cfg.annealed_temp as TDiffusionModule.__init__ hands it to both SO2VESchedule instances
 * (TorsionalDiffusion.py:70-75; configs/model/sample_cfg/Sampling.yaml:4, default 3): the T of the annealed weight
 * w = T / (alpha + (1 - alpha) T) in SO2VESchedule.step (schedule.py:216-217); 0 = no annealing, w = 1 (the reference's
 * `if self.annealed_temp`: a Sampling.yaml with `annealed_temp: 0` or `null`).  Applies to later pp_score / pp_sample calls. */
pp_status pp_plan_set_annealed_temp(pp_plan *plan, float annealed_temp);

/* No reference counterpart.  The split-f16 build rebalances every ReLU chain of the edge-level MLPs by powers of two when the
 * plan is created (W1, b1 times s; W2 divided by s: the same function, hidden activations of size O(1) whatever the checkpoint's
 * split of scale between consecutive layers; csrc/pp_api.hip rebalance_relu_chains): this returns how many of the 15 chains
 * were rescaled (0 for weights whose layer row norms lie within [1/8, 8], e.g. the seeded fixtures; always 0 in
 * libpackppi_hip.f32.so, which needs no such care), -1 for a null plan. */
int pp_plan_rebalanced_chains(const pp_plan *plan);
/* HOST helper, no device call: `out` [n_weights] = the weight vector as pp_plan_create packs it (the rebalanced one in the
 * split-f16 build, a copy in libpackppi_hip.f32.so), `chains` (may be NULL) = how many chains were rescaled.  For tests: the
 * rebalanced network must be the original function (tests/test_host.py runs both through the CPU oracle). */
pp_status pp_rebalance_weights_host(const float *weights, size_t n_weights, float *out, int *chains);

/* No reference counterpart.  Three LayerNorm outputs become f16 operands of the edge-level dense layers: h_E0 (encoder.norm_edges,
 * encoder.py:243-244), the h_E a layer writes and x1 (norm[3], norm[2]: layers.py:128-146).  Where a feature's gain and bias are
 * both far from 1 (a checkpoint that keeps the scale in the consuming weights) the split-f16 build multiplies that operand feature
 * by a power of two before the split and divides the consuming weight column by it when the plan is created -- exact, and only then
 * are the kernel instances with that multiply launched (csrc/pp_rebalance.h ln_operand_scales).  Returns how many of the 5 x 128
 * operand features carry a scale other than 1 (0 for the seeded fixtures; always 0 in libpackppi_hip.f32.so), -1 for a null plan. */
int pp_plan_ln_scaled_features(const pp_plan *plan);
/* HOST helper, no device call: `out` [5][128] = the operand scales pp_plan_create would choose for these weights, in the order
 * h_E0 | h_E after layer 0 | after layer 1 | x1 of layer 0 | of layer 1; `n_scaled` (may be NULL) = how many differ from 1. */
pp_status pp_ln_operand_scales_host(const float *weights, size_t n_weights, float *out, int *n_scaled);

/* HOST helper, no device call: idx_out[0..k-1] = torch.topk(values[0..n-1], k, largest=False) indices as ATen's CPU kernel
 * returns them -- the same code the neighbour search runs on the device for rows with ties.  Returns PP_OK / PP_ERR_INVALID. */
pp_status pp_topk_aten_host(const float *values, int n, int k, int32_t *idx_out);

/* Replaces the timestep-invariant part of ProteinEncoder.forward (encoder.py:198-246):
 * kNN graph, 468-d edge features, edge embedding + LayerNorm, backbone frames.  The batch
 * pointers must stay valid for the lifetime of the ctx.
 * The complexes of a padded batch [B][L] are its B rows, padding rows included: the ctx describes them by the same kind
 * of segment table a packed ctx has (below), here 0, L, 2L ..., which it writes itself.  Every per-complex quantity (noise
 * keys, loss segments, proximal means) is computed from that table by the same code for both kinds of ctx.
 * A ctx keeps all its device workspaces in one allocation that pp_ctx_destroy hands back to the plan
 * (a pool of up to four) instead of freeing it: creating a ctx per batch costs no hipMalloc/hipFree.
 * pp_ctx_destroy does not wait for work already enqueued on the ctx's stream; the next ctx that takes
 * the workspace over either runs on that same stream (ordered behind it) or synchronises with it first.
 * pp_plan_destroy frees the pool: destroy the plan's contexts, and let their work finish, before it. */
pp_status pp_complex_prepare(pp_plan *plan, const pp_batch *batch, void *stream, pp_ctx **ctx);
void pp_ctx_destroy(pp_ctx *ctx);

/* The same for complexes of different lengths WITHOUT the padding rows of collate_fn
 * (complex_datamodule.py:196-226): the batch tensors are [1, sum of lengths, ...] with the complexes'
 * rows back to back, `seg_offsets` (DEVICE, int32 [n_seg + 1], caller-owned like the batch; the ctx keeps a copy, the
 * caller's need not outlive the stream work of this call) gives the first
 * row of every complex and the total, min_len / max_len their shortest and longest length.  Neighbour
 * search, clash partners and E_idx numbering stay inside each complex; every other stage is per row or per
 * edge.  Results equal those of each complex prepared on its own (K = min(32, length): complexes shorter
 * than 32 residues cannot be mixed with longer ones -> PP_ERR_UNSUPPORTED; a plan without network weights builds
 * no graph, has no K and takes segments of any lengths).  pp_proximal needs one complex
 * per ctx; pp_proximal_packed optimises every complex of a packed ctx at once.  CONTRACT: the device table must describe the batch (seg_offsets[0] = 0, seg_offsets[n_seg] = the number of rows,
 * every length within [min_len, max_len]): the library sizes its launches from min_len / max_len and cannot read the table
 * back without stalling the stream; a table that disagrees is clamped where that is cheap, but the behaviour is undefined. */
pp_status pp_complex_prepare_packed(pp_plan *plan, const pp_batch *batch, const int32_t *seg_offsets, int n_seg,
                                    int min_len, int max_len, void *stream, pp_ctx **ctx);

/* Inspection (tests): copy out E_idx [B,L,K] and the embedded edges h_E0 [B,L,K,128]; K = min(32,L).  The copies are enqueued on
 * `stream`; the call does not wait for them. */
pp_status pp_ctx_get_graph(pp_ctx *ctx, int64_t *E_idx, float *hE0, void *stream);

/* Replace the ctx's neighbour lists by the caller's E_idx [B,L,K] (per-complex numbering, as
 * ProteinEncoder._dist returns them, encoder.py:105-118) and redo the edge embedding: for callers who want
 * another tie convention than the two the search offers (e.g. the lists of the reference's GPU path).
 * Validates the indices (one read-back: the call waits for `stream`). */
pp_status pp_ctx_set_graph(pp_ctx *ctx, const int64_t *E_idx, void *stream);

/* Replaces TDiffusionModule.network(batch, SC_D_noised, t) (TorsionalDiffusion.py:90-109) for a
 * timestep shared by all residues.  score [B,L,4]; hV [B,L,128] may be NULL. */
pp_status pp_score(pp_ctx *ctx, const float *chi, float t, float *score, float *hV, void *stream);

/* The same with a timestep PER ROW: t_rows is a DEVICE array [B*L] (packed ctx: [N]).  This is what the denoising
 * score-matching loss calls (TorsionalDiffusion.py:126-137 draws one t per complex).  Only the node embedding sees the time; its
 * 16 sinusoidal features of t_rows[n] * 10000 (layers.py:257-264) are computed on the device the way pp_score computes them on
 * the host, so a constant t_rows gives the bits pp_score gives.  t_rows is not modified (the reference's in-place `*= 10000` is
 * a side effect its own forward never observes).  A non-finite t_rows on an unmasked row sets bit 2 of pp_ctx_saturated. */
pp_status pp_score_rows(pp_ctx *ctx, const float *chi, const float *t_rows, float *score, float *hV, void *stream);

/* Replaces the loop of TDiffusionModule.sampling (TorsionalDiffusion.py:259-280):
 * chi [B,L,4] holds the initial noised angles on entry and the sample on exit.
 * `schedule` is a HOST array of n_schedule times (n_schedule-1 network evaluations); it is read before the
 * call returns, and the per-step scalars derived from it travel as kernel arguments (no staging copy, no wait).
 * mode PP_MODE_SDE needs `sde_noise` [n_schedule-1, 2, B*L, 4] (the two N(0,1) draws of
 * schedule.py:225 per step, 1pi schedule first); NULL is allowed for PP_MODE_ODE. */
pp_status pp_sample(pp_ctx *ctx, float *chi, const float *schedule, int n_schedule, int mode,
                    const float *sde_noise, void *stream);

/* ---- Seeded sampling noise, generated on the device (no reference counterpart) ---------------------
 * The reference draws its noise from torch's global generator over the rows of the whole batch (add_sc_noise,
 * TorsionalDiffusion.py:111-124; torch.normal in SO2VESchedule.step, schedule.py:225).  These calls draw it from a counter-based
 * generator instead -- Philox4x32-10, key = the 64-bit seed, counter = (row WITHIN the complex, 4 * (step + 1) + chi index,
 * complex key lo, hi), words (0, 1) -> the 1pi schedule's N(0,1) draw, (2, 3) -> the 2pi schedule's; step = -1 is the initial
 * noising (csrc/pp_rng.h holds the layout and the normal transform).  The draw is a pure function of (seed, complex key, row in
 * complex, chi, step, schedule): a complex gets the same noise alone, anywhere in a packed batch, on any rank.  This is NOT
 * torch's stream: parity with the reference's SDE step stays with pp_sample and its explicit noise tensor.
 *
 * pp_ctx_set_rng_keys: the 64-bit keys of the ctx's segments (the complexes of a packed ctx, the B rows of a padded one);
 * `keys` is a HOST array [n_seg], read before the call returns (the call may block on that copy; it runs once per ctx, not per
 * sample); NULL restores the default, which also holds if this is never called: a segment's key is its ordinal 0, 1, 2 ... */
pp_status pp_ctx_set_rng_keys(pp_ctx *ctx, const uint64_t *keys, void *stream);

/* What the seeded sampler draws at `step` (-1: the initial noising; 0 .. n_steps - 1: the reverse steps): noise [2,B*L,4], the
 * 1pi draw then the 2pi draw -- one step's slice of pp_sample's sde_noise -- and, if not NULL, words [B*L,4,4], the four raw
 * Philox words of every (row, chi).  The per-step noise hook: a caller may stream explicit noise step by step from it. */
pp_status pp_noise_seeded(pp_ctx *ctx, uint64_t seed, int step, float *noise, uint32_t *words, void *stream);

/* Replaces add_sc_noise (TorsionalDiffusion.py:111-124) at a time t shared by all rows, with the step = -1 draws z1, z2:
 * x = chi0 + (z1 sigma(t)) m1; x = x + (z2 sigma(t)) m2; chi = (x + pi) mod 2 pi - pi (torch.remainder semantics), every
 * operation rounded in fp32 as the reference's tensor operations round; m1 / m2 are the batch's 1pi / 2pi periodic masks.  An
 * entry outside both masks receives no noise and is copied through bit for bit.  chi0, chi [B,L,4], distinct buffers. */
pp_status pp_add_noise_seeded(pp_ctx *ctx, const float *chi0, float t, uint64_t seed, float *chi, void *stream);

/* pp_sample with the SDE draws made inside the reverse step, by the lane that steps (residue, chi): no noise tensor, no staging,
 * and the call never waits for the stream.  Bit-equal to pp_sample on the stack of pp_noise_seeded(step = 0 .. n_schedule - 2).
 * In PP_MODE_ODE nothing is drawn: the call is pp_sample. */
pp_status pp_sample_seeded(pp_ctx *ctx, float *chi, const float *schedule, int n_schedule, int mode, uint64_t seed,
                           void *stream);

/* ---- Partial repacking (no reference counterpart) ---------------------------------------------------
 * pp_sample_seeded with some rows held at given angles: fixed is a DEVICE array [B*L] (packed ctx: [N]) of bytes, 1 = the row keeps
 * chi_ref, 0 = the row is sampled; chi_ref is DEVICE [B*L,4], distinct from chi.  The pin sits inside the reverse step, in the
 * lane that steps (residue, chi), so the network of the next step sees the pinned value.  After step j (0-based) of the
 * n = n_schedule - 1 steps:
 *   free row                   today's step: the ODE formula or the SDE formula with the in-kernel draws, wrap, * SC_D_mask --
 *                              with fixed all 0 the call gives the bits of pp_sample_seeded in either mode;
 *   fixed row, PP_FIX_HOLD     chi_ref, bit for bit, at every step: the free rows are conditioned on the clean neighbours;
 *   fixed row, PP_FIX_RENOISE  j < n - 1: pp_add_noise_seeded's arithmetic on chi_ref with the step-j draws (z1, z2) of that
 *                              (row, chi) -- which a row that does not step leaves unused -- at sigma(schedule[j + 1]), the level
 *                              the free rows arrive at: x = chi_ref + (z1 sigma) m1; x = x + (z2 sigma) m2; wrap, every operation
 *                              rounded on its own; an entry outside both periodic masks is chi_ref bit for bit.  j = n - 1:
 *                              chi_ref bit for bit whatever the schedule ends at (sigma(0) = 0.01 pi is not 0).  This is
 *                              replacement conditioning: the network sees the known part at the noise level of its input.
 * INITIAL STATE: the call does not initialise fixed rows.  chi holds the step-0 state of EVERY row on entry -- for PP_FIX_RENOISE
 * pp_add_noise_seeded(where(fixed, chi_ref, .), t = schedule[0]) gives it, for PP_FIX_HOLD the fixed rows then set to chi_ref --
 * and the sample on exit, fixed rows = chi_ref.  The seed and the ctx's rng keys are used exactly as in pp_sample_seeded, in
 * PP_MODE_ODE too (the free rows draw nothing there; the re-noising does).  chi_traj, if not NULL, receives the angles after every
 * step [n_schedule-1, B*L, 4], written by the stepping lanes.  Never waits for the stream.  PP_ERR_INVALID: a null argument,
 * chi_ref == chi, an unknown fix_mode or mode, a batch without the periodic masks. */
#define PP_FIX_HOLD 0
#define PP_FIX_RENOISE 1
pp_status pp_sample_partial(pp_ctx *ctx, float *chi, const float *chi_ref, const uint8_t *fixed, int fix_mode,
                            const float *schedule, int n_schedule, int mode, uint64_t seed,
                            float *chi_traj /* [n_schedule-1, B*L, 4] or NULL */, void *stream);

/* ---- Clash-guided sampling (no reference counterpart) ------------------------------------------------
 * pp_sample_seeded (chi_ref and fixed NULL) or pp_sample_partial (both given) with a gradient step on the clash loss between the
 * network evaluations.  With n = n_schedule - 1 there are n + 1 nudge points: point j < n in front of evaluation j, point n behind
 * the last reverse step.  At a point with eta[j] != 0, on the current angles x:
 *   1. atom records at x, as pp_clash builds them;
 *   2. G[r][k] = d/d chi_{r,k} of the sum over the rows i of r's segment of per_res_i(x): pp_clash's value and gradient in fp32
 *      with its masks, exclusions and parameters and the obstacle term of a ctx that holds a set (pp_ctx_set_obstacles), the 1 / N
 *      of its mean replaced by exactly 1 -- a row's weight is 1 / (nsc + 1e-10) whatever else the ctx holds.  No float atomics,
 *      pp_clash's fixed summation order;
 *   3. an entry (r, k) is movable iff it is in the 1pi or the 2pi periodic mask, SC_D_mask != 0, row r is not fixed and G is finite:
 *      d = eta[j] * G;  d = fminf(fmaxf(d, -cap), cap);  x' = wrap_pi(x - d) * SC_D_mask, every operation rounded in fp32, wrap_pi
 *      the reverse step's ((x + pi) mod 2 pi - pi, torch.remainder semantics).  Every other entry keeps its bits;
 *   4. clash_trace[s][j] (if not NULL) = the fp64 sum of per_res over segment s at x -- BEFORE the step -- divided by the segment's
 *      length, summed in a fixed tree: the scale of pp_ensemble_reduce's clash.  Entries with eta[j] == 0 are NaN: nothing is
 *      computed there.
 * Evaluation j and today's reverse step (ODE or SDE formula, the seeded in-kernel draws, the pin with either fix mode) then run
 * from x'.  chi_traj[j] (DEVICE [n_schedule-1, N, 4] or NULL) is the state after reverse step j, in front of nudge j + 1; the
 * returned chi includes nudge n.  Fixed rows are never nudged and end as chi_ref bit for bit; under PP_FIX_RENOISE a free row's
 * gradient sees the fixed rows as they are at that moment.  With eta all zero the call gives the bits of pp_sample_seeded /
 * pp_sample_partial and clash_trace is all NaN.
 *   eta  HOST [n_schedule], read before the call returns;  cap > 0, INFINITY = no clamp.
 * Cost: the static partner and obstacle candidate lists of the proximal loop are built once per call; a point with eta[j] == 0
 * enqueues nothing; a nudge is two launches (reconstruction; clash + gradient + step in the residue's own workgroup) plus the node
 * embedding launch of the next evaluation, which the evaluation in front of the nudge then does not fuse, plus one small launch
 * for the trace when it is asked for.  Never waits for the stream, reads nothing back.  The call uses the proximal loop's
 * workspaces: do not overlap it with pp_proximal* or pp_ensemble_recombine on the same ctx.
 * PP_ERR_INVALID: a null ctx, chi, schedule or eta; only one of chi_ref and fixed; chi_ref == chi; an unknown mode or (with a pin)
 * fix_mode; eta[j] negative or not finite; cap <= 0 or NaN; no pp_plan_set_clash_params before; a batch without atom_mask,
 * residue_index, SC_D_mask or the periodic masks; a padded B > 1 ctx; a geometry-only plan. */
pp_status pp_sample_guided(pp_ctx *ctx, float *chi, const float *chi_ref /* or NULL */,
                           const uint8_t *fixed /* or NULL: both or neither */, int fix_mode, const float *schedule,
                           int n_schedule, int mode, uint64_t seed, const float *eta /* HOST [n_schedule] */, float cap,
                           float *chi_traj /* DEVICE [n_schedule-1,N,4] or NULL */,
                           double *clash_trace /* DEVICE [n_seg][n_schedule] or NULL */, void *stream);

/* ---- Predictor-corrector sampling (SO2VESchedule.step_correct, schedule.py:238-273, which the reference's own sampling() never
 * calls; csrc/pp_correct.hip holds the arithmetic) ------------------------------------------------------------
 * pp_sample_seeded / pp_sample_partial (chi_ref and fixed given) / pp_sample_guided (eta given) with one Langevin corrector behind
 * every reverse step j of the n = n_schedule - 1 whose snr[j] != 0.  It runs on the state x after reverse step j and its pin, at
 * t' = schedule[j + 1]:
 *   1. s = the network's score at (x, t'), the bits of pp_score(ctx, x, t'): all rows, one more evaluation;
 *   2. an entry (r, k) is movable iff it is in the 1pi or the 2pi periodic mask, SC_D_mask != 0, row r is not fixed and s is finite;
 *   3. z[r][k] = the N(0,1) draw of words (0, 1) of the seeded generator's counter at step 2^20 + j (the reverse steps use
 *      0 .. 2^20 - 1, the initial noising -1: disjoint ranges; words 2, 3 unused), in PP_MODE_ODE too: the corrector always draws;
 *   4. per segment of the ctx's segment table  s2 = sum (double)s^2,  n2 = sum (double)z^2  over its movable entries, fp64 in an
 *      order that depends on (row in the complex, k) only, no atomics: the same bits alone, padded or anywhere in a packed batch;
 *   5. eps = (float)(2 snr[j]^2 n2 / s2) (fp64 until the cast),  amp = (float)sqrt(2 (double)eps): step_correct's step size and noise
 *      amplitude for ONE complex.  A segment without a movable entry, with s2 == 0 or with eps or amp not finite has no corrector
 *      at this point: its entries keep their bits;
 *   6. movable entries:  y = x + eps s;  y = y + amp z;  x' = wrap_pi(y) * SC_D_mask, every product and sum rounded in fp32, wrap_pi
 *      the reverse step's.  Every other entry keeps its bits; fixed rows are never moved and never counted.
 * Nudge j + 1 (if eta is given and eta[j + 1] != 0), the node embedding of evaluation j + 1 and that evaluation follow.
 * NOT the reference to the letter: step_correct averages the two norms over the complexes of the batch and forms one step size,
 * and it is called per periodic mask; here every complex has its own step size -- the same thing for one complex, and the only
 * choice under which batching does not change a result -- and one corrector covers both masks.
 *   snr         HOST [n_schedule - 1], read before the call returns; finite, not negative; 0 = no corrector behind that step;
 *   eta         HOST [n_schedule] or NULL = no guide (cap, clash_trace and pp_sample_guided's preconditions then do not apply);
 *   chi_traj    (or NULL) the state after reverse step j, IN FRONT OF corrector j; the returned chi includes the last corrector
 *               and nudge;
 *   corr_trace  (or NULL) DEVICE fp64 [n_seg][n_schedule - 1][4] = (s2, n2, eps, amp); NaN where snr[j] == 0 or the segment has no
 *               corrector.
 * Always seeded: seed and the ctx's rng keys as in pp_sample_seeded.  With snr all zero the call gives the bits of pp_sample_guided
 * / pp_sample_partial / pp_sample_seeded with the same arguments and corr_trace is all NaN.  Works on packed, B = 1 and padded
 * B > 1 contexts (with eta: the guide's restriction).  Cost of a corrected step: one evaluation, one launch of one workgroup per
 * segment, and the node embedding launch of the next evaluation, which the reverse step in front can no longer fuse.  Never waits
 * for the stream, reads nothing back.
 * PP_ERR_INVALID: a null ctx, chi, schedule or snr; only one of chi_ref and fixed; chi_ref == chi; an unknown mode or (with a pin)
 * fix_mode; snr[j] negative or not finite; a batch without SC_D_mask or the periodic masks; a geometry-only plan; with eta,
 * everything pp_sample_guided refuses. */
pp_status pp_sample_corrected(pp_ctx *ctx, float *chi, const float *chi_ref /* or NULL */,
                              const uint8_t *fixed /* or NULL: both or neither */, int fix_mode, const float *schedule,
                              int n_schedule, int mode, uint64_t seed, const float *snr /* HOST [n_schedule-1] */,
                              const float *eta /* HOST [n_schedule] or NULL */, float cap,
                              float *chi_traj /* DEVICE [n_schedule-1,N,4] or NULL */, double *clash_trace /* or NULL */,
                              double *corr_trace /* DEVICE [n_seg][n_schedule-1][4] = (s2, n2, eps, amp) or NULL */,
                              void *stream);

/* Replaces get_atom14_coords(X, S, BB_D, SC_D) (components/__init__.py:76-120). xyz [B,L,14,3]. */
pp_status pp_atom14(pp_ctx *ctx, const float *chi, float *xyz, void *stream);

/* Replaces compute_residue_clash (clash.py:335-365) with the parameters last given to
 * pp_plan_set_clash_params.  per_res [B,L]; dchi, if not NULL, receives
 * d(mean over all B*L residues of per_res)/dchi [B,L,4] (the autograd of optimize.py:62-63). */
pp_status pp_clash(pp_ctx *ctx, const float *chi, float *per_res, float *dchi, void *stream);

/* Replaces proximal_optimizer(batch, SC_D, vtf, tol, lamda, num_steps) (optimize.py:21-73),
 * B must be 1.  chi_traj, if not NULL, receives the per-step angles [num_steps,1,L,4];
 * chi_last [1,L,4] the last of them; losses (DEVICE, [num_steps]) the pre-step loss values. */
pp_status pp_proximal(pp_ctx *ctx, const float *chi, float lamda, int num_steps, float *chi_traj,
                      float *chi_last, float *losses, void *stream);

/* proximal_optimizer for EVERY complex of a packed batch at once (a ctx from pp_complex_prepare_packed; a B = 1
 * ctx counts as one complex, a padded B > 1 ctx gives PP_ERR_INVALID).  Each complex keeps the reference's
 * per-complex semantics (optimize.py:5-73): its own mean-clash mask, its own 1/n in the loss and the gradient,
 * its own loss list and accept rule -- the bits pp_proximal gives that complex on its own ctx.  One launch per
 * Adam step for all complexes, no host read-back.
 * norm_rows (HOST int32 [n_seg], read before the call returns, or NULL): the row count each complex's means
 * divide by; NULL = its length.  The reference (and pp_proximal on a padded B = 1 batch) divides by the padded
 * max_size, while batch.pack drops the trailing padding rows: they add exact zeros to every sum (zero angles
 * there), so with norm_rows = the padded lengths the results equal the per-complex runs on the padded batches.
 * An entry below min_len gives PP_ERR_INVALID.  CONTRACT: every entry >= its complex's length (the lengths are on
 * the device only; the kernels use max(entry, length)).
 * chi [1,N,4]; chi_traj (or NULL) [num_steps,1,N,4]; chi_last [1,N,4] the last step; chi_accepted [1,N,4] per
 * complex chi_last where losses[s][num_steps-1] < losses[s][0], else chi (TorsionalDiffusion.py:296-298, decided
 * on the device); losses (DEVICE) [n_seg][num_steps] the pre-step loss values.  Memory: the ctx of a packed
 * batch holds the static clash-partner lists of the loop, 1.5 KB per row. */
pp_status pp_proximal_packed(pp_ctx *ctx, const float *chi, float lamda, int num_steps, const int32_t *norm_rows,
                             float *chi_traj, float *chi_last, float *chi_accepted, float *losses, void *stream);

/* The proximal stage of partial repacking (no reference counterpart): pp_proximal_packed with some rows
 * pinned.  fixed is a DEVICE array [N] of bytes, the `fixed` of pp_sample_partial: 1 = the row keeps its incoming angles, 0 = the
 * row is free.  It is the reference's optimiser (optimize.py:5-73) with SC_D_clash_mask & ~fixed in place of SC_D_clash_mask at
 * optimize.py:29 and nothing else changed.  Per complex of the ctx:
 *   1. the clash statistic is unchanged: per_res at the incoming angles, its mean over ALL rows of the complex, fixed ones
 *      included, with the divisor of pp_proximal_packed (norm_rows, or the length) -- a repacked shell is judged against the
 *      whole complex (optimize.py:5-18);
 *   2. moved[g] = per_res[g] > mean && !fixed[g]: only these rows get z = chi, Adam state and steps (optimize.py:31,47-51); every
 *      other row, fixed or not, is evaluated at chi and comes out as chi bit for bit in every slice of chi_traj, in chi_last and
 *      in chi_accepted (optimize.py:34-35,69);
 *   3. loss, gradient and accept rule are unchanged: anchor term + lamda * mean clash over the whole complex (optimize.py:33-45;
 *      a free atom overlapping a fixed one counts through both residues' per_res), accepted per complex where
 *      losses[s][num_steps-1] < losses[s][0], on the device.
 * With fixed all 0 every output has the bits of pp_proximal_packed.  ctx, norm_rows, chi, chi_traj, chi_last, chi_accepted and
 * losses as in pp_proximal_packed (a packed ctx or a B = 1 one; a padded B > 1 ctx gives PP_ERR_INVALID); moved (DEVICE [N] bytes,
 * or NULL) receives the mask of rule 2.  Waits for the stream no more than pp_proximal_packed does.  PP_ERR_INVALID: a null ctx,
 * chi, fixed, chi_last, chi_accepted or losses (without a pin, call pp_proximal_packed), num_steps < 1. */
pp_status pp_proximal_pinned(pp_ctx *ctx, const float *chi, const uint8_t *fixed /* DEVICE [N] */, float lamda,
                             int num_steps, const int32_t *norm_rows, float *chi_traj, float *chi_last,
                             float *chi_accepted, float *losses, uint8_t *moved /* DEVICE [N] or NULL */, void *stream);

/* ---- Obstacle atoms (no reference counterpart) -------------------------------------------------------------
 * Fixed spheres -- the heavy atoms of ligands, cofactors, nucleic acids, modified residues -- that the side chains of a segment must
 * not overlap.  A segment is a complex of a packed ctx, or the one complex of a B = 1 ctx.  With a set installed, pp_clash, the three
 * pp_proximal* calls and pp_ensemble_recombine add, for every row i of a segment, every own atom a in slots 4..13 with
 * exists * radius = r_a != 0 and every obstacle o of that segment with r_o > 0,
 *     err = max((r_a + r_o) - tol - sqrt(1e-10 + |p_a - q_o|^2), 0)        (fp32, tol of pp_plan_set_clash_params)
 * to atom a's loss sum: it enters per_res[i] = sum_{a >= 4}(...) / (nsc + 1e-10) beside the between-residue and within-residue sums.
 * No exclusions: backbone slots never take part, there is no slot-5 rule and no peptide rule.  Only p_a moves: the gradient gains
 * -w_i / d (p_a - q_o), pushed through the chi axes like every other force.  Everything built on per_res and dchi (the clash mask,
 * the Adam step, the loss list and accept rule, the `moved` mask, pp_ensemble_reduce on that per_res) carries the term unchanged.
 * ANCHOR: take a complex of chains A and B, remove B's rows and hand B's atoms (without its slot-5 atoms) in as obstacles: pp_clash on
 * A's rows gives what it gives on the full complex with B's slot 5 masked, to fp32 rounding.
 *   xyzr       DEVICE [M][4] (x, y, z, radius); the ctx keeps a copy of its own, the caller may free it;
 *   seg_range  HOST int32 [n_seg][2] (first, count) into xyzr per segment, read before the call returns; ranges may overlap or
 *              coincide (the decoys of an ensemble group share theirs: pp_ensemble_recombine leaves a group alone, pick -1, whose
 *              decoys point at different ranges);
 *   M = 0 or xyzr == NULL clears the set: every call then behaves, bit for bit, as on a ctx that never had one.
 * The summation order is fixed (obstacle l of a range belongs to wave (l / 64) mod 4 and partner stripe l mod 4 of the residue's
 * workgroup, ascending l per lane): results are bit-reproducible and a segment's do not depend on the other segments.  The Adam loop
 * does not scan a segment's range at every step: it builds static candidates per row once per pp_proximal* call (|CA_i - q_o| <
 * e_i + r_o + 1.8 - tol, e_i the extent of the residue-partner lists), up to PP_OBSTACLE_CAP = 256 per row; a row with more scans its
 * range, same order, same bits.  pp_clash outside the loop scans.  Cost: 1 KB of ctx memory per row.
 * Does not wait for the stream, except when the set is larger than any this ctx held before (the copy is reallocated, which waits
 * for the device); pp_ctx_destroy of a ctx that ever held obstacles frees that copy and waits likewise.
 * PP_ERR_INVALID: a null ctx, M < 0, a null seg_range with M > 0, a range outside [0, M], a padded B > 1 ctx.  A non-finite
 * coordinate or radius, or a negative radius, is found on the device: it sets bit 2 of pp_ctx_saturated (no read-back here). */
#define PP_OBSTACLE_CAP 256
pp_status pp_ctx_set_obstacles(pp_ctx *ctx, const float *xyzr /* DEVICE [M][4] */, const int32_t *seg_range /* HOST [n_seg][2] */,
                               int M, void *stream);

/* ---- PackPPI-AP: binding ddG prediction (src/models/AffinityPrediction.py) ----------------------------------------------
 * The pretrained network at t = 0 is pp_score (get_pret_feature, :109-122: hV of a ctx of the wild-type batch and of one of
 * the mutant batch).  The mutation encoder + MPNN (mode `network`, :50-71) run on a plan of their own: pp_plan_create with
 * the score network's weight layout built from mutation_encoder.* / mutation_mpnn.*, node-embedding columns 35..50 and the
 * decoder zero (packppi_amd/weights.py mutation_branch_state_dict), and on a ctx whose residue_mask is the local mask of
 * get_local_subgraph (:124-145), which drives the neighbour search, mask_attend and mask_V as ProteinEncoder's `mask` does. */
typedef struct pp_affinity pp_affinity; /* the tensors AffinityPrediction owns besides the two networks, on one GPU */

#define PP_AFF_N_WEIGHTS 101889u        /* mode network: mut_bias, seq_embedding, mutation_fusion, ddg_predictor */
#define PP_AFF_N_WEIGHTS_LINEAR 33153u  /* mode linear: ddg_predictor only */

/* Replaces the construction of mut_bias, seq_embedding, mutation_fusion and ddg_predictor (AffinityPrediction.py:73-94) and
 * their load_from_checkpoint.  `weights` is a HOST buffer of the tensors of packppi_amd/weights.py::affinity_head_spec(mode)
 * concatenated in that order, nn.Linear / nn.Embedding layouts: n_weights = PP_AFF_N_WEIGHTS (network) or
 * PP_AFF_N_WEIGHTS_LINEAR (linear; pp_affinity_encode then gives PP_ERR_INVALID).  mut_bias row 0 is used as given. */
pp_status pp_affinity_create(const float *weights, size_t n_weights, int device, pp_affinity **aff);
void pp_affinity_destroy(pp_affinity *aff);

/* Replaces AffinityPrediction.encode (:148-169) after the pretrained features: the mutation encoder's node embedding
 * Linear(35, 128) + LayerNorm from `residue_type` [N] and `sc_sincos` [N,4,2] AS GIVEN (the batch's SC_D_sincos or
 * SC_D_sincos_mut, not recomputed from angles), the fusion Linear(384,128) ReLU Linear(128,128) of
 * [hV_pret | that embedding | seq_embedding(residue_type)] plus mut_bias[mut_mask] (`mut_mask` int64 [N], 0 / 1), then the
 * 3-layer MPNN on the ctx's graph.  `ctx` is a ctx of the mutation-branch plan whose batch carries the local mask as its
 * residue_mask; one ctx serves the wild type and the mutant (the graph depends on neither).  hV [N,128] receives the MPNN
 * output (exact zeros on rows outside the local mask). */
pp_status pp_affinity_encode(const pp_affinity *aff, pp_ctx *ctx, const int64_t *residue_type, const float *sc_sincos,
                             const int64_t *mut_mask, const float *hV_pret, float *hV, void *stream);

/* Replaces the head of AffinityPrediction.forward (:186-187): per segment s (rows seg_offsets[s] .. seg_offsets[s+1]-1 of
 * h_wt / h_mt [n_rows,128]) the max over rows of h_mt - h_wt and of h_wt - h_mt (a NaN anywhere in a feature's rows gives
 * NaN, as torch.max), then ddg_predictor: ddg[s], ddg_inv[s].  Segments are the complexes of a packed batch or the B rows
 * of a padded batch, padding rows INCLUDED (the reference's max sees them).  seg_offsets: DEVICE int32 [n_seg + 1], every
 * entry within [0, n_rows] (entries are clamped to it); an empty segment gives the ddg_predictor of a -inf vector. */
pp_status pp_affinity_predict(const pp_affinity *aff, const float *h_wt, const float *h_mt, const int32_t *seg_offsets,
                              int n_seg, int n_rows, float *ddg, float *ddg_inv, void *stream);

/* ---- Denoising score-matching loss (TorsionalDiffusion.py:126-154; schedule.py:30-94) ------------------------------------------
 * Replaces SO2Schedule.score(x, sigma) (schedule.py:66-75) for PI = pi / 2 (pi_periodic = 1) and PI = pi (0) WITHOUT the
 * reference's 5001 x 5001 fp64 tables: a table entry is a pure function of its two indices, so it is computed.  x, sigma, score:
 * DEVICE [n] (sigma already expanded to x's shape); idx: DEVICE int32 [n][2] = (sigma index, x index), may be NULL.
 *   - quantisation as schedule.py:67-74: wrap into [-PI, PI), sign, log(|x| / PI + 1e-10), scale, clip to [0, 5000], round half
 *     to even; sigma likewise with SIGMA_MIN = 3e-3, SIGMA_MAX = 2.  NumPy promotion: the first log runs on a float32 array; under
 *     the reference's pinned NumPy 1.22 the scaling that follows stays in float32, under NumPy 2 (which made this project's
 *     fixtures) the float32 log is promoted and the scaling runs in float64.  The kernel follows NumPy 2: fp32 logf, then fp64.
 *   - x_j, sigma_i from the grids of schedule.py:40-43, which the caller computes with NumPy as the reference does and hands
 *     over once per device: pp_so2_set_grids(x_grid, sigma_grid HOST fp64 [2][5001]: schedule 1pi, then 2pi).  Synchronous.
 *     pp_so2_score before it gives PP_ERR_INVALID.
 *   - entry in fp64, terms i = -100 .. 100 in that order: p = sum exp(-(x + 2 PI i)^2 / 2 / sigma^2),
 *     g = sum (x + 2 PI i) / sigma^2 exp(...), entry = g / (p == 0 ? 1e-10 : p); score = (float)(-sign * entry). */
pp_status pp_so2_set_grids(const double *x_grid, const double *sigma_grid, int device);
pp_status pp_so2_score(const float *x, const float *sigma, size_t n, int pi_periodic, float *score, int32_t *idx, int device,
                       void *stream);

/* Replaces the tail of TDiffusionModule.forward (TorsionalDiffusion.py:139-153), per segment: the complexes of a packed ctx, the
 * B rows of a padded ctx (padding rows included), one segment for B = 1.  All DEVICE: pred_score (the network's, unscaled),
 * target_score [N][4]; t_rows [N]; score_norm fp64 [2][5001] (score_norm_ of the 1pi schedule, then of the 2pi one); num, den
 * fp64 [n_seg].  sigma = exp(ln(0.01 pi) + (ln pi - ln(0.01 pi)) t) in fp32, its score_norm index per schedule as
 * schedule.py:88-94, sn chosen by chi_1pi_periodic_mask; in fp64
 *     num[s] = sum (target - pred * sqrt(sn) * SC_D_mask)^2 / (sn + 1e-6),     den[s] = sum SC_D_mask
 * in a fixed order (no float atomics).  The reference's loss is sum_s num / max(sum_s den, 1). */
pp_status pp_dsm_loss(pp_ctx *ctx, const float *pred_score, const float *target_score, const float *t_rows,
                      const double *score_norm, double *num, double *den, void *stream);

/* ---- Decoy ensembles (no reference counterpart; csrc/pp_ensemble.hip holds the arithmetic) -------------
 * D decoys of every complex -> consensus, per-angle confidence, a score per decoy and a selected decoy.  The ctx is a packed one
 * (or B = 1 with n_decoys = 1) whose B segments are B / D groups of D consecutive segments of equal length: segment g * D + d is
 * decoy d of group g (packppi_amd/batch.py replicate / replicate_many).  The consensus row of (group g, row r) is
 * seg_off[g * D] / D + r.  All pointers DEVICE:
 *   chi [N][4] the decoys' angles; per_res [N] (pp_clash at those angles) or NULL;
 *   mean, resultant [N / D][4]: the circular mean of the D angles (period pi where chi_1pi_periodic_mask is set, else 2 pi) and the
 *     length of their mean resultant, 1 = all decoys agree; both 0 where SC_D_mask is 0;
 *   dev fp64 [B]: the root mean square over the segment's unmasked angles of the wrapped difference to the STORED fp32 mean;
 *   clash fp64 [B]: the mean of per_res over the segment's rows (untouched if per_res is NULL);
 *   best int32 [B / D]: per group the decoy with the smallest clash (select = 1) or dev (select = 2), the lowest index on ties, a
 *     NaN losing to any number; select = 0: decoy 0;  chi_best [N / D][4] (or NULL): that decoy's rows, bit for bit.
 * fp64 sums in a fixed order, no float atomics: every output is bit-reproducible, and a group's outputs do not depend on the
 * other groups of the ctx.  Three launches, never waits for the stream.  The rows come from the clamped segment table: a group whose
 * segments differ in length reads nothing outside the batch and reports best = -1 (dev NaN, its chi_best rows not written).
 * PP_ERR_INVALID: n_decoys < 1, B or N not a multiple of n_decoys, a null ctx / chi / mean / resultant / dev / best, per_res
 * without clash, select outside 0 .. 2, select = 1 without per_res, a padded B > 1 ctx, a batch without SC_D_mask /
 * chi_1pi_periodic_mask. */
#define PP_SELECT_NONE 0
#define PP_SELECT_CLASH 1
#define PP_SELECT_MEDOID 2
pp_status pp_ensemble_reduce(pp_ctx *ctx, const float *chi /* [N][4] */, int n_decoys, const float *per_res /* [N] or NULL */,
                             int select, float *mean /* [N/D][4] */, float *resultant /* [N/D][4] */, double *dev /* [B] */,
                             double *clash /* [B] */, int32_t *best /* [B/D] */, float *chi_best /* [N/D][4] or NULL */,
                             void *stream);

/* ---- Recombination of a decoy ensemble per residue (no reference counterpart; csrc/pp_recombine.hip holds
 * the arithmetic).  The ctx is an ensemble ctx as for pp_ensemble_reduce.  The D sampled states of every consensus row are that
 * row's candidates; an assignment s gives every consensus row a decoy, and a conflict-free parallel descent lowers
 *   F(s) = sum_r U(r, s_r) + 1/2 sum_r sum_{r' != r} W(r, s_r; r', s_r'),
 * which is the sum over the complex of pp_clash's per_res at the recombined angles (U: the within-residue term; W: the pair
 * term with both residues' weights; fp32, pp_clash's masks, exclusions and parameters).  One sweep: every row proposes the
 * candidate d with the smallest local energy E_r(d | s) = U(r, d) + sum_r' W(r, d; r', s_r') (lowest d on ties, a NaN loses to
 * any number) and its gain E_r(s_r | s) - E_r(d | s); a row takes its proposal iff its gain is positive and every partner row
 * (the static predicate of the proximal loop's candidate lists) with a positive gain has a smaller one, or an equal one and a
 * higher row number.  Accepted rows are pairwise non-partners: F drops by the sum of their gains.  All pointers DEVICE:
 *   chi [N][4] the decoys' angles (the atom records are reconstructed at them, as in pp_clash);
 *   start int32 [B / D] the decoy every row of the group starts from -- `best` of pp_ensemble_reduce --, or NULL = decoy 0;
 *   pick int32 [N / D] the final s_r;  chi_out [N / D][4] row r of decoy pick[r], bit for bit;
 *   trace fp64 [B / D][max_sweeps + 1]: clash(s) = F(s) / L_g after k sweeps, summed in fp64 in a fixed order from the fp32 row
 *     terms, on the scale of pp_ensemble_reduce's clash; entries behind convergence repeat the last value;
 *   sweeps int32 [B / D] the number of sweeps in which a row of the group moved;
 *   converged int32 [B / D] 1 iff a sweep without a positive gain was seen (max_sweeps = 0: 0, except n_decoys = 1: 1);
 *   energy [N / D][n_decoys] (or NULL): E_r(d | s) at the START assignment.
 * Rows whose candidates are the same in every decoy (no chi angle, padding, the kept rows of a pinned ensemble) get the same E
 * bits for every d, gain exactly 0 and never move.  A group whose start is outside 0 .. D - 1 (the -1 pp_ensemble_reduce gives a
 * ragged group) or whose clamped segments differ in length is left alone: pick -1, its chi_out rows not written, trace NaN, sweeps
 * 0, converged 0, nothing read outside the batch.  Exactly max_sweeps sweeps are enqueued (two launches each, one pass in front,
 * two behind); a converged group's later launches return at once.  Never waits for the stream, reads nothing back.  No float
 * atomics: every output is bit-reproducible, and a group's outputs do not depend on the other groups of the ctx.  Works on a
 * geometry-only plan.  The call uses the proximal loop's workspaces: do not overlap it with pp_proximal* on the same ctx.
 * PP_ERR_INVALID: a null ctx / chi / pick / chi_out / trace / sweeps / converged, n_decoys < 1, B or N not a multiple of n_decoys,
 * max_sweeps < 0, a padded B > 1 ctx, a batch without atom_mask / residue_index, no pp_plan_set_clash_params before. */
pp_status pp_ensemble_recombine(pp_ctx *ctx, const float *chi /* [N][4] */, int n_decoys,
                                const int32_t *start /* DEVICE [B/D] or NULL = decoy 0 */, int max_sweeps,
                                int32_t *pick /* [N/D] */, float *chi_out /* [N/D][4] */,
                                double *trace /* [B/D][max_sweeps+1] */, int32_t *sweeps /* [B/D] */,
                                int32_t *converged /* [B/D] */, float *energy /* [N/D][n_decoys] or NULL */,
                                void *stream);

/* ---- Shell masks (csrc/pp_shell.hip holds the arithmetic) ------------------------------------------------
 * "Which rows lie near these rows", per segment of the ctx's segment table (the complexes of a packed ctx, the B rows of a padded
 * one, padding rows included).  PP_SHELL_CA replaces AffinityPrediction.get_local_subgraph (AffinityPrediction.py:124-145); the
 * result, inverted, is the `fixed` array of pp_sample_partial / pp_proximal_pinned, made without a read-back.
 *   shell[n] = 1 iff a row j of the SAME segment exists with seeds[j] != 0, (PP_SHELL_OTHER_CHAIN) chain_indices[j] !=
 *   chain_indices[n], and
 *     mode CA:   d2(CA_n, CA_j) < r2 (atom14 slot 1; atom_mask is not read);
 *     mode ATOM: atoms a of n, b of j with atom_mask[n][a] != 0, atom_mask[j][b] != 0 and d2 < r2.
 *   j = n counts: a seed row is in its own shell.  residue_mask is not consulted (the reference's get_local_subgraph does not
 *   consult it either).  count[s] (or NULL) = the number of shell rows of segment s.
 * Arithmetic: fp32, fp contract off; d = p - q per component, d2 = ((dx dx) + (dy dy)) + (dz dz), r2 = radius radius computed
 * once, strict <: a NumPy float32 restatement gives the same bytes.  The pruning (ATOM mode: a CA pre-filter with bounding radii
 * computed in the launch from the coordinates given; the seed rows compacted in LDS) changes no output byte.  xyz NULL = the batch's
 * X.  Every output byte has one writer (count: integer atomics); one kernel behind one memset; never waits for the stream.
 * PP_ERR_INVALID: a null ctx, seeds or shell; an unknown mode or flag bit; radius not finite or <= 0; PP_SHELL_ATOM on a batch
 * without atom_mask; PP_SHELL_OTHER_CHAIN on a batch without chain_indices. */
#define PP_SHELL_CA 0          /* CA-CA distance (atom14 slot 1): AffinityPrediction.get_local_subgraph */
#define PP_SHELL_ATOM 1        /* any pair of present atoms */
#define PP_SHELL_OTHER_CHAIN 1 /* flag: the partner row must have a different chain_indices */
pp_status pp_ctx_shell(pp_ctx *ctx, const uint8_t *seeds /* DEVICE [N] */, int mode, float radius, int flags,
                       const float *xyz /* DEVICE [N,14,3] or NULL = the batch's X */,
                       uint8_t *shell /* DEVICE [N] */, int32_t *count /* DEVICE [n_seg] or NULL */, void *stream);

/* ---- Solvent-accessible surface (no reference kernel; csrc/pp_sasa.hip holds the arithmetic) -------------
 * Shrake-Rupley test points with four nested occluder levels in one pass, per segment of the ctx's segment table (the complexes of
 * a packed ctx, the decoys of a group, the B rows of a padded batch).  The reference's interface (src/utils/interface.py: a residue
 * whose accessible area in the isolated chain exceeds that in the complex) needs freesasa; this makes the same statement on the
 * device.  An atom (row n, slot a) is present iff radius[n][a] > 0; residue_mask is not consulted.  The occluders of a present atom
 * are, by class: 0 the other present atoms of its row; 1 those of other rows of the segment with the same chain_indices; 2 those of
 * rows of the segment with another chain_indices; 3 the obstacle atoms of the segment with r_o > 0 (pp_ctx_set_obstacles).
 * Arithmetic (fp32, fp contract off):  R_a = r_a + probe;  q = p_a + (R_a u_k) per component;  for occluder b  R_b = r_b + probe,
 * d = q - p_b,  d2 = ((dx dx) + (dy dy)) + (dz dz);  the point is buried iff d2 < R_b R_b (strict; a NaN buries nothing and is
 * buried by nothing).  m(a, k) = the smallest class that buries point k, 4 if none.
 *   counts[n][a][L] = #{k : m(a, k) > L}, 0 for an absent atom: exposed next to the own residue alone (L = 0), in the isolated
 *                     chain (1), in the protein complex (2), with the obstacles too (3); non-increasing in L; without obstacles
 *                     level 3 = level 2;
 *   area[n][L]      = sum over ascending present slots a of ((kf R_a) R_a) (float)counts[n][a][L], kf = (float)(4 pi / n_points);
 *   seg_area[s][L]  = the fp64 sum of area over the rows of segment s, in a fixed binary tree (no float atomics).
 * m is a minimum over a set: a segment gets the same bits alone, packed in front of or behind others, or as a decoy of a group, and
 * two runs give the same bits.  The candidate search (per-row bounding spheres, an LDS list of at most PP_SASA_LIST_CAP atoms that
 * is worked off and refilled) changes no output word.  points are caller data and are not normalised.  xyz NULL = the batch's X.
 * Absolute areas belong to the radii given; they are not freesasa's numbers.  Never waits for the stream; every output word has
 * one writer.
 * PP_ERR_INVALID: a null ctx, radius, points or area; n_points outside 1 .. PP_SASA_MAX_POINTS; probe negative or not finite; a
 * batch without chain_indices. */
#define PP_SASA_LIST_CAP 768    /* occluder atoms the LDS list of one row holds before it is worked off */
#define PP_SASA_MAX_POINTS 256
pp_status pp_sasa(pp_ctx *ctx, const float *xyz /* DEVICE [N,14,3] or NULL = the batch's X */, const float *radius /* DEVICE [N][14] */,
                  const float *points /* DEVICE [n_points][3] */, int n_points, float probe,
                  int32_t *counts /* DEVICE [N][14][4] or NULL */, float *area /* DEVICE [N][4] */,
                  double *seg_area /* DEVICE [n_seg][4] or NULL */, void *stream);

/* ---- Disulfide bridges (no reference kernel; csrc/pp_disulfide.hip holds the arithmetic) ------------------
 * Finds the cysteine pairs of every segment whose sulfurs can meet -- from the backbone alone -- and closes them by choosing the
 * two chi1 next to the caller's angles.  Per segment of the ctx's segment table; pairs never cross segments.
 *   eligible row   residue_type == PP_RESTYPE_CYS, residue_mask != 0, atom_mask slots 0, 1, 2, 5 (N, CA, C, SG) != 0
 *   grid           theta_k = (float)(-pi + 2 pi k / 72), k = 0 .. 71, for both chi1 of a pair a < b
 *   E(p, q)        ((|A-B| - 2.04) / 0.10)^2 + ((ang(CB_a,A,B) - 104) / 10)^2 + ((ang(CB_b,B,A) - 104) / 10)^2
 *                  + ((|dih(CB_a,A,B,CB_b)| - 90) / 30)^2, A = SG(a, theta_p), B = SG(b, theta_q), the ideal CB and SG of pp_atom14
 *                  built relative to the row's CA; angles in degrees.  Emin = the minimum over the 72 x 72 points.
 *   candidates     both rows eligible, |CB_a - CB_b| <= cb_max, Emin <= max_energy
 *   bonded set     greedy in ascending (Emin, a, b): a pair is taken iff neither row is bonded yet
 *   closure        a row with fixed[n] != 0 keeps its chi1: its table is its SG at chi[n][0], 72 times.  Emin_r = the minimum of E
 *                  over that grid, thr = max(Emin_r, min(max_energy, Emin_r + 4)), F = {E <= thr}; the pick is the argmin over F of
 *                  J = E + (wrap(theta_p - chi[a][0])^2 + wrap(theta_q - chi[b][0])^2) / sigma_chi^2 (a fixed row's term is 0; chi
 *                  NULL: J = E), ties to the lowest 72 p + q.  Detection never reads fixed.
 *   pairs          DEVICE int32 [n_pairs][2] of rows, or NULL.  A list replaces detection: no cb_max, no max_energy.  An entry
 *                  with a row out of range or not eligible, or rows of two segments, is dropped.
 * Outputs, all on the device, every word with one writer; the call never waits for the stream:
 *   partner[n]     the bonded partner's row, or -1
 *   report[n]      (Emin, E at the pick, SG-SG distance at the pick, signed chi3 in radians) on both rows of a bonded pair, else 0
 *   count[s]       bonded pairs of segment s; -1 in EVERY segment when more pairs lie within cb_max than the candidate list holds
 *                  (min(N (N - 1) / 2, 64 N)): then nothing is bonded and chi_out = chi
 *   chi_out        chi bit for bit, except chi_out[a][0] = theta_p and chi_out[b][0] = theta_q of bonded rows that are not fixed.
 *                  May be chi itself; NULL = detection only.
 * The first call on a ctx allocates the workspace (sized from N), pp_ctx_destroy frees it.
 * PP_ERR_INVALID: a null ctx, partner, report or count; chi_out or fixed without chi; n_pairs beyond the list; cb_max or sigma_chi
 * not finite and positive; a batch without X, atom_mask, residue_type or residue_mask. */
#define PP_RESTYPE_CYS 4       /* constants.restype_order['C'] */
pp_status pp_disulfide_close(pp_ctx *ctx, const float *chi /* DEVICE [N,4] or NULL */, const uint8_t *fixed /* DEVICE [N] or NULL */,
                             const int32_t *pairs /* DEVICE [n_pairs][2] or NULL */, int n_pairs, float cb_max, float max_energy,
                             float sigma_chi, float *chi_out /* DEVICE [N,4] or NULL */, int32_t *partner /* DEVICE [N] */,
                             float *report /* DEVICE [N][4] */, int32_t *count /* DEVICE [n_seg] */, void *stream);

/* ---- Anchors: metal sites and covalent links (no reference kernel; csrc/pp_anchor.hip holds the arithmetic) --
 * An anchor is a distance restraint, optionally with an angle term, between a side-chain atom and a fixed point: a metal ion, or the
 * atom of a ligand the residue is covalently linked to.  The call closes anchors next to the caller's angles; the caller then pins
 * the closed rows, as it does with the rows of a disulfide bridge.
 * Arithmetic is fp32 with fp contract off.  Each row's result is a function of that row's data and its anchors only.
 *   anchor i       has: row, the row it belongs to; slot, the donor atom14 slot, 5..13; ante, the slot of the same row the donor is
 *                  bonded to, 0..13; target, xyz in the batch's coordinates; d0 and sigma_d in A; theta0 and sigma_theta in degrees.
 *                  sigma_theta <= 0 means no angle term.  A row may carry at most PP_ANCHOR_PER_ROW = 4 anchors.  They are taken in
 *                  list order.
 *   valid          means all of: row is in range and residue_mask != 0; atom_mask of N, CA, C, slot and ante is non-zero; the rigid
 *                  group of slot (a2g) is a chi group, 4..7 (CB never moves); ante != slot; target, d0, sigma_d > 0, theta0 and
 *                  sigma_theta are finite.  An invalid entry, or a fifth anchor on a row, is dropped on the device and the row's
 *                  status becomes -2.  The Python layer refuses it by name before the call.  (A residue_type outside 0..20 makes
 *                  the entry invalid too; an entry whose row is out of range marks no row; "fifth" counts the valid entries of the
 *                  row in list order.)
 *   geometry       The row's atoms are built as pp_atom14 builds them: backbone frame, default frames of the rigid groups, rotation
 *                  about x by chi, literature positions.  They are built relative to the row's CA, and the target is taken as
 *                  target - CA once (pp_shell's and pp_disulfide's habit, so a structure far from the origin loses nothing).
 *   grid           n = the largest (group - 3) over the row's valid anchors: the number of chi the row's donors depend on, 1..4.
 *                  g(n) = 72, 72, 36, 24.  theta_k = (float)(-pi + 2 pi k / g).  A point is (k1..kn) with flat index
 *                  ((k1 g + k2) g + k3) g + k4, truncated to n digits.  Chi beyond n keep the caller's value (0 without chi).
 *   energy         Sum over the row's valid anchors in list order of
 *                      ((|A - q| - d0) / sigma_d)^2 + ((ang(P, A, q) - theta0) / sigma_theta)^2
 *                  where A is the donor, P its antecedent and q the target.  ang is pp_disulfide_close's, in degrees.  A NaN never
 *                  wins a minimum.
 *   closure        Emin = the minimum over the grid.  If Emin > max_energy, the row is open: status -1 and chi_out row = chi row bit
 *                  for bit.  Otherwise thr = max(Emin, min(max_energy, Emin + 4)) and F = {E <= thr}.
 *                  J = E + (sum over k <= n, left to right, of wrap(theta - chi[row][k])^2) / sigma_chi^2.  chi NULL means J = E.
 *                  The pick is the argmin of J over F, ties to the lowest flat index.  chi_out = chi bit for bit except the first n
 *                  chi of closed rows.  A fixed row is kept: status 2.  Its E, distance and angle at its own angles are reported and
 *                  nothing is written.
 * Outputs, on the device, one writer per word, no read-back, the call never waits for the stream:
 *   status[n]          0 none, 1 closed, 2 kept, -1 open, -2 an entry of this row was dropped (its other anchors close it, keep it or
 *                      leave it open all the same: chi_out and the reports say which)
 *   report[n]          (Emin, E at the pick, the first anchor's distance, the first anchor's angle); an open row has Emin alone, a
 *                      kept row its E twice; 0 on rows without a valid anchor
 *   anchor_report[i]   distance and angle of every anchor at its row's pick; 0 for a dropped entry or an open row
 *   count[s]           rows of status 1 per segment of the ctx's segment table
 *   chi_out            may be chi itself; NULL = reports only
 * Capacity: A <= 8 N.  The first call on a ctx allocates the workspace (sized from N), pp_ctx_destroy frees it.  Works on a
 * geometry-only plan.
 * PP_ERR_INVALID: a null ctx, status, report or count; A > 0 without the three anchor arrays or anchor_report; A negative or beyond
 * 8 N; chi_out or fixed without chi; max_energy NaN; with chi, sigma_chi not finite and positive; a batch without X, atom_mask,
 * residue_type or residue_mask. */
#define PP_ANCHOR_PER_ROW 4
pp_status pp_anchor_close(pp_ctx *ctx, const float *chi /* DEVICE [N,4] or NULL */, const uint8_t *fixed /* DEVICE [N] or NULL */,
                          const int32_t *anchors_i /* DEVICE [A][4] (row, slot, ante, 0) */,
                          const float *anchors_target /* DEVICE [A][4] (x, y, z, 0) */,
                          const float *anchors_param /* DEVICE [A][4] (d0, sigma_d, theta0, sigma_theta) */, int A, float max_energy,
                          float sigma_chi, float *chi_out /* DEVICE [N,4] or NULL */, int32_t *status /* DEVICE [N] */,
                          float *report /* DEVICE [N][4] */, float *anchor_report /* DEVICE [A][2] */,
                          int32_t *count /* DEVICE [n_seg] */, void *stream);

/* ---- Polar contacts (no reference kernel; csrc/pp_polar.hip holds the arithmetic) ------------------------
 * Hydrogen bonds, salt bridges and polar obstacle contacts between the heavy atoms of every segment of the ctx's segment table (the
 * complexes of a packed ctx, the decoys of a group, the B rows of a padded batch).  No pair crosses segments.  Chemistry is caller data:
 *   cls   DEVICE uint8 [N][14]: bit 0 donor, bit 1 acceptor, bit 2 cation, bit 3 anion; 0 = not polar or absent
 *   ante  DEVICE int8 [N][14][2]: the slots of the same row the atom is bonded to, -1 = none.  An entry outside -1 .. 13 is found on
 *         the device: the atom is treated as not polar and bit 2 of pp_ctx_saturated is set
 *   obst_polar  DEVICE uint8 [M] or NULL: != 0 marks a polar atom of the ctx's obstacle set (pp_ctx_set_obstacles)
 * Arithmetic (fp32, fp contract off, every operation rounded on its own).  Atom x at p with antecedents at a1 (and a2): base point
 * b = a1, or (a1 + a2) * 0.5f per component; u = b - p (0 without an antecedent: no direction test).  Pair (x at p, y at q):
 * d = q - p, d2 = ((dx dx) + (dy dy)) + (dz dz), sx = ((ux dx) + (uy dy)) + (uz dz); e = p - q, sy the same sum of u_y and e.
 *   hydrogen bond  x and y in different rows of one segment, (x donor and y acceptor) or (x acceptor and y donor),
 *                  d2 <= hb_max * hb_max (rounded once on the host), sx <= 0 and sy <= 0: both angles antecedent-atom...partner are at
 *                  least 90 degrees.  Symmetric by construction; a NaN makes a comparison false and gives no bond.
 *                  Skipped: both atoms in backbone slots 0 or 3 of adjacent rows (|n - j| = 1) with equal chain_indices.
 *   salt bridge    rows n != j of one segment: a cation atom of one and an anion atom of the other with d2 <= sb_max * sb_max
 *   obstacle       an atom o of the segment's obstacle range with obst_polar[o] != 0 and d2 <= hb_max * hb_max (no direction test)
 * Outputs, all on the device, integers; every word has one writer, except seg (integer atomics).  Does not wait for the stream,
 * except that the first call on a ctx allocates the workspace, which may wait for the device.
 *   n_partners[n][a]   (hydrogen-bond partners of the atom, polar obstacle atoms within reach): the true counts
 *   partners[n][a]     the lowest min(count, PP_POLAR_CAP) partner codes, ascending, then -1; code = (row - first row of the
 *                      segment) * 14 + slot: a segment gets the same words alone, packed behind others, or as a decoy
 *   res[n][0..7]       sums over the row's atoms: partners of side-chain atoms (slot >= 4) in rows of the same chain (0) / another
 *                      chain (1); of backbone atoms (slots 0 and 3) same chain (2) / another (3); salt-bridge partner rows same chain
 *                      (4) / another (5); obstacle partners (6); atoms with cls != 0 and neither kind of partner (7)
 *   seg[s][0..7]       bonds counted once (0), between chains (1), with a side-chain atom (2), both (3); salt-bridged row pairs (4),
 *                      between chains (5); bonds to obstacle atoms (6); unsatisfied polar atoms (7)
 * The row pre-filter (spheres around slot 1 that hold the row's polar atoms) changes no output word.  The first call on a ctx
 * allocates the workspace (sized from N), pp_ctx_destroy frees it.  Works on a geometry-only plan.
 * PP_ERR_INVALID: a null ctx, cls, ante, n_partners, res or seg; hb_max or sb_max not finite or not positive; a batch without
 * chain_indices; no coordinates (xyz NULL and no X); obst_polar on a ctx without obstacles. */
#define PP_POLAR_CAP 4
pp_status pp_polar(pp_ctx *ctx, const float *xyz /* DEVICE [N,14,3] or NULL = the batch's X */, const uint8_t *cls /* DEVICE [N][14] */,
                   const int8_t *ante /* DEVICE [N][14][2] */, const uint8_t *obst_polar /* DEVICE [M] or NULL */, float hb_max,
                   float sb_max, int32_t *partners /* DEVICE [N][14][PP_POLAR_CAP] or NULL */, int32_t *n_partners /* DEVICE [N][14][2] */,
                   int32_t *res /* DEVICE [N][8] */, int32_t *seg /* DEVICE [n_seg][8] */, void *stream);

/* ---- Explicit hydrogens (no reference kernel; csrc/pp_hydrogens.hip holds the arithmetic) -------------------
 * Places the hydrogens of every row from its heavy atoms.  An all-atom row has PP_AA_SLOTS slots: 0 .. 13 atom14, 14 + k the k-th
 * hydrogen of the residue type (k < PP_H_MAX).  Per segment of the ctx's segment table; nothing crosses segments.  Chemistry is
 * caller data (packppi_amd/constants.py derives it from the covalent bonds):
 *   place  DEVICE int8 [21][13][5]: (kind, parent slot, n1, n2, n3) per residue type and hydrogen.  kind & 15: 0 none, 1 SUM (away
 *          from the parent's neighbours n1 .. n3; -1 = none, 14 = the C of the previous row), 2 T2 (two neighbours n1 < n2, one of
 *          the two tetrahedral positions), 3 NERF (n1 = a, the parent's one neighbour, n2 = b, a neighbour of a: bond angle and
 *          dihedral); kind & 16: dropped on a row with link[n] >= 0
 *   param  DEVICE float [21][13][5]: (bond length L, c1, s1, c2, s2): T2 cos alpha and +-sin alpha; NERF cos / sin of the angle
 *          H-parent-a and of the dihedral H-parent-a-b
 *   link   DEVICE int32 [N] or NULL: what pp_disulfide_close writes as partner
 * Arithmetic: fp32, fp contract off, every vector a difference to the parent, in the order csrc/pp_hydrogens.hip states.
 *   link_prev[n]  1 iff row n - 1 is in the same segment with the same chain_indices, atom_mask of its C and of this row's N are
 *                 not 0 and |C - N|^2 <= 4.0: the rows are joined by a peptide bond
 *   hmask[n][k]   1 iff the hydrogen exists: atom_mask != 0 for the parent and every atom read, link_prev[n] if it reads the
 *                 previous C, not dropped for link, all three coordinates finite (atoms exactly in line: dropped)
 *   hxyz[n][k]    its position, 0 where hmask is 0
 * A table entry outside its range, or a residue_type outside 0 .. 20, is found on the device: the hydrogen is dropped and bit 3
 * (value 8) of pp_ctx_saturated is set; it is never used as an index.  Works on a geometry-only plan, never waits for the stream,
 * one writer per word.
 * PP_ERR_INVALID: a null ctx, place, param, hxyz, hmask or link_prev; a batch without chain_indices, residue_type or atom_mask; no
 * coordinates (xyz NULL and no X). */
#define PP_AA_SLOTS 27
#define PP_H_MAX 13
pp_status pp_hydrogens(pp_ctx *ctx, const float *xyz /* DEVICE [N,14,3] or NULL = the batch's X */,
                       const int8_t *place /* DEVICE [21][13][5] */, const float *param /* DEVICE [21][13][5] */,
                       const int32_t *link /* DEVICE [N] or NULL */, float *hxyz /* DEVICE [N][13][3] */,
                       uint8_t *hmask /* DEVICE [N][13] */, uint8_t *link_prev /* DEVICE [N] */, void *stream);

/* ---- All-atom clashscore (no reference kernel; csrc/pp_hydrogens.hip holds the arithmetic) ----------------
 * Serious overlaps between all atoms, hydrogens included, of every segment of the ctx's segment table.  NOT MolProbity: no Reduce
 * flips, no optimisation of rotatable hydrogens, and the numbers belong to the radii given.  Caller data:
 *   hxyz, hmask, link_prev   what pp_hydrogens wrote at the same xyz
 *   radius  DEVICE float [N][27]: atom (n, a) is counted iff radius > 0 (and, for a >= 14, hmask != 0)
 *   acls    DEVICE uint8 [N][27]: bit 0 polar hydrogen, bit 1 acceptor, bit 2 hydrogen, bit 3 backbone
 *   aa_sep  DEVICE uint8 [21][27][27]: bond separation inside a residue of each type, hydrogens included
 *   link, obst_polar   as for pp_hydrogens / pp_polar, or NULL
 * Pair (x at p, y at q) of counted atoms of one segment, fp32, fp contract off: d = q - p, d2 = ((dx dx) + (dy dy)) + (dz dz);
 * t = (rx + ry) - cut; one a polar hydrogen and the other an acceptor: t = t - hb_allow; SERIOUS OVERLAP iff t > 0 and d2 <= t t (a
 * NaN gives none).  Excluded: bond separation <= 3, or <= 4 when either atom is a hydrogen -- same row: aa_sep[type][x][y]; rows i, i +
 * 1 with link_prev[i + 1]: sep(x, slot 2) + 1 + sep(y, slot 0); rows with link[i] == j and link[j] == i: sep(x, slot 5) + 1 + sep(y,
 * slot 5).  An obstacle atom o (r_o > 0) of the segment's range counts against every counted atom: t = (rx + r_o) - cut, minus
 * hb_allow iff x is a polar hydrogen and obst_polar[o] != 0; no exclusions.
 * Outputs, int32 on the device, every word with one writer except seg (integer atomics); no read-back:
 *   n_clash[n][a]   (partner atoms, obstacle atoms): the true counts
 *   partners[n][a]  the lowest min(count, PP_CLASH_CAP) partner codes (row - first row of the segment) * 27 + slot, ascending, then -1
 *   res[n][0..3]    pairs inside the row (each once) plus pairs with other rows of the same chain_indices (0); pairs with rows of
 *                   another chain (1); pairs with obstacle atoms (2); atoms counted (3)
 *   seg[s][0..7]    atoms counted (0); pairs, each once (1); between chains (2); with a hydrogen (3); with an atom that is not
 *                   backbone (4); within a row (5); with obstacle atoms (6); both atoms backbone (7)
 * clashscore = 1000 seg[1] / max(seg[0], 1), for the host to compute.  The row pre-filter changes no output word.  The first call on a
 * ctx allocates the workspace (sized from N), which may wait for the device; pp_ctx_destroy frees it.  Geometry-only plans work.
 * PP_ERR_INVALID: a null ctx, hxyz, hmask, radius, acls, aa_sep, link_prev, n_clash, res or seg; cut not finite; hb_allow not finite
 * or negative; a batch without chain_indices or residue_type; no coordinates; obst_polar on a ctx without obstacles. */
#define PP_CLASH_CAP 4
pp_status pp_clashscore(pp_ctx *ctx, const float *xyz /* DEVICE [N,14,3] or NULL = the batch's X */, const float *hxyz /* DEVICE [N][13][3] */,
                        const uint8_t *hmask /* DEVICE [N][13] */, const float *radius /* DEVICE [N][27] */,
                        const uint8_t *acls /* DEVICE [N][27] */, const uint8_t *aa_sep /* DEVICE [21][27][27] */,
                        const uint8_t *link_prev /* DEVICE [N] */, const int32_t *link /* DEVICE [N] or NULL */,
                        const uint8_t *obst_polar /* DEVICE [M] or NULL */, float cut, float hb_allow,
                        int32_t *partners /* DEVICE [N][27][PP_CLASH_CAP] or NULL */, int32_t *n_clash /* DEVICE [N][27][2] */,
                        int32_t *res /* DEVICE [N][4] */, int32_t *seg /* DEVICE [n_seg][8] */, void *stream);

/* ---- Hydrogen-bond network optimisation (no reference kernel; csrc/pp_hnet.hip holds the arithmetic) ---------
 * Chooses, per segment of the ctx's segment table, a state for every MOVER -- a rotor (hydroxyl, thiol, lysine NH3+: the hydrogens
 * turn about the bond to their parent) or a flip (Asn / Gln / His: the group behind one chi turned by pi) -- by a monotone descent on
 * an integer energy: 64 per serious overlap of pp_clashscore minus 2 per good, 1 per weak explicit-hydrogen bond.  Integer counts,
 * NOT Reduce's dot scores; no exhaustive search of cliques; the numbers belong to the radii given.  Caller data:
 *   xyz0, hxyz0, hmask0   state 0: the heavy atoms and what pp_hydrogens wrote at them
 *   xyz1, hxyz1, hmask1   the same at chi + pi on the flip rows (pp_atom14 and pp_hydrogens made them), or all NULL: no row flips
 *   chi0, chi1, chi_out   DEVICE [N][4]: the angles behind the two sets and the selection, or all NULL
 *   place, param          pp_hydrogens' tables
 *   mover   DEVICE int32 [21][4]: (kind, states, bit mask over the 27 slots of the atoms that move, 0) per residue type; kind 0 none,
 *           1 rotor (1 .. PP_HNET_STATES states, at most PP_HNET_ROT_H moved slots, all hydrogens placed by NERF), 2 flip (2 states,
 *           at most PP_HNET_MOVED moved slots)
 *   rot     DEVICE float [21][12][3][2]: cos / sin of the dihedral of a rotor's j-th moved hydrogen in state c, used in place of
 *           param's in pp_hydrogens' NERF arithmetic; state 0 holds param's own values
 *   ext     DEVICE float [21]: no moved atom of the type is farther from CA than this, in any state
 *   radius, acls, aa_sep, link_prev, link, obst_polar, cut, hb_allow   as for pp_clashscore (rotatable hydrogens kept)
 *   hb_weak, hb_weak2, hb_good2   the bond lengths: hb_weak in A, and the squares of the weak and the good limit rounded on the host
 *   reach   max(2 largest radius - cut, hb_weak): two movers are PARTNERS iff d2(CA, CA') <= ((ext + ext') + reach)^2
 * A row is a mover iff its type has one and a moved slot is a counted atom in state 0.  State 0 is the input; every mover proposes
 * its best state given the others, and a proposal is accepted iff its gain is positive and beats that of every partner (ties: the
 * lower row); accepted movers share no term, so the total energy F drops by exactly the sum of the accepted gains.  max_sweeps
 * sweeps are enqueued (0 .. PP_HNET_MAX_SWEEPS); a segment without a positive gain is converged and its later launches return at
 * once.  Outputs on the device, no read-back:
 *   state[n]      the chosen state, -1 for a row that is no mover
 *   xyz_out, hxyz_out, hmask_out, chi_out   row n of set 1 or of set 0, bit for bit; a rotor's moved hydrogens at the chosen state
 *   e[n]          E of the row at the start and at the end (0 for a row that is no mover)
 *   hb[n]         DEVICE int32 [N][2] or NULL: the explicit-hydrogen bonds (weak or good) of the row's moved atoms at the start and
 *                 at the end, a bond between two movers counted in the higher row only: a segment's sum counts every bond once
 *   trace[s][k]   F after k sweeps, k = 0 .. max_sweeps
 *   sweeps[s], converged[s]   sweeps that moved a row; 1 iff the segment has no positive gain left
 *   cand          DEVICE float [N][12][3][3] or NULL: every rotor candidate position (state, hydrogen), 0 where there is none
 *   energy        DEVICE int32 [N][12] or NULL: E of the row in every state, the others at state 0
 * A mover entry outside its range, or a residue_type outside 0 .. 20, is found on the device: the row is no mover and bit 3 (value 8)
 * of pp_ctx_saturated is set; it is never used as an index.  The first call on a ctx allocates the workspace (sized from N and the
 * segment count), which may wait for the device; pp_ctx_destroy frees it.  Geometry-only plans work.  Never waits for the stream.
 * PP_ERR_INVALID: a null ctx, table, input of set 0 or output other than cand / energy / chi_out; half of set 1 or of the chi
 * triple; chi without set 1; cut, hb_allow as pp_clashscore; a bond length that is not finite and positive, hb_good2 > hb_weak2;
 * reach not finite or below hb_weak; max_sweeps outside 0 .. PP_HNET_MAX_SWEEPS; a batch without chain_indices or residue_type;
 * obst_polar on a ctx without obstacles. */
#define PP_HNET_STATES 12
#define PP_HNET_ROT_H 3
#define PP_HNET_MOVED 7
#define PP_HNET_PCAP 16
#define PP_HNET_MAX_SWEEPS 256
pp_status pp_hnet_optimize(pp_ctx *ctx, const float *xyz0 /* DEVICE [N,14,3] */, const float *hxyz0 /* DEVICE [N][13][3] */,
                           const uint8_t *hmask0 /* DEVICE [N][13] */, const float *xyz1, const float *hxyz1, const uint8_t *hmask1,
                           const float *chi0 /* DEVICE [N][4] or NULL */, const float *chi1, const int8_t *place /* DEVICE [21][13][5] */,
                           const float *param /* DEVICE [21][13][5] */, const int32_t *mover /* DEVICE [21][4] */,
                           const float *rot /* DEVICE [21][12][3][2] */, const float *ext /* DEVICE [21] */,
                           const float *radius /* DEVICE [N][27] */, const uint8_t *acls /* DEVICE [N][27] */,
                           const uint8_t *aa_sep /* DEVICE [21][27][27] */, const uint8_t *link_prev /* DEVICE [N] */,
                           const int32_t *link /* DEVICE [N] or NULL */, const uint8_t *obst_polar /* DEVICE [M] or NULL */, float cut,
                           float hb_allow, float hb_weak, float hb_weak2, float hb_good2, float reach, int max_sweeps,
                           int32_t *state /* DEVICE [N] */, float *xyz_out /* DEVICE [N,14,3] */, float *hxyz_out /* DEVICE [N][13][3] */,
                           uint8_t *hmask_out /* DEVICE [N][13] */, float *chi_out /* DEVICE [N][4] or NULL */, int32_t *e /* DEVICE [N][2] */,
                           int32_t *hb /* DEVICE [N][2] or NULL */, int32_t *trace /* DEVICE [n_seg][max_sweeps + 1] */, int32_t *sweeps /* DEVICE [n_seg] */,
                           int32_t *converged /* DEVICE [n_seg] */, float *cand /* DEVICE [N][12][3][3] or NULL */,
                           int32_t *energy /* DEVICE [N][12] or NULL */, void *stream);

/* ---- All-atom chi refinement (no reference kernel; csrc/pp_refine.hip holds the arithmetic) -------------------
 * Lowers, per segment of the ctx's segment table, the explicit-hydrogen overlap energy by small steps in chi space: a monotone
 * descent on an integer energy, 64 per LEVEL of overlap (level >= 1 is pp_clashscore's serious overlap; each further `band` A of
 * depth is one more level, up to `bands`) minus pp_hnet_optimize's 2 / 1 per good / weak explicit-hydrogen bond.  A residue without
 * a serious overlap is never moved.  Caller data:
 *   chi0    DEVICE [N][4]: the angles to start from
 *   fixed   DEVICE uint8 [N] or NULL: rows that do not move (the caller ORs bridged cysteines into it)
 *   place, param, radius, acls, aa_sep, link, obst_polar, cut, hb_allow   as for pp_hydrogens / pp_clashscore (a rotatable hydrogen
 *           the caller does not want counted has radius 0)
 *   ext     DEVICE float [21]: no side-chain atom behind CB or hydrogen on it is farther from CA than this, at any angles
 *   delta, max_steps   the step in radians; a state is steps int8 [4] with |steps[j]| <= max_steps (1 .. PP_REFINE_MAX_STEPS,
 *           max_steps delta < pi) and angle j = chi0[j] for steps[j] == 0, else chi0[j] + steps[j] delta wrapped into [-pi, pi)
 *   bands, band   1 .. PP_REFINE_MAX_BANDS levels, `band` A apart
 *   hb_weak, hb_weak2, hb_good2, reach   as for pp_hnet_optimize
 * A row is a MOVER iff residue_mask != 0, an SC_D_mask entry != 0, it is not fixed and its residue_type lies in 0 .. 20.  Per sweep a
 * mover with a term of level >= 1 proposes the best of its current state and one step up or down on each chi it has (at most
 * PP_REFINE_CAND candidates; coordinates by pp_atom14 and pp_hydrogens themselves, bit for bit); accept rule, partners, trace and
 * convergence as for pp_hnet_optimize: the total energy F drops by exactly the sum of the accepted gains.  max_sweeps sweeps are
 * enqueued (0 .. PP_REFINE_MAX_SWEEPS).  Outputs on the device, no read-back:
 *   chi_out, steps   the angles and the state of every row; a row that did not move keeps the caller's bits, steps 0
 *   xyz_out, hxyz_out, hmask_out, link_prev   pp_atom14 and pp_hydrogens at chi_out
 *   e[n]             E of the row at the start and at the end (0 for a row that is no mover)
 *   trace[s][k], sweeps[s], converged[s]   as for pp_hnet_optimize
 *   cand_xyz [9][N][14][3], cand_hxyz [9][N][13][3], cand_hmask [9][N][13], cand_mask int32 [N]   all NULL or none: the candidates
 *                    of the first sweep (candidate 0 the input, 1 + 2j / 2 + 2j one step up / down on chi j; one that does not exist
 *                    repeats candidate 0) and the bit mask of those that exist (0 for a row that is no mover)
 *   energy           DEVICE int32 [N][9] or NULL: E of the row at every candidate of the first sweep (0 where there is none)
 * Table entries out of range are handled as by pp_hydrogens (bit 3 of pp_ctx_saturated).  The first call on a ctx allocates the
 * workspace (sized from N and the segment count), which may wait for the device; pp_ctx_destroy frees it.  Geometry-only plans work.
 * Never waits for the stream.
 * PP_ERR_INVALID: a null ctx, table, chi0 or output other than cand_* / energy; part of the cand_* group; delta not finite and
 * positive, max_steps outside 1 .. PP_REFINE_MAX_STEPS or max_steps delta >= pi; bands outside 1 .. PP_REFINE_MAX_BANDS, band not
 * finite and positive; cut, hb_allow, the bond lengths and reach as pp_hnet_optimize; max_sweeps outside 0 .. PP_REFINE_MAX_SWEEPS;
 * a batch without X, BB_D, chain_indices, residue_type, atom_mask, residue_mask or SC_D_mask; obst_polar on a ctx without obstacles. */
#define PP_REFINE_CAND 9
#define PP_REFINE_MOVED 22
#define PP_REFINE_PCAP 16
#define PP_REFINE_MAX_SWEEPS 256
#define PP_REFINE_MAX_STEPS 16
#define PP_REFINE_MAX_BANDS 8
pp_status pp_chi_refine(pp_ctx *ctx, const float *chi0 /* DEVICE [N][4] */, const uint8_t *fixed /* DEVICE [N] or NULL */,
                        const int8_t *place /* DEVICE [21][13][5] */, const float *param /* DEVICE [21][13][5] */,
                        const float *ext /* DEVICE [21] */, const float *radius /* DEVICE [N][27] */,
                        const uint8_t *acls /* DEVICE [N][27] */, const uint8_t *aa_sep /* DEVICE [21][27][27] */,
                        const int32_t *link /* DEVICE [N] or NULL */, const uint8_t *obst_polar /* DEVICE [M] or NULL */, float delta,
                        int max_steps, int bands, float band, float cut, float hb_allow, float hb_weak, float hb_weak2, float hb_good2,
                        float reach, int max_sweeps, float *chi_out /* DEVICE [N][4] */, int8_t *steps /* DEVICE [N][4] */,
                        float *xyz_out /* DEVICE [N,14,3] */, float *hxyz_out /* DEVICE [N][13][3] */,
                        uint8_t *hmask_out /* DEVICE [N][13] */, uint8_t *link_prev /* DEVICE [N] */, int32_t *e /* DEVICE [N][2] */,
                        int32_t *trace /* DEVICE [n_seg][max_sweeps + 1] */, int32_t *sweeps /* DEVICE [n_seg] */,
                        int32_t *converged /* DEVICE [n_seg] */, float *cand_xyz, float *cand_hxyz, uint8_t *cand_hmask,
                        int32_t *cand_mask, int32_t *energy /* DEVICE [N][9] or NULL */, void *stream);

/* Measurement aid, no reference counterpart: average duration (ms) of one launch of a hot kernel
 * (which: 0 = node-message kernel, 1 = edge-update kernel), timed with HIP events on `stream`
 * around `iters` launches.  Synchronises the stream. */
pp_status pp_time_kernel(pp_ctx *ctx, int which, int iters, float *avg_ms, void *stream);

/* Measurement aid, no reference counterpart: in-situ duration of a hot kernel.  After
 * pp_profile_kernel(ctx, which) (0 node message, 1 edge update, 2 node update; 3 the one launch per Adam step
 * inside pp_proximal / pp_proximal_packed: clash loss + gradient, the step, the reconstruction at the new angles; 4, 5, 6 the
 * launches of a nudge of pp_sample_guided: reconstruction, clash loss + gradient + step, the node embedding behind it; 7 the corrector
 * launch of pp_sample_corrected) every launch of that
 * kernel made by pp_score / pp_sample / pp_proximal carries a start / stop HIP event pair on the launch stream
 * (hipExtLaunchKernelGGL: the dispatch's own begin and end, the interval rocprofv3's kernel trace reports);
 * pp_profile_read waits for the last one, returns the summed intervals (ms) and the number of
 * launches, and switches profiling off again. */
pp_status pp_profile_kernel(pp_ctx *ctx, int which);
pp_status pp_profile_read(pp_ctx *ctx, float *total_ms, int *launches);

/* Which edge kernels the library was built with (no reference counterpart; bench.py prices the roofline with it):
 * 1 = split-f16 MFMA with fp32-equivalent accuracy (default, csrc/pp_edge_f16.hip), 0 = exact-fp32 MFMA
 * (PACKPPI_EDGE=f32, csrc/pp_edge.hip). */
int pp_edge_variant(void);

/* f16 operand range check (no reference counterpart).  The default kernels run the dense layers on two-way f16 splits:
 * hidden activations saturate at 65504 and every other operand is assumed to be far below that.  A library built with
 * -DPP_CHECK_RANGE (libpackppi_hip.chk.so; `python -m packppi_amd.rangecheck`) counts every fp32 value at or beyond the
 * limit (or not finite) that its kernels were about to split: pp_range_check waits for the device, returns the events since
 * the last reset and optionally resets.  In any other build pp_has_range_check() is 0 and pp_range_check returns
 * PP_ERR_UNSUPPORTED.  (pp_plan_create rejects weights that are not finite or outside the f16 range in every build.) */
int pp_has_range_check(void);
pp_status pp_range_check(unsigned long long *events, int reset);
/* The same count by kernel family: the edge-level kernels and the node-level kernels.  libpackppi_hip.f32.so replaces BOTH
 * families by fp32 ones (fp32-MFMA edge kernels, csrc/pp_edge.hip; fp32 VALU node update, k_node_update_valu in
 * csrc/pp_node.hip): it has no f16 operand anywhere and is the build for a checkpoint that raises either count. */
pp_status pp_range_check_parts(unsigned long long *edge_events, unsigned long long *node_events, int reset);

/* Sticky saturation flag, every build (no reference counterpart).  The default kernels clamp hidden activations at the f16
 * maximum before splitting them; a context remembers that it happened: *flags bit 0 = in an edge-level kernel, bit 1 = in a
 * node-level kernel, 0 = never since pp_complex_prepare.  The call waits for `stream`.  A set bit means results of this
 * context are not fp32-equivalent for this checkpoint (run python -m packppi_amd.rangecheck for the details).
 * Bit 2 (value 4): a NaN or infinity ENTERED with the caller's tensors (backbone coordinates of an unmasked row at
 * pp_complex_prepare, an angle at pp_score / pp_sample).  The reference propagates it to its output (layers.py:22-33 has no
 * clamp); these kernels' clamps turn it into finite numbers that mean nothing -- the flag is how a caller learns of it.
 * Inside a sampling run the last node update of an evaluation reports bit 1 only for rows whose angles can move (the live rows
 * below, without the fixed rows of pp_sample_partial): what it computes for the others is returned to nobody.
 * Bit 3 (value 8): pp_hydrogens / pp_clashscore met a table entry or a residue_type outside its range and dropped the atom;
 * pp_hnet_optimize met such a mover entry and left the row alone. */
pp_status pp_ctx_saturated(pp_ctx *ctx, int *flags, void *stream);

/* Live rows (no reference counterpart): the rows of the context whose angles a sampling run can move --
 * residue_mask != 0 and at least one SC_D_mask entry != 0 --, in ascending order.  pp_sample / pp_sample_seeded run the layer-1
 * edge update of every evaluation on these rows only (nothing it computes for another row reaches the returned angles);
 * pp_sample_partial also leaves out the call's fixed rows.  PP_EDGE_LIVE=0 in the environment restores the launch over all rows
 * (same results).  rows is a DEVICE array [B*L] (packed ctx: [N]); the entries behind *count are -1.  Waits for `stream`. */
pp_status pp_ctx_live_rows(pp_ctx *ctx, int32_t *rows, int *count, void *stream);

/* The work table of the context's mixed live-row launch, read-only.  At the context sizes where a CU gets
 * three rows in one round, or a full round of two-row workgroups has a tail, the layer-1 edge update of a sampling run is one launch
 * of one- and two-row workgroups; a table made on the device next to the live-row list says which rows workgroup b takes.  mix is a
 * HOST array [N][2]: (r, s) two rows, (r, -1) one row, (-1, -1) no work; two-row entries come first.  *workgroups is the size of
 * that launch -- every live row sits in front of it -- or 0 for a context of another size (mix is then left alone).  A read-back
 * for tests and tools: it takes no stream and waits for the whole device.
 * pp_live_mix_host fills the same table on the host, without a device, for num_cu compute units: rows [N + 2] holds M rows and then
 * -1, mix is a HOST array [N][2].  Both run the same rule (the launch shape of M rows) and the same entry function. */
pp_status pp_ctx_live_mix(pp_ctx *ctx, int32_t *mix, int *workgroups);
pp_status pp_live_mix_host(const int32_t *rows, int M, int N, int num_cu, int32_t *mix, int *workgroups);

/* Diagnostics -- ONLY in libpackppi_hip.dbg.so (built with -DPP_DIAG; same kernels and results as the default library):
 * single launches, internal-buffer copies and a prefix of one network evaluation, for tools/debug/ and the per-layer parity
 * test (tests/test_hip_layers.py).  Not part of the drop-in boundary; the default, .f32 and .chk libraries do not export them
 * and read no environment switches. */
#ifdef PP_DIAG
pp_status pp_debug_edge(pp_ctx *ctx, int layer, void *stream);     /* one edge-update launch (+ next node message) */
pp_status pp_debug_nm(pp_ctx *ctx, int layer, void *stream);       /* one node-message launch */
pp_status pp_debug_set_hE(pp_ctx *ctx, const float *src, size_t n);
/* which: 0 h_E [N,K,128], 1 S [N,128], 2 msum [N], 3 h_E0, 4 Z_em, 5 h_V [N,128], 6 score [N,4], 7 the proximal loop's static
 * candidate counts [N,4] (int32 bits in the 4-byte slots; -1 = that wave scans), 8 the plan's side-chain extents [21], 9 the
 * loop's static obstacle candidate counts [N] (int32 bits; -1 = that row scans its range); waits for the device.
 * After pp_score / pp_sample, h_E holds layer 0's edges: the layer-1 edge update of an evaluation does not write it back
 * (pp_debug_score_prefix and pp_debug_edge do). */
pp_status pp_debug_buffer(pp_ctx *ctx, int which, float *dst, size_t n);
/* the first n_launches launches of pp_score's schedule (embed, NM0, NU0, EU0, NU1, EU1, NU2) */
pp_status pp_debug_score_prefix(pp_ctx *ctx, const float *chi, float t, int n_launches, void *stream);
/* out = {R, mixed, n_pairs, cl, multi}: the kernel instances a network evaluation of this context launches -- residues per edge /
 * node-message workgroup, the mixed pair + single launch and its pair count, workgroups per tile of a middle-layer node update,
 * the node update's instance for more tiles than CUs.  Asked of the launchers' own predicates (tests/test_launch_boundaries.py). */
pp_status pp_debug_launch_plan(pp_ctx *ctx, int32_t out[5]);
void pp_debug_set_dbg(float *p);          /* stamp buffer of the -DPP_LAB -DPP_X_TS builds */
void pp_debug_set_lds_pad(int bytes);     /* occupancy experiments */
void pp_debug_set_edge_R(int R);          /* residues per edge workgroup: 1, 2, 0 = automatic */
#endif

#ifdef __cplusplus
}
#endif
#endif /* PACKPPI_HIP_H */
