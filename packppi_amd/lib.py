"""ctypes binding of ``csrc/libpackppi_hip.so`` (the C ABI declared in ``include/packppi_hip.h``).

There is no CPU fallback: if the library is missing or a call fails, a ``RuntimeError`` is
raised (the reference CLIs only catch/re-raise ``RuntimeError``, eval_diffusion.py:61-64).
"""
import ctypes as C
import os

import numpy as np
import torch

from . import constants as rc
from .weights import check_state_dict

_LIB_PATH = os.environ.get("PACKPPI_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libpackppi_hip.so")     # PACKPPI_LIB: A/B runs of build variants
_lib = None

SYMBOLS = ("pp_version", "pp_last_error", "pp_build_id", "pp_plan_set_knn_ties", "pp_plan_set_annealed_temp", "pp_plan_rebalanced_chains", "pp_rebalance_weights_host", "pp_plan_ln_scaled_features", "pp_ln_operand_scales_host", "pp_topk_aten_host", "pp_plan_create", "pp_plan_destroy", "pp_plan_set_clash_params",
           "pp_complex_prepare", "pp_complex_prepare_packed", "pp_ctx_destroy", "pp_ctx_get_graph", "pp_ctx_set_graph", "pp_score", "pp_sample", "pp_atom14",
           "pp_clash", "pp_proximal", "pp_proximal_packed", "pp_time_kernel", "pp_profile_kernel", "pp_profile_read", "pp_edge_variant", "pp_has_range_check", "pp_range_check", "pp_range_check_parts", "pp_ctx_saturated",
           "pp_affinity_create", "pp_affinity_destroy", "pp_affinity_encode", "pp_affinity_predict",
           "pp_score_rows", "pp_so2_set_grids", "pp_so2_score", "pp_dsm_loss",
           "pp_ctx_set_rng_keys", "pp_noise_seeded", "pp_add_noise_seeded", "pp_sample_seeded",
           "pp_sample_partial", "pp_proximal_pinned", "pp_ctx_live_rows", "pp_ctx_live_mix", "pp_live_mix_host", "pp_ensemble_reduce", "pp_ctx_shell",
           "pp_ensemble_recombine", "pp_ctx_set_obstacles", "pp_sasa", "pp_sample_guided", "pp_sample_corrected",
           "pp_disulfide_close", "pp_polar", "pp_hydrogens", "pp_clashscore", "pp_hnet_optimize", "pp_chi_refine", "pp_anchor_close")


FIX_MODES = {"hold": 0, "renoise": 1}         # PP_FIX_HOLD, PP_FIX_RENOISE
KNN_TIES = {"lower_index": 0, "aten_cpu": 1, "aten_member": 2}
SELECT = {None: 0, "none": 0, "clash": 1, "medoid": 2}       # PP_SELECT_NONE, PP_SELECT_CLASH, PP_SELECT_MEDOID
SHELL_MODES = {"ca": 0, "atom": 1}            # PP_SHELL_CA, PP_SHELL_ATOM
SHELL_OTHER_CHAIN = 1                         # PP_SHELL_OTHER_CHAIN


class EnsembleResult(dict):
    """What ``Context.ensemble_reduce`` returns: a dict with attribute access (``res.mean``, ``res["mean"]``)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


DISULFIDE_OVERFLOW = ("disulfides: more cysteine pairs lie within cb_max than the candidate list of this context holds "
                      "(min(N (N - 1) / 2, 64 N)); nothing was bonded -- lower cb_max or name the pairs")


class DisulfideResult(EnsembleResult):
    """What ``Context.disulfides`` returns, all on the device: ``partner`` int32 [N] (the bonded partner's row or -1), ``report``
    fp32 [N, 4] (Emin, E at the pick, SG-SG distance, signed chi3 in radians; 0 on unbonded rows), ``count`` int32 [n_segments],
    ``chi`` [B, L, 4] (None for a detection without angles).  ``bonds()`` reads the pairs back."""

    def bonds(self):
        """[(a, b), ...] with a < b, ascending: the bonded row pairs, on the host (waits for the stream).  ``RuntimeError`` if the
        call overflowed its candidate list (count -1): it bonded nothing."""
        if bool((self["count"] < 0).any()):
            raise RuntimeError(DISULFIDE_OVERFLOW)
        p = self["partner"].reshape(-1).tolist()
        return [(a, b) for a, b in enumerate(p) if b > a]


class AnchorResult(EnsembleResult):
    """What ``Context.anchors`` returns, all on the device: ``status`` int32 [N] (0 none, 1 closed, 2 kept, -1 open, -2 an entry of
    the row was dropped), ``report`` fp32 [N, 4] (Emin, E at the pick, the first anchor's distance and angle), ``anchor_report`` fp32
    [A, 2] (distance and angle of every anchor at its row's pick), ``count`` int32 [n_segments] (closed rows), ``chi`` [B, L, 4]
    (None for a call without angles).  ``closed()`` and ``pinned()`` read the status back."""

    def _status(self):
        st = self["status"].reshape(-1).tolist()
        bad = [r for r, v in enumerate(st) if v == -2]
        if bad:
            raise RuntimeError(f"anchors: an entry of row {bad[0]} was dropped on the device (invalid, or a fifth anchor of the row); "
                               f"{len(bad)} such row(s) -- Context.check_anchors names the entry")
        return st

    def closed(self):
        """The closed rows, ascending, on the host (waits for the stream).  ``RuntimeError`` if the device dropped an entry
        (status -2)."""
        return [r for r, v in enumerate(self._status()) if v == 1]

    def pinned(self):
        """bool [N] on the device: the rows a later stage must not move -- closed or kept, and every row of status -2: its other
        anchors may have closed it (``chi`` then holds the grid angles), and a row whose angles were written is held whatever its
        status says.  No read-back."""
        st = self["status"].reshape(-1)
        return (st == 1) | (st == 2) | (st == -2)


class PPTables(C.Structure):
    _fields_ = [("default_frames", C.c_void_p), ("atom14_to_group", C.c_void_p), ("atom14_mask", C.c_void_p),
                ("lit_positions", C.c_void_p), ("between_radius", C.c_void_p)]


class PPBatch(C.Structure):
    _fields_ = [("B", C.c_int32), ("L", C.c_int32), ("X", C.c_void_p), ("atom_mask", C.c_void_p),
                ("residue_type", C.c_void_p), ("residue_mask", C.c_void_p), ("residue_index", C.c_void_p),
                ("chain_indices", C.c_void_p), ("BB_D", C.c_void_p), ("BB_D_sincos", C.c_void_p),
                ("SC_D", C.c_void_p), ("SC_D_mask", C.c_void_p), ("chi_1pi_periodic_mask", C.c_void_p),
                ("chi_2pi_periodic_mask", C.c_void_p)]


def load():
    """Load the shared library (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(f"{_LIB_PATH} is missing: build it with `python -m packppi_amd.build` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(_LIB_PATH)
    vp, f, i = C.c_void_p, C.c_float, C.c_int
    try:
        lib.pp_build_id.restype = C.c_char_p
    except AttributeError:
        raise RuntimeError(f"{_LIB_PATH} is stale: it predates the build stamp (no pp_build_id); rebuild with "
                           "`python -m packppi_amd.build` (or `python __graft_entry__.py`)") from None
    # a prebuilt library must come from the sources on disk (content hash, packppi_amd/build.py), and from one of the four
    # product flag sets: a tagged laboratory build (-DPP_LAB -DPP_X_...: timing variants, most with wrong results) only loads
    # with PACKPPI_ALLOW_LAB_LIBRARY=1
    if not os.environ.get("PACKPPI_SKIP_BUILD_CHECK"):
        from .build import product_flag_stamps, source_hash
        have, _, have_flags = lib.pp_build_id().decode().partition("-")
        want = source_hash()
        if have != want:
            raise RuntimeError(f"{_LIB_PATH} is stale: built from sources {have}, csrc/ is now {want}; rebuild with "
                               "`python -m packppi_amd.build` (or `python __graft_entry__.py`)")
        if have_flags not in product_flag_stamps() and not os.environ.get("PACKPPI_ALLOW_LAB_LIBRARY"):
            raise RuntimeError(f"{_LIB_PATH} was built with flags (stamp {have_flags}) that are none of the product sets "
                               f"{sorted(product_flag_stamps().values())}: a laboratory variant; set PACKPPI_ALLOW_LAB_LIBRARY=1 "
                               "to load it for a measurement")
    lib.pp_plan_set_knn_ties.argtypes = [vp, i]
    lib.pp_plan_set_annealed_temp.argtypes = [vp, f]
    lib.pp_plan_rebalanced_chains.argtypes = [vp]
    lib.pp_rebalance_weights_host.argtypes = [vp, C.c_size_t, vp, C.POINTER(C.c_int)]
    lib.pp_plan_rebalanced_chains.restype = C.c_int
    lib.pp_plan_ln_scaled_features.argtypes = [vp]
    lib.pp_plan_ln_scaled_features.restype = C.c_int
    lib.pp_ln_operand_scales_host.argtypes = [vp, C.c_size_t, vp, C.POINTER(C.c_int)]
    lib.pp_topk_aten_host.argtypes = [vp, i, i, vp]
    lib.pp_version.restype = C.c_int
    lib.pp_last_error.restype = C.c_char_p
    lib.pp_plan_create.argtypes = [vp, C.c_size_t, C.POINTER(PPTables), i, C.POINTER(vp)]
    lib.pp_plan_destroy.argtypes = [vp]
    lib.pp_plan_destroy.restype = None
    lib.pp_plan_set_clash_params.argtypes = [vp, f, vp, vp, vp]
    lib.pp_complex_prepare.argtypes = [vp, C.POINTER(PPBatch), vp, C.POINTER(vp)]
    lib.pp_complex_prepare_packed.argtypes = [vp, C.POINTER(PPBatch), vp, i, i, i, vp, C.POINTER(vp)]
    lib.pp_ctx_destroy.argtypes = [vp]
    lib.pp_ctx_destroy.restype = None
    lib.pp_ctx_get_graph.argtypes = [vp, vp, vp, vp]
    lib.pp_ctx_set_graph.argtypes = [vp, vp, vp]
    lib.pp_score.argtypes = [vp, vp, f, vp, vp, vp]
    lib.pp_sample.argtypes = [vp, vp, vp, i, i, vp, vp]
    lib.pp_atom14.argtypes = [vp, vp, vp, vp]
    lib.pp_clash.argtypes = [vp, vp, vp, vp, vp]
    lib.pp_proximal.argtypes = [vp, vp, f, i, vp, vp, vp, vp]
    lib.pp_proximal_packed.argtypes = [vp, vp, f, i, vp, vp, vp, vp, vp, vp]
    lib.pp_time_kernel.argtypes = [vp, i, i, C.POINTER(C.c_float), vp]
    lib.pp_profile_kernel.argtypes = [vp, i]
    lib.pp_profile_read.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    lib.pp_edge_variant.argtypes = []
    lib.pp_has_range_check.argtypes = []
    lib.pp_has_range_check.restype = C.c_int
    lib.pp_range_check.argtypes = [C.POINTER(C.c_ulonglong), i]
    lib.pp_range_check_parts.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), i]
    lib.pp_ctx_saturated.argtypes = [vp, C.POINTER(C.c_int), vp]
    lib.pp_edge_variant.restype = C.c_int
    lib.pp_affinity_create.argtypes = [vp, C.c_size_t, i, C.POINTER(vp)]
    lib.pp_affinity_destroy.argtypes = [vp]
    lib.pp_affinity_destroy.restype = None
    lib.pp_affinity_encode.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.pp_affinity_predict.argtypes = [vp, vp, vp, vp, i, i, vp, vp, vp]
    lib.pp_score_rows.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.pp_so2_set_grids.argtypes = [vp, vp, i]
    lib.pp_so2_score.argtypes = [vp, vp, C.c_size_t, i, vp, vp, i, vp]
    lib.pp_dsm_loss.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.pp_ctx_set_rng_keys.argtypes = [vp, vp, vp]
    lib.pp_noise_seeded.argtypes = [vp, C.c_uint64, i, vp, vp, vp]
    lib.pp_add_noise_seeded.argtypes = [vp, vp, f, C.c_uint64, vp, vp]
    lib.pp_sample_seeded.argtypes = [vp, vp, vp, i, i, C.c_uint64, vp]
    lib.pp_sample_partial.argtypes = [vp, vp, vp, vp, i, vp, i, i, C.c_uint64, vp, vp]
    lib.pp_proximal_pinned.argtypes = [vp, vp, vp, f, i, vp, vp, vp, vp, vp, vp, vp]
    lib.pp_ctx_live_rows.argtypes = [vp, vp, C.POINTER(C.c_int), vp]
    lib.pp_ctx_live_mix.argtypes = [vp, vp, C.POINTER(C.c_int)]
    lib.pp_live_mix_host.argtypes = [vp, i, i, i, vp, C.POINTER(C.c_int)]
    lib.pp_ensemble_reduce.argtypes = [vp, vp, i, vp, i, vp, vp, vp, vp, vp, vp, vp]
    lib.pp_ctx_shell.argtypes = [vp, vp, i, f, i, vp, vp, vp, vp]
    lib.pp_ensemble_recombine.argtypes = [vp, vp, i, vp, i, vp, vp, vp, vp, vp, vp, vp]
    lib.pp_ctx_set_obstacles.argtypes = [vp, vp, vp, i, vp]
    lib.pp_sasa.argtypes = [vp, vp, vp, vp, i, f, vp, vp, vp, vp]
    lib.pp_disulfide_close.argtypes = [vp, vp, vp, vp, i, f, f, f, vp, vp, vp, vp, vp]
    lib.pp_anchor_close.argtypes = [vp, vp, vp, vp, vp, vp, i, f, f, vp, vp, vp, vp, vp, vp]
    lib.pp_polar.argtypes = [vp, vp, vp, vp, vp, f, f, vp, vp, vp, vp, vp]
    lib.pp_hydrogens.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.pp_clashscore.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, f, f, vp, vp, vp, vp, vp]
    lib.pp_hnet_optimize.argtypes = [vp] * 20 + [f] * 6 + [C.c_int] + [vp] * 13
    lib.pp_chi_refine.argtypes = [vp] * 11 + [f, i, i] + [f] * 7 + [i] + [vp] * 16
    lib.pp_sample_guided.argtypes = [vp, vp, vp, vp, i, vp, i, i, C.c_uint64, vp, f, vp, vp, vp]
    lib.pp_sample_corrected.argtypes = [vp, vp, vp, vp, i, vp, i, i, C.c_uint64, vp, vp, f, vp, vp, vp, vp]
    _lib = lib
    return lib


def _check(status, what):
    if status != 0:
        msg = load().pp_last_error()
        raise RuntimeError(f"{what} failed (pp_status {status}): {msg.decode() if msg else ''}")


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _host_f32(seq):
    """A schedule (or the guide's step sizes) as the sampling exports read it: a contiguous float32 array on the host."""
    return np.ascontiguousarray(torch.as_tensor(seq, dtype=torch.float32).cpu().numpy())


def _mode_code(mode) -> int:      # PP_MODE_ODE / PP_MODE_SDE
    if mode not in ("ode", "sde"):
        raise NotImplementedError(mode)
    return 0 if mode == "ode" else 1


def _seed64(seed) -> int:
    """A seed or complex key as the unsigned 64-bit number the generator takes (negative values wrap)."""
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def ln_operand_scales(state_dict):
    """([5, 128] operand scales pp_plan_create would choose behind the edge-level LayerNorms -- rows: h_E0, h_E after layer 0,
    after layer 1, x1 of layer 0, of layer 1 --, how many differ from 1): host only, no device call."""
    lib = load()
    sd = check_state_dict(state_dict)
    flat = np.ascontiguousarray(torch.cat([v.reshape(-1) for v in sd.values()]).numpy(), dtype=np.float32)
    out = np.empty((5, 128), np.float32)
    n = C.c_int(0)
    _check(lib.pp_ln_operand_scales_host(flat.ctypes.data, flat.size, out.ctypes.data, C.byref(n)), "pp_ln_operand_scales_host")
    return torch.from_numpy(out), int(n.value)


def rebalanced_state_dict(state_dict):
    """(state_dict as pp_plan_create packs it, number of ReLU chains rescaled): host only, no device call.  The split-f16 build
    rescales the ReLU chains of the edge-level MLPs by powers of two (same function, hidden activations O(1))."""
    lib = load()
    sd = check_state_dict(state_dict)
    flat = np.ascontiguousarray(torch.cat([v.reshape(-1) for v in sd.values()]).numpy(), dtype=np.float32)
    out = np.empty_like(flat)
    n = C.c_int(0)
    _check(lib.pp_rebalance_weights_host(flat.ctypes.data, flat.size, out.ctypes.data, C.byref(n)), "pp_rebalance_weights_host")
    res, at = {}, 0
    for k, v in sd.items():
        res[k] = torch.from_numpy(out[at:at + v.numel()].reshape(tuple(v.shape)).copy())
        at += v.numel()
    return res, int(n.value)


class Plan:
    """Device-resident weights + chemistry tables (one per GPU)."""

    def __init__(self, state_dict, device):
        """``state_dict=None`` builds a geometry-only plan (atom14 / clash / proximal)."""
        lib = load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("packppi_amd runs on an MI355X HIP device only (got device '%s')" % device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.has_network = state_dict is not None
        if self.has_network:
            sd = check_state_dict(state_dict)
            flat = np.ascontiguousarray(torch.cat([v.reshape(-1) for v in sd.values()]).numpy(), dtype=np.float32)
            wptr, wn = flat.ctypes.data, flat.size
        else:
            wptr, wn = None, 0
        self._keep = [
            np.ascontiguousarray(rc.default_frames, np.float32), np.ascontiguousarray(rc.atom14_to_group, np.int32),
            np.ascontiguousarray(rc.atom14_mask, np.float32), np.ascontiguousarray(rc.lit_positions, np.float32),
            np.ascontiguousarray(rc.between_radius, np.float32)]
        tab = PPTables(*[a.ctypes.data for a in self._keep])
        h = C.c_void_p()
        _check(lib.pp_plan_create(wptr, wn, C.byref(tab), self.device.index, C.byref(h)), "pp_plan_create")
        self.handle = h
        self._clash_params = None
        self.knn_ties = "aten_cpu"
        if os.environ.get("PACKPPI_KNN_TIES"):
            self.set_knn_ties(os.environ["PACKPPI_KNN_TIES"])

    def set_knn_ties(self, mode):
        """What the neighbour search does on exactly equal CA distances: "aten_cpu" (default: the reference CPU path's
        torch.topk choice and order), "aten_member" (that choice only where membership depends on it) or "lower_index"."""
        if mode not in KNN_TIES:
            raise ValueError(f"knn ties mode must be one of {sorted(KNN_TIES)}")
        _check(load().pp_plan_set_knn_ties(self.handle, KNN_TIES[mode]), "pp_plan_set_knn_ties")
        self.knn_ties = mode

    def rebalanced_chains(self) -> int:
        """How many ReLU chains of the edge-level MLPs the split-f16 build rescaled by a power of two at plan creation."""
        return int(load().pp_plan_rebalanced_chains(self.handle))

    def ln_scaled_features(self) -> int:
        """How many of the 5 x 128 LayerNorm-output operand features of the edge kernels carry a power-of-two scale (split-f16 build;
        0 for weights whose LayerNorm gains and biases are of ordinary size)."""
        return int(load().pp_plan_ln_scaled_features(self.handle))

    def set_annealed_temp(self, T):
        """sample_cfg.annealed_temp (Sampling.yaml:4): the T of the annealed score weight in SO2VESchedule.step."""
        _check(load().pp_plan_set_annealed_temp(self.handle, float(T)), "pp_plan_set_annealed_temp")

    def set_clash_params(self, vtf, tol):
        key = (float(vtf), float(tol))
        if self._clash_params == key:
            return
        lo, up = rc.make_atom14_dists_bounds(overlap_tolerance=float(tol), bond_length_tolerance_factor=float(vtf))
        lo, up = np.ascontiguousarray(lo, np.float32), np.ascontiguousarray(up, np.float32)
        _check(load().pp_plan_set_clash_params(self.handle, float(tol), lo.ctypes.data, up.ctypes.data,
                                               _stream(self.device)), "pp_plan_set_clash_params")
        self._clash_params = key

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and _lib is not None:
            _lib.pp_plan_destroy(h)
            self.handle = None


_BATCH_SPEC = (("X", torch.float32), ("atom_mask", torch.float32), ("residue_type", torch.int64),
               ("residue_mask", torch.float32), ("residue_index", torch.int64), ("chain_indices", torch.int64),
               ("BB_D", torch.float32), ("BB_D_sincos", torch.float32), ("SC_D", torch.float32),
               ("SC_D_mask", torch.float32), ("chi_1pi_periodic_mask", torch.bool),
               ("chi_2pi_periodic_mask", torch.bool))


def _get(batch, key):
    return batch.get(key) if hasattr(batch, "get") else getattr(batch, key, None)


class BatchKey:
    """What a cached ``Context`` is valid for: the batch tensors themselves (held, so that their storage cannot be handed to
    another batch while the key lives) and their version counters -- an in-place edit of ``batch.X``, ``residue_mask``,
    ``residue_index`` ... bumps ``_version`` and the graph, frames and edge embedding are rebuilt, as the reference recomputes
    them on every call (encoder.py:198-246).  A tensor the context had to copy (dtype / layout) is covered the same way: the
    key watches the caller's tensor, not the copy."""

    KEYS = tuple(k for k, _ in _BATCH_SPEC) + ("seg_offsets", "obstacle_xyzr", "obstacle_offsets", "obstacle_polar")

    def __init__(self, batch):
        self.tensors = [t if isinstance(t, torch.Tensor) else None for t in (_get(batch, k) for k in self.KEYS)]
        self.meta = self._meta(self.tensors)

    @staticmethod
    def _meta(ts):
        # tensors made under torch.inference_mode() (Lightning's test / predict loops) track no version counter: reading
        # `_version` raises.  They get no version in the key -- and never match (below)
        return [None if t is None else ((None if t.is_inference() else t._version), tuple(t.shape), t.dtype) for t in ts]

    def matches(self, batch) -> bool:
        ts = [t if isinstance(t, torch.Tensor) else None for t in (_get(batch, k) for k in self.KEYS)]
        if any(t is not None and t.is_inference() for t in ts):
            # an in-place edit of an inference tensor cannot be seen (no version counter, same data_ptr): the context is
            # rebuilt on every call, as the reference recomputes graph and embedding on every call (encoder.py:198-246)
            return False
        return all(a is b for a, b in zip(ts, self.tensors)) and self._meta(ts) == self.meta


class Context:
    """One batch of complexes on one GPU: cached kNN graph, edge embedding, frames, workspaces."""

    def __init__(self, plan: Plan, batch):
        lib = load()
        self.plan = plan
        dev = plan.device
        B, L = batch["residue_type"].shape
        self.B, self.L, self.K = int(B), int(L), min(32, int(L))
        self._t = {}
        # tensors this context made and hands to the kernels by raw pointer, and the streams it has run on (``_stream``)
        self._owned, self._streams = [], {}
        for key, dt in _BATCH_SPEC:
            t = _get(batch, key)
            if t is None:
                if plan.has_network or key in ("X", "residue_type", "BB_D"):
                    raise RuntimeError(f"batch.{key} is missing")
                self._t[key] = None
                continue
            if t.device.type != "cuda" or (t.device.index is not None and t.device.index != dev.index):
                raise RuntimeError(f"batch.{key} is on {t.device}, expected {dev} (call batch.to(device) first)")
            self._t[key] = self._own(t.to(dt).contiguous(), t)
        pb = PPBatch(self.B, self.L, *[(self._t[k].data_ptr() if self._t[k] is not None else None)
                                       for k, _ in _BATCH_SPEC])
        h = C.c_void_p()
        # every context has one segment table (csrc/pp_segments.h): the complexes' first rows and the total (host list) --
        # a padded batch 0, L, 2L ..., a packed batch (``packed``) its own
        seg = _get(batch, "seg_offsets")
        self.packed = seg is not None
        if not self.packed:
            self.seg_offsets_host = [s * self.L for s in range(self.B + 1)]
            _check(lib.pp_complex_prepare(plan.handle, C.byref(pb), self._stream(), C.byref(h)), "pp_complex_prepare")
        else:
            # ragged batch without padding rows (batch.pack): [1, sum of lengths, ...] + the complexes' first rows; the host
            # copy of the table that pack() carries along saves the read-back
            host = _get(batch, "seg_offsets_host")
            offs = [int(x) for x in (host if host is not None else seg.tolist())]
            # the device table is what the kernels index with, the host copy is what K and the launch sizes come from: they
            # must be the same table (a batch sliced or edited after pack() would only be clamped on the device)
            if len(offs) != seg.numel():
                raise RuntimeError(f"seg_offsets has {seg.numel()} entries, seg_offsets_host {len(offs)}")
            if host is not None and seg.device.type == "cpu" and [int(x) for x in seg.tolist()] != offs:
                raise RuntimeError("seg_offsets and seg_offsets_host disagree")
            lens = [b - a for a, b in zip(offs[:-1], offs[1:])]
            if self.B != 1 or len(offs) < 2 or offs[-1] != self.L or offs[0] != 0 or min(lens) < 1:
                raise RuntimeError("seg_offsets does not describe this batch")
            self._t["seg_offsets"] = self._own(seg.to(device=dev, dtype=torch.int32).contiguous(), seg)
            self.seg_offsets_host = offs
            self.K = min(32, min(lens))
            _check(lib.pp_complex_prepare_packed(plan.handle, C.byref(pb), self._t["seg_offsets"].data_ptr(), len(lens),
                                                 min(lens), max(lens), self._stream(), C.byref(h)),
                   "pp_complex_prepare_packed")
        self.handle = h
        self.n_obstacles = 0
        ox = _get(batch, "obstacle_xyzr")
        if ox is not None:
            self.set_obstacles(ox, self._obstacle_ranges(batch), polar=_get(batch, "obstacle_polar"))

    def _obstacle_ranges(self, batch):
        """(first, count) per segment from the batch's ``obstacle_offsets``: one range per segment, or, in a batch of decoys
        (``n_decoys``), one per group, shared by the group's segments."""
        host = _get(batch, "obstacle_offsets_host")
        offs = [int(x) for x in (host if host is not None else _get(batch, "obstacle_offsets").tolist())]
        n_seg, n_rng = self.n_segments, len(offs) - 1
        D = int(_get(batch, "n_decoys") or 1)
        if n_rng == n_seg:
            D = 1
        elif n_rng * D != n_seg:
            raise RuntimeError(f"obstacle_offsets describes {n_rng} ranges, the batch has {n_seg} segments (n_decoys {D})")
        return [(offs[s // D], offs[s // D + 1] - offs[s // D]) for s in range(n_seg)]

    def set_obstacles(self, xyzr=None, seg_range=None, polar=None):
        """Install fixed obstacle atoms (pp_ctx_set_obstacles): ``xyzr`` [M, 4] (x, y, z, radius),
        ``seg_range`` one (first, count) per segment (default: every segment owns all M).  ``clash``, the ``proximal*`` calls and
        ``ensemble_recombine`` then count the overlap of every side-chain atom with the obstacles of its segment.  ``xyzr`` None or
        empty clears the set: every call then gives the bits of a context that never had one.  The context keeps its own copy.
        ``ValueError``: a range outside the atoms; non-finite coordinates or radii or a negative radius in a host tensor (in a device
        tensor they are found on the device and set bit 2 of ``saturated()``: no read-back here).  ``polar`` [M] (non-zero = a polar
        atom; the batch's ``obstacle_polar``): what ``polar()`` counts as obstacle partners unless it is told otherwise; None:
        none of them.  Only ``polar()`` reads it."""
        dev = self.plan.device
        self._obst_polar = None
        if xyzr is None or xyzr.numel() == 0:
            _check(load().pp_ctx_set_obstacles(self.handle, None, None, 0, self._stream()), "pp_ctx_set_obstacles")
            self.n_obstacles = 0
            return
        src = torch.as_tensor(xyzr)
        if src.device.type == "cpu" and (not bool(torch.isfinite(src).all()) or bool((src.reshape(-1, 4)[:, 3] < 0).any())):
            raise ValueError("obstacle coordinates and radii must be finite, radii not negative")
        x = src.to(device=dev, dtype=torch.float32).reshape(-1, 4).contiguous()
        M = int(x.shape[0])
        if seg_range is None:
            seg_range = [(0, M)] * self.n_segments
        rng = np.ascontiguousarray([[int(a), int(b)] for a, b in seg_range], dtype=np.int32)
        if rng.shape != (self.n_segments, 2):
            raise ValueError(f"seg_range has {rng.shape[0]} entries for {self.n_segments} segments")
        if (rng < 0).any() or (rng.sum(1) > M).any():
            raise ValueError(f"seg_range reaches outside the {M} obstacle atoms")
        _check(load().pp_ctx_set_obstacles(self.handle, _ptr(x), C.c_void_p(rng.ctypes.data), M, self._stream()), "pp_ctx_set_obstacles")
        self.n_obstacles = M
        if polar is not None:
            pol = (torch.as_tensor(polar).to(device=dev) != 0).to(torch.uint8).reshape(-1).contiguous()
            if pol.numel() != M:
                raise ValueError(f"polar has {pol.numel()} entries for {M} obstacle atoms")
            self._obst_polar = self._own(pol)

    def _own(self, t, src=None):
        """Register a tensor the context keeps and passes to the kernels by raw pointer (a converted copy of a batch tensor, a
        cached table).  torch's caching allocator ties its memory to the stream that was current when it was made and knows
        nothing of the kernels that read it through ``data_ptr()``: every other stream the context runs on is recorded on it
        (``Tensor.record_stream``), so that dropping the context cannot hand the memory out while such a stream still reads it.
        ``src``: the caller's tensor -- if the conversion was no copy the memory is the caller's, and so is that duty."""
        if t is not src:
            self._owned.append(t)
            for s in self._streams.values():
                t.record_stream(s)
        return t

    def _stream(self):
        """The current stream as the exports take it.  The first call under a stream records it on the context's own tensors
        (``_own``): host bookkeeping of the allocator, once per (context, stream), no device call."""
        s = torch.cuda.current_stream(self.plan.device)
        if s.cuda_stream not in self._streams:
            self._streams[s.cuda_stream] = s
            for t in self._owned:
                t.record_stream(s)
        return C.c_void_p(s.cuda_stream)

    def _new(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.plan.device)

    def _chi(self, chi):
        return chi.to(device=self.plan.device, dtype=torch.float32).reshape(self.B, self.L, 4).contiguous()

    def graph(self):
        E = self._new(self.B, self.L, self.K, dtype=torch.int64)
        hE = self._new(self.B, self.L, self.K, 128)
        _check(load().pp_ctx_get_graph(self.handle, _ptr(E), _ptr(hE), self._stream()), "pp_ctx_get_graph")
        return E, hE

    def set_graph(self, E_idx):
        """Use the caller's neighbour lists [B, L, K] (per-complex numbering) instead of the built-in search."""
        E = E_idx.to(device=self.plan.device, dtype=torch.int64).reshape(self.B, self.L, self.K).contiguous()
        _check(load().pp_ctx_set_graph(self.handle, _ptr(E), self._stream()), "pp_ctx_set_graph")

    def score(self, chi, t):
        """``t``: a number, or a tensor; one with mixed values ([B*L], packed: [N]) goes to ``score_rows``."""
        if isinstance(t, torch.Tensor) and t.numel() > 1:
            if not bool((t == t.reshape(-1)[0]).all()):
                return self.score_rows(chi, t)
            t = t.reshape(-1)[0]
        chi = self._chi(chi)
        score, hV = self._new(self.B, self.L, 4), self._new(self.B, self.L, 128)
        _check(load().pp_score(self.handle, _ptr(chi), float(t), _ptr(score), _ptr(hV), self._stream()),
               "pp_score")
        return score, hV

    @property
    def n_rows(self) -> int:
        return self.B * self.L

    @property
    def n_segments(self) -> int:
        """Complexes of a packed context, else the B rows of the padded batch."""
        return len(self.seg_offsets_host) - 1

    def _rows(self, t, what, width=1):
        t = t.to(device=self.plan.device, dtype=torch.float32).contiguous()
        if t.numel() != self.n_rows * width:
            raise ValueError(f"{what} has {t.numel()} elements, this context has {self.n_rows} rows x {width}")
        return t

    def _mask(self, t, what):
        """A per-row mask (one element per row, host or device; non-zero = set) as the exports read it: uint8 [N] on the device."""
        t = torch.as_tensor(t).to(device=self.plan.device)
        if t.numel() != self.n_rows:
            raise ValueError(f"{what} has {t.numel()} elements, this context has {self.n_rows} rows")
        return (t != 0).to(torch.uint8).reshape(-1).contiguous()

    def _xyz(self, xyz):
        xyz = xyz.to(device=self.plan.device, dtype=torch.float32).contiguous()
        if xyz.numel() != self.n_rows * 42:
            raise ValueError(f"xyz has {xyz.numel()} elements, this context has {self.n_rows} rows x 14 x 3")
        return xyz

    def score_rows(self, chi, t_rows):
        """``score`` with a time per row ([B*L], packed: [N]): pp_score_rows.  ``t_rows`` is not modified."""
        chi, t_rows = self._chi(chi), self._rows(t_rows, "t")
        score, hV = self._new(self.B, self.L, 4), self._new(self.B, self.L, 128)
        _check(load().pp_score_rows(self.handle, _ptr(chi), _ptr(t_rows), _ptr(score), _ptr(hV), self._stream()),
               "pp_score_rows")
        return score, hV

    def dsm_loss(self, pred_score, target_score, t_rows, score_norm):
        """(num [n_segments], den [n_segments]) fp64 on the device: the masked, normalised squared error of
        TorsionalDiffusion.py:139-153 per segment.  ``score_norm``: fp64 [2, 5001] on the device (1pi, 2pi)."""
        pred, tgt, t_rows = self._rows(pred_score, "pred_score", 4), self._rows(target_score, "target_score", 4), self._rows(t_rows, "t")
        if score_norm.dtype != torch.float64 or tuple(score_norm.shape) != (2, SO2_GRID) or score_norm.device != self.plan.device:
            raise ValueError(f"score_norm must be a float64 [2, {SO2_GRID}] tensor on {self.plan.device}")
        num, den = self._new(self.n_segments, dtype=torch.float64), self._new(self.n_segments, dtype=torch.float64)
        _check(load().pp_dsm_loss(self.handle, _ptr(pred), _ptr(tgt), _ptr(t_rows), _ptr(score_norm.contiguous()), _ptr(num), _ptr(den),
                                  self._stream()), "pp_dsm_loss")
        return num, den

    # ---- seeded sampling noise, generated on the device (csrc/pp_rng.h) ----------------------------
    def set_rng_keys(self, keys=None):
        """The 64-bit keys of this context's segments (complexes of a packed batch, else the B rows): a list or int64 tensor, one
        entry per segment; None restores the default 0, 1, 2 ...  The noise of a complex depends on its key, never on where it
        sits in the batch."""
        arr = None
        if keys is not None:
            keys = keys.tolist() if isinstance(keys, torch.Tensor) else list(keys)
            arr = np.ascontiguousarray([_seed64(k) for k in keys], dtype=np.uint64)
            if arr.size != self.n_segments:
                raise ValueError(f"{arr.size} complex keys for {self.n_segments} complexes")
        _check(load().pp_ctx_set_rng_keys(self.handle, C.c_void_p(arr.ctypes.data) if arr is not None else C.c_void_p(0),
                                          self._stream()), "pp_ctx_set_rng_keys")

    def noise(self, seed, step, want_words=False):
        """What the seeded sampler draws at ``step`` (-1: the initial noising): [2, N, 4] fp32, the 1pi draw then the 2pi draw --
        one step's slice of ``sample``'s ``sde_noise``.  ``want_words``: also the raw Philox words, int32 [N, 4, 4] holding the
        unsigned 32-bit patterns."""
        nz = self._new(2, self.n_rows, 4)
        words = self._new(self.n_rows, 4, 4, dtype=torch.int32) if want_words else None
        _check(load().pp_noise_seeded(self.handle, _seed64(seed), int(step), _ptr(nz), _ptr(words), self._stream()),
               "pp_noise_seeded")
        return (nz, words) if want_words else nz

    def add_noise(self, chi, t, seed):
        """``add_sc_noise`` at one shared time ``t`` with the step = -1 draws of ``seed``: [B, L, 4]."""
        chi = self._chi(chi)
        out = torch.empty_like(chi)
        _check(load().pp_add_noise_seeded(self.handle, _ptr(chi), float(t), _seed64(seed), _ptr(out), self._stream()),
               "pp_add_noise_seeded")
        return out

    def sample(self, chi, schedule, mode="ode", sde_noise=None, seed=None):
        """``seed``: the sde draws come from the device generator inside the reverse step (pp_sample_seeded; no noise tensor);
        ``sde_noise`` must then be None.  Without a seed: pp_sample."""
        chi = self._chi(chi).clone()
        sched = _host_f32(schedule)
        md = _mode_code(mode)
        if seed is not None:
            if sde_noise is not None:
                raise ValueError("seed and sde_noise exclude each other: the seeded sampler draws its own noise")
            _check(load().pp_sample_seeded(self.handle, _ptr(chi), sched.ctypes.data, int(len(sched)), md, _seed64(seed),
                                           self._stream()), "pp_sample_seeded")
            return chi
        nz = None
        if mode == "sde":
            if sde_noise is None:
                raise RuntimeError("sde sampling needs the per-step noise tensor")
            nz = sde_noise.to(device=self.plan.device, dtype=torch.float32).contiguous()
            assert nz.numel() == (len(sched) - 1) * 2 * self.B * self.L * 4
        _check(load().pp_sample(self.handle, _ptr(chi), sched.ctypes.data, int(len(sched)), md, _ptr(nz), self._stream()),
               "pp_sample")
        return chi

    def sample_partial(self, chi, chi_ref, fixed, schedule, mode, seed, fix_mode="renoise", trajectory=False):
        """Partial repacking (pp_sample_partial): rows with ``fixed`` != 0 ([B, L] bool / uint8, packed: [1, N])
        keep ``chi_ref``, the others are sampled as ``sample(..., seed=seed)`` samples them.  ``fix_mode``: "hold" (fixed rows are
        ``chi_ref`` at every step) or "renoise" (``chi_ref`` re-noised to each step's level with that step's own draws; ``chi_ref``
        after the last step).  ``chi`` is the step-0 state of EVERY row -- the call does not initialise the fixed ones.  Returns the
        sample [B, L, 4], with ``trajectory`` also the angles after every step [n_steps, B, L, 4]."""
        md = _mode_code(mode)
        if fix_mode not in FIX_MODES:
            raise ValueError(f"fix_mode must be one of {sorted(FIX_MODES)}")
        chi = self._chi(chi).clone()
        ref = self._chi(chi_ref)
        fx = self._mask(fixed, "fixed")
        sched = _host_f32(schedule)
        traj = self._new(max(len(sched) - 1, 0), self.B, self.L, 4) if trajectory else None
        _check(load().pp_sample_partial(self.handle, _ptr(chi), _ptr(ref), _ptr(fx), FIX_MODES[fix_mode], sched.ctypes.data,
                                        int(len(sched)), md, _seed64(seed), _ptr(traj), self._stream()), "pp_sample_partial")
        return (chi, traj) if trajectory else chi

    def sample_guided(self, chi, schedule, mode, seed, eta, cap=0.1, chi_ref=None, fixed=None, fix_mode="renoise",
                      trajectory=False, want_trace=False, vtf=12.0, tol=0.5):
        """Clash-guided sampling (pp_sample_guided): ``sample(..., seed=seed)`` -- with ``chi_ref`` and
        ``fixed`` ``sample_partial`` -- with a gradient step on the clash loss (obstacle atoms included) at every nudge point j whose
        ``eta[j]`` is not 0: point j < n_schedule - 1 in front of network evaluation j, the last one behind the last reverse step.
        ``eta``: n_schedule step sizes (``schedule.guide_eta``), finite and not negative; ``cap``: the largest step of one angle at one
        nudge in radians (inf = no clamp).  Fixed rows are never nudged.  With ``eta`` all 0 the result has the bits of ``sample`` /
        ``sample_partial``.  Needs a packed or B = 1 context.  Returns the sample [B, L, 4]; with ``trajectory`` also the angles after
        every reverse step [n_steps, B, L, 4] (in front of the nudge that follows); with ``want_trace`` also the mean clash of every
        segment in front of every nudge, fp64 [n_segments, n_schedule], NaN where ``eta`` is 0.  No host synchronisation."""
        md = _mode_code(mode)
        if (chi_ref is None) != (fixed is None):
            raise ValueError("chi_ref and fixed go together: give both (a pinned run) or neither")
        if fixed is not None and fix_mode not in FIX_MODES:
            raise ValueError(f"fix_mode must be one of {sorted(FIX_MODES)}")
        sched = _host_f32(schedule)
        et = _host_f32(eta).reshape(-1)
        if et.size != sched.size:
            raise ValueError(f"eta has {et.size} entries, the schedule has {sched.size} times (one nudge point per time)")
        self.plan.set_clash_params(vtf, tol)
        chi = self._chi(chi).clone()
        ref = fx = None
        if fixed is not None:
            ref, fx = self._chi(chi_ref), self._mask(fixed, "fixed")
        traj = self._new(max(len(sched) - 1, 0), self.B, self.L, 4) if trajectory else None
        trace = self._new(self.n_segments, len(sched), dtype=torch.float64) if want_trace else None
        _check(load().pp_sample_guided(self.handle, _ptr(chi), _ptr(ref), _ptr(fx), FIX_MODES.get(fix_mode, 1), sched.ctypes.data,
                                       int(len(sched)), md, _seed64(seed if seed is not None else 0),
                                       et.ctypes.data, float(cap), _ptr(traj), _ptr(trace), self._stream()),
               "pp_sample_guided")
        out = (chi,) + ((traj,) if trajectory else ()) + ((trace,) if want_trace else ())
        return out if len(out) > 1 else chi

    def sample_corrected(self, chi, schedule, mode, seed, snr, eta=None, cap=0.1, chi_ref=None, fixed=None, fix_mode="renoise",
                         trajectory=False, want_trace=False, want_corr=False, vtf=12.0, tol=0.5):
        """Predictor-corrector sampling (pp_sample_corrected): ``sample(..., seed=seed)`` -- with ``chi_ref`` and
        ``fixed`` ``sample_partial``, with ``eta`` ``sample_guided`` -- with one Langevin corrector behind every reverse step j whose
        ``snr[j]`` is not 0: a network evaluation at the new state and time, then x += eps s + sqrt(2 eps) z on the movable angles,
        eps = 2 (snr |z| / |s|)^2 with the two norms taken PER COMPLEX (the reference's ``step_correct`` averages them over the
        batch), z from the device generator at counter step 2^20 + j.  ``snr``: n_schedule - 1 values (``schedule.corrector_snr``),
        finite and not negative.  Fixed rows are never moved and never counted.  With ``snr`` all 0 the result has the bits of
        ``sample`` / ``sample_partial`` / ``sample_guided``.  Any context; with ``eta`` a packed or B = 1 one.  Returns the sample
        [B, L, 4]; with ``trajectory`` also the angles after every reverse step [n_steps, B, L, 4], IN FRONT OF that step's corrector;
        with ``want_trace`` (needs ``eta``) the guide's clash trace; with ``want_corr`` (s2, n2, eps, amp) of every segment and
        step, fp64 [n_segments, n_steps, 4], NaN where there is no corrector.  No host synchronisation."""
        md = _mode_code(mode)
        if (chi_ref is None) != (fixed is None):
            raise ValueError("chi_ref and fixed go together: give both (a pinned run) or neither")
        if fixed is not None and fix_mode not in FIX_MODES:
            raise ValueError(f"fix_mode must be one of {sorted(FIX_MODES)}")
        if want_trace and eta is None:
            raise ValueError("want_trace is the guide's clash trace: it needs eta")
        sched = _host_f32(schedule)
        sn = _host_f32(snr).reshape(-1)
        if sn.size != max(sched.size - 1, 0):
            raise ValueError(f"snr has {sn.size} entries, the schedule has {max(sched.size - 1, 0)} reverse steps (one corrector point per step)")
        et = None
        if eta is not None:
            et = _host_f32(eta).reshape(-1)
            if et.size != sched.size:
                raise ValueError(f"eta has {et.size} entries, the schedule has {sched.size} times (one nudge point per time)")
            self.plan.set_clash_params(vtf, tol)
        chi = self._chi(chi).clone()
        ref = fx = None
        if fixed is not None:
            ref, fx = self._chi(chi_ref), self._mask(fixed, "fixed")
        n = max(len(sched) - 1, 0)
        traj = self._new(n, self.B, self.L, 4) if trajectory else None
        trace = self._new(self.n_segments, len(sched), dtype=torch.float64) if want_trace else None
        corr = self._new(self.n_segments, n, 4, dtype=torch.float64) if want_corr else None
        _check(load().pp_sample_corrected(self.handle, _ptr(chi), _ptr(ref), _ptr(fx), FIX_MODES.get(fix_mode, 1), sched.ctypes.data,
                                          int(len(sched)), md, _seed64(seed), sn.ctypes.data,
                                          et.ctypes.data if et is not None else None, float(cap), _ptr(traj), _ptr(trace), _ptr(corr),
                                          self._stream()), "pp_sample_corrected")
        out = (chi,) + ((traj,) if trajectory else ()) + ((trace,) if want_trace else ()) + ((corr,) if want_corr else ())
        return out if len(out) > 1 else chi

    def atom14(self, chi):
        chi = self._chi(chi)
        xyz = self._new(self.B, self.L, 14, 3)
        _check(load().pp_atom14(self.handle, _ptr(chi), _ptr(xyz), self._stream()), "pp_atom14")
        return xyz

    def clash(self, chi, vtf=12.0, tol=0.5, need_grad=False):
        """per_res [B, L] (and its chi gradient) of pp_clash; on a context with obstacle atoms the overlap with them is included."""
        self.plan.set_clash_params(vtf, tol)
        chi = self._chi(chi)
        per_res = self._new(self.B, self.L)
        dchi = self._new(self.B, self.L, 4) if need_grad else None
        _check(load().pp_clash(self.handle, _ptr(chi), _ptr(per_res), _ptr(dchi), self._stream()), "pp_clash")
        return (per_res, dchi) if need_grad else per_res

    def proximal(self, chi, vtf, tol, lamda, num_steps, want_traj=True):
        """proximal_optimizer for the one complex of a B = 1 batch: the single-complex case of the loop ``proximal_packed`` runs, without
        the accept rule.  Returns (traj [num_steps, 1, L, 4] or None, last [1, L, 4], losses [num_steps]) on the device."""
        self.plan.set_clash_params(vtf, tol)
        chi = self._chi(chi)
        traj = self._new(num_steps, self.B, self.L, 4) if want_traj else None
        last = self._new(self.B, self.L, 4)
        losses = self._new(num_steps)
        _check(load().pp_proximal(self.handle, _ptr(chi), float(lamda), int(num_steps), _ptr(traj), _ptr(last),
                                  _ptr(losses), self._stream()), "pp_proximal")
        return traj, last, losses

    def proximal_packed(self, chi, vtf, tol, lamda, num_steps, norm_rows=None, want_traj=False, fixed=None, return_moved=False):
        """proximal_optimizer for every complex of a packed batch at once (a B = 1 batch counts as one complex): each complex with its
        own clash mask, 1/n, losses and accept rule.  The same loop as ``proximal``, which is its one-complex case: a complex gets the
        bits it gets alone.  ``norm_rows`` (one int per complex, or
        None = the complexes' lengths): the row count each complex's means divide by; pass the padded ``max_size`` to reproduce the
        run on a padded batch.  Returns (traj [num_steps, 1, N, 4] or None, last [1, N, 4], accepted [1, N, 4],
        losses [n_complexes, num_steps]), all on the device; no host synchronisation.

        ``fixed`` ([1, N] bool / uint8, as in ``sample_partial``; pp_proximal_pinned): rows with ``fixed`` != 0 are
        taken out of the clash mask -- its mean stays over all rows -- and come out as ``chi`` bit for bit; with ``return_moved`` the
        mask that was optimised (bool [1, N]) is appended to the tuple."""
        if return_moved and fixed is None:
            raise ValueError("return_moved needs fixed: the unpinned call does not report its mask (functional.find_clash_mask does)")
        self.plan.set_clash_params(vtf, tol)
        offs, n_seg = self.seg_offsets_host, self.n_segments
        nr = None
        if norm_rows is not None:
            nr = np.ascontiguousarray([int(x) for x in norm_rows], dtype=np.int32)
            if nr.size != n_seg:
                raise ValueError(f"norm_rows has {nr.size} entries for {n_seg} complexes")
            lens = [b - a for a, b in zip(offs[:-1], offs[1:])]
            short = [(k, int(r), n) for k, (r, n) in enumerate(zip(nr, lens)) if r < n]
            if self.B == 1 and short:
                k, r, n = short[0]
                raise ValueError(f"norm_rows[{k}] = {r} is shorter than complex {k} ({n} rows)")
        chi = self._chi(chi)
        traj = self._new(num_steps, self.B, self.L, 4) if want_traj else None
        last, accepted = self._new(self.B, self.L, 4), self._new(self.B, self.L, 4)
        losses = self._new(n_seg, max(int(num_steps), 1))
        nrp = C.c_void_p(nr.ctypes.data) if nr is not None else C.c_void_p(0)
        if fixed is None:
            _check(load().pp_proximal_packed(self.handle, _ptr(chi), float(lamda), int(num_steps), nrp, _ptr(traj), _ptr(last),
                                             _ptr(accepted), _ptr(losses), self._stream()), "pp_proximal_packed")
            return traj, last, accepted, losses
        fx = self._mask(fixed, "fixed")
        moved = self._new(self.B, self.L, dtype=torch.uint8) if return_moved else None
        _check(load().pp_proximal_pinned(self.handle, _ptr(chi), _ptr(fx), float(lamda), int(num_steps), nrp, _ptr(traj), _ptr(last),
                                         _ptr(accepted), _ptr(losses), _ptr(moved), self._stream()), "pp_proximal_pinned")
        return (traj, last, accepted, losses, moved.bool()) if return_moved else (traj, last, accepted, losses)

    def ensemble_reduce(self, chi, n_decoys, per_res=None, select=None, want_best=True):
        """Consensus, confidence, scores and selection over the decoys of this context (pp_ensemble_reduce).
        The context's segments are groups of ``n_decoys`` consecutive segments of equal length (``batch.replicate`` /
        ``replicate_many``); checked here against the host table, before any launch.  ``chi`` [1, N, 4]; ``per_res`` [N]: ``clash`` at
        those angles, or None; ``select``: "clash" (needs ``per_res``), "medoid" (the decoy closest to the consensus) or None
        (decoy 0); the numbers 1, 2, 0 are accepted too.  Returns an ``EnsembleResult``: ``mean``, ``resultant`` [1, N / D, 4] fp32,
        ``dev``, ``clash`` fp64 [n_segments] (``clash`` None without ``per_res``), ``best`` int32 [n_groups], ``chi_best``
        [1, N / D, 4] (None without ``want_best``), all on the device; no host synchronisation."""
        from .batch import check_groups
        sel = SELECT.get(select, select) if isinstance(select, (str, type(None))) else select
        if isinstance(sel, bool) or sel not in (0, 1, 2):
            raise ValueError(f"select must be one of 'clash', 'medoid' or None, got {select!r}")
        D = int(n_decoys)
        if not self.packed and self.B != 1:
            raise ValueError("ensemble_reduce needs a packed context (or a B = 1 one), not a padded B > 1 batch")
        check_groups(self.seg_offsets_host, D)
        if sel == 1 and per_res is None:
            raise ValueError("select='clash' needs per_res (Context.clash at these angles)")
        chi = self._chi(chi)
        pr = self._rows(per_res, "per_res") if per_res is not None else None
        n_cons, n_seg = self.n_rows // D, self.n_segments
        mean, resultant = self._new(1, n_cons, 4), self._new(1, n_cons, 4)
        dev = self._new(n_seg, dtype=torch.float64)
        clash = self._new(n_seg, dtype=torch.float64) if pr is not None else None
        best = self._new(n_seg // D, dtype=torch.int32)
        chi_best = self._new(1, n_cons, 4) if want_best else None
        _check(load().pp_ensemble_reduce(self.handle, _ptr(chi), D, _ptr(pr), int(sel), _ptr(mean), _ptr(resultant), _ptr(dev),
                                         _ptr(clash), _ptr(best), _ptr(chi_best), self._stream()), "pp_ensemble_reduce")
        return EnsembleResult(mean=mean, resultant=resultant, dev=dev, clash=clash, best=best, chi_best=chi_best)

    def ensemble_recombine(self, chi, n_decoys, start=None, max_sweeps=64, want_energy=False, vtf=12.0, tol=0.5):
        """Recombine the decoys of this context per residue by clash descent (pp_ensemble_recombine): every
        consensus row takes its four angles from one of the ``n_decoys`` decoys, chosen so that the clash loss of the recombined
        structure goes down monotonically from that of the ``start`` decoy.  The context is an ensemble context as for
        ``ensemble_reduce`` (checked against the host table before any launch).  ``chi`` [1, N, 4]; ``start`` int32 [n_groups] on
        the device (``best`` of ``ensemble_reduce``) or None = decoy 0; a group whose entry is outside 0 .. D - 1 is left alone.
        Returns an ``EnsembleResult``: ``pick`` int32 [N / D], ``chi`` [1, N / D, 4] (row r of decoy ``pick[r]``, bit for bit),
        ``clash_trace`` fp64 [n_groups, max_sweeps + 1] (the mean clash after k sweeps), ``sweeps``, ``converged`` int32 [n_groups],
        ``energy`` [N / D, D] (the local energies at the start; None without ``want_energy``), all on the device; no host
        synchronisation."""
        from .batch import check_groups
        D, K = int(n_decoys), int(max_sweeps)
        if K < 0:
            raise ValueError("max_sweeps must not be negative")
        if not self.packed and self.B != 1:
            raise ValueError("ensemble_recombine needs a packed context (or a B = 1 one), not a padded B > 1 batch")
        check_groups(self.seg_offsets_host, D)
        self.plan.set_clash_params(vtf, tol)
        chi = self._chi(chi)
        n_cons, n_grp = self.n_rows // D, self.n_segments // D
        st = None
        if start is not None:
            st = torch.as_tensor(start).to(device=self.plan.device, dtype=torch.int32).reshape(-1).contiguous()
            if st.numel() != n_grp:
                raise ValueError(f"start has {st.numel()} entries for {n_grp} groups")
        pick = self._new(n_cons, dtype=torch.int32)
        out = self._new(1, n_cons, 4)
        trace = self._new(n_grp, K + 1, dtype=torch.float64)
        sweeps, conv = self._new(n_grp, dtype=torch.int32), self._new(n_grp, dtype=torch.int32)
        energy = self._new(n_cons, D) if want_energy else None
        _check(load().pp_ensemble_recombine(self.handle, _ptr(chi), D, _ptr(st), K, _ptr(pick), _ptr(out), _ptr(trace), _ptr(sweeps),
                                            _ptr(conv), _ptr(energy), self._stream()), "pp_ensemble_recombine")
        return EnsembleResult(pick=pick, chi=out, clash_trace=trace, sweeps=sweeps, converged=conv, energy=energy)

    def shell(self, seeds, radius=10.0, mode="ca", other_chain=False, xyz=None, want_count=False):
        """The rows near the ``seeds`` rows, per complex, on the device (pp_ctx_shell): bool [B, L] (packed:
        [1, N]), with ``want_count`` also the shell rows per segment, int32 [n_segments].  ``seeds``: [B, L] bool / uint8 / int (any
        non-zero entry is a seed), on the host or the device.  ``mode`` "ca": CA-CA distance below ``radius``, the local mask of
        AffinityPrediction.get_local_subgraph; "atom": any pair of present atoms below it.  ``other_chain``: the seed must lie in
        another chain -- ``shell(all rows, mode="atom", other_chain=True)`` is the interface.  ``xyz`` [B, L, 14, 3]: coordinates
        other than the batch's X (``atom14`` of sampled angles).  A seed row is in its own shell; ``residue_mask`` is not consulted.
        ``~shell`` is the ``fixed`` mask of ``sample_partial`` / ``proximal_packed``.  No host synchronisation."""
        if mode not in SHELL_MODES:
            raise ValueError(f"mode must be one of {sorted(SHELL_MODES)}")
        sd = self._mask(seeds, "seeds")
        if xyz is not None:
            xyz = self._xyz(xyz)
        out = self._new(self.B, self.L, dtype=torch.uint8)
        count = self._new(self.n_segments, dtype=torch.int32) if want_count else None
        _check(load().pp_ctx_shell(self.handle, _ptr(sd), SHELL_MODES[mode], float(radius), SHELL_OTHER_CHAIN if other_chain else 0,
                                   _ptr(xyz), _ptr(out), _ptr(count), self._stream()), "pp_ctx_shell")
        return (out.bool(), count) if want_count else out.bool()

    def sasa(self, chi=None, xyz=None, n_points=96, probe=1.4, radius=None, want_counts=False):
        """Solvent-accessible surface per residue at four nested levels, on the device (pp_sasa).  Coordinates:
        ``atom14(chi)`` if ``chi`` is given, else ``xyz`` [B, L, 14, 3], else the batch's X.  ``radius`` [B, L, 14] (an atom is
        present iff its radius is > 0; default ``constants.slot_radius[residue_type] * (atom_mask != 0)``: the reference's element
        van der Waals radii, heavy atoms only); ``n_points`` test points per atom (``analysis.sphere_points``), ``probe`` in A.
        Returns an ``EnsembleResult``: ``area`` fp32 [B, L, 4] -- A^2 exposed next to the own residue alone (0), in the isolated
        chain (1), in the protein complex (2), with the context's obstacle atoms too (3) --, ``seg_area`` fp64 [n_segments, 4],
        ``counts`` int32 [B, L, 14, 4] (None without ``want_counts``) and, derived here: ``bsa`` = area[1] - area[2] (the surface
        a row buries in the interface), ``interface`` / ``pocket`` bool [B, L] (a test point of the row is buried by another
        chain / by an obstacle atom: integer tests on the counts; the reference's delta-ASA > 0 rule) and ``exposure`` =
        area[3] / area[0] (0 where area[0] is 0).  Areas are those of this radius set, not freesasa's.  No host synchronisation."""
        from .analysis import sphere_points
        dev = self.plan.device
        if self._t.get("chain_indices") is None:
            raise RuntimeError("sasa needs a batch with chain_indices")
        if chi is not None:
            xyz = self.atom14(chi)
        elif xyz is not None:
            xyz = self._xyz(xyz)
        if radius is None:
            if getattr(self, "_sasa_radius", None) is None:
                if self._t.get("atom_mask") is None:
                    raise RuntimeError("sasa needs a batch with atom_mask (or radius)")
                table = torch.from_numpy(np.asarray(rc.slot_radius, dtype=np.float32)).to(dev)
                self._sasa_radius = self._own((table[self._t["residue_type"]] * (self._t["atom_mask"] != 0)).contiguous())
            radius = self._sasa_radius
        else:
            radius = self._rows(torch.as_tensor(radius), "radius", 14)
        P = int(n_points)
        cache = self.__dict__.setdefault("_sasa_points", {})
        if P not in cache:
            cache[P] = self._own(torch.from_numpy(sphere_points(P)).to(dev) if 1 <= P <= 256 else torch.zeros(1, 3, device=dev))
        counts = self._new(self.B, self.L, 14, 4, dtype=torch.int32)
        area = self._new(self.B, self.L, 4)
        seg_area = self._new(self.n_segments, 4, dtype=torch.float64)
        _check(load().pp_sasa(self.handle, _ptr(xyz), _ptr(radius), _ptr(cache[P]), P, float(probe), _ptr(counts), _ptr(area),
                              _ptr(seg_area), self._stream()), "pp_sasa")
        per_row = counts.sum(2)
        a0 = area[..., 0]
        return EnsembleResult(area=area, seg_area=seg_area, counts=counts if want_counts else None, bsa=area[..., 1] - area[..., 2],
                              interface=per_row[..., 1] - per_row[..., 2] > 0, pocket=per_row[..., 2] - per_row[..., 3] > 0,
                              exposure=torch.where(a0 > 0, area[..., 3] / a0, torch.zeros_like(a0)))

    def disulfide_eligible(self):
        """bool [N] on the device: the rows ``disulfides`` can bond -- cysteines with residue_mask and the atom_mask of N, CA, C and
        SG set (the rule of csrc/pp_disulfide.hip, restated with torch)."""
        for k in ("atom_mask", "residue_mask"):
            if self._t.get(k) is None:
                raise RuntimeError(f"disulfides needs a batch with {k}")
        am = self._t["atom_mask"].reshape(-1, 14)
        return ((self._t["residue_type"].reshape(-1) == rc.restype_order["C"]) & (self._t["residue_mask"].reshape(-1) != 0)
                & (am[:, 0] != 0) & (am[:, 1] != 0) & (am[:, 2] != 0) & (am[:, 5] != 0))

    def check_disulfide_pairs(self, pairs, names=None):
        """Refuse a list of row pairs ``disulfides`` cannot take, naming the offender (``names``: row -> text, default the row
        number): a row outside the context, a row that is not an eligible cysteine, a pair across two segments, a row named twice.
        Reads the eligibility back.  Returns the pairs as [(a, b)] with a < b."""
        from bisect import bisect_right
        name = (lambda r: str(names[r])) if names is not None else (lambda r: f"row {r}")
        elig = self.disulfide_eligible().tolist()
        offs, seen, out = self.seg_offsets_host, {}, []
        for a, b in pairs:
            a, b = int(a), int(b)
            for r in (a, b):
                if not 0 <= r < self.n_rows:
                    raise ValueError(f"disulfides: row {r} is outside the {self.n_rows} rows of this context")
                if not elig[r]:
                    raise ValueError(f"disulfides: {name(r)} is not a cysteine with N, CA, C and SG present")
            if bisect_right(offs, a) != bisect_right(offs, b):
                raise ValueError(f"disulfides: {name(a)} and {name(b)} lie in two segments")
            for r in (a, b):
                if r in seen or a == b:
                    raise ValueError(f"disulfides: {name(r)} is named twice")
                seen[r] = True
            out.append((min(a, b), max(a, b)))
        return out

    def disulfides(self, chi=None, fixed=None, pairs=None, cb_max=5.0, max_energy=10.0, sigma_chi=np.deg2rad(20.0), names=None):
        """Detect the disulfide bridges of every segment from the backbone and close them (pp_disulfide_close, DESIGN.md section
        24).  ``chi`` [B, L, 4]: the angles to close from -- the result's ``chi`` equals them bit for bit except the chi1 of the
        bonded rows; None: detection only.  ``fixed`` [N] mask: rows whose chi1 must not change (needs ``chi``).  ``pairs``: a list
        of row pairs that replaces detection (no ``cb_max``, no ``max_energy``); it is checked first (``check_disulfide_pairs``).
        ``cb_max`` in A between ideal CB atoms, ``max_energy`` the largest grid minimum of the bridge energy that still is a bridge,
        ``sigma_chi`` (radians) what leaving the given chi1 by that much costs next to one unit of bridge energy.  Returns a
        ``DisulfideResult``; the call itself does not wait for the device (validating ``pairs`` does)."""
        dev = self.plan.device
        for k in ("atom_mask", "residue_mask"):
            if self._t.get(k) is None:
                raise RuntimeError(f"disulfides needs a batch with {k}")
        if fixed is not None and chi is None:
            raise ValueError("disulfides: fixed needs chi")
        chi_in = self._chi(chi) if chi is not None else None
        fx = self._mask(fixed, "fixed") if fixed is not None else None
        pr, n_pairs = None, 0
        if pairs is not None:
            rows = self.check_disulfide_pairs(pairs, names)
            n_pairs = len(rows)
            pr = torch.tensor(rows if rows else [[0, 0]], dtype=torch.int32).reshape(-1, 2).to(dev).contiguous()
        out = torch.empty_like(chi_in) if chi_in is not None else None
        partner = self._new(self.n_rows, dtype=torch.int32)
        report = self._new(self.n_rows, 4)
        count = self._new(self.n_segments, dtype=torch.int32)
        _check(load().pp_disulfide_close(self.handle, _ptr(chi_in), _ptr(fx), _ptr(pr), n_pairs, float(cb_max), float(max_energy),
                                         float(sigma_chi), _ptr(out), _ptr(partner), _ptr(report), _ptr(count), self._stream()),
               "pp_disulfide_close")
        return DisulfideResult(partner=partner, report=report, count=count, chi=out)

    def check_anchors(self, anchor_set, names=None):
        """Refuse an ``AnchorSet`` (``selection.AnchorSet``; rows are rows of this context) that ``anchors`` cannot take, naming the
        offender by the set's label (and ``names``: row -> text): an invalid entry -- a row outside the context or masked out, N, CA,
        C, the donor or its antecedent missing, a donor that is no side-chain atom moved by a chi angle, an antecedent equal to the
        donor, a value that is not finite or a ``sigma_d`` that is not positive --, a fifth anchor on a row, and an anchor on a row
        of another segment than the set claims (``anchor_set.segment``; None claims nothing).  The rules are those of
        csrc/pp_anchor.hip, restated on the host; reads the masks back."""
        from .selection import check_anchor_set
        for k in ("atom_mask", "residue_mask"):
            if self._t.get(k) is None:
                raise RuntimeError(f"anchors needs a batch with {k}")
        if len(anchor_set):
            check_anchor_set(anchor_set, self._t["residue_type"].reshape(-1).cpu().numpy(), self._t["residue_mask"].reshape(-1).cpu().numpy(),
                             self._t["atom_mask"].reshape(-1, 14).cpu().numpy(), self.seg_offsets_host, names)
        return anchor_set

    def anchors(self, chi, anchor_set, fixed=None, max_energy=10.0, sigma_chi=np.deg2rad(20.0), names=None, check=True):
        """Close the anchors of ``anchor_set`` (``selection.AnchorSet``, rows of this context; a list of sets is concatenated) next
        to the angles ``chi`` [B, L, 4] (pp_anchor_close): a distance restraint, optionally with an angle
        term, between a side-chain atom and a fixed point -- a metal ion, the atom of a covalently linked ligand.  The result's
        ``chi`` equals ``chi`` bit for bit except the first n chi of the closed rows; None: reports only (J = E).  ``fixed`` [N]
        mask: rows that keep their angles and are only reported (needs ``chi``).  ``max_energy``: the largest grid minimum that still
        closes; ``sigma_chi`` (radians): what leaving the given angles by that much costs next to one unit of anchor energy.  The
        set is checked first (``check_anchors``, which reads masks back; ``check=False`` leaves the entries to the device, which
        drops what it cannot take and sets status -2); the call itself does not wait for the device.  Returns an ``AnchorResult``."""
        from .selection import AnchorSet
        dev = self.plan.device
        if isinstance(anchor_set, (list, tuple)):
            anchor_set = AnchorSet.concat([self.check_anchors(a, names) if check else a for a in anchor_set if a is not None])
        if check:
            self.check_anchors(anchor_set, names)
        if fixed is not None and chi is None:
            raise ValueError("anchors: fixed needs chi")
        chi_in = self._chi(chi) if chi is not None else None
        fx = self._mask(fixed, "fixed") if fixed is not None else None
        return self._anchor_close(chi_in, fx, *anchor_set.device_arrays(dev), len(anchor_set), max_energy, sigma_chi)

    def _anchor_close(self, chi_in, fx, ai, at, ap, A, max_energy, sigma_chi, out=None):
        """pp_anchor_close on device arrays as they are (int32 [A, 4], fp32 [A, 4], fp32 [A, 4]): no check, no read-back.  ``out``:
        where chi_out goes (``chi_in`` itself: in place), default a new tensor."""
        if out is None:
            out = torch.empty_like(chi_in) if chi_in is not None else None
        status = self._new(self.n_rows, dtype=torch.int32)
        report = self._new(self.n_rows, 4)
        arep = self._new(max(A, 1), 2)
        count = self._new(self.n_segments, dtype=torch.int32)
        _check(load().pp_anchor_close(self.handle, _ptr(chi_in), _ptr(fx), _ptr(ai), _ptr(at), _ptr(ap), int(A), float(max_energy),
                                      float(sigma_chi), _ptr(out), _ptr(status), _ptr(report), _ptr(arep), _ptr(count),
                                      self._stream()), "pp_anchor_close")
        return AnchorResult(status=status, report=report, anchor_report=arep[:A], count=count, chi=out)

    def polar_tables(self):
        """(cls uint8 [N, 14], ante int8 [N, 14, 2]) on the device, what ``polar`` hands to pp_polar by default:
        ``constants.polar_class`` / ``polar_antecedent`` gathered by residue_type, with the class zeroed where atom_mask is 0 for the
        atom or for any of its antecedents.  Made once per context."""
        if getattr(self, "_polar_tabs", None) is None:
            dev = self.plan.device
            if self._t.get("atom_mask") is None:
                raise RuntimeError("polar needs a batch with atom_mask (or cls and ante)")
            rt = self._t["residue_type"].reshape(-1)
            am = self._t["atom_mask"].reshape(-1, 14) != 0
            cls = torch.from_numpy(np.asarray(rc.polar_class, dtype=np.uint8)).to(dev)[rt]
            ante = torch.from_numpy(np.asarray(rc.polar_antecedent, dtype=np.int8)).to(dev)[rt]
            ok = am
            for k in range(2):
                a = ante[..., k].long()
                ok = ok & ((a < 0) | torch.gather(am, 1, a.clamp(min=0)))
            self._polar_tabs = (self._own((cls * ok.to(torch.uint8)).contiguous()), self._own(ante.contiguous()))
        return self._polar_tabs

    def polar(self, chi=None, xyz=None, hb_max=3.5, sb_max=4.0, want_partners=True, sasa=None, bury_points=0, obst_polar=None,
              cls=None, ante=None):
        """Hydrogen bonds, salt bridges and polar obstacle contacts per segment, on the device (pp_polar).
        Coordinates as in ``sasa``: ``atom14(chi)`` if ``chi`` is given, else ``xyz`` [B, L, 14, 3], else the batch's X.  ``hb_max``
        and ``sb_max`` in A between heavy atoms.  ``obst_polar`` [M] (non-zero = polar), one entry per atom of the context's obstacle
        set; None: the batch's ``obstacle_polar`` (``protein_to_batch(..., obstacles=...)`` makes it from the elements
        ``pdb_io.obstacle_atoms`` returns: N and O; ``set_obstacles(polar=)``), or no polar obstacle atom if there is none.  ``cls`` [B, L,
        14] / ``ante`` [B, L, 14, 2]: class bits and antecedent slots other than ``polar_tables()``.  Returns an ``EnsembleResult``:
        ``n_partners`` int32 [B, L, 14, 2] (hydrogen-bond partners, polar obstacle atoms in reach), ``partners`` int32 [B, L, 14, 4]
        (the lowest partner codes (row - first row of the segment) * 14 + slot, ascending, then -1; None without
        ``want_partners``), ``res`` int32 [B, L, 8], ``seg`` int32 [n_segments, 8] (include/packppi_hip.h lists the columns), and,
        derived here with torch: ``polar`` bool [B, L, 14] (the class is not 0), ``unsat`` = polar without a partner of either
        kind, and with ``sasa`` (a ``sasa(..., want_counts=True)`` result at the same coordinates) ``buns`` = unsat and
        counts[..., 3] <= bury_points (buried with everything around it) and ``buns_interface`` = buns whose counts[..., 1] >
        bury_points (exposed in the isolated chain: buried by the partner).  No host synchronisation."""
        import math
        dev = self.plan.device
        if self._t.get("chain_indices") is None:
            raise RuntimeError("polar needs a batch with chain_indices")
        for name, v in (("hb_max", hb_max), ("sb_max", sb_max)):
            if not (math.isfinite(float(v)) and float(v) > 0):
                raise ValueError(f"polar: {name} must be finite and positive")
        if int(bury_points) < 0:
            raise ValueError("polar: bury_points must not be negative")
        if sasa is not None and _get(sasa, "counts") is None:
            raise ValueError("polar: sasa must be a Context.sasa(..., want_counts=True) result")
        if (cls is None) != (ante is None):
            raise ValueError("polar: cls and ante go together")
        if cls is None:
            cls, ante = self.polar_tables()
        else:
            cls = torch.as_tensor(cls).to(device=dev, dtype=torch.uint8).contiguous()
            ante = torch.as_tensor(ante).to(device=dev, dtype=torch.int8).contiguous()
            if cls.numel() != self.n_rows * 14 or ante.numel() != self.n_rows * 28:
                raise ValueError(f"polar: cls / ante have {cls.numel()} / {ante.numel()} elements, this context has {self.n_rows} rows")
        op = getattr(self, "_obst_polar", None) if self.n_obstacles else None
        if obst_polar is not None:
            if self.n_obstacles == 0:
                raise ValueError("polar: obst_polar on a context without obstacle atoms")
            op = (torch.as_tensor(obst_polar).to(device=dev) != 0).to(torch.uint8).reshape(-1).contiguous()
            if op.numel() != self.n_obstacles:
                raise ValueError(f"polar: obst_polar has {op.numel()} entries, the context holds {self.n_obstacles} obstacle atoms")
        if chi is not None:
            xyz = self.atom14(chi)
        elif xyz is not None:
            xyz = self._xyz(xyz)
        partners = self._new(self.B, self.L, 14, 4, dtype=torch.int32) if want_partners else None
        n_partners = self._new(self.B, self.L, 14, 2, dtype=torch.int32)
        res = self._new(self.B, self.L, 8, dtype=torch.int32)
        seg = self._new(self.n_segments, 8, dtype=torch.int32)
        _check(load().pp_polar(self.handle, _ptr(xyz), _ptr(cls), _ptr(ante), _ptr(op), float(hb_max), float(sb_max), _ptr(partners),
                               _ptr(n_partners), _ptr(res), _ptr(seg), self._stream()), "pp_polar")
        polar = cls.reshape(self.B, self.L, 14) != 0
        unsat = polar & (n_partners.sum(-1) == 0)
        out = EnsembleResult(n_partners=n_partners, partners=partners, res=res, seg=seg, polar=polar, unsat=unsat, buns=None,
                             buns_interface=None)
        if sasa is not None:
            counts = _get(sasa, "counts").reshape(self.B, self.L, 14, 4)
            out["buns"] = unsat & (counts[..., 3] <= int(bury_points))
            out["buns_interface"] = out["buns"] & (counts[..., 1] > int(bury_points))
        return out

    def _link(self, link):
        """A ``link`` argument (the ``partner`` of ``disulfides``, a ``DisulfideResult``, or None) as int32 [N] on the device."""
        if link is None:
            return None
        if isinstance(link, dict):
            link = link["partner"]
        link = torch.as_tensor(link).to(device=self.plan.device, dtype=torch.int32).reshape(-1).contiguous()
        if link.numel() != self.n_rows:
            raise ValueError(f"link has {link.numel()} entries, this context has {self.n_rows} rows")
        return link

    def allatom_tables(self):
        """The tables of ``hydrogens`` / ``clashscore`` on the device, made once per context from ``constants``: ``place`` int8
        [21, 13, 5], ``param`` fp32 [21, 13, 5], ``aa_sep`` uint8 [21, 27, 27], and gathered by residue_type ``radius`` fp32 [N, 27]
        (the default radii, 0 for the heavy atoms whose atom_mask is 0), ``acls`` uint8 [N, 27] and ``rotatable`` bool [N, 27]."""
        if getattr(self, "_aa_tabs", None) is None:
            dev = self.plan.device
            if self._t.get("atom_mask") is None:
                raise RuntimeError("hydrogens / clashscore need a batch with atom_mask")
            rt = self._t["residue_type"].reshape(-1)
            up = lambda a, dt: self._own(torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev))
            present = torch.cat([self._t["atom_mask"].reshape(-1, 14) != 0,
                                 torch.ones(self.n_rows, rc.PP_H_MAX, dtype=torch.bool, device=dev)], 1)
            radius = torch.from_numpy(rc.allatom_default_radius).to(dev)[rt] * present
            rot = np.zeros((21, rc.PP_AA_SLOTS), bool)
            rot[:, 14:] = (rc.hydrogen_flags & rc.H_ROTATABLE) != 0
            self._aa_tabs = EnsembleResult(
                place=up(rc.hydrogen_place, np.int8), param=up(rc.hydrogen_param, np.float32), aa_sep=up(rc.aa_sep, np.uint8),
                radius=self._own(radius.contiguous()), acls=self._own(torch.from_numpy(rc.allatom_class).to(dev)[rt].contiguous()),
                rotatable=self._own(torch.from_numpy(rot).to(dev)[rt].contiguous()))
        return self._aa_tabs

    def hydrogens(self, chi=None, xyz=None, link=None, place=None, param=None):
        """Place the hydrogens of every row on the device (pp_hydrogens).  Coordinates as in ``sasa``:
        ``atom14(chi)`` if ``chi`` is given, else ``xyz`` [B, L, 14, 3], else the batch's X.  ``link`` int32 [N]: the ``partner`` of
        ``disulfides`` (or its result) -- a bonded cysteine has no HG.  ``place`` / ``param``: tables other than ``constants``'.
        Returns an ``EnsembleResult``: ``hxyz`` fp32 [B, L, 13, 3] (0 where there is none), ``hmask`` uint8 [B, L, 13], ``link_prev``
        uint8 [B, L] (the row is peptide-bonded to the row before it) and ``xyz`` (the heavy atoms used).  The k-th hydrogen of a row
        is ``constants.hydrogen_names[type][k]``.  Rotatable hydrogens (OH, SH, NH3+) sit at a conventional position (``hbond_optimize`` chooses them), not an
        optimised one.  No host synchronisation."""
        dev = self.plan.device
        for k in ("chain_indices", "atom_mask"):
            if self._t.get(k) is None:
                raise RuntimeError(f"hydrogens needs a batch with {k}")
        if (place is None) != (param is None):
            raise ValueError("hydrogens: place and param go together")
        if place is None:
            tabs = self.allatom_tables()
            place, param = tabs.place, tabs.param
        else:
            place = torch.as_tensor(place).to(device=dev, dtype=torch.int8).contiguous()
            param = torch.as_tensor(param).to(device=dev, dtype=torch.float32).contiguous()
            if place.numel() != 21 * 13 * 5 or param.numel() != 21 * 13 * 5:
                raise ValueError("hydrogens: place and param are [21, 13, 5] tables")
        link = self._link(link)
        if chi is not None:
            xyz = self.atom14(chi)
        elif xyz is not None:
            xyz = self._xyz(xyz)
        hxyz = self._new(self.B, self.L, rc.PP_H_MAX, 3)
        hmask = self._new(self.B, self.L, rc.PP_H_MAX, dtype=torch.uint8)
        link_prev = self._new(self.B, self.L, dtype=torch.uint8)
        _check(load().pp_hydrogens(self.handle, _ptr(xyz), _ptr(place), _ptr(param), _ptr(link), _ptr(hxyz), _ptr(hmask),
                                   _ptr(link_prev), self._stream()), "pp_hydrogens")
        return EnsembleResult(hxyz=hxyz, hmask=hmask, link_prev=link_prev, xyz=xyz if xyz is not None else self._t.get("X"))

    def clashscore(self, chi=None, xyz=None, link=None, rotatable="skip", cut=0.4, hb_allow=0.6, radius=None, want_partners=True,
                   obst_polar=None, hydrogens=None):
        """All-atom clashscore per segment on the device (pp_hydrogens + pp_clashscore): serious overlaps
        (more than ``cut`` A of van der Waals overlap, ``hb_allow`` A more between a polar hydrogen and an acceptor) between all atoms,
        placed hydrogens included, per 1000 atoms.  NOT MolProbity's number: no Reduce flips, no optimisation of rotatable
        hydrogens, and the radii are ``constants.allatom_radius``.  Coordinates and ``link`` as in ``hydrogens`` (``hydrogens``: a
        result of it at the same coordinates, else it is called here).  ``rotatable`` "skip" (default): hydroxyl, thiol and lysine
        NH3+ hydrogens are not counted (radius 0); "keep": they are.  ``radius`` [B, L, 27]: radii other than the default (an atom is
        counted iff its radius is > 0).  ``obst_polar`` as in ``polar``.  Returns an ``EnsembleResult``: ``n_clash`` int32 [B, L, 27,
        2], ``partners`` int32 [B, L, 27, 4] (None without ``want_partners``), ``res`` int32 [B, L, 4], ``seg`` int32 [n_segments, 8]
        (include/packppi_hip.h lists the columns), ``clashscore`` = 1000 seg[:, 1] / max(seg[:, 0], 1) and ``clashscore_obstacles``
        (with seg[:, 6] added) fp64 [n_segments], and ``hxyz`` / ``hmask`` / ``link_prev`` / ``xyz``.  No host synchronisation."""
        import math
        dev = self.plan.device
        if rotatable not in ("skip", "keep"):
            raise ValueError('clashscore: rotatable must be "skip" or "keep"')
        if not math.isfinite(float(cut)):
            raise ValueError("clashscore: cut must be finite")
        if not (math.isfinite(float(hb_allow)) and float(hb_allow) >= 0):
            raise ValueError("clashscore: hb_allow must be finite and not negative")
        tabs = self.allatom_tables()
        if radius is None:
            cache = self.__dict__.setdefault("_aa_radius", {})
            if rotatable not in cache:
                cache[rotatable] = tabs.radius if rotatable == "keep" else self._own((tabs.radius * ~tabs.rotatable).contiguous())
            radius = cache[rotatable]
        else:
            radius = self._rows(torch.as_tensor(radius), "radius", rc.PP_AA_SLOTS)
            if rotatable == "skip":
                radius = (radius.reshape(-1, rc.PP_AA_SLOTS) * ~tabs.rotatable).contiguous()
        op = getattr(self, "_obst_polar", None) if self.n_obstacles else None
        if obst_polar is not None:
            if self.n_obstacles == 0:
                raise ValueError("clashscore: obst_polar on a context without obstacle atoms")
            op = (torch.as_tensor(obst_polar).to(device=dev) != 0).to(torch.uint8).reshape(-1).contiguous()
            if op.numel() != self.n_obstacles:
                raise ValueError(f"clashscore: obst_polar has {op.numel()} entries, the context holds {self.n_obstacles} obstacle atoms")
        link = self._link(link)
        h = hydrogens if hydrogens is not None else self.hydrogens(chi=chi, xyz=xyz, link=link)
        xyz = h["xyz"]
        S = rc.PP_AA_SLOTS
        partners = self._new(self.B, self.L, S, 4, dtype=torch.int32) if want_partners else None
        n_clash = self._new(self.B, self.L, S, 2, dtype=torch.int32)
        res = self._new(self.B, self.L, 4, dtype=torch.int32)
        seg = self._new(self.n_segments, 8, dtype=torch.int32)
        _check(load().pp_clashscore(self.handle, _ptr(xyz), _ptr(h["hxyz"]), _ptr(h["hmask"]), _ptr(radius), _ptr(tabs.acls),
                                    _ptr(tabs.aa_sep), _ptr(h["link_prev"]), _ptr(link), _ptr(op), float(cut), float(hb_allow),
                                    _ptr(partners), _ptr(n_clash), _ptr(res), _ptr(seg), self._stream()), "pp_clashscore")
        atoms = seg[:, 0].clamp(min=1).double()
        return EnsembleResult(n_clash=n_clash, partners=partners, res=res, seg=seg, clashscore=1000.0 * seg[:, 1].double() / atoms,
                              clashscore_obstacles=1000.0 * (seg[:, 1] + seg[:, 6]).double() / atoms, hxyz=h["hxyz"], hmask=h["hmask"],
                              link_prev=h["link_prev"], xyz=xyz, radius=radius)

    def hnet_tables(self):
        """The mover tables of ``hbond_optimize`` on the device, made once per context from ``constants``: ``mover`` int32 [21, 4],
        ``rot`` fp32 [21, 12, 3, 2], ``ext`` fp32 [21], ``flip_chi`` int64 [N] (the index of the chi a flip row turns, -1 on
        every other row) and ``seg_of_row`` int64 [N]."""
        if getattr(self, "_hn_tabs", None) is None:
            dev = self.plan.device
            up = lambda a, dt: self._own(torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev))
            fc = -np.ones(21, np.int64)
            for rn, k in rc.mover_flip_chi.items():
                fc[rc.resname_to_idx[rn]] = k
            rt = self._t["residue_type"].reshape(-1)
            self._hn_tabs = EnsembleResult(mover=up(rc.mover_table, np.int32), rot=up(rc.mover_rotor_cs, np.float32),
                                           ext=up(rc.mover_extent, np.float32),
                                           seg_of_row=up(np.repeat(np.arange(self.n_segments), np.diff(self.seg_offsets_host)), np.int64),
                                           flip_chi=self._own(torch.from_numpy(fc).to(dev)[rt.clamp(0, 20)].contiguous()))
        return self._hn_tabs

    def hbond_optimize(self, chi=None, xyz=None, link=None, max_sweeps=32, hb_weak=2.5, hb_good=2.2, cut=0.4, hb_allow=0.6, radius=None,
                       obst_polar=None, want_candidates=False, mover=None):
        """Optimise the hydrogen-bond network of every segment on the device (pp_hnet_optimize): Asn / Gln / His
        flips and the rotatable hydrogens (Ser / Thr / Tyr OH, Cys SH, Lys NH3+), by a monotone descent on an integer energy -- 64 per
        serious overlap of ``clashscore`` minus 2 per good and 1 per weak explicit-hydrogen bond (H ... acceptor within ``hb_good`` A
        at an angle of at least 120 degrees / within ``hb_weak`` A at 90).  Integer counts, not Reduce's dot scores, no exhaustive
        clique search, this package's radii.  Coordinates and ``link`` as in ``hydrogens``; flips need ``chi`` (they are chi + pi),
        with ``xyz`` or the batch's X only rotors are optimised.  ``radius`` [B, L, 27] as in ``clashscore`` (rotatable hydrogens are
        always kept; radii of the caller's cost one read-back); ``mover``: a table other than ``constants.mover_table``.  Returns
        an ``EnsembleResult``: ``state`` int32 [B, L] (-1: no mover), ``xyz`` [B, L, 14, 3], ``hxyz`` / ``hmask`` / ``link_prev`` (what ``clashscore(hydrogens=...)`` takes),
        ``chi`` [B, L, 4] (None without ``chi``), ``e`` int32 [B, L, 2] (the row's energy at the start and at the end), ``hb`` int32
        [B, L, 2] (its explicit-hydrogen bonds, each bond in one row), ``n_bonds`` / ``n_flips`` int64 [n_segments], ``trace`` int32
        [n_segments, max_sweeps + 1] (the total energy after each sweep), ``sweeps`` / ``converged`` int32 [n_segments], ``n_movers``
        int64 [n_segments], and with ``want_candidates`` ``cand`` fp32 [B, L, 12, 3, 3] and ``energy`` int32 [B, L, 12].  No host
        synchronisation."""
        import math
        dev = self.plan.device
        for name, v in (("cut", cut), ("hb_allow", hb_allow), ("hb_weak", hb_weak), ("hb_good", hb_good)):
            if not math.isfinite(float(v)):
                raise ValueError(f"hbond_optimize: {name} must be finite")
        if float(hb_allow) < 0 or not (0 < float(hb_good) <= float(hb_weak)):
            raise ValueError("hbond_optimize: hb_allow must not be negative, and 0 < hb_good <= hb_weak")
        if not (0 <= int(max_sweeps) <= 256):
            raise ValueError("hbond_optimize: max_sweeps must lie in 0 .. 256")
        tabs, ht = self.allatom_tables(), self.hnet_tables()
        if radius is None:
            radius, r_max = tabs.radius, float(rc.allatom_default_radius.max())
        else:
            radius = self._rows(torch.as_tensor(radius), "radius", rc.PP_AA_SLOTS)
            r_max = float(radius.max())                    # the one read-back, only with radii of the caller's
        op = getattr(self, "_obst_polar", None) if self.n_obstacles else None
        if obst_polar is not None:
            if self.n_obstacles == 0:
                raise ValueError("hbond_optimize: obst_polar on a context without obstacle atoms")
            op = (torch.as_tensor(obst_polar).to(device=dev) != 0).to(torch.uint8).reshape(-1).contiguous()
            if op.numel() != self.n_obstacles:
                raise ValueError(f"hbond_optimize: obst_polar has {op.numel()} entries, the context holds {self.n_obstacles} obstacle atoms")
        mv = ht.mover
        if mover is not None:
            mv = torch.as_tensor(mover).to(device=dev, dtype=torch.int32).contiguous()
            if mv.numel() != 21 * 4:
                raise ValueError("hbond_optimize: mover is a [21, 4] table")
        link = self._link(link)
        chi0 = chi1 = chi_out = h1 = None
        if chi is not None:
            chi0 = self._chi(chi)
            fc = ht.flip_chi.reshape(self.B, self.L)
            turn = torch.nn.functional.one_hot(fc.clamp(min=0), 4).bool() & (fc >= 0)[..., None]
            flipped = torch.remainder(chi0 + 2.0 * math.pi, 2.0 * math.pi) - math.pi          # chi + pi wrapped into [-pi, pi)
            chi1 = torch.where(turn, flipped, chi0).contiguous()
            h0 = self.hydrogens(chi=chi0, link=link)
            h1 = self.hydrogens(chi=chi1, link=link)
            chi_out = self._new(self.B, self.L, 4)
        else:
            h0 = self.hydrogens(xyz=xyz, link=link)
        f32 = np.float32
        reach = max(f32(f32(2.0) * f32(r_max) - f32(cut)), f32(hb_weak))
        S = rc.PP_AA_SLOTS
        state = self._new(self.B, self.L, dtype=torch.int32)
        xyz_out = self._new(self.B, self.L, 14, 3)
        hxyz_out = self._new(self.B, self.L, rc.PP_H_MAX, 3)
        hmask_out = self._new(self.B, self.L, rc.PP_H_MAX, dtype=torch.uint8)
        e = self._new(self.B, self.L, 2, dtype=torch.int32)
        hb = self._new(self.B, self.L, 2, dtype=torch.int32)
        trace = self._new(self.n_segments, int(max_sweeps) + 1, dtype=torch.int32)
        sweeps = self._new(self.n_segments, dtype=torch.int32)
        converged = self._new(self.n_segments, dtype=torch.int32)
        cand = self._new(self.B, self.L, 12, 3, 3) if want_candidates else None
        energy = self._new(self.B, self.L, 12, dtype=torch.int32) if want_candidates else None
        g = lambda h, k: _ptr(h[k]) if h is not None else None
        _check(load().pp_hnet_optimize(
            self.handle, _ptr(h0["xyz"]), _ptr(h0["hxyz"]), _ptr(h0["hmask"]), g(h1, "xyz"), g(h1, "hxyz"), g(h1, "hmask"), _ptr(chi0),
            _ptr(chi1), _ptr(tabs.place), _ptr(tabs.param), _ptr(mv), _ptr(ht.rot), _ptr(ht.ext), _ptr(radius), _ptr(tabs.acls),
            _ptr(tabs.aa_sep), _ptr(h0["link_prev"]), _ptr(link), _ptr(op), float(cut), float(hb_allow), float(hb_weak),
            float(f32(hb_weak) * f32(hb_weak)), float(f32(hb_good) * f32(hb_good)), float(reach), int(max_sweeps), _ptr(state),
            _ptr(xyz_out), _ptr(hxyz_out), _ptr(hmask_out), _ptr(chi_out), _ptr(e), _ptr(hb), _ptr(trace), _ptr(sweeps), _ptr(converged),
            _ptr(cand), _ptr(energy), self._stream()), "pp_hnet_optimize")
        per_seg = lambda rows: torch.zeros(self.n_segments, dtype=torch.int64, device=dev).index_add_(0, ht.seg_of_row, rows.to(torch.int64))
        n_movers = per_seg(state.reshape(-1) >= 0)
        flip_row = (ht.flip_chi >= 0) & (state.reshape(-1) == 1)
        return EnsembleResult(state=state, xyz=xyz_out, hxyz=hxyz_out, hmask=hmask_out, link_prev=h0["link_prev"], chi=chi_out, e=e, hb=hb,
                              n_bonds=per_seg(hb.reshape(-1, 2)[:, 1]), n_flips=per_seg(flip_row), trace=trace, sweeps=sweeps,
                              converged=converged, n_movers=n_movers, cand=cand, energy=energy, radius=radius,
                              # the inputs of the call, for whoever holds the result against them
                              xyz0=h0["xyz"], hxyz0=h0["hxyz"], hmask0=h0["hmask"], xyz1=h1["xyz"] if h1 is not None else None,
                              hxyz1=h1["hxyz"] if h1 is not None else None, hmask1=h1["hmask"] if h1 is not None else None,
                              chi0=chi0, chi1=chi1)

    def refine_allatom(self, chi, fixed=None, link=None, deltas_deg=(16, 8, 4), max_steps=3, max_sweeps=32, bands=4, band=0.15, cut=0.4,
                       hb_allow=0.6, hb_weak=2.5, hb_good=2.2, radius=None, obst_polar=None, want_candidates=False):
        """Refine the side chains of every segment in chi space against the explicit-hydrogen overlaps ``clashscore`` counts, on the
        device (pp_chi_refine): a monotone descent on an integer energy -- 64 per level of overlap (level 1 is
        a serious overlap of ``clashscore``, every further ``band`` A of depth one more, up to ``bands``) minus ``hbond_optimize``'s 2
        / 1 per good / weak explicit-hydrogen bond --, by single steps of +-delta on one chi, at most ``max_steps`` steps from the
        start on each chi.  A residue without a serious overlap is never moved and keeps its angles bit for bit.  One device call
        per entry of ``deltas_deg`` (degrees), each starting from the angles of the one before; no angle is read back.  The
        defaults are starting values, not tuned against anything.  ``fixed`` [B, L]: rows that stay; the bridged cysteines of
        ``link`` (as in ``hydrogens``) stay too.  Rotatable hydrogens are not counted (``clashscore``'s ``rotatable="skip"``);
        ``radius`` [B, L, 27] other radii (one read-back), ``obst_polar`` as in ``clashscore``.  Returns an ``EnsembleResult`` that
        ``clashscore(hydrogens=res)`` and ``clashscore(chi=res.chi)`` / ``hbond_optimize(chi=res.chi)`` take: ``chi`` [B, L, 4],
        ``xyz`` / ``hxyz`` / ``hmask`` / ``link_prev`` at ``chi``, ``moved`` bool [B, L], ``rotation`` [B, L, 4] (radians, the sum of
        the steps taken), ``e`` int32 [B, L, 2] (the row's energy at the very start and end), ``F`` int64 [n_segments, 2], and per
        round (leading dimension ``len(deltas_deg)``) ``steps`` int8 [R, B, L, 4], ``trace`` int32 [R, n_segments, max_sweeps + 1],
        ``sweeps`` / ``converged`` int32 [R, n_segments], ``e_round`` int32 [R, B, L, 2]; with ``want_candidates`` also ``cand_xyz``
        [R, 9, B, L, 14, 3], ``cand_hxyz`` [R, 9, B, L, 13, 3], ``cand_hmask`` [R, 9, B, L, 13], ``cand_mask`` int32 [R, B, L],
        ``cand_chi`` [R, B, L, 4] (the angles each round started from) and ``energy`` int32 [R, B, L, 9]."""
        import math
        dev = self.plan.device
        for name, v in (("cut", cut), ("hb_allow", hb_allow), ("hb_weak", hb_weak), ("hb_good", hb_good), ("band", band)):
            if not math.isfinite(float(v)):
                raise ValueError(f"refine_allatom: {name} must be finite")
        if float(hb_allow) < 0 or not (0 < float(hb_good) <= float(hb_weak)):
            raise ValueError("refine_allatom: hb_allow must not be negative, and 0 < hb_good <= hb_weak")
        if not (0 <= int(max_sweeps) <= 256):
            raise ValueError("refine_allatom: max_sweeps must lie in 0 .. 256")
        if not (1 <= int(bands) <= 8) or not float(band) > 0:
            raise ValueError("refine_allatom: bands must lie in 1 .. 8 and band must be positive")
        deltas = [float(np.float32(np.deg2rad(float(d)))) for d in deltas_deg]
        if not deltas or not (1 <= int(max_steps) <= 16) or any(not (math.isfinite(d) and d > 0 and int(max_steps) * d < 3.1415) for d in deltas):
            raise ValueError("refine_allatom: deltas_deg must be positive, max_steps in 1 .. 16 and max_steps * delta below 180 degrees")
        for k in ("X", "BB_D", "chain_indices", "atom_mask", "residue_mask", "SC_D_mask"):
            if self._t.get(k) is None:
                raise RuntimeError(f"refine_allatom needs a batch with {k}")
        tabs = self.allatom_tables()
        if getattr(self, "_rf_ext", None) is None:
            self._rf_ext = self._own(torch.from_numpy(np.ascontiguousarray(rc.refine_extent, dtype=np.float32)).to(dev))
        if radius is None:
            cache = self.__dict__.setdefault("_aa_radius", {})
            if "skip" not in cache:
                cache["skip"] = self._own((tabs.radius * ~tabs.rotatable).contiguous())
            radius, r_max = cache["skip"], float(rc.allatom_default_radius.max())
        else:
            radius = self._rows(torch.as_tensor(radius), "radius", rc.PP_AA_SLOTS)
            radius = (radius.reshape(-1, rc.PP_AA_SLOTS) * ~tabs.rotatable).contiguous()
            r_max = float(radius.max())                    # the one read-back, only with radii of the caller's
        op = getattr(self, "_obst_polar", None) if self.n_obstacles else None
        if obst_polar is not None:
            if self.n_obstacles == 0:
                raise ValueError("refine_allatom: obst_polar on a context without obstacle atoms")
            op = (torch.as_tensor(obst_polar).to(device=dev) != 0).to(torch.uint8).reshape(-1).contiguous()
            if op.numel() != self.n_obstacles:
                raise ValueError(f"refine_allatom: obst_polar has {op.numel()} entries, the context holds {self.n_obstacles} obstacle atoms")
        link = self._link(link)
        fx = self._mask(fixed, "fixed") if fixed is not None else None
        if link is not None:
            bridged = (link >= 0).to(torch.uint8)
            fx = bridged if fx is None else (fx | bridged)
        f32 = np.float32
        reach = max(f32(f32(2.0) * f32(r_max) - f32(cut)), f32(hb_weak))
        R, nseg, ms = len(deltas), self.n_segments, int(max_sweeps)
        cur = self._chi(chi)
        chi_in = cur
        steps = self._new(R, self.B, self.L, 4, dtype=torch.int8)
        e_round = self._new(R, self.B, self.L, 2, dtype=torch.int32)
        trace = self._new(R, nseg, ms + 1, dtype=torch.int32)
        sweeps, converged = self._new(R, nseg, dtype=torch.int32), self._new(R, nseg, dtype=torch.int32)
        xyz, hxyz = self._new(self.B, self.L, 14, 3), self._new(self.B, self.L, rc.PP_H_MAX, 3)
        hmask = self._new(self.B, self.L, rc.PP_H_MAX, dtype=torch.uint8)
        link_prev = self._new(self.B, self.L, dtype=torch.uint8)
        cx = ch = cm = ck = en = cc = None
        if want_candidates:
            cx, ch = self._new(R, 9, self.B, self.L, 14, 3), self._new(R, 9, self.B, self.L, rc.PP_H_MAX, 3)
            cm = self._new(R, 9, self.B, self.L, rc.PP_H_MAX, dtype=torch.uint8)
            ck, en = self._new(R, self.B, self.L, dtype=torch.int32), self._new(R, self.B, self.L, 9, dtype=torch.int32)
            cc = self._new(R, self.B, self.L, 4)
        at = lambda t, r: _ptr(t[r]) if t is not None else None
        for r, delta in enumerate(deltas):
            out = self._new(self.B, self.L, 4)
            if cc is not None:
                cc[r].copy_(cur)
            _check(load().pp_chi_refine(
                self.handle, _ptr(cur), _ptr(fx), _ptr(tabs.place), _ptr(tabs.param), _ptr(self._rf_ext), _ptr(radius), _ptr(tabs.acls),
                _ptr(tabs.aa_sep), _ptr(link), _ptr(op), delta, int(max_steps), int(bands), float(band), float(cut), float(hb_allow),
                float(hb_weak), float(f32(hb_weak) * f32(hb_weak)), float(f32(hb_good) * f32(hb_good)), float(reach), ms, _ptr(out),
                _ptr(steps[r]), _ptr(xyz), _ptr(hxyz), _ptr(hmask), _ptr(link_prev), _ptr(e_round[r]), _ptr(trace[r]), _ptr(sweeps[r]),
                _ptr(converged[r]), at(cx, r), at(ch, r), at(cm, r), at(ck, r), at(en, r), self._stream()), "pp_chi_refine")
            cur = out
        rotation = sum(steps[r].float() * deltas[r] for r in range(R))          # python scalars: no host table to copy
        return EnsembleResult(chi=cur, chi0=chi_in, xyz=xyz, hxyz=hxyz, hmask=hmask, link_prev=link_prev, steps=steps,
                              moved=(steps != 0).any(-1).any(0), rotation=rotation, e=torch.stack([e_round[0, ..., 0], e_round[-1, ..., 1]], -1),
                              e_round=e_round, F=torch.stack([trace[0, :, 0], trace[-1, :, -1]], -1).to(torch.int64), trace=trace,
                              sweeps=sweeps, converged=converged, deltas=deltas, radius=radius, fixed=fx, cand_xyz=cx, cand_hxyz=ch,
                              cand_hmask=cm, cand_mask=ck, cand_chi=cc, energy=en)

    def saturated(self) -> int:
        """Sticky flag word of this context: 0 = clean; bit 0 / bit 1 = a hidden activation was clamped at 65504 in an edge-level /
        node-level kernel; bit 2 (value 4) = a NaN or infinity entered with the caller's tensors (the reference would return NaN, the
        kernels' clamps return finite numbers that mean nothing).  Waits for the stream."""
        v = C.c_int(0)
        _check(load().pp_ctx_saturated(self.handle, C.byref(v), self._stream()), "pp_ctx_saturated")
        return int(v.value)

    def live_rows(self):
        """The rows a sampling run can move (residue_mask != 0 and a non-zero SC_D_mask entry), ascending: int32 [count] on the
        device.  The layer-1 edge update of ``sample`` runs on these rows only (pp_ctx_live_rows).  Waits for the stream."""
        rows, n = self._new(self.n_rows, dtype=torch.int32), C.c_int(0)
        _check(load().pp_ctx_live_rows(self.handle, _ptr(rows), C.byref(n), self._stream()), "pp_ctx_live_rows")
        return rows[:int(n.value)]

    def live_mix(self):
        """The work table of the context's mixed live-row launch (pp_ctx_live_mix): ``(table, workgroups)`` -- int32 [N, 2] on the
        HOST, entry b the one or two rows of workgroup b ((r, -1): one row, (-1, -1): none), and the size of that launch; ``(None, 0)``
        for a context whose size does not take the mixed launch.  A read-back for tests and tools: waits for the whole device."""
        mix, n = torch.empty(self.n_rows, 2, dtype=torch.int32), C.c_int(0)
        _check(load().pp_ctx_live_mix(self.handle, _ptr(mix), C.byref(n)), "pp_ctx_live_mix")
        return (mix, int(n.value)) if n.value else (None, 0)

    def time_kernel(self, which: int, iters: int = 20) -> float:
        """Average ms per launch of the node-message (0) / edge-update (1) kernel, HIP events on the current stream."""
        ms = C.c_float(0.0)
        _check(load().pp_time_kernel(self.handle, int(which), int(iters), C.byref(ms), self._stream()),
               "pp_time_kernel")
        return float(ms.value)

    def profile_kernel(self, which: int):
        """Bracket every later launch of kernel `which` (0 node message, 1 edge update, 2 node update; inside the proximal
        calls: 3 the one launch per Adam step; inside sample_guided(): 4 the reconstruction of a nudge, 5 its clash + gradient +
        step launch, 6 the node embedding launch behind it; inside sample_corrected(): 7 the corrector launch) with HIP events."""
        _check(load().pp_profile_kernel(self.handle, int(which)), "pp_profile_kernel")

    def profile_read(self):
        """(average ms per launch, launches) since profile_kernel(); switches profiling off."""
        ms, n = C.c_float(0.0), C.c_int(0)
        _check(load().pp_profile_read(self.handle, C.byref(ms), C.byref(n)), "pp_profile_read")
        return (float(ms.value) / max(n.value, 1), int(n.value))

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and _lib is not None:
            _lib.pp_ctx_destroy(h)
            self.handle = None


SO2_GRID = 5001
_so2_grids_on = set()


def so2_grids():
    """(x [2, 5001], sigma [2, 5001]) fp64: the grids of SO2Schedule.__init__ (schedule.py:40-43) for PI = pi / 2, then PI = pi,
    computed with NumPy by the reference's own expressions."""
    X_MIN, X_N, SIGMA_MIN, SIGMA_MAX, SIGMA_N = 1e-5, 5000, 3e-3, 2, 5000
    xs, ss = [], []
    for PI in (1 / 2 * np.pi, np.pi):
        xs.append(10 ** np.linspace(np.log10(X_MIN), 0, X_N + 1) * PI)
        ss.append(10 ** np.linspace(np.log10(SIGMA_MIN), np.log10(SIGMA_MAX), SIGMA_N + 1) * PI)
    return np.ascontiguousarray(np.stack(xs)), np.ascontiguousarray(np.stack(ss))


def so2_score(x, sigma, pi_periodic: bool, want_idx: bool = False):
    """SO2Schedule.score(x, sigma) of the schedule with PI = pi / 2 (``pi_periodic``) or pi, computed on the device without the
    reference's tables (pp_so2_score).  ``sigma`` broadcasts to ``x``.  -> fp32 score shaped like ``x`` (and the int32
    [..., 2] (sigma index, x index) pairs)."""
    if x.device.type != "cuda":
        raise RuntimeError(f"so2_score needs tensors on the HIP device, got {x.device}")
    lib, dev = load(), x.device
    idx_dev = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx_dev not in _so2_grids_on:
        xg, sg = so2_grids()
        _check(lib.pp_so2_set_grids(xg.ctypes.data, sg.ctypes.data, idx_dev), "pp_so2_set_grids")
        _so2_grids_on.add(idx_dev)
    xf = x.to(torch.float32).contiguous()
    sf = sigma.to(device=dev, dtype=torch.float32).expand_as(xf).contiguous()
    score = torch.empty_like(xf)
    idx = torch.empty(*xf.shape, 2, dtype=torch.int32, device=dev) if want_idx else None
    _check(lib.pp_so2_score(_ptr(xf), _ptr(sf), xf.numel(), 1 if pi_periodic else 0, _ptr(score), _ptr(idx), idx_dev, _stream(dev)),
           "pp_so2_score")
    return (score, idx) if want_idx else score


class AffinityHead:
    """The tensors PackPPI-AP owns besides the two networks (mut_bias, seq_embedding, mutation_fusion, ddg_predictor) on one
    GPU: ``pp_affinity_create``.  ``state_dict`` holds at least weights.affinity_head_spec(mode)."""

    def __init__(self, state_dict, device, mode="network"):
        from .weights import affinity_head_spec
        lib = load()
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.mode = mode
        flat = np.ascontiguousarray(torch.cat([torch.as_tensor(state_dict[n]).detach().float().cpu().reshape(-1)
                                               for n, _ in affinity_head_spec(mode)]).numpy(), dtype=np.float32)
        h = C.c_void_p()
        _check(lib.pp_affinity_create(flat.ctypes.data, flat.size, self.device.index, C.byref(h)), "pp_affinity_create")
        self.handle = h

    def encode(self, ctx: "Context", residue_type, sc_sincos, mut_mask, hV_pret):
        """AffinityPrediction.encode after the pretrained features, on ``ctx`` (a Context of the mutation-branch plan whose
        batch carries the local mask as residue_mask): [B, L, 128] MPNN output.

        A NaN or infinity in ``hV_pret`` or ``sc_sincos`` is NOT flagged: pp_affinity_encode does not set bit 2 of
        ``ctx.saturated()`` for them (only the context's own batch tensors are scanned when it is built).  ``hV_pret`` is this
        path's own pp_score output, whose inputs are scanned by the pretrained network's context; a caller that passes features
        from elsewhere checks them itself."""
        dev = self.device
        rt = residue_type.to(device=dev, dtype=torch.int64).contiguous()
        sc = sc_sincos.to(device=dev, dtype=torch.float32).contiguous()
        mm = mut_mask.to(device=dev, dtype=torch.int64).contiguous()
        hp = hV_pret.to(device=dev, dtype=torch.float32).contiguous()
        n = ctx.n_rows
        if rt.numel() != n or sc.numel() != 8 * n or mm.numel() != n or hp.numel() != 128 * n:
            raise RuntimeError("pp_affinity_encode: tensors do not match the context's rows")
        hV = torch.empty(hp.shape, dtype=torch.float32, device=dev)
        _check(load().pp_affinity_encode(self.handle, ctx.handle, _ptr(rt), _ptr(sc), _ptr(mm), _ptr(hp), _ptr(hV),
                                         ctx._stream()), "pp_affinity_encode")
        return hV

    def predict(self, h_wt, h_mt, seg_offsets):
        """(ddg [n_seg], ddg_inv [n_seg]): ddg_predictor of the max over each segment's rows of h_mt - h_wt / h_wt - h_mt.
        ``seg_offsets``: int list or tensor [n_seg + 1] of row offsets into the flattened [rows, 128] tensors."""
        dev = self.device
        hw = h_wt.to(device=dev, dtype=torch.float32).contiguous()
        hm = h_mt.to(device=dev, dtype=torch.float32).contiguous()
        if hw.shape != hm.shape or hw.shape[-1] != 128:
            raise RuntimeError("pp_affinity_predict: h_wt and h_mt must have the same shape [..., 128]")
        rows = hw.numel() // 128
        offs = torch.as_tensor(seg_offsets).to(dtype=torch.int32)
        if offs.device.type == "cpu":
            o = offs.tolist()
            if o[0] < 0 or o[-1] > rows or any(b < a for a, b in zip(o[:-1], o[1:])):
                raise RuntimeError(f"seg_offsets {o} do not describe {rows} rows")
        offs = offs.to(dev).contiguous()
        n_seg = offs.numel() - 1
        ddg = torch.empty(n_seg, dtype=torch.float32, device=dev)
        inv = torch.empty(n_seg, dtype=torch.float32, device=dev)
        _check(load().pp_affinity_predict(self.handle, _ptr(hw), _ptr(hm), _ptr(offs), int(n_seg), int(rows), _ptr(ddg), _ptr(inv),
                                          _stream(dev)), "pp_affinity_predict")
        return ddg, inv

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and _lib is not None:
            _lib.pp_affinity_destroy(h)
            self.handle = None
