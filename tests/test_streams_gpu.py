"""GPU: every export that takes a ``void *stream`` on a busy non-default stream.

The rest of the suite runs every kernel on the default stream of an idle device, where no ordering mistake can show.  Here every
stream-taking entry is called under ``torch.cuda.stream(s)`` while ``s`` is still held up by a gate and its inputs hold valid but
WRONG data that the copies behind the gate replace (tests/stream_gate.py); the result must be the default-stream result bit for
bit.  For the entries the header documents as not waiting for the stream the gate must still be pending when the call returns.

``ROWS`` is the entry table, ``EXEMPT`` the exports left out with the reason; tests/test_streams_host.py holds both against
include/packppi_hip.h, so a new stream-taking export cannot be added without a row here.

Shapes: a padded complex of L = 70 (``c70``), a packed batch of 33 + 64 + 40 rows (``pack``), 2 groups x 3 decoys of 33 and 40 rows
(``decoy``); schedules of 4 entries, 5 proximal steps or sweeps.  ``python -m pytest tests/test_streams_gpu.py -m gpu -s`` prints
``entry, t_host, G, pending`` per row.
"""
import ctypes as C
import gc
import threading
import time

import numpy as np
import pytest
import torch

from . import stream_gate as SG

pytestmark = pytest.mark.gpu

DEV = SG.DEV
VTF, TOL, LAMDA = 12.0, 0.5, 1.0
SEED = 7
SCHED = [1.0, 0.66, 0.33, 0.0]
STEPS = 5

# exports that take a stream and have no row, each with its reason
EXEMPT = {
    "pp_time_kernel": "measurement aid: times launches with events and synchronises the stream by design",
    "pp_debug_edge": "laboratory entry of the diagnostic library only: one launch for tools/debug, not part of the product ABI",
    "pp_debug_nm": "laboratory entry of the diagnostic library only: one launch for tools/debug, not part of the product ABI",
    "pp_debug_score_prefix": "laboratory entry of the diagnostic library only: a prefix of pp_score's launches for the layer parity test",
}


class Row:
    def __init__(self, entry, case, make, never_waits=False, network=False, tag=""):
        self.entry, self.case, self.make, self.never_waits, self.network = entry, case, make, never_waits, network
        self.id = f"{entry}-{case}" + (f"-{tag}" if tag else "")


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
class World:
    """Plan, batches and angles of the three shapes; built once per module."""

    def __init__(self, weights):
        from packppi_amd import synth
        from packppi_amd.batch import pack, replicate_many
        from packppi_amd.featurize import protein_to_batch
        from packppi_amd.lib import Plan

        def mk(n, seed):
            return protein_to_batch(synth.make_complex(n, seed))
        self.parts = [mk(33, 11), mk(64, 12), mk(40, 13)]
        self.parts_alt = [mk(33, 21), mk(64, 22), mk(40, 23)]                 # other complexes of the same lengths
        self.cpu = {"c70": mk(70, 101), "pack": pack(self.parts), "decoy": replicate_many([self.parts[0], self.parts[2]], 3)}
        # the poison of a whole batch: another complex of the same length; for the packed batch another VALID segment table of the
        # same total within the same [min_len, max_len]
        self.cpu_alt = {"c70": mk(70, 202), "pack": pack([mk(40, 31), mk(33, 32), mk(64, 33)]),
                        "decoy": replicate_many([self.parts_alt[0], self.parts_alt[2]], 3)}
        assert self.cpu["pack"].seg_offsets_host == [0, 33, 97, 137] and self.cpu_alt["pack"].seg_offsets_host == [0, 40, 73, 137]
        assert self.cpu["decoy"].seg_offsets_host == [0, 33, 66, 99, 139, 179, 219]
        self.plan = Plan(weights, DEV)
        self.plan.set_clash_params(VTF, TOL)
        self.dev = {k: v.to(DEV) for k, v in self.cpu.items()}
        g = torch.Generator().manual_seed(5)
        self.score_norm = (0.5 + torch.rand(2, 5001, generator=g, dtype=torch.float64)).to(DEV)
        torch.cuda.synchronize(DEV)

    def n(self, case):
        return int(self.cpu[case].max_size)

    def ctx(self, case, plan=None):
        """A fresh context of ``case``, prepared on the default stream; the device is idle on return."""
        from packppi_amd.lib import Context
        c = Context(plan or self.plan, self.dev[case])
        c._keep = self.dev[case]
        torch.cuda.synchronize(DEV)
        return c

    def chi(self, case, seed):
        b = self.cpu[case]
        g = torch.Generator().manual_seed(1000 + seed)
        return ((torch.rand(b.SC_D.shape, generator=g) * 2 - 1) * 3.0) * b.SC_D_mask

    def rand(self, seed, *shape, normal=False):
        g = torch.Generator().manual_seed(2000 + seed)
        return torch.randn(*shape, generator=g) if normal else torch.rand(*shape, generator=g)

    def mask(self, case, seed, p):
        return (self.rand(seed, 1, self.n(case)) < p).to(torch.uint8)


@pytest.fixture(scope="module")
def world(weights):
    return World(weights)


def _cur():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# ---- row builders: each returns dict(fn, inputs, poison[, ctx, joint, controls]) ---------------------------------------------------------
def chi_row(call):
    """Rows whose one gated input is the angles."""
    def make(w, case):
        c = w.ctx(case)
        return dict(ctx=c, fn=lambda b: call(c, b["chi"]), inputs={"chi": w.chi(case, 1)}, poison={"chi": w.chi(case, 2)})
    return make


def multi_row(names, call):
    """Rows with several gated inputs: ``names`` maps an input name to (w, case, seed) -> host tensor."""
    def make(w, case):
        c = w.ctx(case)
        return dict(ctx=c, fn=lambda b: call(c, w, b), inputs={k: f(w, case, 1) for k, f in names.items()},
                    poison={k: f(w, case, 2) for k, f in names.items()})
    return make


CHI = lambda w, case, seed: w.chi(case, seed)                                                    # noqa: E731
T_ROWS = lambda w, case, seed: 0.05 + 0.9 * w.rand(10 + seed, w.n(case))                         # noqa: E731
NOISE = lambda w, case, seed: w.rand(20 + seed, len(SCHED) - 1, 2, w.n(case), 4, normal=True)    # noqa: E731
FIXED = lambda w, case, seed: w.mask(case, 30 + seed, 0.4)                                       # noqa: E731
SEEDS = lambda w, case, seed: w.mask(case, 40 + seed, 0.1)                                       # noqa: E731
ROWS4 = lambda w, case, seed: w.rand(50 + seed, w.n(case), 4, normal=True)                       # noqa: E731
TARGET = lambda w, case, seed: w.rand(55 + seed, w.n(case), 4, normal=True)                      # noqa: E731
CHI_REF = lambda w, case, seed: w.chi(case, 10 + seed)                                           # noqa: E731
PER_RES = lambda w, case, seed: w.rand(60 + seed, w.n(case))                                     # noqa: E731


def prepare_row(check):
    """Rows whose gated inputs are the batch itself: every batch tensor and the device segment table go behind the gate, the context
    is prepared under the busy stream and ``check(ctx, chi)`` reads it out.  The poison is another valid batch (``World.cpu_alt``)."""
    def make(w, case):
        from packppi_amd.batch import Batch
        from packppi_amd.lib import Context, _BATCH_SPEC
        real, alt = w.cpu[case], w.cpu_alt[case]
        keys = [k for k, _ in _BATCH_SPEC] + (["seg_offsets"] if case != "c70" else [])
        meta = {k: v for k, v in real.items() if not isinstance(v, torch.Tensor)}
        chi = w.chi(case, 1).to(DEV)
        keep = []

        def fn(b):
            c = Context(w.plan, Batch(meta, **b))
            keep[:] = [c]
            return check(c, chi)
        return dict(fn=fn, inputs={k: real[k] for k in keys}, poison={k: alt[k] for k in keys}, joint=True, keep=keep)
    return make


def _raw_row(case, build):
    """Host-table rows, through raw ctypes (the wrappers build their host arrays themselves, so only a raw call can overwrite the
    array the library was given): ``build(w, c, lib)`` -> (run(b, first, second), A, B); the row passes table A, overwrites the
    array with B the moment the call returns and runs the consumer; the control swaps A and B and must give another result."""
    def make(w, _case):
        from packppi_amd import lib as L
        c = w.ctx(case)
        run, A, B = build(w, c, L)
        return dict(ctx=c, fn=lambda b: run(b, A, B), controls=[("the values the table is overwritten with", lambda b: run(b, B, A))],
                    inputs={"chi": w.chi(case, 1)}, poison={"chi": w.chi(case, 2)})
    return make


def _rng_keys(w, c, L):
    def run(b, first, second):
        keys = np.array(first, dtype=np.uint64)
        L._check(L.load().pp_ctx_set_rng_keys(c.handle, C.c_void_p(keys.ctypes.data), _cur()), "pp_ctx_set_rng_keys")
        keys[:] = np.array(second, dtype=np.uint64)
        return c.sample(b["chi"], SCHED, "sde", seed=SEED)
    return run, [5, 2 ** 40 + 9, 77], [1, 2, 3]


def _obstacles(w, c, L):
    ca = w.cpu["pack"].X[0, :, 1, :]
    xyzr = torch.cat([ca + 2.5, torch.full((ca.shape[0], 1), 1.7)], 1).contiguous().to(DEV)
    M = int(xyzr.shape[0])

    def run(b, first, second):
        rng = np.array(first, dtype=np.int32)
        L._check(L.load().pp_ctx_set_obstacles(c.handle, _ptr(xyzr), C.c_void_p(rng.ctypes.data), M, _cur()), "pp_ctx_set_obstacles")
        rng[:] = np.array(second, dtype=np.int32)
        return c.clash(b["chi"], VTF, TOL, need_grad=True)
    return run, [[0, 33], [33, 64], [97, 40]], [[97, 40], [0, 33], [33, 64]]


def _norm_rows(w, c, L):
    def run(b, first, second):
        nr = np.array(first, dtype=np.int32)
        chi = b["chi"].to(torch.float32).contiguous()
        last, acc = torch.empty_like(chi), torch.empty_like(chi)
        losses = torch.empty(3, STEPS, device=DEV)
        L._check(L.load().pp_proximal_packed(c.handle, _ptr(chi), LAMDA, STEPS, C.c_void_p(nr.ctypes.data), None, _ptr(last), _ptr(acc),
                                             _ptr(losses), _cur()), "pp_proximal_packed")
        nr[:] = np.array(second, dtype=np.int32)
        return last, acc, losses
    return run, [40, 70, 48], [33, 64, 40]


def _schedule(w, c, L):
    def run(b, first, second):
        sched = np.array(first, dtype=np.float32)
        x = b["chi"].to(torch.float32).contiguous().clone()
        L._check(L.load().pp_sample_seeded(c.handle, _ptr(x), C.c_void_p(sched.ctypes.data), len(sched), 1, SEED, _cur()), "pp_sample_seeded")
        sched[:] = np.array(second, dtype=np.float32)
        return x
    return run, SCHED, [1.0, 0.5, 0.25, 0.0]


def _eta(w, c, L):
    def run(b, first, second):
        sched, eta = np.array(SCHED, dtype=np.float32), np.array(first, dtype=np.float32)
        x = b["chi"].to(torch.float32).contiguous().clone()
        L._check(L.load().pp_sample_guided(c.handle, _ptr(x), None, None, 1, C.c_void_p(sched.ctypes.data), len(sched), 1, SEED,
                                           C.c_void_p(eta.ctypes.data), 0.1, None, None, _cur()), "pp_sample_guided")
        eta[:] = np.array(second, dtype=np.float32)
        sched[:] = 0.5
        return x
    return run, [0.05] * 4, [0.2, 0.0, 0.1, 0.0]


def _set_graph(w, case):
    c = w.ctx(case)
    E = c.graph()[0].cpu()
    chi = w.chi(case, 1).to(DEV)

    def fn(b):
        c.set_graph(b["E"])
        return c.graph(), c.score(chi, 0.5)
    return dict(ctx=c, fn=fn, inputs={"E": E}, poison={"E": E.flip(-1).contiguous()})


def _saturated(w, case):
    c = w.ctx(case)

    def fn(b):
        s = c.score(b["chi"], 0.5)
        return s, c.saturated()
    return dict(ctx=c, fn=fn, inputs={"chi": w.chi(case, 1)}, poison={"chi": w.chi(case, 2)})


def _clash_params(w, case):
    """A plan of its own (the shared one keeps its parameters): (12, 0.5), then (10, 0.4), then pp_clash -- the last table must be the
    one the kernel reads."""
    from packppi_amd.lib import Plan
    plan = Plan(None, DEV)
    c = w.ctx(case, plan)

    def run(b, params):
        for vtf, tol in params:
            plan._clash_params = None
            plan.set_clash_params(vtf, tol)
        return c.clash(b["chi"], *params[-1], need_grad=True)
    return dict(ctx=c, plan=plan, fn=lambda b: run(b, [(VTF, TOL), (10.0, 0.4)]), controls=[("the first table", lambda b: run(b, [(VTF, TOL)]))],
                inputs={"chi": w.chi(case, 1)}, poison={"chi": w.chi(case, 2)})


def _so2(w, case):
    from packppi_amd.lib import so2_score
    n = w.n(case)
    return dict(fn=lambda b: so2_score(b["x"], b["sigma"], True, want_idx=True),
                inputs={"x": 0.5 * w.rand(71, n, 4, normal=True), "sigma": 0.05 + 1.5 * w.rand(72, n, 4)},
                poison={"x": 0.5 * w.rand(73, n, 4, normal=True), "sigma": 0.05 + 1.5 * w.rand(74, n, 4)})


def _affinity(which):
    def make(w, _case):
        from packppi_amd.affinity import mutant_view
        from packppi_amd.batch import Batch
        from . import test_affinity_gpu as A
        m = A.model("network")
        batch = A.batch_of("1BRS_LA87F")
        ctx = m._mutation_context(batch, m.get_local_subgraph(batch["X"][:, :, 1, :], batch["mut_mask"]))
        hp, hp_alt = m.get_pret_feature(batch).cpu(), m.get_pret_feature(mutant_view(batch)).cpu()
        mm = batch["mut_mask"].cpu()
        assert bool(mm.any()) and not bool(mm.all())
        torch.cuda.synchronize(DEV)
        if which == "encode":
            return dict(ctx=ctx, fn=lambda b: m.encode(Batch(batch, mut_mask=b["mut_mask"]), b["hV_pret"], ctx),
                        inputs={"mut_mask": mm, "hV_pret": hp}, poison={"mut_mask": mm.roll(3, 1), "hV_pret": hp_alt})
        L = int(batch["residue_type"].shape[1])
        return dict(fn=lambda b: m.head.predict(b["h_wt"], b["h_mt"], [0, L]),
                    inputs={"h_wt": hp, "h_mt": hp_alt}, poison={"h_wt": hp_alt, "h_mt": hp})
    return make


GRAPH_AND_SCORE = lambda c, chi: (c.graph(), c.score(chi, 0.5))                                  # noqa: E731
SHAPES = ("c70", "pack")

ROWS = []


def _add(entry, cases, make, **kw):
    for case in cases:
        ROWS.append(Row(entry, case, make, **kw))


# prepare: every batch tensor and the device segment table behind the gate; pending is not asserted (the first use of an arena may hipMalloc)
_add("pp_complex_prepare", ("c70",), prepare_row(GRAPH_AND_SCORE), network=True)
_add("pp_complex_prepare_packed", ("pack",), prepare_row(GRAPH_AND_SCORE), network=True)
# network
_add("pp_score", SHAPES, chi_row(lambda c, x: c.score(x, 0.37)), never_waits=True, network=True)
_add("pp_score_rows", SHAPES, multi_row({"chi": CHI, "t": T_ROWS}, lambda c, w, b: c.score_rows(b["chi"], b["t"])), never_waits=True, network=True)
_add("pp_sample", SHAPES, chi_row(lambda c, x: c.sample(x, SCHED)), never_waits=True, network=True, tag="ode")
_add("pp_sample", SHAPES, multi_row({"chi": CHI, "noise": NOISE}, lambda c, w, b: c.sample(b["chi"], SCHED, "sde", sde_noise=b["noise"])),
     never_waits=True, network=True, tag="sde")
_add("pp_sample_seeded", SHAPES, chi_row(lambda c, x: c.sample(x, SCHED, "sde", seed=SEED)), never_waits=True, network=True)
_add("pp_sample_partial", SHAPES, multi_row({"chi": CHI, "ref": CHI_REF, "fixed": FIXED}, lambda c, w, b: c.sample_partial(
    b["chi"], b["ref"], b["fixed"], SCHED, "sde", SEED, "renoise", trajectory=True)), never_waits=True, network=True)
_add("pp_sample_guided", SHAPES, chi_row(lambda c, x: c.sample_guided(x, SCHED, "sde", SEED, eta=[0.05] * 4, trajectory=True, want_trace=True)),
     never_waits=True, network=True)
_add("pp_sample_corrected", SHAPES, chi_row(lambda c, x: c.sample_corrected(x, SCHED, "sde", SEED, snr=[0.16] * 3, trajectory=True, want_corr=True)),
     never_waits=True, network=True)
# the draws depend on the segment table alone: the table goes behind the gate, the context is prepared under the busy stream
_add("pp_noise_seeded", ("pack",), prepare_row(lambda c, chi: c.noise(SEED, 0, want_words=True)), network=True)
_add("pp_add_noise_seeded", SHAPES, chi_row(lambda c, x: c.add_noise(x, 0.8, SEED)), never_waits=True, network=True)
_add("pp_dsm_loss", SHAPES, multi_row({"pred": ROWS4, "target": TARGET, "t": T_ROWS},
                                      lambda c, w, b: c.dsm_loss(b["pred"], b["target"], b["t"], w.score_norm)), never_waits=True, network=True)
_add("pp_so2_score", ("pack",), _so2, never_waits=True)
# geometry (sasa, polar and disulfides allocate a side workspace at their first call on a context: the baseline pass makes those
# calls on the same context, the gated call is at least the third)
_add("pp_atom14", SHAPES, chi_row(lambda c, x: c.atom14(x)), never_waits=True)
_add("pp_clash", SHAPES, chi_row(lambda c, x: c.clash(x, VTF, TOL, need_grad=True)), never_waits=True)
_add("pp_proximal", ("c70",), chi_row(lambda c, x: c.proximal(x, VTF, TOL, LAMDA, STEPS)), never_waits=True)
_add("pp_proximal_packed", SHAPES, chi_row(lambda c, x: c.proximal_packed(x, VTF, TOL, LAMDA, STEPS, want_traj=True)), never_waits=True)
_add("pp_proximal_pinned", SHAPES, multi_row({"chi": CHI, "fixed": FIXED}, lambda c, w, b: c.proximal_packed(
    b["chi"], VTF, TOL, LAMDA, STEPS, want_traj=True, fixed=b["fixed"], return_moved=True)), never_waits=True)
_add("pp_ctx_shell", SHAPES, multi_row({"seeds": SEEDS}, lambda c, w, b: c.shell(b["seeds"], radius=8.0, mode="atom", want_count=True)),
     never_waits=True)
_add("pp_sasa", SHAPES, chi_row(lambda c, x: dict(c.sasa(chi=x, want_counts=True))), never_waits=True)
_add("pp_polar", SHAPES, chi_row(lambda c, x: dict(c.polar(chi=x))), never_waits=True)
_add("pp_disulfide_close", SHAPES, chi_row(lambda c, x: dict(c.disulfides(chi=x))), never_waits=True)
_add("pp_ensemble_reduce", ("decoy",), multi_row({"chi": CHI, "per_res": PER_RES}, lambda c, w, b: dict(c.ensemble_reduce(
    b["chi"], 3, per_res=b["per_res"], select="clash"))), never_waits=True)
_add("pp_ensemble_recombine", ("decoy",), chi_row(lambda c, x: dict(c.ensemble_recombine(x, 3, max_sweeps=STEPS, want_energy=True))),
     never_waits=True)
# context setters with caller-owned host tables, overwritten the moment the call returns; a pageable copy may block: pending is recorded
_add("pp_ctx_set_rng_keys", ("pack",), _raw_row("pack", _rng_keys), network=True, tag="host-table")
_add("pp_ctx_set_obstacles", ("pack",), _raw_row("pack", _obstacles), tag="host-table")
_add("pp_proximal_packed", ("pack",), _raw_row("pack", _norm_rows), tag="host-norm_rows")
_add("pp_sample_seeded", ("c70",), _raw_row("c70", _schedule), network=True, tag="host-schedule")
_add("pp_sample_guided", ("c70",), _raw_row("c70", _eta), network=True, tag="host-eta")
# documented waiters (and the graph copy, which does not wait): the result only
_add("pp_ctx_set_graph", ("c70",), _set_graph, network=True)
_add("pp_ctx_get_graph", ("pack",), prepare_row(lambda c, chi: c.graph()), network=True)
_add("pp_ctx_saturated", ("c70",), _saturated, network=True)
_add("pp_ctx_live_rows", ("pack",), prepare_row(lambda c, chi: c.live_rows()), network=True)
_add("pp_plan_set_clash_params", ("c70",), _clash_params)
# PackPPI-AP
_add("pp_affinity_encode", ("1BRS",), _affinity("encode"), never_waits=True, network=True)
_add("pp_affinity_predict", ("1BRS",), _affinity("predict"))

TABLE_ENTRIES = sorted({r.entry for r in ROWS})


# ---- 2. the entry table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_entry_on_a_busy_stream(row, world):
    spec = row.make(world, row.case)
    SG.gated_call(spec["fn"], spec["inputs"], spec["poison"], entry=row.id, never_waits=row.never_waits,
                  joint=spec.get("joint", False), controls=spec.get("controls", ()))
    ctx = spec.get("ctx") or (spec.get("keep") or [None])[0]
    if row.network and ctx is not None:
        assert ctx.saturated() == 0


# ---- 3a. arena hand-over across streams ---------------------------------------------------------------------------------------------------
def _eq(a, b):
    return SG.same(a.detach().cpu(), b.detach().cpu())


@pytest.mark.parametrize("same_stream", [False, True], ids=["other-stream", "same-stream"])
def test_arena_handover_across_streams(same_stream, world):
    """Context A is prepared and sampled on s1 behind a gate and dropped while the gate is pending; B of the same size then takes A's
    workspace.  On another stream the pool has to wait for s1 (pp_ctx_destroy's promise) -- B's own stream is held by a gate of its
    own, so that without that wait the two contexts would run in the same memory at the same time --; on s1 itself nothing waits."""
    from packppi_amd.lib import Context
    w = world
    batch = w.dev["c70"]
    chiA, chiB = w.chi("c70", 1), w.chi("c70", 3)
    run = lambda c, x: c.sample(x, SCHED, "sde", seed=SEED)                                  # noqa: E731
    c0 = w.ctx("c70")
    wantA, wantB = run(c0, chiA.to(DEV)).cpu(), run(c0, chiB.to(DEV)).cpu()
    assert not _eq(wantA, wantB)
    del c0
    hold = [Context(w.plan, batch) for _ in range(4)]          # drains the pool of every workspace that fits: B must take A's
    torch.cuda.synchronize(DEV)
    s1, s2 = SG.side_stream(0), SG.side_stream(1)
    sB = s1 if same_stream else s2
    with torch.cuda.stream(s1):
        bufA, realA = w.chi("c70", 2).to(DEV), chiA.to(DEV)
        outA = torch.full((1, 70, 4), SG.SENTINEL_F, device=DEV)
        first = Context(w.plan, batch)                          # leaves the one pooled workspace that fits, on s1: A needs no hipMalloc,
        run(first, bufA)                                        # and torch's allocator the blocks of a run on s1
        del first
    with torch.cuda.stream(sB):
        bufB, realB = w.chi("c70", 2).to(DEV), chiB.to(DEV)
        if not same_stream:
            run(hold[0], bufB)                                  # likewise on s2
    torch.cuda.synchronize(DEV)
    with SG.quiet_gc():
        if not same_stream:
            with SG.Gated(s2, SG.SCENARIO_T_MS, [(bufB, realB)]):
                pass
        t0 = time.perf_counter()
        with SG.Gated(s1, SG.SCENARIO_T_MS, [(bufA, realA)]) as gA:
            A = Context(w.plan, batch)
            outA.copy_(run(A, bufA))
            del A
            gc.collect()
            dropped_pending = gA.pending()
        window_ms = (time.perf_counter() - t0) * 1e3
        with torch.cuda.stream(sB):
            if same_stream:
                bufB.copy_(realB)
            B = Context(w.plan, batch)
            pending_after_prepare = gA.pending()
            outB = run(B, bufB).clone()
    torch.cuda.synchronize(DEV)
    print(f"arena hand-over, {'same' if same_stream else 'other'} stream: dropped while pending={dropped_pending}, "
          f"pending after B's prepare={pending_after_prepare}; host time from the gate to the drop {window_ms:.2f} ms of G = {gA.G:.0f} ms")
    assert dropped_pending, "the gate had passed before A was dropped: nothing was raced"
    assert _eq(outA, wantA) and _eq(outB, wantB)
    if same_stream:
        assert pending_after_prepare, "taking a workspace over on the stream it was left on must not wait"
    else:
        assert not pending_after_prepare, "B took A's workspace on another stream without waiting for A's stream"
    del hold


def test_graph_copy_on_another_stream_is_covered_by_the_handover(world):
    """pp_ctx_get_graph reads the workspace on its stream like every other entry: a context prepared on s1 whose graph is copied out on
    s2 (ordered behind s1) and which is then dropped hands its workspace to a context on s1 only behind s2's copy."""
    from packppi_amd.lib import Context
    w = world
    batch = w.dev["c70"]
    c0 = w.ctx("c70")
    wantE, wantH = (t.cpu() for t in c0.graph())
    del c0
    hold = [Context(w.plan, batch) for _ in range(4)]
    other = w.cpu_alt["c70"].to(DEV)
    torch.cuda.synchronize(DEV)
    s1, s2 = SG.side_stream(0), SG.side_stream(1)
    with torch.cuda.stream(s2):
        hold[0].graph()                                         # torch's allocator gets the blocks of a graph copy on s2
    with torch.cuda.stream(s1):
        A = Context(w.plan, batch)
    torch.cuda.synchronize(DEV)
    with SG.quiet_gc():
        t0 = time.perf_counter()
        with SG.Gated(s2, SG.SCENARIO_T_MS, []) as g2:
            s2.wait_stream(s1)
            E, hE = A.graph()
            del A
            gc.collect()
            dropped_pending = g2.pending()
        window_ms = (time.perf_counter() - t0) * 1e3
        with torch.cuda.stream(s1):
            B = Context(w.plan, other)                          # another complex: its prepare rewrites the whole workspace
            pending_after_prepare = g2.pending()
    torch.cuda.synchronize(DEV)
    print(f"graph copy hand-over: dropped while pending={dropped_pending}, pending after the next prepare={pending_after_prepare}; "
          f"host time from the gate to the drop {window_ms:.2f} ms of G = {g2.G:.0f} ms")
    assert dropped_pending
    assert _eq(E, wantE) and _eq(hE, wantH)
    assert not pending_after_prepare, "the next context took the workspace without waiting for the stream of the graph copy"
    del B, hold


# ---- 3b. a context that changes stream ----------------------------------------------------------------------------------------------------
def _widen(batch):
    """The same batch in dtypes the context has to convert (float64, int32, uint8): every tensor it hands to the kernels is then a copy of its
    own, made on the stream that is current when the context is built.  The values are exactly representable either way."""
    from packppi_amd.batch import Batch
    out = Batch()
    for k, v in batch.items():
        if isinstance(v, torch.Tensor) and v.dtype == torch.float32:
            v = v.double()
        elif isinstance(v, torch.Tensor) and v.dtype == torch.int64:
            v = v.int()
        elif isinstance(v, torch.Tensor) and v.dtype == torch.bool:
            v = v.to(torch.uint8)
        out[k] = v
    return out


def test_context_changes_stream(world):
    """A context prepared on s1 makes a gated call on s1 and, while that is pending, a call on s2 ordered behind s1 by
    ``s2.wait_stream(s1)`` (the caller's duty, include/packppi_hip.h); it is dropped, tensors of the sizes of its converted batch
    copies are allocated and filled with another valid batch on s1 at once, and a new context is prepared and run on s2."""
    from packppi_amd.lib import Context, _BATCH_SPEC
    w = world
    batch, alt = _widen(w.cpu["c70"]).to(DEV), _widen(w.cpu_alt["c70"]).to(DEV)
    chi1, chi2, chi3 = (w.chi("c70", k) for k in (1, 3, 4))
    run = lambda c, x: c.sample(x, SCHED, "sde", seed=SEED)                                  # noqa: E731
    c0 = Context(w.plan, batch)
    assert len(c0._owned) == len(_BATCH_SPEC)                   # every batch tensor had to be converted
    want = [run(c0, x.to(DEV)).cpu() for x in (chi1, chi2, chi3)]
    del c0
    torch.cuda.synchronize(DEV)
    s1, s2 = SG.side_stream(0), SG.side_stream(1)
    with torch.cuda.stream(s1):
        c = Context(w.plan, batch)
        buf1, real1 = w.chi("c70", 2).to(DEV), chi1.to(DEV)
    with torch.cuda.stream(s2):
        x2, x3 = chi2.to(DEV), chi3.to(DEV)
    torch.cuda.synchronize(DEV)
    with SG.quiet_gc():
        with SG.Gated(s1, SG.SCENARIO_T_MS, [(buf1, real1)]) as g:
            o1 = run(c, buf1)
        s2.wait_stream(s1)
        with torch.cuda.stream(s2):
            o2 = run(c, x2)
        pending = g.pending()
        del c
        gc.collect()
        with torch.cuda.stream(s1):                             # the allocator's chance to hand the old blocks out
            fill = [alt[k].to(dt).contiguous() for k, dt in _BATCH_SPEC]
        with torch.cuda.stream(s2):
            c2 = Context(w.plan, batch)
            o3 = run(c2, x3)
    torch.cuda.synchronize(DEV)
    print(f"context changes stream: pending after the second call={pending}")
    assert pending, "the gate had passed before the context changed stream: nothing was raced"
    assert len(fill) == len(_BATCH_SPEC)
    for k, (got, ref) in enumerate(zip((o1, o2, o3), want)):
        assert _eq(got, ref), f"call {k + 1} differs from its default-stream baseline"
    assert c2.saturated() == 0


# ---- 3c. module level ----------------------------------------------------------------------------------------------------------------------
def _device_copy(b):
    from packppi_amd.batch import Batch
    return Batch({k: (v.to(DEV).clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items()})


def _gate_batches(stream, bufs, reals):
    copies = [(b[k], r[k]) for b, r in zip(bufs, reals) for k in b if isinstance(b[k], torch.Tensor)]
    return SG.Gated(stream, SG.SCENARIO_T_MS, copies)                        # G = 400 ms: module-level calls spend milliseconds on the host


@pytest.mark.parametrize("what", ["sampling", "sample_ensemble", "sample_sharded"])
def test_module_level_calls_under_a_busy_stream(what, world, weights):
    """The Python layer's own torch ops run between the library calls: the packed batch is written behind a gate and the call made
    under the busy stream must give the bits of the same call on the default stream."""
    from packppi_amd.batch import pack
    from packppi_amd.module import TDiffusionModule
    from packppi_amd.parallel import sample_sharded
    w = world
    m = TDiffusionModule(weights, device=DEV)
    m.schedule = torch.tensor(SCHED)
    m.hparams.sample_cfg.num_steps = STEPS
    m.hparams.sample_cfg.mode = "sde"
    if what == "sampling":
        reals, alts = [w.cpu["pack"]], [pack(w.parts_alt)]
        call = lambda bs: m.sampling(bs[0], seed=SEED)                                      # noqa: E731
    elif what == "sample_ensemble":
        reals, alts = w.parts, w.parts_alt
        call = lambda bs: m.sample_ensemble(list(bs), n_decoys=3, seed=SEED, use_proximal=True)      # noqa: E731
    else:
        reals, alts = w.parts, w.parts_alt
        call = lambda bs: sample_sharded(m, list(bs), seed=SEED, rank=0, world=1)            # noqa: E731
    want = SG.host(call([_device_copy(b) for b in reals]))
    assert not SG.differing(SG.host(call([_device_copy(b) for b in reals])), want)
    assert SG.differing(SG.host(call([_device_copy(b) for b in alts])), want)               # the poison is another input
    torch.cuda.synchronize(DEV)
    s = SG.side_stream(0)
    with torch.cuda.stream(s):
        bufs, real_dev = [_device_copy(b) for b in alts], [_device_copy(b) for b in reals]
    s.synchronize()
    with _gate_batches(s, bufs, real_dev) as g:
        out = call(bufs)
        pending = g.pending()
        got = [(n, t.detach().clone()) for n, t in SG.flat(out)]
        s.synchronize()
    print(f"{what:44s} under a busy stream: pending={pending} (not asserted: the Python layer reads back where it says so)")
    bad = SG.differing([(n, t.cpu()) for n, t in got], want)
    assert not bad, (what, bad)
    assert m.saturated() == 0


# ---- 3d. two contexts, two threads, two streams --------------------------------------------------------------------------------------------
def _sequence(w, c, case, chi, pred, target, t_rows):
    """sample_seeded -> proximal -> sasa -> polar -> dsm_loss, three times; every result as host tensors."""
    outs = []
    for _ in range(3):
        x = c.sample(chi, SCHED, "sde", seed=SEED)
        prox = c.proximal(x, VTF, TOL, LAMDA, STEPS) if case == "c70" else c.proximal_packed(x, VTF, TOL, LAMDA, STEPS, want_traj=True)
        sa = c.sasa(chi=x, want_counts=True)
        po = c.polar(chi=x, sasa=sa)
        loss = c.dsm_loss(pred, target, t_rows, w.score_norm)
        outs.append(SG.host((x, prox, dict(sa), dict(po), loss)))
    return outs


def test_two_contexts_two_threads_two_streams(world):
    from packppi_amd import lib as L
    w = world
    cases = ("c70", "pack")
    args = {case: [t.to(DEV) for t in (w.chi(case, 1), ROWS4(w, case, 1), TARGET(w, case, 1), T_ROWS(w, case, 1))] for case in cases}
    want = {case: _sequence(w, w.ctx(case), case, *args[case]) for case in cases}
    ctxs = {case: w.ctx(case) for case in cases}
    streams = {case: SG.side_stream(k) for k, case in enumerate(cases)}
    refused = threading.Event()
    got, errors, last_error = {}, [], {}

    def work(case):
        try:
            with torch.cuda.stream(streams[case]):
                if case == "pack":
                    last_error["before"] = L.load().pp_last_error()
                got[case] = _sequence(w, ctxs[case], case, *args[case])
                if case == "c70":
                    try:
                        ctxs[case].sample(args[case][0], [1.0], "sde", seed=SEED)       # a 1-entry schedule is refused
                        errors.append("a 1-entry schedule was accepted")
                    except RuntimeError as e:
                        last_error["refusal"] = str(e)
                    refused.set()
                else:
                    assert refused.wait(60.0)
                    last_error["after"] = L.load().pp_last_error()
        except Exception as e:                                   # noqa: BLE001
            refused.set()
            errors.append(f"{case}: {type(e).__name__}: {e}")

    threads = [threading.Thread(target=work, args=(case,)) for case in cases]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize(DEV)
    assert not errors, errors
    assert "refusal" in last_error and last_error["before"] == last_error["after"], last_error
    for case in cases:
        for k, (a, b) in enumerate(zip(got[case], want[case])):
            assert not SG.differing(a, b), (case, f"pass {k + 1}", SG.differing(a, b))
        assert ctxs[case].saturated() == 0


def test_rows_that_must_not_wait_did_not():
    """Summary of the run (after the table): every row marked never_waits that ran showed pending=True."""
    ran = {e: p for e, _, _, p in SG.ROWS_SEEN}
    late = [r.id for r in ROWS if r.never_waits and r.id in ran and not ran[r.id]]
    if SG.ROWS_SEEN:
        ts, gs = [t for _, t, _, _ in SG.ROWS_SEEN], [g for _, _, g, _ in SG.ROWS_SEEN]
        print(f"{len(SG.ROWS_SEEN)} rows: t_host {min(ts):.3f} .. {max(ts):.3f} ms, G {min(gs):.1f} .. {max(gs):.1f} ms; "
              f"rows that returned after the gate: {[e for e, _, _, p in SG.ROWS_SEEN if not p]}")
    assert not late, late
