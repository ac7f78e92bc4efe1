"""The shape of the live-row edge launch: one rule for every count of live rows, and the work table built from it (DESIGN.md
section 4.9).

With C compute units and S = 2 C co-resident two-row workgroups, M live rows are launched as
    M <= S: M one-row workgroups | S < M <= 3 S / 2: (M + 2) / 3 pairs + the rest one-row | 3 S / 2 < M <= 2 S: pairs |
    2 S < M <= 3 S: S pairs + M - 2 S one-row workgroups | 3 S < M: pairs
and contexts of S < N <= 3 S / 2 or 2 S < N <= 3 S rows take their live rows from a table ``mix[b]`` = the rows of workgroup b in
dispatch order, sized by N alone (the host never learns M).

CPU: the table on the host (``pp_live_mix_host``: the rule and the entry function the device kernel calls) over every (N, M) of a
small device, and the counts of the real one.  GPU: the device's table (``pp_ctx_live_rows`` + ``pp_ctx_live_mix``) against the host's
and against the same properties, and five reverse steps at live counts either side of every threshold of the rule against the same
run with ``PP_EDGE_LIVE=0`` (all rows, the launches of the parent): a row's arithmetic depends on its workgroup only through the
one- / two-row instance, which ``test_residues_per_workgroup_agree`` holds to 2e-5 rad, and the sticky saturation word must be equal.
"""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SLOTS = 2                           # PP_WGS2: two-row workgroups per CU
N_SCHEDULE = 6                      # five reverse steps
TOL = 2e-5                          # rad: what the one- and two-row instances are held to against each other


# ---- the properties of a table ---------------------------------------------------------------------------------------------------
def host_table(rows, n, cu):
    """(mix [n, 2], workgroups) of pp_live_mix_host for the live rows ``rows`` of an n-row context on ``cu`` compute units"""
    from packppi_amd import lib as L
    lib = L.load()
    rows = np.asarray(rows, dtype=np.int32)
    padded = np.concatenate([rows, np.full(n + 2 - len(rows), -1, np.int32)])
    mix, wg = np.full((n, 2), -7, np.int32), C.c_int(-1)
    st = lib.pp_live_mix_host(padded.ctypes.data_as(C.c_void_p), len(rows), n, cu, mix.ctypes.data_as(C.c_void_p), C.byref(wg))
    assert st == 0, lib.pp_last_error()
    return mix, wg.value


def expected_shape(m, cu):
    """(pairs, one_row) of the rule, written out independently of the library"""
    s = SLOTS * cu
    if m <= s:
        return 0, m
    if 2 * m <= 3 * s:
        return (m + 2) // 3, m - 2 * ((m + 2) // 3)
    if 2 * s < m <= 3 * s:
        return s, m - 2 * s
    return (m + 1) // 2, 0


def check_table(mix, wg, rows, n, cu, what):
    """Every live row exactly once and in front of the launch's end, nothing else, pairs before one-row entries, then (-1, -1)."""
    rows = np.asarray(rows, dtype=np.int32)
    assert mix.shape == (n, 2), what
    x, y = mix[:, 0], mix[:, 1]
    used = int((x >= 0).sum())
    assert np.all(x[:used] >= 0) and np.all(mix[used:] == -1), (what, "entries behind the last workgroup must be (-1, -1)")
    assert np.all(y[x < 0] < 0), what
    got = mix[:used].reshape(-1)
    got = got[got >= 0]
    assert np.array_equal(np.sort(got), rows), (what, "every live row exactly once, no other row")
    pairs = int((y >= 0).sum())
    assert np.all(y[:pairs] >= 0), (what, "pairs precede one-row entries")
    want_pairs, want_one = expected_shape(len(rows), cu)
    half = len(rows) % 2 if want_one == 0 and want_pairs > 0 else 0        # an odd count in pairs: the last pair holds (row, -1)
    assert (pairs, used - pairs) == (want_pairs - half, want_one + half), (what, pairs, used - pairs)
    if wg:
        assert used <= wg <= n, (what, "a live row behind the launch's last workgroup would be dropped", used, wg)


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def test_table_of_every_count_on_a_small_device():
    """C = 4 (S = 8): every context size up to 3 S + 2 rows and every live count 0 .. N, the live rows a random subset (so a dead row
    in the table shows); the launch is sized for the mixed regimes only and always holds the whole table."""
    cu, s = 4, 8
    rng = np.random.default_rng(11)
    sized = []
    for n in range(1, 3 * s + 3):
        for m in range(n + 1):
            rows = np.sort(rng.choice(n, m, replace=False)).astype(np.int32)
            mix, wg = host_table(rows, n, cu)
            check_table(mix, wg, rows, n, cu, (n, m))
            mixed_size = s < n <= 3 * s // 2 or 2 * s < n <= 3 * s
            assert (wg > 0) == mixed_size, (n, wg)
        if wg:
            sized.append(n)
    assert sized == list(range(s + 1, 3 * s // 2 + 1)) + list(range(2 * s + 1, 3 * s + 1))


def test_empty_list_one_row_and_single_row_context():
    for n, rows in ((739, []), (739, [5]), (1, [0]), (1, []), (1500, [1499])):
        mix, wg = host_table(rows, n, 256)
        check_table(mix, wg, rows, n, 256, (n, rows))
        assert (mix >= 0).sum() == len(rows)
        if rows:
            assert tuple(mix[0]) == (rows[0], -1)            # one row is a one-row workgroup, the first of the launch


@pytest.mark.parametrize("n,m,pairs,one_row,wg", [
    (739, 569, 190, 189, 512), (739, 512, 0, 512, 512), (739, 513, 171, 171, 512), (768, 768, 256, 256, 512),
    (1500, 1173, 512, 149, 988), (1500, 769, 385, 0, 988), (1500, 1024, 512, 0, 988), (1500, 1025, 512, 1, 988),
    (1536, 1536, 512, 512, 1024), (1537, 1537, 769, 0, 0), (1024, 1000, 500, 0, 0)])
def test_counts_on_256_compute_units(n, m, pairs, one_row, wg):
    """The fixtures (T1124: 569 live rows of 739, S1500: 1173 of 1500) and both sides of every threshold."""
    rows = np.arange(n - m, n, dtype=np.int32)
    mix, got_wg = host_table(rows, n, 256)
    check_table(mix, got_wg, rows, n, 256, (n, m))
    assert expected_shape(m, 256) == (pairs, one_row) and got_wg == wg
    assert pairs + one_row <= (wg or n)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _gpu_cases():
    """name -> (rows of the context, live rows), from the device's C: live counts either side of 2 C, 3 C, 2 S and 3 S.  The contexts
    of 3 C and 3 S - S / 2 rows hold live counts of a regime their own size is not in (M straddles a threshold that N does not)."""
    c = _cu()
    s = SLOTS * c
    mid, tail = 3 * c, 2 * s + s // 2 - 56
    return {"2C": (mid, 2 * c), "2C+1": (mid, 2 * c + 1), "3C": (mid, 3 * c), "3C+1": (tail, 3 * c + 1), "2S": (tail, 2 * s),
            "2S+1": (tail, 2 * s + 1), "3S": (3 * s, 3 * s), "3S+1": (3 * s + 1, 3 * s + 1)}


def _batch(n, m, seed):
    """A packed batch of three complexes, n rows in all, with exactly m live rows: no residue without an angle to begin with
    (tests/test_live_rows.py _typed), then n - m rows drawn at random lose their SC_D_mask (side chains nobody resolved)."""
    from packppi_amd.batch import pack
    from packppi_amd.featurize import protein_to_batch
    from .test_live_rows import _typed
    lens = [n // 3, n // 3, n - 2 * (n // 3)]
    b = pack([protein_to_batch(_typed(k, seed + i, ())) for i, k in enumerate(lens)])
    dead = np.random.default_rng(seed).choice(n, n - m, replace=False)
    for k in ("SC_D", "SC_D_mask", "SC_D_sincos"):
        b[k][0, dead] = 0
    for k in ("chi_1pi_periodic_mask", "chi_2pi_periodic_mask"):
        b[k][0, dead] = False
    live = np.flatnonzero((b.residue_mask.reshape(-1).numpy() != 0) & (b.SC_D_mask.reshape(-1, 4).numpy() != 0).any(-1))
    assert len(live) == m and b.residue_mask.numel() == n, (n, m, len(live))
    return b, live.astype(np.int32)


def _child_main(out_path):
    """Run in a fresh process (PACKPPI_LIB / PP_EDGE_LIVE in the environment: the switch is read once per process)."""
    from packppi_amd.module import TDiffusionModule
    from packppi_amd.weights import make_random_state_dict
    from .conftest import WEIGHT_SEED
    model = TDiffusionModule(make_random_state_dict(WEIGHT_SEED), device=DEV)
    sched = torch.linspace(1, 0, N_SCHEDULE)
    res = {}
    for i, (name, (n, m)) in enumerate(_gpu_cases().items()):
        b, _ = _batch(n, m, 400 + 10 * i)
        ctx = model._context(b.to(DEV))
        g = torch.Generator().manual_seed(17 + i)
        chi0 = (torch.rand(ctx.B, ctx.L, 4, generator=g) * 2 - 1) * 3.0 * b.SC_D_mask.reshape(ctx.B, ctx.L, 4)
        res[name + "/chi"] = ctx.sample(chi0, sched).cpu().numpy()
        res[name + "/saturated"] = np.array(ctx.saturated())
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def runs():
    """{(library, PP_EDGE_LIVE): arrays} -- four child processes, started together, once for the module."""
    from packppi_amd import build
    tmp = tempfile.mkdtemp(prefix="edge_shape_")
    procs = {}
    for which, lib in (("default", build.LIB), ("f32", build.other_variant_path())):
        assert os.path.exists(lib), f"{lib} is missing (__graft_entry__.build() builds it)"
        for live in ("0", "1"):
            out = os.path.join(tmp, f"{which}_{live}.npz")
            procs[(which, live)] = (subprocess.Popen(
                [sys.executable, "-c", f"import tests.test_edge_shape as t; t._child_main({out!r})"],
                env=dict(os.environ, PACKPPI_LIB=lib, PP_EDGE_LIVE=live), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                text=True), out)
    got = {}
    try:
        for key, (p, out) in procs.items():
            text, _ = p.communicate(timeout=600)
            assert p.returncode == 0, f"{key}: exit {p.returncode}\n{text[-3000:]}"
            got[key] = dict(np.load(out))
    finally:                        # a failure above must not leave a child on the GPU
        for p, _ in procs.values():
            if p.poll() is None:
                p.kill()
                p.wait()
        shutil.rmtree(tmp, ignore_errors=True)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["default", "f32"])
def test_live_launch_agrees_with_all_rows_at_every_threshold(runs, which):
    from .conftest import wrapped_absdiff
    all_rows, live = runs[(which, "0")], runs[(which, "1")]
    assert sorted(all_rows) == sorted(live) and len(live) == 2 * len(_gpu_cases())
    worst = {}
    for name, (n, m) in _gpu_cases().items():
        a, b = torch.from_numpy(all_rows[name + "/chi"]), torch.from_numpy(live[name + "/chi"])
        assert torch.isfinite(b).all() and b.abs().max() > 0.1, name
        worst[name] = float(wrapped_absdiff(a, b).max())
        print(f"{which} {name:5s} N {n:5d} live {m:5d}: max wrapped |dchi| {worst[name]:.2e} rad, saturated "
              f"{int(all_rows[name + '/saturated'])} / {int(live[name + '/saturated'])}")
    for name in worst:
        assert worst[name] <= TOL, (name, worst[name])
        assert int(all_rows[name + "/saturated"]) == int(live[name + "/saturated"]), name


@pytest.mark.gpu
def test_device_table_is_the_host_table(weights):
    """The table k_live_rows made for every case and for the two fixtures, read back through pp_ctx_live_rows and pp_ctx_live_mix."""
    from packppi_amd.module import TDiffusionModule
    from .conftest import load_golden
    model = TDiffusionModule(weights, device=DEV)
    cu = _cu()
    cases = {name: _batch(n, m, 400 + 10 * i) for i, (name, (n, m)) in enumerate(_gpu_cases().items())}
    for name in ("g4_T1124", "g5_S1500"):
        b = load_golden(name)[0]
        cases[name] = (b, np.flatnonzero((b.residue_mask.reshape(-1).numpy() != 0) &
                                         (b.SC_D_mask.reshape(-1, 4).numpy() != 0).any(-1)).astype(np.int32))
    tabled = 0
    for name, (b, live) in cases.items():
        ctx = model._context(b.to(DEV))
        n = ctx.n_rows
        assert np.array_equal(ctx.live_rows().cpu().numpy(), live), name
        mix, wg = ctx.live_mix()
        want, want_wg = host_table(live, n, cu)
        print(name, "rows", n, "live", len(live), "workgroups", wg, "shape", expected_shape(len(live), cu))
        assert wg == want_wg, name
        if wg == 0:
            assert mix is None and not (SLOTS * cu < n <= 3 * SLOTS * cu // 2 or 2 * SLOTS * cu < n <= 3 * SLOTS * cu), name
            continue
        tabled += 1
        mix = mix.cpu().numpy()
        check_table(mix, wg, live, n, cu, name)
        assert np.array_equal(mix, want), name
    assert tabled >= 8
