"""Anchors on the device, through the C ABI (pp_anchor_close).

Reference: tests/anchor_oracle.py, the brute-force restatement of the definition, in float32.  Its float64 form is the arbiter: the
largest difference between the two on the same inputs (Emin, and E, every distance and every angle at the float32 pick), times 4, is
the tolerance of every comparison of an energy, distance or angle (a row left open is held to its own Emin's difference).  A device pick is right if at that point the oracle's E is at most
thr + tol and the oracle's J at most its minimum over F + tol (a near-tie may resolve either way between acos implementations).
status and count must be equal, and every angle outside the first n chi of the closed rows bit for bit.  Nothing measured on the
device enters a bound.

Sites are synthetic: a target is placed at d0 from a donor atom of the structure rebuilt at its own angles, at theta0 to the donor's
antecedent, in a seeded azimuth.  Fixtures: tests/golden/g0_protein_2FTL.npz, g13_incomplete_L40.npz, synth.make_complex and the
packed batches of tests/large_cases.py."""
import functools
import os

import numpy as np
import pytest
import torch

from packppi_amd import constants as rc
from packppi_amd import selection as S

from . import anchor_oracle as O
from . import large_cases as LC
from . import stream_gate as SG
from . import test_streams_gpu as G
from .conftest import GOLD
from .test_streams_gpu import world          # noqa: F401  (the module-scoped fixture of the stream rows)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D0, SD, TH0, ST = 2.1, 0.1, 120.0, 15.0
A2G = np.asarray(rc.atom14_to_group)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch(tag, shift=None):
    from packppi_amd.featurize import protein_to_batch
    z = np.load(os.path.join(GOLD, f"g0_protein_{tag}.npz"))
    prot = {k[5:]: z[k] for k in z.files if k.startswith("prot.")}
    if shift is not None:
        prot = dict(prot, atom_positions=(prot["atom_positions"] + np.asarray(shift, np.float32)).astype(np.float32))
    return protein_to_batch(prot)


@functools.lru_cache(maxsize=None)
def synth_batch(L, seed):
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    return protein_to_batch(synth.make_complex(L, seed))


def host(b):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


def offsets(b):
    return LC.offsets(b)


def new_ctx(b):
    from packppi_amd.functional import geometry_plan
    from packppi_amd.lib import Context
    gb = b.to(DEV)
    ctx = Context(geometry_plan(torch.device(DEV)), gb)
    ctx._keep = gb
    return ctx


def rows_of_type(hb, resname):
    rt = hb["residue_type"].reshape(-1)
    am = hb["atom_mask"].reshape(-1, 14)
    t = rc.resname_to_idx[resname]
    return [int(r) for r in np.nonzero(rt == t)[0] if (am[r][np.asarray(rc.atom14_mask[t]) != 0] != 0).all()]


def donor(hb, row, depth=4):
    """The last slot of ``row`` that a chi angle up to chi ``depth`` moves, or None."""
    rt = int(hb["residue_type"].reshape(-1)[row])
    am = hb["atom_mask"].reshape(-1, 14)[row]
    ok = [s for s in range(5, 14) if rt < 20 and rc.atom14_mask[rt][s] != 0 and am[s] != 0 and 4 <= A2G[rt, s] <= 3 + depth]
    return ok[-1] if ok else None


def native(hb, row):
    """atom14 [14, 3] of ``row`` rebuilt at the batch's own angles, float64, in the batch's coordinates."""
    chi = hb["SC_D"].reshape(-1, 4)[row][None].astype(np.float64)
    return O._atoms(hb, row, chi, np.float64)[0] + hb["X"].reshape(-1, 14, 3)[row, 1].astype(np.float64)


def site(hb, row, slot, az, d0=D0, sd=SD, th0=TH0, st=ST, dist=None):
    """One entry: the target at ``dist`` (default d0) from the native donor at th0 to its antecedent, azimuth ``az``."""
    rt = int(hb["residue_type"].reshape(-1)[row])
    ante = rc.anchor_antecedent(rt, slot)
    q = O.place_target(native(hb, row), slot, ante, d0 if dist is None else dist, th0, az)
    return (row, slot, ante, q, (d0, sd, th0, st), f"row {row} {rc.atom14_names[rt][slot]}", "metal")


def named(hb, resname, atom, k, az, **kw):
    row = rows_of_type(hb, resname)[k]
    return site(hb, row, rc.atom14_names[rc.resname_to_idx[resname]].index(atom), az, **kw)


def noisy(chi, seed, deg=30.0):
    g = torch.Generator().manual_seed(seed)
    x = chi.clone().float()
    return torch.remainder(x + np.deg2rad(deg) * torch.randn(x.shape, generator=g) + np.pi, 2 * np.pi) - np.pi


def run(ctx, a, chi, **kw):
    return ctx.anchors(chi, a, check=False, **kw)


def oracle_tolerance(r32, r64):
    """{row: tolerance} and the largest float32-against-float64 difference of the oracle.  The tolerance of every row that has a pick
    or is kept is ONE number: 4 x the largest difference over all such rows of Emin, and of E, every distance and every angle at the
    float32 pick (a kept row: its report).  A row left open has no pick and only its Emin is compared, within 4 x its own Emin's
    difference: the huge Emin of a far target must not loosen the bound of the rows that close.  Never wider than one bound over
    everything."""
    d, own = 0.0, {}
    for r, e in r32["emin"].items():
        own[r] = abs(float(e) - float(r64["emin"][r]))
    for r, k in r32["pick"].items():
        if not np.isfinite(r32["J"][r][k]):
            continue
        d = max(d, own[r], abs(float(r32["E"][r][k]) - float(r64["E"][r][k])))
        for name in ("D", "ANG"):
            d = max(d, float(np.abs(r32[name][r][:, k].astype(np.float64) - r64[name][r][:, k]).max()))
    kept = [int(r) for r in np.nonzero(r32["status"] == 2)[0]]
    for r in kept:
        d = max(d, float(np.abs(r32["report"][r].astype(np.float64) - r64["report"][r]).max()))
    picked = {r for r, k in r32["pick"].items() if np.isfinite(r32["J"][r][k])} | set(kept)
    return {r: 4.0 * (d if r in picked else own[r]) for r in set(own) | set(kept)}, d


def both(hb, offs, a, chi, cache, **kw):
    """(the float32 oracle, {row: tolerance}); the rows that close or are kept must be resolved to better than 5e-3."""
    r32 = O.solve(hb, offs, a, chi=chi, dtype=np.float32, cache=cache, **kw)
    r64 = O.solve(hb, offs, a, chi=chi, dtype=np.float64, cache=cache, **kw)
    tol, diff = oracle_tolerance(r32, r64)
    print(f"oracle float32 against float64 {diff:.3e}")
    assert np.array_equal(r32["status"], r64["status"])
    assert all(0 < t < 5e-3 for r, t in tol.items() if r32["status"][r] in (1, 2))
    print("tolerance", max(t for r, t in tol.items() if r32["status"][r] in (1, 2, -2)) if tol else 0.0)
    return r32, tol


def flat_index(angles, g):
    k = (np.asarray(angles, np.float64) + np.pi) / (2 * np.pi / g)
    assert np.abs(k - np.rint(k)).max() < 1e-3                      # a closed row's angles are grid angles
    k = np.rint(k).astype(int) % g
    return int(np.ravel_multi_index(tuple(k), [g] * len(k)))


def check_against(res, ref, tol, chi_in):
    """status, count, reports and the picks of a device result against an oracle result."""
    status = res.status.cpu().numpy()
    report = res.report.cpu().numpy().astype(np.float64)
    arep = res.anchor_report.cpu().numpy().astype(np.float64)
    assert np.array_equal(status, ref["status"]), (status[status != ref["status"]], ref["status"][status != ref["status"]])
    assert np.array_equal(res.count.cpu().numpy(), ref["count"])
    out = res.chi.reshape(-1, 4).cpu().numpy() if res.chi is not None else None
    same = np.ones((len(status), 4), bool)
    written = np.zeros(len(arep), bool)
    tols = tol
    for r, idx in ref["lists"].items():
        tol = tols[r]
        if ref["status"][r] == 2 or (ref["status"][r] == -2 and r not in ref["E"]):             # kept
            assert np.abs(report[r] - ref["report"][r]).max() <= tol, (r, report[r], ref["report"][r])
            assert np.abs(arep[idx] - ref["anchor_report"][idx]).max() <= tol
            written[idx] = True
            continue
        assert abs(report[r, 0] - float(ref["emin"][r])) <= tol, (r, report[r], ref["emin"][r])
        if r not in ref["pick"] or not np.isfinite(ref["J"][r][ref["pick"][r]]):                  # open
            assert not report[r, 1:].any()
            continue
        n, g = ref["n"][r], ref["g"][r]
        if out is not None:
            same[r, :n] = False
            k = flat_index(out[r, :n], g)
        else:
            k = ref["pick"][r]
        assert ref["E"][r][k] <= ref["thr"][r] + tol, (r, k, float(ref["E"][r][k]), float(ref["thr"][r]))
        assert ref["Jall"][r][k] <= ref["J"][r].min() + tol, (r, k, float(ref["Jall"][r][k]), float(ref["J"][r].min()))
        want = (ref["emin"][r], ref["E"][r][k], ref["D"][r][0, k], ref["ANG"][r][0, k])
        assert np.abs(report[r] - np.asarray(want, np.float64)).max() <= tol, (r, report[r], want)
        assert np.abs(arep[idx, 0] - ref["D"][r][:, k]).max() <= tol and np.abs(arep[idx, 1] - ref["ANG"][r][:, k]).max() <= tol
        written[idx] = True
    assert not arep[~written].any()
    none = np.ones(len(status), bool)
    none[list(ref["lists"])] = False
    assert not report[none].any()
    if out is not None:
        assert np.array_equal(out[same].view(np.uint32), chi_in.reshape(-1, 4)[same].view(np.uint32))      # every other angle bit for bit
    return status, report, out


FOUR = (("CYS", "SG"), ("HIS", "NE2"), ("GLU", "OE1"), ("LYS", "NZ"))      # n = 1, 2, 3, 4
_CACHE = {}


@functools.lru_cache(maxsize=None)
def four_sites():
    hb = host(batch("2FTL"))
    return S.anchor_set_of([named(hb, rn, atom, 0, 0.4 + k) for k, (rn, atom) in enumerate(FOUR)])


# ---- 1. the device against the float32 oracle, one row of each n -------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["native", "noise"])
def test_device_equals_the_oracle(start):
    b = batch("2FTL")
    hb, a = host(b), four_sites()
    chi = b["SC_D"] if start == "native" else noisy(b["SC_D"], 17)
    ref, tol = both(hb, offsets(b), a, chi.numpy(), _CACHE)
    assert [ref["n"][int(r)] for r in a.rows] == [1, 2, 3, 4] and (ref["status"][a.rows] == 1).all()
    res = run(new_ctx(b), a, chi)
    _, report, _ = check_against(res, ref, tol, chi.numpy())
    assert res.closed() == sorted(int(r) for r in a.rows)
    for r in a.rows:
        print(int(r), report[r], ref["report"][r])
        assert abs(report[r, 2] - D0) <= SD * np.sqrt(report[r, 0] + 4) + tol[int(r)]


# ---- 2. several anchors on a row ----------------------------------------------------------------------------------------------------------------
def test_two_four_and_five_anchors_on_a_row():
    b = batch("2FTL")
    hb = host(b)
    asp, glu = rows_of_type(hb, "ASP")[0], rows_of_type(hb, "GLU")[1]
    t = rc.resname_to_idx
    od1, od2 = (rc.atom14_names[t["ASP"]].index(x) for x in ("OD1", "OD2"))
    oe1, oe2 = (rc.atom14_names[t["GLU"]].index(x) for x in ("OE1", "OE2"))
    e1 = site(hb, asp, od1, 0.3, d0=2.3, st=25.0)
    two = [e1, (asp, od2, e1[2], e1[3], (2.3, SD, TH0, 25.0), "asp od2", "metal")]                  # one target, both oxygens
    four = [site(hb, glu, oe1, 0.2), site(hb, glu, oe2, 1.2), site(hb, glu, oe1, 2.2, dist=2.6), site(hb, glu, oe2, 3.2, dist=2.6)]
    fifth = site(hb, glu, oe1, 4.0)
    chi = noisy(b["SC_D"], 5, 20.0)
    a4, a5 = S.anchor_set_of(two + four), S.anchor_set_of(two + four + [fifth])
    ref, tol = both(hb, offsets(b), a4, chi.numpy(), {}, max_energy=200.0)
    assert ref["status"][asp] == 1 and ref["status"][glu] == 1 and len(ref["lists"][glu]) == 4
    ctx = new_ctx(b)
    res4 = run(ctx, a4, chi, max_energy=200.0)
    check_against(res4, ref, tol, chi.numpy())
    ref5 = O.solve(hb, offsets(b), a5, chi=chi.numpy(), max_energy=200.0, cache={})
    assert ref5["status"][glu] == -2 and ref5["lists"][glu] == ref["lists"][glu]
    res5 = run(ctx, a5, chi, max_energy=200.0)
    assert int(res5.status[glu]) == -2 and int(res5.status[asp]) == 1 and res5.count.tolist() == [1]
    assert torch.equal(res5.chi, res4.chi) and torch.equal(res5.report, res4.report)                 # the fifth is dropped, nothing else
    assert torch.equal(res5.anchor_report[:6], res4.anchor_report) and not bool(res5.anchor_report[6].any())
    with pytest.raises(RuntimeError, match="dropped"):
        res5.closed()
    with pytest.raises(ValueError, match="fifth"):
        ctx.anchors(chi, a5)


# ---- 3. open and kept rows ------------------------------------------------------------------------------------------------------------------------
def test_open_and_kept_rows():
    b = batch("2FTL")
    hb, a = host(b), four_sites()
    far = named(hb, "HIS", "NE2", 1, 0.9, dist=15.0)
    a = S.anchor_set_of([tuple(x[i] for x in (a.rows, a.slots, a.antes, a.targets, a.params, a.labels, a.kinds)) for i in range(4)] + [far])
    chi = noisy(b["SC_D"], 23)
    fixed = np.zeros(hb["residue_type"].size, np.uint8)
    fixed[[int(a.rows[1]), int(a.rows[3])]] = 1
    ref, tol = both(hb, offsets(b), a, chi.numpy(), _CACHE, fixed=fixed)
    assert ref["status"][a.rows].tolist() == [1, 2, 1, 2, -1]
    res = run(new_ctx(b), a, chi, fixed=torch.from_numpy(fixed))
    _, report, out = check_against(res, ref, tol, chi.numpy())
    rows = [int(r) for r in a.rows]
    for r in (rows[1], rows[3], rows[4]):                                                         # kept and open rows: bit-equal
        assert np.array_equal(out[r].view(np.uint32), chi.numpy().reshape(-1, 4)[r].view(np.uint32))
    assert report[rows[1], 0] == report[rows[1], 1] and report[rows[1], 2] > 0 and report[rows[4], 0] > 10.0
    assert res.count.tolist() == [2] and res.pinned().sum().item() == 4


# ---- 4 / 5. in place; no angles -----------------------------------------------------------------------------------------------------------------
def test_in_place_equals_out_of_place():
    b = batch("2FTL")
    a = four_sites()
    chi = noisy(b["SC_D"], 29)
    ctx = new_ctx(b)
    res = run(ctx, a, chi)
    x = ctx._chi(chi).clone()
    inp = ctx._anchor_close(x, None, *a.device_arrays(DEV), len(a), 10.0, np.deg2rad(20.0), out=x)
    assert inp.chi is x
    for k in ("chi", "status", "report", "anchor_report", "count"):
        assert torch.equal(res[k].view(torch.int32), inp[k].view(torch.int32)), k
    assert not torch.equal(x.cpu(), chi.reshape(x.shape))


def test_without_angles_the_pick_is_at_emin():
    b = batch("2FTL")
    hb, a = host(b), four_sites()
    ref, tol = both(hb, offsets(b), a, None, {})
    res = run(new_ctx(b), a, None)
    assert res.chi is None
    _, report, _ = check_against(res, ref, tol, None)
    rows = [int(r) for r in a.rows[:2]]                              # chi1 and chi2 alone: no angle beyond n reads the missing chi
    assert all(abs(report[r, 0] - report[r, 1]) <= tol[r] for r in rows)


# ---- 6. packing invariance ----------------------------------------------------------------------------------------------------------------------
def segment_sites(hb, seed, want=3):
    rng = np.random.default_rng(seed)
    rows = [r for r in range(hb["residue_type"].size) if donor(hb, r) is not None]
    rows = sorted(rng.choice(rows, size=min(want, len(rows)), replace=False).tolist())
    return S.anchor_set_of([site(hb, r, donor(hb, r), float(rng.uniform(0, 6))) for r in rows])


def test_a_segment_gets_the_same_bits_alone_and_packed():
    from packppi_amd.batch import pack
    parts = [synth_batch(40, 13), synth_batch(64, 12), synth_batch(33, 11)]
    sets = [segment_sites(host(p), 50 + i) for i, p in enumerate(parts)]
    packed = pack(parts)
    offs = packed["seg_offsets_host"]
    assert offs == [0, 40, 104, 137]
    chi = noisy(packed["SC_D"], 31)
    ctx = new_ctx(packed)
    res = ctx.anchors(chi, [s.shifted(offs[i], i) for i, s in enumerate(sets)])
    a0 = 0
    for i, (p, s) in enumerate(zip(parts, sets)):
        lo, hi = offs[i], offs[i + 1]
        alone = new_ctx(p).anchors(chi[:, lo:hi], s)
        assert int(alone.count[0]) == int(res.count[i]) and int(alone.count[0]) >= 1
        for k, sl in (("chi", slice(lo, hi)), ("status", slice(lo, hi)), ("report", slice(lo, hi)), ("anchor_report", slice(a0, a0 + len(s)))):
            got = res[k].reshape(-1, *res[k].shape[2:])[sl] if k == "chi" else res[k][sl]
            want = alone[k].reshape(-1, *alone[k].shape[2:]) if k == "chi" else alone[k]
            assert torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)), (i, k)
        a0 += len(s)
    with pytest.raises(ValueError, match="segment"):
        ctx.anchors(chi, [sets[0].shifted(offs[1], 0)])


# ---- 7. every row; more than 1024 rows ------------------------------------------------------------------------------------------------------------
def test_every_row_of_a_complex():
    b = synth_batch(24, 7)
    hb = host(b)
    rows = [r for r in range(24) if donor(hb, r, 2) is not None]
    assert len(rows) >= 12
    a = S.anchor_set_of([site(hb, r, donor(hb, r, 2), 0.25 * r) for r in rows])
    chi = noisy(b["SC_D"], 37)
    ref, tol = both(hb, offsets(b), a, chi.numpy(), {})
    res = run(new_ctx(b), a, chi)
    check_against(res, ref, tol, chi.numpy())
    assert int(res.count[0]) == int((ref["status"] == 1).sum()) >= 10


def test_rows_at_the_scan_boundaries_of_a_large_context():
    b = LC.many()
    hb = host(b)
    entries = []
    for r in (255, 256, 1023, 1024, LC.N_ROWS - 1):
        s = donor(hb, r, 2)
        # a row without a side chain still goes through the row scan: its entry is invalid and marks the row
        entries.append(site(hb, r, s, 0.1 * (r % 7)) if s is not None else (r, 5, 4, np.zeros(3), (D0, SD, TH0, ST), f"row {r}", "metal"))
    a = S.anchor_set_of(entries)
    chi = noisy(b["SC_D"], 41)
    ref, tol = both(hb, offsets(b), a, chi.numpy(), {})
    assert set(ref["status"][a.rows].tolist()) <= {1, -2} and (ref["status"] == 1).sum() >= 2
    res = run(new_ctx(b), a, chi)
    check_against(res, ref, tol, chi.numpy())


# ---- 8. incomplete side chains --------------------------------------------------------------------------------------------------------------------
def test_an_anchor_on_a_missing_atom_is_dropped():
    from .test_incomplete_host import load_incomplete
    b, _ = load_incomplete("L40")
    hb = host(b)
    rt, am = hb["residue_type"].reshape(-1), hb["atom_mask"].reshape(-1, 14)
    missing = [(r, s) for r in range(rt.size) if rt[r] < 20 and hb["residue_mask"].reshape(-1)[r] != 0 and am[r, :3].all()
               for s in range(5, 14) if rc.atom14_mask[rt[r]][s] != 0 and am[r, s] == 0 and 4 <= A2G[rt[r], s] <= 5]
    whole = [r for r in range(rt.size) if donor(hb, r, 2) is not None and hb["residue_mask"].reshape(-1)[r] != 0 and am[r, :5].all()
             and r not in {m[0] for m in missing}][:3]
    assert missing and len(whole) == 3
    r0, s0 = missing[0]
    bad = (r0, s0, rc.anchor_antecedent(int(rt[r0]), s0), hb["X"].reshape(-1, 14, 3)[r0, 1] + 3.0, (D0, SD, TH0, ST), "missing", "metal")
    a = S.anchor_set_of([bad] + [site(hb, r, donor(hb, r, 2), 0.5 + r) for r in whole])
    chi = noisy(b["SC_D"], 43)
    ref, tol = both(hb, offsets(b), a, chi.numpy(), {})
    assert ref["status"][r0] == -2 and (ref["status"][whole] == 1).all()
    ctx = new_ctx(b)
    check_against(run(ctx, a, chi), ref, tol, chi.numpy())
    with pytest.raises(ValueError, match="missing.*lacks"):
        ctx.anchors(chi, a)


# ---- 9. far from the origin: the reported distance is the distance of the written atoms ---------------------------------------------------------
@pytest.mark.parametrize("shift,bound", [(None, 1e-3), ((1000.0, -2000.0, 500.0), 1e-2)])
def test_reported_distance_is_the_atoms_distance(shift, bound):
    """The bounds of tests/test_disulfide_gpu.py for the same comparison: fp32 spacing at 100 A is 8e-6 and a few dozen operations lie
    between the backbone and the distance: 1e-3 A; at (1000, -2000, 500) the spacing is 1.2e-4 and pp_atom14 works in absolute
    coordinates: 1e-2 A."""
    b = batch("2FTL", shift)
    hb = host(b)
    a = S.anchor_set_of([named(hb, rn, atom, 0, 0.4 + k) for k, (rn, atom) in enumerate(FOUR)])
    ctx = new_ctx(b)
    res = run(ctx, a, noisy(b["SC_D"], 17))
    assert res.closed() == sorted(int(r) for r in a.rows)
    xyz = ctx.atom14(res.chi).reshape(-1, 14, 3).double().cpu().numpy()
    arep = res.anchor_report.cpu().numpy()
    for i in range(len(a)):
        d = np.linalg.norm(xyz[a.rows[i], a.slots[i]] - a.targets[i].astype(np.float64))
        print(int(a.rows[i]), d, arep[i, 0])
        assert abs(d - arep[i, 0]) <= bound and abs(d - D0) < 0.3
    if shift is not None:                                            # and the closure itself does not see the shift
        here = run(new_ctx(batch("2FTL")), four_sites(), noisy(b["SC_D"], 17))
        assert torch.equal(here.status, res.status)
        assert float((here.report - res.report).abs().max()) < 0.05


# ---- 10. a target on the chi axis -----------------------------------------------------------------------------------------------------------------
def test_energy_constant_in_chi_picks_the_grid_angle_nearest_the_sample():
    b = batch("2FTL")
    hb = host(b)
    row = rows_of_type(hb, "CYS")[1]
    nat = native(hb, row)
    axis = (nat[4] - nat[1]) / np.linalg.norm(nat[4] - nat[1])
    q = nat[4] + 1.5 * axis                                          # on the CA-CB line: chi1 turns SG about it
    d0 = float(np.linalg.norm(nat[5] - q))
    u, v = nat[4] - nat[5], q - nat[5]
    th0 = float(np.degrees(np.arccos(u @ v / np.linalg.norm(u) / np.linalg.norm(v))))
    a = S.AnchorSet.concat([S.AnchorSet([row], [5], [4], [q], [(d0, SD, th0, ST)]), four_sites()])      # next to the four rows of test 1
    assert row not in four_sites().rows.tolist()
    chi = b["SC_D"].clone()
    chi[0, row, 0] = 0.5 + 0.4 * (2 * np.pi / 72)                    # 0.4 of a step above a grid angle: no tie
    ref, tol = both(hb, offsets(b), a, chi.numpy(), _CACHE)
    assert float(ref["E"][row].max()) < 1e-3                         # constant in chi1 up to rounding
    res = run(new_ctx(b), a, chi)
    check_against(res, ref, tol, chi.numpy())
    th = O.theta(72)
    want = int(np.argmin(np.abs(O.wrap(th.astype(np.float64) - float(chi[0, row, 0]), np.float64))))
    assert float(res.chi[0, row, 0]) == float(th[want]) and ref["pick"][row] == want


def test_an_exact_tie_goes_to_the_lowest_flat_index():
    """d0 = 1e9 A swallows the distance: (d - d0) is -1e9 at every grid point in float32, E is the same word everywhere, and so is J
    (the angle term of J is below half an ulp of 1e18).  5184 equal values over all 256 lanes: the pick must be flat index 0, with
    angles and without.  (A start halfway between two grid angles on a target on the chi axis is only a near-tie: E there is constant
    up to rounding, and rounding would choose.)"""
    b = batch("2FTL")
    hb = host(b)
    row = rows_of_type(hb, "HIS")[0]
    slot = rc.atom14_names[rc.resname_to_idx["HIS"]].index("NE2")
    a = S.AnchorSet([row], [slot], [rc.anchor_antecedent(rc.resname_to_idx["HIS"], slot)], [hb["X"].reshape(-1, 14, 3)[row, 1] + 3.0],
                    [(1e9, 1.0, 0.0, 0.0)])
    ref = O.solve(hb, offsets(b), a, chi=b["SC_D"].numpy(), max_energy=np.inf, cache={})
    assert ref["n"][row] == 2 and np.unique(ref["E"][row]).size == 1 and np.unique(ref["J"][row]).size == 1 and ref["pick"][row] == 0
    ctx = new_ctx(b)
    for chi in (b["SC_D"], None):
        res = run(ctx, a, chi, max_energy=float("inf"))
        assert int(res.status[row]) == 1 and res.count.tolist() == [1]
        assert float(res.report[row, 0]) == float(res.report[row, 1]) == float(ref["E"][row][0])
        if chi is not None:
            th0 = float(O.theta(72)[0])
            assert res.chi[0, row, :2].tolist() == [th0, th0]
            assert torch.equal(res.chi[0, row, 2:].cpu().view(torch.int32), chi[0, row, 2:].view(torch.int32))


# ---- 11. a busy non-default stream ----------------------------------------------------------------------------------------------------------------
def _anchor_row(w, case):
    """The angles behind the gate; the anchors (three rows per segment) are on the device before it."""
    b = w.cpu[case]
    hb = host(b)
    offs = offsets(b)
    rng = np.random.default_rng(3)
    entries = []
    for s in range(len(offs) - 1):
        rows = [r for r in range(offs[s], offs[s + 1]) if donor(hb, r) is not None]
        for r in sorted(rng.choice(rows, size=3, replace=False).tolist()):
            entries.append(site(hb, r, donor(hb, r), float(rng.uniform(0, 6))))
    a = S.anchor_set_of(entries)
    c = w.ctx(case)
    arrays = a.device_arrays(DEV)
    torch.cuda.synchronize(DEV)

    def fn(bufs):
        return dict(c._anchor_close(c._chi(bufs["chi"]), None, *arrays, len(a), 10.0, np.deg2rad(20.0)))
    return dict(ctx=c, fn=fn, inputs={"chi": w.chi(case, 1)}, poison={"chi": w.chi(case, 2)})


ROWS = [G.Row("pp_anchor_close", case, _anchor_row, never_waits=True) for case in G.SHAPES]
# new lists, not appends: that file's own parametrised test keeps the table it was decorated with (tests/test_refine_streams_gpu.py)
G.ROWS = G.ROWS + [r for r in ROWS if r.id not in {q.id for q in G.ROWS}]
G.TABLE_ENTRIES = sorted({r.entry for r in G.ROWS})


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_entry_on_a_busy_stream(row, world):     # noqa: F811
    spec = row.make(world, row.case)
    SG.gated_call(spec["fn"], spec["inputs"], spec["poison"], entry=row.id, never_waits=row.never_waits)


# ---- 12. through the module -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(weights):
    from packppi_amd.module import TDiffusionModule
    return TDiffusionModule(weights, device=DEV)


def test_sampling_with_anchors(model):
    b = synth_batch(24, 7)
    hb = host(b)
    rows = [r for r in range(24) if donor(hb, r, 2) is not None][:3]
    a = S.anchor_set_of([site(hb, r, donor(hb, r, 2), 0.7 * r) for r in rows])
    gb = b.to(DEV)
    plain = model.sampling(gb, seed=11)
    assert torch.equal(model.sampling(gb, seed=11, anchors=None), plain) and model.anchor_reports == []      # None is today's path
    model.keep_anchor_report = True
    try:
        out = model.sampling(gb, seed=11, anchors=a)
        rep = model.anchor_reports[-1]
        assert torch.equal(rep["chi_before"], plain) and torch.equal(rep["chi_after"], out)
        status = rep["status"].cpu().numpy()
        assert (status[rows] == 1).all() and int(rep["count"][0]) == 3
        same = torch.ones(24, 4, dtype=torch.bool)
        for r in rows:
            n = int(A2G[int(hb["residue_type"].reshape(-1)[r]), donor(hb, r, 2)]) - 3
            same[r, :n] = False
            assert not torch.equal(out[0, r, :n], plain[0, r, :n])
        assert torch.equal(out.cpu().reshape(24, 4)[same].view(torch.int32), plain.cpu().reshape(24, 4)[same].view(torch.int32))
        prox = model.sampling(gb, seed=11, anchors=a, use_proximal=True)
        closed = model.anchor_reports[-1]["chi_after"]
        assert torch.equal(closed, out)                                  # the same sample, the same closure
        assert torch.equal(prox[0, rows].view(torch.int32), closed[0, rows].view(torch.int32))      # the pinned stage keeps the grid angles
        assert torch.equal(model.repack(gb, torch.zeros(1, 24), seed=11, anchors=[a]), model.repack(gb, torch.zeros(1, 24), seed=11, anchors=a))
    finally:
        model.keep_anchor_report = False
        model.anchor_reports.clear()
    with pytest.raises(ValueError, match="return_trajectory with anchors"):
        model.sampling(gb, seed=11, anchors=a, return_trajectory=True, fixed_mask=torch.zeros(1, 24))      # behind every other refusal
    with pytest.raises(ValueError, match="needs batch.pdb_path"):
        model.sampling(gb, seed=11, anchors="auto")


# ---- argument rules of the export ----------------------------------------------------------------------------------------------------------------
def test_argument_rules():
    b = batch("2FTL")
    a = four_sites()
    ctx = new_ctx(b)
    arrays = a.device_arrays(DEV)
    x = ctx._chi(b["SC_D"])
    for kw, msg in ((dict(max_energy=float("nan")), "max_energy"), (dict(sigma_chi=0.0), "sigma_chi"), (dict(sigma_chi=float("inf")), "sigma_chi")):
        with pytest.raises(RuntimeError, match=msg):
            ctx._anchor_close(x, None, *arrays, len(a), kw.get("max_energy", 10.0), kw.get("sigma_chi", 0.35))
    with pytest.raises(RuntimeError, match="need chi"):
        ctx._anchor_close(None, ctx._mask(np.zeros(ctx.n_rows), "fixed"), *arrays, len(a), 10.0, 0.35)
    with pytest.raises(RuntimeError, match="anchors, a context"):
        ctx._anchor_close(x, None, *arrays, 8 * ctx.n_rows + 1, 10.0, 0.35)
    with pytest.raises(ValueError, match="fixed needs chi"):
        ctx.anchors(None, a, fixed=np.zeros(ctx.n_rows))
    none = ctx.anchors(b["SC_D"], S.AnchorSet())                      # an empty set: nothing closes, the angles come back
    assert not bool(none.status.any()) and none.count.tolist() == [0] and torch.equal(none.chi.cpu(), b["SC_D"].float())
