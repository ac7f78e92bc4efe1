"""Structures far from the origin and in arbitrary orientation, host side: the generators (``synth.rigid_motion``,
``synth.snap_to_grid``), the inputs and references that tests/test_rigid_motion_gpu.py shares, the conditions the reference alone must
satisfy for those tests to say anything, the PDB round trip at the edge of the 8.3f columns, and what a rigid motion does to the
featurisation of a planar omega.

Deposited structures sit hundreds of A from the origin (the PDB columns allow -999.999 .. 9999.999); one float32 ulp is 9.5e-7 A at
15 A and 2.4e-4 A at 3000 A.  Every reference here is ``oracle.ref_cpu`` (or a test module's restatement) on the SAME featurised batch
the device gets, in float64; its own float32 run on that batch says how much of a distance is the input's conditioning (``d_ref``).
A moved structure's result is never compared with the unmoved structure's: they are different inputs (see
``test_planar_omegas_are_decided_by_rounding``).

Motions: ``id`` (the control), ``R1@0`` (rotation only), ``R1@300``, ``R1@3000``, ``R2@3000``, ``R3@3000``: rotation ``k`` from the unit
quaternion of seed k, then a shift of the stated length along ``direction(k)``.  Inputs: A = make_complex(40, 3) (K = 32, three 16-row
tiles), B = make_complex(24, 5) (K = 24), C = drop_atoms(make_complex(64, 11), 64) (incomplete side chains, one row without atoms),
P = the pack of 37, 40 and 33 residues under ``id``, ``R1@3000`` and ``R2@3000`` with the direction negated, D = the padded batch of 40
and 36 residues at ``R1@3000`` with one residue masked mid-chain (its padding and masked rows sit at the origin).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from packppi_amd import constants as rc
from packppi_amd import synth
from packppi_amd.batch import Batch, collate, split
from packppi_amd.featurize import protein_to_batch, protein_to_data
from . import test_sasa_host as S
from .conftest import WEIGHT_SEED, wrapped_absdiff
from .test_clash_capacity import marginal_hinge_rows
from .test_obstacles_host import cast

MOTIONS = ("id", "R1@0", "R1@300", "R1@3000", "R2@3000", "R3@3000")
SINGLES = {"A": (40, 3, None), "B": (24, 5, None), "C": (64, 11, 64)}        # n_res, seed, drop_atoms seed
P_PARTS = ((37, 1437, "id", False), (40, 3, "R1@3000", False), (33, 1433, "R2@3000", True))
D_PARTS, D_MOTION, D_MASKED_ROW = ((40, 2), (36, 3)), "R1@3000", 17
EXACT_SHIFT = (2048.0, -3072.0, 2560.0)
VTF, TOL, LAMDA = 12.0, 0.5, 1.0
TIMES = ((1.0, "t1"), (0.5, "t05"), (1.0 / 30, "t30"))
BETA = dict(score=5e-5, hV=1e-4, hE0=2e-5, atom14=2e-5, sampling=1e-4, loss_rel=2e-5)
PROBE, N_POINTS = 1.4, 96


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ---- motions ---------------------------------------------------------------------------------------------------------------------
def parse(motion):
    """-> (rotation seed or None, shift length in A)."""
    if motion == "id":
        return None, 0.0
    rot, length = motion.split("@")
    return int(rot[1:]), float(length)


def direction(seed):
    """A seeded unit vector whose three components are all at least 0.2 in size and of mixed sign."""
    rng = np.random.default_rng(7000 + seed)
    while True:
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        if np.abs(v).min() >= 0.2 and abs(np.sign(v).sum()) == 1:
            return v


def shift_of(motion, negate=False):
    seed, length = parse(motion)
    if length == 0:
        return np.zeros(3)
    return (-1.0 if negate else 1.0) * length * direction(seed)


def move(protein, motion, negate=False):
    return synth.rigid_motion(protein, parse(motion)[0], shift_of(motion, negate))


def pool(cid):
    """The cases whose d_ref are pooled with ``cid``'s: the rotations of the same input at the same shift length (one rotation is one
    sample of fp32 rounding)."""
    if "-" not in cid:
        return [cid]
    inp, motion = cid.split("-")
    length = parse(motion)[1]
    return [f"{inp}-{m}" for m in MOTIONS if m != "id" and parse(m)[1] == length] if motion != "id" else [cid]


def mask_out(b, rows):
    """What featurisation does to a residue with a missing backbone atom, on the first complex of a batch (as
    tools/debug/fuzz_parity.py): its rows sit at the origin afterwards."""
    for r in rows:
        b.residue_mask[0, r] = 0.0
        for k in ("X", "atom_mask", "SC_D", "SC_D_mask", "BB_D", "BB_D_mask", "BB_D_sincos", "SC_D_sincos"):
            b[k][0, r] = 0
        for k in ("chi_1pi_periodic_mask", "chi_2pi_periodic_mask"):
            b[k][0, r] = False


@functools.lru_cache(maxsize=None)
def protein_of(inp):
    n, seed, damage = SINGLES[inp]
    p = synth.make_complex(n, seed)
    return synth.drop_atoms(p, damage) if damage is not None else p


# ---- cases -----------------------------------------------------------------------------------------------------------------------
class Case:
    """One input as the device gets it (``device_batch``) and as the oracle does: ``parts``, B = 1 batches on the host (the segments of
    a pack; the rows of the padded batch with their padding kept), never modified.  ``join`` / ``cut`` go between per-part tensors
    [1, L_s, ...] and the device layout."""

    def __init__(self, cid):
        self.id = cid
        if cid == "P":
            self.kind = "pack"
            self.parts = [protein_to_batch(move(synth.make_complex(n, s), m, neg)) for n, s, m, neg in P_PARTS]
        elif cid == "D":
            self.kind = "padded"
            self.whole = collate([protein_to_data(move(synth.make_complex(n, s), D_MOTION)) for n, s in D_PARTS])
            mask_out(self.whole, [D_MASKED_ROW])
            self.parts = split(self.whole)
        else:
            self.kind = "single"
            inp, motion = cid.split("-")
            self.parts = [protein_to_batch(move(protein_of(inp), motion))]
        self.lens = [int(p.residue_type.shape[1]) for p in self.parts]
        self.n_rows = sum(self.lens)
        self.max_abs = max(float(p.X.abs().max()) for p in self.parts)
        # the angle seed is chosen on the reference alone: with it at most 5 % of a case's residues sit at a hinge threshold
        # (test_few_residues_sit_at_a_hinge_threshold; of the offsets 0, 1000 .. 7000 three satisfy that)
        self.chi = [((torch.rand(1, n, 4, generator=torch.Generator().manual_seed(7000 + 100 * k + n)) * 2 - 1) * 3.0) * p.SC_D_mask
                    for k, (n, p) in enumerate(zip(self.lens, self.parts))]

    def device_batch(self, dev):
        from packppi_amd.batch import pack
        if self.kind == "pack":
            return pack([p.to(dev) for p in self.parts])
        return (self.whole if self.kind == "padded" else self.parts[0]).to(dev)

    def join(self, xs):
        return torch.cat(list(xs), 1 if self.kind == "pack" else 0)

    def cut(self, t):
        t = t.cpu()
        if self.kind == "pack":
            return list(torch.split(t, self.lens, 1))
        return [t[s:s + 1] for s in range(len(self.parts))]


@functools.lru_cache(maxsize=None)
def case(cid):
    return Case(cid)


def case_ids(inputs, extra=()):
    return [f"{i}-{m}" for i in inputs for m in MOTIONS] + list(extra)


@functools.lru_cache(maxsize=None)
def _weights():
    from packppi_amd.weights import make_random_state_dict
    return make_random_state_dict(WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def _weights64():
    return {k: v.double() for k, v in _weights().items()}


def bar(cid, beta, own, factor=3, control_at_beta=True):
    """(bar, pooled d_ref): ``max(beta, factor x d_ref)`` with d_ref pooled over ``pool(cid)`` by ``own(cid)``; the ``id`` motion is held
    to ``beta`` alone unless ``control_at_beta`` is off."""
    d_ref = max(own(c) for c in pool(cid))
    return (beta if cid.endswith("-id") and control_at_beta else max(beta, factor * d_ref)), d_ref


# ---- references, each computed once ------------------------------------------------------------------------------------------------
def _sorted_edges(E, hE):
    idx, perm = E.sort(-1)
    return idx, torch.gather(hE, 2, perm[..., None].expand(-1, -1, -1, hE.shape[-1]))


def real_edges(b, idx):
    """bool [1, L, K]: the row and the neighbour are both residues."""
    L = idx.shape[1]
    return (torch.gather(b.residue_mask[:, None].expand(-1, L, -1), 2, idx) > 0) & b.residue_mask.bool()[..., None]


@functools.lru_cache(maxsize=None)
def graph_ref(cid):
    """Per part: dict(idx: the fp64 oracle's lists sorted by neighbour, hE64 / hE32: both oracles' h_E0 in that order, E32: the fp32
    oracle's lists as they come, real, self_edge: bool [1, L, K] in the sorted order, gap: [L] the fp64 distance between ranks K and
    K + 1 of every row (inf where the row has no rank K + 1), d_ref: |hE32 - hE64| over real edges j != i)."""
    out = []
    for b in case(cid).parts:
        b64 = cast(b, torch.float64)
        E64, h64 = O.encode_static(_weights64(), b64)
        E32, h32 = O.encode_static(_weights(), b)
        idx, h64 = _sorted_edges(E64, h64)
        idx32, h32s = _sorted_edges(E32, h32)
        real = real_edges(b, idx)
        L = idx.shape[1]
        self_edge = idx == torch.arange(L).view(1, L, 1)
        valid = b.residue_mask[0].bool()
        ca = b64.X[0, :, 1]
        dist = torch.sqrt(((ca[:, None] - ca[None]) ** 2).sum(-1) + 1e-6)
        dist[:, ~valid] = float("inf")
        ranked = dist.sort(-1)[0]
        K = idx.shape[2]
        gap = (ranked[:, K] - ranked[:, K - 1]) if L > K else torch.full((L,), float("inf"), dtype=torch.float64)
        gap = torch.where(torch.isnan(gap), torch.full_like(gap, float("inf")), gap)          # inf - inf: fewer than K residues
        same = torch.equal(idx32[0][valid], idx[0][valid])
        use = real & ~self_edge
        d_ref = float((h32s.double() - h64)[use].abs().max()) if same else float("nan")
        out.append(dict(idx=idx, hE64=h64, hE32=h32s, E32=E32, real=real, self_edge=self_edge, gap=gap, valid=valid, d_ref=d_ref))
    return out


@functools.lru_cache(maxsize=None)
def network_ref(cid):
    """Per part: {32, 64: dict(score_<t>, hV_<t> at the three times, ode: ten ODE steps from the case's angles)}."""
    c = case(cid)
    sched = torch.linspace(1, 0, 11)
    out = []
    with torch.no_grad():
        for b, chi in zip(c.parts, c.chi):
            per = {}
            for prec, sd, bb, x, sc in ((32, _weights(), b, chi, sched), (64, _weights64(), cast(b, torch.float64), chi.double(), sched.double())):
                r = {}
                n = b.residue_type.numel()
                for tval, tn in TIMES:
                    t = torch.tensor([tval], dtype=x.dtype).repeat_interleave(n)
                    r[f"score_{tn}"], r[f"hV_{tn}"] = O.network(sd, bb, x, t)
                r["ode"] = O.sampling(sd, bb, x, sc)
                per[prec] = r
            out.append(per)
    return out


def network_dref(cid, what):
    """max over parts (and times) of |oracle fp32 - oracle fp64| of ``what``: score, hV or sampling."""
    worst = 0.0
    for b, per in zip(case(cid).parts, network_ref(cid)):
        if what == "sampling":
            m = b.SC_D_mask.bool()
            worst = max(worst, float(wrapped_absdiff(per[32]["ode"], per[64]["ode"])[m].max()))
        else:
            v = b.residue_mask.bool()
            worst = max([worst] + [float((per[32][f"{what}_{tn}"].double() - per[64][f"{what}_{tn}"])[v].abs().max()) for _, tn in TIMES])
    return worst


def hinge_window(cid):
    return max(1e-5, 4 * ulp32(case(cid).max_abs))


@functools.lru_cache(maxsize=None)
def geometry_ref(cid):
    """Per part: dict(xyz32, xyz64, pr32, pr64, g32, g64 at the case's angles -- the gradient is of the mean over the part's own rows --,
    marginal: bool [L] residues owning an atom pair within ``hinge_window`` of its hinge threshold in fp64)."""
    c = case(cid)
    out = []
    for b, chi in zip(c.parts, c.chi):
        b64 = cast(b, torch.float64)
        r = dict(xyz32=O.atom14_coords(b.X, b.residue_type, b.BB_D, chi),
                 xyz64=O.atom14_coords(b64.X, b64.residue_type, b64.BB_D, chi.double()))
        r["pr32"], r["g32"] = O.clash_and_grad(b, chi, VTF, TOL)
        r["pr64"], r["g64"] = O.clash_and_grad(b64, chi.double(), VTF, TOL)
        r["marginal"] = marginal_hinge_rows(b64, chi.double(), hinge_window(cid))
        out.append(r)
    return out


def geometry_dref(cid, what):
    worst = 0.0
    for r in geometry_ref(cid):
        if what == "atom14":
            worst = max(worst, float((r["xyz32"].double() - r["xyz64"]).abs().max()))
        elif what == "clash":
            worst = max(worst, float((r["pr32"].double() - r["pr64"]).abs().max()))
        else:
            use = ~r["marginal"]
            worst = max(worst, float((r["g32"].double() - r["g64"])[0][use].abs().max()))
    return worst


@functools.lru_cache(maxsize=None)
def proximal_ref(cid):
    """(losses of five proximal steps in fp32, in fp64) of a single-complex case."""
    c = case(cid)
    b, chi = c.parts[0], c.chi[0]
    _, l32 = O.proximal_optimizer(b, chi.clone(), VTF, TOL, LAMDA, 5)
    _, l64 = O.proximal_optimizer(cast(b, torch.float64), chi.double(), VTF, TOL, LAMDA, 5)
    return np.array(l32), np.array(l64)


def proximal_dref(cid):
    l32, l64 = proximal_ref(cid)
    return float(np.abs(l32 / l64 - 1).max())


def sasa_threshold(cid):
    """A^2: a test point is ambiguous when an occluder's |d2 - R_b^2| is below this in float64.  Two roundings at magnitude |X| per
    component of a test point (the coordinate itself and the point added to it) move d by up to sqrt(3) x 2 x ulp32(max |X|) / 2 each
    way, and d2 by 2 |d| times that with |d| <= R_b: 2 sqrt(3) max R_b ulp32(max |X|); never below the 1e-4 of tests/test_sasa_host.py."""
    rb = float(np.max(rc.slot_radius)) + PROBE
    return max(S.AMBIGUOUS, 2 * np.sqrt(3.0) * rb * ulp32(case(cid).max_abs))


@functools.lru_cache(maxsize=None)
def sasa_ref(cid):
    """(counts of the float32 restatement, counts of the float64 one, ambiguous points at ``sasa_threshold``, radius) over the rows of
    the device layout."""
    from packppi_amd.analysis import sphere_points
    c = case(cid)
    pts = sphere_points(N_POINTS)
    outs = []
    old = S.AMBIGUOUS
    S.AMBIGUOUS = sasa_threshold(cid)                     # restate() reads the module's threshold when it is called
    try:
        for b in c.parts:
            X, radius, chain = S.arrays(b)
            n = X.shape[0]
            c32 = S.restate(X, radius, chain, [0, n], pts, PROBE)
            c64, amb = S.restate(X, radius, chain, [0, n], pts, PROBE, dtype=np.float64, want_ambiguous=True)
            outs.append((c32, c64, amb, radius))
    finally:
        S.AMBIGUOUS = old
    return tuple(np.concatenate([o[k] for o in outs]) for k in range(4))


def shell_fp64(xyz, seeds, offs, radius, mode, amask, eps):
    """(shell uint8 [N] of tests/test_mutate_host.shell_numpy in float64 -- xyz as given, no fp32 rounding of the differences --,
    decided bool [N]: the row's membership is the same at radius - eps and radius + eps)."""
    from .test_mutate_host import shell_from_near
    xyz = np.asarray(xyz, np.float64).reshape(-1, 14, 3)
    res = []
    for r in (radius, radius - eps, radius + eps):
        near = []
        for a, b in zip(offs[:-1], offs[1:]):
            P = xyz[a:b]
            if mode == "ca":
                near.append(((P[:, None, 1] - P[None, :, 1]) ** 2).sum(-1) < r * r)
            else:
                m = np.asarray(amask).reshape(-1, 14)[a:b] != 0
                d2 = ((P[:, None, :, None] - P[None, :, None, :]) ** 2).sum(-1)
                near.append(((d2 < r * r) & m[:, None, :, None] & m[None, :, None, :]).any(axis=(2, 3)))
        res.append(shell_from_near(near, seeds, offs)[0])
    return res[0], res[1] == res[2]


def obstacle_case(motion):
    """tests/test_obstacles_host.chain_as_obstacles on input A under ``motion``: (chain A's rows as a B = 1 batch, its angles [1, La, 4],
    chain B's atoms at their angles as obstacles [M, 4] float64 -- they move with the complex, being built from its moved backbone)."""
    from packppi_amd.batch import TENSOR_KEYS
    full = protein_to_batch(move(protein_of("A"), motion))
    rows_a = (full.chain_indices[0] == 1).nonzero().flatten()
    rows_b = (full.chain_indices[0] != 1).nonzero().flatten()
    chi = ((torch.rand(1, 40, 4, generator=torch.Generator().manual_seed(1003)) * 2 - 1) * np.pi) * full.SC_D_mask
    part = Batch(num_proteins=1, max_size=int(rows_a.numel()))
    for k in TENSOR_KEYS:
        part[k] = full[k][:, rows_a]
    f = cast(full, torch.float64)
    xyz = O.atom14_coords(f["X"], f["residue_type"], f["BB_D"], chi.double())[0, rows_b]
    rad = (f["atom_mask"] * torch.as_tensor(rc.between_radius, dtype=torch.float64)[f["residue_type"]])[0, rows_b]
    keep = rad > 0
    return part, chi[:, rows_a], torch.cat((xyz[keep], rad[keep][:, None]), 1).float()


@functools.lru_cache(maxsize=None)
def obstacle_ref(motion):
    """(part, chi, obstacles float32 [M, 4] -- the device's and both references' input --, per_res and gradient of the restatement of
    tests/test_obstacles_host.py in fp32 and in fp64, marginal: bool [La] rows owning an atom within the hinge window of a protein or an
    obstacle hinge threshold in fp64)."""
    from .test_obstacles_host import clash_and_grad_obst
    part, chi, ob = obstacle_case(motion)
    p64 = cast(part, torch.float64)
    pr32, g32 = clash_and_grad_obst(part, chi, ob)
    pr64, g64 = clash_and_grad_obst(p64, chi.double(), ob.double())
    window = max(1e-5, 4 * ulp32(max(float(part.X.abs().max()), float(ob[:, :3].abs().max()))))
    xyz = O.atom14_coords(p64.X, p64.residue_type, p64.BB_D, chi.double())[0]
    rad = (p64.atom_mask * torch.as_tensor(rc.between_radius, dtype=torch.float64)[p64.residue_type])[0]
    d = torch.sqrt(1e-10 + ((xyz[:, :, None] - ob.double()[None, None, :, :3]) ** 2).sum(-1))             # [La, 14, M]
    near = ((rad[..., None] + ob.double()[None, None, :, 3] - TOL - d).abs() < window) & (rad[..., None] != 0)
    near[:, :4] = False
    marginal = marginal_hinge_rows(p64, chi.double(), window) | near.any(-1).any(-1)
    return dict(part=part, chi=chi, ob=ob, pr32=pr32, g32=g32, pr64=pr64, g64=g64, marginal=marginal)


def obstacle_dref(motion, what):
    r = obstacle_ref(motion)
    if what == "clash":
        return float((r["pr32"].double() - r["pr64"]).abs().max())
    return float((r["g32"].double() - r["g64"])[0][~r["marginal"]].abs().max())


class DecoyCase:
    """Input A under a motion with four uniform decoys, as tests/test_recombine_host.Case (whose properties it borrows)."""

    def __init__(self, motion):
        from . import test_recombine_host as R
        self.name, self.n, self.D = f"A-{motion}", 40, 4
        self.b = case(f"A-{motion}").parts[0]
        self.chis = R.decoy_angles(self.b, 40, 4, "uniform")

    @functools.cached_property
    def d_ref(self):
        """|oracle fp32 - oracle fp64| of the per-residue clash over the four decoys: the reference's own rounding of a sum of the kind
        a local energy is (hinges over the atoms of one row against its partners) on this batch."""
        b64 = cast(self.b, torch.float64)
        return max(float((O.residue_clash(self.b, x[None], VTF, TOL).double() - O.residue_clash(b64, x[None].double(), VTF, TOL)).abs().max())
                   for x in self.chis)


@functools.lru_cache(maxsize=None)
def decoy_case(motion):
    from . import test_recombine_host as R
    cls = type("MovedDecoyCase", (DecoyCase, R.Case), {})
    return cls(motion)


# ---- the generators ------------------------------------------------------------------------------------------------------------------
def test_rigid_motion_is_a_proper_rigid_motion():
    p = protein_of("C")
    before = {k: np.array(v, copy=True) for k, v in p.items()}
    same = synth.rigid_motion(p, None, (0.0, 0.0, 0.0))
    assert np.array_equal(same["atom_positions"], p["atom_positions"], equal_nan=True)        # the identity: bit for bit
    for seed in (1, 2, 3):
        R = synth.rotation_matrix(seed)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1.0) < 1e-15
        assert np.abs(R - np.eye(3)).max() > 0.3 and np.array_equal(R, synth.rotation_matrix(seed))
    assert np.array_equal(synth.rotation_matrix(None), np.eye(3))
    for motion in MOTIONS[1:]:
        seed, length = parse(motion)
        v = direction(seed)
        assert abs(np.linalg.norm(v) - 1) < 1e-12 and np.abs(v).min() >= 0.2 and set(np.sign(v)) == {-1.0, 1.0}
        assert abs(np.linalg.norm(shift_of(motion)) - length) < 1e-9 and length <= 3000.0
        assert np.array_equal(shift_of(motion, True), -shift_of(motion))
        q = move(p, motion)
        for k, v0 in before.items():                                  # a new dict, the input untouched
            assert np.array_equal(p[k], v0, equal_nan=v0.dtype.kind == "f")
            if k != "atom_positions":
                assert q[k] is p[k]
        x0, x1 = p["atom_positions"], q["atom_positions"]
        assert x1.dtype == np.float64 and np.array_equal(x1, x1.astype(np.float32).astype(np.float64), equal_nan=True)
        assert np.array_equal(np.isnan(x1), np.isnan(x0)) and np.isnan(x1).sum() > 0          # NaN slots stay NaN
        want = x0 @ synth.rotation_matrix(seed).T + shift_of(motion)
        ok = ~np.isnan(x0)
        assert np.abs(x1 - want)[ok].max() <= 0.5 * ulp32(np.abs(want[ok]).max())             # float64 arithmetic, one fp32 rounding
        # distances are kept to the rounding of the moved coordinates
        a, b = x0[:, 1], x1[:, 1]
        d0, d1 = np.linalg.norm(a[:, None] - a[None], axis=-1), np.linalg.norm(b[:, None] - b[None], axis=-1)
        assert np.abs(d0 - d1).max() <= 2 * np.sqrt(3.0) * ulp32(np.abs(b).max())
        if length:
            centre = np.nanmean(x1.reshape(-1, 3), 0)
            assert abs(np.linalg.norm(centre) - length) < 60.0 and np.abs(centre).min() > 0.15 * length
    assert np.array_equal(move(p, "R2@3000")["atom_positions"], move(p, "R2@3000")["atom_positions"], equal_nan=True)


def test_snap_to_grid_makes_a_translation_exact():
    p = protein_of("A")
    s = synth.snap_to_grid(p)
    x = s["atom_positions"]
    ok = ~np.isnan(x)
    assert np.array_equal(np.isnan(x), np.isnan(p["atom_positions"]))
    assert np.array_equal((x * 512)[ok], np.round(x * 512)[ok]) and np.abs(x - p["atom_positions"])[ok].max() <= 2.0 ** -10
    assert np.array_equal(synth.snap_to_grid(p, 4)["atom_positions"][ok] * 16, np.round(p["atom_positions"][ok] * 16))
    moved = synth.rigid_motion(s, None, EXACT_SHIFT)["atom_positions"]
    assert np.array_equal(moved[ok], (x + np.array(EXACT_SHIFT))[ok])                         # nothing was rounded
    b0, b1 = protein_to_batch(s), protein_to_batch(synth.rigid_motion(s, None, EXACT_SHIFT))
    ca0, ca1 = b0.X[0, :, 1], b1.X[0, :, 1]
    assert torch.equal(ca0[:, None] - ca0[None], ca1[:, None] - ca1[None])                    # every CA difference in float32
    assert torch.equal(O.knn_graph(ca0[None], b0.residue_mask), O.knn_graph(ca1[None], b1.residue_mask))


# ---- conditions the reference alone must satisfy ---------------------------------------------------------------------------------------
GRAPH_CASES = case_ids("AB", ("P", "D"))
NETWORK_CASES = GRAPH_CASES
GEOMETRY_CASES = case_ids("AC", ("P", "D"))
PROXIMAL_CASES = case_ids("AC")
SASA_CASES = case_ids("BC", ("P",))


@pytest.mark.parametrize("cid", GRAPH_CASES)
def test_neighbour_sets_are_decided_on_every_row(cid):
    c = case(cid)
    need = 8 * ulp32(max(float(b.X[0, :, 1].abs().max()) for b in c.parts))
    for b, g in zip(c.parts, graph_ref(cid)):
        gap = g["gap"][g["valid"]]
        print(f"{cid}: smallest fp64 gap between rank K and K + 1 {float(gap.min()):.3e} A, needed {need:.3e}")
        assert (gap > need).all()
        assert np.isfinite(g["d_ref"])                          # the fp32 oracle has the fp64 oracle's sets
        assert int((g["real"] & ~g["self_edge"]).sum()) > 100 and int((g["real"] & g["self_edge"]).sum()) == int(g["valid"].sum())
    if cid == "D":
        b = c.whole
        gone = ~b.residue_mask.bool()
        assert gone[0, D_MASKED_ROW] and gone[1, 36:].all() and int(gone.sum()) == 5 and (b.X[gone] == 0).all()
        assert float(b.X[~gone][:, 1].abs().max()) > 1000.0
    if cid == "P":
        far = [float(np.linalg.norm(b.X[0, :, 1].mean(0).numpy())) for b in c.parts]
        assert far[0] < 30 and far[1] > 2900 and far[2] > 2900
        assert float((c.parts[1].X[0, :, 1].mean(0) - c.parts[2].X[0, :, 1].mean(0)).norm()) > 3000      # on opposite sides


@pytest.mark.parametrize("inp", ["A", "B"])
def test_the_network_reference_is_usable_to_3000(inp):
    """Where d_ref itself exceeded 10 beta for the score or the sampled angles the case would say nothing."""
    for m in MOTIONS:
        cid = f"{inp}-{m}"
        ds, da = network_dref(cid, "score"), network_dref(cid, "sampling")
        print(f"{cid}: oracle fp32 vs fp64: score {ds:.2e}, hV {network_dref(cid, 'hV'):.2e}, ten ODE steps {da:.2e} rad")
        assert ds <= 10 * BETA["score"] and da <= 10 * BETA["sampling"]


@pytest.mark.parametrize("cid", GEOMETRY_CASES)
def test_few_residues_sit_at_a_hinge_threshold(cid):
    refs = geometry_ref(cid)
    n = sum(len(r["marginal"]) for r in refs)
    k = sum(int(r["marginal"].sum()) for r in refs)
    print(f"{cid}: {k} of {n} residues own an atom pair within {hinge_window(cid):.2e} A of its hinge threshold; oracle fp32 vs fp64: "
          f"atom14 {geometry_dref(cid, 'atom14'):.2e} A, clash {geometry_dref(cid, 'clash'):.2e}, gradient {geometry_dref(cid, 'grad'):.2e}")
    assert k <= 0.05 * n
    assert all(float(r["pr64"].max()) > 0 and float(r["g64"].abs().max()) > 0 for r in refs)
    assert all(bool((r["g64"] == 0).any()) for r in refs)           # exact zeros exist: angles that move no clashing atom


@pytest.mark.parametrize("cid", SASA_CASES)
def test_few_sasa_points_are_ambiguous(cid):
    c32, c64, amb, radius = sasa_ref(cid)
    frac = amb[radius > 0].mean()
    clear = ~amb.any(-1)
    print(f"{cid}: threshold {sasa_threshold(cid):.2e} A^2, ambiguous points {frac:.2e}, atoms whose words differ fp32/fp64 "
          f"{int((c32 != c64).any(-1).sum())}, outside ambiguous points {int((c32[clear] != c64[clear]).any(-1).sum())}")
    assert frac <= 0.01
    assert np.array_equal(c32[clear], c64[clear])


@pytest.mark.parametrize("motion", MOTIONS)
def test_obstacle_case_has_active_terms_and_few_marginal_rows(motion):
    from .test_obstacles_host import residue_clash_obst
    r = obstacle_ref(motion)
    share = residue_clash_obst(cast(r["part"], torch.float64), r["chi"].double(), r["ob"].double(), parts=True)[0]
    print(f"A+ob-{motion}: {len(r['ob'])} obstacle atoms, {int((share > 0).sum())} rows with an obstacle term, {int(r['marginal'].sum())} marginal; "
          f"restatement fp32 vs fp64: clash {obstacle_dref(motion, 'clash'):.2e}, gradient {obstacle_dref(motion, 'grad'):.2e}")
    assert int((share > 0).sum()) >= 3 and int(r["marginal"].sum()) <= 0.05 * len(r["marginal"])
    if parse(motion)[1]:
        assert float(r["ob"][:, :3].norm(dim=-1).min()) > parse(motion)[1] - 100.0             # the obstacles moved with the complex


@pytest.mark.parametrize("motion", MOTIONS)
def test_shell_restatement_agrees_with_fp64_on_decided_rows(motion):
    from .test_mutate_host import shell_numpy
    b = case(f"A-{motion}").parts[0]
    X, amask = b.X[0].numpy(), b.atom_mask[0].numpy()
    seeds = np.zeros(40, np.uint8)
    seeds[20] = 1
    for mode in ("ca", "atom"):
        for radius in (4.0, 8.0, 10.0):
            want, decided = shell_fp64(X, seeds, [0, 40], radius, mode, amask, 4 * ulp32(float(np.abs(X).max())))
            got = shell_numpy(X, seeds, [0, 40], radius, mode, amask)[0]
            assert decided.mean() >= 0.9 and np.array_equal(got[decided], want[decided]) and 0 < want.sum() < 40


def test_decoy_energies_reference_noise():
    for motion in MOTIONS:
        c = decoy_case(motion)
        print(f"A-{motion}: per-residue clash over four decoys, oracle fp32 vs fp64 {c.d_ref:.2e}")
        assert np.isfinite(c.d_ref) and c.d_ref > 0


def test_missing_atoms_and_masked_rows_sit_at_the_origin_far_from_the_complex():
    b = case("C-R1@3000").parts[0]
    table = torch.from_numpy(rc.atom14_mask)[b.residue_type]
    gone = (table > 0) & (b.atom_mask == 0)
    assert int(gone.sum()) >= 20 and (b.X[gone] == 0).all()
    assert int((b.residue_mask == 0).sum()) == 1
    assert float(b.X[b.atom_mask > 0].norm(dim=-1).min()) > 2900.0


# ---- the PDB columns -------------------------------------------------------------------------------------------------------------------
def _round_trip(p):
    from packppi_amd.pdb_io import parse_atom_records, to_pdb
    text = to_pdb(p)
    lines = [ln for ln in text.splitlines() if ln.startswith("ATOM")]
    assert all(len(ln) == 80 and ln[26:30] == "    " and ln[54:60] == "  1.00" for ln in lines)
    return lines, parse_atom_records(lines)


def _same_featurisation(p, q):
    a, b = protein_to_batch(p), protein_to_batch(q)
    for k in ("residue_type", "residue_mask", "atom_mask", "residue_index", "chain_indices", "SC_D_mask", "BB_D_mask",
              "chi_1pi_periodic_mask", "chi_2pi_periodic_mask"):
        assert torch.equal(a[k], b[k]), k


def test_pdb_round_trip_at_the_edge_of_the_columns():
    p = move(protein_of("A"), "R1@3000")
    ok = ~np.isnan(p["atom_positions"])
    lines, q = _round_trip(p)
    assert np.abs(q["atom_positions"] - p["atom_positions"])[ok].max() <= 5e-4
    _same_featurisation(p, q)
    # the widest numbers the columns hold: -999.999 and 9999.999, the three fields touching each other
    x = protein_of("A")["atom_positions"].copy()
    lo, hi = np.nanmin(x[..., 0]), np.nanmax(x[..., 1])
    x[..., 0] += -999.999 - lo
    x[..., 1] += 9999.999 - hi
    x[..., 2] += -999.999 - np.nanmin(x[..., 2])
    edge = dict(protein_of("A"), atom_positions=x)
    lines, q = _round_trip(edge)
    assert any(ln[30:38] == "-999.999" for ln in lines) and any(ln[38:46] == "9999.999" for ln in lines)
    assert any(ln[46:54] == "-999.999" for ln in lines)
    assert np.abs(q["atom_positions"] - x)[ok].max() <= 5e-4 + 0.5 * ulp32(9999.999)        # the parser keeps float32
    _same_featurisation(edge, q)


@pytest.mark.parametrize("axis,value", [(0, -1000.0), (1, 10000.0), (2, -999.9996), (0, 9999.9996), (1, -31000.0)])
def test_to_pdb_refuses_a_coordinate_beyond_the_columns(axis, value):
    """-1000 and below or 10000 and above (after rounding to three decimals) need nine characters: the record would shift every
    column behind it, and a reader would take other digits for the coordinate.  to_pdb raises instead."""
    from packppi_amd.pdb_io import to_pdb
    x = protein_of("A")["atom_positions"].copy()
    x[5, 1, axis] = value
    with pytest.raises(ValueError, match="8.3f"):
        to_pdb(dict(protein_of("A"), atom_positions=x))
    x[5, 1, axis] = np.sign(value) * 999.9994
    to_pdb(dict(protein_of("A"), atom_positions=x))
    # a missing atom's NaN is never written
    x[5, 6, axis] = np.nan
    mask = protein_of("A")["atom_mask"].copy()
    mask[5, 6] = 0
    assert "nan" not in to_pdb(dict(protein_of("A"), atom_positions=x, atom_mask=mask))


# ---- planar omegas ---------------------------------------------------------------------------------------------------------------------
def test_planar_omegas_are_decided_by_rounding():
    """Why no moved structure is compared with the unmoved one.  The generator's peptide bonds are exactly planar, and
    featurize.dihedrals_along computes sign(x) acos(c): for a planar omega x is rounding noise -- +, - or exactly 0 -- and when it is
    exactly 0 the angle comes out as 0 instead of +-pi, cos 1 instead of -1.  Every BB_D_sincos entry that changes by more than 1e-3
    under a motion must be such an entry: |BB_D| is 0 or pi (to the acos of 1 - 2^-23, 5e-4) in both copies, it is the pre-omega, its
    mask is 1, and the change is the 2.0 of cos 0 - cos pi.  Anything else would be a featurisation bug."""
    base = protein_to_batch(protein_of("A"))
    total = 0
    for motion in MOTIONS[1:]:
        b = protein_to_batch(move(protein_of("A"), motion))
        assert torch.equal(b.BB_D_mask, base.BB_D_mask) and torch.equal(b.SC_D_mask, base.SC_D_mask)
        changed = (b.BB_D_sincos - base.BB_D_sincos).abs() > 1e-3                             # [1, L, 3, 2]
        where = changed.any(-1)
        for bb in (b, base):
            a = bb.BB_D[where].abs()
            assert ((a == 0) | ((a - np.pi).abs() < 5e-4)).all(), motion
        # the sign-decided case is what happened: exactly one copy has the angle exactly 0, the other has +-pi
        zero0, zero1 = base.BB_D[where] == 0, b.BB_D[where] == 0
        assert (zero0 ^ zero1).all(), motion
        assert not where[..., 1:].any() and (base.BB_D_mask[where] == 1).all()                # pre-omega only, and it counts
        assert not changed[..., 0].any()                                                      # the sine does not notice
        assert ((b.BB_D_sincos - base.BB_D_sincos)[..., 1][where].abs() - 2.0).abs().max() < 1e-6 if where.any() else True
        # every other entry moves by rounding only
        assert (b.BB_D_sincos - base.BB_D_sincos)[~changed].abs().max() < 1e-3
        total += int(where.sum())
        print(f"{motion}: {int(where.sum())} of {int(base.BB_D_mask.sum())} backbone angles flip between 0 and pi")
    assert total > 0
    # and the side chains: chi angles are not planar, they move by the rounding of the coordinates
    far = protein_to_batch(move(protein_of("A"), "R1@0"))
    assert wrapped_absdiff(far.SC_D, base.SC_D).max() < 1e-4
