"""Polar contacts (pp_polar) restated with NumPy, brute force over all polar atoms of a segment.  Not a test
module: tests/test_polar_host.py and tests/test_polar_gpu.py import it.

The class and antecedent tables are built here from literal name lists of this file, not from ``constants.polar_*``: a wrong table
in the package is caught by the comparison.  Run in float32 -- every operation rounded on its own, in the order of
include/packppi_hip.h -- it is what the device is compared with, word for word; run in float64 it is the arbiter, and the pairs at
which the two may differ are the AMBIGUOUS ones: a comparison within 1e-4 of its threshold in float64.

The adjacency rule of step 6 is the one the kernel states: ROWS that differ by one (not residue numbers)."""
import functools
import os

import numpy as np

from packppi_amd import constants as rc

CAP = 4
DON, ACC, CAT, ANI = 1, 2, 4, 8
SIDE_DONORS = ["ARG NE", "ARG NH1", "ARG NH2", "ASN ND2", "GLN NE2", "HIS ND1", "HIS NE2", "LYS NZ", "SER OG", "THR OG1", "TYR OH",
               "TRP NE1"]
SIDE_ACCEPTORS = ["ASP OD1", "ASP OD2", "GLU OE1", "GLU OE2", "ASN OD1", "GLN OE1", "HIS ND1", "HIS NE2", "SER OG", "THR OG1",
                  "TYR OH"]
CATIONS = ["LYS NZ", "ARG NE", "ARG NH1", "ARG NH2"]
ANIONS = ["ASP OD1", "ASP OD2", "GLU OE1", "GLU OE2"]
# the heavy atoms bonded to each polar atom within its residue
BONDED = {"N": ["CA"], "O": ["C"],
          "ARG NE": ["CD", "CZ"], "ARG NH1": ["CZ"], "ARG NH2": ["CZ"], "ASN OD1": ["CG"], "ASN ND2": ["CG"], "ASP OD1": ["CG"],
          "ASP OD2": ["CG"], "GLN OE1": ["CD"], "GLN NE2": ["CD"], "GLU OE1": ["CD"], "GLU OE2": ["CD"], "HIS ND1": ["CG", "CE1"],
          "HIS NE2": ["CD2", "CE1"], "LYS NZ": ["CE"], "SER OG": ["CB"], "THR OG1": ["CB"], "TRP NE1": ["CD1", "CE2"], "TYR OH": ["CZ"]}


def tables():
    """(cls uint8 [21, 14], ante int8 [21, 14, 2]) from the lists above and the slot names of the atom14 layout."""
    cls = np.zeros((21, 14), np.uint8)
    ante = -np.ones((21, 14, 2), np.int8)
    for t in range(20):
        rn, names = rc.resnames[t], rc.atom14_names[t]
        for s, nm in enumerate(names):
            if not nm:
                continue
            full = f"{rn} {nm}"
            c = 0
            if s == 0:
                assert nm == "N"
                c = 0 if rn == "PRO" else DON
            elif s == 3:
                assert nm == "O"
                c = ACC
            else:
                c = (DON * (full in SIDE_DONORS)) | (ACC * (full in SIDE_ACCEPTORS)) | (CAT * (full in CATIONS)) | (ANI * (full in ANIONS))
            cls[t, s] = c
            if c:
                for k, a in enumerate(BONDED[nm if s in (0, 3) else full]):
                    ante[t, s, k] = names.index(a)
    return cls, ante


def classify(residue_type, atom_mask):
    """(cls [N, 14], ante [N, 14, 2]) of the rows: the tables gathered by type, the class zeroed where the atom or one of its
    antecedents is absent."""
    tc, ta = tables()
    rt = np.asarray(residue_type).reshape(-1).astype(np.int64)
    am = np.asarray(atom_mask).reshape(-1, 14) != 0
    cls, ante = tc[rt].copy(), ta[rt].copy()
    ok = am.copy()
    for k in range(2):
        a = ante[..., k].astype(np.int64)
        ok &= (a < 0) | np.take_along_axis(am, np.maximum(a, 0), 1)
    return (cls * ok).astype(np.uint8), ante


def arrays(batch):
    """(X [N, 14, 3] float32, cls, ante, chain [N], segment table) of a batch: padded [B, L] (segments 0, L, 2L ...) or packed."""
    X = np.asarray(batch["X"], dtype=np.float32).reshape(-1, 14, 3)
    cls, ante = classify(batch["residue_type"], batch["atom_mask"])
    chain = np.asarray(batch["chain_indices"]).reshape(-1).astype(np.int64)
    offs = batch.get("seg_offsets_host")
    if offs is None:
        B, L = np.asarray(batch["residue_type"]).shape
        offs = [s * L for s in range(B + 1)]
    return X, cls, ante, chain, [int(x) for x in offs]


def _dot(ax, ay, az, bx, by, bz):
    return ((ax * bx) + (ay * by)) + (az * bz)


def segment(X, cls, ante, chain, lo, hi, dtype=np.float32, hb_max=3.5, sb_max=4.0, obst=None):
    """One segment (rows lo .. hi - 1), brute force.  ``obst``: (xyz [m, 3], polar [m]) of the segment's obstacle range.  Returns a
    dict: ``atoms`` (row - lo, slot) of the polar atoms in code order, the pair matrices ``hb`` and ``salt`` (atom x atom), ``cand``
    (pairs that can bond or bridge, in different rows, within 4.0 A) and ``amb`` (candidates with a comparison within 1e-4 of its
    threshold), ``n_ob`` per atom."""
    f = dtype
    with np.errstate(invalid="ignore", over="ignore"):
        c_all = cls[lo:hi]
        r, s = np.nonzero(c_all != 0)                    # row-major: ascending code
        c = c_all[r, s].astype(np.int64)
        Xs = X[lo:hi].astype(f)
        P = Xs[r, s]
        a = ante[lo:hi][r, s].astype(np.int64)
        a1, a2 = a[:, 0], a[:, 1]
        one = np.where(a1 >= 0, a1, a2)
        both = (a1 >= 0) & (a2 >= 0)
        base = Xs[r, np.maximum(one, 0)]
        mid = (Xs[r, np.maximum(a1, 0)] + Xs[r, np.maximum(a2, 0)]) * f(0.5)
        base = np.where(both[:, None], mid, base)
        u = np.where(((a1 >= 0) | (a2 >= 0))[:, None], base - P, f(0))
        hb2, sb2 = f(np.float32(hb_max)) * f(np.float32(hb_max)), f(np.float32(sb_max)) * f(np.float32(sb_max))
        d = P[None, :, :] - P[:, None, :]                # d[x, y] = q - p
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        d2 = _dot(dx, dy, dz, dx, dy, dz)
        sx = _dot(u[:, None, 0], u[:, None, 1], u[:, None, 2], dx, dy, dz)
        sy = sx.T                                        # u_y . (p - q), and p - q is d[y, x]
        don, acc, cat, ani = (c & DON) > 0, (c & ACC) > 0, (c & CAT) > 0, (c & ANI) > 0
        da = (don[:, None] & acc[None]) | (acc[:, None] & don[None])
        ca = (cat[:, None] & ani[None]) | (ani[:, None] & cat[None])
        diff = r[:, None] != r[None]
        bb = (s == 0) | (s == 3)
        same = chain[lo + r][:, None] == chain[lo + r][None]
        skip = bb[:, None] & bb[None] & (np.abs(r[:, None] - r[None]) == 1) & same
        hb = da & diff & ~skip & (d2 <= hb2) & (sx <= 0) & (sy <= 0)
        salt = ca & diff & (d2 <= sb2)
        cand = (da | ca) & diff & (d2 <= f(16.0))
        near = lambda v, t: np.abs(v.astype(np.float64) - float(t)) < 1e-4
        amb = cand & (near(d2, hb2) | near(d2, sb2) | near(sx, 0) | near(sy, 0))
        n_ob = np.zeros(len(r), np.int64)
        if obst is not None and len(r):
            oxyz, opol = np.asarray(obst[0]).astype(f).reshape(-1, 3), np.asarray(obst[1]).reshape(-1) != 0
            e = oxyz[None] - P[:, None]
            n_ob = ((_dot(e[..., 0], e[..., 1], e[..., 2], e[..., 0], e[..., 1], e[..., 2]) <= hb2) & opol[None]).sum(1)
    return dict(atoms=(r, s), hb=hb, salt=salt, cand=cand, amb=amb, n_ob=n_ob, same=same)


def contacts(X, cls, ante, chain, offs, dtype=np.float32, hb_max=3.5, sb_max=4.0, obst=None):
    """The four arrays of pp_polar over all segments, plus ``segments`` (the dicts of ``segment``).  ``obst``: (xyz [M, 3], polar
    [M], [(first, count)] per segment) or None."""
    N = X.shape[0]
    partners = -np.ones((N, 14, CAP), np.int32)
    n_partners = np.zeros((N, 14, 2), np.int32)
    res = np.zeros((N, 8), np.int32)
    seg = np.zeros((len(offs) - 1, 8), np.int32)
    segs = []
    for k, (lo, hi) in enumerate(zip(offs[:-1], offs[1:])):
        ob = None
        if obst is not None:
            first, cnt = obst[2][k]
            ob = (np.asarray(obst[0])[first:first + cnt], np.asarray(obst[1])[first:first + cnt])
        g = segment(X, cls, ante, chain, lo, hi, dtype, hb_max, sb_max, ob)
        segs.append(g)
        r, s = g["atoms"]
        hb, same = g["hb"], g["same"]
        code = r * 14 + s
        side, back = s >= 4, (s == 0) | (s == 3)
        nhb = hb.sum(1)
        for x in range(len(r)):
            n_partners[lo + r[x], s[x]] = (nhb[x], g["n_ob"][x])
            lst = code[hb[x]][:CAP]
            partners[lo + r[x], s[x], :len(lst)] = lst
        np.add.at(res[lo:hi, 0], r[side], (hb & same)[side].sum(1))
        np.add.at(res[lo:hi, 1], r[side], (hb & ~same)[side].sum(1))
        np.add.at(res[lo:hi, 2], r[back], (hb & same)[back].sum(1))
        np.add.at(res[lo:hi, 3], r[back], (hb & ~same)[back].sum(1))
        xs, ys = np.nonzero(g["salt"])
        rows = sorted({(int(r[x]), int(r[y])) for x, y in zip(xs, ys)})          # ordered row pairs, both directions
        for a, b in rows:
            res[lo + a, 4 if chain[lo + a] == chain[lo + b] else 5] += 1
        np.add.at(res[lo:hi, 6], r, g["n_ob"])
        np.add.at(res[lo:hi, 7], r, ((nhb == 0) & (g["n_ob"] == 0)).astype(np.int64))
        sc = side[:, None] | side[None]
        seg[k] = (hb.sum() // 2, (hb & ~same).sum() // 2, (hb & sc).sum() // 2, (hb & sc & ~same).sum() // 2,
                  len(rows) // 2, sum(chain[lo + a] != chain[lo + b] for a, b in rows) // 2, g["n_ob"].sum(), res[lo:hi, 7].sum())
    return dict(partners=partners, n_partners=n_partners, res=res, seg=seg, segments=segs)


def of_batch(batch, dtype=np.float32, **kw):
    X, cls, ante, chain, offs = arrays(batch)
    return contacts(X, cls, ante, chain, offs, dtype, **kw)


def compare_precisions(X, cls, ante, chain, offs, **kw):
    """(pairs at which the float32 and float64 restatements differ outside the ambiguous pairs, ambiguous pairs, candidate pairs) --
    unordered pairs, summed over the segments."""
    bad = n_amb = n_cand = 0
    for lo, hi in zip(offs[:-1], offs[1:]):
        a = segment(X, cls, ante, chain, lo, hi, np.float32, **kw)
        b = segment(X, cls, ante, chain, lo, hi, np.float64, **kw)
        amb = b["amb"] | b["amb"].T
        differ = (a["hb"] != b["hb"]) | (a["salt"] != b["salt"])
        bad += int((differ & ~amb).sum()) // 2
        n_amb += int(amb.sum()) // 2
        n_cand += int(b["cand"].sum()) // 2
    return bad, n_amb, n_cand


# ---- the cases both test files share (built once) --------------------------------------------------------------------------------------------
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def protein(name):
    from packppi_amd import synth
    if name in ("1BRS", "2FTL"):
        z = np.load(os.path.join(GOLD, f"g0_protein_{name}.npz"))
        return {k[5:]: z[k] for k in z.files if k.startswith("prot.")}
    if name == "damaged64":
        return synth.drop_atoms(synth.make_complex(64, 11), 64)
    spec = {"c24": (24, 5), "c64": (64, 11), "c97": (97, 267), "c65": (65, 9), "three_chains": (45, 3, 3), "c40": (40, 2),
            "c36": (36, 3)}[name]
    return synth.make_complex(*spec)


@functools.lru_cache(maxsize=None)
def batch(name):
    from packppi_amd.featurize import protein_to_batch
    return protein_to_batch(protein(name))


@functools.lru_cache(maxsize=None)
def reference(name):
    return of_batch(batch(name))


SINGLES = ("c24", "c64", "c97", "c65", "three_chains", "1BRS", "2FTL", "damaged64")
