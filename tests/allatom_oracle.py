"""Brute-force NumPy oracle of pp_hydrogens / pp_clashscore, float64 or float32.

Its chemistry is written out here by atom name and shares nothing with ``packppi_amd.constants`` but the atom14 slot order
(``atom14_names``, data): every hydrogen with its parent, class and the atoms it is built from, every side-chain bond, the radii.
The float32 form restates the kernels' operation order (no root, no fused multiply-add), so the integer outputs of pp_clashscore
can be compared as bytes; hydrogen positions are compared with the float64 form within a tolerance.
"""
import numpy as np

from packppi_amd import constants as rc

S, HMAX = 27, 13
BOND_L = {"C": 1.09, "N": 1.01, "O": 0.96, "S": 1.34}

# (parent, class, atoms, hydrogen names).  P1bb / P1 / T1 / T2: the parent's heavy neighbours ("-C": the previous residue's C);
# T3 / P2 / R1: (a, b) of the dihedral H-parent-a-b.
_BB = [("N", "P1bb", ("CA", "-C"), ("H",)), ("CA", "T1", ("N", "C", "CB"), ("HA",))]
_T2 = lambda p, a, b: (p, "T2", (a, b), ("H" + p[1:] + "2", "H" + p[1:] + "3"))
_AR = lambda p, a, b: (p, "P1", (a, b), ("H" + p[1:],))
_ME = lambda p, a, b: (p, "T3", (a, b), ("H" + p[1:] + "1", "H" + p[1:] + "2", "H" + p[1:] + "3"))
HYDROGENS = {
    "ALA": _BB + [_ME("CB", "CA", "N")],
    "ARG": _BB + [_T2("CB", "CA", "CG"), _T2("CG", "CB", "CD"), _T2("CD", "CG", "NE"), ("NE", "P1", ("CD", "CZ"), ("HE",)),
                  ("NH1", "P2", ("CZ", "NE"), ("HH11", "HH12")), ("NH2", "P2", ("CZ", "NE"), ("HH21", "HH22"))],
    "ASN": _BB + [_T2("CB", "CA", "CG"), ("ND2", "P2", ("CG", "CB"), ("HD21", "HD22"))],
    "ASP": _BB + [_T2("CB", "CA", "CG")],
    "CYS": _BB + [_T2("CB", "CA", "SG"), ("SG", "R1", ("CB", "CA"), ("HG",))],
    "GLN": _BB + [_T2("CB", "CA", "CG"), _T2("CG", "CB", "CD"), ("NE2", "P2", ("CD", "CG"), ("HE21", "HE22"))],
    "GLU": _BB + [_T2("CB", "CA", "CG"), _T2("CG", "CB", "CD")],
    "GLY": [_BB[0], ("CA", "T2", ("N", "C"), ("HA2", "HA3"))],
    "HIS": _BB + [_T2("CB", "CA", "CG"), _AR("CD2", "CG", "NE2"), _AR("CE1", "ND1", "NE2"), ("NE2", "P1", ("CD2", "CE1"), ("HE2",))],
    "ILE": _BB + [("CB", "T1", ("CA", "CG1", "CG2"), ("HB",)), _T2("CG1", "CB", "CD1"), _ME("CG2", "CB", "CA"), _ME("CD1", "CG1", "CB")],
    "LEU": _BB + [_T2("CB", "CA", "CG"), ("CG", "T1", ("CB", "CD1", "CD2"), ("HG",)), _ME("CD1", "CG", "CB"), _ME("CD2", "CG", "CB")],
    "LYS": _BB + [_T2("CB", "CA", "CG"), _T2("CG", "CB", "CD"), _T2("CD", "CG", "CE"), _T2("CE", "CD", "NZ"), _ME("NZ", "CE", "CD")],
    "MET": _BB + [_T2("CB", "CA", "CG"), _T2("CG", "CB", "SD"), _ME("CE", "SD", "CG")],
    "PHE": _BB + [_T2("CB", "CA", "CG"), _AR("CD1", "CG", "CE1"), _AR("CD2", "CG", "CE2"), _AR("CE1", "CD1", "CZ"),
                  _AR("CE2", "CD2", "CZ"), _AR("CZ", "CE1", "CE2")],
    "PRO": [_BB[1], _T2("CB", "CA", "CG"), _T2("CG", "CB", "CD"), _T2("CD", "N", "CG")],
    "SER": _BB + [_T2("CB", "CA", "OG"), ("OG", "R1", ("CB", "CA"), ("HG",))],
    "THR": _BB + [("CB", "T1", ("CA", "OG1", "CG2"), ("HB",)), ("OG1", "R1", ("CB", "CA"), ("HG1",)), _ME("CG2", "CB", "CA")],
    "TRP": _BB + [_T2("CB", "CA", "CG"), _AR("CD1", "CG", "NE1"), ("NE1", "P1", ("CD1", "CE2"), ("HE1",)), _AR("CE3", "CD2", "CZ3"),
                  _AR("CZ2", "CE2", "CH2"), _AR("CZ3", "CE3", "CH2"), _AR("CH2", "CZ2", "CZ3")],
    "TYR": _BB + [_T2("CB", "CA", "CG"), _AR("CD1", "CG", "CE1"), _AR("CD2", "CG", "CE2"), _AR("CE1", "CD1", "CZ"),
                  _AR("CE2", "CD2", "CZ"), ("OH", "R1", ("CZ", "CE1"), ("HH",))],
    "VAL": _BB + [("CB", "T1", ("CA", "CG1", "CG2"), ("HB",)), _ME("CG1", "CB", "CA"), _ME("CG2", "CB", "CA")],
    "UNK": [],
}
SIDE_BONDS = {
    "ALA": "CA-CB", "ARG": "CA-CB CB-CG CG-CD CD-NE NE-CZ CZ-NH1 CZ-NH2", "ASN": "CA-CB CB-CG CG-OD1 CG-ND2",
    "ASP": "CA-CB CB-CG CG-OD1 CG-OD2", "CYS": "CA-CB CB-SG", "GLN": "CA-CB CB-CG CG-CD CD-OE1 CD-NE2",
    "GLU": "CA-CB CB-CG CG-CD CD-OE1 CD-OE2", "GLY": "", "HIS": "CA-CB CB-CG CG-ND1 CG-CD2 ND1-CE1 CD2-NE2 CE1-NE2",
    "ILE": "CA-CB CB-CG1 CB-CG2 CG1-CD1", "LEU": "CA-CB CB-CG CG-CD1 CG-CD2", "LYS": "CA-CB CB-CG CG-CD CD-CE CE-NZ",
    "MET": "CA-CB CB-CG CG-SD SD-CE", "PHE": "CA-CB CB-CG CG-CD1 CG-CD2 CD1-CE1 CD2-CE2 CE1-CZ CE2-CZ",
    "PRO": "CA-CB CB-CG CG-CD CD-N", "SER": "CA-CB CB-OG", "THR": "CA-CB CB-OG1 CB-CG2",
    "TRP": "CA-CB CB-CG CG-CD1 CG-CD2 CD1-NE1 NE1-CE2 CD2-CE2 CD2-CE3 CE2-CZ2 CE3-CZ3 CZ2-CH2 CZ3-CH2",
    "TYR": "CA-CB CB-CG CG-CD1 CG-CD2 CD1-CE1 CD2-CE2 CE1-CZ CE2-CZ CZ-OH", "VAL": "CA-CB CB-CG1 CB-CG2", "UNK": "",
}
ACCEPTORS = {"ASP": ("OD1", "OD2"), "GLU": ("OE1", "OE2"), "ASN": ("OD1",), "GLN": ("OE1",), "HIS": ("ND1", "NE2"), "SER": ("OG",),
             "THR": ("OG1",), "TYR": ("OH",)}
CARBONYL = {"ASP": "CG", "GLU": "CD", "ASN": "CG", "GLN": "CD"}
AROMATIC_RES = ("HIS", "PHE", "TYR", "TRP")
ROTATABLE = {("SER", "HG"), ("THR", "HG1"), ("TYR", "HH"), ("CYS", "HG"), ("LYS", "HZ1"), ("LYS", "HZ2"), ("LYS", "HZ3")}
ANGLES = {"T3": (109.5, (60.0, 180.0, 300.0)), "P2": (120.0, (0.0, 180.0)), "R1": (109.5, (180.0,))}


def tables():
    """Per residue type (the order of ``constants.resnames``): ``names`` [21] lists of 27 names ("" = empty), ``hyd`` [21] lists of
    (class, parent slot, atom slots (-2 = the previous C), q = which of the parent's hydrogens, L), ``sep`` uint8 [21, 27, 27],
    ``radius`` f32 [21, 27], ``acls`` u8 [21, 27], ``rot`` bool [21, 27]."""
    names, hyd = [], []
    sep = np.full((21, S, S), 9, np.uint8)
    radius, acls, rot = np.zeros((21, S), np.float32), np.zeros((21, S), np.uint8), np.zeros((21, S), bool)
    for t, rn in enumerate(rc.resnames):
        a14 = list(rc.atom14_names[t])
        slot = {n: i for i, n in enumerate(a14) if n}
        slot["-C"] = -2
        hs, hn = [], []
        for parent, cls, atoms, hnames in sorted(HYDROGENS[rn], key=lambda e: slot[e[0]]):
            at = sorted(slot[a] for a in atoms if a != "-C") + ([-2] if "-C" in atoms else []) if cls in ("T2",) else [slot[a] for a in atoms]
            for q, nm in enumerate(hnames):
                hs.append((cls, slot[parent], at, q, BOND_L[parent[0]]))
                hn.append(nm)
        assert len(hn) <= HMAX
        names.append(a14 + hn + [""] * (HMAX - len(hn)))
        hyd.append(hs)
        bonds = [("N", "CA"), ("CA", "C"), ("C", "O")] if rn != "UNK" else []
        bonds += [tuple(b.split("-")) for b in SIDE_BONDS[rn].split()]
        adj = [set() for _ in range(S)]
        for a, b in bonds:
            adj[slot[a]].add(slot[b])
            adj[slot[b]].add(slot[a])
        for k, h in enumerate(hs):
            adj[14 + k].add(h[1])
            adj[h[1]].add(14 + k)
        for s0 in range(S):
            dist = {s0: 0}
            front = [s0]
            while front:
                nxt = []
                for u in front:
                    for v in adj[u]:
                        if v not in dist:
                            dist[v] = dist[u] + 1
                            nxt.append(v)
                front = nxt
            for v, d in dist.items():
                sep[t, s0, v] = min(d, 9)
        for s0, nm in enumerate(names[t]):
            if not nm:
                continue
            if s0 < 14:
                el = nm[0]
                radius[t, s0] = {"C": 1.75, "N": 1.55, "O": 1.40, "S": 1.80}[el]
                if nm == "C" or CARBONYL.get(rn) == nm:
                    radius[t, s0] = 1.65
                acls[t, s0] = (2 if (nm == "O" or nm in ACCEPTORS.get(rn, ())) else 0) | (8 if s0 < 4 else 0)
            else:
                pn = a14[hs[s0 - 14][1]]
                polar = pn[0] in "NOS"
                arom = pn[0] == "C" and (rn in AROMATIC_RES and pn not in ("CA", "CB")) or (rn, pn) in (
                    ("ARG", "CZ"), ("ASN", "CG"), ("ASP", "CG"), ("GLN", "CD"), ("GLU", "CD"))
                radius[t, s0] = 1.00 if (polar or arom) else 1.17
                acls[t, s0] = 4 | (1 if polar else 0) | (8 if pn in ("N", "CA") else 0)
                rot[t, s0] = (rn, nm) in ROTATABLE
    return dict(names=names, hyd=hyd, sep=sep, radius=radius, acls=acls, rot=rot)


_TABLES = None


def get_tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = tables()
    return _TABLES


def _unit(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def link_prev_of(X, amask, chain, seg_off, dtype=np.float64):
    X = np.asarray(X, dtype).reshape(-1, 14, 3)
    amask, chain = np.asarray(amask).reshape(-1, 14), np.asarray(chain).reshape(-1)
    N = X.shape[0]
    lp = np.zeros(N, np.uint8)
    firsts = set(int(o) for o in seg_off[:-1])
    for n in range(1, N):
        if n in firsts or chain[n] != chain[n - 1] or amask[n - 1, 2] == 0 or amask[n, 0] == 0:
            continue
        d = X[n - 1, 2] - X[n, 0]
        with np.errstate(all="ignore"):
            lp[n] = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) <= dtype(4.0)
    return lp


def hydrogens(X, amask, rtype, chain, seg_off, link=None, dtype=np.float64):
    """(hxyz [N, 13, 3] dtype, hmask uint8 [N, 13], link_prev uint8 [N]) by the definition of DESIGN.md section 29."""
    tb = get_tables()
    X = np.asarray(X, dtype).reshape(-1, 14, 3)
    amask, rtype = np.asarray(amask).reshape(-1, 14), np.asarray(rtype).reshape(-1)
    N = X.shape[0]
    lp = link_prev_of(X, amask, chain, seg_off, dtype)
    hxyz, hmask = np.zeros((N, HMAX, 3), dtype), np.zeros((N, HMAX), np.uint8)
    f = lambda deg, fn: dtype(np.float32(fn(np.deg2rad(deg))))       # the kernel's constants: rounded to float once
    for n in range(N):
        rn = rc.resnames[int(rtype[n])]
        for k, (cls, p, at, q, L) in enumerate(tb["hyd"][int(rtype[n])]):
            ok = amask[n, p] != 0
            pos = lambda s: X[n - 1, 2] if s == -2 else X[n, s]
            for s in at:
                ok = ok and (bool(lp[n]) if s == -2 else amask[n, s] != 0)
            if cls == "R1" and rn == "CYS" and link is not None and link[n] >= 0:
                ok = False
            if not ok:
                continue
            P, L = X[n, p], dtype(np.float32(L))
            with np.errstate(all="ignore"):
                if cls in ("T1", "P1", "P1bb"):
                    s = sum(_unit(pos(a) - P) for a in at)
                    h = P - L * _unit(s)
                elif cls == "T2":
                    u1, u2 = _unit(pos(at[0]) - P), _unit(pos(at[1]) - P)
                    b, nn = -_unit(u1 + u2), _unit(np.cross(u1, u2))
                    sgn = dtype(1.0) if q == 0 else dtype(-1.0)
                    h = P + L * (f(54.75, np.cos) * b + sgn * f(54.75, np.sin) * nn)
                else:
                    theta, phis = ANGLES[cls]
                    qa, qb = pos(at[0]) - P, pos(at[1]) - P
                    e = _unit(-qa)
                    nn = _unit(np.cross(qa - qb, e))
                    m = np.cross(nn, e)
                    h = P + (-(L * f(theta, np.cos)) * e + (L * f(theta, np.sin)) * f(phis[q], np.cos) * m
                             + (L * f(theta, np.sin)) * f(phis[q], np.sin) * nn)
            if np.all(np.isfinite(h)) and np.all(np.abs(h.astype(np.float32)) <= np.finfo(np.float32).max):
                hxyz[n, k], hmask[n, k] = h, 1
    return hxyz, hmask, lp


def default_radius(rtype, amask, rotatable="skip"):
    tb = get_tables()
    rtype = np.asarray(rtype).reshape(-1)
    r = tb["radius"][rtype].copy()
    r[:, :14] *= (np.asarray(amask).reshape(-1, 14) != 0)
    if rotatable == "skip":
        r[tb["rot"][rtype]] = 0
    return r


def clash(X, hxyz, hmask, radius, rtype, chain, seg_off, link_prev, link=None, obst=None, obst_off=None, obst_polar=None, cut=0.4,
          hb_allow=0.6, dtype=np.float32, acls=None):
    """Brute force over every pair of counted atoms of a segment.  Returns a dict: ``n_clash`` [N, 27, 2], ``partners`` [N, 27, 4],
    ``res`` [N, 4], ``seg`` [n_seg, 8] (int32, the layout of pp_clashscore), ``pairs``: the serious overlaps as (row, slot, row,
    slot), lower (row, slot) first, and ``near``: (row, slot, row, slot, t - d in A) of every non-excluded pair of counted atoms
    within 0.5 A of the threshold -- what the float32 / float64 comparison needs."""
    tb = get_tables()
    rtype, chain = np.asarray(rtype).reshape(-1), np.asarray(chain).reshape(-1)
    N = rtype.shape[0]
    A = np.concatenate([np.asarray(X, dtype).reshape(N, 14, 3), np.asarray(hxyz, dtype).reshape(N, HMAX, 3)], 1)
    r = np.asarray(radius, dtype).reshape(N, S).copy()
    with np.errstate(invalid="ignore"):
        r[~(r > 0)] = 0
    r[:, 14:][np.asarray(hmask).reshape(N, HMAX) == 0] = 0
    cls = (tb["acls"][rtype] if acls is None else np.asarray(acls).reshape(N, S)).astype(np.int32)
    sep = tb["sep"][rtype].astype(np.int32)                   # [N, 27, 27]
    cut, hb_allow = dtype(cut), dtype(hb_allow)
    n_clash = np.zeros((N, S, 2), np.int32)
    partners = -np.ones((N, S, 4), np.int32)
    res = np.zeros((N, 4), np.int32)
    n_seg = len(seg_off) - 1
    seg = np.zeros((n_seg, 8), np.int32)
    pairs, near = [], []
    hyd, bb = (cls & 4) != 0, (cls & 8) != 0
    for s in range(n_seg):
        lo, hi = int(seg_off[s]), int(seg_off[s + 1])
        rows = np.arange(lo, hi)
        for i in rows:
            res[i, 3] = int((r[i] > 0).sum())
            seg[s, 0] += res[i, 3]
            # [27 own, rows, 27]
            with np.errstate(all="ignore"):
                d = A[lo:hi][None, :, :, :] - A[i][:, None, None, :]
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                t = (r[i][:, None, None] + r[lo:hi][None]) - cut
                hbp = (((cls[i] & 1) != 0)[:, None, None] & ((cls[lo:hi] & 2) != 0)[None]) | \
                      (((cls[i] & 2) != 0)[:, None, None] & ((cls[lo:hi] & 1) != 0)[None])
                t = np.where(hbp, t - hb_allow, t)
                hit = (t > 0) & (d2 <= t * t)
            hit &= (r[i] > 0)[:, None, None] & (r[lo:hi] > 0)[None]
            sp = np.full((S, hi - lo, S), 99, np.int32)
            sp[:, i - lo, :] = sep[i]
            if i + 1 < hi and link_prev[i + 1]:
                sp[:, i + 1 - lo, :] = np.minimum(sp[:, i + 1 - lo, :], sep[i][:, 2][:, None] + 1 + sep[i + 1][0][None, :])
            if i - 1 >= lo and link_prev[i]:
                sp[:, i - 1 - lo, :] = np.minimum(sp[:, i - 1 - lo, :], sep[i][:, 0][:, None] + 1 + sep[i - 1][2][None, :])
            if link is not None:
                j = int(link[i])
                if lo <= j < hi and j != i and int(link[j]) == i:
                    sp[:, j - lo, :] = np.minimum(sp[:, j - lo, :], sep[i][:, 5][:, None] + 1 + sep[j][5][None, :])
            anyh = hyd[i][:, None, None] | hyd[lo:hi][None]
            allowed = sp > np.where(anyh, 4, 3)
            allowed[np.arange(S), i - lo, np.arange(S)] = False
            hit &= allowed
            same = (chain[lo:hi] == chain[i])[None, :, None]
            for x, jr, y in zip(*np.nonzero(hit)):
                j = lo + int(jr)
                if n_clash[i, x, 0] < 4:
                    partners[i, x, n_clash[i, x, 0]] = int(jr) * S + int(y)
                n_clash[i, x, 0] += 1
                up = j > i or (j == i and y > x)
                if j == i:
                    res[i, 0] += 1 if up else 0
                elif chain[j] == chain[i]:
                    res[i, 0] += 1
                else:
                    res[i, 1] += 1
                if up:
                    pairs.append((int(i), int(x), j, int(y)))
                    seg[s, 1] += 1
                    seg[s, 2] += chain[j] != chain[i]
                    seg[s, 3] += bool(hyd[i, x] or hyd[j, y])
                    both = bool(bb[i, x] and bb[j, y])
                    seg[s, 4] += not both
                    seg[s, 5] += j == i
                    seg[s, 7] += both
            # every allowed pair near the threshold, from its lower end: for the float32 / float64 comparison
            with np.errstate(all="ignore"):
                ov = t - np.sqrt(d2)
            cand = allowed & (r[i] > 0)[:, None, None] & (r[lo:hi] > 0)[None] & (np.abs(ov) <= 0.5)
            for x, jr, y in zip(*np.nonzero(cand)):
                j = lo + int(jr)
                if j > i or (j == i and y > x):
                    near.append((int(i), int(x), j, int(y), float(ov[x, jr, y])))
            if obst is not None and obst_off is not None:
                o0, o1 = int(obst_off[s]), int(obst_off[s + 1])
                if o1 > o0:
                    O = np.asarray(obst, dtype).reshape(-1, 4)[o0:o1]
                    pol = np.zeros(o1 - o0, bool) if obst_polar is None else (np.asarray(obst_polar).reshape(-1)[o0:o1] != 0)
                    with np.errstate(all="ignore"):
                        d = O[None, :, :3] - A[i][:, None, :]
                        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                        t = (r[i][:, None] + O[None, :, 3]) - cut
                        t = np.where(((cls[i] & 1) != 0)[:, None] & pol[None], t - hb_allow, t)
                        oh = (t > 0) & (d2 <= t * t) & (r[i] > 0)[:, None] & (O[:, 3] > 0)[None]
                    n_clash[i, :, 1] = oh.sum(1)
                    res[i, 2] = int(oh.sum())
                    seg[s, 6] += res[i, 2]
    return dict(n_clash=n_clash, partners=partners, res=res, seg=seg, pairs=pairs, near=near)


def clashscore(seg, obstacles=False):
    seg = np.asarray(seg)
    return 1000.0 * (seg[:, 1] + (seg[:, 6] if obstacles else 0)) / np.maximum(seg[:, 0], 1)
