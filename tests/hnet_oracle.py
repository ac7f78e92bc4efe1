"""Brute-force NumPy oracle of pp_hnet_optimize, float64 or float32.

No row filter and no partner cap.  The movers are typed out here by name (which residues, which atoms move, the rotor states in
degrees); radii, classes, bond separations and the hydrogen geometry are those of tests/allatom_oracle.py, which types them out as
well.  The float32 form restates the kernel's operation order, so its integers can be compared with the device's as bytes.
"""
import numpy as np

from packppi_amd import constants as rc

from . import allatom_oracle as A

S, HMAX, NSTATE = 27, 13, 12
# residue: (moved hydrogens, dihedral of the first one per state in degrees; the others follow at + 120 and + 240)
ROTORS = {"SER": (("HG",), [180.0 + 30.0 * c for c in range(12)]), "THR": (("HG1",), [180.0 + 30.0 * c for c in range(12)]),
          "CYS": (("HG",), [180.0 + 30.0 * c for c in range(12)]), "TYR": (("HH",), [180.0, 0.0]),
          "LYS": (("HZ1", "HZ2", "HZ3"), [60.0 + 30.0 * c for c in range(4)])}
# residue: (index of the flipped chi, the atoms that move)
FLIPS = {"ASN": (1, ("OD1", "ND2", "HD21", "HD22")), "GLN": (2, ("OE1", "NE2", "HE21", "HE22")),
         "HIS": (1, ("ND1", "CD2", "CE1", "NE2", "HD2", "HE1", "HE2"))}


def mover_of_type(t):
    """(kind 0 / 1 / 2, states, moved slots ascending) of residue type t."""
    rn, names = rc.resnames[t], A.get_tables()["names"][t]
    if rn in ROTORS:
        return 1, len(ROTORS[rn][1]), sorted(names.index(a) for a in ROTORS[rn][0])
    if rn in FLIPS:
        return 2, 2, sorted(names.index(a) for a in FLIPS[rn][1])
    return 0, 0, []


def flipped_chi(chi, rtype):
    """chi with pi added to the flipped angle of every Asn / Gln / His row, wrapped into [-pi, pi); float32 like the host's."""
    chi = np.asarray(chi, np.float32).reshape(-1, 4).copy()
    for n, t in enumerate(np.asarray(rtype).reshape(-1)):
        rn = rc.resnames[int(t)]
        if rn in FLIPS:
            k = FLIPS[rn][0]
            chi[n, k] = np.float32(np.remainder(np.float32(chi[n, k] + np.float32(2.0 * np.pi)), np.float32(2.0 * np.pi)) - np.float32(np.pi))
    return chi


def _unit(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def candidates(X, rtype, hmask0, dtype=np.float64):
    """Every rotor candidate [N, 12, 3, 3] (state, hydrogen): pp_hydrogens' NERF at the state's dihedral; 0 where there is none."""
    tb = A.get_tables()
    X = np.asarray(X, dtype).reshape(-1, 14, 3)
    rtype, hmask0 = np.asarray(rtype).reshape(-1), np.asarray(hmask0).reshape(-1, HMAX)
    out = np.zeros((X.shape[0], NSTATE, 3, 3), dtype)
    f = lambda deg, fn: dtype(np.float32(fn(np.deg2rad(deg))))
    for n, t in enumerate(rtype):
        kind, ns, moved = mover_of_type(int(t))
        if kind != 1:
            continue
        degs = ROTORS[rc.resnames[int(t)]][1]
        for j, slot in enumerate(moved):
            k = slot - 14
            if hmask0[n, k] == 0:
                continue
            cls, p, at, q, L = tb["hyd"][int(t)][k]
            theta, phis = A.ANGLES[cls]
            P, L = X[n, p], dtype(np.float32(L))
            qa, qb = X[n, at[0]] - P, X[n, at[1]] - P
            e = _unit(-qa)
            nn = _unit(np.cross(qa - qb, e))
            m = np.cross(nn, e)
            for c in range(ns):
                phi = phis[q] if c == 0 else degs[c] + 120.0 * j          # state 0: the very constants of the placement
                with np.errstate(all="ignore"):
                    out[n, c, j] = P + (-(L * f(theta, np.cos)) * e + (L * f(theta, np.sin)) * f(phi, np.cos) * m
                                        + (L * f(theta, np.sin)) * f(phi, np.sin) * nn)
    return out


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


class Problem:
    """One call: the atoms of both sets, the movers, and the energy by the definition."""

    def __init__(self, X0, H0, M0, rtype, chain, seg_off, link_prev, radius, ext, X1=None, H1=None, M1=None, cand=None, link=None,
                 obst=None, obst_off=None, obst_polar=None, cut=0.4, hb_allow=0.6, hb_weak=2.5, hb_good=2.2, dtype=np.float32, acls=None):
        tb = A.get_tables()
        self.dtype, self.tb = dtype, tb
        self.rtype, self.chain = np.asarray(rtype).reshape(-1), np.asarray(chain).reshape(-1)
        N = self.N = self.rtype.shape[0]
        self.seg_off, self.link_prev, self.link = [int(o) for o in seg_off], np.asarray(link_prev).reshape(-1), link
        cat = lambda X, H: np.concatenate([np.asarray(X, dtype).reshape(N, 14, 3), np.asarray(H, dtype).reshape(N, HMAX, 3)], 1)
        self.sets = [cat(X0, H0)] + ([cat(X1, H1)] if X1 is not None else [])
        r = np.asarray(radius, dtype).reshape(N, S).copy()
        with np.errstate(invalid="ignore"):
            r[~(r > 0)] = 0
        self.w = []
        for M in [M0] + ([M1] if X1 is not None else []):
            w = r.copy()
            w[:, 14:][np.asarray(M).reshape(N, HMAX) == 0] = 0
            self.w.append(w)
        self.hmasks = [np.asarray(M0).reshape(N, HMAX)] + ([np.asarray(M1).reshape(N, HMAX)] if X1 is not None else [])
        self.cls = (tb["acls"][self.rtype] if acls is None else np.asarray(acls).reshape(N, S)).astype(np.int32)
        self.sep = tb["sep"][self.rtype].astype(np.int32)
        self.parent = np.zeros((N, S), np.int64)
        for n, t in enumerate(self.rtype):
            for k, h in enumerate(tb["hyd"][int(t)]):
                self.parent[n, 14 + k] = h[1]
        self.cand = None if cand is None else np.asarray(cand, dtype).reshape(N, NSTATE, 3, 3)
        self.cut, self.hb_allow = dtype(cut), dtype(hb_allow)
        self.hbw2 = dtype(np.float32(hb_weak) * np.float32(hb_weak))
        self.hbg2 = dtype(np.float32(hb_good) * np.float32(hb_good))
        self.ext = np.asarray(ext, np.float32)
        self.reach = np.float32(max(np.float32(np.float32(2.0) * np.float32(rc.allatom_default_radius.max()) - np.float32(cut)),
                                    np.float32(hb_weak)))
        self.obst = None if obst is None else np.asarray(obst, dtype).reshape(-1, 4)
        self.obst_off = obst_off
        self.obst_polar = None if obst_polar is None else np.asarray(obst_polar).reshape(-1) != 0
        # the movers
        self.kind, self.ns, self.moved = np.zeros(N, np.int64), np.zeros(N, np.int64), [[] for _ in range(N)]
        for n, t in enumerate(self.rtype):
            kind, ns, moved = mover_of_type(int(t))
            if kind == 2 and X1 is None:
                continue
            if kind and any(self.w[0][n, s] > 0 for s in moved):
                self.kind[n], self.ns[n], self.moved[n] = kind, ns, moved
        self.movers = [n for n in range(N) if self.kind[n]]
        self.seg_of = np.zeros(N, np.int64)
        for s in range(len(self.seg_off) - 1):
            self.seg_of[self.seg_off[s]:self.seg_off[s + 1]] = s
        self.state = np.where(self.kind > 0, 0, -1).astype(np.int32)
        self.cur, self.cur_w = self.sets[0].copy(), self.w[0].copy()
        self.is_moved = np.zeros((N, S), bool)
        for n in self.movers:
            self.is_moved[n, self.moved[n]] = True

    def atoms_at(self, n, c):
        """(positions [nx, 3], radius-or-0 [nx], parent positions [nx, 3]) of the moved atoms of mover n in state c."""
        mv = self.moved[n]
        if self.kind[n] == 1:
            pos = np.stack([self.cand[n, c, j] for j in range(len(mv))])
            w = self.w[0][n, mv]
            pos = np.where((self.hmasks[0][n, [s - 14 for s in mv]] != 0)[:, None], pos, 0)
            par = self.cur[n, self.parent[n, mv]]
        else:
            pos, w = self.sets[c][n, mv], self.w[c][n, mv]
            par = np.stack([self.sets[c][n, self.parent[n, s]] if self.parent[n, s] in mv else self.cur[n, self.parent[n, s]] for s in mv])
        return pos, w, par

    def _allowed(self, i, lo, hi):
        """[27, rows, 27]: the pair (slot of row i, atom of the segment) is not excluded by its bond separation.  Kept per row."""
        memo = self.__dict__.setdefault("_allowed_memo", {})
        if i not in memo:
            memo[i] = self._allowed_now(i, lo, hi)
        return memo[i]

    def _allowed_now(self, i, lo, hi):
        sep, S_ = self.sep, S
        sp = np.full((S_, hi - lo, S_), 99, np.int32)
        sp[:, i - lo, :] = sep[i]
        if i + 1 < hi and self.link_prev[i + 1]:
            sp[:, i + 1 - lo, :] = np.minimum(sp[:, i + 1 - lo, :], sep[i][:, 2][:, None] + 1 + sep[i + 1][0][None, :])
        if i - 1 >= lo and self.link_prev[i]:
            sp[:, i - 1 - lo, :] = np.minimum(sp[:, i - 1 - lo, :], sep[i][:, 0][:, None] + 1 + sep[i - 1][2][None, :])
        if self.link is not None:
            j = int(self.link[i])
            if lo <= j < hi and j != i and int(self.link[j]) == i:
                sp[:, j - lo, :] = np.minimum(sp[:, j - lo, :], sep[i][:, 5][:, None] + 1 + sep[j][5][None, :])
        hyd = (self.cls & 4) != 0
        anyh = hyd[i][:, None, None] | hyd[lo:hi][None]
        return sp > np.where(anyh, 4, 3)

    def _terms(self, p, pw, xcls, pD, Q, qw, qcls, qD, ok, far):
        """Terms [nx, ...] of moved atoms against atoms Q [..., 3]: 64 [overlap] - bond."""
        dt = self.dtype
        ex = (slice(None),) + (None,) * (Q.ndim - 1)
        with np.errstate(all="ignore"):
            d = Q[None] - p[ex]
            d2 = _dot(d, d)
            t = (pw[ex] + qw[None]) - self.cut
            xh = ((xcls & 1) != 0)[ex] & ((qcls & 2) != 0)[None]
            yh = ((xcls & 2) != 0)[ex] & ((qcls & 1) != 0)[None]
            t = np.where(xh | yh, t - self.hb_allow, t)
            ok = ok & (pw > 0)[ex] & (qw > 0)[None]
            ov = ok & (t > 0) & (d2 <= t * t)
            # the bond on the pairs that can have one; the same arithmetic, element by element
            hb = ok & far & (xh | yh)
            bond = np.zeros(hb.shape, np.int64)
            idx = np.nonzero(hb)
            if len(idx[0]):
                isx = xh[idx]
                dd = d[idx]
                v = np.where(isx[:, None], dd, -dd)
                w = np.where(isx[:, None], (pD - p)[idx[0]], (qD - Q)[idx[1:]])
                s, ww, dh = _dot(v, w), _dot(w, w), d2[idx]
                weak = (dh <= self.hbw2) & (s <= 0)
                good = weak & (dh <= self.hbg2) & ((s * s) >= dt(0.25) * (ww * dh))
                bond[idx] = np.where(good, 2, np.where(weak, 1, 0))
        return 64 * ov.astype(np.int64) - bond

    def energy(self, n, c, split=False):
        """E_n(c | current state).  With ``split`` also the part against moved atoms of movers in lower rows."""
        s = int(self.seg_of[n])
        lo, hi = self.seg_off[s], self.seg_off[s + 1]
        mv = self.moved[n]
        p, pw, pD = self.atoms_at(n, c)
        xcls = self.cls[n, mv]
        Q, qw, qcls = self.cur[lo:hi], self.cur_w[lo:hi], self.cls[lo:hi]
        if self.__dict__.get("_curD") is None:
            self._curD = np.take_along_axis(self.cur, self.parent[..., None], 1)
        qD = self._curD[lo:hi]
        ok = self._allowed(n, lo, hi)[mv]                          # a copy: a list index
        ok[:, n - lo, mv] = False                                  # not against a moved atom of its own
        far = np.ones((1, hi - lo, S), bool)
        far[:, n - lo] = False
        T = self._terms(p, pw, xcls, pD, Q, qw, qcls, qD, ok, far)
        E = int(T.sum())
        low = int(T[:, :n - lo][:, self.is_moved[lo:n]].sum()) if split else 0
        has_bond = lambda T: np.where(T > 32, 64 - T, -T) > 0          # a term is 64 [overlap] - bond
        once = np.ones(T.shape[1:], bool)
        once[:n - lo][self.is_moved[lo:n]] = False                 # a bond with a mover in a lower row is counted there
        nb = int((has_bond(T) & once[None]).sum())
        if self.obst is not None:
            o0, o1 = int(self.obst_off[s]), int(self.obst_off[s + 1])
            if o1 > o0:
                O = self.obst[o0:o1]
                pol = np.zeros(o1 - o0, bool) if self.obst_polar is None else self.obst_polar[o0:o1]
                T = self._terms(p, pw, xcls & 1, pD, O[:, :3], O[:, 3], np.where(pol, 2, 0), np.zeros_like(O[:, :3]),
                                np.ones((1, o1 - o0), bool), np.ones((1, o1 - o0), bool))
                E += int(T.sum())
                nb += int(has_bond(T).sum())
        return (E, low, nb) if split else E

    def F(self):
        tot = np.zeros(len(self.seg_off) - 1, np.int64)
        for n in self.movers:
            E, low, _ = self.energy(n, int(self.state[n]), split=True)
            tot[self.seg_of[n]] += E - low
        return tot

    def partners(self, n):
        f = np.float32
        s = int(self.seg_of[n])
        out = []
        ca = self.sets[0][:, 1].astype(np.float32)
        for m in self.movers:
            if m == n or self.seg_of[m] != s:
                continue
            b = f(f(self.ext[self.rtype[n]] + self.ext[self.rtype[m]]) + self.reach)
            d = ca[m] - ca[n]
            with np.errstate(all="ignore"):
                if f(f(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) <= f(b * b):
                    out.append(m)
        return out

    def set_state(self, n, c):
        p, w, _ = self.atoms_at(n, c)
        self.cur[n, self.moved[n]], self.cur_w[n, self.moved[n]] = p, w
        self._curD = None
        self.state[n] = c


def optimize(prob, max_sweeps=32, accept="rule"):
    """The sweep.  Returns a dict: ``state`` [N], ``e`` [N, 2], ``hb`` [N, 2], ``energy`` [N, 12], ``trace`` [n_seg, max_sweeps + 1], ``sweeps``,
    ``converged`` [n_seg] (int32, the device's layout), and ``history``: per sweep the list of (row, from, to, gain) accepted.
    ``accept`` "all" takes every positive proposal at once (not monotone in general: what the partner rule is for)."""
    n_seg, N = len(prob.seg_off) - 1, prob.N
    e, hb, energy = np.zeros((N, 2), np.int32), np.zeros((N, 2), np.int32), np.zeros((N, NSTATE), np.int32)
    trace = np.zeros((n_seg, max_sweeps + 1), np.int32)
    sweeps, conv = np.zeros(n_seg, np.int32), np.zeros(n_seg, np.int32)
    plist = {n: prob.partners(n) for n in prob.movers}
    history = []
    for k in range(max_sweeps + 1):
        prop, gain = {}, {}
        live = [n for n in prob.movers if not conv[prob.seg_of[n]]]
        Fk = np.zeros(n_seg, np.int64)
        for n in live:
            cur = int(prob.state[n])
            E = [prob.energy(n, c, split=True) for c in range(int(prob.ns[n]))]
            low, nb = E[cur][1], E[cur][2]
            E = [v[0] for v in E]
            Fk[prob.seg_of[n]] += E[cur] - low
            best = cur
            for c in range(len(E)):
                if E[c] < E[best]:
                    best = c
            prop[n], gain[n] = best, E[cur] - E[best]
            if k == 0:
                e[n, 0], hb[n, 0] = E[cur], nb
                energy[n, :len(E)] = E
            e[n, 1], hb[n, 1] = E[cur], nb
        for s in range(n_seg):
            if conv[s]:
                trace[s, k] = trace[s, k - 1]
            else:
                trace[s, k] = Fk[s]
                if not any(gain[n] > 0 for n in live if prob.seg_of[n] == s):
                    conv[s] = 1
        if k == max_sweeps:
            break
        acc = []
        for n in live:
            if gain[n] <= 0:
                continue
            if accept == "all" or all(not (gain.get(m, 0) > 0) or gain[m] < gain[n] or (gain[m] == gain[n] and m > n) for m in plist[n]):
                acc.append((n, int(prob.state[n]), prop[n], gain[n]))
        for n, _, c, _ in acc:
            prob.set_state(n, c)
        for s in range(n_seg):
            if any(prob.seg_of[n] == s for n, _, _, _ in acc):
                sweeps[s] += 1
        history.append(acc)
    hmask_out = prob.hmasks[0].copy()
    for n in prob.movers:
        if prob.kind[n] == 2 and prob.state[n] == 1:
            hmask_out[n] = prob.hmasks[1][n]
    return dict(state=prob.state.copy(), e=e, hb=hb, energy=energy, trace=trace, sweeps=sweeps, converged=conv, history=history,
                hmask_out=hmask_out.astype(np.uint8), plist=plist)


def near_threshold(prob64, n, c, tol=1e-4, within=4.0):
    """(candidate pairs, pairs with a float64 distance within ``tol`` A of a threshold) of mover n at state c against the protein
    atoms: masks [nx, rows, 27].  Thresholds: the overlap distance, hb_weak, hb_good, the right angle (the projection of A - h on
    D - h is 0) and 120 degrees (it is half of |A - h|).  Candidates: allowed pairs of counted atoms within ``within`` A."""
    p = prob64
    s = int(p.seg_of[n])
    lo, hi = p.seg_off[s], p.seg_off[s + 1]
    mv = p.moved[n]
    pos, pw, pD = p.atoms_at(n, c)
    Q, qw, qcls = p.cur[lo:hi], p.cur_w[lo:hi], p.cls[lo:hi]
    qD = np.take_along_axis(Q, p.parent[lo:hi][..., None], 1)
    ok = p._allowed(n, lo, hi)[mv]
    ok[:, n - lo, mv] = False
    xcls = p.cls[n, mv]
    with np.errstate(all="ignore"):
        d = Q[None] - pos[:, None, None]
        dist = np.sqrt(_dot(d, d))
        xh = ((xcls & 1) != 0)[:, None, None] & ((qcls & 2) != 0)[None]
        yh = ((xcls & 2) != 0)[:, None, None] & ((qcls & 1) != 0)[None]
        t = (pw[:, None, None] + qw[None]) - p.cut - np.where(xh | yh, p.hb_allow, 0.0)
        ok = ok & (pw > 0)[:, None, None] & (qw > 0)[None]
        cand = ok & (dist <= within)
        near = np.abs(dist - t) <= tol
        v = np.where(xh[..., None], d, -d)
        w = np.where(xh[..., None], (pD - pos)[:, None, None], qD[None] - Q[None])
        proj = _dot(v, w) / np.sqrt(_dot(w, w))
        hb = (xh | yh) & (np.arange(lo, hi) != n)[None, :, None]
        near |= hb & ((np.abs(dist - np.sqrt(p.hbw2)) <= tol) | (np.abs(dist - np.sqrt(p.hbg2)) <= tol))
        near |= hb & (dist <= np.sqrt(p.hbw2) + tol) & ((np.abs(proj) <= tol) | (np.abs(np.abs(proj) - 0.5 * dist) <= tol))
    return cand, cand & near


def pair_terms(prob, n, c):
    """The terms [nx, rows, 27] of mover n at state c against the protein atoms of its segment."""
    s = int(prob.seg_of[n])
    lo, hi = prob.seg_off[s], prob.seg_off[s + 1]
    mv = prob.moved[n]
    p, pw, pD = prob.atoms_at(n, c)
    Q, qw, qcls = prob.cur[lo:hi], prob.cur_w[lo:hi], prob.cls[lo:hi]
    qD = np.take_along_axis(Q, prob.parent[lo:hi][..., None], 1)
    ok = prob._allowed(n, lo, hi)[mv]
    ok[:, n - lo, mv] = False
    far = np.ones((1, hi - lo, S), bool)
    far[:, n - lo] = False
    return prob._terms(p, pw, prob.cls[n, mv], pD, Q, qw, qcls, qD, ok, far)


def host_problem(batch, chi=None, dtype=np.float32, link=None, **kw):
    """A ``Problem`` made on the host alone: heavy atoms from the CPU reconstruction at ``chi`` (default: the batch's own angles) and at
    the flipped angles, hydrogens and candidates from the oracles, ``ext`` from ``constants``."""
    import torch
    from oracle import ref_cpu as O
    from . import polar_oracle as PO
    _, _, _, chain, offs = PO.arrays(batch)
    am, rt = batch["atom_mask"].reshape(-1, 14).numpy(), batch["residue_type"].reshape(-1).numpy()
    chi0 = np.asarray(batch["SC_D"] if chi is None else chi, np.float32).reshape(-1, 4)
    chi1 = flipped_chi(chi0, rt)
    shape = tuple(batch["SC_D"].shape)
    sets = []
    for ch in (chi0, chi1):
        X = O.atom14_coords(batch["X"].double(), batch["residue_type"], batch["BB_D"].double(), torch.from_numpy(ch).double().reshape(shape))
        X = X.reshape(-1, 14, 3).numpy().astype(np.float32).astype(dtype)
        H, M, lp = A.hydrogens(X, am, rt, chain, offs, link=link, dtype=dtype)
        sets.append((X, H, M, lp))
    radius = A.default_radius(rt, am, rotatable="keep")
    cand = candidates(sets[0][0], rt, sets[0][2], dtype)
    return Problem(sets[0][0], sets[0][1], sets[0][2], rt, chain, offs, sets[0][3], radius, rc.mover_extent, sets[1][0], sets[1][1],
                   sets[1][2], cand=cand, link=link, dtype=dtype, **kw)
