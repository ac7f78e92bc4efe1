"""Brute-force NumPy oracle of pp_chi_refine, float64 or float32.

No row filter and no partner cap.  Which atoms move is typed out here from the hydrogen lists of tests/allatom_oracle.py (radii,
classes, bond separations and the hydrogen geometry are that file's); the bond term and the exclusions are tests/hnet_oracle.py's.
The float32 form restates the kernel's operation order, so its integers can be compared with the device's as bytes.  Coordinates
come from a ``build`` callable: on the host the CPU reconstruction and the hydrogen oracle, in the GPU tests the device's own
``atom14`` / ``hydrogens``, which is what "fed the device's own candidates" means for a state that changes from sweep to sweep.
"""
import numpy as np

from packppi_amd import constants as rc

from . import allatom_oracle as A
from . import hnet_oracle as H

S, HMAX, NCAND = 27, 13, 9
PI, TWO_PI = np.float32(3.14159274), np.float32(6.28318548)


def moved_of_type(t):
    """The slots a chi step can move: atom14 slots 5 .. 13 that exist, and every hydrogen whose parent or one of the atoms it is built
    from is such a slot."""
    tb = A.get_tables()
    names = tb["names"][t]
    heavy = [s for s in range(5, 14) if names[s]]
    hyd = [14 + k for k, (cls, p, at, q, L) in enumerate(tb["hyd"][t]) if p >= 5 or any(a >= 5 for a in at)]
    return heavy + hyd


def angles(chi0, steps, delta):
    """float32 [.., 4]: chi0 where steps == 0 (its bits), else chi0 + steps * delta wrapped once into [-pi, pi)."""
    chi0 = np.asarray(chi0, np.float32)
    with np.errstate(all="ignore"):
        a = chi0 + np.asarray(steps).astype(np.float32) * np.float32(delta)
        a = np.where(a >= PI, a - TWO_PI, a)
        a = np.where(a < -PI, a + TWO_PI, a)
    return np.where(np.asarray(steps) == 0, chi0, a).astype(np.float32)


def cand_step(c):
    """(chi index, +1 / -1) of candidate c >= 1."""
    return (c - 1) >> 1, (1 if c & 1 else -1)


class Problem:
    """One call of pp_chi_refine.  ``build(chi [N, 4] float32, rows)`` returns (X [N, 14, 3], H [N, 13, 3], M [N, 13]) in ``dtype``,
    valid at least on ``rows`` (None: every row)."""

    def __init__(self, chi0, build, rtype, chain, seg_off, link_prev, rmask, scd_mask, radius, ext, fixed=None, link=None, obst=None,
                 obst_off=None, obst_polar=None, delta=np.deg2rad(16.0), max_steps=3, bands=4, band=0.15, cut=0.4, hb_allow=0.6,
                 hb_weak=2.5, hb_good=2.2, dtype=np.float32, acls=None, r_max=None):
        tb = A.get_tables()
        self.dtype, self.build = dtype, build
        self.rtype, self.chain = np.asarray(rtype).reshape(-1), np.asarray(chain).reshape(-1)
        N = self.N = len(self.rtype)
        self.seg_off, self.link_prev = [int(o) for o in seg_off], np.asarray(link_prev).reshape(-1)
        self.link = None if link is None else np.asarray(link).reshape(-1)
        self.chi0 = np.asarray(chi0, np.float32).reshape(N, 4).copy()
        self.delta, self.max_steps = np.float32(delta), int(max_steps)
        self.bands, self.band = int(bands), dtype(band)
        self.cut, self.hb_allow = dtype(cut), dtype(hb_allow)
        self.hbw2 = dtype(np.float32(hb_weak) * np.float32(hb_weak))
        self.hbg2 = dtype(np.float32(hb_good) * np.float32(hb_good))
        r = np.asarray(radius, dtype).reshape(N, S).copy()
        with np.errstate(invalid="ignore"):
            r[~(r > 0)] = 0
        self.r = r
        self.cls = (tb["acls"][self.rtype] if acls is None else np.asarray(acls).reshape(N, S)).astype(np.int32)
        self.sep = tb["sep"][self.rtype].astype(np.int32)
        self.parent = np.zeros((N, S), np.int64)
        for n, t in enumerate(self.rtype):
            for k, h in enumerate(tb["hyd"][int(t)]):
                self.parent[n, 14 + k] = h[1]
        self.ext = np.asarray(ext, np.float32)
        r_max = tb["radius"].max() if r_max is None else r_max      # the largest radius of the table, whatever atoms the rows have
        self.reach = np.float32(max(np.float32(np.float32(2.0) * np.float32(r_max) - np.float32(cut)), np.float32(hb_weak)))
        self.obst = None if obst is None else np.asarray(obst, dtype).reshape(-1, 4)
        self.obst_off = obst_off
        self.obst_polar = None if obst_polar is None else np.asarray(obst_polar).reshape(-1) != 0
        self.scd = np.asarray(scd_mask).reshape(N, 4) != 0
        fx = np.zeros(N, bool) if fixed is None else np.asarray(fixed).reshape(-1) != 0
        if self.link is not None:
            fx = fx | (self.link >= 0)
        self.fixed = fx
        is_mover = (np.asarray(rmask).reshape(-1) != 0) & self.scd.any(1) & ~fx & (self.rtype >= 0) & (self.rtype <= 20)
        self.movers = [int(n) for n in np.nonzero(is_mover)[0]]
        self.moved = [moved_of_type(int(t)) if is_mover[n] else [] for n, t in enumerate(self.rtype)]
        self.is_moved = np.zeros((N, S), bool)
        for n in self.movers:
            self.is_moved[n, self.moved[n]] = True
        self.seg_of = np.zeros(N, np.int64)
        for s in range(len(self.seg_off) - 1):
            self.seg_of[self.seg_off[s]:self.seg_off[s + 1]] = s
        self.steps = np.zeros((N, 4), np.int8)
        X, Hh, M = build(self.chi0, None)
        self.cur = np.concatenate([np.asarray(X, dtype).reshape(N, 14, 3), np.asarray(Hh, dtype).reshape(N, HMAX, 3)], 1)
        self.cur_w = self._w(np.asarray(M).reshape(N, HMAX), slice(None))
        self.sets = [self.cur]                                 # H.Problem.partners reads slot 1 of sets[0]: the backbone does not move
        self._curD = None

    # the exclusions of step 5 and the partner predicate are tests/hnet_oracle.py's, on this object's tables
    _allowed_now = H.Problem._allowed_now
    partners = H.Problem.partners

    def _w(self, M, rows):
        w = self.r[rows].copy()
        w[..., 14:][M == 0] = 0
        return w

    def chi(self):
        return angles(self.chi0, self.steps, self.delta)

    def exists(self, n, c):
        if c == 0:
            return True
        j, d = cand_step(c)
        return bool(self.scd[n, j]) and abs(int(self.steps[n, j]) + d) <= self.max_steps

    def candidate_sets(self, rows):
        """Per candidate c: (chi [N, 4], atoms [N, 27, 3], radius-or-0 [N, 27]) with rows outside ``rows`` (or without the candidate)
        at their current state."""
        out = []
        for c in range(NCAND):
            st = self.steps.copy()
            have = [n for n in rows if self.exists(n, c)]
            if c > 0:
                j, d = cand_step(c)
                st[have, j] += d
            ch = angles(self.chi0, st, self.delta)
            if c > 0 and not have:
                out.append((ch, None, None))
                continue
            X, Hh, M = self.build(ch, have)
            at = np.concatenate([np.asarray(X, self.dtype).reshape(self.N, 14, 3), np.asarray(Hh, self.dtype).reshape(self.N, HMAX, 3)], 1)
            out.append((ch, at, self._w(np.asarray(M).reshape(self.N, HMAX), slice(None))))
        return out

    def _terms(self, p, pw, xcls, pD, Q, qw, qcls, qD, ok, far):
        """Terms [nx, ...] of moved atoms against atoms Q [..., 3]: 64 level - bond.  Also the levels."""
        dt = self.dtype
        ex = (slice(None),) + (None,) * (Q.ndim - 1)
        with np.errstate(all="ignore"):
            d = Q[None] - p[ex]
            d2 = H._dot(d, d)
            t = (pw[ex] + qw[None]) - self.cut
            xh = ((xcls & 1) != 0)[ex] & ((qcls & 2) != 0)[None]
            yh = ((xcls & 2) != 0)[ex] & ((qcls & 1) != 0)[None]
            t = np.where(xh | yh, t - self.hb_allow, t)
            ok = ok & (pw > 0)[ex] & (qw > 0)[None]
            level = np.zeros(d2.shape, np.int64)
            for k in range(self.bands):
                tk = t - dt(k) * self.band
                level += (tk > 0) & (d2 <= tk * tk)
            level = np.where(ok, level, 0)
            hb = ok & far & (xh | yh)
            bond = np.zeros(hb.shape, np.int64)
            idx = np.nonzero(hb)
            if len(idx[0]):
                isx = xh[idx]
                dd = d[idx]
                v = np.where(isx[:, None], dd, -dd)
                w = np.where(isx[:, None], (pD - p)[idx[0]], (qD - Q)[idx[1:]])
                s, ww, dh = H._dot(v, w), H._dot(w, w), d2[idx]
                weak = (dh <= self.hbw2) & (s <= 0)
                good = weak & (dh <= self.hbg2) & ((s * s) >= dt(0.25) * (ww * dh))
                bond[idx] = np.where(good, 2, np.where(weak, 1, 0))
        return 64 * level - bond, level

    def pair_terms(self, n, atoms, w):
        """(terms, levels) [nx, rows, 27] of mover n with its moved atoms taken from ``atoms`` / ``w`` [N, 27, ..], against the protein
        atoms of its segment at their current state; and the same against its obstacle atoms ([nx, M] or None)."""
        s = int(self.seg_of[n])
        lo, hi = self.seg_off[s], self.seg_off[s + 1]
        mv = self.moved[n]
        p, pw, pD = atoms[n, mv], w[n, mv], atoms[n, self.parent[n, mv]]
        xcls = self.cls[n, mv]
        Q, qw, qcls = self.cur[lo:hi], self.cur_w[lo:hi], self.cls[lo:hi]
        if self._curD is None:
            self._curD = np.take_along_axis(self.cur, self.parent[..., None], 1)
        memo = self.__dict__.setdefault("_allowed_memo", {})
        if n not in memo:
            memo[n] = self._allowed_now(n, lo, hi)
        ok = memo[n][mv]
        ok[:, n - lo, mv] = False                              # not against a moved atom of its own
        far = np.ones((1, hi - lo, S), bool)
        far[:, n - lo] = False
        T, Lv = self._terms(p, pw, xcls, pD, Q, qw, qcls, self._curD[lo:hi], ok, far)
        TO = LO = None
        if self.obst is not None:
            o0, o1 = int(self.obst_off[s]), int(self.obst_off[s + 1])
            if o1 > o0:
                O = self.obst[o0:o1]
                pol = np.zeros(o1 - o0, bool) if self.obst_polar is None else self.obst_polar[o0:o1]
                TO, LO = self._terms(p, pw, xcls & 1, pD, O[:, :3], O[:, 3], np.where(pol, 2, 0), np.zeros_like(O[:, :3]),
                                     np.ones((1, o1 - o0), bool), np.ones((1, o1 - o0), bool))
        return T, Lv, TO, LO

    def energy(self, n, atoms, w):
        """(E, the part against moved atoms of movers in lower rows, a term has level >= 1)."""
        s = int(self.seg_of[n])
        lo = self.seg_off[s]
        T, Lv, TO, LO = self.pair_terms(n, atoms, w)
        E, hot = int(T.sum()), bool((Lv >= 1).any())
        low = int(T[:, :n - lo][:, self.is_moved[lo:n]].sum())
        if TO is not None:
            E += int(TO.sum())
            hot = hot or bool((LO >= 1).any())
        return E, low, hot

    def F(self):
        tot = np.zeros(len(self.seg_off) - 1, np.int64)
        for n in self.movers:
            E, low, _ = self.energy(n, self.cur, self.cur_w)
            tot[self.seg_of[n]] += E - low
        return tot

    def set_state(self, n, c, atoms, w):
        j, d = cand_step(c)
        self.steps[n, j] += d
        self.cur[n], self.cur_w[n] = atoms[n], w[n]
        self._curD = None


def optimize(prob, max_sweeps=32, accept="rule", want_energy=True, reuse=True):
    """The sweep.  Returns a dict: ``steps`` int8 [N, 4], ``chi`` float32 [N, 4], ``e`` [N, 2], ``energy`` [N, 9], ``cand_mask`` [N],
    ``trace`` [n_seg, max_sweeps + 1], ``sweeps``, ``converged`` [n_seg] (int32, the device's layout), ``history``: per sweep the list
    of (row, candidate, gain) accepted, ``proposers``: per sweep the rows with a positive gain, ``hot``: per sweep the movers with a
    term of level >= 1, ``gains``: per sweep the gain of every live mover, and ``plist``.  Without ``want_energy`` the candidates of movers without an overlap are not built (``energy`` and
    ``cand_mask`` then hold the others only).  ``reuse``: the energies of a mover are taken over from the sweep before when no row
    that moved since can share a term with it in any state -- every atom of a row lies within max(ext, 3 A) of its CA (``ext``
    is checked against a chi grid; the backbone and its hydrogens are within 2.5 A) and a term needs two atoms within
    max(2 x the largest radius of the call - cut, hb_weak), so a row whose CA is farther than its bound + that reach from every
    atom of the row that moved, before and after, shares none with it.  The reach is taken from the call's own radii and
    ``hb_weak``, so the argument holds for any of them; it would stop holding only for an ``ext`` table that does not bound the
    side chains, which is what tests/test_refine_host.py checks.  It saves time and changes no
    word (``reuse=False`` recomputes everything; the tests compare the two)."""
    n_seg, N = len(prob.seg_off) - 1, prob.N
    e, energy, cmask = np.zeros((N, 2), np.int32), np.zeros((N, NCAND), np.int32), np.zeros(N, np.int32)
    trace = np.zeros((n_seg, max_sweeps + 1), np.int32)
    sweeps, conv = np.zeros(n_seg, np.int32), np.zeros(n_seg, np.int32)
    plist = {n: prob.partners(n) for n in prob.movers}
    history, proposers, hots, gains = [], [], [], []
    base, cands, dirty = {}, {}, set(prob.movers)
    bound = np.maximum(prob.ext[np.clip(prob.rtype, 0, 20)].astype(np.float64), 3.0)
    with np.errstate(all="ignore"):
        span = max(2.0 * float(np.nanmax(prob.r)) - float(prob.cut), float(np.sqrt(prob.hbw2)), float(prob.reach)) + 1e-3
    ca = prob.cur[:, 1].astype(np.float64)
    for k in range(max_sweeps + 1):
        live = [n for n in prob.movers if not conv[prob.seg_of[n]]]
        # candidate 0 first: who is hot decides whose other candidates are ever looked at
        for n in live:
            if n in dirty or not reuse:
                base[n] = prob.energy(n, prob.cur, prob.cur_w)
                cands.pop(n, None)
        hot = [n for n in live if base[n][2]]
        first = k == 0 and want_energy
        sets = prob.candidate_sets(live if first else hot)
        prop, gain = {}, {}
        Fk = np.zeros(n_seg, np.int64)
        for n in live:
            E0, low, is_hot = base[n]
            Fk[prob.seg_of[n]] += E0 - low
            E = [E0] + [None] * (NCAND - 1)
            if n in cands:
                E = cands[n]
            elif is_hot or first:
                for c in range(1, NCAND):
                    if prob.exists(n, c):
                        E[c] = prob.energy(n, sets[c][1], sets[c][2])[0]
                cands[n] = E
            best = 0
            if is_hot:
                for c in range(1, NCAND):
                    if E[c] is not None and E[c] < E[best]:
                        best = c
            prop[n], gain[n] = best, E0 - E[best]
            if k == 0:
                e[n, 0] = E0
                energy[n] = [0 if v is None else v for v in E]
                cmask[n] = sum(1 << c for c in range(NCAND) if E[c] is not None)
            e[n, 1] = E0
        for s in range(n_seg):
            if conv[s]:
                trace[s, k] = trace[s, k - 1]
            else:
                trace[s, k] = Fk[s]
                if not any(gain[n] > 0 for n in live if prob.seg_of[n] == s):
                    conv[s] = 1
        hots.append(hot)
        gains.append(dict(gain))
        proposers.append([n for n in live if gain[n] > 0])
        if k == max_sweeps:
            break
        acc = []
        for n in live:
            if gain[n] <= 0:
                continue
            if accept == "all" or all(not (gain.get(m, 0) > 0) or gain[m] < gain[n] or (gain[m] == gain[n] and m > n) for m in plist[n]):
                acc.append((n, prop[n], gain[n]))
        old_atoms = {n: prob.cur[n].copy() for n, _, _ in acc}
        for n, c, _ in acc:
            prob.set_state(n, c, sets[c][1], sets[c][2])
        dirty = set()
        for m, _, _ in acc:
            pts = np.concatenate([old_atoms[m], prob.cur[m]]).astype(np.float64)
            with np.errstate(all="ignore"):
                far = np.nanmin(np.linalg.norm(ca[:, None] - pts[None], axis=-1), axis=1) > bound + span
            dirty |= {n for n in prob.movers if not far[n]} | {m}
        for s in range(n_seg):
            if any(prob.seg_of[n] == s for n, _, _ in acc):
                sweeps[s] += 1
        history.append(acc)
    return dict(steps=prob.steps.copy(), chi=prob.chi(), e=e, energy=energy, cand_mask=cmask, trace=trace, sweeps=sweeps, converged=conv,
                history=history, proposers=proposers, hot=hots, gains=gains, plist=plist)


def host_build(batch, dtype=np.float32, link=None):
    """A ``build`` made on the host alone: heavy atoms from the CPU reconstruction (rounded to float32 as the device stores them, then
    taken in ``dtype``), hydrogens from tests/allatom_oracle.py.  A row's atoms depend on its own angles alone (the hydrogen on the
    backbone N reads the previous C, which no angle moves), so rows are built on request and remembered by their angle bytes."""
    import torch
    from oracle import ref_cpu as O
    from . import polar_oracle as PO
    _, _, _, chain, offs = PO.arrays(batch)
    N = batch["residue_type"].numel()
    am, rt = batch["atom_mask"].reshape(N, 14).numpy(), batch["residue_type"].reshape(N).numpy()
    X0, bb = batch["X"].double().reshape(1, N, 14, 3), batch["BB_D"].double().reshape(1, N, 3)
    firsts = set(int(o) for o in offs[:-1])
    memo = {}
    lk = None if link is None else np.asarray(link).reshape(-1)

    def build(chi, rows):
        chi = np.asarray(chi, np.float32).reshape(N, 4)
        rows = list(range(N)) if rows is None else [int(r) for r in rows]
        need = [r for r in rows if (r, chi[r].tobytes()) not in memo]
        if need:
            idx = torch.tensor(need)
            X = O.atom14_coords(X0[:, idx], batch["residue_type"].reshape(1, N)[:, idx], bb[:, idx],
                                torch.from_numpy(chi[need]).double()[None]).reshape(-1, 14, 3).numpy().astype(np.float32).astype(dtype)
            # every row behind its predecessor, a segment of two: the hydrogen oracle sees the previous C and nothing else
            m = len(need)
            X2, am2, rt2, ch2 = np.zeros((2 * m, 14, 3), dtype), np.zeros((2 * m, 14), am.dtype), np.zeros(2 * m, rt.dtype), np.zeros(2 * m, np.int64)
            for q, r in enumerate(need):
                has_prev = r not in firsts and r > 0
                p = r - 1 if has_prev else r
                X2[2 * q] = X0[0, p].numpy().astype(np.float32).astype(dtype)
                X2[2 * q + 1] = X[q]
                am2[2 * q], am2[2 * q + 1] = am[p], am[r]
                rt2[2 * q], rt2[2 * q + 1] = rt[p], rt[r]
                ch2[2 * q], ch2[2 * q + 1] = (chain[p] if has_prev else chain[r] + 1), chain[r]
            l2 = None if lk is None else np.repeat(lk[need], 2)
            Hh, M, _ = A.hydrogens(X2, am2, rt2, ch2, list(range(0, 2 * m + 1, 2)), link=l2, dtype=dtype)
            for q, r in enumerate(need):
                memo[(r, chi[r].tobytes())] = (X[q], Hh[2 * q + 1], M[2 * q + 1])
        Xo, Ho, Mo = np.zeros((N, 14, 3), dtype), np.zeros((N, HMAX, 3), dtype), np.zeros((N, HMAX), np.uint8)
        for r in rows:
            Xo[r], Ho[r], Mo[r] = memo[(r, chi[r].tobytes())]
        return Xo, Ho, Mo
    return build


def host_problem(batch, chi=None, dtype=np.float32, link=None, **kw):
    """A ``Problem`` made on the host alone, rotatable hydrogens not counted, ``ext`` from ``constants``."""
    from . import polar_oracle as PO
    _, _, _, chain, offs = PO.arrays(batch)
    N = batch["residue_type"].numel()
    am, rt = batch["atom_mask"].reshape(N, 14).numpy(), batch["residue_type"].reshape(N).numpy()
    chi0 = np.asarray(batch["SC_D"] if chi is None else chi, np.float32).reshape(N, 4)
    X = batch["X"].reshape(N, 14, 3).numpy()
    lp = A.link_prev_of(X.astype(dtype), am, chain, offs, dtype)
    return Problem(chi0, host_build(batch, dtype, link), rt, chain, offs, lp, batch["residue_mask"].reshape(N).numpy(),
                   batch["SC_D_mask"].reshape(N, 4).numpy(), A.default_radius(rt, am, "skip"), rc.refine_extent, link=link, dtype=dtype, **kw)

