"""Anchors (pp_anchor_close) restated with NumPy, by brute force.  Not a test module: tests/test_anchor_host.py
and tests/test_anchor_gpu.py import it.

The atoms of every grid point come from ``oracle.ref_cpu.atom14_coords`` -- the reconstruction pp_atom14 follows --, in the precision
asked for, on the row moved to its own CA (the definition builds relative to CA); validity, the grid, the energy and the closure follow
include/packppi_hip.h.  Run in float32 it is what the device is compared with; run in float64 it is the arbiter, and the difference
between the two is the tolerance of that comparison."""
import numpy as np
import torch

from oracle import ref_cpu
from packppi_amd import constants as rc

PER_ROW = 4
GRID = {1: 72, 2: 72, 3: 36, 4: 24}


def theta(g, dtype=np.float32):
    """The grid: (dtype)(-pi + 2 pi k / g), the double expression rounded once."""
    return np.array([-np.pi + 2 * np.pi * k / g for k in range(g)], dtype=np.float64).astype(dtype)


def _dot(a, b):
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def _angle(P, V, Q, f):
    u, v = P - V, Q - V
    c = _dot(u, v) / (np.sqrt(_dot(u, u)) * np.sqrt(_dot(v, v)))
    return np.arccos(np.clip(c, f(-1), f(1))) * f(180.0 / np.pi)


def wrap(x, f):
    return x - np.rint(x / f(2 * np.pi)) * f(2 * np.pi)


def valid(batch, anchors):
    """bool [A]: the entries the device keeps before it counts four per row."""
    rt = np.asarray(batch["residue_type"]).reshape(-1)
    rm = np.asarray(batch["residue_mask"]).reshape(-1)
    am = np.asarray(batch["atom_mask"]).reshape(-1, 14)
    a2g = np.asarray(rc.atom14_to_group)
    N = rt.size
    ok = np.zeros(len(anchors), bool)
    for i in range(len(anchors)):
        r, s, a = int(anchors.rows[i]), int(anchors.slots[i]), int(anchors.antes[i])
        if not (0 <= r < N and 5 <= s <= 13 and 0 <= a <= 13 and a != s):
            continue
        if not 0 <= rt[r] <= 20 or rm[r] == 0 or not all(am[r, k] != 0 for k in (0, 1, 2, s, a)):
            continue
        if not 4 <= a2g[rt[r], s] <= 7:
            continue
        v = np.concatenate([anchors.targets[i], anchors.params[i]]).astype(np.float32)
        ok[i] = bool(np.isfinite(v).all() and v[4] > 0)
    return ok


def row_lists(batch, anchors):
    """({row: [anchor indices, at most four, in list order]}, set of rows with a dropped entry)."""
    ok = valid(batch, anchors)
    N = np.asarray(batch["residue_type"]).size
    lists, bad = {}, set()
    for i in range(len(anchors)):
        r = int(anchors.rows[i])
        if not ok[i]:
            if 0 <= r < N:
                bad.add(r)
            continue
        if len(lists.setdefault(r, [])) < PER_ROW:
            lists[r].append(i)
        else:
            bad.add(r)
    return lists, bad


def _atoms(batch, row, chis, dtype):
    """atom14 [m, 14, 3] of ``row`` at the m angle sets ``chis`` [m, 4], relative to the row's CA, through atom14_coords."""
    td = torch.float32 if dtype == np.float32 else torch.float64
    m = len(chis)
    X = torch.as_tensor(np.asarray(batch["X"])).reshape(-1, 14, 3)[row].to(td)
    X = (X - X[1]).expand(m, 14, 3)[None]
    S = torch.as_tensor(np.asarray(batch["residue_type"])).reshape(-1)[row].long().expand(m)[None]
    BB = torch.as_tensor(np.asarray(batch["BB_D"])).reshape(-1, 3)[row].to(td).expand(m, 3)[None]
    return ref_cpu.atom14_coords(X, S, BB, torch.as_tensor(np.ascontiguousarray(chis), dtype=td)[None])[0].numpy()


def row_energy(batch, anchors, idx, row, chis, dtype):
    """(E [m], D [na, m], ANG [na, m]) of the anchors ``idx`` of ``row`` at the angle sets ``chis`` [m, 4]."""
    f = dtype
    xyz = _atoms(batch, row, chis, dtype)
    ca = np.asarray(batch["X"]).reshape(-1, 14, 3)[row, 1].astype(dtype)
    E, Ds, As = None, [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in idx:
            q = anchors.targets[i].astype(dtype) - ca
            d0, sd, th0, st = (f(v) for v in anchors.params[i])
            A, P = xyz[:, int(anchors.slots[i])], xyz[:, int(anchors.antes[i])]
            dv = A - q
            d = np.sqrt(_dot(dv, dv))
            ang = _angle(P, A, q[None], f)
            t = ((d - d0) / sd) ** 2
            if st > 0:
                t = t + ((ang - th0) / st) ** 2
            E = t if E is None else E + t
            Ds.append(d)
            As.append(ang)
    return np.where(np.isnan(E), f(np.inf), E), np.stack(Ds), np.stack(As)


def row_n(batch, anchors, idx, row):
    """The number of chi the donors of the anchors ``idx`` of ``row`` depend on."""
    rt = int(np.asarray(batch["residue_type"]).reshape(-1)[row])
    return max(int(np.asarray(rc.atom14_to_group)[rt, int(anchors.slots[i])]) - 3 for i in idx)


def row_grid(batch, anchors, idx, row, own, dtype):
    """(n, g, E [g^n], D [na, g^n], ANG [na, g^n]) over the row's grid in flat-index order; chi beyond n are ``own``'s."""
    n = row_n(batch, anchors, idx, row)
    g = GRID[n]
    th = theta(g, dtype)
    inner = np.stack(np.meshgrid(*([th] * (n - 1)), indexing="ij"), -1).reshape(-1, n - 1) if n > 1 else np.zeros((1, 0), dtype)
    Es, Ds, As = [], [], []
    for k1 in range(g):                                        # one slab per first digit: the 24^4 grid does not fit in one call
        chis = np.tile(np.asarray(own, dtype)[None], (len(inner), 1))
        chis[:, 0] = th[k1]
        chis[:, 1:n] = inner
        e, d, a = row_energy(batch, anchors, idx, row, chis, dtype)
        Es.append(e); Ds.append(d); As.append(a)
    return n, g, np.concatenate(Es), np.concatenate(Ds, 1), np.concatenate(As, 1)


def solve(batch, seg_offs, anchors, chi=None, fixed=None, max_energy=10.0, sigma_chi=np.deg2rad(20.0), dtype=np.float32, cache=None):
    """The definition, brute force.  ``anchors``: a ``selection.AnchorSet`` with rows of the batch.  Returns a dict: ``status`` [N],
    ``report`` [N, 4], ``anchor_report`` [A, 2], ``count`` [n_seg], ``chi`` (None without chi), and per anchored row ``lists`` (its
    anchor indices), ``n``, ``g``, ``E`` (the grid, flat), ``J`` (J over F, +inf outside), ``Jall`` (J everywhere), ``thr``, ``emin``, ``pick`` (flat index),
    ``D`` / ``ANG`` [na, g^n].  ``cache``: a dict that keeps the grids of E between calls with the same rows and anchors."""
    f = dtype
    N = np.asarray(batch["residue_type"]).size
    lists, bad = row_lists(batch, anchors)
    seg_of = np.searchsorted(np.asarray(seg_offs), np.arange(N), side="right") - 1
    status = np.zeros(N, np.int64)
    report = np.zeros((N, 4), dtype)
    arep = np.zeros((len(anchors), 2), dtype)
    chi_out = None if chi is None else np.array(np.asarray(chi, dtype=np.float32).reshape(-1, 4), copy=True)
    chi_in = np.zeros((N, 4), dtype) if chi is None else np.asarray(chi, dtype=np.float32).reshape(-1, 4).astype(dtype)
    fx = np.zeros(N, bool) if fixed is None else (np.asarray(fixed).reshape(-1) != 0)
    out = dict(lists=lists, n={}, g={}, E={}, J={}, Jall={}, thr={}, emin={}, pick={}, D={}, ANG={})
    for r in bad:
        status[r] = -2
    for r, idx in sorted(lists.items()):
        if fx[r]:
            e, d, a = row_energy(batch, anchors, idx, r, chi_in[r][None], dtype)
            report[r] = (e[0], e[0], d[0, 0], a[0, 0])
            arep[idx, 0], arep[idx, 1] = d[:, 0], a[:, 0]
            status[r] = -2 if r in bad else 2
            continue
        # E reads the chi beyond n alone; the key names the row's anchors by value (one cache per batch)
        key = (r, np.dtype(dtype).name, chi_in[r, row_n(batch, anchors, idx, r):].tobytes(), anchors.slots[idx].tobytes(),
               anchors.antes[idx].tobytes(), anchors.targets[idx].tobytes(), anchors.params[idx].tobytes())
        if cache is not None and key in cache:
            n, g, E, D, ANG = cache[key]
        else:
            n, g, E, D, ANG = row_grid(batch, anchors, idx, r, chi_in[r], dtype)
            if cache is not None:
                cache[key] = (n, g, E, D, ANG)
        emin = E.min()
        out["n"][r], out["g"][r], out["E"][r], out["D"][r], out["ANG"][r], out["emin"][r] = n, g, E, D, ANG, emin
        report[r, 0] = emin
        if emin > f(max_energy):
            status[r] = -2 if r in bad else -1
            continue
        thr = max(min(f(max_energy), emin + f(4)), emin)
        J = E.copy()
        if chi is not None:
            th = theta(g, dtype)
            w = None
            for k in range(n):
                wk = wrap(th - chi_in[r, k], f) ** 2
                wk = wk.reshape([g if q == k else 1 for q in range(n)])
                w = wk if w is None else w + wk
            J = E + (np.broadcast_to(w, [g] * n).reshape(-1) / (f(sigma_chi) * f(sigma_chi)))
        out["Jall"][r] = J
        J = np.where(E <= thr, J, f(np.inf))
        k = int(np.argmin(J))                                  # the first minimum: the lowest flat index
        out["J"][r], out["thr"][r], out["pick"][r] = J, thr, k
        if not np.isfinite(J[k]):
            status[r] = -2 if r in bad else -1
            continue
        digits = np.unravel_index(k, [g] * n)
        if chi_out is not None:
            chi_out[r, :n] = theta(g, np.float32)[list(digits)]
        report[r] = (emin, E[k], D[0, k], ANG[0, k])
        arep[idx, 0], arep[idx, 1] = D[:, k], ANG[:, k]
        status[r] = -2 if r in bad else 1
    count = np.array([int(((status == 1) & (seg_of == s)).sum()) for s in range(len(seg_offs) - 1)], np.int64)
    out.update(status=status, report=report, anchor_report=arep, count=count, chi=chi_out, bad=bad)
    return out


def place_target(xyz_row, slot, ante, d0, theta0, azimuth):
    """A point at ``d0`` from the atom in ``slot`` at ``theta0`` degrees to its antecedent, at ``azimuth`` (radians) about the bond:
    how the tests synthesise a site from native coordinates (float64)."""
    A, P = np.asarray(xyz_row[slot], np.float64), np.asarray(xyz_row[ante], np.float64)
    u = (P - A) / np.linalg.norm(P - A)
    h = np.cross(u, [1.0, 0.0, 0.0]) if abs(u[0]) < 0.9 else np.cross(u, [0.0, 1.0, 0.0])
    h /= np.linalg.norm(h)
    k = np.cross(u, h)
    t = np.radians(theta0)
    return A + d0 * (np.cos(t) * u + np.sin(t) * (np.cos(azimuth) * h + np.sin(azimuth) * k))
