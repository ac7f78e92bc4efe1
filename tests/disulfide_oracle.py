"""Disulfide bridges (pp_disulfide_close) restated with NumPy.  Not a test module: tests/test_disulfide_host.py
and tests/test_disulfide_gpu.py import it.

The ideal CB and the SG of every grid angle come from ``oracle.ref_cpu.atom14_coords`` -- the reconstruction pp_atom14 follows --,
in the precision asked for; the energy, the candidates, the greedy matching and the closure follow include/packppi_hip.h.  Run in
float32 it is what the device is compared with; run in float64 it is the arbiter, and the difference between the two is the
tolerance of that comparison."""
import numpy as np
import torch

from oracle import ref_cpu
from packppi_amd import constants as rc

G = 72
CYS = rc.restype_order["C"]


def theta(dtype=np.float32):
    """The grid: (dtype)(-pi + 2 pi k / 72), the double expression rounded once."""
    return np.array([-np.pi + 2 * np.pi * k / 72 for k in range(G)], dtype=np.float64).astype(dtype)


def eligible(batch):
    """bool [N] (rows flattened): cysteine, residue_mask set, N, CA, C and SG in atom_mask."""
    rt = np.asarray(batch["residue_type"]).reshape(-1)
    rm = np.asarray(batch["residue_mask"]).reshape(-1)
    am = np.asarray(batch["atom_mask"]).reshape(-1, 14)
    return (rt == CYS) & (rm != 0) & (am[:, 0] != 0) & (am[:, 1] != 0) & (am[:, 2] != 0) & (am[:, 5] != 0)


def tables(batch, rows, dtype, chi=None):
    """(CB [n, 3], SG [n, 72, 3], SG at the rows' own chi1 [n, 3] or None) of ``rows`` through atom14_coords, in ``dtype``."""
    td = torch.float32 if dtype == np.float32 else torch.float64
    rows = np.asarray(rows, dtype=np.int64)
    X = torch.as_tensor(np.asarray(batch["X"])).reshape(-1, 14, 3)[rows].to(td)[None]
    S = torch.as_tensor(np.asarray(batch["residue_type"])).reshape(-1)[rows].long()[None]
    BB = torch.as_tensor(np.asarray(batch["BB_D"])).reshape(-1, 3)[rows].to(td)[None]
    th = torch.as_tensor(theta(dtype))
    n = len(rows)
    sg = np.zeros((n, G, 3), dtype)
    cb = np.zeros((n, 3), dtype)
    for k in range(G):
        sc = torch.zeros(1, n, 4, dtype=td)
        sc[..., 0] = th[k]
        xyz = ref_cpu.atom14_coords(X, S, BB, sc)[0].numpy()
        sg[:, k] = xyz[:, 5]
        cb = xyz[:, 4]
    own = None
    if chi is not None:
        sc = torch.zeros(1, n, 4, dtype=td)
        sc[..., 0] = torch.as_tensor(np.asarray(chi, dtype=dtype).reshape(-1, 4)[rows, 0])
        own = ref_cpu.atom14_coords(X, S, BB, sc)[0].numpy()[:, 5]
    return cb.astype(dtype), sg, own


def _dot(a, b):
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def _cross(a, b):
    return np.stack([(a[..., 1] * b[..., 2]) - (a[..., 2] * b[..., 1]), (a[..., 2] * b[..., 0]) - (a[..., 0] * b[..., 2]),
                     (a[..., 0] * b[..., 1]) - (a[..., 1] * b[..., 0])], -1)


def _angle(P, V, Q, f):
    u, v = P - V, Q - V
    c = _dot(u, v) / (np.sqrt(_dot(u, u)) * np.sqrt(_dot(v, v)))
    return np.arccos(np.clip(c, f(-1), f(1))) * f(180.0 / np.pi)


def energy(cba, A, B, cbb, want_geometry=False):
    """E of the definition for broadcastable [.., 3] arrays, in their dtype; with ``want_geometry`` also (distance, chi3 radians)."""
    f = A.dtype.type
    b1, b2, b3 = A - cba, B - A, cbb - B
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.sqrt(_dot(b2, b2))
        n1, n2 = _cross(b1, b2), _cross(b2, b3)
        dih = np.arctan2(d * _dot(b1, n2), _dot(n1, n2))
        e = ((d - f(2.04)) / f(0.10)) ** 2
        e = e + ((_angle(cba, A, B, f) - f(104)) / f(10)) ** 2
        e = e + ((_angle(cbb, B, A, f) - f(104)) / f(10)) ** 2
        e = e + (((np.abs(dih) * f(180.0 / np.pi)) - f(90)) / f(30)) ** 2
    e = np.where(np.isnan(e), f(np.inf), e)                     # a NaN (two atoms in one place) never wins a minimum, as on the device
    return (e, d, dih) if want_geometry else e


def pair_grid(cb, sg, i, j, want_geometry=False):
    """E [72, 72] (p of row i, q of row j)."""
    return energy(cb[i][None, None], sg[i][:, None], sg[j][None, :], cb[j][None, None], want_geometry)


def wrap(x, f):
    return x - np.rint(x / f(2 * np.pi)) * f(2 * np.pi)


def solve(batch, seg_offs, chi=None, fixed=None, pairs=None, cb_max=5.0, max_energy=10.0, sigma_chi=np.deg2rad(20.0),
          dtype=np.float32, tabs=None):
    """The definition, brute force.  Returns a dict: ``partner`` int [N], ``report`` [N, 4] (dtype), ``count`` [n_seg], ``chi``
    (None without chi), ``emin`` {(a, b): Emin} of every pair within cb_max (or listed), ``pick`` {(a, b): 72 p + q},
    ``J`` {(a, b): [72, 72] J over F, +inf outside}, ``E`` / ``D`` / ``X3`` {(a, b): the restricted grids of E, the SG-SG
    distance and chi3}, ``bonded`` the accepted pairs in the order of the matching."""
    f = dtype
    el = np.nonzero(eligible(batch))[0]
    N = np.asarray(batch["residue_type"]).size
    pos = {int(r): k for k, r in enumerate(el)}
    cb, sg, own = tabs if tabs is not None else tables(batch, el, dtype, chi)
    seg_of = np.searchsorted(np.asarray(seg_offs), np.arange(N), side="right") - 1
    th = theta(dtype)
    listed = pairs is not None
    me = f(np.inf) if listed else f(max_energy)
    emin = {}
    if listed:
        cand = [(min(a, b), max(a, b)) for a, b in pairs]
    else:
        cand = []
        for i, a in enumerate(el):
            for j in range(i + 1, len(el)):
                b = el[j]
                if seg_of[a] != seg_of[b]:
                    continue
                d = cb[j] - cb[i]
                if np.sqrt(_dot(d, d)) <= f(cb_max):
                    cand.append((int(a), int(b)))
    for a, b in cand:
        emin[(a, b)] = pair_grid(cb, sg, pos[a], pos[b]).min()
    partner = np.full(N, -1, np.int64)
    bonded = []
    for (a, b) in sorted((k for k in emin if emin[k] <= me), key=lambda k: (emin[k], k[0], k[1])):
        if partner[a] < 0 and partner[b] < 0:
            partner[a], partner[b] = b, a
            bonded.append((a, b))
    count = np.zeros(len(seg_offs) - 1, np.int64)
    report = np.zeros((N, 4), dtype)
    chi_out = None if chi is None else np.array(np.asarray(chi, dtype=np.float32).reshape(-1, 4), copy=True)
    chi_in = None if chi is None else np.asarray(chi, dtype=dtype).reshape(-1, 4)
    fx = np.zeros(N, bool) if fixed is None else (np.asarray(fixed).reshape(-1) != 0)
    pick, Js, Es, Ds, X3s = {}, {}, {}, {}, {}
    for a, b in bonded:
        count[seg_of[a]] += 1
        i, j = pos[a], pos[b]
        sa = np.repeat(own[i][None], G, 0) if fx[a] else sg[i]
        sb = np.repeat(own[j][None], G, 0) if fx[b] else sg[j]
        E, D, X3 = energy(cb[i][None, None], sa[:, None], sb[None, :], cb[j][None, None], True)
        er = E.min()
        thr = max(min(me, er + f(4)), er)
        J = E.copy()
        if chi is not None:
            wa = np.zeros(G, dtype) if fx[a] else wrap(th - chi_in[a, 0], f)
            wb = np.zeros(G, dtype) if fx[b] else wrap(th - chi_in[b, 0], f)
            J = E + (((wa * wa)[:, None] + (wb * wb)[None, :]) / (f(sigma_chi) * f(sigma_chi)))
        J = np.where(E <= thr, J, f(np.inf))
        k = int(np.argmin(J.reshape(-1)))                      # the first minimum: the lowest 72 p + q
        p, q = divmod(k, G)
        pick[(a, b)], Js[(a, b)], Es[(a, b)], Ds[(a, b)], X3s[(a, b)] = k, J, E, D, X3
        if chi_out is not None:
            if not fx[a]:
                chi_out[a, 0] = np.float32(theta(np.float32)[p])
            if not fx[b]:
                chi_out[b, 0] = np.float32(theta(np.float32)[q])
        report[a] = report[b] = (emin[(a, b)], E[p, q], D[p, q], X3[p, q])
    return dict(partner=partner, report=report, count=count, chi=chi_out, emin=emin, pick=pick, J=Js, E=Es, D=Ds, X3=X3s, bonded=bonded)
