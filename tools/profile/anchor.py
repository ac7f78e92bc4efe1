"""pp_anchor_close on 2FTL (tests/golden/g0_protein_2FTL.npz, 280 rows) with synthetic sites: the timing tool of DESIGN.md section 34.

    python tools/profile/anchor.py --out profiles/r34_anchor.json      # HIP events, five repetitions after a warm-up

Every anchored row carries one anchor on its last side-chain atom that a chi angle moves (so the rows mix n = 1 .. 4), with the target
2.1 A from that atom of the structure rebuilt at its own angles, at 120 degrees to its antecedent.  4 and 32 anchored rows are the
first rows with such an atom, "all" is every one of them (glycine and alanine have none).  The time is that of the whole
``Context.anchors`` call without its host-side check -- the memsets, the copy of chi and the launches -- from angles 30 degrees
off, on the complex alone and on its 16-decoy replicate (``batch.replicate``: a decoy is a segment, its anchors are repeated per
decoy).  A record only: nothing asserts these numbers."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def load_2ftl():
    from packppi_amd.featurize import protein_to_batch
    z = np.load(os.path.join(ROOT, "tests", "golden", "g0_protein_2FTL.npz"))
    return protein_to_batch({k[5:]: z[k] for k in z.files if k.startswith("prot.")})


def place(xyz_row, slot, ante, d0, theta0, azimuth):
    A, P = xyz_row[slot], xyz_row[ante]
    u = (P - A) / np.linalg.norm(P - A)
    h = np.cross(u, [1.0, 0.0, 0.0]) if abs(u[0]) < 0.9 else np.cross(u, [0.0, 1.0, 0.0])
    h /= np.linalg.norm(h)
    k = np.cross(u, h)
    t = np.radians(theta0)
    return A + d0 * (np.cos(t) * u + np.sin(t) * (np.cos(azimuth) * h + np.sin(azimuth) * k))


def sites(b, xyz):
    """One entry per row of the complex that has a chi-moved side-chain atom, in row order."""
    from packppi_amd import constants as rc
    rt = b.residue_type.reshape(-1).cpu().numpy()
    am = b.atom_mask.reshape(-1, 14).cpu().numpy()
    rng = np.random.default_rng(0)
    out = []
    for r in range(rt.size):
        ok = [s for s in range(5, 14) if rt[r] < 20 and am[r, s] != 0 and 4 <= rc.atom14_to_group[rt[r], s] <= 7]
        if ok and am[r, :5].all():
            ante = rc.anchor_antecedent(int(rt[r]), ok[-1])
            out.append((r, ok[-1], ante, place(xyz[r], ok[-1], ante, 2.1, 120.0, float(rng.uniform(0, 2 * np.pi))), (2.1, 0.1, 120.0, 15.0),
                        f"row {r}", "metal"))
    return out


def run(reps):
    import torch
    from packppi_amd.batch import replicate
    from packppi_amd.functional import geometry_plan
    from packppi_amd.lib import Context
    from packppi_amd.selection import AnchorSet, anchor_set_of
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "repetitions": reps, "runs": {}}

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    b = load_2ftl().to(dev)
    L = int(b.X.shape[1])
    xyz = Context(geometry_plan(dev), b).atom14(b.SC_D).reshape(-1, 14, 3).double().cpu().numpy()
    every = sites(b, xyz)
    g = torch.Generator().manual_seed(1)
    for D in (1, 16):
        pb = b if D == 1 else replicate(b, D)
        ctx = Context(geometry_plan(dev), pb)
        noise = np.deg2rad(30.0) * torch.randn(pb.SC_D.shape, generator=g).to(dev)
        chi = ctx._chi(torch.remainder(pb.SC_D + noise + np.pi, 2 * np.pi) - np.pi)
        for want in (4, 32, len(every)):
            one = anchor_set_of(every[:want])
            a = AnchorSet.concat([one.shifted(d * L) for d in range(D)])
            arrays = a.device_arrays(dev)
            res = ctx._anchor_close(chi, None, *arrays, len(a), 10.0, np.deg2rad(20.0))
            status = res.status.cpu().numpy()
            ms = timed(lambda: ctx._anchor_close(chi, None, *arrays, len(a), 10.0, np.deg2rad(20.0)))
            key = f"2FTL_decoys_{D}_rows_{'all' if want == len(every) else want}"
            out["runs"][key] = {"rows": int(pb.X.shape[1]), "anchored_rows": len(a), "closed": int((status == 1).sum()),
                                "open": int((status == -1).sum()), "close_ms": ms, "median_close_ms": float(np.median(ms))}
            print(f"{key}: {len(a)} anchored rows, {int((status == 1).sum())} closed, {np.median(ms):.3f} ms", flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rec = run(a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
