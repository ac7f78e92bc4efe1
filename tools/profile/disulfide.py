"""pp_disulfide_close on 2FTL (tests/golden/g0_protein_2FTL.npz: 280 rows, 18 cysteines, 9 bridges) and on T1124
(tests/golden/T1124_lig.pdb.gz): the record behind DESIGN.md section 26.

    python tools/profile/disulfide.py --out profiles/r26_disulfide.json      # HIP events, five repetitions after a warm-up

The time is that of the whole ``Context.disulfides`` call from the structure's own angles -- three memsets, the copy of chi and the six
launches -- on the complex alone and on its 16-decoy replicate (``batch.replicate``: a decoy is a segment).  A record only: nothing
asserts these numbers."""
import argparse
import gzip
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def load_2ftl():
    from packppi_amd.featurize import protein_to_batch
    z = np.load(os.path.join(ROOT, "tests", "golden", "g0_protein_2FTL.npz"))
    return protein_to_batch({k[5:]: z[k] for k in z.files if k.startswith("prot.")})


def load_t1124():
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.pdb_io import from_pdb_file
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "T1124_lig.pdb")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "T1124_lig.pdb.gz"), "rt") as fh, open(path, "w") as out:
            out.write(fh.read())
        return protein_to_batch(from_pdb_file(path))


def run(reps):
    import torch
    from packppi_amd.batch import replicate
    from packppi_amd.functional import geometry_plan
    from packppi_amd.lib import Context
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

    for name, load in (("2FTL", load_2ftl), ("T1124", load_t1124)):
        b = load().to(dev)
        for D in (1, 16):
            pb = b if D == 1 else replicate(b, D)
            ctx = Context(geometry_plan(dev), pb)
            res = ctx.disulfides(chi=pb.SC_D)
            ms = timed(lambda: ctx.disulfides(chi=pb.SC_D))
            det = timed(lambda: ctx.disulfides())
            out["runs"][f"{name}_decoys_{D}"] = {
                "rows": int(pb.X.shape[1]), "cysteines": int(ctx.disulfide_eligible().sum()), "bridges": res.count.cpu().tolist(),
                "close_ms": ms, "median_close_ms": float(np.median(ms)), "detect_only_ms": det, "median_detect_only_ms": float(np.median(det))}
            print(f"{name} x {D}: {int(pb.X.shape[1])} rows, {int(res.count.sum())} bridges, close {np.median(ms):.3f} ms, "
                  f"detect {np.median(det):.3f} ms", flush=True)
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
