"""PackPPI-AP throughput: an alanine scan of T1124's interface (network mode, seeded weights).

    python tools/profile/affinity_scan.py [--sets 64] [--reps 5] [--out FILE.json]

Mutation sets: the first --sets chain-A residues (not Ala / Gly) whose CA lies within 10 A of a chain-B CA, one
single-mutation set X->A each.  Reports mutation sets per second evaluated packed (AffinityPrediction.predict_many: one
packed context per branch) and one at a time (forward per set), and the packed run's split into the pretrained passes
(get_pret_feature, wild type + mutant), the mutation branch (local masks, its context, encode x 2) and the head
(k_affinity_head).  Each figure is the median of --reps timed runs after one warm-up, wall clock around a device
synchronisation.  For the kernels' own durations run it under `rocprofv3 --kernel-trace --stats -- python ...`.
"""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from packppi_amd import constants as rc  # noqa: E402
from packppi_amd.affinity import AffinityPrediction, mutant_view  # noqa: E402
from packppi_amd.batch import as_single, pack  # noqa: E402
from packppi_amd.featurize import mutant_data  # noqa: E402
from packppi_amd.pdb_io import from_pdb_file  # noqa: E402
from packppi_amd.weights import make_random_affinity_state_dict, make_random_state_dict  # noqa: E402


def scan_sets(prot, n):
    X = torch.from_numpy(prot["atom_positions"])[:, 1].float()
    ch, ri, aa = prot["chain_id"], prot["residue_index"], prot["aaindex"]
    a = torch.from_numpy(ch == "A")
    b = torch.from_numpy(ch == "B")
    near = (torch.cdist(X[a], X[b]).nan_to_num(1e9) < 10).any(1)
    rows = torch.nonzero(a).reshape(-1)[near].tolist()
    sets = []
    for r in rows:
        wt = rc.restypes[int(aa[r])] if int(aa[r]) < 20 else None
        if wt not in (None, "A", "G"):
            sets.append([{"wt": wt, "chain": "A", "resseq": int(ri[r]), "mt": "A"}])
    return sets[:n]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    with gzip.open(os.path.join(ROOT, "tests", "golden", "T1124_lig.pdb.gz"), "rt") as fh, \
            tempfile.NamedTemporaryFile("w", suffix=".pdb") as tmp:
        tmp.write(fh.read())
        tmp.flush()
        prot = from_pdb_file(tmp.name)
    sets = scan_sets(prot, args.sets)
    datas = [mutant_data(prot, s, log=lambda m: None) for s in sets]
    dev = "cuda:0"
    m = AffinityPrediction(make_random_affinity_state_dict(1), make_random_state_dict(1), mode="network", device=dev)
    singles = [as_single(d).to(dev) for d in datas]

    t_packed = timed(lambda: m.predict_many(datas), args.reps)
    t_single = timed(lambda: [m.forward(b) for b in singles], max(1, args.reps // 2))

    wt = pack(datas, trim=False).to(dev)
    mt = mutant_view(wt)
    def pret():
        m._contexts = []            # let the previous run's contexts go: their workspaces are reused, not reallocated
        return m.get_pret_feature(wt), m.get_pret_feature(mt)

    t_pret = timed(pret, args.reps)
    h_pw, h_pm = pret()

    def branch():
        m._contexts = m._contexts[:2]
        local = torch.cat([m.get_local_subgraph(b["X"][:, :, 1, :], b["mut_mask"]).reshape(-1) for b in singles]).unsqueeze(0)
        ctx = m._mutation_context(wt, local)
        return m.encode(wt, h_pw, ctx), m.encode(mt, h_pm, ctx)

    t_branch = timed(branch, args.reps)
    h_wt, h_mt = branch()
    t_head = timed(lambda: m.head.predict(h_wt, h_mt, wt["seg_offsets_host"]), args.reps)
    res = {"complex": "T1124", "residues": int(datas[0]["num_nodes"]), "sets": len(sets), "mode": "network",
           "edge_variant": int(__import__("packppi_amd.lib", fromlist=["load"]).load().pp_edge_variant()),
           "packed_s": t_packed, "packed_sets_per_s": len(sets) / t_packed,
           "one_at_a_time_s": t_single, "one_at_a_time_sets_per_s": len(sets) / t_single,
           "packed_split_s": {"pretrained_wt_mt": t_pret, "mutation_branch": t_branch, "head": t_head},
           "saturated": m.saturated(), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
