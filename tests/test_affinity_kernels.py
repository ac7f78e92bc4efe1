"""PackPPI-AP's kernels (k_affinity_embed in csrc/pp_node.hip, k_affinity_head in csrc/pp_affinity.hip, the mutation-branch
plan) against oracle/ref_affinity.py -- pinned to the unmodified reference by tests/test_affinity_oracle.py -- beyond the five
fixtures of tests/test_affinity_gpu.py: the head's pooling bit for bit and what include/packppi_hip.h promises for it, its MLP
against fp64, the mutation branch at every N % NB, local masks below K / up to 4K / over the whole complex, masked residues,
padded and packed batches, one context serving several encodes, weights outside the seeded draw, and all of it once more on
the exact-fp32 library.

Arithmetic is compared on the device's own neighbour lists (ctx.graph()): graph equality is tests/test_hip_parity.py's
subject.  Bounds against the fp64 oracle are max(the fixtures' bound, 3 x cond), cond = |fp32 oracle - fp64 oracle| of the same
case (the envelope convention of test_weight_range_envelope); both oracles use the build's self-edge dihedral convention
(exactly 0), which leaves less room than the reference's own arccos noise would.

Every figure is printed before it is asserted.  With PACKPPI_AFFINITY_PARITY_OUT=FILE.json the measured figures are also
written there (profiles/r10_affinity_parity.json is such a record).
"""
import json
import os
import re

import numpy as np
import pytest
import torch

from .conftest import ROOT, WEIGHT_SEED

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AFF_SEED = 20261016
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    yield
    torch.set_num_threads(n)
    out = os.environ.get("PACKPPI_AFFINITY_PARITY_OUT")
    if out and RECORD:
        with open(out, "w") as fh:
            json.dump(RECORD, fh, indent=1, sort_keys=True)


def note(key, **figs):
    print(f"{key}: " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in figs.items()))
    RECORD[key] = figs


def node_block_rows():
    """NB of csrc/pp_node.hip: rows per workgroup of k_affinity_embed, read from the source."""
    from packppi_amd.build import FLAGS
    assert not any("PP_NODE_GROUPS" in f for f in FLAGS)        # the product builds take the source's default
    src = open(os.path.join(ROOT, "packppi_amd", "csrc", "pp_node.hip")).read()
    groups = int(re.search(r"^#define PP_NODE_GROUPS (\d+)", src, re.M).group(1))
    assert re.search(r"^#define NG PP_NODE_GROUPS$", src, re.M)
    per = int(re.search(r"^#define NB \((\d+) \* NG\)", src, re.M).group(1))
    return per * groups


def same(a, b):
    """Bit-for-bit as numbers: equal, or NaN in both."""
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def dist(a, ref):
    return float((a.detach().cpu().double().reshape(-1) - ref.detach().cpu().double().reshape(-1)).abs().max())


def exact_library():
    from packppi_amd import lib as L
    return L.load().pp_edge_variant() == 0


# ---- the head ---------------------------------------------------------------------------------------------------------------------
def head_of(sd):
    from packppi_amd.lib import AffinityHead
    return AffinityHead(sd, DEV, "linear")


def selector(sign, f):
    """ddg_predictor that returns relu(sign * pooled[f]) exactly: every product is with 0 or 1, every sum adds zeros."""
    eye = torch.eye(128)
    w4 = torch.zeros(1, 128)
    w4[0, f] = 1.0
    return {"ddg_predictor.0.weight": sign * eye, "ddg_predictor.0.bias": torch.zeros(128),
            "ddg_predictor.2.weight": eye.clone(), "ddg_predictor.2.bias": torch.zeros(128),
            "ddg_predictor.4.weight": w4, "ddg_predictor.4.bias": torch.zeros(1)}


def seeded_head_sd(scale=1.0, positive=False):
    from packppi_amd.weights import make_random_affinity_state_dict
    sd = dict(make_random_affinity_state_dict(AFF_SEED, "linear"))
    for k in sd:
        if k.endswith("weight"):
            sd[k] = (sd[k].abs() if positive else sd[k]) * scale
    return sd


FEATURES = (0, 1, 63, 64, 127)
SEG_LENS = (1, 2, 3, 255, 256, 257, 50001, 2, 257, 1)      # >= 50 000 rows once; odd and even first rows for every short length


def test_head_pooling_bit_for_bit():
    """Per-segment max of h_mt - h_wt and of h_wt - h_mt through selector weights: torch.equal with fp32 torch, for 1-, 2-, 3-row
    segments, 255 / 256 / 257 rows and 50 001 rows, the maximum planted in the first, the last, an even and an odd row."""
    from oracle import ref_affinity as A
    offs = [0] + list(np.cumsum(SEG_LENS))
    n = offs[-1]
    g = torch.Generator().manual_seed(11)
    heads = {(sign, f): head_of(selector(sign, f)) for sign in (1.0, -1.0) for f in FEATURES}
    checked = 0
    for place in ("first", "last", "even", "odd", "none"):
        hw, hm = torch.randn(n, 128, generator=g), torch.randn(n, 128, generator=g)
        for a, ln in zip(offs[:-1], SEG_LENS):
            r = {"first": 0, "last": ln - 1, "even": 2 * (ln // 4), "odd": min(2 * (ln // 4) + 1, ln - 1), "none": None}[place]
            if r is not None:
                hm[a + r] += 16.0                                   # the max of h_mt - h_wt sits in this row, in every feature
                hw[a + (ln - 1 - r)] += 24.0                        # and that of h_wt - h_mt in the mirrored row
        fwd, inv = A.pooled(hw, hm, offs)                           # fp32 torch
        hwd, hmd = hw.to(DEV), hm.to(DEV)
        for (sign, f), hd in heads.items():
            ddg, dinv = hd.predict(hwd, hmd, offs)
            assert torch.equal(ddg.cpu(), torch.relu(sign * fwd[:, f])), (place, sign, f)
            assert torch.equal(dinv.cpu(), torch.relu(sign * inv[:, f])), (place, sign, f)
            checked += 2 * len(SEG_LENS)
    note("head_pooling_exact", values_compared=checked, rows=int(n))


def test_head_nan_and_inf_semantics():
    """torch.max / torch.relu semantics: a NaN in one row of one feature gives NaN for that segment only (the other segments keep
    their bits), whichever half of the workgroup reads the row; +-inf behave as in torch."""
    from oracle import ref_affinity as A
    lens = (5, 6, 7, 8)
    offs = [0] + list(np.cumsum(lens))
    g = torch.Generator().manual_seed(12)
    hw, hm = torch.randn(offs[-1], 128, generator=g), torch.randn(offs[-1], 128, generator=g)
    for tag, sd in (("seeded", seeded_head_sd()), ("positive", seeded_head_sd(positive=True))):
        hd = head_of(sd)
        base = [t.cpu() for t in hd.predict(hw.to(DEV), hm.to(DEV), offs)]
        assert all(bool(torch.isfinite(t).all()) for t in base)
        for seg in (0, 1, 3):
            for rel in (0, 1, lens[seg] - 1):                        # even rows: half 0, odd rows: half 1
                for which in ("mt", "wt"):
                    for f in (0, 77, 127):
                        for val in (float("nan"), float("inf"), float("-inf")):
                            w, m = hw.clone(), hm.clone()
                            (m if which == "mt" else w)[offs[seg] + rel, f] = val
                            ddg, inv = [t.cpu() for t in hd.predict(w.to(DEV), m.to(DEV), offs)]
                            keep = [s for s in range(len(lens)) if s != seg]
                            assert torch.equal(ddg[keep], base[0][keep]) and torch.equal(inv[keep], base[1][keep])
                            ref, ref_inv = A.head(sd, w, m, offs)          # fp32 torch
                            if val != val:
                                assert bool(ddg[seg].isnan()) and bool(inv[seg].isnan()), (tag, seg, rel, which, f)
                                assert bool(ref[seg].isnan()) and bool(ref_inv[seg].isnan())
                            for got, want in ((ddg[seg], ref[seg]), (inv[seg], ref_inv[seg])):
                                if bool(torch.isfinite(want)):
                                    assert abs(float(got) - float(want)) <= 1e-4 + 1e-4 * abs(float(want)), (tag, seg, rel, which, f, val)
                                else:
                                    assert same(got, want), (tag, seg, rel, which, f, val, float(got), float(want))
    note("head_nan_inf", cases=2 * 3 * 3 * 2 * 3 * 3)


def test_head_empty_segment():
    """An empty segment pools to -inf in every feature: ddg_predictor(full(-inf)) as torch computes it, NaN or +-inf included."""
    from oracle import ref_affinity as A
    g = torch.Generator().manual_seed(13)
    hw, hm = torch.randn(11, 128, generator=g), torch.randn(11, 128, generator=g)
    seen = set()
    for tag, sd in (("seeded", seeded_head_sd()), ("positive", seeded_head_sd(positive=True)), ("selector", selector(1.0, 5)),
                    ("selector -", selector(-1.0, 5))):
        hd = head_of(sd)
        for offs in ([0, 5, 5, 11], [0, 0], [11, 11], [0, 0, 0, 11, 11]):
            ddg, inv = [t.cpu() for t in hd.predict(hw.to(DEV), hm.to(DEV), offs)]
            ref, ref_inv = A.head(sd, hw, hm, offs)
            for s in range(len(offs) - 1):
                empty = offs[s] == offs[s + 1]
                for got, want in ((ddg[s], ref[s]), (inv[s], ref_inv[s])):
                    if bool(torch.isfinite(want)):
                        assert abs(float(got) - float(want)) <= 1e-4 + 1e-4 * abs(float(want)), (tag, offs, s)
                    else:
                        assert empty and same(got, want), (tag, offs, s, float(got), float(want))
                    if empty:
                        seen.add("nan" if bool(want.isnan()) else "finite" if bool(torch.isfinite(want)) else "inf")
    assert "nan" in seen and "finite" in seen, seen
    note("head_empty_segment", outcomes=sorted(seen))


def test_head_device_offsets_are_clamped():
    """Offsets given as a DEVICE tensor skip the host check: negative, beyond n_rows and decreasing entries give the result of
    the clamped table, a = clamp(off[s], 0, n), b = clamp(off[s + 1], a, n).  Valid input by the header's contract."""
    n = 300
    g = torch.Generator().manual_seed(14)
    hw, hm = torch.randn(n, 128, generator=g).to(DEV), torch.randn(n, 128, generator=g).to(DEV)
    hd = head_of(seeded_head_sd(positive=True))                         # positive weights: an empty segment gives a finite number
    tables = [[-5, 400], [200, 100], [-3, -1], [n + 5, n + 9], [0, n], [-5, 100, 50], [250, 400, -1]]
    for n_seg in (1, 2, 1000, 4096):
        tables.append(torch.randint(-60, n + 60, (n_seg + 1,), generator=g).tolist())
    memo = {}
    for offs in tables:
        n_seg = len(offs) - 1
        ddg, inv = [t.cpu() for t in hd.predict(hw, hm, torch.tensor(offs, dtype=torch.int32, device=DEV))]
        assert ddg.shape == (n_seg,) and inv.shape == (n_seg,)
        want, want_inv = torch.empty(n_seg), torch.empty(n_seg)
        for s in range(n_seg):
            a = min(max(offs[s], 0), n)
            b = min(max(offs[s + 1], a), n)
            if (a, b) not in memo:
                d1, i1 = hd.predict(hw, hm, [a, b])                      # host-checked, already inside [0, n] and increasing
                memo[(a, b)] = (float(d1), float(i1))
            want[s], want_inv[s] = memo[(a, b)]
        assert same(ddg, want) and same(inv, want_inv), offs[:8]
    note("head_device_offsets", tables=len(tables), distinct_segments=len(memo))


def test_head_padding_row_wins_the_max():
    """Padding rows are part of the max (the reference's max sees them, AffinityPrediction.py:189): with every real-row difference
    negative in a feature the pooled value is the padding rows' exact 0."""
    from oracle import ref_affinity as A
    B, L, real = 3, 40, (40, 31, 17)
    g = torch.Generator().manual_seed(15)
    hw, hm = torch.randn(B, L, 128, generator=g), torch.randn(B, L, 128, generator=g)
    for b in range(B):
        hw[b, real[b]:] = 0
        hm[b, real[b]:] = 0
    f = 64
    hm[:, :, f] = hw[:, :, f] - torch.rand(B, L, generator=g) - 0.5      # h_mt - h_wt < 0 on every real row of feature f ...
    for b in range(B):
        hm[b, real[b]:, f] = 0                                           # ... and exactly 0 on the padding rows
    offs = [0, L, 2 * L, 3 * L]
    fwd, inv = A.pooled(hw, hm, offs)
    assert float(fwd[0, f]) < 0 and float(fwd[1, f]) == 0 and float(fwd[2, f]) == 0
    for sign in (1.0, -1.0):
        ddg, dinv = head_of(selector(sign, f)).predict(hw.to(DEV), hm.to(DEV), offs)
        assert torch.equal(ddg.cpu(), torch.relu(sign * fwd[:, f])) and torch.equal(dinv.cpu(), torch.relu(sign * inv[:, f]))
    sd = seeded_head_sd()
    ddg, dinv = head_of(sd).predict(hw.to(DEV), hm.to(DEV), offs)
    r64 = A.head(A.to_double(sd), hw.double(), hm.double(), offs)
    r32 = A.head(sd, hw, hm, offs)
    for name, got, w32, w64 in (("ddg", ddg, r32[0], r64[0]), ("ddg_inv", dinv, r32[1], r64[1])):
        d, cond = dist(got, w64), dist(w32, w64)
        note(f"head_padding_rows_{name}", distance=d, cond=cond)
        assert d <= max(1e-4 + 1e-4 * float(w64.abs().max()), 3 * cond)


def test_head_mlp_against_fp64():
    """ddg_predictor on random pooled vectors, inputs N(0,1) and x 1e-3 / x 1e3, seeded and rescaled weights: 36 cases in 9
    families (one input scale, one weight set).  Bound per family: 3 x the largest |fp32 oracle - fp64 oracle| of the family --
    measured on the reference arithmetic, never on the kernel."""
    from oracle import ref_affinity as A
    lens = (1, 2, 9, 64, 257)
    offs = [0] + list(np.cumsum(lens))
    failures = []
    for wname, wscale in (("seeded", 1.0), ("x4", 4.0), ("x1/32", 1 / 32.)):
        sd = seeded_head_sd(wscale)
        sd64 = A.to_double(sd)
        hd = head_of(sd)
        for sname, scale in (("1", 1.0), ("1e-3", 1e-3), ("1e3", 1e3)):
            conds, dists = [], []
            for case in range(4):
                g = torch.Generator().manual_seed(1000 * case + 17)
                hw, hm = torch.randn(offs[-1], 128, generator=g) * scale, torch.randn(offs[-1], 128, generator=g) * scale
                r32, r64 = A.head(sd, hw, hm, offs), A.head(sd64, hw.double(), hm.double(), offs)
                got = hd.predict(hw.to(DEV), hm.to(DEV), offs)
                conds.append(max(dist(r32[0], r64[0]), dist(r32[1], r64[1])))
                dists.append(max(dist(got[0], r64[0]), dist(got[1], r64[1])))
            bound = 3 * max(conds)
            note(f"head_mlp[weights {wname}, inputs x{sname}]", distance=max(dists), cond=max(conds), bound=bound)
            if not max(dists) <= bound:
                failures.append((wname, sname, max(dists), max(conds)))
    assert not failures, failures


# ---- the mutation branch ----------------------------------------------------------------------------------------------------------
_model = []


def weights():
    from packppi_amd.weights import make_random_affinity_state_dict, make_random_state_dict
    return make_random_affinity_state_dict(AFF_SEED, "network"), make_random_state_dict(WEIGHT_SEED)


def model():
    from packppi_amd.affinity import AffinityPrediction
    if not _model:
        _model.append(AffinityPrediction(*weights(), mode="network", device=DEV))
    return _model[0]


def pick_sites(prot, n_sites, layout, seed):
    """Row numbers of the residues to mutate.  ``clustered``: consecutive residues of chain A; ``far``: spread evenly over chain A;
    ``both``: spread evenly over the whole complex (both chains); ``origin`` / ``rim``: the residue nearest to / farthest from
    the origin."""
    L = len(prot["aaindex"])
    first_b = int(np.argmax(prot["chain_id"] != prot["chain_id"][0]))
    ca = np.nan_to_num(prot["atom_positions"][:, 1])
    if layout == "clustered":
        start = np.random.default_rng(seed).integers(0, first_b - n_sites)
        return [int(start + i) for i in range(n_sites)]
    if layout == "far":
        return [int(x) for x in np.linspace(0, first_b - 1, n_sites).round()]
    if layout == "both":
        return [int(x) for x in np.linspace(0, L - 1, max(n_sites, 2)).round()][:max(n_sites, 2)]
    r = np.linalg.norm(ca, axis=1)
    return [int(np.argmin(r) if layout == "origin" else np.argmax(r))]


def mutation_set(L, seed, n_sites, layout, ddg=0.5, hide=(), hide_site=False):
    """``featurize.mutant_data`` of a synthetic complex with ``n_sites`` substitutions.  ``hide``: offsets from the first site of
    residues that lose their CA (pdb_io's NaN for a missing atom; featurize masks the residue and zeroes its rows).
    ``hide_site``: the first mutated residue itself is masked afterwards, with its mut_mask kept."""
    from packppi_amd import constants as rc
    from packppi_amd import synth
    from packppi_amd.featurize import mutant_data
    prot = synth.make_complex(L, seed)
    sites = pick_sites(prot, n_sites, layout, seed)
    for off in hide:
        prot["atom_positions"][sites[0] + off, 1] = np.nan
    muts = []
    for i in sites:
        wt = int(prot["aaindex"][i])
        muts.append({"wt": rc.restypes[wt], "mt": rc.restypes[(wt + 7) % 20], "chain": str(prot["chain_id"][i]),
                     "resseq": int(prot["residue_index"][i])})
    d = mutant_data(prot, muts, ddg=ddg, log=lambda s: None)
    assert int(d["mut_mask"].sum()) == len(sites)
    if hide_site:
        j = sites[0]
        d["residue_mask"][j] = 0.0
        for k in ("X", "atom_mask", "SC_D", "SC_D_mask", "BB_D", "BB_D_mask", "BB_D_sincos", "SC_D_sincos", "atom_mask_mut",
                  "SC_D_mut", "SC_D_mask_mut", "SC_D_sincos_mut", "residue_type", "residue_type_mut", "residue_index", "chain_indices"):
            d[k][j] = 0
        for k in ("chi_1pi_periodic_mask", "chi_2pi_periodic_mask", "chi_1pi_periodic_mask_mut", "chi_2pi_periodic_mask_mut"):
            d[k][j] = False
    return d, sites


def device_run(m, b):
    """One forward's pieces on the device, plus the two contexts' neighbour lists."""
    from packppi_amd.affinity import mutant_view
    m._contexts = []
    mt = mutant_view(b)
    p_wt, p_mt = m.get_pret_feature(b), m.get_pret_feature(mt)
    local = m.get_local_subgraph(b["X"][:, :, 1, :], b["mut_mask"])
    ctx = m._mutation_context(b, local)
    out = {"h_wt": m.encode(b, p_wt, ctx).cpu(), "h_mt": m.encode(mt, p_mt, ctx).cpu(), "local": local.cpu(),
           "E_pret": m._contexts[0].graph()[0].cpu(), "E_mut": ctx.graph()[0].cpu()}
    assert torch.equal(out["E_pret"], m._contexts[1].graph()[0].cpu())          # the graph does not depend on the side chains
    assert m.saturated() == 0
    loss, ddg = m.forward(b)
    out["loss"], out["ddg"], out["ddg_inv"] = loss.cpu(), ddg.cpu(), m.last_ddg_inv.cpu()
    assert m.saturated() == 0
    return out


def oracle_run(ap, pret, b, dev):
    """fp32 and fp64 oracle of the same case on the device's neighbour lists and the reference's local mask."""
    from oracle import ref_affinity as A
    res = []
    with torch.no_grad():
        local = A.local_subgraph(b["X"][:, :, 1, :], b["mut_mask"])
        for a_sd, p_sd, bb in ((ap, pret, b), (A.to_double(ap), A.to_double(pret), A.to_double(b))):
            kw = dict(pret_static=dev["E_pret"], mut_static=dev["E_mut"], local_mask=local, zero_self_dihedral=True)
            h_wt, h_mt = A.features(a_sd, p_sd, bb, "network", **kw)
            B, L = bb["residue_type"].shape
            ddg, inv = A.head(a_sd, h_wt, h_mt, [i * L for i in range(B + 1)])
            res.append({"h_wt": h_wt, "h_mt": h_mt, "ddg": ddg.reshape(B, 1), "ddg_inv": inv.reshape(B, 1), "local": local})
    return res


def check_against_oracle(key, dev, o32, o64):
    """Every row, every complex of the batch: exact zeros outside the local mask, encode within max(1e-4, 3 cond) of fp64, ddg /
    ddg_inv within max(1e-4 + 1e-4 |ref|, 3 cond)."""
    assert torch.equal(dev["local"], o64["local"])
    outside = o64["local"] == 0
    for k in ("h_wt", "h_mt"):
        assert not dev[k][outside].any(), (key, k)
        d, cond = dist(dev[k], o64[k]), dist(o32[k], o64[k])
        note(f"{key} {k}", distance=d, cond=cond, local_rows=int(o64["local"].sum()), rows=int(outside.numel()))
        assert d <= max(1e-4, 3 * cond), (key, k, d, cond)
    for k in ("ddg", "ddg_inv"):
        d, cond = dist(dev[k], o64[k]), dist(o32[k], o64[k])
        note(f"{key} {k}", distance=d, cond=cond)
        assert d <= max(1e-4 + 1e-4 * float(o64[k].abs().max()), 3 * cond), (key, k, d, cond)


# (L, sites, layout, seed): every required length; the local mask of each is printed and its regime asserted below
SHAPES = [(33, 1, "clustered", 1), (47, 8, "both", 2), (64, 2, "both", 3), (65, 1, "origin", 4), (130, 8, "clustered", 5),
          (130, 2, "far", 6), (300, 2, "both", 7), (300, 1, "rim", 8), (739, 8, "both", 9), (1200, 8, "far", 10)]
_single = {}


def single_case(spec):
    """Device and oracle results of one B = 1 case, computed once per test run."""
    from packppi_amd.batch import as_single
    if spec not in _single:
        L, n_sites, layout, seed = spec
        d, _ = mutation_set(L, 500 + seed, n_sites, layout, ddg=0.25 * seed)
        b = as_single(d)
        ap, pret = weights()
        dev = device_run(model(), b.to(DEV))
        o32, o64 = oracle_run(ap, pret, b, dev)
        _single[spec] = (d, dev, o32, o64)
    return _single[spec]


def test_shapes_cover_every_block_tail_and_mask_regime():
    """The cases of test_mutation_branch_shapes: every N % NB occurs, local masks below K, between K and 4K and over the whole
    complex occur, sites sit on one chain and on both."""
    from oracle import ref_affinity as A
    from oracle.ref_cpu import TOP_K as K
    from packppi_amd.batch import as_single
    nb = node_block_rows()
    assert {s[0] % nb for s in SHAPES} == set(range(nb))            # a kernel with another NB needs further lengths here
    regimes, chains = set(), set()
    for L, n_sites, layout, seed in SHAPES:
        d, sites = mutation_set(L, 500 + seed, n_sites, layout)
        n_local = int(A.local_subgraph(as_single(d)["X"][:, :, 1, :], as_single(d)["mut_mask"]).sum())
        regimes.add("whole" if n_local == L else "below K" if n_local < K else "K..4K" if n_local <= 4 * K else "above 4K")
        chains.add(len({int(d["chain_indices"][i]) for i in sites}))
        print(f"L {L} sites {n_sites} {layout}: local mask {n_local} rows")
    assert {"whole", "below K", "K..4K"} <= regimes and chains == {1, 2}, (regimes, chains)


@pytest.mark.parametrize("spec", SHAPES, ids=lambda s: f"L{s[0]}_{s[1]}{s[2]}")
def test_mutation_branch_shapes(spec):
    d, dev, o32, o64 = single_case(spec)
    check_against_oracle(f"shape L{spec[0]} {spec[1]} {spec[2]}", dev, o32, o64)


@pytest.mark.parametrize("kind", ["masked_in_ball", "masked_site", "masked_at_origin"])
def test_mutation_branch_masked_residues(kind):
    """A residue masked mid-chain next to the mutation site; a mutated residue that is itself masked; a masked residue
    whose zeroed coordinates fall inside the ball of a site near the origin -- the local mask is not multiplied by residue_mask
    (AffinityPrediction.py:124-145), here as there."""
    from packppi_amd.batch import as_single
    if kind == "masked_in_ball":
        d, sites = mutation_set(130, 611, 1, "rim", hide=(1,))
        j = sites[0] + 1
    elif kind == "masked_site":
        d, sites = mutation_set(130, 612, 2, "clustered", hide_site=True)
        j = sites[0]
        assert int(d["mut_mask"][j]) == 1
    else:
        d, sites = mutation_set(130, 613, 1, "origin", hide=(3,))
        j = sites[0] + 3
    assert float(d["residue_mask"][j]) == 0 and not d["X"][j].any() and 0 < j < 129
    b = as_single(d)
    ap, pret = weights()
    dev = device_run(model(), b.to(DEV))
    if kind == "masked_in_ball":
        assert float(dev["local"][0, j]) == 0 and float(dev["local"][0, j - 1]) == 1 and float(dev["local"][0, j + 1]) == 1
    else:
        assert float(dev["local"][0, j]) == 1                          # residue_mask 0, local mask 1
    o32, o64 = oracle_run(ap, pret, b, dev)
    check_against_oracle(f"masks {kind}", dev, o32, o64)


@pytest.mark.parametrize("lengths", [(65, 47), (47, 130, 64)], ids=["B2", "B3"])
def test_mutation_branch_padded_batches(lengths):
    """Padded batches of unequal lengths: every row of every complex against the oracle of the padded batch, whose head keeps the
    padding rows in the max."""
    from packppi_amd.batch import collate_affinity
    sets = [mutation_set(L, 700 + i, 1 + i, "both" if i else "clustered", ddg=0.5 - i)[0] for i, L in enumerate(lengths)]
    b = collate_affinity(sets)
    ap, pret = weights()
    dev = device_run(model(), b.to(DEV))
    o32, o64 = oracle_run(ap, pret, b, dev)
    check_against_oracle(f"padded B{len(lengths)}", dev, o32, o64)
    from oracle import ref_affinity as A
    loss64 = float(A.forward(A.to_double(ap), A.to_double(pret), A.to_double(b), "network", pret_static=dev["E_pret"],
                             mut_static=dev["E_mut"], zero_self_dihedral=True)[0])
    note(f"padded B{len(lengths)} loss", value=float(dev["loss"]), fp64=loss64)
    assert abs(float(dev["loss"]) - loss64) <= 1e-4 * abs(loss64)


def test_predict_many_against_the_oracle_in_two_orders():
    """Eight sets from eight complexes of six different lengths through predict_many, in two orders: each set gets the oracle's answer for
    that set alone and, bit for bit, the ddg of its own single forward."""
    m = model()
    specs = [SHAPES[i] for i in (0, 1, 2, 3, 4, 6, 5, 7)]
    assert len({s[0] for s in specs}) >= 4
    cases = [single_case(s) for s in specs]
    for order in (list(range(len(specs))), [5, 2, 7, 0, 3, 6, 1, 4]):
        ddg, inv = m.predict_many([cases[i][0] for i in order])
        assert m.saturated() == 0
        for pos, i in enumerate(order):
            d, dev, o32, o64 = cases[i]
            assert torch.equal(ddg[pos].cpu(), dev["ddg"].reshape(())) and torch.equal(inv[pos].cpu(), dev["ddg_inv"].reshape(())), (order, pos)
            for k, got in (("ddg", ddg[pos]), ("ddg_inv", inv[pos])):
                dd, cond = dist(got, o64[k]), dist(o32[k], o64[k])
                note(f"predict_many order {order[0]} set L{specs[i][0]} {specs[i][2]} {k}", distance=dd, cond=cond)
                assert dd <= max(1e-4 + 1e-4 * float(o64[k].abs().max()), 3 * cond)


@pytest.mark.parametrize("L", [130, 2100], ids=["split_node_update", "plain_node_update"])
def test_one_context_serves_wild_type_and_mutant(L):
    """encode(wt), encode(mt), encode(wt) on one mutation context: the third equals the first, and encode(mt) first on a fresh
    context equals the second.  130 rows take the split middle-layer node update (h_V / h_V_alt swap), 2100 rows do not."""
    from packppi_amd.affinity import mutant_view
    from packppi_amd.batch import as_single
    m = model()
    b = as_single(mutation_set(L, 800 + L, 2, "both")[0]).to(DEV)
    mt = mutant_view(b)
    m._contexts = []
    p_wt, p_mt = m.get_pret_feature(b), m.get_pret_feature(mt)
    local = m.get_local_subgraph(b["X"][:, :, 1, :], b["mut_mask"])
    ctx = m._mutation_context(b, local)
    first, second, third = m.encode(b, p_wt, ctx).clone(), m.encode(mt, p_mt, ctx).clone(), m.encode(b, p_wt, ctx).clone()
    fresh = m.encode(mt, p_mt, m._mutation_context(b, local))
    assert not torch.equal(first, second)
    assert torch.equal(first, third) and torch.equal(fresh, second)
    assert m.saturated() == 0


def test_weights_outside_the_seeded_draw():
    """The families of tools/oracle/envelope_weights.py on PackPPI-AP's own tensors, in the mostly-masked regime of the mutation
    branch: same bounds against fp64, no saturation, and the rescaled kernel instances really run (rebalanced chains, LayerNorm
    operand scales).  A weight outside the f16 range is refused by pp_plan_create."""
    from packppi_amd.affinity import AffinityPrediction
    from packppi_amd.batch import as_single
    from tools.oracle.envelope_weights import affinity_envelope_variants
    ap0, pret = weights()
    b = as_single(mutation_set(96, 905, 2, "far", ddg=1.0)[0])
    rebalanced, ln_scaled = 0, 0
    for name, ap in affinity_envelope_variants(ap0).items():
        m = AffinityPrediction(ap, pret, mode="network", device=DEV)
        n_rb, n_ln = m.mutation_plan.rebalanced_chains(), m.mutation_plan.ln_scaled_features()
        print(f"envelope [{name}]: rebalanced chains {n_rb}, LayerNorm-scaled features {n_ln}")
        rebalanced, ln_scaled = max(rebalanced, n_rb), max(ln_scaled, n_ln)
        dev = device_run(m, b.to(DEV))
        o32, o64 = oracle_run(ap, pret, b, dev)
        check_against_oracle(f"envelope [{name}]", dev, o32, o64)
    if not exact_library():             # include/packppi_hip.h: both counts are always 0 in the exact-fp32 build
        assert rebalanced > 0 and ln_scaled > 0, (rebalanced, ln_scaled)
    bad = dict(ap0)
    bad["mutation_mpnn.mpnn_layers.1.edge_dense.W_in.weight"] = ap0["mutation_mpnn.mpnn_layers.1.edge_dense.W_in.weight"] * 1e7
    with pytest.raises(RuntimeError, match="f16 range"):
        AffinityPrediction(bad, pret, mode="network", device=DEV)


def test_library_variant_is_the_requested_one():
    """PACKPPI_EXPECT_VARIANT (set by test_fp32_variant_library_affinity's child run): the loaded library really is that build."""
    from packppi_amd import lib as L
    want = os.environ.get("PACKPPI_EXPECT_VARIANT")
    got = L.load().pp_edge_variant()
    assert got in (0, 1) and (want is None or got == int(want))


def test_fp32_variant_library_affinity():
    """This file and the fixtures' forward once more on the exact-fp32 library (fp32 MFMA edge kernels, VALU node update): one
    child test run with PACKPPI_LIB."""
    import subprocess
    import sys
    from packppi_amd.build import other_variant_path
    lib = other_variant_path()
    if os.environ.get("PACKPPI_LIB"):
        pytest.skip("already a child run")
    if not os.path.exists(lib):
        pytest.skip(f"{os.path.basename(lib)} not built (__graft_entry__.build() builds it)")
    env = dict(os.environ, PACKPPI_LIB=lib, PACKPPI_EXPECT_VARIANT="0" if lib.endswith(".f32.so") else "1")
    env.pop("PACKPPI_AFFINITY_PARITY_OUT", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_affinity_kernels.py"),
                        os.path.join(ROOT, "tests", "test_affinity_gpu.py") + "::test_forward_against_reference", "-q", "-x", "-m", "gpu",
                        "-p", "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=1100)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout
