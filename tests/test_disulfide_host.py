"""Disulfide bridges (pp_disulfide_close) on the CPU: the NumPy restatement of tests/disulfide_oracle.py on the
fixtures -- the figures the definition's defaults rest on --, and the host-side surfaces: the pair lists, the SSBOND records,
disulfides.csv and the argument rules of ``sampling`` / ``repack``."""
import functools
import os

import numpy as np
import pytest
import torch

from . import disulfide_oracle as O
from .conftest import GOLD, ROOT

NATIVE = ["E7-E136", "E25-E41", "E108-E209", "E115-E182", "E147-E161", "E172-E196", "I5-I55", "I14-I38", "I30-I51"]


@functools.lru_cache(maxsize=None)
def fixture(tag, chain=None):
    """(protein dict, batch arrays as NumPy) of a g0 fixture, or of one chain of it."""
    z = np.load(os.path.join(GOLD, f"g0_protein_{tag}.npz"))
    prot = {k[5:]: z[k] for k in z.files if k.startswith("prot.")}
    ref = {k[4:]: z[k] for k in z.files if k.startswith("ref.")}
    if chain is not None:
        keep = prot["chain_id"] == chain
        prot = {k: v[keep] for k, v in prot.items()}
        ref = {k: v[keep] for k, v in ref.items()}
    return prot, ref


def name(prot, row):
    return f"{prot['chain_id'][row]}{int(prot['residue_index'][row])}"


def named(prot, pairs):
    return sorted((f"{name(prot, a)}-{name(prot, b)}" for a, b in pairs), key=NATIVE.index)


@functools.lru_cache(maxsize=None)
def solved(tag, chain, dtype, **kw):
    prot, b = fixture(tag, chain)
    return O.solve(b, [0, len(b["residue_type"])], chi=b["SC_D"], dtype=dtype, **kw)


# ---- the restatement on the fixtures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_2FTL_native_bridges_and_only_those(dtype):
    prot, b = fixture("2FTL")
    r = solved("2FTL", None, dtype)
    assert named(prot, r["bonded"]) == NATIVE and r["count"].tolist() == [9]
    emin = sorted(float(v) for v in r["emin"].values())
    assert len(emin) == 9 and 0.1 < emin[0] and emin[-1] < 2.4                 # 0.13 .. 2.32, far below max_energy = 10
    # the best candidate that is rejected: visible with a wider cb_max, and far above max_energy (I51-I55, Emin 131)
    wide = solved("2FTL", None, dtype, cb_max=6.0)
    rejected = {k: float(v) for k, v in wide["emin"].items() if k not in r["emin"]}
    best = min(rejected, key=rejected.get)
    assert f"{name(prot, best[0])}-{name(prot, best[1])}" == "I51-I55" and 120 < rejected[best] < 140
    assert sorted(wide["bonded"]) == sorted(r["bonded"])
    # SG-SG of the closed bridges, and what the closure did to the fixture's own angles
    rows = [a for a, _ in r["bonded"]]
    d = r["report"][rows, 2]
    assert 1.96 < d.min() and d.max() < 2.13
    chi0 = b["SC_D"].reshape(-1, 4)
    moved = np.abs(O.wrap(r["chi"][:, 0].astype(np.float64) - chi0[:, 0], np.float64))
    assert np.rad2deg(moved.max()) < 20.0 and 7.0 < np.rad2deg(moved.max()) < 7.6      # the reference's accuracy criterion; 7.3 deg
    bonded = r["partner"] >= 0
    assert bonded.sum() == 18 and not moved[~bonded].any()
    assert np.array_equal(r["chi"][:, 1:].view(np.uint32), chi0[:, 1:].view(np.uint32))
    assert np.array_equal(r["chi"][~bonded].view(np.uint32), chi0[~bonded].view(np.uint32))


def test_geometric_optimum_alone_is_ambiguous():
    """Why the closure reads the sample: the argmin of E lies 45 deg or more from the native chi1 on several of the nine pairs."""
    prot, b = fixture("2FTL")
    r = O.solve(b, [0, 280], dtype=np.float64)                    # detection only: J = E
    th = O.theta(np.float64)
    chi0 = b["SC_D"].reshape(-1, 4)
    far = 0
    for (a, c), k in r["pick"].items():
        p, q = divmod(k, O.G)
        dev = max(abs(O.wrap(th[p] - chi0[a, 0], np.float64)), abs(O.wrap(th[q] - chi0[c, 0], np.float64)))
        far += np.rad2deg(dev) > 45
    assert far == 4


def test_1BRS_has_no_bridge():
    prot, b = fixture("1BRS")
    assert not (b["residue_type"] == O.CYS).any()
    r = solved("1BRS", None, np.float32)
    assert r["bonded"] == [] and not r["emin"] and (r["partner"] == -1).all() and not r["report"].any() and r["count"].tolist() == [0]
    assert r["chi"].tobytes() == np.ascontiguousarray(b["SC_D"].reshape(-1, 4)).tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_greedy_matching_drops_the_bridge_between_two_bonded_rows(dtype):
    prot, b = fixture("2FTL", "I")
    r = solved("2FTL", "I", dtype, cb_max=6.0, max_energy=200.0)
    row = {int(n): k for k, n in enumerate(prot["residue_index"])}
    assert (row[51], row[55]) in r["emin"] and float(r["emin"][(row[51], row[55])]) <= 200.0       # now a candidate
    assert named(prot, r["bonded"]) == ["I5-I55", "I14-I38", "I30-I51"] and r["count"].tolist() == [3]


def test_pairs_never_cross_segments():
    """Chain I twice, same coordinates: a row and its copy would be the best pair of all."""
    prot, b = fixture("2FTL", "I")
    two = {k: np.concatenate([v, v]) for k, v in b.items()}
    r = O.solve(two, [0, 58, 116], chi=two["SC_D"])
    assert r["count"].tolist() == [3, 3] and all((a < 58) == (c < 58) for a, c in r["bonded"])
    one = O.solve(two, [0, 116], chi=two["SC_D"], max_energy=1e9)
    assert any((a < 58) != (c < 58) for a, c in one["bonded"])


# ---- pair lists ----------------------------------------------------------------------------------------------------------------------------
def test_parse_disulfides_and_its_refusals():
    from packppi_amd.selection import parse_disulfides, residue_names
    prot, b = fixture("2FTL")
    r = solved("2FTL", None, np.float32)
    spec = ",".join(s.replace("E", "E:").replace("I", "I:") for s in NATIVE)
    assert spec.startswith("E:7-E:136,")
    assert sorted(parse_disulfides(spec, prot)) == sorted(r["bonded"])
    assert parse_disulfides([(("I", 5), ("I", 55))], prot) == parse_disulfides(" I:5-I:55 ", prot)
    assert residue_names(prot)[0] == ("E", int(prot["residue_index"][0]))
    neg = dict(chain_id=np.array(["A", "A"]), residue_index=np.array([-3, 12]))
    assert parse_disulfides("A:-3-A:12", neg) == [(0, 1)]
    for bad in ("I:5", "I5-I55", "I:5-I:55-I:51", "I:5-I:x", ""):
        with pytest.raises(ValueError, match="expected CHAIN:N-CHAIN:M|empty"):
            parse_disulfides(bad, prot)
    with pytest.raises(ValueError, match="no residue Q:5"):
        parse_disulfides("Q:5-I:55", prot)
    with pytest.raises(ValueError, match="no residue I:999"):
        parse_disulfides("I:5-I:999", prot)
    twice = dict(chain_id=np.array(["A", "A", "A"]), residue_index=np.array([5, 5, 9]))
    with pytest.raises(ValueError, match="2 rows carry A:5"):
        parse_disulfides("A:5-A:9", twice)


class _Rows:
    """``Context.check_disulfide_pairs`` on a stand-in ``self``: the rule runs on the host."""

    def __init__(self, elig, offs):
        self._e, self.seg_offsets_host, self.n_rows = elig, offs, len(elig)

    def disulfide_eligible(self):
        return torch.tensor(self._e)


def test_pair_list_refusals_name_the_offender():
    from packppi_amd.lib import Context
    ctx = _Rows([True, True, False, True, True, True], [0, 4, 6])
    check = lambda pairs, names=None: Context.check_disulfide_pairs(ctx, pairs, names)
    assert check([(1, 0), (4, 5)]) == [(0, 1), (4, 5)]
    with pytest.raises(ValueError, match="A:7 is not a cysteine"):
        check([(0, 2)], ["A:5", "A:6", "A:7", "A:8", "B:1", "B:2"])
    with pytest.raises(ValueError, match="row 3 and row 4 lie in two segments"):
        check([(3, 4)])
    with pytest.raises(ValueError, match="row 1 is named twice"):
        check([(0, 1), (1, 3)])
    with pytest.raises(ValueError, match="row 9 is outside"):
        check([(0, 9)])


# ---- the texts -----------------------------------------------------------------------------------------------------------------------------
def test_ssbond_records():
    from packppi_amd.pdb_io import ssbond_records, to_pdb
    prot, b = fixture("2FTL")
    r = solved("2FTL", None, np.float32)
    pairs = sorted(r["bonded"])
    text = ssbond_records(prot, pairs, [r["report"][a, 2] for a, _ in pairs])
    lines = text.splitlines()
    assert len(lines) == 9 and all(len(ln) == 80 for ln in lines) and text.endswith("\n")
    assert lines[0].rstrip() == "SSBOND   1 CYS E    7    CYS E  136                          1555   1555  " + f"{r['report'][pairs[0][0], 2]:.2f}"
    assert lines[8][:35] == "SSBOND   9 CYS I   30    CYS I   51"
    assert ssbond_records(prot, []) == ""
    assert ssbond_records(prot, pairs[:1]).rstrip().endswith("1555   1555")
    assert to_pdb(prot).startswith("MODEL")                       # to_pdb itself is as it was: the records go in front of its text


def test_disulfides_csv():
    from packppi_amd.cli.eval_diffusion import disulfides_csv
    prot, b = fixture("2FTL", "I")
    r = solved("2FTL", "I", np.float32)
    text, pairs = disulfides_csv(prot, r["partner"].tolist(), r["report"].tolist(), b["SC_D"].reshape(-1, 4)[:, 0].tolist(),
                                 r["chi"][:, 0].tolist())
    lines = text.splitlines()
    assert lines[0] == "chain,number,partner_chain,partner_number,emin,energy,sg_sg_distance,chi3,chi1_before,chi1_after"
    assert len(lines) == 7 and pairs == sorted(r["bonded"])
    a, c = pairs[0]
    f = lines[1].split(",")
    assert f[:4] == ["I", "5", "I", "55"] and lines[-1].split(",")[:4] == ["I", "55", "I", "5"]
    assert float(f[4]) == pytest.approx(float(r["report"][a, 0]), abs=1e-4) and float(f[6]) == pytest.approx(float(r["report"][a, 2]), abs=1e-4)
    assert float(f[9]) == pytest.approx(np.rad2deg(float(r["chi"][a, 0])), abs=0.01)


def test_command_line_takes_the_flag():
    from packppi_amd.cli import eval_diffusion as mod
    from .test_guided_host import BASE, TODAY
    p = mod.build_parser()
    plain = p.parse_args(BASE["eval_diffusion"])
    assert sorted(vars(plain)) == TODAY["eval_diffusion"] and mod.disulfides_from_args(plain) is None
    a = p.parse_args(BASE["eval_diffusion"] + ["--disulfides", "auto"])
    assert mod.disulfides_from_args(a, p) == "auto"
    prot, _ = fixture("2FTL", "I")
    a = p.parse_args(BASE["eval_diffusion"] + ["--disulfides", "I:5-I:55"])
    assert mod.disulfides_from_args(a, p, prot) == [(4, 54)]
    with pytest.raises(SystemExit):
        mod.disulfides_from_args(p.parse_args(BASE["eval_diffusion"] + ["--disulfides", "auto", "--n_decoys", "4", "--seed", "1"]), p)


# ---- the argument rules of sampling(disulfides=) / repack(disulfides=) -------------------------------------------------------------------------
def test_sampling_and_repack_argument_rules():
    import inspect
    from packppi_amd.batch import Batch, collate
    from packppi_amd.module import TDiffusionModule
    from .test_guided_host import _Probe, complex_cpu
    b = complex_cpu(24, 5)
    run = lambda **kw: TDiffusionModule.sampling(_Probe("ode"), b, **kw)
    with pytest.raises(AssertionError, match="reached the device"):               # a valid request goes on to the context
        run(seed=1, disulfides="auto")
    with pytest.raises(AssertionError, match="reached the device"):
        run(seed=1, disulfides=[(3, 9)], use_proximal=True)
    with pytest.raises(ValueError, match="return_trajectory with disulfides"):
        run(seed=1, disulfides="auto", guide=0.02, return_trajectory=True)
    with pytest.raises(ValueError, match="return_list with disulfides"):
        run(seed=1, disulfides="auto", use_proximal=True, return_list=True)
    with pytest.raises(ValueError, match="needs batch.residue_names"):
        run(seed=1, disulfides="A:5-A:55")
    with pytest.raises(ValueError, match="expected CHAIN:N-CHAIN:M"):
        named = Batch(b)
        named["residue_names"] = [("A", k) for k in range(24)]
        TDiffusionModule.sampling(_Probe("ode"), named, seed=1, disulfides="A:5")
    # today's refusal stays, and points at repack
    with pytest.raises(ValueError, match="repack"):
        run(seed=1, disulfides="auto", use_proximal=True, fixed_mask=torch.zeros(1, 24, dtype=torch.bool))
    # a padded B > 1 batch is refused with the reason, as guide refuses it
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_data
    padded = collate([protein_to_data(synth.make_complex(24, 5)), protein_to_data(synth.make_complex(20, 3))])
    with pytest.raises(ValueError, match="disulfides needs a B = 1 batch or a packed one"):
        TDiffusionModule.sampling(_Probe("ode"), padded, seed=1, disulfides="auto")
    with pytest.raises(ValueError, match="disulfides needs a B = 1 batch or a packed one"):
        TDiffusionModule.repack(_Probe("ode"), padded, torch.zeros(2, 24, dtype=torch.bool), seed=1, disulfides="auto")
    for fn in ("sampling", "repack"):
        assert inspect.signature(getattr(TDiffusionModule, fn)).parameters["disulfides"].default is None
    for fn in ("sample_ensemble", "repack_ensemble", "mutate"):                   # out of scope, DESIGN.md section 26
        assert "disulfides" not in inspect.signature(getattr(TDiffusionModule, fn)).parameters


def test_header_binding_and_build_list_name_the_export():
    import re
    from packppi_amd import build, constants as rc, lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "packppi_hip.h")).read(), flags=re.S)
    decl = re.search(r"pp_status pp_disulfide_close\((.*?)\);", src, flags=re.S)
    assert decl is not None and decl.group(1).count(",") == 12
    assert "pp_disulfide_close" in lib.SYMBOLS
    assert int(re.search(r"#define PP_RESTYPE_CYS (\d+)", src).group(1)) == rc.restype_order["C"] == O.CYS
    for edge_f16 in (True, False):
        assert "pp_disulfide.hip" in build.sources_for(edge_f16)
