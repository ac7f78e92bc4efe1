"""Decoy ensembles, the host side: the decoy keys, the replicated batches, the command line's refusals and
the new C entry in header, binding and library.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = (33, 40)


def splitmix_np(k, d):
    """decoy_key restated on NumPy uint64 arrays (wrapping arithmetic): k, d arrays of the same shape, d >= 1."""
    with np.errstate(over="ignore"):
        z = np.asarray(k, dtype=np.uint64) + np.asarray(d, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


@pytest.fixture(scope="module")
def complexes():
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    return [protein_to_batch(synth.make_complex(n, 70 + n)) for n in LENS]


def test_decoy_key():
    from packppi_amd.batch import decoy_key
    for k in (0, 7, 2 ** 40 + 3, 2 ** 64 - 1):
        assert decoy_key(k, 0) == k
    # SplitMix64's own stream: seeded with 0, its first outputs are the finaliser of 1 * gamma, 2 * gamma ... (Vigna's splitmix64.c)
    assert [decoy_key(0, d) for d in (1, 2, 3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    ks = np.array([0, 7, 2 ** 40 + 3, 2 ** 63 + 5, 2 ** 64 - 1], dtype=np.uint64)
    for d in (1, 2, 9, 1000):
        want = splitmix_np(ks, np.full(ks.shape, d))
        assert [decoy_key(int(k), d) for k in ks] == [int(w) for w in want]
    assert decoy_key(-1, 0) == 2 ** 64 - 1 and 0 <= decoy_key(-1, 3) < 2 ** 64         # negative keys wrap like the sampler's
    with pytest.raises(ValueError):
        decoy_key(7, -1)


def test_decoy_keys_are_distinct():
    """100 base keys (small ones, 2**40 + small ones, as the tests of the seeded sampler use them) x 100 decoys: 10**4 different keys."""
    from packppi_amd.batch import decoy_key
    base = list(range(50)) + [2 ** 40 + i for i in range(50)]
    keys = {decoy_key(k, d) for k in base for d in range(100)}
    assert len(keys) == 10 ** 4


def test_replicate(complexes):
    from packppi_amd.batch import TENSOR_KEYS, decoy_key, replicate, unpack
    c = complexes[0]
    pb = replicate(c, 3)
    assert pb.n_decoys == 3 and pb.n_groups == 1 and pb.num_proteins == 1 and pb.max_size == 99
    assert pb.seg_offsets_host == [0, 33, 66, 99] and pb.seg_offsets.tolist() == [0, 33, 66, 99]
    assert pb.complex_keys == [decoy_key(0, d) for d in range(3)] and pb.complex_keys[0] == 0
    for k in TENSOR_KEYS:
        for part in unpack(pb, pb[k]):
            assert torch.equal(part, c[k])
    assert replicate(c, 3, key=7).complex_keys == [decoy_key(7, d) for d in range(3)]
    keyed = type(c)(c)
    keyed["complex_keys"] = [2 ** 40 + 3]                      # a B = 1 batch as sampling(seed=...) reads its key
    assert replicate(keyed, 2).complex_keys == [2 ** 40 + 3, decoy_key(2 ** 40 + 3, 1)]
    keyed = type(c)(c)
    keyed["complex_key"] = 11
    assert replicate(keyed, 2).complex_keys == [11, decoy_key(11, 1)]
    one = replicate(c, 1)
    assert one.seg_offsets_host == [0, 33] and one.complex_keys == [0] and one.n_decoys == 1
    for bad in (0, -2):
        with pytest.raises(ValueError, match="n_decoys"):
            replicate(c, bad)


def test_replicate_many(complexes):
    from packppi_amd.batch import check_groups, decoy_key, replicate_many, unpack
    pb = replicate_many(complexes, 5)
    assert pb.n_decoys == 5 and pb.n_groups == 2 and pb.max_size == 365
    assert pb.seg_offsets_host == [33 * i for i in range(6)] + [165 + 40 * i for i in range(1, 6)]
    assert pb.complex_keys == [decoy_key(g, d) for g in range(2) for d in range(5)]          # no complex_key: the ordinal
    parts = unpack(pb, pb.SC_D)
    for g, c in enumerate(complexes):
        for d in range(5):
            assert torch.equal(parts[g * 5 + d], c.SC_D)                                     # group-major
    keyed = []
    for c, k in zip(complexes, (7, 2 ** 40 + 3)):
        c = type(c)(c)
        c["complex_key"] = k
        keyed.append(c)
    assert replicate_many(keyed, 2).complex_keys == [7, decoy_key(7, 1), 2 ** 40 + 3, decoy_key(2 ** 40 + 3, 1)]
    assert check_groups(pb.seg_offsets_host, 5) == [33, 40]
    # the refusals: keys that collide, no decoys, no complexes, and tables that are not groups of equal copies
    with pytest.raises(ValueError, match="distinct"):
        replicate_many([keyed[0], keyed[0]], 2)
    with pytest.raises(ValueError, match="distinct"):
        replicate_many(complexes, 2, keys=[0, decoy_key(0, 1)])
    with pytest.raises(ValueError, match="n_decoys"):
        replicate_many(complexes, 0)
    with pytest.raises(ValueError):
        replicate_many([], 2)
    with pytest.raises(ValueError, match="differ in length"):
        check_groups([0, 33, 73], 2)
    with pytest.raises(ValueError, match="groups of"):
        check_groups([0, 33, 66, 99], 2)


def test_cli_refusals(capsys):
    from packppi_amd.cli import eval_diffusion
    base = ["--input", "x.pdb", "--outdir", "out", "--molprobity_clash_loc", "/nonexistent"]
    with pytest.raises(SystemExit):
        eval_diffusion.parse_args(base + ["--n_decoys", "4"])
    assert "--n_decoys needs --seed" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        eval_diffusion.parse_args(base + ["--n_decoys", "4", "--seed", "1", "--repack", "interface"])
    assert "--repack is not supported" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        eval_diffusion.parse_args(base + ["--n_decoys", "0", "--seed", "1"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        eval_diffusion.parse_args(base + ["--n_decoys", "2", "--seed", "1", "--select", "best"])
    capsys.readouterr()
    args = eval_diffusion.parse_args(base + ["--n_decoys", "4", "--seed", "1", "--use_proximal", "--select", "medoid"])
    assert args.n_decoys == 4 and args.select == "medoid" and args.use_proximal
    args = eval_diffusion.parse_args(base + ["--seed", "1"])
    assert args.n_decoys is None and args.select == "clash"


def test_sample_ensemble_needs_a_seed():
    """Refused before anything touches the device: the module is not even constructed."""
    from packppi_amd.module import TDiffusionModule
    with pytest.raises(ValueError, match="seed"):
        TDiffusionModule.sample_ensemble(object.__new__(TDiffusionModule), None, 3)


def test_header_binding_and_libraries_agree():
    from packppi_amd import build
    from packppi_amd.lib import SELECT, SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "packppi_hip.h")).read()
    diag = re.search(r"#ifdef PP_DIAG\n(.*?)#endif", hdr, flags=re.S)
    assert "pp_ensemble_reduce" in SYMBOLS
    assert re.search(r"pp_status\s+pp_ensemble_reduce\s*\(", hdr.replace(diag.group(0), "")) and "pp_ensemble_reduce" not in diag.group(1)
    for name, val in (("PP_SELECT_NONE", SELECT[None]), ("PP_SELECT_CLASH", SELECT["clash"]), ("PP_SELECT_MEDOID", SELECT["medoid"])):
        assert re.search(rf"#define {name} {val}\b", hdr)
    # the new file is a source of all four libraries, and every library that is built exports the entry
    assert "pp_ensemble.hip" in build.SOURCES and len(build.product_flag_stamps()) == 4
    assert build.embedded_build_id(build.build_library(verbose=False)) == build.build_id(build.FLAGS, build.SOURCES)
    for path in (build.LIB, build.other_variant_path(), build.check_variant_path(), build.diag_variant_path()):
        if os.path.exists(path):
            assert build.embedded_build_id(path).split("-")[1] in build.product_flag_stamps(), path
            assert hasattr(ctypes.CDLL(path), "pp_ensemble_reduce"), path


def test_reduce_refuses_bad_arguments_before_the_device():
    """PP_ERR_INVALID for a null context, checked before any device call (the other refusals need a context: the GPU tests)."""
    from packppi_amd import build
    lib = ctypes.CDLL(build.build_library(verbose=False))
    lib.pp_last_error.restype = ctypes.c_char_p
    vp = ctypes.c_void_p
    lib.pp_ensemble_reduce.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp]
    assert lib.pp_ensemble_reduce(None, None, 2, None, 0, None, None, None, None, None, None, None) == 1
    assert b"pp_ensemble_reduce" in lib.pp_last_error()
