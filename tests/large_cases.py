"""The cases of tests/test_large_cases_host.py and tests/test_large_batches_gpu.py: packed batches of more
than 1024 rows and more than 64 segments, one segment of more than 512 rows, and complexes of one, two and three residues.  Not a
test module.  Every builder is cached: the batches are shared, nobody writes to them.

``many()``        71 segments, 1087 rows (1087 = 1024 + 63 = 8 x 135 + 7): the first and the last segment one row long, a two- and
                  a three-row segment mid-pack (34, 35), row 1024 in segment 66 (rows 1014 .. 1028).
``many_rows(n)``  the same list up to the last whole segment below ``n`` rows, and one complex of the missing length: exactly ``n``.
``many_padded()`` the 68 multi-row complexes in front of the 24-row one, padded to [68][17]: 1156 rows on the uniform table.
``long530()``     one segment of 530 rows (256 + 256 + 18; 530 = 8 x 66 + 2).
``tiny(L)``       one complex of L = 1, 2 or 3 rows.
"""
import functools

import numpy as np
import torch

LENGTHS = [1, 16, 17, 15] + [15, 16, 17] * 10 + [2, 3] + [15, 16, 17] * 11 + [24] + [1]
OFFSETS = [0] + [int(x) for x in np.cumsum(LENGTHS)]
N_SEG, N_ROWS = len(LENGTHS), OFFSETS[-1]
assert (N_SEG, N_ROWS) == (71, 1087)
SEG_1024 = next(s for s in range(N_SEG) if OFFSETS[s] <= 1024 < OFFSETS[s + 1])          # 66: rows 1014 .. 1028
OBSTACLE_SEGMENTS = (1, SEG_1024, 69)
# alone, packed: both one-row ends, the two-row segment, and three of several rows -- the second, the one holding row 1024, the 24-row one
ALONE_SEGMENTS = (0, 34, 70, 1, SEG_1024, 69)


def _chains(L):
    return 1 if L == 1 else 2


@functools.lru_cache(maxsize=None)
def segment(i):
    """Segment ``i`` of ``many()`` as a B = 1 batch."""
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    return protein_to_batch(synth.make_complex(LENGTHS[i], 300 + i, _chains(LENGTHS[i])))


@functools.lru_cache(maxsize=None)
def top_up(L):
    """The complex that fills ``many_rows`` up: ``L`` rows, seed 400 + L."""
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    return protein_to_batch(synth.make_complex(L, 400 + L, _chains(L)))


@functools.lru_cache(maxsize=None)
def many():
    from packppi_amd.batch import pack
    b = pack([segment(i) for i in range(N_SEG)])
    assert b["seg_offsets_host"] == OFFSETS
    return b


@functools.lru_cache(maxsize=None)
def many_rows(n):
    from packppi_amd.batch import pack
    whole = max(s for s in range(N_SEG + 1) if OFFSETS[s] < n)
    b = pack([segment(i) for i in range(whole)] + [top_up(n - OFFSETS[whole])])
    assert b["seg_offsets_host"] == OFFSETS[:whole + 1] + [n]
    return b


PADDED_SEGMENTS = [i for i in range(N_SEG - 2) if LENGTHS[i] > 1]       # the multi-row complexes in front of the 24-row one


@functools.lru_cache(maxsize=None)
def many_padded():
    from packppi_amd.batch import collate
    b = collate([{**{k: (v[0] if isinstance(v, torch.Tensor) else v) for k, v in segment(i).items()}, "num_nodes": LENGTHS[i]}
                 for i in PADDED_SEGMENTS])
    assert tuple(b["residue_type"].shape) == (68, 17)
    return b


def padding_rows():
    """bool [68 x 17]: the rows of ``many_padded()`` that no complex owns."""
    return np.concatenate([np.arange(17) >= LENGTHS[i] for i in PADDED_SEGMENTS])


@functools.lru_cache(maxsize=None)
def long530():
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    return protein_to_batch(synth.make_complex(530, 41))


# the first seeds from 500 on at which every stage has work: one ASN (a flip with no partner row), SER + CYS (two rotors), THR + ASN + PRO
# (a rotor, a flip and a proline behind a peptide link, in two chains).  The types are asserted in tests/test_large_cases_host.py
TINY_SEEDS = {1: 502, 2: 510, 3: 534}


@functools.lru_cache(maxsize=None)
def tiny(L):
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    return protein_to_batch(synth.make_complex(L, TINY_SEEDS[L], _chains(L)))


def offsets(b):
    host = b.get("seg_offsets_host")
    if host is not None:
        return [int(x) for x in host]
    B, L = b["residue_type"].shape
    return [s * L for s in range(B + 1)]


CASES = {"many": many, "many1024": functools.partial(many_rows, 1024), "many1025": functools.partial(many_rows, 1025),
         "many_padded": many_padded, "long530": long530, "tiny1": functools.partial(tiny, 1), "tiny2": functools.partial(tiny, 2),
         "tiny3": functools.partial(tiny, 3)}


# ---- references that need no device, computed once ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sasa_ref(name, P, obstacles=False):
    """counts int32 [N, 14, 4] of the float32 restatement (tests/test_sasa_host.py), probe 1.4."""
    from packppi_amd.analysis import sphere_points
    from . import test_sasa_host as SH
    b = CASES[name]()
    ob, rg = (many_obstacles()[0], obstacle_ranges()) if obstacles else (None, None)
    return SH.restate(*SH.arrays(b), offsets(b), sphere_points(P), 1.4, ob, rg)


@functools.lru_cache(maxsize=None)
def polar_ref(name):
    from . import polar_oracle as PO
    return PO.of_batch(CASES[name]())


def _seeds(n, rows):
    s = np.zeros(n, np.uint8)
    s[list(rows)] = 1
    return s


def many_seed_sets():
    """every row; one seed in the segment holding row 1024 (row 1024 itself); no seed at all"""
    return {"every row": _seeds(N_ROWS, range(N_ROWS)), "row 1024": _seeds(N_ROWS, [1024]), "none": _seeds(N_ROWS, [])}


def long530_seed_sets():
    """one seed at row 520 (the third workgroup); seeds on rows 256 .. 511 only (the second); every row"""
    return {"row 520": _seeds(530, [520]), "rows 256..511": _seeds(530, range(256, 512)), "every row": _seeds(530, range(530))}


# ---- chi for the movers: the suites' ``seeded_chi`` helpers ---------------------------------------------------------------------------------
def seeded_chi(b, seed, amp):
    g = torch.Generator().manual_seed(seed)
    chi = b["SC_D"].clone().float()
    return torch.remainder(chi + amp * torch.randn(chi.shape, generator=g) + np.pi, 2 * np.pi) - np.pi


def hnet_chi(b):
    return seeded_chi(b, 3, 0.5)


def refine_chi(b):
    return seeded_chi(b, 11, 0.35)


def rows_of(t, b, s):
    """Rows of segment ``s`` of a per-row tensor [1, N, ...] of batch ``b``, as a [1, L, ...] tensor of their own."""
    offs = offsets(b)
    return t.reshape(1, offs[-1], *t.shape[2:])[:, offs[s]:offs[s + 1]].clone()


# ---- the obstacle variant of many() -----------------------------------------------------------------------------------------------------
N_OBSTACLES = 12
# a segment here has three to seven hydrogen-network movers, and the recipe puts its atoms outside one surface side chain: with 12
# atoms spread over 9 A these are the first seeds from 40 on at which the atoms come near enough to a mover to change an energy of
# the hydrogen-network ORACLE (tests/test_large_cases_host.py asserts it, and that the clash words and the SASA counts change too)
OBSTACLE_SEEDS = {1: 41, SEG_1024: 131, 69: 45}


@functools.lru_cache(maxsize=None)
def many_obstacles():
    """(xyzr float32 [36, 4], obstacle offsets [72], polar uint8 [36]): twelve atoms next to each of ``OBSTACLE_SEGMENTS`` (the
    ``ligand_near`` recipe of tests/test_sasa_host.py on that segment's own batch), no atom for the other 68."""
    from .test_sasa_host import ligand_near
    blocks, offs = [], [0]
    for s in range(N_SEG):
        if s in OBSTACLE_SEGMENTS:
            blocks.append(ligand_near(segment(s), N_OBSTACLES, OBSTACLE_SEEDS[s], 9.0))
        offs.append(offs[-1] + (N_OBSTACLES if s in OBSTACLE_SEGMENTS else 0))
    xyzr = np.concatenate(blocks).astype(np.float32)
    return xyzr, offs, (np.arange(len(xyzr)) % 2).astype(np.uint8)


def obstacle_ranges():
    offs = many_obstacles()[1]
    return [(offs[s], offs[s + 1] - offs[s]) for s in range(N_SEG)]
