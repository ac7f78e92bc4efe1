"""``batch.group_rows`` and ``batch.pad_rows`` against the loops they replaced in ``TDiffusionModule.mutate`` and
``parallel.sample_sharded``.  ``old_groups`` is the loop as both drivers wrote it, kept verbatim."""
import pytest
import torch

from packppi_amd.batch import group_rows, pad_rows


def old_groups(sizes, alone, max_rows, n_decoys=1):
    groups, cur, rows_in = [], [], 0
    for i, n in enumerate(sizes):
        if alone[i]:
            groups.append([i])
            continue
        if cur and n_decoys * (rows_in + n) > max_rows:
            groups.append(cur)
            cur, rows_in = [], 0
        cur.append(i)
        rows_in += n
    if cur:
        groups.append(cur)
    return groups


# (sizes, max_rows, multiplier); a complex is alone iff it has fewer than 32 rows, plus the indices named in the fourth entry
# (32 rows or more, fewer than 32 true residues)
CASES = [
    ([], 100, 1, ()),
    ([40], 100, 1, ()),
    ([20], 100, 1, ()),
    ([40, 50, 60], 1000, 1, ()),                       # one group
    ([40, 50, 60], 90, 1, ()),                         # exactly full, then a new group
    ([40, 50, 60], 89, 1, ()),                         # one row short: every complex its own group
    ([200, 40, 50], 100, 1, ()),                       # a complex larger than max_rows still gets a group
    ([40, 20, 50, 10, 60], 1000, 1, ()),               # alone complexes are put down in front of the group that is still open
    ([20, 40, 33, 31, 32, 48], 75, 1, ()),
    ([40, 50, 60, 33], 200, 2, ()),                    # decoys: 2 x rows
    ([40, 50, 60, 33], 180, 2, ()),                    # exactly full with the multiplier
    ([40, 50, 60, 33, 20, 48], 179, 3, (2,)),
    ([33] * 9, 100, 1, (4,)),
    ([64, 64, 64, 64], 0, 1, ()),                      # max_rows 0: a group never stays empty
]


@pytest.mark.parametrize("sizes,max_rows,mult,extra", CASES)
def test_group_rows_is_the_old_loop(sizes, max_rows, mult, extra):
    alone = [n < 32 or i in extra for i, n in enumerate(sizes)]
    got = group_rows(sizes, alone, max_rows, mult)
    assert got == old_groups(sizes, alone, max_rows, mult)
    assert sorted(i for g in got for i in g) == list(range(len(sizes)))
    if mult == 1:
        assert got == group_rows(sizes, alone, max_rows)


def test_pad_rows():
    t = torch.arange(24, dtype=torch.float32).reshape(1, 6, 4)
    assert pad_rows(t, 6) is t
    own = pad_rows(t, 6, fresh=True)
    assert own is not t and own.data_ptr() != t.data_ptr() and torch.equal(own, t)
    full = pad_rows(t, 9)
    assert full.shape == (1, 9, 4) and full.dtype == t.dtype and torch.equal(full[:, :6], t) and not full[:, 6:].any()
    tail = torch.full((1, 9, 4), 7.0)
    assert torch.equal(pad_rows(t, 9, tail), torch.cat([t, tail[:, 6:]], 1))
    m = torch.tensor([[True, False, True]])
    assert pad_rows(m, 5, True).tolist() == [[True, False, True, True, True]] and pad_rows(m, 5, True).dtype == torch.bool
    assert pad_rows(m, 5, False).tolist() == [[True, False, True, False, False]]
    best = torch.tensor(3, dtype=torch.int32)
    pick = torch.tensor([[0, 1]], dtype=torch.int32)
    assert pad_rows(pick, 4, best.expand(1, 4)).tolist() == [[0, 1, 3, 3]]
