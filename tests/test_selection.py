"""Residue selections for partial repacking (packppi_amd/selection.py) and the fixed_mask key through pack() / unpack(): CPU only."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def protein():
    """Two chains of 20 residues, both numbered 1..20 in the file (the featurisation pushes chain B's numbers past chain A's)."""
    from packppi_amd import synth
    return synth.make_complex(40, 11)


def test_parser(protein):
    from packppi_amd.featurize import chain_numbers_and_offset_index
    from packppi_amd.selection import parse_selection
    rows = lambda spec: np.flatnonzero(parse_selection(spec, protein)).tolist()
    assert rows("A:5-8") == [4, 5, 6, 7]
    assert rows("B:12") == [31]
    assert rows("A") == list(range(20)) and rows("B") == list(range(20, 40))
    assert rows("A:19-20, B:1-2,B:12") == [18, 19, 20, 21, 31]
    assert rows("A:18-99") == [17, 18, 19]                       # a range may reach past the chain's end
    m = parse_selection("A:3", protein)
    assert m.dtype == bool and m.shape == (40,)
    # the file's numbering, not the offset numbering of the batch: B:12 is row 31, whose batch residue_index is 132
    offset = chain_numbers_and_offset_index(protein)[1]
    assert int(offset[31]) == 132 and int(protein["residue_index"][31]) == 12
    with pytest.raises(ValueError, match="matches no residue"):
        parse_selection("B:132", protein)
    with pytest.raises(ValueError, match="no chain 'C'"):
        parse_selection("A:1-5,C", protein)
    with pytest.raises(ValueError, match="matches no residue"):
        parse_selection("A:30-40", protein)
    with pytest.raises(ValueError, match="expected CHAIN"):
        parse_selection("A:x-5", protein)
    with pytest.raises(ValueError, match="empty selection"):
        parse_selection(" , ", protein)


def test_negative_residue_numbers():
    from packppi_amd import synth
    from packppi_amd.selection import parse_selection
    p = synth.make_complex(12, 3, n_chains=1)
    p["residue_index"] = np.arange(-3, 9)
    assert np.flatnonzero(parse_selection("A:-3--1", p)).tolist() == [0, 1, 2]
    assert np.flatnonzero(parse_selection("A:-1-1", p)).tolist() == [2, 3, 4]
    assert np.flatnonzero(parse_selection("A:-2", p)).tolist() == [1]


def test_pack_and_unpack_carry_fixed_mask():
    from packppi_amd import synth
    from packppi_amd.batch import pack, unpack
    from packppi_amd.featurize import protein_to_batch, protein_to_data
    a, b = protein_to_batch(synth.make_complex(17, 1)), protein_to_data(synth.make_complex(23, 2))
    a["fixed_mask"] = (torch.arange(17) % 3 != 0).unsqueeze(0)          # [1, L] beside a B = 1 batch
    b["fixed_mask"] = torch.arange(23) < 5                               # [L] beside per-complex data
    pb = pack([a, b])
    assert pb.fixed_mask.shape == (1, 40) and pb.fixed_mask.dtype == torch.bool
    back = unpack(pb, pb.fixed_mask)
    assert torch.equal(back[0], a["fixed_mask"]) and torch.equal(back[1][0], b["fixed_mask"])
    # only when every complex carries one
    del b["fixed_mask"]
    assert "fixed_mask" not in pack([a, b])


def test_interface_selection(protein, tmp_path):
    from packppi_amd.pdb_io import from_pdb_file, to_pdb
    from packppi_amd.selection import interface_selection
    pdb = tmp_path / "complex.pdb"
    pdb.write_text(to_pdb(protein))
    read = from_pdb_file(pdb, mse_to_met=True)
    sel = interface_selection(read, pdb, radius=6.0)
    assert sel.dtype == bool and sel.shape == (40,)
    assert 0 < sel.sum() < 40                                    # non-empty, a strict subset
    assert sel[:20].any() and sel[20:].any()                     # an interface has two sides
    wide = interface_selection(read, pdb, radius=10.0)
    assert (wide | sel).sum() == wide.sum()                      # a larger radius only adds residues
    one = tmp_path / "one.pdb"
    from packppi_amd import synth
    one.write_text(to_pdb(synth.make_complex(12, 3, n_chains=1)))
    with pytest.raises(ValueError, match="two protein chains"):
        interface_selection(from_pdb_file(one, mse_to_met=True), one)
