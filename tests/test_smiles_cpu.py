"""`parse_smiles` on hand-checked molecules: atoms, bonds, orders, hydrogen counts, charges and the neighbour order of stereocentres,
the first lines of the reference's screening demo as data, and every refusal with its character position."""
import os

import numpy as np
import pytest

from physdock_amd.smiles import MAX_ATOMS, parse_smiles

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bonds(r):
    return [(int(i), int(j), float(o)) for (i, j), o in zip(r["bonds"].tolist(), r["bond_orders"])]


def test_ethanol():
    r = parse_smiles("CCO")
    assert r["elements"].tolist() == [6, 6, 8] and _bonds(r) == [(0, 1, 1.0), (1, 2, 1.0)]
    assert r["h_count"].tolist() == [3, 2, 1] and r["charges"].tolist() == [0, 0, 0] and not r["aromatic"].any()
    assert r["chiral"].tolist() == [0, 0, 0] and r["chiral_order"] == {} and r["isotopes"].tolist() == [0, 0, 0]
    assert r["bonds"].dtype == np.int64 and r["bonds"].shape == (2, 2)


def test_benzene():
    r = parse_smiles("c1ccccc1")
    assert r["elements"].tolist() == [6] * 6 and r["aromatic"].all() and r["h_count"].tolist() == [1] * 6
    assert _bonds(r) == [(0, 1, 1.5), (1, 2, 1.5), (2, 3, 1.5), (3, 4, 1.5), (4, 5, 1.5), (0, 5, 1.5)]


def test_paracetamol():
    r = parse_smiles("CC(=O)Nc1ccc(O)cc1")
    assert r["elements"].tolist() == [6, 6, 8, 7, 6, 6, 6, 6, 8, 6, 6]
    assert _bonds(r) == [(0, 1, 1.0), (1, 2, 2.0), (1, 3, 1.0), (3, 4, 1.0), (4, 5, 1.5), (5, 6, 1.5), (6, 7, 1.5), (7, 8, 1.0), (7, 9, 1.5),
                         (9, 10, 1.5), (4, 10, 1.5)]
    assert r["h_count"].tolist() == [3, 0, 0, 1, 0, 1, 1, 0, 1, 1, 1]
    assert r["aromatic"].tolist() == [False] * 4 + [True] * 4 + [False] + [True] * 2


def test_tetramethylammonium():
    r = parse_smiles("C[N+](C)(C)C")
    assert r["elements"].tolist() == [6, 7, 6, 6, 6] and r["charges"].tolist() == [0, 1, 0, 0, 0]
    assert r["h_count"].tolist() == [3, 0, 3, 3, 3] and _bonds(r) == [(0, 1, 1.0), (1, 2, 1.0), (1, 3, 1.0), (1, 4, 1.0)]


def test_pyrrole_carboxylate():
    r = parse_smiles("[O-]C(=O)c1ccc[nH]1")
    assert r["elements"].tolist() == [8, 6, 8, 6, 6, 6, 6, 7] and r["charges"].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0]
    assert r["h_count"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert _bonds(r) == [(0, 1, 1.0), (1, 2, 2.0), (1, 3, 1.0), (3, 4, 1.5), (4, 5, 1.5), (5, 6, 1.5), (6, 7, 1.5), (3, 7, 1.5)]


def test_two_digit_ring_closure():
    r = parse_smiles("C%10CC%10")
    assert r["elements"].tolist() == [6, 6, 6] and _bonds(r) == [(0, 1, 1.0), (1, 2, 1.0), (0, 2, 1.0)] and r["h_count"].tolist() == [2, 2, 2]


def test_alanine_and_its_neighbour_order():
    r = parse_smiles("N[C@@H](C)C(=O)O")
    assert r["elements"].tolist() == [7, 6, 6, 6, 8, 8] and r["h_count"].tolist() == [2, 1, 3, 0, 0, 1]
    assert _bonds(r) == [(0, 1, 1.0), (1, 2, 1.0), (1, 3, 1.0), (3, 4, 2.0), (3, 5, 1.0)]
    assert r["chiral"].tolist() == [0, 2, 0, 0, 0, 0] and r["chiral_order"] == {1: [0, -1, 2, 3]}
    assert parse_smiles("N[C@H](C)C(=O)O")["chiral"].tolist() == [0, 1, 0, 0, 0, 0]
    # ring-closure partners stand where their digits do, in front of the branches and the chain
    assert parse_smiles("[C@]1(F)(Cl)CC1")["chiral_order"] == {0: [4, 1, 2, 3]}
    assert parse_smiles("C[C@@]12CC1O2")["chiral_order"] == {1: [0, 3, 4, 2]}


def test_directional_bonds_are_single():
    r = parse_smiles("F/C=C/F")
    assert r["elements"].tolist() == [9, 6, 6, 9] and _bonds(r) == [(0, 1, 1.0), (1, 2, 2.0), (2, 3, 1.0)] and r["h_count"].tolist() == [0, 1, 1, 0]
    assert _bonds(parse_smiles("F\\C=C/F")) == _bonds(r)


def test_isotope_and_written_hydrogens():
    r = parse_smiles("[13CH4]")
    assert r["elements"].tolist() == [6] and r["isotopes"].tolist() == [13] and r["h_count"].tolist() == [4] and r["bonds"].shape == (0, 2)
    assert parse_smiles("[CH3:7][NH3+]")["h_count"].tolist() == [3, 3]                      # the class is read and dropped
    assert parse_smiles("[Fe++]")["charges"].tolist() == [2] and parse_smiles("[O-2]")["charges"].tolist() == [-2]
    assert parse_smiles("[Cl-]")["elements"].tolist() == [17] and parse_smiles("[se]1cccc1")["elements"].tolist()[0] == 34


def test_explicit_hydrogens_are_folded():
    r = parse_smiles("C([H])([H])O")
    assert r["elements"].tolist() == [6, 8] and _bonds(r) == [(0, 1, 1.0)] and r["h_count"].tolist() == [3, 1]
    assert parse_smiles("[C@@]([H])(N)(C)O")["chiral_order"] == {0: [-1, 1, 2, 3]}
    with pytest.raises(ValueError, match="position 0"):
        parse_smiles("[H][H]")


def test_the_valence_rule():
    h = lambda s: parse_smiles(s)["h_count"].tolist()
    assert h("B") == [3] and h("N") == [3] and h("P") == [3] and h("S") == [2] and h("Cl") == [1] and h("I") == [1]
    assert h("CS(=O)(=O)C") == [3, 0, 0, 0, 3] and h("OP(=O)(O)O") == [1, 0, 0, 1, 1] and h("CS(C)=O") == [3, 0, 3, 0]
    assert h("c1ccncc1") == [1, 1, 1, 0, 1, 1] and h("c1ccsc1") == [1, 1, 1, 0, 1] and h("c1ccoc1") == [1, 1, 1, 0, 1]
    assert h("Cn1cccc1") == [3, 0, 1, 1, 1, 1] and h("c1ccc2ccccc2c1") == [1, 1, 1, 0, 1, 1, 1, 1, 0, 1]
    # an unmarked bond between aromatic atoms that closes no ring is single
    r = parse_smiles("c1ccccc1c1ccccc1")
    assert dict(((i, j), o) for i, j, o in _bonds(r))[(5, 6)] == 1.0 and r["h_count"].tolist() == [1] * 5 + [0, 0] + [1] * 5


def test_the_demo_library_parses():
    with open(os.path.join(GOLDEN, "smiles_demo.txt")) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    assert len(lines) == 5
    # heavy atoms counted by hand, symbol by symbol
    assert [len(parse_smiles(s)["elements"]) for s in lines] == [23, 26, 26, 28, 18]
    first = parse_smiles(lines[0])
    assert first["charges"].tolist().count(-1) == 1 and int(first["bond_orders"].tolist().count(3.0)) == 1
    for s in lines:
        r = parse_smiles(s)
        assert len(r["bonds"]) >= len(r["elements"])                                           # every one has at least one ring


@pytest.mark.parametrize("text, position, word", [
    ("CC.O", 2, "dot"), ("C*C", 1, r"\*"), ("[*]", 1, r"\*"), ("CXC", 1, "'X'"), ("C[Xx]C", 2, "unknown"), ("C1CC", 1, "ring closure 1"),
    ("CC(C", 2, "branch"), ("CC)C", 2, "branch"), ("C11", 2, "itself"), ("C12CC12", 6, "second bond"), ("C1CC1C1", 6, "ring closure 1"),
    ("", 0, "empty"), ("   ", 0, "empty"), ("C=1CC#1", 6, "one end"), ("C" * (MAX_ATOMS + 1), MAX_ATOMS, "129 heavy atoms"), ("C=", 1, "bond"),
    ("C[CH", 1, "not closed"), ("C%1C", 1, "two digits"), ("=C", 0, "bond"),
])
def test_refusals_name_the_position(text, position, word):
    with pytest.raises(ValueError, match=rf"parse_smiles: position {position}: .*{word}"):
        parse_smiles(text)


def test_ring_bond_symbols():
    assert _bonds(parse_smiles("C=1CCCCC1"))[-1] == (0, 5, 2.0) and _bonds(parse_smiles("C1CCCCC=1"))[-1] == (0, 5, 2.0)
    assert _bonds(parse_smiles("C=1CCCCC=1"))[-1] == (0, 5, 2.0)
    assert _bonds(parse_smiles("c1ccccc1-c1ccccc1"))[6] == (5, 6, 1.0) and _bonds(parse_smiles("c:1:c:c:c:c:c1"))[0] == (0, 1, 1.5)
