"""BondStereo without a device: the reading of `/` and `\\` against the written rule (tests/bond_stereo_ref.py), the refusals, that
unmarked input keeps every bit, the stereogenic bonds, the bounds that pin the isomer, the ABI and the restatement of the per-pose check
on constructed coordinates."""
import os

import numpy as np
import pytest

import bond_stereo_ref as ref
from physdock_amd.conformers import TOL_PLANAR, ideal_bounds
from physdock_amd.ligand import Ligand, LigandLibrary, normalise_bond_stereo, stereo_bonds_from_bonds
from physdock_amd.smiles import parse_smiles

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CIS, TRANS = 1, 2


def _table(s):
    return parse_smiles(s)["bond_stereo"]


def _kinds(s):
    return _table(s)[:, 4].tolist()


# ---------------------------------------------------------------------- the parser
def test_anchors():
    t = _table("F/C=C/F")
    assert t.dtype == np.int32 and t.tolist() == [[0, 1, 2, 3, TRANS, -1, -1]]
    assert _table("F/C=C\\F").tolist() == [[0, 1, 2, 3, CIS, -1, -1]]
    assert _kinds("F\\C=C\\F") == [TRANS] and _kinds("F\\C=C/F") == [CIS]
    # a branch atom: C(\F)=C/F is F/C=C/F written from the carbon (the atoms are numbered in another order)
    assert _table("C(\\F)=C/F").tolist() == [[1, 0, 2, 3, TRANS, -1, -1]]
    # the middle single bond serves both double bonds
    assert _table("C/C=C/C=C\\C").tolist() == [[0, 1, 2, 3, TRANS, -1, -1], [2, 3, 4, 5, CIS, -1, -1]]
    # a mark on a folded hydrogen passes, inverted, to the other substituent
    assert _kinds("[H]/C(F)=C/F") == _kinds("F\\C=C/F") == [CIS]
    assert _kinds("[H]\\C(F)=C/F") == [TRANS]
    assert _kinds("C/C=N/O") == [TRANS] and _kinds("C/C=N\\O") == [CIS]


def test_reference_substituents_are_the_lowest_and_the_kind_follows():
    # the mark stands on atom 3, the lowest substituent of atom 2; atom 4 is the other one
    assert _table("C/C=C(/C)CC").tolist() == [[0, 1, 2, 3, TRANS, -1, 4]]
    # the same molecule with the mark on the ethyl branch written first: the reference stays the lowest atom, the kind flips once
    assert _table("C/C=C(/CC)C").tolist() == [[0, 1, 2, 3, TRANS, -1, 5]]
    assert _table("C/C=C(\\CC)C").tolist() == [[0, 1, 2, 3, CIS, -1, 5]]
    # both substituents marked, consistently
    assert _table("C/C=C(/C)\\CC").tolist() == [[0, 1, 2, 3, TRANS, -1, 4]]


def test_no_entry():
    assert _table("C/C=C(/C)C").shape == (0, 7)                   # two substituents no walk of the graph tells apart
    assert _table("F/C=CF").shape == (0, 7) and _table("FC=C/F").shape == (0, 7)      # marks on one end only
    assert _table("C/CCC").shape == (0, 7) and _table("C/C\\C").shape == (0, 7)       # no double bond next to the mark
    assert _table("C/1=C/CCCC1").shape == (0, 7) and _table("C1=CCCCC1").shape == (0, 7)       # a ring of 6
    assert _table("F/C=C/C#N").tolist() == [[0, 1, 2, 3, TRANS, -1, -1]]
    assert _table("CC=CC").shape == (0, 7) and _table("CC=CC").dtype == np.int32


def test_ring_closures():
    # the bond from atom 2 to atom 10 closes a ring of 9: marked on the opening end, the closing end, or both (opposite characters)
    one, other, both = _table("C/C=C/1CCCCCCCC1F"), _table("C/C=C1CCCCCCCC\\1F"), _table("C/C=C/1CCCCCCCC\\1F")
    assert one.tolist() == other.tolist() == both.tolist() and one.shape == (1, 7)
    assert one[0, :4].tolist() == [0, 1, 2, 3] and one[0, 6] == 10
    # atom 3 is the reference and atom 10 carries the mark: `/` from 2 to 10 puts 10 up, so 3 is down, as atom 0 is: cis
    assert one[0, 4] == CIS and _kinds("C/C=C\\1CCCCCCCC1F") == [TRANS]
    assert _table("C/C=C/1CCCCCCCC1").shape == (0, 7)             # the two ring arms are alike


@pytest.mark.parametrize("s", ["F/C=C/F", "F/C=C\\F", "C(\\F)=C/F", "C/C=C/C=C\\C", "[H]/C(F)=C/F", "C/C=C(/C)C", "C/C=C(/C)CC",
                               "C/C=C(/CC)C", "C/C=N/O", "C/1=C/CCCC1", "OC(=O)/C=C/C(=O)O", "OC(=O)/C=C\\C(=O)O",
                               "C/C=C/1CCCCCCCC1F", "C/C=C1CCCCCCCC\\1F", "F/C=C/1CCCC\\C1=C\\F", "N/C(C)=C(/O)Cl", "C/C=C/[H]",
                               "Cl/C=C/C(=C/F)/Br"])
def test_the_parser_is_the_written_rule(s):
    got, want = _table(s), ref.table(s)
    assert got.shape == want.shape and (got == want).all(), (got.tolist(), want.tolist())


@pytest.mark.parametrize("text, position, word", [("C/C(\\F)=C/F", 4, "contradict"), ("F/C=C(/F)/Cl", 9, "contradict"),
                                                  ("[H]/C(\\F)=C/F", 6, "contradict"), ("C/C=C/1CCCCCCCC/1F", 16, "both ends")])
def test_refusals_name_the_position(text, position, word):
    with pytest.raises(ValueError, match=rf"parse_smiles: position {position}: .*{word}"):
        parse_smiles(text)


def _demo():
    with open(os.path.join(GOLDEN, "smiles_demo.txt")) as f:
        return [ln.strip() for ln in f if ln.strip()]


#: what parse_smiles returned before it kept the direction
PARENT_KEYS = ("elements", "bonds", "bond_orders", "charges", "aromatic", "h_count", "isotopes", "chiral", "chiral_order")


def test_unmarked_input_keeps_its_bits():
    for s in _demo() + ["CC=CC", "N[C@@H](C)C(=O)O", "C=1CCCCC=1"]:
        r = parse_smiles(s)
        assert set(r) == set(PARENT_KEYS) | {"bond_stereo"} and r["bond_stereo"].shape == (0, 7)
    # marks change nothing but the table: every other key has the bits of the string without them
    for marked in ["C/C=C/C", "C/C=C\\C", "OC(=O)/C=C/C(=O)O", "C/C=C/1CCCCCCCC\\1F", "[H]/C(F)=C/F"]:
        plain = marked.replace("/", "").replace("\\", "")
        a, b = parse_smiles(marked), parse_smiles(plain)
        for k in PARENT_KEYS:
            if k == "chiral_order":
                assert a[k] == b[k]
            else:
                assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (marked, k)


# ---------------------------------------------------------------------- Ligand
def test_candidates():
    un = lambda s: Ligand.from_smiles(s).unspecified_stereo_bonds
    assert un("CC=CC") == [(1, 2)]
    assert un("C/C=C/C") == [] and un("CC=C") == [] and un("CC(C)=CC") == []
    assert un("C1=CCCCC1") == [] and un("C1=CCCCCCC1") == [(0, 1)]          # a ring of 6, a ring of 8
    assert un("CC=NO") == [(1, 2)] and un("CC=O") == [] and un("CC=C=CC") == []
    assert un("C/C=C/C=CC") == [(3, 4)]
    for s in ["CC=CC", "CC(C)=CC", "CC=NO", "C1=CCCCCCC1", "FC=C1CCCCC1=CF", "CC=C=CC"]:
        r = parse_smiles(s)
        assert stereo_bonds_from_bonds(len(r["elements"]), r["bonds"], r["bond_orders"], r["elements"], r["h_count"]) == \
            ref.candidates(len(r["elements"]), r["bonds"].tolist(), r["bond_orders"].tolist(), r["elements"].tolist(), r["h_count"].tolist())


def test_ligand_carries_the_table():
    lig = Ligand.from_smiles("C/C=C(/CC)C")
    assert lig.bond_stereo.tolist() == [[0, 1, 2, 3, TRANS, -1, 5]] and not lig.bond_stereo.flags.writeable
    assert Ligand.from_smiles("CC=CC").bond_stereo.shape == (0, 7)
    r = parse_smiles("CC=C(CC)C")
    # rows (a, b, c, d, kind) are normalised: named the other substituent, or written c before b
    for rows in ([(0, 1, 2, 5, CIS)], [(5, 2, 1, 0, CIS)], [(0, 1, 2, 3, TRANS)]):
        g = Ligand.from_graph(r["elements"], r["bonds"], r["bond_orders"], h_count=r["h_count"], bond_stereo=rows)
        assert g.bond_stereo.tolist() == lig.bond_stereo.tolist()
    assert (normalise_bond_stereo(6, r["bonds"], [(0, 1, 2, 5, CIS)]) == ref.normalise(6, r["bonds"].tolist(), [(0, 1, 2, 5, CIS)])).all()
    for rows, word in (([(0, 1, 2, 4, CIS)], "not bonded"), ([(0, 1, 2, 3, 3)], "kind"), ([(0, 1, 2, 3, CIS), (5, 2, 1, 0, CIS)], "two rows"),
                       ([(0, 1, 2, 9, CIS)], "leaves")):
        with pytest.raises(ValueError, match=word):
            Ligand.from_graph(r["elements"], r["bonds"], r["bond_orders"], h_count=r["h_count"], bond_stereo=rows)
    iso = parse_smiles("CC=C(C)C")
    with pytest.raises(ValueError, match="not stereogenic"):
        Ligand.from_graph(iso["elements"], iso["bonds"], iso["bond_orders"], h_count=iso["h_count"], bond_stereo=[(0, 1, 2, 3, CIS)])
    assert len(LigandLibrary([lig, Ligand.from_smiles("CCO")])) == 2              # the library's tables do not read it


# ---------------------------------------------------------------------- the bounds
def test_bounds_pin_the_isomer():
    trans, cis = Ligand.from_smiles("C/C=C/C"), Ligand.from_smiles("C/C=C\\C")
    raw_t, raw_c = ideal_bounds(trans, smooth=False), ideal_bounds(cis, smooth=False)
    for raw in (raw_t, raw_c):
        assert raw["up"][0, 3] - raw["lo"][0, 3] == pytest.approx(2.0 * TOL_PLANAR, abs=1e-12)
    t, c = ideal_bounds(trans), ideal_bounds(cis)                                    # (smoothing raises for neither)
    assert c["up"][0, 3] < t["lo"][0, 3]                                             # disjoint
    assert t["stereo_bonds"].tolist() == trans.bond_stereo.tolist()
    # the wide interval of the unmarked bond holds both
    plain = ideal_bounds(Ligand.from_smiles("CC=CC"))
    assert plain["lo"][0, 3] <= c["lo"][0, 3] and t["up"][0, 3] <= plain["up"][0, 3] and plain["stereo_bonds"].shape == (0, 7)


def test_bounds_without_entries_keep_their_bits():
    for s in ["CC=CC", "CC(=O)Nc1ccc(O)cc1", "OC(=O)C=CC(=O)O"] + _demo()[:1]:
        r = parse_smiles(s)
        a = ideal_bounds(Ligand.from_smiles(s))
        b = ideal_bounds(Ligand.from_graph(r["elements"], r["bonds"], r["bond_orders"], r["charges"], r["h_count"], r["aromatic"], r["chiral"]))
        assert a["lo"].tobytes() == b["lo"].tobytes() and a["up"].tobytes() == b["up"].tobytes()
    # ... and dropping the marks from a marked ligand gives the unmarked ligand's bounds
    a, b = ideal_bounds(Ligand.from_smiles("CC=CC")), ideal_bounds(Ligand.from_smiles("C/C=C/C"))
    assert a["lo"].tobytes() != b["lo"].tobytes()


def test_fumaric_against_maleic_acid():
    f, m = (ideal_bounds(Ligand.from_smiles(s), smooth=False) for s in ("OC(=O)/C=C/C(=O)O", "OC(=O)/C=C\\C(=O)O"))
    differ = {(int(i), int(j)) for i, j in np.argwhere((f["lo"] != m["lo"]) | (f["up"] != m["up"])) if i < j}
    assert differ == {(1, 5)}                                                        # the one 1-4 pair across C3=C4
    for s in ("OC(=O)/C=C/C(=O)O", "OC(=O)/C=C\\C(=O)O", "C/C=C/C=C\\C", "C/C=C(/CC)C"):
        ideal_bounds(Ligand.from_smiles(s))                                          # triangle smoothing raises for none
    # two substituents on one end: the pair with the reference and the mixed pair get the two different distances
    raw = ideal_bounds(Ligand.from_smiles("C/C=C(/CC)C"), smooth=False)              # (0, 1, 2, 3, trans, -1, 5)
    assert raw["lo"][0, 3] > raw["up"][0, 5] and raw["up"][0, 5] - raw["lo"][0, 5] == pytest.approx(2.0 * TOL_PLANAR, abs=1e-12)


# ---------------------------------------------------------------------- the ABI
def test_the_symbol_is_bound():
    from physdock_amd import _lib
    L = _lib.lib()
    assert "pd_bond_stereo" in _lib.SYMBOLS and "pd_bond_stereo" in _lib.header_symbols()
    assert len(L.pd_bond_stereo.argtypes) == 15


# ---------------------------------------------------------------------- the restatement on constructed coordinates
@pytest.mark.parametrize("phi, state, twist", [(0.0, 1, 0.0), (1.0, 1, 1.0), (-1.0, 1, 1.0), (89.0, 1, 89.0), (-89.0, 1, 89.0), (91.0, 2, 89.0),
                                               (-91.0, 2, 89.0), (179.0, 2, 1.0), (-179.0, 2, 1.0), (180.0, 2, 0.0)])
def test_restatement_on_constructed_dihedrals(phi, state, twist):
    x = ref.place(phi, np.random.default_rng(int(abs(phi)) + 7))[None]
    got = ref.check(x, [[0, 1, 2, 3, -1, -1]], [1], max_twist=30.0)
    assert got["state"][0, 0] == state and abs(abs(got["dihedral64"][0, 0]) - abs(phi)) < 1e-4
    assert np.sign(got["dihedral64"][0, 0]) == np.sign(phi) or abs(phi) in (0.0, 180.0)
    assert abs(got["twist64"][0, 0] - twist) < 1e-4
    assert got["n_wrong"][0] == int(state != 1) and got["ok"][0] == int(state == 1) and got["n_twisted"][0] == int(twist > 30.0)


def test_restatement_undefined_and_second_substituents():
    x = ref.place(10.0)[None].repeat(3, axis=0)
    x[1, 0] = x[1, 1] - (x[1, 2] - x[1, 1])                      # a, b, c on one line
    x[2, 3, 1] = np.nan
    got = ref.check(x, [[0, 1, 2, 3, -1, -1]], [1])
    assert got["state"][:, 0].tolist() == [1, 0, 0] and got["n_wrong"].tolist() == [0, 1, 1] and got["n_twisted"].tolist() == [0, 1, 1]
    assert got["max_twist_seen"][0] == got["twist"][0, 0] and np.isnan(got["max_twist_seen"][1:]).all()
    # a pyramidal end: a2 stands 40 degrees out of the plane of a, b, c while a-b-c-d is flat
    flat, bent = ref.place(180.0), ref.place(140.0)
    x = np.concatenate([flat, bent[3:]])[None]                    # atoms 0 .. 3 and a second "d" at 140 degrees as atom 4
    got = ref.check(x, [[0, 1, 2, 3, -1, 4]], [2])
    assert got["state"][0, 0] == 2 and abs(got["twist64"][0, 0] - 40.0) < 1e-4 and got["n_twisted"][0] == 1 and got["ok"][0] == 1
