"""The restatement of `CanonicalForm` (tests/canonical_ref.py) and the SMILES writer (`physdock_amd.canonical.write_smiles`) on the host:
invariance under renumbering, discrimination against networkx's isomorphism test, the search beyond refinement, the budget, the
terminal-twin rule, the round trip through `parse_smiles` and the refusals.  No GPU."""
import itertools

import numpy as np
import pytest

import canonical_cases as cc
import canonical_ref as cr
from physdock_amd.canonical import _check_steps, library_tables, renumber, write_smiles
from physdock_amd.ligand import Ligand, LigandLibrary

N_RENUMBERINGS = 8


@pytest.fixture(scope="module")
def cases():
    return cc.all_cases()


@pytest.fixture(scope="module")
def forms(cases):
    """the restatement of every case, computed once"""
    return {name: cr.canonical(lig) for name, lig in cases.items()}


def _text(lig, form):
    return write_smiles(lig, form["labels"])


def test_step_counts_of_the_table(forms):
    want = {name: steps for name, (_, steps) in cc.STEP_TABLE.items()}
    want.update(cc.CAGE_STEPS)
    for name, steps in want.items():
        assert (forms[name]["steps"], forms[name]["status"], forms[name]["canonical"]) == (steps, 0, 1), name
    assert forms["cubane"]["leaves"] == 48 and forms["hexaphenylbenzene"]["leaves"] == 768
    import aromaticity_ref as ar
    for s in ar.DEMO_SMILES:
        assert 2 <= forms[s]["steps"] <= 3, s


def test_invariance_under_renumbering(cases, forms):
    """one certificate, one key and one text for 8 seeded renumberings of atoms and bond rows"""
    for k, (name, lig) in enumerate(cases.items()):
        rng = np.random.default_rng(1000 + k)
        want = forms[name]
        text = _text(lig, want)
        for _ in range(N_RENUMBERINGS):
            other = cr.renumbered(lig, rng)
            got = cr.canonical(other)
            assert got["cert"] == want["cert"] and got["key"] == want["key"], name
            assert (got["steps"], got["leaves"], got["status"]) == (want["steps"], want["leaves"], 0), name
            assert sorted(got["labels"]) == list(range(lig.n_atoms)), name
            assert [got["order"][k] for k in got["labels"]] == list(range(lig.n_atoms)), name
            assert _text(other, got) == text, name


def test_discrimination_against_networkx(cases, forms):
    """certificates are equal exactly when the annotated graphs are isomorphic; the stereo families are compared by hand below, so
    here every case stands with its constitution only"""
    nx = pytest.importorskip("networkx")
    flat, graphs = {}, {}
    for name, lig in cases.items():
        plain = Ligand(lig.elements, lig.bonds, lig.bond_orders, lig.charges, lig.h_count, lig.aromatic, None, None, lig.isotopes)
        flat[name] = cr.canonical(plain)["cert"]
        t = cr.tables(plain)
        g = nx.Graph()
        for a, row in enumerate(t["atoms"]):
            g.add_node(a, inv=(row[0], row[1], row[2], t["isotopes"][a], row[3] & 1))
        for i, j, o2, _ in t["bonds"]:
            g.add_edge(i, j, o2=o2)
        graphs[name] = g
    n_equal = 0
    for p, q in itertools.combinations(cases, 2):
        iso = nx.is_isomorphic(graphs[p], graphs[q], node_match=lambda x, y: x["inv"] == y["inv"], edge_match=lambda x, y: x["o2"] == y["o2"])
        assert (flat[p] == flat[q]) == iso, (p, q)
        n_equal += iso
    assert n_equal >= 3 + 3 + 6 + 3 + 3                             # the spellings inside the stereo families at least


def test_stereo_families(forms):
    """alanine 3 + 3, the tartaric acids 1 + 1 + 2, the difluoroethenes 3 + 1, the three propan-2-ols all equal"""
    for family, groups in cc.FAMILIES.items():
        for group in groups:
            assert len({tuple(forms[s]["cert"]) for s in group}) == 1, (family, group)
            assert len({forms[s]["key"] for s in group}) == 1, (family, group)
        assert len({tuple(forms[group[0]]["cert"]) for group in groups}) == len(groups), family
    assert [len(g) for g in cc.ALANINES] == [3, 3] and sorted(len(g) for g in cc.TARTARIC) == [1, 1, 2]
    assert sorted(len(g) for g in cc.DIFLUOROETHENES) == [1, 3] and [len(g) for g in cc.PROPANOLS] == [3]
    # the mark of propan-2-ol cannot mean anything (two terminal methyls): parity 0 in every spelling
    assert all(((w >> 16) & 3) == 0 for w in forms["C[C@H](C)O"]["cert"][3:3 + 2 * 4:2])
    # the caveat: a mark whose equal substituents are not terminal is kept
    a, b, c = (cr.canonical(Ligand.from_smiles(s))["cert"] for s in ("CC[C@H](CC)O", "CC[C@@H](CC)O", "CCC(CC)O"))
    assert a == b and a != c


def test_search_not_refinement(forms):
    """cubane and cuneane: one root class of eight CH each, told apart by the search alone"""
    for name in ("cubane", "cuneane"):
        assert len(set(forms[name]["classes"])) == 1, name
    assert forms["cubane"]["cert"] != forms["cuneane"]["cert"]
    assert forms["cubane"]["cert"][:2 + 16] == forms["cuneane"]["cert"][:2 + 16]      # the same atoms, other bonds


def test_budget(cases):
    chain = cr.canonical(Ligand.from_smiles(cc.CHAIN_21), max_steps=300)
    assert (chain["status"], chain["steps"], chain["canonical"]) == (2, 300, 0) and chain["leaves"] >= 1
    full = cr.canonical(cases["cubane"], max_steps=81)
    assert (full["status"], full["steps"], full["canonical"]) == (0, 81, 1)
    short = cr.canonical(cases["cubane"], max_steps=80)
    assert (short["status"], short["steps"], short["canonical"]) == (2, 80, 0)
    one = cr.canonical(cases["cubane"], max_steps=1)
    assert (one["status"], one["steps"], one["leaves"], one["canonical"]) == (2, 1, 0, 0)
    assert one["labels"] == list(range(8)) == one["order"]
    g = cr._Graph(cr.tables(cases["cubane"]))
    assert one["cert"] == g.certificate(list(range(8)))


def test_twin_rule(cases, forms):
    assert forms["tri-t-butylbenzene"]["steps"] == 46 and forms["neopentane"]["steps"] == 4
    assert cr.canonical(cases["tri-t-butylbenzene"], twins=False)["steps"] == 2332
    n_checked = 0
    for name, lig in cases.items():
        plain = cr.canonical(lig, max_steps=5000, twins=False)
        if plain["status"] == 0:
            assert plain["cert"] == forms[name]["cert"] and plain["steps"] >= forms[name]["steps"], name
            n_checked += 1
    assert n_checked >= len(cases) - 1                              # all but p-decaphenyl at most


def test_round_trip(cases, forms):
    """reading the written text gives the certificate back, and writing that again the same text"""
    for name, lig in cases.items():
        text = _text(lig, forms[name])
        back = Ligand.from_smiles(text)
        again = cr.canonical(back)
        assert again["cert"] == forms[name]["cert"], (name, text)
        assert _text(back, again) == text, (name, text)
    assert _text(cases["[13CH4]"], forms["[13CH4]"]) == "[13CH4]" and _text(cases["[Na+]"], forms["[Na+]"]) == "[Na+]"
    assert _text(cases["CC#N"], forms["CC#N"]) in ("CC#N", "N#CC", "C(C)#N", "C(#N)C")


def test_renumber_gives_identity_labels(cases, forms):
    for name, lig in cases.items():
        new = renumber(lig, forms[name]["labels"])
        got = cr.canonical(new)
        assert got["labels"] == list(range(lig.n_atoms)) and got["cert"] == forms[name]["cert"], name


def test_first_of_on_the_restatement(cases, forms):
    names = ["benzene", "cubane", "benzene", "cuneane", "cubane"]
    results = [forms[n] for n in names] + [cr.canonical(cases["cubane"], max_steps=80)]
    assert cr.first_of(results) == [0, 1, 0, 3, 1, 5]


def test_library_tables(cases):
    lib = LigandLibrary([cases["N[C@@H](C)C(=O)O"], cases["F/C=C/F"], cases["[13CH4]"]])
    t = library_tables(lib)
    assert t["isotopes"].tolist() == [0] * 10 + [13] and t["chiral_order"].shape == (11, 4)
    assert t["chiral_order"][1].tolist() == [0, -1, 2, 3] and (t["chiral_order"][[0, 2, 3]] == -2).all()
    assert t["stereo_start"].tolist() == [0, 0, 1, 1] and t["stereo"].tolist() == [[0, 1, 2, 3, 2, -1, -1, 0]]
    assert t["cert_start"].tolist() == [0, 3 + 12 + 5, 3 + 12 + 5 + 3 + 8 + 3 + 1, 3 + 12 + 5 + 3 + 8 + 3 + 1 + 3 + 2]


def test_refusals(cases):
    for bad in (0, -1, 2 ** 31, 1.5, True, None, "7"):
        with pytest.raises(ValueError):
            _check_steps(bad, "test")
    lig = cases["benzene"]
    for labels in ([0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 4], [1, 2, 3, 4, 5, 6]):
        with pytest.raises(ValueError):
            write_smiles(lig, labels)
    with pytest.raises(ValueError):                                 # a bond order outside 1, 1.5, 2, 3
        write_smiles(Ligand.from_graph(["C", "C"], [(0, 1)], [2.5], h_count=[0, 0]), [0, 1])
    with pytest.raises(ValueError):                                 # an aromatic atom without a lower-case symbol
        write_smiles(Ligand.from_graph(["Si", "C"], [(0, 1)], [1.0], aromatic=[1, 0]), [0, 1])
    with pytest.raises(ValueError):                                 # an isotope the certificate has no room for
        library_tables(LigandLibrary([Ligand([6], np.zeros((0, 2)), [], None, [4], None, None, isotopes=[70000])]))
    from physdock_amd import canonical as cm

    def directions(rows, bonds, orders):
        class Rows:
            bond_stereo = np.asarray(rows)
        table = {(i, j): o for (a, b), o in zip(bonds, orders) for i, j in ((a, b), (b, a))}
        return cm._directions(Rows, {k: k for k in range(6)}, None, table)
    with pytest.raises(ValueError, match="not single"):             # the bond beside a stated double bond is not single
        directions([[0, 1, 2, 3, 1, -1, -1]], [(0, 1), (1, 2), (2, 3)], [1.0, 2.0, 2.0])
    # rows that admit no consistent marking: three conjugated double bonds in a cycle, each single bond between them read from
    # both of its ends (opposite signs), all three cis - the product of the three relations is -1, the rows ask for +1
    ring = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)]
    with pytest.raises(ValueError, match="no consistent marking"):
        directions([[0, 1, 2, 3, 1, -1, -1], [2, 3, 4, 5, 1, -1, -1], [4, 5, 0, 1, 1, -1, -1]], ring, [1.0, 2.0] * 3)
