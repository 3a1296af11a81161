"""pd_canonical_form and pd_canonical_first against tests/canonical_ref.py on an MI355X.  Everything is integer work in a fixed order, so
every comparison is EXACT, exhausted budgets included.  One library of the case set with 3 renumberings of each molecule (at most 42
atoms a ligand) is launched once with the default budget; a second, small one holds the 126-atom chain and runs at 300 steps."""
import numpy as np
import pytest
import torch

import canonical_cases as cc
import canonical_ref as cr
from physdock_amd import CanonicalForm, write_smiles
from physdock_amd.ligand import Ligand, LigandLibrary

pytestmark = pytest.mark.gpu

PER_LIGAND = ("status", "steps", "leaves", "canonical")
PER_ATOM = ("labels", "order", "classes")
SHORT = 300


@pytest.fixture(scope="module")
def ligands():
    """every case of at most 42 atoms followed by 3 seeded renumberings of it"""
    out = []
    for k, (name, lig) in enumerate(cc.all_cases().items()):
        if lig.n_atoms > 42:
            continue
        rng = np.random.default_rng(2000 + k)
        out += [lig] + [cr.renumbered(lig, rng) for _ in range(3)]
    assert 140 <= len(out) <= 170 and max(l.n_atoms for l in out) == 42
    return out


@pytest.fixture(scope="module")
def want(ligands):
    return [cr.canonical(l) for l in ligands]


@pytest.fixture(scope="module")
def form(ligands):
    return LigandLibrary(ligands).canonical()


@pytest.fixture(scope="module")
def short_ligands(ligands):
    cases = cc.all_cases()
    chain = Ligand.from_smiles(cc.CHAIN_21)
    assert chain.n_atoms == 126
    return [cases["cubane"], chain, cases["hexaphenylbenzene"], cases["cubane"], cases["benzene"], chain, ligands[5]]


def _got(found):
    out = {}
    for key in PER_LIGAND + PER_ATOM + ("cert", "key"):
        v = getattr(found, key)
        assert v.is_cuda and v.dtype == torch.int32, key
        out[key] = v.cpu().numpy()
    out["cert"], out["key"] = out["cert"].view(np.uint32), out["key"].view(np.uint32)
    return out


def _same(found, want, what=""):
    got, a, w0 = _got(found), 0, 0
    for g, w in enumerate(want):
        n, length = len(w["labels"]), len(w["cert"])
        for key in PER_LIGAND:
            assert int(got[key][g]) == w[key], (what, g, key, int(got[key][g]), w[key])
        for key in PER_ATOM:
            assert got[key][a:a + n].tolist() == w[key], (what, g, key)
        assert (int(found.cert_start[g]), int(found.cert_start[g + 1])) == (w0, w0 + length), (what, g)
        assert got["cert"][w0:w0 + length].tolist() == w["cert"], (what, g)
        assert tuple(got["key"][g].tolist()) == w["key"], (what, g)
        a, w0 = a + n, w0 + length
    assert a == got["labels"].shape[0] and w0 == got["cert"].shape[0]
    return got


def test_every_output_equals_the_restatement(form, want):
    assert isinstance(form, CanonicalForm) and form.n_ligands == len(want)
    got = _same(form, want, "library")
    assert not got["status"].any() and got["canonical"].all() and got["steps"].max() == 1531


def test_exhausted_budgets_equal_the_restatement(short_ligands):
    want = [cr.canonical(l, max_steps=SHORT) for l in short_ligands]
    found = LigandLibrary(short_ligands).canonical(max_steps=SHORT)
    got = _same(found, want, "300 steps")
    assert got["status"].tolist() == [0, 2, 2, 0, 0, 2, 0] and got["steps"][1] == SHORT and got["canonical"].tolist() == [1, 0, 0, 1, 1, 0, 1]
    assert got["leaves"][1] >= 1                                    # the chain ran out with a best leaf, which is what was compared
    # first_of: the second cubane points at the first and the renumbered benzene at benzene; a ligand that ran out matches nothing,
    # not even its own copy
    assert short_ligands[6].n_atoms == 6
    assert found.first_of.cpu().tolist() == cr.first_of(want) == [0, 1, 2, 0, 4, 5, 4]
    # a budget of one step: no leaf, the input order
    one = LigandLibrary(short_ligands[:1]).canonical(max_steps=1)
    _same(one, [cr.canonical(short_ligands[0], max_steps=1)], "1 step")
    assert one.labels.cpu().tolist() == list(range(8)) and int(one.canonical[0]) == 0 and int(one.leaves[0]) == 0
    # the step count of cubane, from both sides
    assert int(LigandLibrary(short_ligands[:1]).canonical(max_steps=81).status[0]) == 0
    assert int(LigandLibrary(short_ligands[:1]).canonical(max_steps=80).status[0]) == 2


def test_alone_first_and_last(ligands, want):
    """a ligand has the same words wherever it stands"""
    picks = [k for k, l in enumerate(ligands) if l.source in ("C/C=C/C=C\\C", "N[C@@H](C)C(=O)O")][:2] + [len(ligands) - 1, 33]
    for k in picks:
        for lib, at in (([ligands[k]], 0), ([ligands[k]] + ligands[:6], 0), (ligands[:6] + [ligands[k]], 6)):
            found = LigandLibrary(lib).canonical()
            expect = [want[k]] if len(lib) == 1 else ([want[k]] + want[:6] if at == 0 else want[:6] + [want[k]])
            _same(found, expect, f"ligand {k} at {at} of {len(lib)}")


def test_aromatize():
    lib = LigandLibrary.from_smiles(["C1=CC=CC=C1", "c1ccccc1"])
    plain, perceived = lib.canonical(), lib.canonical(aromatize=True)
    assert plain.first_of.cpu().tolist() == [0, 1] and not plain.same(0, 1)
    assert perceived.first_of.cpu().tolist() == [0, 0] and perceived.same(0, 1)
    assert perceived.aromaticity_status.cpu().tolist() == [0, 0] and plain.aromaticity_status is None
    c = perceived.cert.cpu().numpy()
    assert c[:c.shape[0] // 2].tolist() == c[c.shape[0] // 2:].tolist() == cr.canonical(Ligand.from_smiles("c1ccccc1"))["cert"]
    assert perceived.smiles() == ["c1ccccc1", "c1ccccc1"] and plain.smiles()[1] == "c1ccccc1" and "=" in plain.smiles()[0]


def test_first_of_and_unique(form, want):
    first = form.first_of
    assert first.is_cuda and first.dtype == torch.int32
    assert first.cpu().tolist() == cr.first_of(want)
    molecules = {}
    for g, w in enumerate(want):
        molecules.setdefault(tuple(w["cert"]), g)
    assert first.cpu().tolist() == [molecules[tuple(w["cert"])] for w in want]
    host = first.cpu().tolist()
    for g in range(0, len(want), 4):                                # every renumbering points at or before its first spelling
        assert all(host[g + k] == host[g] <= g for k in range(4)), g
    unique = form.unique()
    assert unique.is_cuda and unique.cpu().tolist() == sorted(molecules.values())
    assert form.is_first.cpu().tolist() == [molecules[tuple(w["cert"])] == g for g, w in enumerate(want)]
    assert form.same(0, 3) and not form.same(0, 4)
    assert form.first_of is first                                  # the second launch happens once


def test_smiles_and_renumbered(form, ligands, want):
    texts = form.smiles()
    labels = form.labels.cpu().numpy()
    a = 0
    for g, lig in enumerate(ligands):
        assert texts[g] == write_smiles(lig, labels[a:a + lig.n_atoms]) == write_smiles(lig, want[g]["labels"]), g
        a += lig.n_atoms
    for g in range(0, len(ligands), 4):
        assert len(set(texts[g:g + 4])) == 1, g
    assert len(set(texts)) == len({tuple(w["cert"]) for w in want})
    new = form.renumbered()
    again = new.canonical()
    start = new.atom_start
    assert again.labels.cpu().tolist() == [k for g in range(len(ligands)) for k in range(int(start[g + 1] - start[g]))]
    assert again.cert.cpu().tolist() == form.cert.cpu().tolist() and again.smiles() == texts


def test_two_launches_give_identical_bits(ligands, form):
    again = LigandLibrary(ligands).canonical()
    for key in PER_LIGAND + PER_ATOM + ("cert", "key"):
        assert torch.equal(getattr(again, key), getattr(form, key)), key
    assert torch.equal(again.first_of, form.first_of)


def test_single_ligand_conveniences_and_refusals():
    a, b = Ligand.from_smiles("OC(=O)[C@@H](N)C"), Ligand.from_smiles("N[C@@H](C)C(=O)O")
    assert a.canonical_smiles() == b.canonical_smiles() and a.identity_key() == b.identity_key()
    w = cr.canonical(a)
    assert a.identity_key() == w["key"][0] << 32 | w["key"][1]
    assert Ligand.from_smiles("N[C@H](C)C(=O)O").identity_key() != a.identity_key()
    lib = LigandLibrary([a])
    for bad in (0, -3, 2 ** 31, 2.5, None):
        with pytest.raises(ValueError):
            lib.canonical(max_steps=bad)
    with pytest.raises(ValueError):
        Ligand.from_smiles(cc.CHAIN_21).canonical_smiles(max_steps=300)
    with pytest.raises(AttributeError):
        lib.canonical().labels = None
