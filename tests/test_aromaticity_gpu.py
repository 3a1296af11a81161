"""pd_aromaticity against tests/aromaticity_ref.py on an MI355X: the atom rows, the bond rows, the status and the counts must be EXACTLY
equal in every mode (the kernel is integer work; there is no tolerance to choose), a ligand's bits must not depend on the library around
it, and the outputs feed pd_ligand_features as `LigandLibrary.features(aromatize=True)` says."""
import os

import numpy as np
import pytest
import torch

import aromaticity_ref as ar
import ligand_features_ref as lf
from physdock_amd import ops
from physdock_amd.ligand import ATOM_COLUMNS, PAIR_COLUMNS, Ligand, LigandLibrary
from physdock_amd.ring_interactions import aromatic_rings_from_bonds
from physdock_amd.sdfio import parse_sdf

pytestmark = pytest.mark.gpu

MODES = ("kekulise", "perceive", "normalise")
BIG = (ar.POLYPHENYLENE_128, ar.CHAIN_128)
EVERY = ar.ALL_SMILES + BIG
KEYS = ("atoms", "bonds", "status", "counts")
TABLES = ("atom_table", "pair_table", "ref_feat", "rel_tok_feat")


def _expected(lig, mode, max_steps=ar.DEFAULT_MAX_STEPS):
    g = ar.graph(lig)
    r = ar.run(g, mode, max_steps)
    atoms, bonds = ar.rows(g, r, lig.chiral)
    return {"atoms": atoms, "bonds": bonds, "status": np.asarray([r["status"]], dtype=np.int32),
            "counts": np.asarray([r["counts"]], dtype=np.int32)}


def _run(lib, mode, max_steps=ar.DEFAULT_MAX_STEPS):
    out = lib.aromaticity(mode, max_steps, "cuda")
    assert set(out) == set(KEYS) and all(out[k].is_cuda and out[k].dtype == torch.int32 for k in KEYS)
    return {k: out[k].cpu().numpy() for k in KEYS}


def _same(got, want, what):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist(), want[k].tolist())


@pytest.fixture(scope="module")
def ligands():
    return {s: Ligand.from_smiles(s) for s in EVERY}


@pytest.fixture(scope="module")
def expected(ligands):
    return {(s, m): _expected(ligands[s], m) for s in EVERY for m in MODES}


@pytest.fixture(scope="module")
def alone(ligands):
    return {(s, m): _run(LigandLibrary([ligands[s]]), m) for s in EVERY for m in MODES}


@pytest.fixture(scope="module")
def ejq():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "EJQ.sdf")) as f:
        return Ligand.from_sdf(parse_sdf(f.read())[0])


@pytest.mark.parametrize("smiles", ar.ALL_SMILES)
def test_every_mode_equals_the_definition(smiles, expected, alone):
    for mode in MODES:
        _same(alone[smiles, mode], expected[smiles, mode], (smiles, mode))


@pytest.mark.parametrize("case", list(ar.STATUS.items()), ids=lambda c: f"{c[0][0][:12]}-{c[0][1]}")
def test_status_and_steps(case):
    (smiles, max_steps), (status, steps) = case
    lig = Ligand.from_smiles(smiles)
    lib = LigandLibrary([lig])
    for mode in ("kekulise", "normalise"):
        got = _run(lib, mode, max_steps)
        _same(got, _expected(lig, mode, max_steps), (smiles, mode, max_steps))
        assert got["status"][0] == status and got["counts"][0, 3] == steps
        if status:
            assert np.array_equal(got["atoms"], lib.atoms) and np.array_equal(got["bonds"], lib.bonds)


def test_the_smallest_ligands(alone, expected):
    for mode in MODES:
        got = alone["[Na+]", mode]                                              # L = 1, no bonds: a null bonds pointer
        assert got["atoms"].tolist() == [[11, 1, 0, 0]] and got["bonds"].shape == (0, 4)
        assert got["status"].tolist() == [0] and got["counts"].tolist() == [[0, 0, 0, 0]]
    furan = alone["c1ccoc1", "normalise"]
    assert furan["counts"].tolist() == [[1, 5, 5, 3]] and furan["bonds"][:, 2].tolist() == [3] * 5 and furan["bonds"][:, 3].tolist().count(3) == 2
    assert alone["c1ccoc1", "kekulise"]["bonds"][:, 2].tolist().count(4) == 2


@pytest.mark.parametrize("smiles", BIG, ids=["polyphenylene128", "chain128"])
def test_the_largest_ligands(smiles, ligands, alone, expected):
    assert ligands[smiles].n_atoms == 128
    for mode in MODES:
        _same(alone[smiles, mode], expected[smiles, mode], (smiles[:12], mode))
    got = alone[smiles, "normalise"]
    if smiles == ar.CHAIN_128:
        lib = LigandLibrary([ligands[smiles]])
        assert np.array_equal(got["atoms"], lib.atoms) and np.array_equal(got["bonds"], lib.bonds) and not got["counts"].any()
    else:
        assert got["counts"].tolist() == [[21, 126, 126, 63]] and got["atoms"][64:, 3].sum() > 0


@pytest.mark.parametrize("mode", MODES)
def test_one_launch_for_a_library_gives_each_ligand_its_own_bits(mode, ligands, alone):
    for order in (list(range(len(EVERY))), list(reversed(range(len(EVERY))))):
        lib = LigandLibrary([ligands[EVERY[k]] for k in order])
        out = _run(lib, mode)
        assert out["atoms"].shape == (lib.n_atoms, 4) and out["bonds"].shape == (lib.n_bonds, 4) and out["counts"].shape == (len(EVERY), 4)
        for g, k in enumerate(order):
            a0, a1, b0, b1 = (int(v) for v in (*lib.atom_start[g:g + 2], *lib.bond_start[g:g + 2]))
            want = alone[EVERY[k], mode]
            assert np.array_equal(out["atoms"][a0:a1], want["atoms"]) and np.array_equal(out["bonds"][b0:b1], want["bonds"]), (EVERY[k][:16], g)
            assert out["status"][g] == want["status"][0] and np.array_equal(out["counts"][g], want["counts"][0]), (EVERY[k][:16], g)


def test_aromatized_and_kekulized_return_new_ligands(ligands, ejq):
    lig = Ligand.from_smiles("N[C@@H](Cc1ccccc1)C(=O)O")
    kek = lig.kekulized("cuda")
    assert kek is not lig and not kek.aromatic.any() and sorted(kek.bond_orders.tolist()).count(2.0) == 4 and 1.5 not in kek.bond_orders
    back = kek.aromatized("cuda")
    for name in ("elements", "bonds", "bond_orders", "charges", "h_count", "aromatic", "chiral", "isotopes"):
        assert np.array_equal(getattr(back, name), getattr(lig, name)), name
        assert not getattr(back, name).flags.writeable
    assert back.chiral_order == lig.chiral_order and back.source == lig.source == kek.source and lig.bond_orders.tolist().count(1.5) == 6
    seen = ejq.aromatized("cuda")
    assert aromatic_rings_from_bonds(ejq.n_atoms, ejq.bonds.tolist(), ejq.bond_orders) == []
    assert aromatic_rings_from_bonds(seen.n_atoms, seen.bonds.tolist(), seen.bond_orders) == [(3, 4, 5, 6, 7, 8)]
    assert np.nonzero(seen.aromatic)[0].tolist() == [3, 4, 5, 6, 7, 8] and np.array_equal(seen.h_count, ejq.h_count) and seen.source == ejq.source
    lib = LigandLibrary([ligands["c1ccccc1"], ligands["c1cccc1"], ligands["CCO"]])
    with pytest.raises(ValueError, match=r"ligand 1 \(c1cccc1\): status 1"):
        lib.aromatized("cuda")
    kept = lib.kekulized("cuda", errors="keep")
    assert kept.status.tolist() == [0, 1, 0] and kept.ligands[1] is lib.ligands[1] and kept.ligands[0].bond_orders.tolist().count(2.0) == 3
    assert LigandLibrary([ligands["c1ccccc1"]]).aromatized("cuda").status.tolist() == [0]


def test_features_chain_without_a_read_back(ligands, ejq):
    chosen = [ejq] + [Ligand.from_smiles(s) for s in ar.KEKULE] + [ligands[s] for s in ("c1cccc1", ar.BACKTRACK, "CCO", "[Na+]", ar.PERYLENE)]
    lib = LigandLibrary(chosen)
    today = {k: v.cpu().numpy() for k, v in lib.features("cuda").items()}
    assert sorted(today) == sorted(TABLES)
    chained = lib.features("cuda", aromatize=True)
    assert sorted(chained) == sorted(TABLES + ("aromaticity_status",)) and chained["aromaticity_status"].is_cuda
    rewritten = lib.aromatized("cuda", errors="keep")
    assert chained["aromaticity_status"].cpu().numpy().tolist() == rewritten.status.tolist() == [0] * 9 + [1, 0, 0, 0, 0]
    two_step = rewritten.features("cuda")
    for name in TABLES:
        assert torch.equal(chained[name], two_step[name]), name
    first = lib.split(chained, 0)
    assert int(first["bond_is_aromatic"].sum()) == 12 and int((first["bond_type"] == 3).sum()) == 12
    assert first["ref_is_aromatic"].cpu().numpy().tolist() == [1 if 3 <= a <= 8 else 0 for a in range(ejq.n_atoms)]
    assert int(lib.split({k: torch.from_numpy(v) for k, v in today.items()}, 0)["bond_is_aromatic"].sum()) == 0
    # without the keyword nothing changes: the tables of a second call, and the restatement of the feature definition
    again = lib.features("cuda", aromatize=False)
    for name in TABLES:
        assert np.array_equal(again[name].cpu().numpy(), today[name]), name
    for g, lig in enumerate(chosen[:4]):
        rec = {k: getattr(lig, k) for k in ("elements", "bonds", "bond_orders", "charges", "h_count", "aromatic", "chiral")}
        want = lf.features(rec)
        got = lib.split(again, g)
        for name in ATOM_COLUMNS + PAIR_COLUMNS + ("ref_feat", "rel_tok_feat"):
            assert np.array_equal(got[name].cpu().numpy(), want[name]), (g, name)


def _launch(tables, n_ligands, n_atoms, n_bonds, mode=2):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in tables.items()}
    out = {"atoms": torch.full((t["atoms"].shape[0], 4), -7, dtype=torch.int32, device="cuda"),
           "bonds": torch.full((t["bonds"].shape[0], 4), -7, dtype=torch.int32, device="cuda"),
           "status": torch.full((n_ligands,), -7, dtype=torch.int32, device="cuda"),
           "counts": torch.full((n_ligands, 4), -7, dtype=torch.int32, device="cuda")}
    code = ops._lib.init().pd_aromaticity(ops.ptr(t["atom_start"]), ops.ptr(t["bond_start"]), ops.ptr(t["atoms"]), ops.ptr(t["bonds"]),
                                          ops.ptr(out["atoms"]), ops.ptr(out["bonds"]), ops.ptr(out["status"]), ops.ptr(out["counts"]),
                                          n_ligands, n_atoms, n_bonds, mode, 65536, ops.stream())
    torch.cuda.synchronize()
    return code, {k: v.cpu().numpy() for k, v in out.items()}


def test_a_ligand_whose_rows_leave_the_arrays_is_not_written(ligands, alone):
    names = ("c1ccccc1", "CCO", "c1ccoc1")
    lib = LigandLibrary([ligands[s] for s in names])
    tables = {k: getattr(lib, k) for k in ("atom_start", "bond_start", "atoms", "bonds")}
    a, b = lib.atom_start, lib.bond_start

    def check(out, written):
        for g, s in enumerate(names):
            if g in written:
                want = alone[s, "normalise"]
                assert np.array_equal(out["atoms"][a[g]:a[g + 1]], want["atoms"]) and np.array_equal(out["bonds"][b[g]:b[g + 1]], want["bonds"])
                assert out["status"][g] == 0 and np.array_equal(out["counts"][g], want["counts"][0])
            else:
                assert (out["atoms"][a[g]:a[g + 1]] == -7).all() and (out["bonds"][b[g]:b[g + 1]] == -7).all()
                assert out["status"][g] == -7 and (out["counts"][g] == -7).all()

    code, out = _launch(tables, 3, lib.n_atoms, lib.n_bonds)
    assert code == 0
    check(out, (0, 1, 2))
    code, out = _launch(tables, 3, lib.n_atoms - 1, lib.n_bonds)                 # the last ligand's atoms end past n_atoms
    assert code == 0
    check(out, (0, 1))
    code, out = _launch(tables, 3, lib.n_atoms, lib.n_bonds - 1)                 # its bonds end past n_bonds
    assert code == 0
    check(out, (0, 1))
    # an empty ligand, a negative start, rows that run backwards: that ligand alone is left out
    for start, status in (([0, 9, 9, 14], [0, -7, 0]), ([-3, 0, 9, 14], [-7, 0, 0]), ([0, 6, 9, 8], [0, 0, -7])):
        code, out = _launch(dict(tables, atom_start=np.asarray(start, dtype=np.int32)), 3, lib.n_atoms, lib.n_bonds)
        assert code == 0 and out["status"].tolist() == status
        assert all((out["counts"][g] == -7).all() == (status[g] == -7) for g in range(3))
    wide = dict(tables, atom_start=np.asarray([0, 6, 6 + 129, 6 + 129 + 5], dtype=np.int32),
                atoms=np.concatenate([lib.atoms[:6], np.tile(lib.atoms[6:7], (129, 1)), lib.atoms[9:]]))
    code, out = _launch(wide, 3, 6 + 129 + 5, lib.n_bonds)                       # 129 atoms
    assert code == 0
    assert (out["atoms"][6:6 + 129] == -7).all() and out["status"].tolist() == [0, -7, 0]
    assert np.array_equal(out["atoms"][:6], alone["c1ccccc1", "normalise"]["atoms"])
    # a bond that leaves its ligand is copied through and otherwise skipped
    bad = lib.bonds.copy()
    bad[7] = [0, 5, 4, 9]                                                        # CCO has 3 atoms
    code, out = _launch(dict(tables, bonds=bad), 3, lib.n_atoms, lib.n_bonds)
    assert code == 0 and out["bonds"][7].tolist() == [0, 5, 4, 9] and out["status"].tolist() == [0, 0, 0]
    assert np.array_equal(out["bonds"][:6], alone["c1ccccc1", "normalise"]["bonds"])


def test_rejected_calls_launch_nothing(ligands):
    lib = LigandLibrary([ligands["c1ccccc1"]])
    tables = {k: getattr(lib, k) for k in ("atom_start", "bond_start", "atoms", "bonds")}
    for kw in ({"mode": 3}, {"mode": -1}):
        code, out = _launch(tables, 1, lib.n_atoms, lib.n_bonds, **kw)
        assert code == -1 and (out["atoms"] == -7).all() and (out["status"] == -7).all()
    code, out = _launch(tables, 0, lib.n_atoms, lib.n_bonds)
    assert code == -1
    t = lib.tables("cuda")
    L_ = ops._lib.init()
    status, counts = torch.full((1,), -7, dtype=torch.int32, device="cuda"), torch.full((1, 4), -7, dtype=torch.int32, device="cuda")
    spare = torch.full((6, 4), -7, dtype=torch.int32, device="cuda")
    args = (ops.ptr(status), ops.ptr(counts), 1, 6, 6, 2, 65536, ops.stream())
    assert L_.pd_aromaticity(ops.ptr(t["atom_start"]), ops.ptr(t["bond_start"]), ops.ptr(t["atoms"]), ops.ptr(t["bonds"]),
                             ops.ptr(t["atoms"]), ops.ptr(spare), *args) == -1   # an output that is its input
    assert L_.pd_aromaticity(ops.ptr(t["atom_start"]), ops.ptr(t["bond_start"]), ops.ptr(t["atoms"]), None, ops.ptr(spare), None, *args) == -1
    torch.cuda.synchronize()
    assert (status == -7).all() and (spare == -7).all() and np.array_equal(t["atoms"].cpu().numpy(), lib.atoms)


def test_the_defaults_run_on_the_current_device(expected):
    lib = LigandLibrary.from_smiles(["C1=CC=CC=C1"])
    out = lib.aromaticity()
    assert out["atoms"].is_cuda and out["atoms"].device.index == torch.cuda.current_device()
    assert out["bonds"][:, 2].tolist() == [3] * 6 and out["counts"].tolist() == [[1, 6, 6, 0]]
    assert lib.aromatized().ligands[0].bond_orders.tolist() == [1.5] * 6
    assert Ligand.from_smiles("c1ccccc1").kekulized().bond_orders.tolist().count(2.0) == 3
