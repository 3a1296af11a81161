"""Properties of the written definition of MorganFingerprint (tests/fingerprint_ref.py) and the host refusals of the new API, which are
raised before any launch - no GPU is needed for either."""
import numpy as np
import pytest
import torch

import aromaticity_ref as ar
import fingerprint_ref as fr
import physdock_amd
from physdock_amd import _lib
from physdock_amd.fingerprints import MorganFingerprint
from physdock_amd.ligand import Ligand, LigandLibrary

SMILES = ar.DEMO_SMILES + ("c1ccccc1", "CC(=O)Nc1ccc(O)cc1", "C1CC12CCC2", "N[C@@H](C)C(=O)O", "c1ccc2c(c1)[nH]c1ccccc12")


def test_the_hash_is_the_written_one():
    assert fr.fmix(0) == 0 and fr.fmix(1) == 0x514E28B7                         # the finaliser of MurmurHash3
    assert fr.push(0, 0) == fr.fmix(0x9E3779B9) and fr.push(7, -1) == fr.fmix((7 * 0x01000193 + 0xFFFFFFFF + 0x9E3779B9) & fr.M)
    assert fr.chain((6, 4)) == fr.push(fr.push(0, 6), 4)


def test_the_small_cases_by_hand():
    c = fr.fingerprint(Ligand.from_smiles("C"), 2)
    assert c["kept"].tolist() == [[1, 1, 0]] and c["n_features"] == 2               # no bond: the empty set, kept once
    assert c["ids"][0, 0] == fr.chain((6, 0, 4, 0, 0, 0)) and c["ids"][0, 1] == fr.chain((1, c["ids"][0, 0]))
    cc = fr.fingerprint(Ligand.from_smiles("CC"), 2)
    assert cc["kept"].sum(axis=0).tolist() == [2, 1, 0] and cc["n_features"] == 3
    assert cc["kept"][:, 1].tolist() == [1, 0]                                      # equal ids: the lower atom is the first
    assert cc["ids"][0, 1] == fr.chain((1, cc["ids"][0, 0], 2, cc["ids"][1, 0]))
    bz = fr.fingerprint(Ligand.from_smiles("c1ccccc1"), 3)
    assert bz["kept"].sum(axis=0).tolist() == [6, 6, 6, 1] and bz["n_features"] == 19
    assert [len(set(bz["ids"][:, r].tolist())) for r in range(4)] == [1, 1, 1, 1] and bz["popcount"] <= 4
    assert [bin(e).count("1") for e in bz["env"][1]] == [2] * 6 and [bin(e).count("1") for e in bz["env"][3]] == [6] * 6
    sf6 = fr.fingerprint(Ligand.from_graph(["S"] + ["F"] * 6, [(0, k) for k in range(1, 7)], None), 2)
    assert sf6["kept"].sum(axis=0).tolist() == [7, 7, 0]
    ring = fr.fingerprint(Ligand.from_smiles("CC1CC1"), 0)                          # the in-ring flag separates the two CH2 from the CH3
    assert len(set(ring["ids"][:, 0].tolist())) == 3


@pytest.mark.parametrize("smiles", SMILES)
def test_renumbering_the_atoms_and_bonds_changes_nothing(smiles):
    lig = Ligand.from_smiles(smiles)
    want = fr.fingerprint(lig, 4)
    rng = np.random.default_rng(len(smiles))
    for _ in range(3):
        atoms, bonds, perm = fr.renumbered(lig, rng)
        got = fr.morgan(atoms, bonds, 4)
        assert np.array_equal(got["bits"], want["bits"]) and got["n_features"] == want["n_features"]
        assert np.array_equal(got["ids"][perm], want["ids"])
        assert np.array_equal(got["kept"].sum(axis=0), want["kept"].sum(axis=0))


@pytest.mark.parametrize("smiles", SMILES[:6])
def test_a_short_row_is_the_fold_of_a_long_one(smiles):
    lig = Ligand.from_smiles(smiles)
    long = fr.fingerprint(lig, 3, 4096)
    for n_bits in (512, 1024, 2048):
        short = fr.fingerprint(lig, 3, n_bits)
        assert np.array_equal(short["bits"], fr.fold(long["bits"], n_bits))
        assert np.array_equal(short["ids"], long["ids"]) and np.array_equal(short["kept"], long["kept"])
    assert np.array_equal(fr.fingerprint(lig, 3, 512)["bits"], fr.fold(fr.fingerprint(lig, 3, 2048)["bits"], 512))


def test_invariants_replace_the_first_identifiers():
    lig = Ligand.from_smiles("CC(=O)Nc1ccc(O)cc1")
    inv = [int(z) for z in lig.elements]
    out = fr.fingerprint(lig, 2, 1024, atom_invariants=inv)
    assert out["ids"][:, 0].tolist() == inv and not np.array_equal(out["bits"], fr.fingerprint(lig, 2, 1024)["bits"])
    assert fr.fingerprint(lig, 1, 512, atom_invariants=[-1] * lig.n_atoms)["ids"][0, 0] == 0xFFFFFFFF


def test_tanimoto_top_k_and_maxmin_of_the_restatement():
    a = np.zeros((4, 16), dtype=np.uint32)
    a[0, 0], a[1, 0], a[2, 0], a[3, 5] = 0b0111, 0b0011, 0b0111, 0b1
    sim, common = fr.tanimoto(a, a)
    assert sim.dtype == np.float32 and sim[0, 1] == np.float32(2) / np.float32(3) and common[0, 1] == 2 and sim[0, 3] == 0
    assert np.array_equal(sim, sim.T) and (np.diag(sim) == 1).all()
    zero = np.zeros((1, 16), dtype=np.uint32)
    assert fr.tanimoto(zero, zero)[0][0, 0] == 1.0 and fr.tanimoto(zero, a)[0].tolist() == [[0.0] * 4]     # an empty union is 1
    index, s, c = fr.nearest(a, a, 2)
    assert index.tolist() == [[0, 2], [1, 0], [0, 2], [3, 0]]                       # ties: the lower column
    assert fr.nearest(a, a, 2, exclude_self=True)[0].tolist() == [[2, 1], [0, 2], [0, 1], [0, 1]]
    picks, far = fr.maxmin(a, 4, first=1)
    assert picks.tolist() == [1, 3, 0, 2] and np.isnan(far[0]) and far[1:].tolist() == [0.0, float(np.float32(2) / np.float32(3)), 1.0]
    assert fr.colliding_fractions(4096) is None and fr.colliding_fractions(8192) == ((8191, 8192), (8190, 8191))


def test_the_host_refuses_before_any_launch():
    lib = LigandLibrary.from_smiles(["CCO", "c1ccccc1"])
    for kw in ({"radius": 5}, {"radius": -1}, {"radius": 1.5}, {"n_bits": 1000}, {"n_bits": 256}, {"n_bits": 8192},
               {"atom_invariants": [1, 2, 3]}, {"atom_invariants": np.zeros((9, 1), dtype=np.int64)},
               {"atom_invariants": np.zeros(9, dtype=np.float32)}):
        with pytest.raises(ValueError, match="LigandLibrary.fingerprints"):
            lib.fingerprints(**kw)
    with pytest.raises(ValueError, match="radius"):
        lib.ligands[0].fingerprint(radius=7)
    a = MorganFingerprint(torch.zeros(3, 16, dtype=torch.int32), None, 512)
    b = MorganFingerprint(torch.zeros(5, 64, dtype=torch.int32), None, 2048)
    assert a.n_ligands == 3 and len(b) == 5 and a.radius is None
    for call in (lambda: a.cross(b), lambda: a.nearest(b), lambda: b.nearest(a, 2)):
        with pytest.raises(ValueError, match="512 bits against 2048|2048 bits against 512"):
            call()
    for call, text in ((lambda: a.nearest(a, 4), "k 4 of 3"), (lambda: a.neighbours(3), "k 3 of 2"), (lambda: a.nearest(a, 0), "k 0"),
                       (lambda: b.nearest(b, 17), "k 17"), (lambda: a.maxmin(4), "n_pick 4"), (lambda: a.maxmin(0), "n_pick 0"),
                       (lambda: a.maxmin(2, first=3), "first 3"), (lambda: a.cross(a.bits), "must be a MorganFingerprint"),
                       (lambda: a.explain(0, 3), "no features")):
        with pytest.raises(ValueError, match=text):
            call()
    for bad in (np.zeros((2, 10), dtype=np.uint32), np.zeros(16, dtype=np.uint32), np.zeros((2, 16), dtype=np.float32),
                np.zeros((0, 16), dtype=np.uint32), torch.zeros(2, 16, dtype=torch.int64)):
        with pytest.raises(ValueError, match="from_bits"):
            MorganFingerprint.from_bits(bad)
    with pytest.raises(AttributeError):
        a.bits = None


def test_the_symbols_and_the_export():
    new = {"pd_morgan_fingerprint", "pd_fingerprint_tanimoto", "pd_fingerprint_nearest", "pd_fingerprint_maxmin",
           "pd_fingerprint_maxmin_workspace_numel"}
    assert new <= set(_lib.header_symbols()) and _lib.ABI_VERSION == 11
    L = _lib.lib()
    assert new <= set(_lib.SYMBOLS) and all(hasattr(L, n) for n in new)
    assert L.pd_fingerprint_maxmin_workspace_numel(1000) == 3 * 1000 + 3 * 4 and L.pd_fingerprint_maxmin_workspace_numel(0) == -1
    assert physdock_amd.MorganFingerprint is MorganFingerprint
