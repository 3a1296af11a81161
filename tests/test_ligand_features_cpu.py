"""The written definition of the ligand features (tests/ligand_features_ref.py) against tables worked out by hand, the host
perception of physdock_amd/ligand.py against it, and the ideal bounds: they smooth without contradiction and the CPU restatement of the
conformer embedding (tests/conformers_ref.py) accepts a conformer from them.

Candidates that were tried for the embedding list and dropped: the bridged bicycles `C1C2CC1C2` and `C1CC2CCC1C2` (norbornane).
None of their 32 starts is accepted - the smallest violations are 0.13 and 0.11 A: ideal ring and tetrahedral angles cannot all hold at
a bridgehead.  Every other candidate tried was accepted (cubane, the spiro and the fused rings and the 26-atom demo ligand among them)."""
import os

import numpy as np
import pytest

import conformers_ref as cref
import ligand_features_ref as ref
from physdock_amd.conformers import COVALENT_RADII, ideal_bounds
from physdock_amd.ligand import GROUP_ELECTRONS, Ligand, LigandLibrary, chordless_rings
from physdock_amd.sdfio import parse_sdf
from physdock_amd.smiles import parse_smiles

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
#: the ligands whose bounds must embed on the CPU (test_the_cpu_restatement_accepts_a_conformer)
EMBED_SMILES = ("CCO", "CC#N", "c1ccccc1", "CC(=O)N", "C1CC1", "CS(=O)(=O)C", "N[C@@H](C)C(=O)O", "N[C@H](C)C(=O)O", "Oc1ccccc1",
                "CC(=O)Nc1ccc(O)cc1", "c1ccc2ccccc2c1", "C1CC12CCC2", "C12C3C4C1C5C2C3C45", "C1CCCCCCCC1",
                "c1cccc(c1C#N)NC(=S)NC(=O)c2ccc(o2)-c3ccc(Br)cc3")


def _t(smiles):
    r = parse_smiles(smiles)
    return r, ref.features(r)


def test_benzene():
    r, t = _t("c1ccccc1")
    assert t["ref_hybridization"].tolist() == [2] * 6 and t["ref_is_aromatic"].tolist() == [1] * 6 and t["ref_degree"].tolist() == [2] * 6
    assert set(ref.bond_table(r, t, "bond_is_conjugated").values()) == {1} and set(ref.bond_table(r, t, "bond_in_ring").values()) == {1}
    assert t["ref_in_ring_of_6"].tolist() == [1] * 6 and not any(t[f"ref_in_ring_of_{k}"].any() for k in (3, 4, 5, 7, 8))
    assert t["d_token"].tolist() == [[min((i - j) % 6, (j - i) % 6) for j in range(6)] for i in range(6)]
    assert set(ref.bond_table(r, t, "bond_type").values()) == {3} and set(ref.bond_table(r, t, "bond_as_double").values()) == {1}


def test_acetamide():
    r, t = _t("CC(=O)N")
    assert t["ref_hybridization"].tolist() == [3, 2, 2, 2]                                   # the amide N is SP2
    assert ref.bond_table(r, t, "bond_is_conjugated") == {(0, 1): 0, (1, 2): 1, (1, 3): 1}
    assert not t["bond_in_ring"].any() and t["d_token"].tolist() == [[0, 1, 2, 2], [1, 0, 1, 1], [2, 1, 0, 2], [2, 1, 2, 0]]
    assert t["ref_implicit_valence"].tolist() == [3, 0, 0, 2] and ref.bond_table(r, t, "bond_type") == {(0, 1): 0, (1, 2): 1, (1, 3): 0}
    assert not any(t[f"ref_in_ring_of_{k}"].any() for k in range(3, 9))


def test_phenol():
    r, t = _t("Oc1ccccc1")
    assert t["ref_hybridization"].tolist() == [2] * 7                                        # the phenol O is SP2
    assert ref.bond_table(r, t, "bond_is_conjugated")[(0, 1)] == 1 and ref.bond_table(r, t, "bond_in_ring")[(0, 1)] == 0
    assert t["ref_in_ring_of_6"].tolist() == [0] + [1] * 6 and not any(t[f"ref_in_ring_of_{k}"].any() for k in (3, 4, 5, 7, 8))
    assert t["d_token"].tolist() == [[0, 1, 2, 3, 4, 3, 2], [1, 0, 1, 2, 3, 2, 1], [2, 1, 0, 1, 2, 3, 2], [3, 2, 1, 0, 1, 2, 3],
                                     [4, 3, 2, 1, 0, 1, 2], [3, 2, 3, 2, 1, 0, 1], [2, 1, 2, 3, 2, 1, 0]]
    assert ref.bond_table(r, t, "bond_is_conjugated") == {(0, 1): 1, (1, 2): 1, (2, 3): 1, (3, 4): 1, (4, 5): 1, (5, 6): 1, (1, 6): 1}
    assert ref.bond_table(r, t, "bond_in_ring") == {(0, 1): 0, (1, 2): 1, (2, 3): 1, (3, 4): 1, (4, 5): 1, (5, 6): 1, (1, 6): 1}
    assert t["ref_is_aromatic"].tolist() == [0] + [1] * 6


def test_acetonitrile():
    r, t = _t("CC#N")
    assert t["ref_hybridization"].tolist() == [3, 1, 1] and ref.bond_table(r, t, "bond_is_conjugated") == {(0, 1): 0, (1, 2): 0}
    assert ref.bond_table(r, t, "bond_type") == {(0, 1): 0, (1, 2): 2} and ref.bond_table(r, t, "bond_as_double") == {(0, 1): 1, (1, 2): 3}
    assert t["d_token"].tolist() == [[0, 1, 2], [1, 0, 1], [2, 1, 0]] and not t["bond_in_ring"].any()
    assert not any(t[f"ref_in_ring_of_{k}"].any() for k in range(3, 9))


def test_dimethyl_sulfone():
    r, t = _t("CS(=O)(=O)C")
    assert t["ref_hybridization"].tolist() == [3, 3, 2, 2, 3] and t["ref_degree"].tolist() == [1, 4, 1, 1, 1]
    assert set(ref.bond_table(r, t, "bond_is_conjugated").values()) == {0} and not t["bond_in_ring"].any()
    assert t["d_token"].tolist() == [[0, 1, 2, 2, 2], [1, 0, 1, 1, 1], [2, 1, 0, 2, 2], [2, 1, 2, 0, 2], [2, 1, 2, 2, 0]]
    assert not any(t[f"ref_in_ring_of_{k}"].any() for k in range(3, 9))


def test_cyclopropane():
    r, t = _t("C1CC1")
    assert t["ref_hybridization"].tolist() == [3, 3, 3] and t["ref_in_ring_of_3"].tolist() == [1, 1, 1] and not t["ref_in_ring_of_4"].any()
    assert set(ref.bond_table(r, t, "bond_in_ring").values()) == {1} and set(ref.bond_table(r, t, "bond_is_conjugated").values()) == {0}
    assert t["d_token"].tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 0]]
    assert not any(t[f"ref_in_ring_of_{k}"].any() for k in (4, 5, 6, 7, 8))


def test_naphthalene():
    r, t = _t("c1ccc2ccccc2c1")
    assert t["ref_hybridization"].tolist() == [2] * 10 and t["ref_in_ring_of_6"].tolist() == [1] * 10
    assert not any(t[f"ref_in_ring_of_{k}"].any() for k in (3, 4, 5, 7, 8))                 # the perimeter of ten atoms has a chord
    assert set(ref.bond_table(r, t, "bond_in_ring").values()) == {1} and set(ref.bond_table(r, t, "bond_is_conjugated").values()) == {1}
    assert len(r["bonds"]) == 11 and t["ref_degree"].tolist() == [2, 2, 2, 3, 2, 2, 2, 2, 3, 2]
    assert t["d_token"][0].tolist() == [0, 1, 2, 3, 4, 5, 4, 3, 2, 1] and t["d_token"][3].tolist() == [3, 2, 1, 0, 1, 2, 3, 2, 1, 2]


def test_other_tables_by_hand():
    _, t = _t("N[C@@H](C)C(=O)O")
    assert t["ref_chirality"].tolist() == [2, 0, 2, 2, 2, 2] and _t("N[C@H](C)C(=O)O")[1]["ref_chirality"].tolist() == [2, 1, 2, 2, 2, 2]
    _, t = _t("[O-]C(=O)c1ccc[nH]1")
    assert t["ref_charge"].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0] and t["ref_hybridization"].tolist() == [2] * 8
    assert t["ref_feat"][0, 3] == -1.0 and t["ref_feat"][0, 4 + 7] == 1.0 and t["ref_feat"][:, :3].sum() == 0.0
    _, t = _t("[Na+]")
    assert t["ref_hybridization"].tolist() == [0] and t["ref_element"].tolist() == [10]
    _, t = _t("C1CCCCCCCC1")
    assert not any(t[f"ref_in_ring_of_{k}"].any() for k in range(3, 9)) and t["bond_in_ring"].sum() == 18
    _, t = _t("C1CCCCCC1C1CCCCCCC1")                                                         # a seven-ring, a bridge, an eight-ring
    assert t["ref_in_ring_of_7"].tolist() == [1] * 7 + [0] * 8 and t["ref_in_ring_of_8"].tolist() == [0] * 7 + [1] * 8
    assert t["bond_in_ring"][6, 7] == 0 and t["bond_in_ring"].sum() == 2 * 15
    _, t = _t(ref.CHAIN_128)
    assert t["d_token"][0, 29] == 29 and t["d_token"][0, 30] == 30 and t["d_token"][0, 127] == 30 and t["d_token"].max() == 30


@pytest.mark.parametrize("smiles", ref.PARITY_SMILES)
def test_host_perception_equals_the_restatement(smiles):
    r, t = _t(smiles)
    lig = Ligand.from_smiles(smiles)
    p = lig.perceive()
    assert p["hybridization"].tolist() == t["ref_hybridization"].tolist()
    want = ref.bond_table(r, t, "bond_is_conjugated")
    assert [int(c) for c in p["conjugated"]] == [want[(min(i, j), max(i, j))] for i, j in r["bonds"].tolist()]
    sizes = np.zeros((lig.n_atoms, 9), dtype=np.int8)
    for ring in p["rings"]:
        sizes[list(ring), len(ring)] = 1
    assert all(sizes[:, k].tolist() == t[f"ref_in_ring_of_{k}"].tolist() for k in range(3, 9))
    assert all(GROUP_ELECTRONS[z] == e for z, e in ref.ELECTRONS.items())


def test_constructors_and_refusals():
    assert chordless_rings(3, [(0, 1), (1, 2), (0, 2)]) == [(0, 1, 2)]
    a, b = Ligand.from_smiles("CC(=O)Nc1ccc(O)cc1"), None
    el, bonds, orders, charges = a.graph()
    b = Ligand.from_graph(el, bonds, orders, charges, aromatic=a.aromatic)
    assert b.h_count.tolist() == a.h_count.tolist()                                          # the valence rule, from the graph alone
    assert Ligand.from_graph(["C", "N", "C", "C", "C"], [(0, 1), (1, 2), (1, 3), (1, 4)], None, charges=[0, 1, 0, 0, 0]).h_count.tolist() == [3, 0, 3, 3, 3]
    with pytest.raises(ValueError, match="not connected"):
        Ligand.from_graph([6, 6, 8], [(0, 1)], [1.0])
    with pytest.raises(ValueError, match="129"):
        Ligand.from_graph([6] * 129, [(k, k + 1) for k in range(128)], [1.0] * 128)
    with pytest.raises(ValueError, match="0 ligands"):
        LigandLibrary([])
    with pytest.raises((ValueError, AttributeError)):
        a.elements[0] = 7                                                                     # immutable
    lib = LigandLibrary([a, Ligand.from_smiles("CCO")])
    assert lib.atom_start.tolist() == [0, 11, 14] and lib.bond_start.tolist() == [0, 11, 13] and lib.pair_start.tolist() == [0, 121, 130]
    assert lib.atoms.shape == (14, 4) and lib.bonds.shape == (13, 4) and lib.bonds[4].tolist() == [4, 5, 3, 0]


def test_the_crystal_ligand_from_its_sd_file():
    with open(os.path.join(GOLDEN, "EJQ.sdf")) as f:
        rec = parse_sdf(f.read())[0]
    lig = Ligand.from_sdf(rec)
    assert lig.n_atoms == 16 and lig.n_bonds == 17 and int(lig.h_count.sum()) == 15 and lig.symbols().count("F") == 1
    heavy = [k for k, e in enumerate(rec["elements"]) if e != "H"]
    assert heavy == list(range(16))                                                          # the heavy atoms come first and keep their order
    t = ideal_bounds(lig)
    x = rec["coords"]
    crystal = np.asarray([np.linalg.norm(x[i] - x[j]) for i, j in lig.bonds.tolist()])
    dev = np.abs(t["lengths"] - crystal)
    print(f"EJQ: ideal 1-2 lengths against the crystal's: mean |dev| {dev.mean():.3f} A, max {dev.max():.3f} A over {len(dev)} bonds")
    assert dev.max() < 0.15                 # a Kekule ring: 1.33 / 1.46 for 1.39; recorded in NOTES.md, the table is not fitted to it


@pytest.mark.parametrize("smiles", sorted(set(ref.PARITY_SMILES + EMBED_SMILES)))
def test_ideal_bounds_smooth_without_contradiction(smiles):
    lig = Ligand.from_smiles(smiles)
    t = ideal_bounds(lig)
    L = lig.n_atoms
    off = ~np.eye(L, dtype=bool)
    assert t["lo"].shape == (L, L) and (t["lo"] == t["lo"].T).all() and (t["up"] == t["up"].T).all()
    assert (t["lo"][off] > 0).all() and (t["lo"] <= t["up"]).all() and np.isfinite(t["up"]).all()
    for (i, j), d in zip(lig.bonds.tolist(), t["lengths"]):
        assert abs(t["up"][i, j] - (d + 0.01)) < 1e-12 and t["lo"][i, j] >= d - 0.01 - 1e-12
        r = COVALENT_RADII[int(lig.elements[i])] + COVALENT_RADII[int(lig.elements[j])] if {int(lig.elements[i]), int(lig.elements[j])} <= set(COVALENT_RADII) else None
        assert r is None or r - 0.32 - 1e-12 <= d <= r + 1e-12


def test_ideal_lengths_angles_and_volumes():
    lig = Ligand.from_smiles("CC(=O)Nc1ccc(O)cc1")
    t = ideal_bounds(lig)
    want = [1.52, 0.76 + 0.66 - 0.19, 0.76 + 0.71 - 0.06, 0.76 + 0.71 - 0.06, 1.39, 1.39, 1.39, 0.76 + 0.66 - 0.06, 1.39, 1.39, 1.39]
    assert np.allclose(t["lengths"], want, atol=1e-12)
    para = 2 * 1.39                                                                           # across the ring: cis over an aromatic bond
    assert abs(0.5 * (t["lo"][4, 7] + t["up"][4, 7]) - para) < 1e-9 and t["up"][4, 7] - t["lo"][4, 7] <= 0.1 + 1e-12
    meta = 1.39 * np.sqrt(3.0)
    assert abs(t["up"][4, 6] - (meta + 0.04)) < 1e-9
    ala, mirror = ideal_bounds(Ligand.from_smiles("N[C@@H](C)C(=O)O")), ideal_bounds(Ligand.from_smiles("N[C@H](C)C(=O)O"))
    assert ala["centres"].tolist() == [[1, 0, 2, 3]] and mirror["centres"].tolist() == [[1, 0, 2, 3]]
    v = 4 / (3 * np.sqrt(3)) * 1.47 * 1.52 * 1.52
    assert np.allclose([ala["vol_lo"][0], ala["vol_hi"][0]], [-1.4 * v, -0.6 * v]) and np.allclose([mirror["vol_lo"][0], mirror["vol_hi"][0]], [0.6 * v, 1.4 * v])
    assert ideal_bounds(Ligand.from_smiles("NC(C)C(=O)O"))["unspecified_centres"] == [1] and ala["unspecified_centres"] == []


@pytest.mark.parametrize("smiles", EMBED_SMILES)
def test_the_cpu_restatement_accepts_a_conformer(smiles):
    lig = Ligand.from_smiles(smiles)
    b = ideal_bounds(lig)
    t = dict(lo=b["lo"], up=b["up"], centres=b["centres"].astype(np.int64), vol_lo=b["vol_lo"], vol_hi=b["vol_hi"], box=0.5 * float(b["up"].max()))
    for c in range(32):
        got = cref.embed_one(t, cref.start(0, c, lig.n_atoms, t["box"]))
        if got["ok"]:
            break
    assert got["ok"], f"none of 32 starts of {smiles} was accepted"
    assert got["max_violation"] <= 0.1 and np.isfinite(got["x"]).all()
    if len(b["centres"]):                                                                     # L-alanine: CB on the positive side
        x = got["x"].astype(np.float64)
        side = float((x[2] - x[1]) @ np.cross(x[0] - x[1], x[3] - x[1]))
        assert (side > 0) == ("@@" in smiles)


def test_the_kernel_holds_the_same_valence_electron_table():
    """csrc/ligand_features.hip writes the table out; physdock_amd/ligand.py derives it from the periods: all 129 entries agree"""
    import re
    from physdock_amd import build
    with open(os.path.join(build.CSRC, "ligand_features.hip")) as f:
        text = f.read()
    body = re.search(r"LF_GROUP_ELECTRONS\[129\]\s*=\s*\{(.*?)\};", text, flags=re.S).group(1)
    table = [int(v) for v in re.findall(r"\d+", re.sub(r"//[^\n]*", "", body))]
    assert len(table) == 129 and tuple(table) == tuple(GROUP_ELECTRONS)
    assert [GROUP_ELECTRONS[z] for z in (1, 6, 7, 8, 16, 26, 35, 53, 57, 71, 72, 79, 82, 118)] == [1, 4, 5, 6, 6, 8, 7, 7, 3, 3, 4, 11, 4, 8]
