"""The Vina-style score without a GPU: the float64 restatement (tests/vina_ref.py) against closed forms worked out by hand and
against its own central differences, the typing helpers of physdock_amd/scoring.py on small molecules and residues,
count_rotatable_bonds, rank_by_score, the argument checks, the header - and the condition the GPU tests rest on: every seeded case
of tests/vina_ref.py keeps MARGIN clear of the cutoff and of the kinks (one `MARGIN | ...` line per case, pytest -s)."""
import math
import re

import numpy as np
import pytest
import torch

import vina_ref as ref

W = dict(zip(ref.TERM_NAMES, (-0.0356, -0.00516, 0.840, -0.0351, -0.587)))


def pair(r, type_a, type_b):
    x = np.zeros((1, 2, 3))
    x[0, 1, 0] = r
    return ref.vina(x, [0], [type_a, type_b], [0, 1], [1], 0.0)


# ------------------------------------------------------------------ the restatement against hand-computed pairs
@pytest.mark.parametrize("d", [-0.3, 0.25, 1.0, 3.0])
def test_two_hydrophobic_carbons(d):
    out = pair(3.8 + d, ref.C_H, ref.C_H)                              # two carbons: R_i + R_j = 3.8
    g1, g2 = math.exp(-(d / 0.5) ** 2), math.exp(-((d - 3.0) / 2.0) ** 2)
    rep = d * d if d < 0 else 0.0
    hyd = {-0.3: 1.0, 0.25: 1.0, 1.0: 0.5, 3.0: 0.0}[d]
    want = [g1, g2, rep, hyd, 0.0]
    assert out["terms"][0] == pytest.approx(want, rel=1e-12, abs=1e-15)
    e = W["gauss1"] * g1 + W["gauss2"] * g2 + W["repulsion"] * rep + W["hydrophobic"] * hyd
    assert out["inter"][0] == pytest.approx(e, rel=1e-12) and out["per_atom"][0, 0] == pytest.approx(e, rel=1e-12)
    # the force on atom 0 (at the origin, its partner on +x): -dE/dx_0 = +dE/dd
    de = W["gauss1"] * (-2.0 * d / 0.25 * g1) + W["gauss2"] * (-2.0 * (d - 3.0) / 4.0 * g2)
    de += W["repulsion"] * 2.0 * d if d < 0 else 0.0
    de += -W["hydrophobic"] if 0.5 < d < 1.5 else 0.0
    assert out["forces"][0, 0] == pytest.approx([de, 0.0, 0.0], rel=1e-12, abs=1e-15)


@pytest.mark.parametrize("d", [-1.0, -0.35, 0.2])
def test_a_donor_acceptor_pair(d):
    want = {-1.0: 1.0, -0.35: 0.5, 0.2: 0.0}[d]
    for ta, tb in ((ref.N_D, ref.O_A), (ref.O_A, ref.N_D), (ref.N_DA, ref.N_DA)):
        rsum = ref.CLASS_RADII[ta & 15] + ref.CLASS_RADII[tb & 15]
        out = pair(rsum + d, ta, tb)
        assert out["terms"][0, 4] == pytest.approx(want, abs=1e-12) and out["terms"][0, 3] == 0.0
        assert out["terms"][0, 2] == pytest.approx(d * d if d < 0 else 0.0, abs=1e-12)
    assert ref.CLASS_RADII[1] + ref.CLASS_RADII[2] == pytest.approx(3.5)
    # two donors, two acceptors, or an atom without flags: no hydrogen bond
    for ta, tb in ((ref.N_D, ref.N_D), (ref.O_A, ref.O_A), (ref.N_D, 2), (ref.C_H, ref.O_A)):
        assert pair(3.0, ta, tb)["terms"][0, 4] == 0.0


def test_a_pair_beyond_the_cutoff_contributes_nothing():
    out = pair(8.5, ref.C_H, ref.C_H)
    assert not out["terms"].any() and not out["forces"].any() and out["inter"][0] == 0.0 and out["n_pairs"][0] == 0
    assert pair(7.9, ref.C_H, ref.C_H)["n_pairs"][0] == 1


def test_radii_weights_and_the_rotor_factor():
    from physdock_amd import scoring
    assert scoring.TERM_NAMES == ref.TERM_NAMES and list(scoring.WEIGHTS) == list(ref.WEIGHTS)
    assert [scoring.RADII[z] for z in (6, 7, 8, 15, 16, 9, 17, 35, 53)] == [1.9, 1.8, 1.7, 2.1, 2.0, 1.5, 1.8, 2.0, 2.2]
    assert scoring.radius_class([6, 7, 8, 15, 16, 9, 17, 35, 53, 30, 26]).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9]
    assert [ref.CLASS_RADII[c] for c in scoring.radius_class([6, 7, 8, 15, 16, 9, 17, 35, 53, 30])] == [1.9, 1.8, 1.7, 2.1, 2.0, 1.5, 1.8, 2.0, 2.2, 1.2]
    assert (scoring.HYDROPHOBIC, scoring.DONOR, scoring.ACCEPTOR) == (ref.HYDROPHOBIC, ref.DONOR, ref.ACCEPTOR) == (16, 32, 64)
    x = np.zeros((1, 2, 3))
    x[0, 1, 2] = 3.6
    a, b = ref.vina(x, [0], [ref.C_H, ref.C_H], [0, 1], [1], 0.0), ref.vina(x, [0], [ref.C_H, ref.C_H], [0, 1], [1], 4.0)
    assert b["inter"][0] == a["inter"][0] and b["score"][0] == pytest.approx(a["inter"][0] / (1 + 0.0585 * 4))
    assert np.array_equal(a["forces"], b["forces"])                     # the forces are those of inter


@pytest.mark.parametrize("name", list(ref.CASES))
def test_analytic_gradient_against_central_differences_and_the_margin_of_the_seeds(name):
    c = ref.make_case(name)
    tab = (c["lig_idx"], c["types"], c["rec_mask"], c["lig_active"])
    out = ref.vina(c["x"], *tab, c["n_rot"])
    print(f"MARGIN | {name} | pairs {out['n_pairs'].tolist()} | {out['margin']:.2e} |")
    assert out["margin"] >= ref.MARGIN, "a committed seed puts a pair on the cutoff or on a kink"
    assert (out["terms"] > 0).all(), ("every term must be at work", out["terms"])
    h = 1e-5
    x = c["x"].astype(np.float64)
    fd = np.zeros_like(out["forces"])
    for i, a in enumerate(c["lig_idx"]):
        for k in range(3):
            xp, xm = x.copy(), x.copy()
            xp[:, a, k] += h
            xm[:, a, k] -= h
            fd[:, i, k] = -(ref.energy(xp, *tab) - ref.energy(xm, *tab)) / (2 * h)
    # central differences: h^2 / 6 times the third derivative (below ~50 per pair) and the rounding of the energies over 2h
    assert np.abs(fd - out["forces"]).max() <= 1e-7, np.abs(fd - out["forces"]).max()
    assert np.abs(out["forces"]).max() > 1e-2
    inactive = c["lig_active"] == 0
    assert not out["forces"][:, inactive].any() and not out["per_atom"][:, inactive].any()
    assert np.allclose(out["per_atom"].sum(1), out["inter"], rtol=1e-12)
    assert (out["bound"]["score"] < 1e-4).all() and (out["bound"]["forces"] < 1e-4).all() and (out["bound"]["score"] > 0).all()


# ------------------------------------------------------------------ typing helpers
def flags(t):
    return [("H" if v & 16 else "") + ("D" if v & 32 else "") + ("A" if v & 64 else "") for v in t]


def test_ligand_types_of_small_molecules():
    from physdock_amd.scoring import ligand_types_from_bonds as types
    # ethanol C-C-O
    t = types([6, 6, 8], [(0, 1), (1, 2)])
    assert flags(t) == ["H", "", "DA"] and (t & 15).tolist() == [0, 0, 2]
    # acetic acid CH3-C(=O)-OH
    assert flags(types([6, 6, 8, 8], [(0, 1), (1, 2), (1, 3)], [1, 2, 1])) == ["H", "", "A", "DA"]
    # the acetate anion: neither oxygen has a hydrogen
    assert flags(types([6, 6, 8, 8], [(0, 1), (1, 2), (1, 3)], [1, 2, 1], formal_charges=[0, 0, 0, -1])) == ["H", "", "A", "A"]
    ring = [(i, (i + 1) % 6) for i in range(6)]
    # pyridine: N (atom 0) without hydrogen and with two heavy neighbours accepts; its two neighbours are polar carbons
    assert flags(types([7, 6, 6, 6, 6, 6], ring, [1.5] * 6)) == ["A", "", "H", "H", "H", ""]
    # aniline: ring 0 - 5, N (6) on atom 0
    assert flags(types([6] * 6 + [7], ring + [(0, 6)], [1.5] * 6 + [1])) == ["", "H", "H", "H", "H", "H", "D"]
    # chlorobenzene
    t = types([6] * 6 + [17], ring + [(0, 6)], [1.5] * 6 + [1])
    assert flags(t) == ["H"] * 7 and int(t[6] & 15) == 6
    # a quaternary ammonium N accepts nothing; explicit hydrogens are counted; n_hydrogens overrides the valence rule
    assert flags(types([7, 6, 6, 6, 6], [(0, 1), (0, 2), (0, 3), (0, 4)], formal_charges=[1, 0, 0, 0, 0]))[0] == ""
    assert flags(types([7, 1, 1, 6], [(0, 1), (0, 2), (0, 3)]))[0] == "D"
    assert flags(types([7, 6, 6], [(0, 1), (0, 2)], n_hydrogens=[0, 3, 3]))[0] == "A"
    assert flags(types(["N", "C", "Cl", "Zn"], [(0, 1), (1, 2)]))[2:] == ["H", ""] and int(types(["Zn"], [])[0]) == 9
    with pytest.raises(ValueError, match="bond"):
        types([6, 6], [(0, 2)])
    with pytest.raises(ValueError, match="bond orders"):
        types([6, 6], [(0, 1)], [1, 1])


def test_receptor_types_by_names():
    from physdock_amd.scoring import receptor_types_from_names as types
    residues = {
        "ASP": (["N", "CA", "C", "O", "CB", "CG", "OD1", "OD2"], ["D", "", "", "A", "H", "", "A", "A"]),
        "LYS": (["N", "CA", "C", "O", "CB", "CG", "CD", "CE", "NZ"], ["D", "", "", "A", "H", "H", "H", "", "D"]),
        "SER": (["N", "CA", "C", "O", "CB", "OG"], ["D", "", "", "A", "", "DA"]),
        "PRO": (["N", "CA", "C", "O", "CB", "CG", "CD"], ["", "", "", "A", "H", "H", ""]),
        "PHE": (["N", "CA", "C", "O", "CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ", "OXT"], ["D", "", "", "A"] + ["H"] * 7 + ["A"]),
    }
    for res, (names, want) in residues.items():
        t = types([res] * len(names), names, [n[0] for n in names])
        assert flags(t) == want, res
        assert (t & 15).tolist() == [{"C": 0, "N": 1, "O": 2}[n[0]] for n in names]
    assert flags(types(["HIS"] * 3, ["ND1", "NE2", "CE1"], [7, 7, 6])) == ["DA", "DA", ""]
    # an unknown residue: the element rules, no donors
    assert flags(types(["XYZ"] * 4, ["N1", "C1", "O1", "ZN"], ["N", "C", "O", "Zn"])) == ["", "H", "A", ""]
    with pytest.raises(ValueError):
        types(["ALA"], ["N", "CA"], [7, 6])


def test_count_rotatable_bonds():
    from physdock_amd.scoring import count_rotatable_bonds as count
    chain = [(0, 1), (1, 2), (2, 3)]
    ring = [(i, (i + 1) % 6) for i in range(6)]
    assert count(4, chain, [1, 1, 1]) == 1 and count(4, chain) == 1                               # butane
    assert count(6, ring, [1] * 6) == 0                                                           # cyclohexane
    biphenyl = ring + [(6 + i, 6 + (i + 1) % 6) for i in range(6)] + [(0, 6)]
    assert count(12, biphenyl, [1.5] * 12 + [1]) == 1
    assert count(4, chain, [1, 3, 1]) == 0                                                        # 2-butyne
    assert count(5, chain + [(3, 4)], [1, 3, 1, 1]) == 0 and count(6, chain + [(3, 4), (4, 5)], [1, 3, 1, 1, 1]) == 1
    assert count(4, chain, [1, 2, 1]) == 0                                                        # 2-butene: the middle bond is double


# ------------------------------------------------------------------ VinaScore on the host, rank_by_score, arguments
def test_from_bonds_builds_the_tables_and_counts_the_rotors():
    from physdock_amd.scoring import VinaScore, receptor_types_from_names
    # pose: a SER residue (atoms 0 - 5), a zinc, a hydrogen, then butanol C-C-C-C-O scattered at 9, 8, 11, 10, 12
    names = ["N", "CA", "C", "O", "CB", "OG"]
    elements = [7, 6, 6, 8, 6, 8, 30, 1, 6, 6, 6, 6, 8]
    lig = [9, 8, 11, 10, 12]
    bonds = [(0, 1), (1, 2), (2, 3), (3, 4)]
    plain = VinaScore.from_bonds(elements, bonds, lig)
    assert plain.receptor_typing == "elements" and plain.n_rot == 2.0 and plain.n_atoms == 5 and plain.n_pose_atoms == 13
    assert plain.rec_mask.tolist() == [1] * 7 + [0] * 6 and plain.lig_active.tolist() == [1] * 5
    assert flags(plain.types[:7]) == ["", "H", "H", "", "H", "", ""] and int(plain.types[6] & 15) == 9
    assert flags(plain.types[lig]) == ["H", "H", "H", "", "DA"]
    rt = np.zeros(13, np.uint8)
    rt[:6] = receptor_types_from_names(["SER"] * 6, names, elements[:6])
    rt[6] = 9
    named = VinaScore.from_bonds(elements, bonds, lig, receptor_types=rt, n_rot=7, a_mask=[1] * 3 + [0] + [1] * 9)
    assert named.receptor_typing == "given" and named.n_rot == 7.0 and named.rec_mask.tolist() == [1, 1, 1, 0, 1, 1, 1] + [0] * 6
    assert flags(named.types[:6]) == ["D", "", "", "A", "", "DA"] and "VinaScore(n_atoms=5" in repr(named)
    with pytest.raises(ValueError, match="distinct"):
        VinaScore.from_bonds(elements, bonds, [9, 9, 11, 10, 12])
    with pytest.raises(ValueError, match="distinct"):
        VinaScore.from_types(np.zeros(4, np.uint8), [1, 4], np.ones(4), 0)
    with pytest.raises(ValueError, match="bits 0 - 6"):
        VinaScore.from_types(np.full(4, 200), [1], np.ones(4), 0)
    with pytest.raises(ValueError, match="n_rot"):
        VinaScore.from_types(np.zeros(4, np.uint8), [1], np.ones(4), -1)
    with pytest.raises(ValueError, match="receptor_mask"):
        VinaScore.from_types(np.zeros(4, np.uint8), [1], np.ones(5), 0)
    with pytest.raises(ValueError, match="ligand atoms"):
        VinaScore.from_types(np.zeros(2000, np.uint8), np.arange(1025), np.ones(2000), 0)
    with pytest.raises(ValueError, match="pose atoms"):
        plain.score(torch.zeros(2, 12, 3))
    v = VinaScore.from_types(np.zeros(4, np.uint8), [1], np.ones(4), 0)
    assert v.rec_mask.tolist() == [1, 0, 1, 1]                                      # a ligand atom never counts as receptor


def test_from_batch_reads_elements_masks_and_names():
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.scoring import VinaScore, names_from_meta
    from physdock_amd.synthetic import make_batch, pdb_meta
    batch = make_batch(20, 4, 9, 4, seed=6)
    is_lig = ligand_atom_mask(batch)
    n_lig = int(is_lig.sum())
    bonds = [(i, i + 1) for i in range(n_lig - 1)]
    v = VinaScore.from_batch(batch, bonds)
    z = (batch["ref_feat"][:, 4:132].argmax(-1) + 1).numpy()
    assert v.receptor_typing == "elements" and v.ligand_idx.tolist() == torch.nonzero(is_lig).flatten().tolist()
    exists = batch["a_mask"].numpy() > 0 if "a_mask" in batch else np.ones(len(z), bool)
    assert v.rec_mask.tolist() == (exists & ~is_lig.numpy() & (z != 1)).astype(int).tolist()
    assert not (v.types[~is_lig.numpy()] & 96).any() and (v.types & 15).tolist() == [ref_class(e) for e in z]
    meta = pdb_meta({k: batch[k].numpy() for k in ("token_id_to_chunk_sizes", "asym_id", "is_ligand", "residue_index")})
    res, names, zz, cls = names_from_meta(meta)
    assert len(res) == len(names) == len(zz) == len(cls) == len(z)
    named = VinaScore.from_batch(batch, bonds, infer_meta_data=meta, n_rot=2)
    assert named.receptor_typing == "names" and named.n_rot == 2.0 and np.array_equal(named.rec_mask, v.rec_mask)


def ref_class(z):
    return {6: 0, 7: 1, 8: 2, 15: 3, 16: 4, 9: 5, 17: 6, 35: 7, 53: 8}.get(int(z), 9)


def test_rank_by_score_orders_ascending_with_ties_and_valid_first():
    from physdock_amd.ranking import rank_by_score
    s = torch.tensor([-3.0, -7.5, -3.0, 1.0, -7.5, -9.0])
    assert rank_by_score({"score": s}).tolist() == [5, 1, 4, 0, 2, 3] == rank_by_score(s).tolist()
    valid = torch.tensor([True, False, True, True, True, False])
    assert rank_by_score({"score": s}, valid=valid).tolist() == [4, 0, 2, 3, 5, 1]
    assert rank_by_score(s, valid=torch.ones(6, dtype=torch.bool)).tolist() == [5, 1, 4, 0, 2, 3]
    assert rank_by_score(s).dtype == torch.long
    with pytest.raises(ValueError, match="bool mask"):
        rank_by_score(s, valid=torch.ones(5, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool mask"):
        rank_by_score(s, valid=torch.ones(6))


# ------------------------------------------------------------------ header, binding, package
def test_header_declares_the_launcher_and_the_abi_stays_11():
    import physdock_amd
    from physdock_amd import _lib, scoring
    assert physdock_amd.VinaScore is scoring.VinaScore
    assert _lib.ABI_VERSION == 11
    assert "pd_vina_score" in set(_lib.header_symbols())
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "physdock_hip.h")).read()
    assert int(re.search(r"#define\s+PD_VINA_TERMS\s+(\d+)", hdr).group(1)) == len(scoring.TERM_NAMES) == len(scoring.WEIGHTS) == 5
    src = open(_lib.os.path.join(_lib._HERE, "csrc", "vina.hip")).read()
    assert "PD_EXPORT int pd_vina_score(" in src and "expf(" in src and "__expf" not in src


def test_the_built_library_exports_and_binds_the_launcher():
    from physdock_amd import _lib
    L = _lib.lib()
    assert L.pd_abi_version() == 11
    assert hasattr(L, "pd_vina_score") and len(_lib.SYMBOLS["pd_vina_score"].argtypes) == 16
