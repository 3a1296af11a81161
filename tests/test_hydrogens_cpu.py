"""Hydrogens without a GPU: hydrogen perception of physdock_amd/hydrogens.py on small molecules and on the 20 residues, the float64
restatement (tests/hydrogens_ref.py) on hand-placed geometries, its invariance under a rigid motion, the class's derived tables and
checks, the header, the PDB template - and the conditions the GPU tests rest on: in every seeded case the best and the second-best
candidate of every rotor differ by at least 1e-6 A and no hydrogen-bond condition lies within 1e-9 (relative) of its threshold (one
`MARGIN | ...` line per case, pytest -s)."""
import re

import numpy as np
import pytest
import torch

import hydrogens_ref as ref

HEAVY = {"GLY": "", "ALA": "CB", "SER": "CB OG", "CYS": "CB SG", "VAL": "CB CG1 CG2", "THR": "CB OG1 CG2", "LEU": "CB CG CD1 CD2",
         "ILE": "CB CG1 CG2 CD1", "MET": "CB CG SD CE", "PRO": "CB CG CD", "PHE": "CB CG CD1 CD2 CE1 CE2 CZ",
         "TYR": "CB CG CD1 CD2 CE1 CE2 CZ OH", "TRP": "CB CG CD1 CD2 NE1 CE2 CE3 CZ2 CZ3 CH2", "ASP": "CB CG OD1 OD2",
         "GLU": "CB CG CD OE1 OE2", "ASN": "CB CG OD1 ND2", "GLN": "CB CG CD OE1 NE2", "HIS": "CB CG ND1 CD2 CE1 NE2", "LYS": "CB CG CD CE NZ",
         "ARG": "CB CG CD NE CZ NH1 NH2"}
IN_CHAIN = {"GLY": 3, "ALA": 5, "SER": 5, "CYS": 5, "VAL": 9, "THR": 7, "LEU": 11, "ILE": 11, "MET": 9, "PRO": 7, "PHE": 9, "TYR": 9, "TRP": 10,
            "ASP": 4, "GLU": 6, "ASN": 6, "GLN": 8, "HIS": 7, "LYS": 13, "ARG": 13}
DEG = np.pi / 180.0


def atoms_of(name):
    return ["N", "CA", "C", "O"] + HEAVY[name].split()


def rows_of(t, parent):
    return [(int(t["mode"][h]), t["ref"][h].tolist(), float(t["a"][h]), float(t["b"][h]), int(t["group"][h])) for h in np.nonzero(t["parent"] == parent)[0]]


# ------------------------------------------------------------------ perception
def test_ligand_hydrogens_of_small_molecules():
    from physdock_amd.hydrogens import BISECT, LINEAR, NERF, TRI, ligand_hydrogens_from_bonds as perceive
    f32 = lambda v: float(np.float32(v))
    tet, half, oh, trig = f32(ref.TETRAHEDRAL), f32(ref.HALF_TETRAHEDRAL), f32(ref.HYDROXYL), f32(ref.TRIGONAL)
    stag = [f32(60 * DEG), f32(np.pi), f32(300 * DEG)]
    # ethanol C0 - C1 - O2: a methyl, a CH2, a hydroxyl that is the one rotor
    t = perceive([6, 6, 8], [(0, 1), (1, 2)])
    assert len(t["parent"]) == 6 and t["parent"].tolist() == [0, 0, 0, 1, 1, 2]
    assert rows_of(t, 0) == [(NERF, [1, 2, -1], tet, b, -1) for b in stag]
    assert rows_of(t, 1) == [(BISECT, [0, 2, -1], half, 0.0, -1), (BISECT, [0, 2, -1], -half, 0.0, -1)]
    assert rows_of(t, 2) == [(NERF, [1, 0, -1], oh, f32(np.pi), 0)]
    assert t["length"].tolist() == [f32(1.09)] * 5 + [f32(0.96)]
    assert all(t[k].dtype == dt for k, dt in (("parent", np.int32), ("ref", np.int32), ("mode", np.uint8), ("length", np.float32),
                                              ("a", np.float32), ("b", np.float32), ("group", np.int32)))
    # benzene: six aromatic C-H in the plane of their neighbours
    ring = [(i, (i + 1) % 6) for i in range(6)]
    t = perceive([6] * 6, ring, [1.5] * 6)
    assert t["parent"].tolist() == list(range(6)) and (t["mode"] == BISECT).all() and not t["a"].any() and (t["group"] == -1).all()
    assert t["ref"].tolist() == [sorted([(i - 1) % 6, (i + 1) % 6]) + [-1] for i in range(6)]
    assert len(perceive([6] * 6, ring)["parent"]) == 12, "cyclohexane: two per carbon"
    # acetamide C0 - C1(=O2) - N3: a methyl and a planar NH2, cis and trans to the methyl carbon
    t = perceive([6, 6, 8, 7], [(0, 1), (1, 2), (1, 3)], [1, 2, 1])
    assert t["parent"].tolist() == [0, 0, 0, 3, 3]
    assert rows_of(t, 0) == [(NERF, [1, 2, -1], tet, b, -1) for b in stag]
    assert rows_of(t, 3) == [(NERF, [1, 0, -1], trig, 0.0, -1), (NERF, [1, 0, -1], trig, f32(np.pi), -1)]
    assert t["length"].tolist()[3:] == [f32(1.01)] * 2
    # methylammonium C0 - N1(+): too small to supply n2 - six rows, none can be placed, no rotor
    t = perceive([6, 7], [(0, 1)], formal_charges=[0, 1])
    assert t["parent"].tolist() == [0, 0, 0, 1, 1, 1] and (t["mode"] == NERF).all() and (t["ref"][:, 1:] == -1).all() and (t["group"] == -1).all()
    assert t["ref"][:, 0].tolist() == [1, 1, 1, 0, 0, 0]
    assert len(perceive([6, 7], [(0, 1)])["parent"]) == 5, "the neutral amine: two on the nitrogen"
    # ethylammonium C0 - C1 - N2(+): the three on the nitrogen are one rotor
    t = perceive([6, 6, 7], [(0, 1), (1, 2)], formal_charges=[0, 0, 1])
    assert rows_of(t, 2) == [(NERF, [1, 0, -1], tet, b, 0) for b in stag]
    # propyne C0 # C1 - C2: an sp C-H, and a methyl whose reference atoms are collinear in a straight molecule
    t = perceive([6, 6, 6], [(0, 1), (1, 2)], [3, 1])
    assert t["parent"].tolist() == [0, 2, 2, 2] and rows_of(t, 0) == [(LINEAR, [1, -1, -1], 0.0, 0.0, -1)]
    assert rows_of(t, 2) == [(NERF, [1, 0, -1], tet, b, -1) for b in stag]
    # isobutane: a methine on three methyls
    t = perceive([6] * 4, [(0, 1), (0, 2), (0, 3)])
    assert len(t["parent"]) == 10 and rows_of(t, 0) == [(TRI, [1, 2, 3], 0.0, 0.0, -1)]
    assert rows_of(t, 2) == [(NERF, [0, 1, -1], tet, b, -1) for b in stag]
    # explicit hydrogens are not placed twice; n_hydrogens overrides the valences; lengths= overrides the defaults
    assert perceive([6, 6, 8, 1], [(0, 1), (1, 2), (2, 3)])["parent"].tolist() == [0, 0, 0, 1, 1]
    assert perceive([6, 6, 8], [(0, 1), (1, 2)], n_hydrogens=[3, 2, 0])["parent"].tolist() == [0, 0, 0, 1, 1]
    assert perceive([6, 8], [(0, 1)], lengths={"O": 1.0, 6: 1.1})["length"].tolist() == [f32(1.1)] * 3 + [1.0]
    with pytest.raises(ValueError, match="lengths are positive"):
        perceive([6, 8], [(0, 1)], lengths={"P": 1.4})
    with pytest.raises(ValueError, match="another length"):
        perceive([6, 8], [(0, 1)], formal_charges=[0])


def test_the_hydrogen_count_is_the_one_the_typing_uses():
    """one valence rule: an atom is a DONOR of ligand_types_from_bonds exactly when it is N or O and rows ride on it"""
    from physdock_amd.hydrogens import ligand_hydrogens_from_bonds as perceive
    from physdock_amd.scoring import DONOR, ligand_types_from_bonds
    elements = [6, 6, 8, 7, 8, 6, 7, 16]
    bonds, orders = [(0, 1), (1, 2), (1, 3), (3, 5), (5, 4), (5, 6), (6, 7)], [1, 2, 1, 1, 2, 1, 1]
    t = perceive(elements, bonds, orders)
    types = ligand_types_from_bonds(elements, bonds, orders)
    carried = np.bincount(t["parent"], minlength=len(elements))
    assert carried.tolist() == [3, 0, 0, 1, 0, 0, 1, 1]
    assert [bool(types[i] & DONOR) for i in range(8)] == [bool(carried[i]) and elements[i] in (7, 8) for i in range(8)]


@pytest.mark.parametrize("name", sorted(IN_CHAIN))
def test_hydrogens_of_a_residue_in_chain_and_at_a_break(name):
    from physdock_amd.hydrogens import BISECT, receptor_hydrogens_from_names as perceive
    first, this = atoms_of("ALA"), atoms_of(name)
    res_names, atom_names = ["ALA"] * len(first) + [name] * len(this), first + this
    residue_of = [0] * len(first) + [1] * len(this)
    t = perceive(res_names, atom_names, residue_of)
    mine = t["parent"] >= len(first)
    assert int(mine.sum()) == IN_CHAIN[name] and int((~mine).sum()) == IN_CHAIN["ALA"] - 1
    n_atom = len(first) + this.index("N")
    amide = np.nonzero(t["parent"] == n_atom)[0]
    if name == "PRO":
        assert len(amide) == 0
    else:
        assert len(amide) == 1 and t["mode"][amide[0]] == BISECT and t["a"][amide[0]] == 0
        assert t["ref"][amide[0]].tolist() == [len(first) + this.index("CA"), first.index("C"), -1], "CA and the C of the previous residue"
    alone = perceive([name] * len(this), this, [0] * len(this))
    assert len(alone["parent"]) == IN_CHAIN[name] - (name != "PRO")
    for kw in (dict(chain_of=[0] * len(first) + [1] * len(this)), dict(residue_number=[4] * len(first) + [9] * len(this))):
        assert len(perceive(res_names, atom_names, residue_of, **kw)["parent"]) == IN_CHAIN["ALA"] - 1 + IN_CHAIN[name] - (name != "PRO")
    kw = dict(chain_of=[2] * len(atom_names), residue_number=[4] * len(first) + [5] * len(this))
    assert len(perceive(res_names, atom_names, residue_of, **kw)["parent"]) == len(t["parent"])
    # every ref lies in the residue (or is the previous C), differs from the parent, and rotors are the hydroxyls, thiols and ammonium
    assert all(r == -1 or (r != p and (residue_of[r] == residue_of[p] or atom_names[r] == "C")) for p, refs in zip(t["parent"], t["ref"]) for r in refs)
    rotors = sorted(atom_names[t["parent"][np.nonzero(t["group"] == g)[0][0]]] for g in range(t["group"].max() + 1))
    assert rotors == sorted({"SER": ["OG"], "THR": ["OG1"], "TYR": ["OH"], "CYS": ["SG"], "LYS": ["NZ"]}.get(name, []))


def test_missing_atoms_and_unknown_residues():
    from physdock_amd.hydrogens import receptor_hydrogens_from_names as perceive
    ser = atoms_of("SER")
    assert len(perceive(["SER"] * 6, ser, [0] * 6)["parent"]) == 4
    mask = [a != "CB" for a in ser]
    t = perceive(["SER"] * 6, ser, [0] * 6, mask=mask)
    assert len(t["parent"]) == 0, "without CB nothing on CA, CB or OG can be built"
    assert len(perceive(["SER"] * 5, ser[:5], [0] * 5)["parent"]) == 1, "a crop without OG keeps HA alone: OG is a ref of the CH2"
    assert len(perceive(["XYZ"] * 6, ser, [0] * 6)["parent"]) == 0
    assert len(perceive(["ser "] * 6, [" " + a.lower() for a in ser], [0] * 6)["parent"]) == 4
    with pytest.raises(ValueError, match="residue names"):
        perceive(["SER"] * 5, ser, [0] * 6)


# ------------------------------------------------------------------ the restatement on hand geometries
def angle(u, v):
    return np.arccos(np.clip(u @ v / np.linalg.norm(u) / np.linalg.norm(v), -1, 1)) / DEG


def dihedral(a, b, c, d):
    b0, b1, b2 = a - b, c - b, d - c
    b1 = b1 / np.linalg.norm(b1)
    v, w = b0 - (b0 @ b1) * b1, b2 - (b2 @ b1) * b1
    return np.arctan2(np.cross(b1, v) @ w, v @ w) / DEG


def test_the_restatement_on_hand_placed_geometries():
    c = ref.make_case("a_hand_P2")
    r = ref.reference("a_hand_P2")
    t, x = c["table"], c["x"].astype(np.float64)
    assert r["placed"].all() and sorted(set(t["mode"].tolist())) == [0, 1, 2, 3]
    for p in range(2):
        H = r["x_h64"][p]
        # every hydrogen at its length from its parent
        assert np.abs(np.linalg.norm(H - x[p, t["parent"]], axis=1) - t["length"].astype(np.float64)).max() < 1e-12
        par = lambda h: x[p, t["parent"][h]]
        # the CH2 (rows 1, 2) and the methyl (rows 4 - 6): H - C - H = 109.47 deg
        assert abs(angle(H[1] - par(1), H[2] - par(2)) - 109.4712) < 1e-3
        for i, j in ((4, 5), (5, 6), (4, 6)):
            assert abs(angle(H[i] - par(i), H[j] - par(j)) - 109.4712) < 1e-3
        # TRI: equal angles to the three neighbours;  BISECT in the plane: in the plane of the neighbours, equal angles to both
        tri = [angle(H[0] - x[p, 0], x[p, q] - x[p, 0]) for q in (1, 2, 3)]
        assert max(tri) > 90 and abs(angle(H[3] - x[p, 4], x[p, 1] - x[p, 4]) - angle(H[3] - x[p, 4], x[p, 5] - x[p, 4])) < 1e-9
        assert abs(np.cross(x[p, 1] - x[p, 4], x[p, 5] - x[p, 4]) @ (H[3] - x[p, 4])) < 1e-9
        # LINEAR: on the line through n1 and the parent, away from n1
        assert np.linalg.norm(np.cross(H[8] - x[p, 7], x[p, 7] - x[p, 5])) < 1e-12 and (H[8] - x[p, 7]) @ (x[p, 7] - x[p, 5]) > 0
        # NERF: a is the angle n1 - p - H, b the dihedral n2 - n1 - p - H; 0 is cis, 180 deg trans to n2
        assert abs(dihedral(x[p, 4], x[p, 5], x[p, 8], H[9])) < 1e-4 and abs(abs(dihedral(x[p, 4], x[p, 5], x[p, 8], H[10])) - 180) < 1e-4
        assert abs(angle(H[9] - x[p, 8], x[p, 5] - x[p, 8]) - 120) < 1e-4
        assert np.linalg.norm(H[9] - x[p, 4]) < np.linalg.norm(H[10] - x[p, 4]), "cis is the near one"
        for h, b in ((4, 60), (5, 180), (6, -60)):
            assert abs((dihedral(x[p, 1], x[p, 0], x[p, 2], H[h]) - b + 180) % 360 - 180) < 1e-3
        # the rotors: the hydroxyl H points at O12, an ammonium H at O14, and the choices are the ones the case was built for
        assert r["rotor_choice"][p].tolist() == [ref.A_OH_CHOICE[p], ref.A_NH3_CHOICE[p]]
        assert angle(H[7] - x[p, 6], x[p, 12] - x[p, 6]) < 1e-3
        assert min(angle(H[h] - x[p, 11], x[p, 14] - x[p, 11]) for h in (11, 12, 13)) < 1e-3
        assert abs(r["rotor_scores"][p, 0, ref.A_OH_CHOICE[p]] - (2.8 - 0.96)) < 1e-5 and np.isinf(r["rotor_scores"][p, 1, 4:]).all()
    # the bonds: the hydroxyl donates to residue 1, the ammonium of residue 0 to the ligand's O14; the far residue sees nothing
    assert r["bits"].tolist() == [[2, 1, 0]] * 2 and r["counts"].tolist() == [[1, 1]] * 2
    assert r["ligand_bits"].tolist() == [[0, 0, 0, 0, 0, 0, 1, 0, 0, 2]] * 2
    assert r["h_bits"][0].tolist() == [0] * 7 + [1] + [0] * 3 + [2 if h == int(np.argmax(r["h_bits"][0, 11:])) else 0 for h in range(3)]
    # without orientation the rotors keep their table angles and the hydroxyl no longer reaches O12 in pose 0 (it is 90 degrees off)
    plain = ref.place(c, orient=False)
    assert not plain["rotor_choice"].any() and np.array_equal(plain["x_h"][:, :7], r["x_h"][:, :7])
    assert abs(abs(dihedral(x[0, 0], x[0, 3], x[0, 6], plain["x_h64"][0, 7])) - 180) < 1e-4


@pytest.mark.parametrize("name", ["a_hand_P2", "b_seeded_P3"])
def test_the_hydrogens_move_rigidly_with_the_pose(name):
    c = ref.make_case(name)
    base = ref.reference(name)
    rot, shift = ref._rotation((0.3, -1.0, 0.7), 1.1), np.array([0.25, -0.5, 1.0])
    moved = dict(c, x=(c["x"].astype(np.float64) @ rot.T + shift).astype(np.float32))
    got = ref.place(moved)
    assert np.array_equal(got["placed"], base["placed"]) and np.array_equal(got["rotor_choice"], base["rotor_choice"])
    ok = base["placed"] > 0
    err = np.abs(got["x_h64"][ok] - (base["x_h64"][ok] @ rot.T + shift)).max()
    assert err < 2e-5, err                                            # the moved pose is rounded to fp32 anew: 1e-6 A per atom, levered by the frames
    hb = ref.hbonds(moved, got["x_h"], got["placed"])
    assert all(np.array_equal(hb[k], base[k]) for k in ("bits", "ligand_bits", "h_bits", "counts"))


# ------------------------------------------------------------------ the conditions the GPU tests rest on
@pytest.mark.parametrize("name", ref.CASES)
def test_no_rotor_and_no_bond_of_a_seeded_case_is_near_a_tie(name):
    c, r = ref.make_case(name), ref.reference(name)
    d = ref.derived(c)
    print(f"MARGIN | {name} | rotor {r['rotor_margin'].min():.3e} A | hbond {r['margin']:.3e} |")
    assert r["rotor_margin"].min() >= 1e-6 and r["margin"] >= 1e-9
    # the norms that decide `placed` are far from 1e-6 too: a row is placed in float64 exactly when it is with the limit at 1e-9 or 1e-3
    for tiny in (1e-9, 1e-3):
        old, ref.TINY = ref.TINY, tiny
        try:
            assert np.array_equal(ref.place(c, orient=False)["placed"], r["placed"])
        finally:
            ref.TINY = old
    t = c["table"]
    assert (r["bits"] & 1).any() and (r["bits"] & 2).any() and r["counts"].all() and not np.isnan(r["x_h"][r["placed"] > 0]).any()
    assert np.isnan(r["x_h"][r["placed"] == 0]).all() and not r["h_bits"][r["placed"] == 0].any()
    sizes = sorted({int((g >= 0).sum()) for g in d["group_h"]})
    assert sizes == [1, 3] and {int(d["side"][g[0]]) for g in d["group_h"]} == {0, 1}
    if name == "b_seeded_P3":
        assert c["x"].shape == (3, 64, 3) and len(c["lig_idx"]) == 24 and c["n_residues"] == 6 and int(np.isnan(c["x"]).sum()) == 1
        assert not r["placed"][:, c["degenerate_row"]].any(), "collinear neighbours"
        assert r["placed"][:, c["nan_row"]].tolist() == [1, 0, 1], "the NaN poisons its row in its pose alone"
        g = [k for k, rows in enumerate(d["group_h"]) if rows[0] == c["lone_rotor_row"]][0]
        assert np.isinf(r["rotor_scores"][:, g]).all() and not r["rotor_choice"][:, g].any() and r["placed"][:, c["lone_rotor_row"]].all()
        assert (r["rotor_choice"] > 0).any() and len(set(map(bytes, r["bits"]))) > 1
    if name == "c_blocks_P2":
        H, L, R = len(t["parent"]), len(c["lig_idx"]), c["n_residues"]
        assert c["x"].shape[0] == 2 and H > ref.PLACE_BLOCK and d["NA_r"] > ref.HBOND_BLOCK and d["NA_l"] > ref.ROTOR_BLOCK
        assert R > ref.FOLD_BLOCK and L > ref.FOLD_BLOCK and H > ref.FOLD_BLOCK and d["HP_l"] > 0 and d["HP_r"] > ref.FOLD_BLOCK
        assert (r["bits"][:, ref.FOLD_BLOCK:] != 0).any() and (r["ligand_bits"][:, ref.FOLD_BLOCK:] != 0).any() and (r["h_bits"][:, ref.PLACE_BLOCK:] != 0).any()
        src = open(__file__.replace("tests/test_hydrogens_cpu.py", "physdock_amd/csrc/hydrogens.hip")).read()
        for const in ("PLACE_BLOCK", "ROTOR_BLOCK", "HBOND_BLOCK", "FOLD_BLOCK"):
            assert int(re.search(rf"constexpr int {const} = (\d+);", src).group(1)) == getattr(ref, const)


# ------------------------------------------------------------------ the class on the host
def hy_of(c, **kw):
    from physdock_amd.hydrogens import Hydrogens
    return Hydrogens.from_tables(c["types"], c["lig_idx"], c["rec_mask"], c["residue_of"], c["table"], n_residues=c["n_residues"],
                                 ligand_active=c["lig_active"], thresholds=c["thresholds"], **kw)


@pytest.mark.parametrize("name", ref.CASES)
def test_the_tables_of_the_seeded_cases(name):
    c = ref.make_case(name)
    f, d = hy_of(c), ref.derived(c)
    for k in ("side", "group_h", "acc", "racc_start", "lig_acc_slot", "polar", "rh_start", "polar_slot"):
        assert np.array_equal(getattr(f, k), d[k]) and getattr(f, k).dtype == d[k].dtype, k
    assert (f.n_receptor_acceptors, f.n_ligand_acceptors, f.n_ligand_polar, f.n_receptor_polar) == (d["NA_r"], d["NA_l"], d["HP_l"], d["HP_r"])
    assert (f.n_hydrogens, f.n_groups, f.n_atoms, f.n_pose_atoms) == (len(c["table"]["parent"]), len(d["group_h"]), len(c["lig_idx"]), c["x"].shape[1])
    assert list(f._thr) == [4.1, np.cos(np.deg2rad(100.0))] and f.thresholds == {"d_da": 4.1, "angle_min": 100.0}
    assert all(np.array_equal(f.table[k], c["table"][k]) for k in ("parent", "ref", "mode", "length", "a", "b"))


def test_constructor_argument_errors():
    from physdock_amd import hydrogens as HY
    c = ref.make_case("a_hand_P2")
    t = c["table"]
    hy_of(c)
    change = lambda **kw: dict(c, table={**t, **kw})
    edit = lambda key, h, v: (lambda a: (a.__setitem__(h, v), a)[1])(t[key].copy())
    for bad, match in ((change(ref=edit("ref", 0, [0, 2, 3])), "other than the parent"), (change(ref=edit("ref", 0, [1, 2, 16])), "other than the parent"),
                       (change(parent=edit("parent", 0, 16)), "rides on"), (change(mode=edit("mode", 0, 4)), "the modes are"),
                       (change(length=edit("length", 0, 0.0)), "finite and positive"), (change(b=edit("b", 0, np.nan)), "finite"),
                       (change(group=edit("group", 8, 0)), "1 or 3 hydrogens"), (change(group=edit("group", 12, -1)), "1 or 3 hydrogens"),
                       (change(group=edit("group", 11, 0), ), "1 or 3 hydrogens"),
                       (change(parent=t["parent"][:5]), "another length")):
        with pytest.raises(ValueError, match=match):
            hy_of(bad)
    three = edit("group", 4, 5)
    three[5] = three[6] = 5                                            # the methyl as a group: fine, it shares parent, n1 and n2
    assert hy_of(change(group=three)).n_groups == 3
    mixed = edit("group", 9, 7)
    mixed[10], mixed[8] = 7, 7                                         # two NH2 rows and the LINEAR row: not one rotor
    with pytest.raises(ValueError, match="share parent, n1 and n2"):
        hy_of(change(group=mixed))
    with pytest.raises(ValueError, match="lacks"):
        hy_of(dict(c, table={k: v for k, v in t.items() if k != "b"}))
    many = HY.join_hydrogen_tables(*[{k: v[:4] for k, v in t.items()}] * 16384)
    assert len(many["parent"]) == 65536
    with pytest.raises(ValueError, match="1 .. 65535"):
        hy_of(dict(c, table=many))
    with pytest.raises(ValueError, match="1 .. 65535"):
        hy_of(dict(c, table={k: v[:0] for k, v in t.items()}))
    for thr, match in (({"d_da": -1.0}, "finite and not negative"), ({"angle_min": 181.0}, "0 .. 180"), ({"hbond": 3.5}, "unknown thresholds"),
                       ((4.1,), "got 1 values")):
        with pytest.raises(ValueError, match=match):
            hy_of(dict(c, thresholds=thr))
    f = hy_of(dict(c, thresholds={"angle_min": 120.0}), residue_labels=["LYS7", "ASP9", "GLU30"])
    assert f.thresholds == {"d_da": 4.1, "angle_min": 120.0} and f._thr[1] == np.cos(np.deg2rad(120.0))
    assert f.describe(np.array([2, 1, 0], np.uint8)) == [("LYS7", ["hbond_acceptor"]), ("ASP9", ["hbond_donor"])]
    assert f.required_row([("ASP9", "hbond_donor"), (0, "hbond_acceptor")]).tolist() == [2, 1, 0]
    with pytest.raises(ValueError, match="unknown interaction kind"):
        f.required_row([(0, "contact")])
    with pytest.raises(ValueError, match="pose atoms"):
        f.place(torch.zeros(2, 15, 3))
    with pytest.raises(ValueError, match="Hydrogens.compare: bits must be a uint8 tensor"):
        f.compare(torch.zeros(2, 3), torch.zeros(3, dtype=torch.uint8))
    assert HY.hbond_kind_mask() == 3 and HY.hbond_kind_mask("hbond_acceptor") == 2
    assert "Hydrogens(n_atoms=10, n_pose_atoms=16, residues=3, hydrogens=14, rotor_groups=2, polar=3+3, acceptors=2+2" in repr(f)
    joined = HY.join_hydrogen_tables(t, t)
    assert joined["group"].tolist() == t["group"].tolist() + [g + 2 if g >= 0 else -1 for g in t["group"].tolist()]


def test_from_bonds_and_from_batch():
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.hydrogens import Hydrogens, ligand_hydrogens_from_bonds, receptor_hydrogens_from_names
    from physdock_amd.interactions import InteractionFingerprint
    from physdock_amd.scoring import names_from_meta
    from physdock_amd.synthetic import make_batch, pdb_meta
    # ethanol next to a serine: local bond indices become pose atoms, the receptor's table is taken as given
    ser = atoms_of("SER")
    rec = receptor_hydrogens_from_names(["SER"] * 6, ser, [0] * 6)
    elements = [7, 6, 6, 8, 6, 8] + [8, 6, 6]                          # the ligand is O6 - C7 - C8: pose atoms 8, 7, 6 in local order
    f = Hydrogens.from_bonds(elements, [(0, 1), (1, 2)], [8, 7, 6], [0] * 6 + [1] * 3, receptor_hydrogens=rec)
    assert f.receptor_typing == "elements" and f.n_hydrogens == 4 + 6 and f.side.tolist() == [0] * 4 + [1] * 6
    assert f.parent[4:].tolist() == [8, 8, 8, 7, 7, 6] and f.ref[4].tolist() == [7, 6, -1] and f.ref[9].tolist() == [7, 8, -1]
    assert f.n_groups == 2 and f.group_h.tolist() == [[3, -1, -1], [9, -1, -1]] and f.n_receptor_acceptors == 0
    assert f.polar.tolist() == [9, 3] and f.n_ligand_acceptors == 1 and f.acc.tolist() == [6]
    gone = Hydrogens.from_bonds(elements, [(0, 1), (1, 2)], [8, 7, 6], [0] * 6 + [1] * 3, a_mask=[1] * 8 + [0])
    assert gone.parent.tolist() == [7, 7, 6] and gone.ref.tolist() == [[-1, 6, -1]] * 2 + [[7, -1, -1]], "an atom that does not exist"
    # a feature dict without and with names
    batch = make_batch(20, 4, 9, 4, seed=6)
    is_lig = ligand_atom_mask(batch).numpy()
    n_lig = int(is_lig.sum())
    bonds = [(i, i + 1) for i in range(n_lig - 1)]
    f = Hydrogens.from_batch(batch, bonds)
    g = InteractionFingerprint.from_batch(batch, bonds)
    z = (batch["ref_feat"][:, 4:132].argmax(-1) + 1).numpy()
    want = ligand_hydrogens_from_bonds(z[g.ligand_idx], bonds)
    assert f.receptor_typing == "elements" and f.residue_labels is None and f.side.all() and f.n_receptor_acceptors == 0
    assert f.n_hydrogens == int((g.lig_active[want["parent"]] > 0).sum()) > 0
    for k in ("types", "ligand_idx", "lig_active", "rec_mask", "residue_of"):
        assert np.array_equal(getattr(f, k), getattr(g, k)), k
    meta = pdb_meta({k: batch[k].numpy() for k in ("token_id_to_chunk_sizes", "asym_id", "is_ligand", "residue_index")})
    named = Hydrogens.from_batch(batch, bonds, infer_meta_data=meta, thresholds={"d_da": 3.9})
    gn = InteractionFingerprint.from_batch(batch, bonds, infer_meta_data=meta)
    assert named.receptor_typing == "names" and named.thresholds == {"d_da": 3.9, "angle_min": 100.0} and named.residue_labels == gn.residue_labels
    assert np.array_equal(named.types, gn.types) and (named.side == 0).sum() > 0 and named.n_receptor_acceptors > 0
    res, names, zz, _ = names_from_meta(meta)
    rid = batch["atom_id_to_token_id"].numpy()
    rec = receptor_hydrogens_from_names(res, names, rid, named.rec_mask, chain_of=batch["asym_id"].numpy()[rid],
                                        residue_number=batch["residue_index"].numpy()[rid])
    assert np.array_equal(named.parent[named.side == 0], rec["parent"]) and (named.rec_mask[rec["parent"]] > 0).all()


def test_constants_header_and_library():
    import physdock_amd
    from physdock_amd import _lib, hydrogens as HY
    assert physdock_amd.Hydrogens is HY.Hydrogens and issubclass(HY.Hydrogens, physdock_amd.interactions._ByteRows)
    assert HY.HBOND_KIND_NAMES == ref.HBOND_KIND_NAMES == ("hbond_donor", "hbond_acceptor") and HY.HBOND_THRESHOLD_NAMES == ref.THRESHOLD_NAMES
    assert tuple(HY.DEFAULT_HBOND_THRESHOLDS[k] for k in HY.HBOND_THRESHOLD_NAMES) == ref.THRESHOLDS == (4.1, 100.0)
    assert HY.DEFAULT_LENGTHS == ref.LENGTHS == {6: 1.09, 7: 1.01, 8: 0.96, 16: 1.34}
    assert (HY.TRI, HY.BISECT, HY.NERF, HY.LINEAR) == (ref.TRI, ref.BISECT, ref.NERF, ref.LINEAR) and HY.ACCEPTOR == ref.ACCEPTOR
    assert HY.TETRAHEDRAL == ref.TETRAHEDRAL and abs(HY.HALF_TETRAHEDRAL / DEG - 54.7356) < 1e-4 and HY.MAX_HYDROGENS == 65535
    assert _lib.ABI_VERSION == 11
    new = {"pd_place_hydrogens": 22, "pd_hydrogen_bonds": 28, "pd_hydrogen_bonds_workspace": 5}
    assert set(new) <= set(_lib.header_symbols())
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "physdock_hip.h")).read()
    for k, v in (("PD_H_TRI", 0), ("PD_H_BISECT", 1), ("PD_H_NERF", 2), ("PD_H_LINEAR", 3), ("PD_HBOND_KINDS", 2), ("PD_HBOND_THRESHOLDS", 2)):
        assert int(re.search(rf"#define\s+{k}\s+(\d+)", hdr).group(1)) == v
    for name, n in new.items():
        decl = re.search(rf"^int {name}\((.*?)\);", hdr, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == n, name
    L = _lib.lib()
    assert L.pd_abi_version() == 11
    assert all(hasattr(L, k) and k in _lib.SYMBOLS and len(_lib.SYMBOLS[k].argtypes) == n for k, n in new.items())
    # the workspace size needs no device: per pose an int per polar row and a byte per (row, acceptor of the other side)
    ws = L.pd_hydrogen_bonds_workspace
    assert ws(3, 5, 40, 30, 7) == (3 * (4 * 45 + 5 * 30 + 40 * 7) + 7) // 8 * 8
    assert ws(1, 1, 0, 1, 0) == 8 and ws(1, 0, 0, 0, 0) == 8 and ws(2, 0, 3, 0, 0) == 24
    assert ws(0, 5, 40, 30, 7) == -1 and ws(3, -1, 40, 30, 7) == -1 and ws(3, 5, 40, 30, -2) == -1
    assert ws(65535, 100, 60000, 1 << 20, 1024) == -3, "more than an int holds"


def test_redock_takes_the_keyword_on_every_path():
    import inspect
    from physdock_amd import driver
    assert inspect.signature(driver.redock).parameters["hydrogens"].default is None
    assert inspect.signature(driver._RedockState.__init__).parameters["hydrogens"].default is None
    c = ref.make_case("a_hand_P2")
    batch = {"x_gt": torch.zeros(17, 3)}
    with pytest.raises(ValueError, match="built over 16 pose atoms, the batch holds 17"):
        driver.check_hydrogens(hy_of(c), batch)
    with pytest.raises(ValueError, match="takes a hydrogens.Hydrogens"):
        driver.check_hydrogens(object(), batch)
    driver.check_hydrogens(None, batch), driver.check_hydrogens(hy_of(c), {"x_gt": torch.zeros(16, 3)})


# ------------------------------------------------------------------ the PDB template
def test_pdb_template_text_of_a_two_residue_system():
    from physdock_amd.hydrogens import Hydrogens, receptor_hydrogens_from_names
    from physdock_amd.pdbio import PdbTemplate
    from physdock_amd.scoring import receptor_types_from_names
    ser, gly = atoms_of("SER"), atoms_of("GLY")
    z_of = {"C": 6, "N": 7, "O": 8}
    conf = {"SER": {"ref_atom_name_chars": ser, "ref_element": [z_of[a[0]] - 1 for a in ser]},
            "GLY": {"ref_atom_name_chars": gly, "ref_element": [z_of[a[0]] - 1 for a in gly]},
            "LIG": {"ref_atom_name_chars": ["C1", "O1"], "ref_element": [5, 7]}}
    meta = {"ccds": ["SER", "GLY", "LIG"], "atom_id_to_conformer_atom_id": np.array(list(range(6)) + list(range(4)) + [0, 1]),
            "conformer_id_to_chunk_sizes": np.array([6, 4, 2]), "CHAIN_CLASS": ["protein", "protein", "ligand"], "CONF_META_DATA": conf,
            "residue_index": np.array([6, 7, 0]), "asym_id": np.array([0, 0, 1])}
    res, names, residue_of = ["SER"] * 6 + ["GLY"] * 4 + ["LIG"] * 2, ser + gly + ["C1", "O1"], [0] * 6 + [1] * 4 + [2] * 2
    elements = [z_of[a[0]] for a in names]
    rec = receptor_hydrogens_from_names(res[:10], names[:10], residue_of[:10])
    hy = Hydrogens.from_bonds(elements, [(0, 1)], [10, 11], residue_of, receptor_types=receptor_types_from_names(res, names, elements),
                              receptor_hydrogens=rec)
    assert hy.n_hydrogens == 4 + 3 + 4
    base = PdbTemplate(meta)
    full = hy.pdb_template(base)
    assert (full.n_atoms, full.n_records) == (12 + 11, 12 + 11) and full.atom.tolist() == list(range(23))
    assert torch.equal(full.rows[:12], base.rows) and full.rows.dtype == torch.uint8
    text = [bytes(r).decode("ascii") for r in full.rows.numpy()]
    assert all(len(t) == 81 and t[-1] == "\n" for t in text)
    line = lambda rec_, serial, name, resn, chain, num: (f"{rec_:<6}{serial:>5}  {name:<3} {resn:>3} {chain}{num:>4}    {'':>24}{1.0:>6.2f}{70.0:>6.2f}"
                                                       f"          {'H':>2}{0:>2}\n")
    want = [line("ATOM", 13 + k, f"H{k + 1}", "SER", "A", 7) for k in range(4)] + [line("ATOM", 17 + k, f"H{k + 1}", "GLY", "A", 8) for k in range(3)] + \
           [line("HETATM", 20 + k, f"H{k + 1}", "LIG", "B", 1) for k in range(4)]
    assert text[12:] == want
    assert text[12] == "ATOM     13  H1  SER A   7                              1.00 70.00           H 0\n"
    # the receptor-only template keeps the receptor's hydrogens, with the same serials and atom indices
    rec_only = hy.pdb_template(PdbTemplate(meta, receptor_only=True))
    assert rec_only.n_records == 10 + 7 and rec_only.atom.tolist() == list(range(10)) + list(range(12, 19))
    assert [bytes(r).decode("ascii") for r in rec_only.rows.numpy()][10:] == want[:7]
    with pytest.raises(ValueError, match="the template is over"):
        hy.pdb_template(PdbTemplate.from_rows(base.rows[:3], base.atom[:3], 5))
    with pytest.raises(ValueError, match="from_rows"):
        PdbTemplate.from_rows(base.rows[:3], [0, 1, 7], 5)
