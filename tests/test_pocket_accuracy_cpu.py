"""PocketAccuracy without a GPU: the float64 restatement (tests/pocket_accuracy_ref.py) on the seeded cases of
tests/pocket_accuracy_cases.py, the host code that builds the tables (physdock_amd/pocket_accuracy.py), the header and the driver's
argument checks.

The SEED CONDITION is checked here on the restatement alone: for every case and pose no compare | |d_pose - d_ref| - t | falls below
1e-9 A and no swap decision of a residue with pairs is a tie.  Two float64 evaluations of a distance differ by a few ulp (about 1e-14 A
inside the box), so a device that counts in float64 must then reproduce every integer exactly - what tests/test_pocket_accuracy_gpu.py
demands."""
import re

import numpy as np
import pytest
import torch

import pocket_accuracy_cases as cases
import pocket_accuracy_ref as ref

MIN_MARGIN = 1e-9


def spec(name, **over):
    from physdock_amd import PocketAccuracy
    r = cases.reference(name)
    s = r["s"]
    return PocketAccuracy.from_names(s["res_names"], s["atom_names"], s["residue_of"], s["x_ref"], s["ligand_idx"], mask=s["mask"],
                                     **dict(r["kw"], **over))


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize("name", list(cases.CASES))
def test_host_tables_equal_the_restatement(name):
    r = cases.reference(name)
    t, obj = r["tab"], spec(name)
    same = dict(pocket_residues="pocket", patom="patom", res_atom_start="res_atom_start", pair_start="pair_start", pair_atom="pair_atom",
                pair_dist="pair_dist", atom_partner="partner", atom_slot="atom_slot", named="named", patom_ref="patom_ref",
                swappable="swappable")
    for mine, theirs in same.items():
        a, b = getattr(obj, mine), t[theirs]
        assert a.shape == b.shape and (a == b).all(), (name, mine)
    assert (obj.patom_partner == t["partner"][t["patom"]]).all()
    assert ((obj.patom_kind & 1 != 0) == t["patom_ca"]).all() and ((obj.patom_kind & 2 != 0) == t["patom_bb"]).all()
    assert obj.pair_dist.dtype == np.float64 and obj.patom_ref.dtype == np.float64 and obj.n_pairs == r["out"]["n_pairs"]
    assert (obj.residue_pairs == r["out"]["res_pairs"]).all() and obj.n_pose_atoms == t["A"]


@pytest.mark.parametrize("name", ["nine", "far", "row256"])
def test_pairs_against_brute_force(name):
    r = cases.reference(name)
    s, t = r["s"], r["tab"]
    x, res = s["x_ref"], s["residue_of"]
    rec = s["mask"].copy()
    rec[s["ligand_idx"]] = False
    radius = r["kw"].get("inclusion_radius", 15.0)
    pocket_radius = r["kw"].get("pocket_radius", 8.0)
    d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    near = {int(res[a]) for a in np.nonzero(rec)[0] if (d[a, s["ligand_idx"]] < pocket_radius).any()}
    assert sorted(near) == t["pocket"].tolist()
    assert t["patom"].tolist() == [a for a in sorted(np.nonzero(rec)[0], key=lambda a: (res[a], a)) if int(res[a]) in near]
    for k, i in enumerate(t["patom"]):
        row = t["pair_atom"][t["pair_start"][k]:t["pair_start"][k + 1]]
        want = [j for j in range(len(x)) if rec[j] and res[j] != res[i] and d[i, j] < radius]
        assert row.tolist() == want and (t["pair_dist"][t["pair_start"][k]:t["pair_start"][k + 1]] == d[i, want]).all()
    assert not np.isin(t["pair_atom"], s["ligand_idx"]).any() and not np.isin(t["named"], np.nonzero(~rec)[0]).any()


def test_pocket_choice_environment_and_missing_atoms():
    r = cases.reference("far")
    s, t = r["s"], r["tab"]
    assert t["pocket"].tolist() == [0, 1, 2, 3, 4, 5, 6]                       # the residues 5 A from the ligand; 13 A and 17 A are not
    env = set(s["residue_of"][t["pair_atom"]].tolist()) - set(t["pocket"].tolist())
    assert {7, 8, 9} <= env                                                    # environment residues are pair partners only
    assert t["swappable"].tolist() == [True, True, False, True, True, True, False]      # GLY has none; ASP 6 lacks OD2
    od1 = cases.atom(s, 6, "OD1")
    assert t["partner"][od1] == od1 and not s["mask"][cases.atom(s, 6, "OD2")]
    hydrogens = [a for a, n in enumerate(s["atom_names"]) if n == "H"]
    assert len(hydrogens) == 2 and not np.isin(hydrogens, t["named"]).any()
    assert (t["partner"][s["residue_of"] >= 7] == np.arange(t["A"])[s["residue_of"] >= 7]).all(), "swaps are for pocket residues only"


def test_swap_table_from_names():
    from physdock_amd import swap_table_from_names
    from physdock_amd.pocket_accuracy import SWAP_NAMES
    assert SWAP_NAMES == ref.SWAPS and set(SWAP_NAMES) == {"ASP", "GLU", "ARG", "LEU", "VAL", "PHE", "TYR"}
    s = cases.reference("nine")["s"]
    tab = swap_table_from_names(s["res_names"], s["atom_names"], s["residue_of"])
    assert tab.dtype == np.int32 and tab.shape == (9, 2)                       # five residues with one pair, PHE and TYR with two
    assert (tab == ref.swap_table(s["res_names"], s["atom_names"], s["residue_of"])).all()
    named = [(s["res_names"][a], s["atom_names"][a], s["atom_names"][b]) for a, b in tab]
    assert named == [("ASP", "OD1", "OD2"), ("GLU", "OE1", "OE2"), ("ARG", "NH1", "NH2"), ("LEU", "CD1", "CD2"), ("VAL", "CG1", "CG2"),
                     ("PHE", "CD1", "CD2"), ("PHE", "CE1", "CE2"), ("TYR", "CD1", "CD2"), ("TYR", "CE1", "CE2")]
    mask = np.ones(len(s["atom_names"]), bool)
    mask[cases.atom(s, 5, "CE2")] = False                                      # PHE without CE2: neither of its pairs
    cut = swap_table_from_names(s["res_names"], s["atom_names"], s["residue_of"], mask)
    assert cut.shape == (7, 2) and not any(s["res_names"][a] == "PHE" for a, _ in cut)


def test_row_lengths_of_the_tile_cases():
    from physdock_amd.pocket_accuracy import PAIR_TILE
    assert PAIR_TILE == 256
    for name, n in (("row1", 1), ("row256", 256), ("row257", 257)):
        t = cases.reference(name)["tab"]
        assert np.diff(t["pair_start"])[0] == n, name
        assert t["A"] % 64 != 0
    rows = np.diff(cases.reference("row257")["tab"]["pair_start"])
    assert rows.max() > 257 and rows.min() < 256                               # rows on both sides of the tile in one launch


# ------------------------------------------------------------------ the restatement on the special poses
def test_a_pose_equal_to_the_reference():
    o = cases.reference("nine")["out"]
    assert o["lddt_lp"][0] == 1.0 and (o["residue_lddt"][0] == 1.0).all() and o["swapped"][0].sum() == 0
    assert (o["conserved"][0] == o["n_pairs"]).all() and o["ok"][0] == 1 and o["fit_ok"][0] == 1
    assert max(o["ca_rmsd"][0], o["backbone_rmsd"][0], o["heavy_rmsd"][0], o["residue_rmsd"][0].max()) <= 1e-6


@pytest.mark.parametrize("pose,residues", [(1, [0]), (2, [5]), (3, [3, 4])])
def test_exchanged_names_are_found_and_undone(pose, residues):
    r = cases.reference("nine")
    o = r["out"]
    assert o["lddt_lp"][pose] == 1.0 and np.nonzero(o["swapped"][pose])[0].tolist() == residues
    assert o["heavy_rmsd"][pose] <= 1e-6 and o["residue_rmsd"][pose].max() <= 1e-6
    plain = ref.score(r["tab"], r["x"][pose:pose + 1], swaps=False)
    assert plain["lddt_lp"][0] < 1.0 and plain["swapped"].sum() == 0, "the swap logic is live"
    assert plain["residue_rmsd"][0][residues].min() > 0.1 and plain["heavy_rmsd"][0] > 0.01


def test_a_rigidly_moved_reference():
    o = cases.reference("nine")["out"]
    assert o["lddt_lp"][4] == 1.0 and o["swapped"][4].sum() == 0
    assert max(o["ca_rmsd"][4], o["backbone_rmsd"][4], o["heavy_rmsd"][4], o["residue_rmsd"][4].max()) <= 1e-6
    # pose = Q ref + SHIFT, so the transform from the pose to the reference is (Q^T, -Q^T SHIFT)
    assert np.abs(ref.rotation(o["quat"][4]) - cases.QUARTER.T).max() <= 1e-9
    assert np.abs(o["t"][4] + cases.QUARTER.T @ cases.SHIFT).max() <= 1e-9
    # a general rotation is rounded to the grid of 2^-10 A: at most 2^-11 A per coordinate
    assert o["lddt_lp"][5] == 1.0 and o["heavy_rmsd"][5] <= np.sqrt(3.0) * 2.0 ** -11 and o["ca_rmsd"][5] > 0


def test_a_mirrored_pocket_does_not_fit():
    o = cases.reference("nine")["out"]
    assert o["lddt_lp"][6] == 1.0 and o["fit_ok"][6] == 1 and o["ca_rmsd"][6] > 1.0 and o["heavy_rmsd"][6] > 1.0


def test_small_pockets_and_no_pairs():
    one, two, nop = (cases.reference(n) for n in ("one", "two", "nopairs"))
    assert len(one["tab"]["pocket"]) == 1 and len(two["tab"]["pocket"]) == 2
    for r in (one, two):
        o = r["out"]
        assert (o["fit_ok"] == 0).all() and (o["ok"] == 1).all() and np.isnan(o["ca_rmsd"]).all() and np.isnan(o["quat"]).all()
        assert np.isfinite(o["lddt_lp"]).all() and o["lddt_lp"][0] == 1.0 and o["lddt_lp"][-1] < 1.0
    assert one["out"]["swapped"][:, 0].tolist() == [0, 1, 0] and one["out"]["lddt_lp"][1] == 1.0
    assert nop["out"]["n_pairs"] == 0 and (nop["out"]["lddt_lp"] == 0).all() and (nop["out"]["residue_lddt"] == 0).all()
    assert (nop["out"]["conserved"] == 0).all() and (nop["out"]["swapped"] == 0).all()


def test_non_finite_coordinates():
    r = cases.reference("far")
    t, s = r["tab"], r["s"]
    pocket_atom = int(t["patom"][3])
    env_atom = int(next(j for j in t["pair_atom"] if t["atom_slot"][j] < 0))
    unnamed = int(s["ligand_idx"][0])
    x = np.repeat(r["x"][:1], 4, 0)
    x[1, pocket_atom, 0], x[2, env_atom, 2], x[3, unnamed, 1] = np.nan, np.inf, np.nan
    o = ref.score(t, x)
    assert o["ok"].tolist() == [1, 0, 0, 1] and o["fit_ok"].tolist() == [1, 0, 0, 1]
    for p in (1, 2):
        assert np.isnan(o["lddt_lp"][p]) and np.isnan(o["residue_lddt"][p]).all() and np.isnan(o["heavy_rmsd"][p]) and np.isnan(o["t"][p]).all()
        assert (o["conserved"][p] == 0).all() and (o["swapped"][p] == 0).all()
    for k in ("lddt_lp", "residue_lddt", "conserved", "swapped", "ca_rmsd", "heavy_rmsd", "residue_rmsd", "quat", "t"):
        assert (o[k][3] == o[k][0]).all(), "an atom no table names changes nothing"


@pytest.mark.parametrize("name", list(cases.CASES))
def test_seed_condition(name):
    o = cases.reference(name)["out"]
    print(f"POCKET-ACCURACY | {name} | smallest margin {o['margin'].min():.3e} A | ties {int(o['ties'].sum())} |")
    assert o["margin"].min() >= MIN_MARGIN and o["ties"].sum() == 0


# ------------------------------------------------------------------ the host class
def test_the_spec_is_immutable_and_checks_its_arguments():
    from physdock_amd import PocketAccuracy
    obj = spec("nine")
    with pytest.raises(AttributeError):
        obj.pocket_radius = 9.0
    with pytest.raises(ValueError):
        obj.pair_atom[0] = 0
    assert "pocket_residues=9" in repr(obj) and obj.n_ca == 9 and obj.thresholds == (0.5, 1.0, 2.0, 4.0)
    s = cases.reference("nine")["s"]
    args = (s["res_names"], s["atom_names"], s["residue_of"], s["x_ref"], s["ligand_idx"])
    with pytest.raises(ValueError, match="four positive thresholds"):
        PocketAccuracy.from_names(*args, thresholds=(0.5, 1.0, 2.0))
    with pytest.raises(ValueError, match="no receptor atom"):
        PocketAccuracy.from_names(*args, pocket_radius=1e-3)
    with pytest.raises(ValueError, match="ligand_idx"):
        PocketAccuracy.from_names(*args[:4], [0, 0])
    with pytest.raises(ValueError, match="not finite"):
        bad = np.array(s["x_ref"])
        bad[3, 0] = np.nan
        PocketAccuracy.from_names(*args[:3], bad, s["ligand_idx"])
    with pytest.raises(ValueError, match="pose atoms"):
        PocketAccuracy.from_tables(np.zeros((4097, 3)), np.zeros(4097), np.ones(4097), [0], np.zeros(4097), np.zeros(4097))
    with pytest.raises(ValueError, match="x_pred has shape"):
        obj.score(torch.zeros(2, 79, 3))
    other = spec("nine", pocket_radius=6.5, inclusion_radius=9.0, thresholds=(0.25, 0.5, 1.0, 2.0))
    assert other.n_pairs < obj.n_pairs and other.thresholds[0] == 0.25 and other.inclusion_radius == 9.0


def test_describe_lists_the_worst_residue_first():
    obj = spec("nine")
    o = cases.reference("nine")["out"]
    lines = obj.describe(o, 2)                                                 # PHE was exchanged in the pose and found
    assert len(lines) == 9 and sum("swapped" in ln for ln in lines) == 1 and "residue 5" in next(ln for ln in lines if "swapped" in ln)
    lines = obj.describe(o, 10)
    worst = int(np.argmax(o["residue_rmsd"][10]))
    assert lines[0].startswith(f"residue {worst}:") and f"rmsd {o['residue_rmsd'][10][worst]:.2f}" in lines[0]
    o1 = cases.reference("one")["out"]
    assert "rmsd nan" in spec("one").describe(o1, 2)[0]                        # not fitted: ordered by the lDDT


def test_from_batch_names_atoms_as_receptor_geometry_does():
    from physdock_amd import PocketAccuracy
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.interactions import residue_labels_from_meta
    from physdock_amd.scoring import names_from_meta
    from physdock_amd.synthetic import make_batch, pdb_meta
    batch = make_batch(20, 4, 9, 4, seed=6)
    meta = pdb_meta({k: batch[k].numpy() for k in ("token_id_to_chunk_sizes", "asym_id", "is_ligand", "residue_index")})
    batch["a_mask"] = batch["a_mask"].clone()
    gone = 7
    batch["a_mask"][gone] = 0
    obj = PocketAccuracy.from_batch(batch, meta, pocket_radius=10.0)
    res, names, z, _ = names_from_meta(meta)
    rid = batch["atom_id_to_token_id"].numpy()
    lig = ligand_atom_mask(batch).numpy()
    exists = batch["a_mask"].numpy() > 0
    assert obj.n_pose_atoms == len(res) == batch["x_gt"].shape[0] and obj.n_pairs > 0 and (z == 1).any() and not lig[gone]
    heavy_receptor = exists & (z != 1) & ~lig
    assert heavy_receptor[obj.named].all(), "hydrogens, ligand and masked atoms are not named"
    assert set(rid[obj.patom].tolist()) == set(obj.pocket_residues.tolist())
    assert ((obj.patom_kind & 1 != 0) == np.asarray([names[a].upper() == "CA" for a in obj.patom])).all()
    labels = residue_labels_from_meta(meta, rid, int(batch["is_ligand"].shape[0]))
    assert list(obj.residue_labels) == [labels[r] for r in obj.pocket_residues]
    same = PocketAccuracy.from_names(res, names, rid, batch["x_gt"], np.nonzero(lig & exists)[0], mask=heavy_receptor, pocket_radius=10.0)
    assert all((getattr(obj, k) == getattr(same, k)).all() for k in ("patom", "pair_atom", "pair_dist", "atom_partner", "atom_slot"))
    moved = PocketAccuracy.from_batch(batch, meta, x_ref=batch["x_gt"] + 1.0, pocket_radius=10.0)
    assert (moved.patom == obj.patom).all() and np.abs(moved.patom_ref - obj.patom_ref - 1.0).max() < 1e-5


# ------------------------------------------------------------------ header, library, driver
def test_header_declares_the_symbols_and_the_abi_stays_11():
    import physdock_amd
    from physdock_amd import _lib, pocket_accuracy
    assert physdock_amd.PocketAccuracy is pocket_accuracy.PocketAccuracy
    assert physdock_amd.swap_table_from_names is pocket_accuracy.swap_table_from_names
    assert _lib.ABI_VERSION == 11 and {"pd_pocket_accuracy", "pd_pocket_accuracy_workspace_numel"} <= set(_lib.header_symbols())
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "physdock_hip.h")).read()
    assert int(re.search(r"#define\s+PD_POCKET_ACCURACY_MAX_ATOMS\s+(\d+)", hdr).group(1)) == pocket_accuracy.MAX_ATOMS == 4096
    assert int(re.search(r"#define\s+PD_POCKET_ACCURACY_MAX_RESIDUES\s+(\d+)", hdr).group(1)) == pocket_accuracy.MAX_RESIDUES == 1024
    assert int(re.search(r"#define\s+PD_POCKET_ACCURACY_TILE\s+(\d+)", hdr).group(1)) == pocket_accuracy.PAIR_TILE
    src = open(_lib.os.path.join(_lib._HERE, "csrc", "pocket_accuracy.hip")).read()
    assert not re.search(r"atomic\w*\s*\(", src) and'#include "geom3.h"' in src and "horn_lambda_max<true>" in src and "block_sum_d(" in src
    bestfit = open(_lib.os.path.join(_lib._HERE, "csrc", "bestfit_rmsd.hip")).read()
    assert "horn_lambda_max<" in bestfit and "inline double horn_lambda_max" not in bestfit + src, "one copy, in geom3.h"
    for text in (pocket_accuracy.__doc__, hdr[hdr.index("pocket_accuracy.hip"):]):
        assert re.search(r"own\s+definition", text, flags=re.I) and "OpenStructure" in text


def test_the_built_library_exports_and_binds_the_symbols():
    from physdock_amd import _lib
    L = _lib.lib()
    assert L.pd_abi_version() == 11 and hasattr(L, "pd_pocket_accuracy") and len(_lib.SYMBOLS["pd_pocket_accuracy"].argtypes) == 35
    numel = L.pd_pocket_accuracy_workspace_numel
    assert numel(3, 9) == 108 and numel(65535, 1024) == 65535 * 4096 and numel(0, 9) == numel(3, 0) == -1
    assert numel(65536, 9) == numel(3, 1025) == -3


def test_redock_refuses_a_wrong_spec_before_sampling():
    from physdock_amd import driver
    obj = spec("nine")

    class Never:
        def sample_diffusion(self, *a, **k):
            raise AssertionError("sampled")

    batch = {"x_gt": torch.zeros(79, 3), "is_ligand": torch.zeros(3), "atom_id_to_token_id": torch.zeros(79, dtype=torch.long)}
    with pytest.raises(ValueError, match="built over 80 pose atoms, the batch holds 79"):
        driver.redock(Never(), batch, pocket_accuracy=obj)
    with pytest.raises(ValueError, match="takes a pocket_accuracy.PocketAccuracy"):
        driver.redock(Never(), batch, pocket_accuracy=object())
    with pytest.raises(ValueError, match="needs the ground truth"):
        driver.check_pocket_accuracy(obj, {"is_ligand": torch.zeros(3)})
    driver.check_pocket_accuracy(None, {})
    import inspect
    assert "pocket_accuracy" in inspect.signature(driver.redock).parameters
    assert inspect.signature(driver.redock).parameters["pocket_accuracy"].default is None
