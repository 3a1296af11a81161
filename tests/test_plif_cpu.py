"""The interaction fingerprint without a GPU: the charge typing of physdock_amd/interactions.py on small molecules and residues, the
float64 restatement (tests/plif_ref.py) on hand-placed pairs, the host tables (CSR), the integer edge cases of compare and pairwise,
the argument checks, describe, the header - and the condition the GPU tests rest on: in every seeded case of tests/plif_ref.py the
fingerprints with the thresholds lowered and raised by MARGIN are the same in every byte (one `OPEN | ...` line per case, pytest -s)."""
import re

import numpy as np
import pytest
import torch

import plif_ref as ref

RING = [(i, (i + 1) % 6) for i in range(6)]


def names(q):
    return ["+" if v == 1 else "-" if v == 2 else "" if v == 0 else "?" for v in q]


# ------------------------------------------------------------------ typing
def test_charged_ligand_groups():
    from physdock_amd.interactions import ligand_charges_from_bonds as charges
    # acetate CH3-C(=O)-O: both oxygens, with and without bond orders
    assert names(charges([6, 6, 8, 8], [(0, 1), (1, 2), (1, 3)], [1, 2, 1])) == ["", "", "-", "-"]
    assert names(charges([6, 6, 8, 8], [(0, 1), (1, 2), (1, 3)])) == ["", "", "-", "-"]
    # methyl phosphate CH3-O-P(=O)(O)O: the three terminal oxygens, not the ester oxygen
    assert names(charges([6, 8, 15, 8, 8, 8], [(0, 1), (1, 2), (2, 3), (2, 4), (2, 5)], [1, 1, 2, 1, 1])) == ["", "", "", "-", "-", "-"]
    # methanesulfonate CH3-S(=O)(=O)-O and methylphosphonate CH3-P(=O)(O)O
    assert names(charges([6, 16, 8, 8, 8], [(0, 1), (1, 2), (1, 3), (1, 4)], [1, 2, 2, 1])) == ["", "", "-", "-", "-"]
    assert names(charges([6, 15, 8, 8, 8], [(0, 1), (1, 2), (1, 3), (1, 4)], [1, 2, 1, 1])) == ["", "", "-", "-", "-"]
    # methylamine, trimethylamine
    assert names(charges([6, 7], [(0, 1)])) == ["", "+"]
    assert names(charges([7, 6, 6, 6], [(0, 1), (0, 2), (0, 3)], [1, 1, 1])) == ["+", "", "", ""]
    # guanidine N=C(N)N
    assert names(charges([7, 6, 7, 7], [(0, 1), (1, 2), (1, 3)], [2, 1, 1])) == ["+", "", "+", "+"]
    # benzamidine: ring 0 - 5, C6 on atom 0, =N7, -N8
    assert names(charges([6] * 7 + [7, 7], RING + [(0, 6), (6, 7), (6, 8)], [1.5] * 6 + [1, 2, 1])) == [""] * 7 + ["+", "+"]


def test_neutral_ligand_groups():
    from physdock_amd.interactions import ligand_charges_from_bonds as charges
    # acetamide CH3-C(=O)-N
    assert names(charges([6, 6, 8, 7], [(0, 1), (1, 2), (1, 3)], [1, 2, 1])) == [""] * 4
    # aniline
    assert names(charges([6] * 6 + [7], RING + [(0, 6)], [1.5] * 6 + [1])) == [""] * 7
    # methanesulfonamide CH3-S(=O)(=O)-N: two oxygens only, and the nitrogen has a hetero-atom neighbour
    assert names(charges([6, 16, 8, 8, 7], [(0, 1), (1, 2), (1, 3), (1, 4)], [1, 2, 2, 1])) == [""] * 5
    # methyl acetate (an ester), ethanol, pyridine, acetonitrile, dimethyl sulfone
    assert names(charges([6, 6, 8, 8, 6], [(0, 1), (1, 2), (1, 3), (3, 4)], [1, 2, 1, 1])) == [""] * 5
    assert names(charges([6, 6, 8], [(0, 1), (1, 2)])) == [""] * 3
    assert names(charges([7, 6, 6, 6, 6, 6], RING, [1.5] * 6)) == [""] * 6
    assert names(charges([6, 6, 7], [(0, 1), (1, 2)], [1, 3])) == [""] * 3
    assert names(charges([6, 16, 8, 8, 6], [(0, 1), (1, 2), (1, 3), (1, 4)], [1, 2, 2, 1])) == [""] * 5


def test_formal_charges_override_the_rules():
    from physdock_amd.interactions import ligand_charges_from_bonds as charges
    acetate = ([6, 6, 8, 8], [(0, 1), (1, 2), (1, 3)], [1, 2, 1])
    assert names(charges(*acetate, formal_charges=[0, 0, 0, -1])) == ["", "", "", "-"]
    assert names(charges(*acetate, formal_charges=[0, 0, 0, 0])) == [""] * 4            # given and neutral: neutral
    assert names(charges([6, 6, 8, 7], [(0, 1), (1, 2), (1, 3)], [1, 2, 1], formal_charges=[0, 0, -1, 2])) == ["", "", "-", "+"]
    assert names(charges([6, 7], [(0, 1)], formal_charges=torch.tensor([0, 0]))) == ["", ""]
    with pytest.raises(ValueError, match="formal charges"):
        charges([6, 7], [(0, 1)], formal_charges=[0])
    with pytest.raises(ValueError, match="bond"):
        charges([6, 7], [(0, 2)])


def test_receptor_charges_by_names():
    from physdock_amd.interactions import ANION, CATION, receptor_charges_from_names as charges
    assert (CATION, ANION) == (ref.CATION, ref.ANION) == (1, 2)
    table = {"LYS": (["N", "CA", "CE", "NZ"], ["", "", "", "+"]), "ARG": (["NE", "CZ", "NH1", "NH2", "N"], ["+", "", "+", "+", ""]),
             "ASP": (["CG", "OD1", "OD2", "O"], ["", "-", "-", ""]), "GLU": (["CD", "OE1", "OE2", "OXT"], ["", "-", "-", ""]),
             "HIS": (["ND1", "NE2", "CE1"], ["", "", ""]), "ASN": (["OD1", "ND2"], ["", ""]), "XYZ": (["NZ", "OD1"], ["", ""])}
    for res, (atoms, want) in table.items():
        assert names(charges([res] * len(atoms), atoms)) == want, res
    assert names(charges([" lys "], [" nz"])) == ["+"]
    with pytest.raises(ValueError):
        charges(["LYS"], ["NZ", "CE"])


# ------------------------------------------------------------------ the restatement on hand-placed pairs
def pair(r, lig, rec, thresholds=ref.THRESHOLDS, active=1):
    """one ligand atom (type, charge) at the origin and one receptor atom (type, charge) at distance r: the residue's byte"""
    x = np.zeros((1, 2, 3))
    x[0, 1, 1] = r
    c = dict(x=x, lig_idx=[0], types=[lig[0], rec[0]], charges=[lig[1], rec[1]], lig_active=[active], rec_mask=[0, 1], residue_of=[0, 0],
             n_residues=1, thresholds=thresholds)
    return ref.fingerprint(c)


KIND_PAIRS = [  # kind, ligand (type, charge), receptor (type, charge), threshold
    ("contact", (0, 0), (0, 0), 4.0),
    ("hydrophobic", (ref.HYDROPHOBIC, 0), (ref.HYDROPHOBIC, 0), 4.5),
    ("hbond_donor", (ref.DONOR, 0), (ref.ACCEPTOR, 0), 3.5),
    ("hbond_acceptor", (ref.ACCEPTOR, 0), (ref.DONOR, 0), 3.5),
    ("cationic", (0, ref.CATION), (0, ref.ANION), 4.5),
    ("anionic", (0, ref.ANION), (0, ref.CATION), 4.5),
]


@pytest.mark.parametrize("kind,lig,rec,thr", KIND_PAIRS)
def test_each_kind_sets_below_and_clears_above_its_threshold(kind, lig, rec, thr):
    k = ref.KIND_NAMES.index(kind)
    near, far = pair(thr - 0.1, lig, rec), pair(thr + 0.1, lig, rec)
    assert near["bits"][0, 0] >> k & 1 and not far["bits"][0, 0] >> k & 1
    assert near["ligand_bits"][0, 0] == near["bits"][0, 0] and near["counts"][0, k] == 1 and far["counts"][0, k] == 0
    assert near["min_dist"][0, 0] == pytest.approx(thr - 0.1, abs=1e-12)
    # the kinds the types do not allow stay clear however close the atoms are
    others = {j for j in range(6) if j != k and j != 0}
    assert not any(pair(1.0, lig, rec)["bits"][0, 0] >> j & 1 for j in others)
    # the roles do not swap: the same two atoms the other way round show the mirrored kind, not this one
    if kind in ("hbond_donor", "cationic"):
        assert pair(1.0, rec, lig)["bits"][0, 0] == 1 | 1 << (k + 1)
    # an inactive ligand atom shows nothing and leaves the residue without a distance
    off = pair(1.0, lig, rec, active=0)
    assert off["bits"][0, 0] == 0 and off["ligand_bits"][0, 0] == 0 and np.isinf(off["min_dist"][0, 0])


def test_a_donor_and_an_acceptor_at_3_4_and_3_6():
    d, a = (ref.DONOR, 0), (ref.ACCEPTOR, 0)
    assert pair(3.4, d, a)["bits"][0, 0] == 1 | 4 and pair(3.6, d, a)["bits"][0, 0] == 1
    assert pair(3.4, a, d)["bits"][0, 0] == 1 | 8 and pair(3.6, a, d)["bits"][0, 0] == 1
    assert pair(3.6, d, a, thresholds=(4.0, 4.5, 3.7, 4.5))["bits"][0, 0] == 1 | 4          # the threshold is an argument
    assert pair(3.9, d, a, thresholds=(3.8, 4.5, 3.5, 4.5))["bits"][0, 0] == 0


def test_constants_agree_with_the_package():
    from physdock_amd import interactions as I, scoring
    assert I.KIND_NAMES == ref.KIND_NAMES and tuple(I.DEFAULT_THRESHOLDS[k] for k in I.THRESHOLD_NAMES) == ref.THRESHOLDS
    assert (scoring.HYDROPHOBIC, scoring.DONOR, scoring.ACCEPTOR) == (ref.HYDROPHOBIC, ref.DONOR, ref.ACCEPTOR)
    assert (I.MAX_ATOMS, I.MAX_POSE_ATOMS, I.MAX_POSES) == (1024, 1 << 22, 65535)
    assert I.kind_mask() == 63 and I.kind_mask(("hbond_donor", "anionic")) == 4 | 32 and I.kind_mask("contact") == 1
    with pytest.raises(ValueError, match="unknown interaction kind"):
        I.kind_mask(("hbond",))
    with pytest.raises(ValueError, match="at least one"):
        I.kind_mask(())


# ------------------------------------------------------------------ the condition on the seeds
@pytest.mark.parametrize("name", list(ref.CASES))
def test_no_seeded_case_leaves_a_bit_open(name):
    c = ref.make_case(name)
    r = ref.restate(c)
    print(f"OPEN | {name} | bytes {r['n_bytes']} | open {r['open_bytes']} | counts of pose 0 {r['lo']['counts'][0].tolist()} |")
    assert r["open_bytes"] == 0, "a committed seed puts a pair within MARGIN of a threshold"
    for k in ("bits", "ligand_bits", "counts"):
        assert np.array_equal(r["lo"][k], r["hi"][k]) and np.array_equal(r["lo"][k], ref.fingerprint(c)[k])
    assert not (r["lo"]["bits"] >> 6).any() and not (r["lo"]["ligand_bits"] >> 6).any()
    assert np.array_equal(r["lo"]["counts"], ref.popcounts(r["lo"]["bits"]))
    assert (r["bound"][np.isfinite(r["min_dist"])] > 0).all() and r["bound"].max() < 1e-5


def test_case_a_is_the_shape_that_takes_every_path():
    n, A, lig, inactive, R, _, _ = ref.CASES["a_P3_A300_L5_R40"]
    assert (n, A, len(lig), R) == (3, 300, 5, 40) and A - 1 in lig and 256 in lig and inactive is not None
    c = ref.make_case("a_P3_A300_L5_R40")
    res = c["residue_of"]
    assert len({int(res[a]) for a in range(252, 260)} & {int(res[255])}) == 1 and res[255] == res[256]      # a run across atom 256
    start, atom = ref.csr(c)
    runs = [atom[start[s]:start[s + 1]] for s in range(R)]
    assert any(len(r) > 1 and np.diff(r).max() > 8 for r in runs), "interleaved ids: a residue's atoms are not one block"
    assert sum(len(r) == 0 for r in runs) >= 2, "an id without atoms, and a residue whose atoms are all masked"
    assert len(atom) > 256, "the receptor list crosses a block of plif_atom_kernel"
    bits = ref.fingerprint(c)["bits"]
    for k in range(6):
        assert (bits >> k & 1).any() and not (bits >> k & 1).all(), ref.KIND_NAMES[k]
    assert set((c["types"] >> 4).tolist()) == set(range(8)) and set(c["charges"][c["rec_mask"] > 0].tolist()) == {0, 1, 2}
    assert [ref.CASES[k][:2] for k in ref.CASES][1:] == [(2, 65), (2, 257), (66, 65)] and 66 % ref.PAIR_TILE not in (0, 1)


# ------------------------------------------------------------------ host tables
def fp_of(c, **kw):
    from physdock_amd.interactions import InteractionFingerprint
    return InteractionFingerprint.from_types(c["types"], c["charges"], c["lig_idx"], c["rec_mask"], c["residue_of"], n_residues=c["n_residues"],
                                             ligand_active=c["lig_active"], thresholds=c["thresholds"], **kw)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_the_csr_of_the_seeded_cases(name):
    c = ref.make_case(name)
    f = fp_of(c)
    start, atom = ref.csr(c)
    assert np.array_equal(f.res_start, start) and np.array_equal(f.res_atom, atom) and f.res_start.dtype == f.res_atom.dtype == np.int32
    assert f.n_receptor_atoms == int(c["rec_mask"].sum()) == start[-1] and f.n_residues == c["n_residues"]
    assert sorted(atom.tolist()) == np.nonzero(c["rec_mask"])[0].tolist()
    for s in range(f.n_residues):
        run = atom[start[s]:start[s + 1]]
        assert (c["residue_of"][run] == s).all() and (np.diff(run) > 0).all()


def test_csr_with_interleaved_single_masked_and_empty_residues():
    from physdock_amd.interactions import InteractionFingerprint, residue_csr
    #           atom  0  1  2  3  4  5  6  7  8  9
    residue_of = [2, 0, 2, 4, 0, 3, 3, 2, 1, 1]          # residue 4: one atom; residue 3: both atoms masked; residue 1: the ligand
    f = InteractionFingerprint.from_types(np.zeros(10, np.uint8), np.zeros(10, np.uint8), [8, 9], [1, 1, 1, 1, 1, 0, 0, 1, 1, 1], residue_of,
                                          n_residues=6)
    assert f.res_start.tolist() == [0, 2, 2, 5, 5, 6, 6] and f.res_atom.tolist() == [1, 4, 0, 2, 7, 3]
    assert f.rec_mask.tolist() == [1, 1, 1, 1, 1, 0, 0, 1, 0, 0] and f.n_receptor_atoms == 6 and f.n_residues == 6
    start, atom = residue_csr(residue_of, f.rec_mask, 6)
    assert np.array_equal(start, f.res_start) and np.array_equal(atom, f.res_atom)
    with pytest.raises(ValueError, match="residue_of must lie"):
        residue_csr(residue_of, f.rec_mask, 4)
    # a masked atom (a_mask) leaves the receptor; a ligand atom that does not exist is inactive
    g = InteractionFingerprint.from_types(np.zeros(10, np.uint8), np.zeros(10, np.uint8), [8, 9], np.ones(10), residue_of,
                                          a_mask=[1, 0, 1, 1, 1, 1, 1, 1, 1, 0])
    assert g.res_atom.tolist() == [4, 0, 2, 7, 5, 6, 3] and g.lig_active.tolist() == [1, 0] and g.n_residues == 5
    # no receptor atom at all is a valid system
    h = InteractionFingerprint.from_types(np.zeros(3, np.uint8), np.zeros(3, np.uint8), [0, 1, 2], np.ones(3), [0, 0, 0])
    assert h.n_receptor_atoms == 0 and h.res_start.tolist() == [0, 0]


def test_from_batch_takes_tokens_as_residues_and_names_from_the_meta_data():
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.interactions import InteractionFingerprint, receptor_charges_from_names
    from physdock_amd.scoring import VinaScore, names_from_meta
    from physdock_amd.synthetic import make_batch, pdb_meta
    batch = make_batch(20, 4, 9, 4, seed=6)
    is_lig = ligand_atom_mask(batch).numpy()
    n_lig, T = int(is_lig.sum()), int(batch["is_ligand"].shape[0])
    bonds = [(i, i + 1) for i in range(n_lig - 1)]
    f = InteractionFingerprint.from_batch(batch, bonds)
    v = VinaScore.from_batch(batch, bonds)
    assert f.receptor_typing == "elements" and f.n_residues == T and f.residue_labels is None
    assert np.array_equal(f.rec_mask, v.rec_mask) and np.array_equal(f.ligand_idx, v.ligand_idx) and np.array_equal(f.lig_active, v.lig_active)
    assert np.array_equal(f.types, v.types) and not f.charges[~is_lig].any() and not (f.types[~is_lig] & 96).any()
    assert np.array_equal(f.residue_of, batch["atom_id_to_token_id"].numpy())
    lig_tokens = np.nonzero(batch["is_ligand"].numpy() > 0)[0]
    assert (np.diff(f.res_start)[lig_tokens] == 0).all(), "the ligand's tokens own no receptor atom"
    assert int(np.diff(f.res_start).sum()) == f.n_receptor_atoms == int(f.rec_mask.sum())
    meta = pdb_meta({k: batch[k].numpy() for k in ("token_id_to_chunk_sizes", "asym_id", "is_ligand", "residue_index")})
    named = InteractionFingerprint.from_batch(batch, bonds, infer_meta_data=meta, thresholds={"hbond": 3.2})
    res, atom_names, _, _ = names_from_meta(meta)
    assert named.receptor_typing == "names" and named.thresholds == {"contact": 4.0, "hydrophobic": 4.5, "hbond": 3.2, "ionic": 4.5}
    assert np.array_equal(named.charges[~is_lig], receptor_charges_from_names(res, atom_names)[~is_lig])
    assert np.array_equal(named.types, VinaScore.from_batch(batch, bonds, infer_meta_data=meta).types)
    assert len(named.residue_labels) == T and named.residue_labels[0] == f"{res[0]}{int(meta['residue_index'][0])}"
    first_lig = int(np.nonzero(is_lig)[0][0])
    assert named.residue_labels[int(f.residue_of[first_lig])] == f"{res[first_lig]}:{atom_names[first_lig]}"
    given = InteractionFingerprint.from_batch(batch, bonds, receptor_types=named.types, receptor_charges=named.charges)
    assert given.receptor_typing == "given" and np.array_equal(given.charges[~is_lig], named.charges[~is_lig])


def test_from_bonds_types_and_charges_the_ligand():
    from physdock_amd.interactions import InteractionFingerprint
    # pose: an ASP side chain (CG OD1 OD2), a hydrogen, then ethylamine C-C-N at 6, 4, 5
    elements = [6, 8, 8, 1, 6, 7, 6]
    f = InteractionFingerprint.from_bonds(elements, [(0, 1), (1, 2)], [6, 4, 5], [0, 0, 0, 0, 1, 1, 1])
    assert f.receptor_typing == "elements" and f.rec_mask.tolist() == [1, 1, 1, 0, 0, 0, 0] and f.charges.tolist() == [0, 0, 0, 0, 0, 1, 0]
    assert f.types[5] & ref.DONOR and not (f.types[:3] & 96).any() and f.n_residues == 2
    g = InteractionFingerprint.from_bonds(elements, [(0, 1), (1, 2)], [6, 4, 5], [0, 0, 0, 0, 1, 1, 1], receptor_types=[0, 2 | 64, 2 | 64, 0, 0, 0, 0],
                                          receptor_charges=[0, 2, 2, 0, 0, 0, 0], formal_charges=[0, 0, 0], residue_labels=["ASP25", "LIG"])
    assert g.receptor_typing == "given" and g.charges.tolist() == [0, 2, 2, 0, 0, 0, 0] and g.residue_labels == ["ASP25", "LIG"]
    with pytest.raises(ValueError, match="without receptor_types"):
        InteractionFingerprint.from_bonds(elements, [], [6, 4, 5], [0] * 7, receptor_charges=[0] * 7)


# ------------------------------------------------------------------ integer edge cases of compare and pairwise
def test_compare_edge_cases():
    bits = np.array([[0, 0, 0], [1, 5, 0], [63, 63, 63], [1, 4, 32]], dtype=np.uint8)
    empty = ref.compare(bits, np.zeros(3, np.uint8))
    assert empty["n_reference"] == 0 and empty["shared"].tolist() == [0] * 4 and empty["recovery"].tolist() == [1.0] * 4
    assert empty["tanimoto"].tolist() == [1.0, 0.0, 0.0, 0.0], "an empty union counts as agreement"
    full = ref.compare(bits, np.array([1, 5, 0], np.uint8))
    assert full["n_reference"] == 3 and full["shared"].tolist() == [0, 3, 3, 2] and full["n_pose"].tolist() == [0, 3, 18, 3]
    assert full["recovery"].tolist() == [0.0, 1.0, 1.0, np.float32(2) / np.float32(3)]
    assert full["tanimoto"].tolist() == [0.0, 1.0, np.float32(3) / np.float32(18), np.float32(2) / np.float32(4)]
    assert full["recovery"].dtype == full["tanimoto"].dtype == np.float32
    # a kind mask leaves the other kinds out on both sides
    hb = ref.compare(bits, np.array([1, 5, 0], np.uint8), mask=4 | 8)
    assert hb["n_reference"] == 1 and hb["shared"].tolist() == [0, 1, 1, 1] and hb["n_pose"].tolist() == [0, 1, 6, 1]
    none = ref.compare(bits, np.array([1, 5, 0], np.uint8), mask=16)
    assert none["n_reference"] == 0 and none["recovery"].tolist() == [1.0] * 4 and none["tanimoto"].tolist() == [1.0, 1.0, 0.0, 1.0]


def test_pairwise_edge_cases():
    bits = np.array([[0, 0, 0], [1, 5, 0], [63, 63, 63], [1, 4, 32], [0, 0, 0]], dtype=np.uint8)
    t = ref.pairwise(bits)
    assert t.dtype == np.float32 and np.array_equal(t, t.T) and (np.diag(t) == 1.0).all()
    assert t[0, 4] == 1.0 and t[0, 1] == 0.0 and t[1, 2] == np.float32(3) / np.float32(18) and t[1, 3] == np.float32(2) / np.float32(4)
    for p in range(5):
        assert np.array_equal(ref.compare(bits, bits[p])["tanimoto"], t[p])
    m = ref.pairwise(bits, mask=1)
    assert m[1, 3] == 0.5 and m[1, 2] == np.float32(2) / np.float32(3) and m[0, 1] == 0.0


# ------------------------------------------------------------------ arguments, describe, header
def test_constructor_argument_errors():
    from physdock_amd.interactions import InteractionFingerprint as F
    z8 = np.zeros(8, np.uint8)
    ok = dict(types=z8, charges=z8, ligand_idx=[1], receptor_mask=np.ones(8), residue_of=[0, 0, 1, 1, 2, 2, 3, 3])
    F.from_types(**ok)
    for change, match in ((dict(ligand_idx=[1, 1]), "distinct"), (dict(ligand_idx=[8]), "distinct"), (dict(types=np.full(8, 200)), "bits 0 - 6"),
                          (dict(charges=np.full(8, 4)), "CATION, ANION"), (dict(charges=np.zeros(7)), "CATION, ANION"),
                          (dict(receptor_mask=np.ones(9)), "receptor_mask"), (dict(residue_of=[0] * 7), "residue_of"),
                          (dict(residue_of=[0, 0, 1, 1, 2, 2, 3, -1]), "residue_of must lie"), (dict(n_residues=3), "residue_of must lie"),
                          (dict(n_residues=9), "at most one residue per atom"), (dict(ligand_active=[1, 1]), "ligand_active"),
                          (dict(thresholds={"hbond": -1.0}), "finite and not negative"), (dict(thresholds={"hbond": float("nan")}), "finite"),
                          (dict(thresholds={"contact": float("inf")}), "finite"), (dict(thresholds={"pi": 4.0}), "unknown thresholds"),
                          (dict(thresholds=(4.0, 4.5, 3.5)), "got 3 values"), (dict(residue_labels=["A", "B"]), "residue labels")):
        with pytest.raises(ValueError, match=match):
            F.from_types(**{**ok, **change})
    with pytest.raises(ValueError, match="ligand atoms"):
        F.from_types(np.zeros(2000, np.uint8), np.zeros(2000, np.uint8), np.arange(1025), np.ones(2000), np.zeros(2000))
    f = F.from_types(**ok, thresholds=(3.0, 4.0, 3.0, 4.0))
    assert f.thresholds == {"contact": 3.0, "hydrophobic": 4.0, "hbond": 3.0, "ionic": 4.0} and list(f._thr) == [3.0, 4.0, 3.0, 4.0]
    assert "InteractionFingerprint(n_atoms=1, n_pose_atoms=8, residues=4, receptor_atoms=7" in repr(f)
    with pytest.raises(ValueError, match="pose atoms"):
        f.fingerprint(torch.zeros(2, 7, 3))
    with pytest.raises(ValueError, match="uint8 tensor"):
        f.compare(torch.zeros(2, 4), torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8 tensor"):
        f.pairwise(torch.zeros(2, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="unknown interaction kind"):
        f.compare(torch.zeros(2, 4, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8), kinds=("stacking",))
    with pytest.raises(ValueError, match="reference row holds"):
        f.compare(torch.zeros(2, 4, dtype=torch.uint8), torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="coordinates"):
        f.compare(torch.zeros(2, 4, dtype=torch.uint8), torch.zeros(7, 3))
    with pytest.raises(ValueError, match="not in 0"):
        f.required_row([(4, "contact")])
    with pytest.raises(ValueError, match="labelled"):
        f.required_row([("ASP25", "contact")])


def test_describe_and_the_required_row():
    from physdock_amd.interactions import InteractionFingerprint as F
    z8 = np.zeros(8, np.uint8)
    plain = F.from_types(z8, z8, [1], np.ones(8), [0, 0, 1, 1, 2, 2, 3, 3])
    assert plain.describe(np.array([0, 5, 0, 63], np.uint8)) == [(1, ["contact", "hbond_donor"]), (3, list(ref.KIND_NAMES))]
    assert plain.describe(torch.zeros(4, dtype=torch.uint8)) == []
    named = F.from_types(z8, z8, [1], np.ones(8), [0, 0, 1, 1, 2, 2, 3, 3], residue_labels=["LIG:C1", "ASP25", "", "LYS83"])
    assert named.describe(torch.tensor([0, 17, 2, 32], dtype=torch.uint8)) == [("ASP25", ["contact", "cationic"]), (2, ["hydrophobic"]),
                                                                              ("LYS83", ["anionic"])]
    assert named.required_row([("ASP25", "cationic"), (1, "contact"), (3, "hbond_acceptor")]).tolist() == [0, 17, 0, 8]
    assert named.required_row([]).tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="a row holds"):
        named.describe(np.zeros(5, np.uint8))


def test_header_declares_the_launchers_and_the_abi_stays_11():
    import physdock_amd
    from physdock_amd import _lib, interactions
    assert physdock_amd.InteractionFingerprint is interactions.InteractionFingerprint
    assert _lib.ABI_VERSION == 11
    assert {"pd_plif_fingerprint", "pd_plif_compare", "pd_plif_pairwise"} <= set(_lib.header_symbols())
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "physdock_hip.h")).read()
    assert int(re.search(r"#define\s+PD_PLIF_KINDS\s+(\d+)", hdr).group(1)) == len(interactions.KIND_NAMES) == 6
    assert int(re.search(r"#define\s+PD_PLIF_THRESHOLDS\s+(\d+)", hdr).group(1)) == len(interactions.THRESHOLD_NAMES) == 4
    src = open(_lib.os.path.join(_lib._HERE, "csrc", "plif.hip")).read()
    assert "sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)))" in src and "atomic" not in src.split("#include")[1]
    assert int(re.search(r"PAIR_TILE = (\d+)", src).group(1)) == ref.PAIR_TILE


def test_the_built_library_exports_and_binds_the_launchers():
    from physdock_amd import _lib
    L = _lib.lib()
    assert L.pd_abi_version() == 11
    want = {"pd_plif_fingerprint": 20, "pd_plif_compare": 11, "pd_plif_pairwise": 6}
    assert all(hasattr(L, k) and len(_lib.SYMBOLS[k].argtypes) == n for k, n in want.items())
