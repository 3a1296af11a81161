"""The torsion fingerprint and TFD without a GPU: the definition tests/torsion_ref.py against closed forms, the host side of
physdock_amd/torsions.py (perception, tables, refusals) against it, and the conditioning of every kernel case of
tests/test_torsion_gpu.py.  The tests named `test_ref_*` exercise only the reference, the test inputs and code the package had before
(`symmetry.LigandSymmetry`): they pass without the package's new module.  Every other test needs physdock_amd.torsions or the new exports."""
import inspect
import os

import numpy as np
import pytest
import torch

import torsion_cases as tc
import torsion_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: closed forms hold up to the rounding of the coordinates to fp32 60 - 100 A from the origin: 7.6e-6 A on each of four atoms over a
#: lever of about 1.3 A is 2e-5 rad = 1.3e-3 degrees per angle, 1.5e-5 of max_dev = 180 for two structures, 7e-5 of a six-ring's 36.3
TOL, TOL_RING = 5e-5, 5e-4
MOLECULES = {"butane": tc.butane(180.0), "biphenyl": tc.biphenyl(40.0), "tbutyl": tc.tbutyl(20.0), "cyclohexane": tc.cyclohexane(),
             "amide": tc.amide_ligand(180.0), "chain9": (tc.chain(9), None),
             "norbornane": (dict(n=7, bonds=[(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 6), (6, 3)], orders=[1.0] * 8,
                                 elements=[6] * 7), None),
             "naphthalene": (dict(n=10, bonds=[(k, k + 1) for k in range(9)] + [(9, 0), (4, 9)], orders=[1.5] * 11, elements=[6] * 10),
                             None)}


def fingerprint(mol, uniform=False):
    ents = ref.entries(mol["n"], mol["bonds"], mol["orders"])
    return ents, (np.ones(len(ents)) if uniform else ref.weights(mol["n"], mol["bonds"], ents))


def value(mol, x, y, perms=None, seed=0, uniform=False):
    ents, w = fingerprint(mol, uniform)
    return ref.tfd(tc.moved(x, seed), tc.moved(y, seed + 1), ents, w, perms), ents


def group(mol):
    from physdock_amd.symmetry import LigandSymmetry
    return LigandSymmetry.from_bonds(mol["n"], mol["bonds"], mol["elements"], mol["orders"])


# ------------------------------------------------------------------ the reference against closed forms
def test_ref_butane_anti_against_gauche():
    mol, anti = tc.butane(180.0)
    r, ents = value(mol, anti, tc.butane(60.0)[1])
    assert len(ents) == 1 and ents[0]["quads"] == [(0, 1, 2, 3)] and ents[0]["max_dev"] == 180.0
    assert abs(abs(ref.dihedral(tc.butane(60.0)[1])) - 60.0) < 1e-9
    assert abs(r["tfd"] - 120.0 / 180.0) < TOL and r["E"] < 1e-7          # (the anti angle is planar: the acos form is good to sqrt(eps) there)


def test_ref_biphenyl_ring_flip():
    mol, x = tc.biphenyl(40.0)
    y = tc.biphenyl(220.0)[1]
    ents, _ = fingerprint(mol)
    assert [e["kind"] for e in ents] == [ref.ROT, ref.RING, ref.RING] and len(ents[0]["quads"]) == 4 and ents[0]["atoms"] == (0, 6)
    r, _ = value(mol, x, y)
    assert abs(r["dev"][0, 0] - 1.0) < TOL and max(r["dev"][0, 1:]) < TOL_RING
    flip = np.arange(14)
    flip[[7, 11, 8, 10]] = [11, 7, 10, 8]
    r, _ = value(mol, x, y, np.stack([np.arange(14), flip]))
    assert r["row"] == 1 and r["tfd"] < TOL and abs(r["per_m"][0] - value(mol, x, y)[0]["tfd"]) == 0.0


def test_ref_tbutyl_turned_by_120():
    mol, x = tc.tbutyl(20.0)
    y = tc.tbutyl(140.0)[1]
    r, ents = value(mol, x, y)
    assert len(ents) == 1 and len(ents[0]["quads"]) == 3 and abs(r["tfd"] - 120.0 / 180.0) < TOL
    turn = np.array([0, 2, 3, 1, 4, 5])
    rows = np.stack([np.arange(6), turn, turn[turn]])
    r, _ = value(mol, x, y, rows)
    assert r["tfd"] < TOL and r["row"] in (1, 2)


def test_ref_cyclohexane_chair_inversion():
    mol, chair = tc.cyclohexane(1.0)
    r, ents = value(mol, chair, tc.cyclohexane(-1.0)[1])
    assert len(ents) == 1 and ents[0]["kind"] == ref.RING and len(ents[0]["quads"]) == 6
    assert abs(ents[0]["max_dev"] - 180.0 * np.exp(-0.025 * 64)) < 1e-12
    assert r["tfd"] == 1.0
    same, _ = value(mol, chair, chair)
    assert same["tfd"] < TOL
    x = tc.moved(chair)
    assert ref.tfd(x, x, ents, [1.0])["tfd"] == 0.0


def test_ref_amide_flip_is_the_single_worst_entry():
    mol, trans = tc.amide_ligand(180.0)
    r, ents = value(mol, tc.amide_ligand(0.0)[1], trans)
    assert mol["n"] == 25
    amide = [t for t, e in enumerate(ents) if e["atoms"] == (11, 12)]
    assert len(amide) == 1 and len(ents[amide[0]]["quads"]) == 2
    dev = r["dev"][0]
    assert int(np.argmax(dev)) == amide[0] and abs(dev[amide[0]] - 1.0) < TOL
    assert np.delete(dev, amide[0]).max() < TOL_RING


def test_ref_weights_of_a_linear_chain():
    mol = tc.chain(9)
    ents, w = fingerprint(mol)
    assert [e["atoms"] for e in ents] == [(k, k + 1) for k in range(1, 7)]
    d, C = ref.entry_distances(9, mol["bonds"], ents)
    assert list(C) == [4] and list(d) == [2, 1, 0, 0, 1, 2]
    assert np.allclose(w, [1e-4, 0.1, 1.0, 1.0, 0.1, 1e-4], rtol=1e-12)          # beta = ln 10 / (2 / 2)^2
    ents7, w7 = fingerprint(tc.chain(7))
    assert np.allclose(w7, [1e-4, 1.0, 1.0, 1e-4], rtol=1e-12)                    # max d = 1: beta = ln 10 / (1 / 2)^2


def test_ref_rings_are_the_chordless_cycles():
    assert ref.rings(7, MOLECULES["norbornane"][0]["bonds"]) == [(0, 1, 2, 3, 4, 5), (0, 1, 2, 3, 6), (0, 5, 4, 3, 6)]
    assert [len(r) for r in ref.rings(10, MOLECULES["naphthalene"][0]["bonds"])] == [6, 6]
    assert ref.rings(3, [(0, 1), (1, 2), (2, 0)]) == [] and ref.rings(9, [(k, (k + 1) % 9) for k in range(9)]) == []
    assert abs(ref.ring_max_dev(4) - 180 * np.exp(-2.5)) < 1e-12


def test_ref_degenerate_input():
    mol, x = tc.butane(70.0)
    ents, w = fingerprint(mol)
    line = np.array([[0, 0, 0], [1.5, 0, 0], [3.0, 0, 0], [4.0, 1.0, 0]], dtype=np.float32) + 70
    assert np.isnan(ref.dihedral(line)) and np.isnan(ref.dihedral_acos(line))
    r = ref.tfd(tc.moved(x), line, ents, w)
    assert np.isnan(r["tfd"]) and r["row"] == -1
    bad = tc.moved(x)
    bad[3, 1] = np.nan
    assert np.isnan(ref.tfd(bad, tc.moved(x), ents, w)["tfd"])
    # a NaN atom no quadruple names changes nothing; T = 0 gives 0 whatever the coordinates
    mol6, x6 = tc.tbutyl(20.0)
    ents6, w6 = fingerprint(mol6)
    D, _ = ref.pairwise(np.stack([tc.moved(x6), bad6 := np.where(np.arange(6)[:, None] == 1, np.nan, tc.moved(x6, 1)), tc.moved(x6, 2)]),
                        None, ents6, w6, None, 6)
    assert np.isnan(D[1]).all() and np.isnan(D[:, 1]).all() and np.isfinite(np.delete(np.delete(D, 1, 0), 1, 1)).all() and bad6.shape == (6, 3)
    assert ref.entries(2, [(0, 1)]) == [] and ref.tfd(np.full((2, 3), np.nan), np.zeros((2, 3)), [], [])["tfd"] == 0.0


def test_ref_the_case_list_covers_every_axis_value():
    """the kernel cases of tests/test_torsion_gpu.py reach every tile from both sides, both table kinds, both index forms and both limits of Q"""
    kws = [kw for _, kw, _, _ in tc.KERNEL_CASES]
    tiles = {(tj, kw["nb"]) for (_, kw, tj, _) in tc.KERNEL_CASES}
    assert {(64, 63), (64, 65), (16, 15), (16, 17), (4, 3), (4, 5), (1, 1), (1, 2)} <= tiles
    assert {1, 5} <= {kw["na"] for kw in kws} and {1, 3} <= {kw.get("M", 1) for kw in kws} and any(kw.get("M", 1) == 257 for kw in kws)
    assert {kw.get("scattered", False) for kw in kws} == {False, True} and any(kw.get("T") == 1 for kw in kws)
    assert {kw.get("Q") for kw in kws} >= {4079, 4096} and any(kw.get("nblocks") == 1 for kw in kws)
    assert {in_lds for *_, in_lds in tc.KERNEL_CASES} == {True, False}


@pytest.mark.parametrize("k", range(len(tc.KERNEL_CASES)))
def test_ref_is_well_conditioned_on_every_kernel_case(k):
    """the two float64 forms of every angle agree: E is a few ulp, so that B is set by its explicit term; the tile is the one the case
    was written for"""
    c = tc.kernel_case(k)
    E, B = ref.field(c["ref"], "E"), ref.field(c["ref"], "B")
    assert np.isfinite(E).all() and E.max() <= 1e-12, E.max()
    assert B.max() <= 1e-11
    assert tc.expected_tile(c["tables"]["quads"].shape[0], c["perms"].shape[0]) == (c["tile"], c["row_in_lds"])
    assert c["Lg"] <= 1024 and len(c["ents"]) <= 1024 and c["tables"]["quads"].shape[0] <= 4096


# ------------------------------------------------------------------ the host side of the package against the reference
@pytest.mark.parametrize("name", sorted(MOLECULES))
def test_perception_matches_the_reference(name):
    from physdock_amd.torsions import TorsionFingerprint
    mol = MOLECULES[name][0]
    spec = TorsionFingerprint.from_bonds(mol["n"], mol["bonds"], mol["orders"])
    ents, w = fingerprint(mol)
    assert spec.n_entries == len(ents) == len(spec.entries)
    for e, r, wt in zip(spec.entries, ents, w):
        assert (e.kind, e.atoms, list(e.quads), e.max_dev) == (r["kind"], tuple(r["atoms"]), r["quads"], r["max_dev"])
        assert abs(e.weight - wt) <= 1e-15
    t = tc.tables(ents, w, np.arange(mol["n"])[None])
    assert np.array_equal(spec.quads, t["quads"]) and np.array_equal(spec.image, t["image"]) and np.array_equal(spec.qstart, t["qstart"])
    uni = TorsionFingerprint.from_bonds(mol["n"], mol["bonds"], mol["orders"], weights="uniform")
    assert all(e.weight == 1.0 for e in uni.entries)


@pytest.mark.parametrize("name", ["biphenyl", "tbutyl", "cyclohexane", "norbornane", "naphthalene"])
def test_entries_and_weights_are_invariant_under_every_automorphism(name):
    from physdock_amd.torsions import TorsionFingerprint
    mol = MOLECULES[name][0]
    sym = group(mol)
    assert sym.complete and sym.n_perms > 1
    spec = TorsionFingerprint.from_bonds(mol["n"], mol["bonds"], mol["orders"], symmetry=sym)
    own = {(frozenset(tc.canonical(q) for q in e.quads), e.weight, e.max_dev, e.kind) for e in spec.entries}
    for p in sym.perms:
        assert {(frozenset(tc.canonical(p[list(q)]) for q in e.quads), e.weight, e.max_dev, e.kind) for e in spec.entries} == own
    base = {tc.canonical(q) for e in spec.entries for q in e.quads}
    assert {tuple(q) for q in spec.quads.tolist()} == base          # closing under a complete table adds nothing
    ents, w = fingerprint(mol)
    t = tc.tables(ents, w, sym.perms)
    assert np.array_equal(spec.quads, t["quads"]) and np.array_equal(spec.image, t["image"])
    assert spec.symmetry_complete


def test_ref_biphenyl_and_tbutyl_with_the_table_of_from_bonds():
    for (mol, x), y, n_rows in ((tc.biphenyl(40.0), tc.biphenyl(220.0)[1], 4), (tc.tbutyl(20.0), tc.tbutyl(140.0)[1], 6)):
        sym = group(mol)
        assert sym.n_perms == n_rows and sym.complete
        r, _ = value(mol, x, y, sym.perms)
        assert r["tfd"] < TOL and r["row"] > 0 and r["per_m"][0] > 0.1


def test_refusals_on_the_host():
    from physdock_amd.symmetry import LigandSymmetry
    from physdock_amd.torsions import TorsionFingerprint, check_redock_torsions
    mol = tc.butane(60.0)[0]
    ok = TorsionFingerprint.from_bonds(4, mol["bonds"])
    bad = [lambda: TorsionFingerprint.from_bonds(0, []), lambda: TorsionFingerprint.from_bonds(1025, []),
           lambda: TorsionFingerprint.from_bonds(4, [(0, 4)]), lambda: TorsionFingerprint.from_bonds(4, [(1, 1)]),
           lambda: TorsionFingerprint.from_bonds(4, mol["bonds"], weights="gaussian"),
           lambda: TorsionFingerprint.from_bonds(4, mol["bonds"], weights=[1.0, 2.0]),
           lambda: TorsionFingerprint.from_bonds(4, mol["bonds"], weights=[-1.0]),
           lambda: TorsionFingerprint.from_bonds(4, mol["bonds"], weights=[0.0]),
           lambda: TorsionFingerprint.from_bonds(4, mol["bonds"], ligand_idx=[0, 1, 2]),
           lambda: TorsionFingerprint.from_bonds(4, mol["bonds"], ligand_idx=[0, 1, 2, -3]),
           lambda: TorsionFingerprint.from_bonds(4, mol["bonds"], ligand_idx=[[0, 1], [2, 3]]),
           lambda: TorsionFingerprint.from_bonds(4, mol["bonds"], ligand_idx=[]),
           lambda: ok.pairwise(torch.zeros(2, 4, 3, device="meta")),
           lambda: TorsionFingerprint.from_bonds(4, mol["bonds"], ligand_idx=torch.tensor([0.0, 1, 2, 3])),
           lambda: TorsionFingerprint.from_bonds(4, mol["bonds"], symmetry=LigandSymmetry.from_permutations(np.arange(5)[None])),
           lambda: TorsionFingerprint.from_bonds(4, mol["bonds"], symmetry="c2"),
           lambda: TorsionFingerprint.from_tables(4, [("bond", (1, 2), [(0, 1, 2, 4)], 1.0, 180.0)]),
           lambda: TorsionFingerprint.from_tables(4, [("bond", (1, 2), [(0, 1, 2)], 1.0, 180.0)]),
           lambda: TorsionFingerprint.from_tables(4, [("bond", (1, 2), [], 1.0, 180.0)]),
           lambda: TorsionFingerprint.from_tables(4, [("angle", (1, 2), [(0, 1, 2, 3)], 1.0, 180.0)]),
           lambda: TorsionFingerprint.from_tables(4, [("bond", (1, 2), [(0, 1, 2, 3)], 1.0, 0.0)]),
           lambda: TorsionFingerprint.from_tables(4, [("bond", (1, 2), [(0, 1, 2, 3)], float("nan"), 180.0)]),
           lambda: TorsionFingerprint.from_tables(4, [("bond", (1, 2), [(0, 1, 2, 3)], 1.0, 180.0)] * 1025),
           # structures: shape, dtype, atom count, an index outside the pose, not on the GPU
           lambda: ok.pairwise(torch.zeros(4, 3)), lambda: ok.pairwise(torch.zeros(2, 4, 3, dtype=torch.int32)),
           lambda: ok.pairwise(torch.zeros(2, 5, 3)), lambda: ok.pairwise(torch.zeros(0, 4, 3)), lambda: ok.pairwise(torch.zeros(2, 4, 3)),
           lambda: TorsionFingerprint.from_bonds(4, mol["bonds"], ligand_idx=[0, 1, 2, 9]).angles(torch.zeros(2, 6, 3)),
           lambda: ok.to_reference(torch.zeros(2, 4, 3), torch.zeros(1, 4, 3)), lambda: ok.describe([0.0, 1.0]),
           lambda: check_redock_torsions("tfd", {}),
           ]
    for k, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"refusal {k} did not raise")
    # more than 4096 distinct quadruples after closing under the table
    rng = np.random.default_rng(5)
    many = [("bond", (1, 2), [tuple(q)], 1.0, 180.0) for q in {tuple(rng.permutation(40)[:4]) for _ in range(1000)}]
    table = LigandSymmetry.from_permutations(np.stack([np.arange(40)] + [rng.permutation(40) for _ in range(9)]))
    with pytest.raises(ValueError, match="4096"):
        TorsionFingerprint.from_tables(40, many, symmetry=table)
    with pytest.raises(AttributeError):
        ok.n_atoms = 5
    assert "bond" in ok.describe([0.5]) and ok.n_entries == 1 and ok.symmetry_complete
    assert TorsionFingerprint.from_bonds(2, [(0, 1)]).n_entries == 0


def test_from_sdf_and_from_batch():
    from physdock_amd.sdfio import parse_sdf
    from physdock_amd.torsions import TorsionFingerprint
    mol, x = tc.butane(60.0)
    atoms = "".join(f"{p[0]:10.4f}{p[1]:10.4f}{p[2]:10.4f} C   0  0  0  0  0  0  0  0  0  0  0  0\n" for p in x)
    text = "butane\n  test\n\n  4  3  0  0  0  0  0  0  0  0999 V2000\n" + atoms + "  1  2  1  0\n  2  3  1  0\n  3  4  1  0\nM  END\n$$$$\n"
    want = TorsionFingerprint.from_bonds(4, mol["bonds"]).entries
    assert TorsionFingerprint.from_sdf(parse_sdf(text)[0]).entries == want and TorsionFingerprint.from_sdf(text).entries == want
    assert len(want) == 1 and want[0].quads == ((0, 1, 2, 3),)
    assert callable(TorsionFingerprint.from_batch)


def test_abi_header_exports_and_keywords():
    import physdock_amd
    from physdock_amd import _lib, clustering, driver
    header = open(os.path.join(ROOT, "include", "physdock_hip.h")).read()
    assert "#define PD_ABI_VERSION 11" in header
    src = inspect.getsource(_lib)
    for name in ("pd_torsion_workspace_numel", "pd_torsion_prepare", "pd_torsion_tfd", "pd_torsion_deviation"):
        assert f"int {name}(" in header and f'sig("{name}"' in src
    assert os.path.exists(os.path.join(ROOT, "physdock_amd", "csrc", "torsion.hip"))
    assert physdock_amd.TorsionFingerprint is physdock_amd.torsions.TorsionFingerprint
    assert inspect.signature(driver.redock).parameters["torsions"].default is None
    assert inspect.signature(driver._RedockState.__init__).parameters["torsions"].default is None
    assert clustering.PoseClusters(cutoff=0.2, metric="torsion").metric == "torsion"
    with pytest.raises(ValueError, match="torsions="):
        clustering.check_redock_prerequisites(clustering.PoseClusters(metric="torsion"))
