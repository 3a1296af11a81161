"""RingInteractions without a GPU: ring, receptor-ring and halogen perception of physdock_amd/ring_interactions.py on small
molecules and residues, the float64 restatement (tests/plif_rings_ref.py) on hand-placed geometries, its invariance under rotating
and reversing a ring's list, the constructors' checks, the header - and the condition the GPU tests rest on: in every seeded case the
fingerprints with the thresholds moved against and with the margins are the same in every byte (one `OPEN | ...` line per case,
pytest -s)."""
import re

import numpy as np
import pytest
import torch

import plif_rings_ref as ref

BENZENE = [(i, (i + 1) % 6) for i in range(6)]
# naphthalene: two six-rings sharing the bond 4 - 5; indole: a six-ring 0 - 5 and the five-ring 4 5 6 7 8 (8 = N)
NAPHTHALENE = BENZENE + [(5, 6), (6, 7), (7, 8), (8, 9), (9, 4)]
INDOLE = BENZENE + [(5, 6), (6, 7), (7, 8), (8, 4)]


def bonded(ring, bonds):
    pairs = {frozenset(b) for b in bonds}
    return all(frozenset((ring[i], ring[(i + 1) % len(ring)])) in pairs for i in range(len(ring)))


# ------------------------------------------------------------------ perception
def test_aromatic_rings_in_canonical_cyclic_order():
    from physdock_amd.ring_interactions import aromatic_rings_from_bonds as rings
    assert rings(6, BENZENE, [1.5] * 6) == [(0, 1, 2, 3, 4, 5)]
    naph = rings(10, NAPHTHALENE, [1.5] * 11)
    assert len(naph) == 2 and sorted(map(sorted, naph)) == [[0, 1, 2, 3, 4, 5], [4, 5, 6, 7, 8, 9]]
    indole = rings(9, INDOLE, [1.5] * 10)
    assert sorted(len(r) for r in indole) == [5, 6] and sorted(map(sorted, indole)) == [[0, 1, 2, 3, 4, 5], [4, 5, 6, 7, 8]]
    assert rings(6, BENZENE, [1.5] * 6) == rings(6, BENZENE[::-1], [1.5] * 6), "the order of the bonds does not matter"
    assert len(rings(6, BENZENE, [1.5] * 6)) == 1                     # pyridine: the same graph, elements are not looked at
    assert rings(6, BENZENE, [1.0] * 6) == []                        # cyclohexane
    assert rings(6, BENZENE, [1, 2, 1, 2, 1, 2]) == []               # a Kekule benzene
    # a scrambled numbering: every consecutive pair of a ring is bonded, the ring starts at its smallest atom and steps down first
    perm = [7, 2, 9, 0, 5, 3, 8, 1, 6, 4]
    scrambled = [(perm[i], perm[j]) for i, j in NAPHTHALENE]
    for ring in rings(10, scrambled, [1.5] * 11) + naph + indole:
        assert ring[0] == min(ring) and ring[1] < ring[-1]
    assert all(bonded(r, scrambled) for r in rings(10, scrambled, [1.5] * 11)) and all(bonded(r, NAPHTHALENE) for r in naph)
    assert all(bonded(r, INDOLE) for r in indole)
    with pytest.raises(ValueError, match="bond orders"):
        rings(6, BENZENE, [1.5] * 5)


def test_kekule_input_needs_explicit_ligand_rings():
    from physdock_amd.ring_interactions import RingInteractions
    elements = [6] * 6 + [6, 8]                                       # a benzene and two receptor atoms
    kw = dict(elements=elements, bonds=BENZENE, ligand_idx=list(range(6)), residue_of=[0] * 6 + [1, 1], bond_orders=[1, 2, 1, 2, 1, 2])
    assert RingInteractions.from_bonds(**kw).n_ligand_rings == 0
    given = RingInteractions.from_bonds(**kw, ligand_rings=[(0, 1, 2, 3, 4, 5)])
    assert given.n_ligand_rings == 1 and given.ring_atom.tolist() == [0, 1, 2, 3, 4, 5] and given.ring_residue.tolist() == [-1]
    assert RingInteractions.from_bonds(**{**kw, "bond_orders": [1.5] * 6}).n_ligand_rings == 1
    assert RingInteractions.from_bonds(**{**kw, "bond_orders": None}).n_ligand_rings == 0


def test_receptor_rings_by_names():
    from physdock_amd.ring_interactions import receptor_rings_from_names as rings
    phe = ["N", "CA", "CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ"]
    trp = ["CB", "CG", "CD1", "CD2", "NE1", "CE2", "CE3", "CZ2", "CZ3", "CH2"]
    his = ["CG", "ND1", "CD2", "CE1", "NE2"]
    names = phe + trp + his + ["CG", "CD1"]
    res = ["PHE"] * 9 + ["TRP"] * 10 + ["HIS"] * 5 + ["LEU"] * 2
    rid = [3] * 9 + [0] * 10 + [5] * 5 + [1] * 2
    got = rings(res, names, rid)
    at = lambda base, table, *ns: tuple(base + table.index(n) for n in ns)
    assert got == [at(9, trp, "CD2", "CE2", "CZ2", "CH2", "CZ3", "CE3"), at(9, trp, "CG", "CD1", "NE1", "CE2", "CD2"),
                   at(0, phe, "CG", "CD1", "CE1", "CZ", "CE2", "CD2"), at(19, his, "CG", "ND1", "CE1", "NE2", "CD2")]
    assert rings(["TYR"] * 9, phe, [0] * 9) == [at(0, phe, "CG", "CD1", "CE1", "CZ", "CE2", "CD2")]
    mask = np.ones(len(names))
    mask[phe.index("CZ")] = 0
    assert len(rings(res, names, rid, mask)) == 3 and all(phe.index("CG") not in r for r in rings(res, names, rid, mask)), "PHE without CZ"
    assert rings(res[:8], names[:8], rid[:8]) == []                  # CZ missing
    assert rings([" phe "] * 9, [n.lower() for n in phe], [0] * 9) == [at(0, phe, "CG", "CD1", "CE1", "CZ", "CE2", "CD2")]
    with pytest.raises(ValueError, match="atom names"):
        rings(["PHE"], ["CG", "CZ"], [0])


def test_ligand_halogens():
    from physdock_amd.ring_interactions import ligand_halogens_from_bonds as halogens
    assert halogens([6] * 6 + [17], BENZENE + [(0, 6)]) == [(6, 0)]                      # chlorobenzene
    assert halogens([6] * 6 + [9], BENZENE + [(0, 6)]) == []                             # a fluorine
    assert halogens([6, 17, 6], [(0, 1), (1, 2)]) == []                                  # a bridging Cl
    assert halogens([7, 35], [(0, 1)]) == []                                             # N - Br: the neighbour is no carbon
    assert halogens(["C", "I", "H", "Br", "C"], [(0, 1), (0, 2), (3, 4)]) == [(1, 0), (3, 4)]
    assert halogens([6, 17, 1], [(0, 1), (1, 2)]) == [(1, 0)]                            # a hydrogen neighbour does not count


# ------------------------------------------------------------------ analytic geometry on the restatement
def scene(lig_ring=None, rec_ring=None, rec_point=None, lig_point=None, halogen=None, thresholds=ref.THRESHOLDS):
    """one pose: an optional ligand ring (corners [k,3]), a receptor ring in residue 0, a receptor atom ((type, charge), xyz) in
    residue 1, a ligand atom ((type, charge), xyz), a ligand halogen (xyz X, xyz C); -> the restatement's fingerprint"""
    xs, types, charges, rec, lig = [], [], [], [], []

    def add(p, t=0, q=0, receptor=False):
        xs.append(np.asarray(p, dtype=np.float64)); types.append(t); charges.append(q); rec.append(int(receptor))
        if not receptor:
            lig.append(len(xs) - 1)
        return len(xs) - 1
    c = dict(lig_rings=[], rec_rings=[], rec_ring_residue=[], halogens=[], n_residues=2, thresholds=thresholds)
    if lig_ring is not None:
        c["lig_rings"].append([add(p) for p in lig_ring])
    if lig_point is not None:
        add(lig_point[1], *lig_point[0])
    if halogen is not None:
        X, Cc = add(halogen[0]), add(halogen[1])
        c["halogens"].append((lig.index(X), lig.index(Cc)))
    if not lig:
        add([50.0, 50.0, 50.0])
    if rec_ring is not None:
        c["rec_rings"].append([add(p, receptor=True) for p in rec_ring])
        c["rec_ring_residue"].append(0)
    if rec_point is not None:
        add(rec_point[1], *rec_point[0], receptor=True)
    residue_of = [0 if any(a in r for r in c["rec_rings"]) else 1 for a in range(len(xs))]
    c.update(x=np.asarray(xs)[None], lig_idx=lig, types=types, charges=charges, lig_active=[1] * len(lig), rec_mask=rec, residue_of=residue_of)
    return ref.fingerprint(c)


def test_two_benzenes():
    flat = ref.polygon(6, [0, 0, 0], [0, 0, 1])
    stacked = scene(flat, ref.polygon(6, [0, 0, 3.8], [0, 0, 1], 0.3))
    assert stacked["bits"][0].tolist() == [1, 0] and stacked["ring_bits"][0].tolist() == [1] and stacked["ligand_bits"][0].tolist() == [1] * 6
    assert stacked["min_centroid_dist"][0, 0] == pytest.approx(3.8, abs=1e-12) and np.isinf(stacked["min_centroid_dist"][0, 1])
    assert stacked["counts"][0].tolist() == [1, 0, 0, 0, 0]
    assert np.allclose(np.abs(stacked["normal"][0, :, 2]), 1.0) and np.allclose(stacked["centroid"][0], [[0, 0, 0], [0, 0, 3.8]])
    slid = scene(flat, ref.polygon(6, [3.0, 0, 3.8], [0, 0, 1], 0.3))
    assert not slid["bits"].any() and slid["min_centroid_dist"][0, 0] == pytest.approx(np.hypot(3.0, 3.8), abs=1e-12)
    tee = scene(flat, ref.polygon(6, [0, 0, 5.0], [1, 0, 0]))
    assert tee["bits"][0].tolist() == [2, 0] and tee["ring_bits"][0].tolist() == [2]
    tilted = scene(flat, ref.polygon(6, [0, 0, 4.5], [np.sin(np.pi / 4), 0, np.cos(np.pi / 4)]))
    assert not tilted["bits"].any() and not tilted["ring_bits"].any()
    far = scene(flat, ref.polygon(6, [0, 0, 5.6], [0, 0, 1]))
    assert not far["bits"].any()


def test_cations_and_rings():
    flat = ref.polygon(6, [0, 0, 0], [0, 0, 1])
    cation = (ref.DONOR, ref.CATION)
    above = scene(flat, rec_point=(cation, [0, 0, 4.0]))
    assert above["bits"][0].tolist() == [0, 4] and above["ring_bits"][0].tolist() == [4] and above["ligand_bits"][0].tolist() == [4] * 6
    assert not scene(flat, rec_point=(cation, [4.0, 0, 0]))["bits"].any(), "in the ring's plane: the offset is 4 A"
    assert not scene(flat, rec_point=((ref.DONOR, ref.ANION), [0, 0, 4.0]))["bits"].any(), "an anion is no cation"
    assert not scene(flat, rec_point=(cation, [0, 0, 6.1]))["bits"].any()
    swapped = scene(rec_ring=flat, lig_point=(cation, [0, 0, -4.0]))
    assert swapped["bits"][0].tolist() == [8, 0] and swapped["ligand_bits"][0].tolist() == [8]
    assert not scene(rec_ring=flat, lig_point=(cation, [4.0, 0, 0]))["bits"].any()


def test_halogen_bonds():
    acceptor = (ref.ACCEPTOR, 0)
    at = lambda deg, r=3.3: [r * np.cos(np.deg2rad(deg)), r * np.sin(np.deg2rad(deg)), 0.0]       # C at angle 0 from X
    C = [1.74, 0, 0]
    good = scene(halogen=([0, 0, 0], C), rec_point=(acceptor, at(170)))
    assert good["bits"][0].tolist() == [0, 16] and good["ligand_bits"][0].tolist() == [16, 0] and good["counts"][0].tolist() == [0, 0, 0, 0, 1]
    assert not scene(halogen=([0, 0, 0], C), rec_point=(acceptor, at(100)))["bits"].any()
    assert scene(halogen=([0, 0, 0], C), rec_point=(acceptor, at(136)))["bits"].any() and not scene(halogen=([0, 0, 0], C), rec_point=(acceptor, at(134)))["bits"].any()
    assert not scene(halogen=([0, 0, 0], C), rec_point=(acceptor, at(170, 4.1)))["bits"].any()
    assert not scene(halogen=([0, 0, 0], C), rec_point=((ref.DONOR, 0), at(170)))["bits"].any(), "a donor is no acceptor"
    wide = scene(halogen=([0, 0, 0], C), rec_point=(acceptor, at(100)), thresholds=ref.THRESHOLDS[:7] + (95.0,))
    assert wide["bits"][0].tolist() == [0, 16], "the angle is an argument"


# ------------------------------------------------------------------ the condition on the seeds
@pytest.mark.parametrize("name", ref.CASES)
def test_no_seeded_case_leaves_a_bit_open(name):
    c = ref.make_case(name)
    r = ref.restate(c)
    print(f"OPEN | {name} | P {c['x'].shape[0]} A {c['x'].shape[1]} L {len(c['lig_idx'])} R {c['n_residues']} G_l {len(c['lig_rings'])} "
          f"G_r {len(c['rec_rings'])} | bytes {r['n_bytes']} | open {r['open_bytes']} | counts {r['lo']['counts'].sum(0).tolist()} |")
    assert r["open_bytes"] == 0, "a committed seed puts a geometry within the margin of a threshold"
    for k in ("bits", "ligand_bits", "ring_bits", "counts"):
        assert np.array_equal(r["lo"][k], r["hi"][k]) and np.array_equal(r["lo"][k], r["mid"][k])
        assert not np.isnan(r["lo"][k].astype(np.float64)).any()
    assert not (r["lo"]["bits"] >> 5).any() and not (r["lo"]["ligand_bits"] >> 5).any() and not (r["lo"]["ring_bits"] >> 5).any()
    assert np.array_equal(r["lo"]["counts"], ref.popcounts(r["lo"]["bits"]))
    assert r["centroid_bound"].max() < 1e-12 and r["normal_bound"].max() < 1e-10 and r["min_bound"].max() < 1e-5
    x = c["x"][np.isfinite(c["x"]).all((1, 2))]
    assert np.abs(x - np.round(x)).max() > 0, "jittered"


def test_case_a_shows_and_misses_every_kind():
    c = ref.make_case("a_P3_L16_R14")
    assert c["x"].shape[0] == 3 and 150 <= c["x"].shape[1] <= 170 and len(c["lig_idx"]) == 16 and c["n_residues"] == 14
    assert sorted(len(r) for r in c["lig_rings"]) == [5, 6] and sorted(len(r) for r in c["rec_rings"]) == [5, 5, 6, 6, 6, 6]
    assert c["rec_ring_residue"] == [0, 1, 2, 3, 3, 8], "PHE, TYR, HIS, TRP with both rings in one residue, PHE"
    assert c["lig_active"].tolist().count(0) == 1 and len(c["halogens"]) == 2
    f = ref.fingerprint(c)
    bits = f["bits"]
    for k, kind in enumerate(ref.RING_KIND_NAMES):
        shown = (bits >> k & 1).astype(bool)
        assert shown.any() and not shown.all(), kind
        assert (shown.any(0) & ~shown.all(0)).any(), (kind, "a residue shows it in one pose and misses it in another")
    # the designed near misses of pose 0: HIS by the offset alone, TRP by the angle alone, ARG by the offset, residue 7 by the angle
    assert bits[0, [2, 3, 5, 7]].tolist() == [0, 0, 0, 0] and bits[0, [0, 1, 4, 6, 8]].tolist() == [1, 2, 4, 16, 8]
    x0 = c["x"][0].astype(np.float64)
    cen, nrm, ok, _, _ = ref.frames(x0[None], c["lig_rings"] + c["rec_rings"])
    five, his, trp5 = 1, 2 + 2, 2 + 3
    d, off = ref.plane_offset(cen[0, his] - cen[0, five], nrm[0, five])
    assert d < 5.5 - 0.3 and off > 2.0 + 0.3 and abs(nrm[0, five] @ nrm[0, his]) > np.cos(np.deg2rad(30 - 10)), "HIS: distance and angle pass"
    d, off = ref.plane_offset(cen[0, trp5] - cen[0, five], nrm[0, five])
    cosang = abs(nrm[0, five] @ nrm[0, trp5])
    assert d < 5.5 - 0.3 and off < 2.0 - 0.3 and np.cos(np.deg2rad(30 + 8)) > cosang > np.cos(np.deg2rad(60 - 8)), "TRP: 45 degrees"
    br, cb, acc = (x0[c["lig_idx"][i]] for i in (ref.LIG_BR, ref.LIG_BR_C)), None, None
    br, cb = br
    j = [a for a in np.nonzero(c["rec_mask"])[0] if c["residue_of"][a] == 7 and c["types"][a] & ref.ACCEPTOR][0]
    ang = np.rad2deg(np.arccos((cb - br) @ (x0[j] - br) / np.linalg.norm(cb - br) / np.linalg.norm(x0[j] - br)))
    assert np.linalg.norm(x0[j] - br) < 4.0 - 0.3 and 95 < ang < 105, "the bromine's contact: within the distance, at 100 degrees"
    start, _ = ref.csr(c)
    plain = [s for s in range(14) if s not in c["rec_ring_residue"] and
             not any((c["charges"][a] & ref.CATION) or (c["types"][a] & ref.ACCEPTOR) for a in np.nonzero(c["rec_mask"])[0] if c["residue_of"][a] == s)]
    assert len(plain) >= 2 and not bits[:, plain].any() and (np.diff(start)[plain] > 0).any()
    assert not f["ligand_bits"][:, c["lig_active"] == 0].any()


def test_the_other_cases_are_the_shapes_the_issue_names():
    b1, b2, c0 = (ref.make_case(n) for n in ("b_no_ligand_ring", "b_no_receptor_ring", "c_no_receptor_atom"))
    f1, f2, f0 = ref.fingerprint(b1), ref.fingerprint(b2), ref.fingerprint(c0)
    assert not b1["lig_rings"] and b1["rec_rings"] and len(b1["halogens"]) == 1 and (b1["charges"][b1["lig_idx"]] & ref.CATION).any()
    assert not (f1["bits"] & 7).any() and (f1["bits"] & 8).any() and (f1["bits"] & 16).any() and np.isinf(f1["min_centroid_dist"]).all()
    assert b2["lig_rings"] and not b2["rec_rings"] and not (f2["bits"] & 11).any() and (f2["bits"] & 4).any() and np.isinf(f2["min_centroid_dist"]).all()
    assert not c0["rec_mask"].any() and not f0["bits"].any() and not f0["ligand_bits"].any() and not f0["ring_bits"].any()
    assert np.isinf(f0["min_centroid_dist"]).all() and not f0["counts"].any()
    d = ref.make_case("d_P2_A700")
    rec = np.nonzero(d["rec_mask"])[0]
    n_acc, n_cat = int((d["types"][rec] & ref.ACCEPTOR > 0).sum()), int((d["charges"][rec] & ref.CATION > 0).sum())
    G, E = len(d["lig_rings"]) + len(d["rec_rings"]), len(d["rec_rings"]) + len(rec)
    assert d["x"].shape[0] == 2 and 650 <= d["x"].shape[1] <= 760 and n_acc > 256 and len(d["rec_rings"]) > 64 and n_cat > 2
    assert G > ref.FRAME_BLOCK and E > 2 * ref.RECEPTOR_BLOCK and len(d["rec_rings"]) > ref.LIGAND_BLOCK and len(rec) > ref.LIGAND_BLOCK
    assert d["n_residues"] > ref.FOLD_BLOCK and len(d["lig_idx"]) > ref.FOLD_BLOCK
    fd = ref.fingerprint(d)
    assert all((fd["bits"] >> k & 1).any() for k in range(5))
    assert (fd["bits"][:, max(d["rec_ring_residue"])] != 0).any() or (fd["bits"][:, 14:76] != 0).any(), "rings behind the first block take part"
    src = open(__file__.replace("tests/test_plif_rings_cpu.py", "physdock_amd/csrc/plif_rings.hip")).read()
    for name in ("FRAME_BLOCK", "RECEPTOR_BLOCK", "LIGAND_BLOCK", "FOLD_BLOCK"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) == getattr(ref, name)
    e = ref.make_case("e_P66")
    assert e["x"].shape[0] == 66 and len(set(map(bytes, ref.fingerprint(e)["bits"]))) > 10, "66 poses that differ"
    f = ref.make_case("f_degenerate_and_nan")
    ff = ref.fingerprint(f)
    assert len(f["lig_rings"]) == 3 and len(f["lig_rings"][2]) == 3 and not ff["ok"][:, 2].any() and not ff["normal"][:, 2].any()
    assert np.isnan(f["x"]).sum() == 1 and not ff["ok"][ref.F_NAN_POSE, 0] and ff["ok"][ref.F_NAN_POSE, 1:2].all() and ff["ok"][0, :2].all()
    assert ff["ring_bits"][0, 0] and not ff["ring_bits"][ref.F_NAN_POSE, 0] and not ff["ring_bits"][:, 2].any()
    clean = dict(f, x=np.where(np.isnan(f["x"]), np.float32(0.0), f["x"]))
    clean["x"][ref.F_NAN_POSE] = f["x"][0]                             # pose 0 in place of the poisoned pose: the other poses and rings
    fc = ref.fingerprint(clean)
    keep = [p for p in range(3) if p != ref.F_NAN_POSE]
    assert all(np.array_equal(ff[k][keep], fc[k][keep]) for k in ("bits", "ligand_bits", "ring_bits"))
    assert ff["ring_bits"][ref.F_NAN_POSE, 1] == ff["ring_bits"][0, 1] != 0, "the five-ring of the poisoned pose is untouched"
    assert np.isnan(ff["centroid"][ref.F_NAN_POSE, 0]).any() and np.isfinite(ff["min_centroid_dist"][ref.F_NAN_POSE, 2])


@pytest.mark.parametrize("name", ["a_P3_L16_R14", "f_degenerate_and_nan"])
def test_the_restatement_does_not_depend_on_where_a_ring_starts_or_which_way_it_runs(name):
    c = ref.make_case(name)
    base = ref.fingerprint(c)
    for which in ("lig_rings", "rec_rings"):
        for g in range(len(c[which])):
            ring = list(c[which][g])
            for new in (ring[2:] + ring[:2], ring[::-1], ring[:1] + ring[:0:-1]):
                moved = dict(c, **{which: c[which][:g] + [new] + c[which][g + 1:]})
                got = ref.fingerprint(moved)
                assert all(np.array_equal(got[k], base[k]) for k in ("bits", "ligand_bits", "ring_bits", "counts")), (which, g, new)
                assert np.allclose(got["min_centroid_dist"], base["min_centroid_dist"], rtol=1e-13, atol=0)
                assert ref.restate(moved)["open_bytes"] == 0


# ------------------------------------------------------------------ the class on the host
def ri_of(c, **kw):
    from physdock_amd.ring_interactions import RingInteractions
    local = {int(a): i for i, a in enumerate(c["lig_idx"])}
    return RingInteractions.from_tables(c["types"], c["charges"], c["lig_idx"], c["rec_mask"], c["residue_of"],
                                        ligand_rings=[[local[int(a)] for a in r] for r in c["lig_rings"]], receptor_rings=c["rec_rings"],
                                        halogens=c["halogens"], n_residues=c["n_residues"], ligand_active=c["lig_active"],
                                        thresholds=c["thresholds"], **kw)


@pytest.mark.parametrize("name", ref.CASES)
def test_the_tables_of_the_seeded_cases(name):
    c = ref.make_case(name)
    f = ri_of(c)
    start, atom = ref.csr(c)
    ring_start, ring_atom, ring_residue, halogen = ref.ring_tables(c)
    assert np.array_equal(f.res_start, start) and np.array_equal(f.res_atom, atom)
    assert np.array_equal(f.ring_start, ring_start) and np.array_equal(f.ring_atom, ring_atom) and np.array_equal(f.ring_residue, ring_residue)
    assert np.array_equal(f.halogens, halogen) and f.halogens.shape == (len(c["halogens"]), 2)
    assert all(a.dtype == np.int32 for a in (f.ring_start, f.ring_atom, f.ring_residue, f.halogens))
    assert (f.n_ligand_rings, f.n_receptor_rings, f.n_halogens) == (len(c["lig_rings"]), len(c["rec_rings"]), len(c["halogens"]))
    assert list(f._thr)[:5] == list(ref.THRESHOLDS[:5]) and list(f._thr)[5:] == [np.cos(np.deg2rad(v)) for v in ref.THRESHOLDS[5:]]


def test_receptor_rings_are_sorted_by_residue_and_labels_reach_describe():
    from physdock_amd.ring_interactions import RingInteractions as F
    z = np.zeros(14, np.uint8)
    residue_of = [2] * 5 + [0] * 6 + [1, 1, 1]
    f = F.from_tables(z, z, [11, 12, 13], np.ones(14), residue_of, ligand_rings=[(0, 1, 2)], receptor_rings=[(0, 1, 2, 3, 4), (5, 6, 7, 8, 9, 10)],
                      halogens=[(2, 1)], residue_labels=["PHE82", "LIG", "HIS41"])
    assert f.ring_residue.tolist() == [-1, 0, 2] and f.ring_start.tolist() == [0, 3, 9, 14] and f.ring_atom.tolist()[:3] == [11, 12, 13]
    assert f.describe(np.array([3, 0, 24], np.uint8)) == [("PHE82", ["pi_parallel", "pi_tshaped"]), ("HIS41", ["cation_pi", "halogen_bond"])]
    assert f.required_row([("PHE82", "pi_parallel"), (2, "halogen_bond")]).tolist() == [1, 0, 16]
    assert "RingInteractions(n_atoms=3, n_pose_atoms=14, residues=3, receptor_atoms=11, ligand_rings=1, receptor_rings=2, halogens=1" in repr(f)


def test_from_batch_with_and_without_names():
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.interactions import InteractionFingerprint
    from physdock_amd.ring_interactions import RingInteractions, receptor_rings_from_names
    from physdock_amd.scoring import names_from_meta
    from physdock_amd.synthetic import make_batch, pdb_meta
    batch = make_batch(20, 4, 9, 4, seed=6)
    is_lig = ligand_atom_mask(batch).numpy()
    n_lig = int(is_lig.sum())
    bonds = [(i, i + 1) for i in range(n_lig - 1)]
    f = RingInteractions.from_batch(batch, bonds)
    g = InteractionFingerprint.from_batch(batch, bonds)
    assert f.receptor_typing == "elements" and f.n_receptor_rings == 0 and f.n_ligand_rings == 0 and f.residue_labels is None
    assert not f.charges[~is_lig].any() and not (f.types[~is_lig] & ref.ACCEPTOR).any(), "nothing on the receptor side can fire"
    for k in ("types", "charges", "ligand_idx", "lig_active", "rec_mask", "residue_of", "res_start", "res_atom"):
        assert np.array_equal(getattr(f, k), getattr(g, k)), k
    meta = pdb_meta({k: batch[k].numpy() for k in ("token_id_to_chunk_sizes", "asym_id", "is_ligand", "residue_index")})
    named = RingInteractions.from_batch(batch, bonds, infer_meta_data=meta, thresholds={"stack_dist": 6.0})
    gn = InteractionFingerprint.from_batch(batch, bonds, infer_meta_data=meta)
    assert named.receptor_typing == "names" and named.thresholds["stack_dist"] == 6.0 and named.thresholds["t_angle"] == 60.0
    assert np.array_equal(named.types, gn.types) and np.array_equal(named.charges, gn.charges) and named.residue_labels == gn.residue_labels
    res, names, z, _ = names_from_meta(meta)
    want = receptor_rings_from_names(res, names, batch["atom_id_to_token_id"].numpy(), named.rec_mask)
    assert named.n_receptor_rings == len(want) and sorted(named.ring_atom.tolist()) == sorted(a for r in want for a in r)
    assert (np.diff(named.ring_residue) >= 0).all()
    heavy = np.nonzero(f.lig_active)[0][:3].tolist()                  # a ring with an atom that takes no part would be dropped
    ringed = RingInteractions.from_batch(batch, bonds, ligand_rings=[heavy])
    assert len(heavy) == 3 and ringed.n_ligand_rings == 1 and ringed.ring_atom.tolist() == f.ligand_idx[heavy].tolist()


def test_constructor_argument_errors():
    from physdock_amd import ring_interactions as RI
    F = RI.RingInteractions
    z = np.zeros(12, np.uint8)
    ok = dict(types=z, charges=z, ligand_idx=[0, 1, 2, 3], receptor_mask=np.ones(12), residue_of=[0] * 4 + [1] * 4 + [2] * 4,
              ligand_rings=[(0, 1, 2)], receptor_rings=[(4, 5, 6, 7)], halogens=[(3, 2)])
    F.from_tables(**ok)
    for change, match in ((dict(ligand_rings=[(0, 1)]), "ligand ring holds 3 .. 8"), (dict(ligand_rings=[(0, 1, 1)]), "distinct"),
                          (dict(ligand_rings=[(0, 1, 4)]), "below 4"), (dict(ligand_rings=[tuple(range(9))]), "3 .. 8"),
                          (dict(receptor_rings=[(4, 5, 12)]), "receptor ring holds"), (dict(receptor_rings=[(6, 7, 8)]), "inside one residue"),
                          (dict(receptor_rings=[(1, 2, 3)]), "made of receptor atoms"), (dict(halogens=[(3, 3)]), "halogens are"),
                          (dict(halogens=[(4, 0)]), "halogens are"), (dict(ligand_rings=[(0, 1, 2)] * 65), "at most 64"),
                          (dict(halogens=[(3, 2)] * 65), "at most 64"), (dict(thresholds={"stack_dist": -1.0}), "finite and not negative"),
                          (dict(thresholds={"halogen_dist": float("nan")}), "finite"), (dict(thresholds={"t_angle": 181.0}), "0 .. 180"),
                          (dict(thresholds={"parallel_angle": float("nan")}), "0 .. 180"), (dict(thresholds={"contact": 4.0}), "unknown thresholds"),
                          (dict(thresholds=(5.5, 2.0, 6.0)), "got 3 values"), (dict(residue_labels=["A"]), "residue labels"),
                          (dict(ligand_idx=[0, 0, 1, 2]), "distinct"), (dict(charges=np.full(12, 4)), "CATION, ANION")):
        with pytest.raises(ValueError, match=match):
            F.from_tables(**{**ok, **change})
    f = F.from_tables(**ok, thresholds={"halogen_angle": 140.0})
    assert f.thresholds == {**RI.DEFAULT_RING_THRESHOLDS, "halogen_angle": 140.0} and f._thr[7] == np.cos(np.deg2rad(140.0))
    with pytest.raises(ValueError, match="pose atoms"):
        f.fingerprint(torch.zeros(2, 11, 3))
    with pytest.raises(ValueError, match="RingInteractions.compare: bits must be a uint8 tensor"):
        f.compare(torch.zeros(2, 3), torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="RingInteractions.pairwise"):
        f.pairwise(torch.zeros(2, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="unknown interaction kind"):
        f.compare(torch.zeros(2, 3, dtype=torch.uint8), torch.zeros(3, dtype=torch.uint8), kinds=("contact",))
    with pytest.raises(ValueError, match="unknown interaction kind"):
        f.required_row([(0, "hbond_donor")])
    with pytest.raises(ValueError, match="RingInteractions: residue 3 is not in"):
        f.required_row([(3, "pi_cation")])
    with pytest.raises(ValueError, match="one shape"):
        F.combined(torch.zeros(2, 3, dtype=torch.uint8), torch.zeros(2, 4, dtype=torch.uint8))
    both = F.combined(torch.full((2, 3), 63, dtype=torch.uint8), torch.full((2, 3), 31, dtype=torch.uint8))
    assert both.shape == (2, 6) and both.dtype == torch.uint8 and both[0].tolist() == [63] * 3 + [31] * 3
    assert RI.ring_kind_mask() == 31 and RI.ring_kind_mask(("pi_parallel", "halogen_bond")) == 17 and RI.ring_kind_mask("cation_pi") == 8
    with pytest.raises(ValueError, match="at least one"):
        RI.ring_kind_mask(())


def test_constants_header_and_library():
    import physdock_amd
    from physdock_amd import _lib, interactions, ring_interactions as RI
    assert physdock_amd.RingInteractions is RI.RingInteractions
    assert RI.RING_KIND_NAMES == ref.RING_KIND_NAMES and RI.RING_THRESHOLD_NAMES == ref.THRESHOLD_NAMES
    assert tuple(RI.DEFAULT_RING_THRESHOLDS[k] for k in RI.RING_THRESHOLD_NAMES) == ref.THRESHOLDS
    assert (interactions.CATION, RI.ACCEPTOR) == (ref.CATION, ref.ACCEPTOR)
    assert (RI.MAX_LIGAND_RINGS, RI.MAX_RECEPTOR_RINGS, RI.MAX_HALOGENS, RI.MAX_RING_SIZE) == (64, 4096, 64, 8)
    assert _lib.ABI_VERSION == 11
    assert {"pd_plif_rings", "pd_plif_rings_workspace"} <= set(_lib.header_symbols())
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "physdock_hip.h")).read()
    assert int(re.search(r"#define\s+PD_PLIF_RING_KINDS\s+(\d+)", hdr).group(1)) == len(RI.RING_KIND_NAMES) == 5
    assert int(re.search(r"#define\s+PD_PLIF_RING_THRESHOLDS\s+(\d+)", hdr).group(1)) == len(RI.RING_THRESHOLD_NAMES) == 8
    assert int(re.search(r"#define\s+PD_PLIF_KINDS\s+(\d+)", hdr).group(1)) == 6, "the six kinds stay"
    L = _lib.lib()
    assert L.pd_abi_version() == 11
    want = {"pd_plif_rings": 30, "pd_plif_rings_workspace": 6}
    assert all(hasattr(L, k) and k in _lib.SYMBOLS and len(_lib.SYMBOLS[k].argtypes) == n for k, n in want.items())
    # the workspace size needs no device: 9 bytes per receptor ring and one per list entry, ligand atom and halogen, per pose
    assert L.pd_plif_rings_workspace(3, 16, 100, 2, 6, 2) == (3 * (9 * 6 + 100 + 16 + 2) + 7) // 8 * 8
    assert L.pd_plif_rings_workspace(1, 1, 0, 0, 0, 0) == 8
    assert L.pd_plif_rings_workspace(0, 16, 100, 2, 6, 2) == -1 and L.pd_plif_rings_workspace(3, 16, -1, 2, 6, 2) == -1
    assert L.pd_plif_rings_workspace(65535, 1024, 1 << 22, 64, 4096, 64) == -3, "more than an int holds"


def test_redock_takes_the_keyword_on_every_path():
    import inspect
    from physdock_amd import driver
    assert inspect.signature(driver.redock).parameters["ring_interactions"].default is None
    assert inspect.signature(driver._RedockState.__init__).parameters["ring_interactions"].default is None
    extra = set(inspect.signature(driver._RedockState.__init__).parameters) - set(inspect.signature(driver.redock).parameters)
    assert extra == {"self", "pbatch"}, "the grouped path takes the keywords of redock, no others"
