"""The pocket grid without a GPU: the float64 restatement (tests/pocket_ref.py) on hand-made lattices, the step table, the host tables of
physdock_amd/pocket.py and their argument checks, describe, lining, the OpenDX text, the header, the keyword plumbing of redock - and
the conditions the GPU tests rest on: every seeded case of tests/pocket_ref.py is closed (no flag differs between the thresholds moved
by -MARGIN and +MARGIN; one `OPEN | ...` line per case, pytest -s) and shows the structure it was planted for."""
import re

import numpy as np
import pytest
import torch

import pocket_ref as ref


@pytest.fixture(scope="module")
def restated():
    """every seeded case and its restatement, computed once"""
    cases = {name: ref.make_case(name) for name in ref.CASES}
    return {name: (c, ref.restate(c)) for name, c in cases.items()}


# ------------------------------------------------------------------ the restatement on hand-made input
def test_enclosure_and_components_follow_the_definition():
    n = 9
    solid = np.zeros((n, n, n), dtype=bool)
    solid[2, 4, 4] = solid[6, 4, 4] = True                           # a wall on either side of (4, 4, 4) along x only
    b = ref.enclosure(solid, [12] * 7)
    assert b[4, 4, 4] == 1 and b[3, 4, 4] == 1 and b[1, 4, 4] == 0 and b[4, 4, 5] == 0
    assert ref.enclosure(solid, [1] * 7)[4, 4, 4] == 0 and ref.enclosure(solid, [2] * 7)[4, 4, 4] == 1, "a hit counts within the steps only"
    solid[:] = True
    solid[4, 4, 4] = False
    assert ref.enclosure(solid, [1] * 7)[4, 4, 4] == 7
    solid[4, 4, 0] = False                                           # a point on a face: leaving the lattice is not a hit
    assert ref.enclosure(solid, [12] * 7)[4, 4, 0] == 2
    pocket = np.zeros((n, n, n), dtype=bool)
    pocket[1, 1, 1:4] = pocket[1, 2, 3] = True                       # an L of four points
    pocket[2, 2, 2] = True                                           # touches it only across a diagonal: its own component
    pocket[0, 8, 8] = True
    lab = ref.components(pocket)
    assert lab[1, 1, 1] == lab[1, 1, 3] == lab[1, 2, 3] == 1 and lab[2, 2, 2] == 2 and lab[0, 8, 8] == 0, "ranked by the smallest index"
    assert (lab[~pocket] == -1).all() and lab.max() == 2


@pytest.mark.parametrize("reach,h,want", [(12.0, 1.0, [12, 12, 12, 6, 6, 6, 6]), (12.0, 0.5, [24, 24, 24, 13, 13, 13, 13]),
                                          (8.0, 1.5, [5, 5, 5, 3, 3, 3, 3]), (0.9, 1.0, [0] * 7), (np.sqrt(3.0) * 2, 1.0, [3, 3, 3, 2, 2, 2, 2])])
def test_the_step_table(reach, h, want):
    from physdock_amd import pocket
    assert pocket.step_table(reach, h) == want == ref.step_table(reach, h)
    assert pocket.DIRECTIONS == ref.DIRECTIONS and len(pocket.DIRECTIONS) == 7


def test_centre_mean_snap_and_origin():
    x = np.float32([[1.25, 2.5, -3.75], [2.25, 3.5, -2.75], [100, 100, 100], [9, 9, 9]])
    cls = np.uint8([2, 2, 1, 0])
    assert ref.centre_of(x, cls, [0, 1, 3], 1.0, snap=False).tolist() == [1.75, 3.0, -3.25]
    assert ref.centre_of(x, cls, [0, 1, 3], 1.0).tolist() == [2.0, 3.0, -3.0], "rint: halves go to the even neighbour"
    assert ref.centre_of(x, cls, [0, 1, 3], 0.5).tolist() == [2.0, 3.0, -3.0] and ref.centre_of(x, cls, [3], 1.0).tolist() != [9, 9, 9]
    assert np.isnan(ref.centre_of(x, cls, [3], 1.0)).all(), "no active ligand atom: no centre"
    assert ref.centre_of(x, cls, [0], 1.0, centre=[0.3, 0.5, 1.5]).tolist() == [0.0, 0.0, 2.0]


# ------------------------------------------------------------------ the conditions on the seeds
@pytest.mark.parametrize("name", list(ref.CASES))
def test_every_seeded_case_is_closed(restated, name):
    c, r = restated[name]
    v = ref.values_of(c, r["counts"], r["atom_buried"])
    print(f"OPEN | {name} | x {c['x'].shape} n {c['n']} | open {r['open_flags']} | band pairs {r['band']} | counts {r['counts'].tolist()} | "
          f"filled {np.round(v['filled_fraction'][0], 3).tolist()} |")
    assert r["open_flags"] == 0, "a committed seed puts a point within MARGIN of a threshold"
    assert c["x"].dtype == np.float32 and np.abs(c["x"]).max() <= 64.0 and (r["ok"] == 1).all()
    assert (r["counts"][:, 0] + r["counts"][:, 1] == c["n"] ** 3).all() and (r["counts"][:, 4] <= r["counts"][:, 3]).all()
    assert (r["counts"][:, 3] <= r["counts"][:, 2]).all() and (r["counts"][:, 7] <= r["counts"][:, 6]).all()
    assert c["x"].shape[1] <= 1 << 22 and len(c["lig_idx"]) <= 1024 and c["n_residues"] <= 4096 and 8 <= c["n"] <= 48


def test_the_cases_show_what_they_were_planted_for(restated):
    shape = lambda k: restated[k][0]["x"].shape[:2] + (len(restated[k][0]["lig_idx"]), restated[k][0]["n"])
    assert shape("a") == (3, 70, 9, 9) and shape("c")[1:] == (530, 9, 33) and shape("b")[3] == shape("d")[3] == 16
    c, r = restated["a"]
    f = ref.values_of(c, r["counts"], r["atom_buried"])["filled_fraction"][0]
    assert (r["counts"][:, 3] > 0).all() and (f > 0).all() and (f < 1).all(), "a: a site the ligand fills in part"
    assert (r["lining_residues"] > 0).all() and (r["atom_class"] == 4).all()
    c, r = restated["b"]
    assert r["counts"][0, 6] >= 2 and r["counts"][0, 7] == 1 and (r["classes"] == 2).any(), "b: a second cavity outside the site"
    c, r = restated["c"]
    assert (r["counts"][:, 3] > 0).all() and c["x"].shape[1] > 2 * 256, "c: more than two LDS tiles of atoms, rows of two words"
    c, r = restated["d"]
    tun = ref.tunnel_points()
    assert len(tun) >= 60 and len(set(tun)) == len(tun) and r["counts"][0].tolist()[1:8] == [len(tun), len(tun), len(tun), 2, 2, 1, 1]
    cl = r["classes"][0].reshape(16, 16, 16)
    assert all(cl[q] in (3, 4) for q in tun) and (cl > 0).sum() == len(tun), "d: the tunnel and nothing else is the site"
    for q in tun:                                                    # one point wide: a tunnel point touches its two neighbours along the walk only
        nb = sum(tuple(np.add(q, d)) in set(tun) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)))
        assert nb == (1 if q in (tun[0], tun[-1]) else 2)
    c, r = restated["e"]
    v = ref.values_of(c, r["counts"], r["atom_buried"])
    assert (r["counts"][:, 3] == 0).all() and (r["counts"][:, 5] > 0).all() and (r["atom_class"] == 1).all(), "e: free, not pocket"
    assert all((v[k][0] == 0).all() for k in ("site_volume", "filled_fraction", "ligand_in_site", "ligand_enclosure"))
    c, r = restated["f"]
    assert r["truncated"][0] == 1 and r["counts"][0, 3] > 0 and c["min_enclosed"] == 2, "f: the site reaches a face"
    assert not any(r["truncated"].any() for k, (c, r) in restated.items() if k != "f")
    c, r = restated["g"]
    cls = ref.classes(c)
    assert cls[ref.G_HOLE] == 0 and cls[ref.G_HYDROGEN] == 0 and cls[c["lig_idx"][ref.G_INACTIVE]] == 0 and cls[ref.G_NAN[1]] == 1
    assert (r["atom_class"][:, [ref.G_INACTIVE, ref.G_OUTSIDE]] == 255).all() and (r["atom_buried"][:, ref.G_OUTSIDE] == 255).all()
    assert (np.delete(r["atom_class"], [ref.G_INACTIVE, ref.G_OUTSIDE], axis=1) != 255).all() and (r["counts"][:, 3] > 0).all()
    x = c["x"].copy()
    x[ref.G_NAN[0], ref.G_NAN[1], 1] = np.nan
    bad = ref.restate(c, x)
    assert bad["ok"].tolist() == [1, 0, 1] and not bad["counts"][1].any() and (bad["classes"][1] == 255).all() and np.isnan(bad["centre"][1]).all()
    assert all(np.array_equal(bad[k][[0, 2]], r[k][[0, 2]]) for k in ("classes", "buried", "counts", "atom_class", "lining_points"))
    c, r = restated["h"]
    wide = ref.restate(c, margin=ref.BAND)
    print(f"PLANTED | h | flags open at +-{ref.BAND} A: {wide['open_flags']} | band pairs {r['band']} |")
    assert wide["open_flags"] >= 4 * c["x"].shape[0] and r["band"] >= 6 * c["x"].shape[0], "h: planted pairs decide flags inside any fp32 band"
    assert (r["counts"][:, 3] > 0).all() and (r["lining_residues"] > 0).all()
    for p in range(c["x"].shape[0]):                                 # every planted atom sits within 3e-6 A of its threshold, outside MARGIN
        ctr = ref.centre_of(c["x"][p], ref.classes(c), c["lig_idx"], c["h"])
        for m, (a, t) in enumerate(zip(ref.H_PLANTED, ref.H_TARGETS)):
            g, xa = ctr + np.asarray(t) * c["h"], c["x"][p, a].astype(np.float64)
            off = (xa[0] - g[0]) - (float(c["radius"][a]) + (c["probe"] if m < 4 else c["lining"]))
            assert xa[1] == g[1] and xa[2] == g[2] and 100 * ref.MARGIN < abs(off) < 3e-6 and (off < 0) == (m % 2 == 0), (p, a, off)


# ------------------------------------------------------------------ host tables
@pytest.mark.parametrize("name", ["a", "d", "g"])
def test_the_tables_of_the_seeded_cases(name):
    from physdock_amd.pocket import PocketGrid
    c = ref.make_case(name)
    s = PocketGrid.from_arrays(c["elements"], c["lig_idx"], c["receptor_mask"], c["residue_of"], n_residues=c["n_residues"], a_mask=c["a_mask"],
                               ligand_active=c["lig_active"], n=c["n"], probe=c["probe"], lining=c["lining"], min_enclosed=c["min_enclosed"],
                               radii={6: float(c["radius"][0])} if name == "d" else None)
    start, atom = ref.csr(c)
    assert np.array_equal(s.cls, ref.classes(c)) and s.cls.dtype == np.uint8
    assert np.array_equal(s.radius, c["radius"]) and s.radius.dtype == np.float32 and np.array_equal(s.ligand_idx, c["lig_idx"])
    assert np.array_equal(s.res_start, start) and np.array_equal(s.res_atom, atom) and s.res_start.dtype == s.res_atom.dtype == np.int32
    assert (s.n_atoms, s.n_pose_atoms, s.n_residues, s.n_receptor_atoms) == (len(c["lig_idx"]), c["x"].shape[1], c["n_residues"], len(atom))
    assert (s.h, s.n, s.probe, s.lining_distance, s.reach, s.min_enclosed, s.snap) == (1.0, c["n"], c["probe"], c["lining"], 12.0, c["min_enclosed"], True)
    assert s.steps == [min(v, c["n"]) for v in ref.step_table(12.0, 1.0)]


def test_defaults_masks_radii_and_repr():
    from physdock_amd import pocket, validity
    from physdock_amd.pocket import PocketGrid as G
    assert (pocket.DEFAULT_SPACING, pocket.DEFAULT_N, pocket.DEFAULT_REACH, pocket.DEFAULT_MIN_ENCLOSED) == (ref.H, ref.N, ref.REACH, ref.MIN_ENCLOSED)
    assert np.float32(pocket.DEFAULT_PROBE) == np.float32(ref.PROBE) and np.float32(pocket.DEFAULT_LINING) == np.float32(ref.LINING)
    assert validity.VDW_RADII == ref.VDW_RADII and validity.DEFAULT_RADIUS == ref.DEFAULT_RADIUS
    assert pocket.COUNT_NAMES == ref.COUNT_NAMES and pocket.VALUE_NAMES == ref.VALUE_NAMES and (pocket.MIN_N, pocket.MAX_N) == (8, 48)
    elements = [6, 7, 8, 1, 16, 30, 6, 7, 8, 6]
    residue_of = [2, 0, 2, 4, 0, 3, 3, 2, 1, 1]
    s = G.from_arrays(elements, [7, 8, 9], [1, 1, 1, 1, 1, 0, 1, 1, 1, 1], residue_of, n_residues=6, a_mask=[1, 0, 1, 1, 1, 1, 1, 1, 1, 1],
                      ligand_active=[1, 1, 0])
    assert s.cls.tolist() == [1, 0, 1, 0, 1, 0, 1, 2, 2, 0]
    assert np.array_equal(s.radius, np.float32([1.7, 1.6, 1.55, 1.2, 1.8, 2.0, 1.7, 1.6, 1.55, 1.7]))
    assert s.res_start.tolist() == [0, 1, 1, 3, 4, 4, 4] and s.res_atom.tolist() == [4, 0, 2, 6]
    assert s.probe == float(np.float32(1.4)) and s.lining_distance == float(np.float32(2.4)) and s.steps == [12, 12, 12, 6, 6, 6, 6]
    assert repr(s) == ("PocketGrid(n_atoms=3, n_pose_atoms=10, residues=6, receptor_atoms=4, active_ligand_atoms=2, h=1, n=32, probe=1.4, "
                       "lining=2.4, reach=12, min_enclosed=5, snap=True)")
    over = G.from_arrays(elements, [7, 8, 9], np.ones(10), residue_of, radii={6: 1.9, 30: 1.4}, h=0.5, n=48, reach=100.0, snap=False)
    assert np.array_equal(over.radius, np.float32([1.9, 1.6, 1.55, 1.2, 1.8, 1.4, 1.9, 1.6, 1.55, 1.9])) and over.steps == [48] * 7
    given = G.from_arrays(None, [7, 8, 9], np.ones(10), residue_of, radius=np.full(10, 1.5))
    assert np.array_equal(given.radius, np.full(10, 1.5, np.float32)) and given.cls.tolist() == [1] * 7 + [2] * 3


def test_from_batch_takes_tokens_as_residues():
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.pocket import PocketGrid
    from physdock_amd.synthetic import make_batch, pdb_meta
    batch = make_batch(20, 4, 9, 4, seed=6)
    is_lig = ligand_atom_mask(batch).numpy()
    T = int(batch["is_ligand"].shape[0])
    s = PocketGrid.from_batch(batch)
    z = (batch["ref_feat"][:, 4:132].argmax(-1) + 1).numpy()
    assert s.n_residues == T and s.residue_labels is None and np.array_equal(s.ligand_idx, np.nonzero(is_lig)[0])
    assert np.array_equal(s.cls == 2, is_lig & (z != 1)) and np.array_equal(s.cls == 1, ~is_lig & (z != 1))
    assert np.array_equal(s.radius, ref.radii_of(z)) and np.array_equal(s.residue_of, batch["atom_id_to_token_id"].numpy())
    meta = pdb_meta({k: batch[k].numpy() for k in ("token_id_to_chunk_sizes", "asym_id", "is_ligand", "residue_index")})
    named = PocketGrid.from_batch(batch, infer_meta_data=meta, n=16, probe=1.2)
    assert len(named.residue_labels) == T and named.residue_labels[0] and named.n == 16 and named.probe == float(np.float32(1.2))


def test_constructor_and_measure_argument_errors():
    from physdock_amd.pocket import PocketGrid as G
    ok = dict(elements=[6] * 8, ligand_idx=[1], receptor_mask=np.ones(8), residue_of=[0, 0, 1, 1, 2, 2, 3, 3])
    G.from_arrays(**ok)
    for change, match in ((dict(ligand_idx=[1, 1]), "distinct"), (dict(ligand_idx=[8]), "distinct"), (dict(elements=[6] * 7), "elements for 7"),
                          (dict(residue_of=[0] * 7), "residue_of 7"), (dict(residue_of=[0, 0, 1, 1, 2, 2, 3, -1]), "residue_of must lie"),
                          (dict(n_residues=3), "residue_of must lie"), (dict(ligand_active=[1, 1]), "ligand_active 2"),
                          (dict(a_mask=np.ones(9)), "a_mask 9"), (dict(n=7), "n = 7"), (dict(n=49), "n = 49"), (dict(h=0.0), "spacing"),
                          (dict(h=float("nan")), "spacing"), (dict(h=100.0, n=48), "spacing"), (dict(probe=-0.1), "probe"),
                          (dict(lining=float("inf")), "lining"), (dict(reach=-1.0), "reach"), (dict(min_enclosed=8), "min_enclosed = 8"),
                          (dict(min_enclosed=-1), "min_enclosed"), (dict(radii={6: -1.0}), "finite and positive"),
                          (dict(radius=np.ones(7)), "radius for 7"), (dict(radius=np.ones(8), radii={6: 1.0}), "cannot be combined"),
                          (dict(elements=None), "elements or radius"), (dict(residue_labels=["A", "B"]), "residue labels")):
        with pytest.raises(ValueError, match=match):
            G.from_arrays(**{**ok, **change})
    with pytest.raises(ValueError, match="ligand atoms"):
        G.from_arrays([6] * 2000, np.arange(1025), np.ones(2000), np.zeros(2000))
    with pytest.raises(ValueError, match="at most 4096"):
        G.from_arrays([6] * 5000, [0], np.ones(5000), np.arange(5000))
    s = G.from_arrays(**ok)
    with pytest.raises(ValueError, match=r"8 pose atoms, x_pred has shape \(2, 7, 3\)"):
        s.measure(torch.zeros(2, 7, 3))
    with pytest.raises(ValueError, match="centre"):
        s.measure(torch.zeros(2, 8, 3), centre="receptor")
    with pytest.raises(ValueError, match=r"centre has shape \(3, 3\)"):
        s.measure(torch.zeros(2, 8, 3), centre=np.zeros((3, 3)))


def test_describe_lining_and_the_dx_text():
    from physdock_amd.pocket import PocketGrid as G
    ok = dict(elements=[6] * 8, ligand_idx=[1], receptor_mask=np.ones(8), residue_of=[0, 0, 1, 1, 2, 2, 3, 3], n=8, h=0.5)
    plain, named = G.from_arrays(**ok), G.from_arrays(**ok, residue_labels=["LIG:C1", "ASP25", "", "LYS83"])
    classes = torch.arange(2 * 512).reshape(2, 512) % 5
    res = {"lining_points": torch.tensor([[0, 5, 12, 5], [1, 0, 0, 0]], dtype=torch.int32), "centre": torch.tensor([[1.0, 2.0, 3.5], [0.0, 0.0, 0.0]]),
           "classes": classes.to(torch.uint8)}
    assert plain.describe(res, 0) == [(2, 12), (1, 5), (3, 5)] and plain.describe(res, 0, min_points=6) == [(2, 12)] and plain.describe(res, 1) == [(0, 1)]
    assert named.describe(res, 0) == [(2, 12), ("ASP25", 5), ("LYS83", 5)]
    assert plain.lining(res).tolist() == [[False, True, True, True], [True, False, False, False]]
    assert plain.lining(res, min_points=6).tolist() == [[False, False, True, False], [False] * 4]
    with pytest.raises(ValueError, match="a row holds 4 counts, got 3"):
        plain.describe({"lining_points": torch.zeros(2, 3)}, 0)
    text = plain.to_dx(res, 0)
    lines = text.splitlines()
    assert lines[1] == "object 1 class gridpositions counts 8 8 8" and lines[2] == "origin -0.750000 0.250000 1.750000"      # 1 - 0.5 * 7 / 2
    assert lines[3:6] == ["delta 0.500000 0 0", "delta 0 0.500000 0", "delta 0 0 0.500000"] and lines[6] == "object 2 class gridconnections counts 8 8 8"
    assert lines[7] == "object 3 class array type double rank 0 items 512 data follows" and lines[8] == "0 1 2" and text.endswith("\n")
    data = [int(v) for ln in lines[8:8 + 171] for v in ln.split()]
    assert data == classes[0].tolist() and lines[8 + 171] == 'attribute "dep" string "positions"' and lines[-4] == 'object "classes" class field'
    with pytest.raises(ValueError, match="classes"):
        plain.to_dx(res, 0, what="labels")
    with pytest.raises(ValueError, match="holds no buried map"):
        plain.to_dx(res, 0, what="buried")


# ------------------------------------------------------------------ header, library, driver
def test_header_declares_the_symbols_and_the_abi_stays_11():
    import physdock_amd
    from physdock_amd import _lib, pocket
    assert physdock_amd.PocketGrid is pocket.PocketGrid
    assert _lib.ABI_VERSION == 11 and "pd_pocket_grid" in set(_lib.header_symbols())
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "physdock_hip.h")).read()
    assert re.search(r"^long long pd_pocket_grid_workspace_numel\(int P, int n, int A\);", hdr, flags=re.M)
    assert int(re.search(r"#define\s+PD_POCKET_MIN_N\s+(\d+)", hdr).group(1)) == pocket.MIN_N == 8
    assert int(re.search(r"#define\s+PD_POCKET_MAX_N\s+(\d+)", hdr).group(1)) == pocket.MAX_N == 48
    assert int(re.search(r"#define\s+PD_POCKET_COUNTS\s+(\d+)", hdr).group(1)) == len(pocket.COUNT_NAMES) == 8
    assert int(re.search(r"#define\s+PD_POCKET_VALUES\s+(\d+)", hdr).group(1)) == len(pocket.VALUE_NAMES) == 6
    src = open(_lib.os.path.join(_lib._HERE, "csrc", "pocket.hip")).read()
    assert "atomicAdd(float" not in src and '#include "geom3.h"' in src and "fp contract(off)" in src
    for text in (hdr, src, pocket.__doc__):
        assert "LIGSITE" in text and re.search(r"heavy atoms only", text, flags=re.I) and re.search(r"not\s+(been\s+)?validated", text, flags=re.I)


def test_the_built_library_exports_and_binds_the_symbols():
    from physdock_amd import _lib
    L = _lib.lib()
    assert L.pd_abi_version() == 11 and hasattr(L, "pd_pocket_grid") and len(_lib.SYMBOLS["pd_pocket_grid"].argtypes) == 34
    numel = L.pd_pocket_grid_workspace_numel
    assert numel(3, 9, 70) == 3 * (2 * 729 + 2 * 81) and numel(1, 33, 5) == 2 * 33 ** 3 + 2 * 33 * 33 * 2 and numel(64, 48, 2048) == 64 * (2 * 48 ** 3 + 4 * 48 * 48)
    assert numel(65535, 48, 1) == 65535 * (2 * 48 ** 3 + 4 * 48 * 48) > 2 ** 31, "a long long"
    assert numel(1, 7, 5) == numel(1, 49, 5) == numel(65536, 9, 5) == -3 and numel(0, 9, 5) == numel(1, 9, 0) == -1


class FakeModel:
    def __init__(self, A):
        self.A = A

    def sample_diffusion(self, batch, **kw):
        n = kw["num_sample"]
        return torch.arange(n, dtype=torch.float32)[:, None, None].expand(n, self.A, 3).clone()


class RecordingPocket:
    n_pose_atoms = 12

    def __init__(self):
        self.seen = []

    def measure(self, x, centre="ligand", maps=True):
        from physdock_amd import driver
        self.seen.append((x.clone(), maps))
        return dict({k: len(self.seen) for k in driver.POCKET_KEYS}, classes="left out", centre="left out")


def test_redock_without_the_keyword_returns_what_it_returned_and_with_it_measures_poses_and_ground_truth(monkeypatch):
    from physdock_amd import driver
    A, T = 12, 5
    batch = {"is_ligand": torch.tensor([0, 0, 0, 0, 1.0]), "atom_id_to_token_id": torch.tensor([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4]),
             "pocket_res_feat": torch.ones(T), "x_gt": torch.full((A, 3), 0.5), "msa_feat": torch.zeros(2, T, 34)}
    monkeypatch.setattr(driver, "weighted_rigid_align", lambda x_gt, x, w: x)
    kw = dict(max_samples=3, num_samples_per_round=5, ranking=False)
    plain = driver.redock(FakeModel(A), batch, **kw)
    assert set(plain) == {"poses", "accepted", "rounds", "gamma_factor", "ranking"}
    rec = RecordingPocket()
    out = driver.redock(FakeModel(A), batch, pocket=rec, **kw)
    assert set(out) == set(plain) | {"pocket", "pocket_gt"} and set(out["pocket"]) == set(driver.POCKET_KEYS) == set(out["pocket_gt"])
    assert out["pocket"]["counts"] == 1 and out["pocket_gt"]["counts"] == 2 and {"counts", "atom_buried", "lining_points", "site_volume"} <= set(driver.POCKET_KEYS)
    assert torch.equal(out["poses"], plain["poses"]) and all(out[k] == plain[k] for k in ("accepted", "rounds", "gamma_factor", "ranking"))
    assert torch.equal(rec.seen[0][0], out["poses"]) and rec.seen[1][0].shape == (1, A, 3) and torch.equal(rec.seen[1][0][0], batch["x_gt"])
    assert rec.seen[0][1] is False and rec.seen[1][1] is False, "the byte maps are not asked for"
    assert set(driver.score_pocket(RecordingPocket(), out["poses"], {})) == {"pocket"}
    many = driver.redock_many(FakeModel(A), [(batch, {"pocket": RecordingPocket()}), batch], **kw)
    assert set(many[0]) == set(out) and set(many[1]) == set(plain)
    other = RecordingPocket()
    other.n_pose_atoms = 13
    sampled = []
    model = FakeModel(A)
    model.sample_diffusion = lambda *a, **k: sampled.append(1)
    with pytest.raises(ValueError, match="pocket= was built over 13 pose atoms, the batch holds 12"):
        driver.redock(model, batch, pocket=other, **kw)
    with pytest.raises(ValueError, match="pocket= takes a pocket.PocketGrid"):
        driver.redock(model, batch, pocket=object(), **kw)
    assert not sampled, "raised before anything was sampled"
    with pytest.raises(TypeError):
        driver._RedockState(batch, batch, pockets=rec)
    assert driver._RedockState(batch, batch, pocket=rec).pocket is rec
