"""The buried-surface measure without a GPU: the float64 restatement (tests/sasa_ref.py) on an isolated atom and on two spheres against
the analytic cap, the point table, the host tables of physdock_amd/surface.py, the argument checks, describe, the header, the keyword
plumbing of redock - and the condition the GPU tests rest on: every seeded case of tests/sasa_ref.py is closed, no flag of any point
differs between the covering radii moved by -MARGIN and +MARGIN (one `OPEN | ...` line per case, pytest -s)."""
import re

import numpy as np
import pytest
import torch

import sasa_ref as ref


def case_of(x, elements, lig_idx, n_points, **kw):
    A = len(elements)
    c = dict(x=np.asarray(x, dtype=np.float64)[None], elements=np.asarray(elements), radius=ref.radii_of(elements), lig_idx=np.asarray(lig_idx),
             lig_active=np.ones(len(lig_idx)), receptor_mask=np.ones(A), a_mask=np.ones(A), polar=np.zeros(len(lig_idx)),
             residue_of=np.zeros(A, dtype=np.int64), n_residues=1, probe=ref.PROBE, n_points=n_points)
    c["receptor_mask"][np.asarray(lig_idx)] = 0
    c.update(kw)
    return c


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n", [1, 96, 960])
def test_an_isolated_atom_is_fully_exposed(n):
    c = case_of([[3.0, -2.0, 7.0], [40.0, 0.0, 0.0]], [6, 8], [0], n)
    r = ref.restate(c)
    assert r["open_flags"] == 0 and r["n_free"].tolist() == [[n, n]] and r["n_bound"].tolist() == [[n, n]] and r["n_buried"].tolist() == [[0, 0]]
    a = ref.areas(c, r["n_free"][:, [0]], r["n_buried"])
    assert a["ligand_free"][0][0] == pytest.approx(4 * np.pi * (1.7 + 1.4) ** 2, rel=1e-6)      # the fp32 radius 1.7 is not 1.7
    assert a["ligand_buried"][0][0] == 0 and a["buried_fraction"][0][0] == 0 and a["interface_residues"][0] == 0


@pytest.mark.parametrize("n,allowed", [(96, 4.0), (960, 10.0)])
def test_two_spheres_against_the_analytic_cap(n, allowed):
    """a sphere of radius a = 3.1 (a carbon + probe) cut by one of radius b = 3.0 (a nitrogen + probe) at centre distance d: the
    covered fraction is (1 - cos) / 2 with cos = (d^2 + a^2 - b^2) / (2 a d); 400 draws of d and of the direction.  Measured with the
    restatement when the bounds were set: worst deviation 2.7 points at n = 96 and 6.6 at n = 960; the assertion is 1.5 x that, because
    the sweep is a sample (this seeded sweep: 3.2 and 5.7, the CAP line of pytest -s)."""
    rng = np.random.default_rng(1973)
    a, b = float(np.float32(1.7)) + ref.PROBE, float(np.float32(1.6)) + ref.PROBE
    worst = 0.0
    for _ in range(400):
        d = rng.uniform(abs(a - b) + 0.05, a + b + 0.3)
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        c = case_of([rng.uniform(-5, 5, 3), [0, 0, 0]], [6, 7], [0], n)
        c["x"][0, 1] = c["x"][0, 0] + d * v
        same, other = ref.flags(c["x"][0], ref.classes(c), c["radius"], c["probe"], n)
        assert not same.any()
        cos = (d * d + a * a - b * b) / (2 * a * d)
        want = n * (1 - min(max(cos, -1.0), 1.0)) / 2 if d < a + b else 0.0
        worst = max(worst, abs(other[0].sum() - want))
    print(f"CAP | n {n} | worst deviation {worst:.2f} points | allowed {allowed} |")
    assert worst <= allowed


def test_counts_follow_the_definition_on_three_atoms():
    # a ligand carbon between a receptor carbon (close) and a second ligand atom: same and other are told apart, the index excludes
    c = case_of([[0, 0, 0], [2.5, 0, 0], [-2.0, 0, 0]], [6, 6, 8], [0, 2], 96)
    r = ref.restate(c)
    same, other = ref.flags(c["x"][0], ref.classes(c), c["radius"], c["probe"], 96)
    assert same[0].any() and other[0].any() and not same[1].any() and other[1].any()
    assert r["n_free"][0, 0] == (~same[0]).sum() and r["n_bound"][0, 0] == (~same[0] & ~other[0]).sum()
    assert (r["n_buried"] == r["n_free"] - r["n_bound"]).all() and (r["n_buried"] >= 0).all()
    # two atoms at the same place with different radii: the larger covers every point of the smaller, the smaller none of the larger
    t = case_of([[0, 0, 0], [0, 0, 0]], [6, 8], [0], 96)
    rt = ref.restate(t)
    assert rt["open_flags"] == 0 and rt["n_bound"].tolist() == [[96, 0]] and rt["n_buried"].tolist() == [[0, 96]]
    # an ignored atom covers nothing and reports nothing
    g = case_of([[0, 0, 0], [2.5, 0, 0]], [6, 6], [0], 96, a_mask=np.array([1, 0]))
    assert ref.restate(g)["n_bound"].tolist() == [[96, 0]]


def test_sphere_points_equal_the_restated_formula():
    from physdock_amd.surface import sphere_points
    for n in (1, 2, 96, 257, 960, 1024):
        u = sphere_points(n)
        assert u.dtype == np.float32 and u.shape == (n, 3)
        assert np.array_equal(u, ref.sphere_points(n).astype(np.float32))
        assert np.abs(np.linalg.norm(u.astype(np.float64), axis=1) - 1).max() < 2e-7
    k, n = 5, 96
    t = k + 0.5
    z = 1 - 2 * t / n
    phi = t * np.pi * (3 - np.sqrt(5))
    assert np.allclose(ref.sphere_points(n)[k], [np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], rtol=0, atol=1e-15)
    assert abs(sphere_points(96).astype(np.float64).sum(0)).max() < 1.0       # spread over the sphere: the mean vector is small
    for bad in (0, 1025, -3):
        with pytest.raises(ValueError, match="points"):
            sphere_points(bad)


# ------------------------------------------------------------------ the condition on the seeds
@pytest.mark.parametrize("name", list(ref.CASES))
def test_every_seeded_case_is_closed(name):
    c = ref.make_case(name)
    r = ref.restate(c)
    bound = ref.distance_error_bound(c)
    lig = c["lig_idx"]
    a = ref.areas(c, r["n_free"][:, lig], r["n_buried"])
    print(f"OPEN | {name} | flags {r['n_flags']} | open {r['open_flags']} | distance bound {bound:.2e} A | buried fraction "
          f"{np.round(a['buried_fraction'][0], 3).tolist()} |")
    assert r["open_flags"] == 0, "a committed seed puts a point within MARGIN of a covering sphere"
    assert bound < ref.MARGIN / 10 and np.abs(c["x"]).max() <= 64.0 and c["radius"].max() + c["probe"] <= 3.6
    assert c["x"].dtype == np.float32 and (r["n_buried"] >= 0).all() and (r["n_free"] <= c["n_points"]).all()


def test_the_cases_reach_what_they_are_there_for():
    frac = {}
    for name in ref.CASES:
        c = ref.make_case(name)
        r = ref.restate(c)
        frac[name] = ref.areas(c, r["n_free"][:, c["lig_idx"]], r["n_buried"])["buried_fraction"][0]
        if name.startswith("f_"):
            cls = ref.classes(c)
            assert cls[ref.F_HOLE] == 0 and cls[c["lig_idx"][ref.F_INACTIVE]] == 0 and cls[ref.F_FAR] == 1 and (cls[list(ref.F_TWIN)] == 1).all()
            assert (r["n_buried"][:, ref.F_FAR] == 0).all() and (r["n_free"][:, ref.F_FAR] == c["n_points"]).all()
            assert np.array_equal(c["x"][:, ref.F_TWIN[0]], c["x"][:, ref.F_TWIN[1]]) and c["radius"][ref.F_TWIN[0]] != c["radius"][ref.F_TWIN[1]]
            assert (r["n_free"][:, ref.F_TWIN[1]] == 0).all(), "the oxygen lies inside the carbon's sphere"
            assert (r["n_buried"][:, cls == 1] > 0).any()
        if name.startswith("g_"):
            x, i = c["x"][0].astype(np.float64), int(c["lig_idx"][0])
            R = c["radius"].astype(np.float64) + c["probe"]
            reach = np.linalg.norm(x - x[i], axis=1) < R + R[i]
            reach[i] = False
            assert reach.sum() == ref.LIST + 5 and reach[:256].all() and reach[520:525].all() and c["x"].shape[1] > 512
            assert r["n_bound"][0, i] == 0 and r["n_free"][0, i] == c["n_points"]
    assert (frac["e_P3_A70_L9_n96_rim"] > 0.3).all() and (frac["e_P3_A70_L9_n96_rim"] < 0.8).all(), "a half-exposed ligand"
    assert (frac["a_P3_A70_L9_n96"] > 0.9).all() and (frac["d_P3_A70_L1_n96"] == 1.0).all()
    assert [ref.CASES[k][3] for k in ref.CASES][:3] == [96, 257, 1] and ref.CASES["d_P3_A70_L1_n96"][2] == (69,)


# ------------------------------------------------------------------ host tables
def surface_of(c, **kw):
    from physdock_amd.surface import BuriedSurface
    return BuriedSurface.from_arrays(c["elements"], c["lig_idx"], c["receptor_mask"], c["residue_of"], n_residues=c["n_residues"],
                                     a_mask=c["a_mask"], ligand_active=c["lig_active"], probe=c["probe"], n_points=c["n_points"], **kw)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_the_tables_of_the_seeded_cases(name):
    c = ref.make_case(name)
    s = surface_of(c)
    start, atom = ref.csr(c)
    assert np.array_equal(s.cls, ref.classes(c)) and s.cls.dtype == np.uint8
    assert np.array_equal(s.radius, c["radius"]) and s.radius.dtype == np.float32
    assert np.array_equal(s.polar, c["polar"]) and np.array_equal(s.ligand_idx, c["lig_idx"])
    assert np.array_equal(s.res_start, start) and np.array_equal(s.res_atom, atom) and s.res_start.dtype == s.res_atom.dtype == np.int32
    assert np.array_equal(s.unit, ref.sphere_points(c["n_points"]).astype(np.float32))
    assert (s.n_atoms, s.n_pose_atoms, s.n_residues, s.n_receptor_atoms) == (len(c["lig_idx"]), c["x"].shape[1], c["n_residues"], len(atom))
    assert s.probe == ref.PROBE and s.n_points == c["n_points"]


def test_masks_inactive_atoms_polar_radii_and_the_csr():
    from physdock_amd import surface, validity
    from physdock_amd.surface import BuriedSurface as S
    assert surface.DEFAULT_PROBE == ref.PROBE and surface.DEFAULT_POINTS == ref.DEFAULT_POINTS == 96 and surface.MAX_POINTS == 1024
    assert validity.VDW_RADII == ref.VDW_RADII and validity.DEFAULT_RADIUS == ref.DEFAULT_RADIUS and surface.TOTAL_NAMES == ref.TOTAL_NAMES
    #            atom 0  1  2  3  4  5   6  7  8  9
    elements = [6, 7, 8, 1, 16, 30, 6, 7, 8, 6]
    residue_of = [2, 0, 2, 4, 0, 3, 3, 2, 1, 1]
    s = S.from_arrays(elements, [7, 8, 9], [1, 1, 1, 1, 1, 0, 1, 1, 1, 1], residue_of, n_residues=6, a_mask=[1, 0, 1, 1, 1, 1, 1, 1, 1, 1],
                      ligand_active=[1, 1, 0])
    # atom 1 does not exist, atom 3 is a hydrogen, atom 5 is not in the receptor mask; ligand atoms never count as receptor
    assert s.cls.tolist() == [1, 0, 1, 0, 1, 0, 1, 2, 2, 0]
    assert s.polar.tolist() == [1, 1, 0], "N and O are polar by default"
    assert np.array_equal(s.radius, np.float32([1.7, 1.6, 1.55, 1.2, 1.8, 2.0, 1.7, 1.6, 1.55, 1.7]))
    assert s.res_start.tolist() == [0, 1, 1, 3, 4, 4, 4] and s.res_atom.tolist() == [4, 0, 2, 6]
    assert (s.n_atoms, s.n_pose_atoms, s.n_residues, s.n_receptor_atoms, s.n_points, s.probe) == (3, 10, 6, 4, 96, 1.4)
    assert "BuriedSurface(n_atoms=3, n_pose_atoms=10, residues=6, receptor_atoms=4, active_ligand_atoms=2, probe=1.4, n_points=96)" == repr(s)
    over = S.from_arrays(elements, [7, 8, 9], np.ones(10), residue_of, radii={6: 1.9, 30: 1.4}, polar=[0, 0, 1], probe=1.2, n_points=960)
    assert np.array_equal(over.radius, np.float32([1.9, 1.6, 1.55, 1.2, 1.8, 1.4, 1.9, 1.6, 1.55, 1.9])) and over.polar.tolist() == [0, 0, 1]
    assert over.probe == 1.2 and over.unit.shape == (960, 3) and over.n_residues == 5 and over.cls.tolist() == [1, 1, 1, 0, 1, 1, 1, 2, 2, 2]
    given = S.from_arrays(None, [7, 8, 9], np.ones(10), residue_of, radius=np.full(10, 1.5), polar=[1, 0, 0])
    assert np.array_equal(given.radius, np.full(10, 1.5, np.float32)) and given.cls.tolist() == [1] * 7 + [2] * 3
    # an all-inactive ligand and a system without receptor atoms are valid
    none = S.from_arrays(elements, [7, 8, 9], np.zeros(10), residue_of, ligand_active=[0, 0, 0])
    assert not none.cls.any() and none.n_receptor_atoms == 0 and none.res_start.tolist() == [0] * 6


def test_from_batch_takes_tokens_as_residues():
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.surface import BuriedSurface
    from physdock_amd.synthetic import make_batch, pdb_meta
    batch = make_batch(20, 4, 9, 4, seed=6)
    is_lig = ligand_atom_mask(batch).numpy()
    T = int(batch["is_ligand"].shape[0])
    s = BuriedSurface.from_batch(batch)
    z = (batch["ref_feat"][:, 4:132].argmax(-1) + 1).numpy()
    assert s.n_residues == T and s.residue_labels is None and np.array_equal(s.ligand_idx, np.nonzero(is_lig)[0])
    assert np.array_equal(s.cls == 2, is_lig & (z != 1)) and np.array_equal(s.cls == 1, ~is_lig & (z != 1))
    assert np.array_equal(s.radius, ref.radii_of(z)) and np.array_equal(s.polar, np.isin(z[is_lig], (7, 8)).astype(np.uint8))
    assert np.array_equal(s.residue_of, batch["atom_id_to_token_id"].numpy())
    assert (np.diff(s.res_start)[batch["is_ligand"].numpy() > 0] == 0).all(), "the ligand's tokens own no receptor atom"
    meta = pdb_meta({k: batch[k].numpy() for k in ("token_id_to_chunk_sizes", "asym_id", "is_ligand", "residue_index")})
    named = BuriedSurface.from_batch(batch, infer_meta_data=meta, n_points=257, probe=1.2)
    assert len(named.residue_labels) == T and named.residue_labels[0] and named.n_points == 257 and named.probe == 1.2
    masked = BuriedSurface.from_batch(dict(batch, a_mask=torch.cat([torch.zeros(1), torch.ones(len(z) - 1)])))
    assert masked.cls[0] == 0 and np.array_equal(masked.cls[1:], s.cls[1:])


def test_constructor_argument_errors():
    from physdock_amd.surface import BuriedSurface as S
    ok = dict(elements=[6] * 8, ligand_idx=[1], receptor_mask=np.ones(8), residue_of=[0, 0, 1, 1, 2, 2, 3, 3])
    S.from_arrays(**ok)
    for change, match in ((dict(ligand_idx=[1, 1]), "distinct"), (dict(ligand_idx=[8]), "distinct"), (dict(elements=[6] * 7), "elements for 7"),
                          (dict(residue_of=[0] * 7), "residue_of 7"), (dict(residue_of=[0, 0, 1, 1, 2, 2, 3, -1]), "residue_of must lie"),
                          (dict(n_residues=3), "residue_of must lie"), (dict(n_residues=9), "at most one residue per atom"),
                          (dict(ligand_active=[1, 1]), "ligand_active 2"), (dict(a_mask=np.ones(9)), "a_mask 9"), (dict(polar=[1, 0]), "polar 2"),
                          (dict(n_points=0), "n_points = 0"), (dict(n_points=1025), "n_points = 1025"), (dict(probe=-0.1), "probe"),
                          (dict(probe=float("nan")), "probe"), (dict(radii={6: -1.0}), "finite and positive"),
                          (dict(radius=np.ones(7)), "radius for 7"), (dict(radius=np.ones(8), radii={6: 1.0}), "cannot be combined"),
                          (dict(elements=None), "elements or radius"), (dict(elements=None, radius=np.ones(8)), "polar bytes must be given"),
                          (dict(residue_labels=["A", "B"]), "residue labels")):
        with pytest.raises(ValueError, match=match):
            S.from_arrays(**{**ok, **change})
    with pytest.raises(ValueError, match="ligand atoms"):
        S.from_arrays([6] * 2000, np.arange(1025), np.ones(2000), np.zeros(2000))
    s = S.from_arrays(**ok)
    with pytest.raises(ValueError, match=r"8 pose atoms, x_pred has shape \(2, 7, 3\)"):
        s.measure(torch.zeros(2, 7, 3))
    with pytest.raises(ValueError, match="pose atoms"):
        s.measure(torch.zeros(8, 3))


def test_describe_sorts_by_area():
    from physdock_amd.surface import BuriedSurface as S
    ok = dict(elements=[6] * 8, ligand_idx=[1], receptor_mask=np.ones(8), residue_of=[0, 0, 1, 1, 2, 2, 3, 3])
    plain = S.from_arrays(**ok)
    assert plain.describe(np.array([0.0, 5.5, 12.25, 5.5])) == [(2, 12.25), (1, 5.5), (3, 5.5)]
    assert plain.describe(torch.tensor([0.0, 5.5, 12.25, 5.5]), min_area=6.0) == [(2, 12.25)] and plain.describe(np.zeros(4)) == []
    named = S.from_arrays(**ok, residue_labels=["LIG:C1", "ASP25", "", "LYS83"])
    assert named.describe(np.array([1.0, 3.0, 2.0, 4.0]), min_area=1.0) == [("LYS83", 4.0), ("ASP25", 3.0), (2, 2.0)]
    with pytest.raises(ValueError, match="a row holds 4 areas, got 5"):
        named.describe(np.zeros(5))


# ------------------------------------------------------------------ header, library, driver
def test_header_declares_the_launcher_and_the_abi_stays_11():
    import physdock_amd
    from physdock_amd import _lib, surface
    assert physdock_amd.BuriedSurface is surface.BuriedSurface
    assert _lib.ABI_VERSION == 11 and "pd_buried_surface" in set(_lib.header_symbols())
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "physdock_hip.h")).read()
    assert int(re.search(r"#define\s+PD_SASA_MAX_POINTS\s+(\d+)", hdr).group(1)) == surface.MAX_POINTS == 1024
    assert int(re.search(r"#define\s+PD_SASA_LIST\s+(\d+)", hdr).group(1)) == ref.LIST
    assert int(re.search(r"#define\s+PD_SASA_TOTALS\s+(\d+)", hdr).group(1)) == len(surface.TOTAL_NAMES) == 8
    src = open(_lib.os.path.join(_lib._HERE, "csrc", "sasa.hip")).read()
    assert "fmaf(dz, dz, fmaf(dy, dy, dx * dx))" in src and "atomic" not in src.split("#include")[1]
    for text in (hdr, src, surface.__doc__):
        assert "Shrake" in text and re.search(r"heavy atoms only", text, flags=re.I) and re.search(r"not\s+(been\s+)?validated", text, flags=re.I)


def test_the_built_library_exports_and_binds_the_launcher():
    from physdock_amd import _lib
    L = _lib.lib()
    assert L.pd_abi_version() == 11 and hasattr(L, "pd_buried_surface") and len(_lib.SYMBOLS["pd_buried_surface"].argtypes) == 23


class FakeModel:
    def __init__(self, A):
        self.A = A

    def sample_diffusion(self, batch, **kw):
        n = kw["num_sample"]
        return torch.arange(n, dtype=torch.float32)[:, None, None].expand(n, self.A, 3).clone()


class RecordingSurface:
    def __init__(self):
        self.seen = []

    def measure(self, x):
        self.seen.append(x.clone())
        return {"tag": len(self.seen)}


def test_redock_without_the_keyword_returns_what_it_returned_and_with_it_measures_poses_and_ground_truth(monkeypatch):
    from physdock_amd import driver
    A, T = 12, 5
    batch = {"is_ligand": torch.tensor([0, 0, 0, 0, 1.0]), "atom_id_to_token_id": torch.tensor([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4]),
             "pocket_res_feat": torch.ones(T), "x_gt": torch.full((A, 3), 0.5), "msa_feat": torch.zeros(2, T, 34)}
    monkeypatch.setattr(driver, "weighted_rigid_align", lambda x_gt, x, w: x)
    kw = dict(max_samples=3, num_samples_per_round=5, ranking=False)
    plain = driver.redock(FakeModel(A), batch, **kw)
    assert set(plain) == {"poses", "accepted", "rounds", "gamma_factor", "ranking"}
    rec = RecordingSurface()
    out = driver.redock(FakeModel(A), batch, surface=rec, **kw)
    assert set(out) == set(plain) | {"surface", "surface_gt"} and out["surface"] == {"tag": 1} and out["surface_gt"] == {"tag": 2}
    assert torch.equal(out["poses"], plain["poses"]) and all(out[k] == plain[k] for k in ("accepted", "rounds", "gamma_factor", "ranking"))
    assert torch.equal(rec.seen[0], out["poses"]) and rec.seen[1].shape == (1, A, 3) and torch.equal(rec.seen[1][0], batch["x_gt"])
    no_gt = driver.score_surface(RecordingSurface(), out["poses"], {})
    assert set(no_gt) == {"surface"}
    many = driver.redock_many(FakeModel(A), [(batch, {"surface": RecordingSurface()}), batch], **kw)
    assert set(many[0]) == set(out) and set(many[1]) == set(plain)
    with pytest.raises(TypeError):
        driver._RedockState(batch, batch, surfaces=rec)
    assert driver._RedockState(batch, batch, surface=rec).surface is rec
