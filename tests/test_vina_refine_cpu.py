"""VinaRefine on the host: the torsion table and the intramolecular pair list of physdock_amd/refine.py against the rules and
against the restatement tests/vina_refine_ref.py, argument validation, and the restatement itself - its gradients against central
differences, `move` as an isometry of every rigid fragment, its `inter` against tests/vina_ref.py, the minimiser's descent, and the
conditioning guard of the GPU trajectory test: the reference run with reversed summation order must end within 1e-8 A of itself
with the same counts, at max_iters 3 and 20 (a condition on the seeded inputs, not a tolerance on the kernel).

Central differences: the error of (E(h) - E(-h)) / 2h is h^2 |E'''| / 6 + u |E| / h.  The stiffest term is gauss1, exp(-(d / 0.5)^2)
with |t'''| <= 8 * 4.2 / 0.5 = 67 (the maximum of |H_3(q)| exp(-q^2) is 4.2 in q = d / 0.5, times 1 / 0.5^3), weight 0.0356; at
most 40 pairs of one atom lie in the gaussian's range and a coordinate moves an atom by at most LEVER = 8 A per radian, so
|E'''| <= 0.0356 * 67 * 40 * 8^3 =: D3.  The step is h = 1e-5: an atom moves by at most 8e-5 A, less than the 1e-4 A every pair keeps
from the cutoff and the kinks, so no pair changes its branch inside the stencil; the truncation is h^2 D3 / 6 = 8.1e-7 and the
rounding 2^-53 * 10 / h = 1.1e-10 (|E| < 10).  FD_TOL is their sum."""
import numpy as np
import pytest

import vina_ref
import vina_refine_ref as ref

H_FD = 1e-5
LEVER = 8.0
D3 = 0.0356 * 67.0 * 40.0 * LEVER ** 3
FD_TOL = H_FD ** 2 * D3 / 6.0 + 2.0 ** -53 * 10.0 / H_FD


@pytest.fixture(scope="module")
def cases():
    return {name: ref.make_case(name) for name in ref.CASES}


def pose(c, p):
    xp = c["x"][p].astype(np.float64)
    return xp, xp[c["lig_idx"]]


# ------------------------------------------------------------------ tables
def test_ring_bonds_are_excluded_and_the_count_matches():
    from physdock_amd.refine import rotatable_bonds
    from physdock_amd.scoring import count_rotatable_bonds
    ligands = [(12, ref.LIG12_BONDS, None), (5, ref.LIG6_BONDS[:4], None), (4, [(0, 1), (1, 2), (2, 3)], None),
               (6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)], [1, 1, 3, 1, 1]), (5, [(0, 1), (1, 2), (2, 3), (3, 4)], [1, 2, 1, 1]),
               (1, [], None), (7, [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 5), (5, 6), (6, 4)], None)]
    for n, bonds, orders in ligands:
        rot = rotatable_bonds(n, bonds, orders)
        assert len(rot) == count_rotatable_bonds(n, bonds, orders), (n, bonds)
        assert rot == ref.rotatable_bonds(n, bonds, orders)
    assert rotatable_bonds(12, ref.LIG12_BONDS) == [(0, 6), (6, 7), (3, 10)]          # no ring bond, no bond to a terminal atom
    assert rotatable_bonds(6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)], [1, 1, 3, 1, 1]) == []
    assert rotatable_bonds(7, ligands[-1][1]) == [(2, 3), (3, 4)]                       # the bridge between two three-rings


def test_the_smaller_side_moves_and_a_tie_goes_to_the_higher_index():
    from physdock_amd.refine import torsion_table
    rot, sets, mask = torsion_table(12, ref.LIG12_BONDS, [(0, 6), (6, 7), (3, 10)])
    assert rot.tolist() == [[0, 6], [6, 7], [3, 10]] and [s.tolist() for s in sets] == [[6, 7, 8, 9], [7, 8, 9], [10, 11]]
    assert mask.dtype == np.uint32 and mask.shape == (3, 1) and mask[:, 0].tolist() == [0b1111000000, 0b1110000000, 0b110000000000]
    # a chain of four: the middle bond splits it 2 : 2, the side with atom 3 moves; given the other way round it is turned
    for bond in ((1, 2), (2, 1)):
        rot, sets, _ = torsion_table(4, [(0, 1), (1, 2), (2, 3)], [bond])
        assert rot.tolist() == [[1, 2]] and sets[0].tolist() == [2, 3]
    # the smaller side moves even when it holds the lower indices
    rot, sets, _ = torsion_table(6, ref.LIG6_BONDS, [(1, 2)])
    assert rot.tolist() == [[2, 1]] and sets[0].tolist() == [0, 1]
    # more than 32 atoms: the mask's second word
    chain = [(i, i + 1) for i in range(39)]
    rot, sets, mask = torsion_table(40, chain, [(33, 34)])
    assert rot.tolist() == [[33, 34]] and mask.shape == (1, 2) and mask[0].tolist() == [0, 0b11111100]
    with pytest.raises(ValueError, match="ring"):
        torsion_table(3, [(0, 1), (1, 2), (2, 0)], [(0, 1)])


def test_the_intra_list_holds_exactly_the_pairs_more_than_three_bonds_apart():
    from physdock_amd.refine import intra_pairs
    n, bonds = 12, ref.LIG12_BONDS
    dist = np.full((n, n), np.inf)
    np.fill_diagonal(dist, 0)
    for i, j in bonds:
        dist[i, j] = dist[j, i] = 1
    for k in range(n):                                                              # Floyd - Warshall
        dist = np.minimum(dist, dist[:, k:k + 1] + dist[k:k + 1, :])
    want = [(i, j) for i in range(n) for j in range(i + 1, n) if dist[i, j] > 3]
    assert intra_pairs(n, bonds).tolist() == [list(p) for p in want] and len(want) == 26
    active = np.ones(n, dtype=bool)
    active[8] = False
    assert intra_pairs(n, bonds, active).tolist() == [list(p) for p in want if 8 not in p]
    assert intra_pairs(3, [(0, 1)]).tolist() == [[0, 2], [1, 2]]                      # another component
    assert intra_pairs(1, []).shape == (0, 2)


def vina_refine_of(c, device=None):
    from physdock_amd.refine import VinaRefine
    from physdock_amd.scoring import VinaScore
    v = VinaScore.from_types(c["types"], c["lig_idx"], c["rec_mask"], c["n_rot"], ligand_active=c["lig_active"], device=device)
    return VinaRefine.from_vina(v, c["bonds"], device=device)


def test_the_package_builds_the_tables_of_the_restatement(cases):
    for name, c in cases.items():
        r = vina_refine_of(c)
        assert r.n_torsions == len(c["rot"]) == int(c["n_rot"]) and r.n_atoms == len(c["lig_idx"])
        assert np.array_equal(r.rot, c["rot"]) and np.array_equal(r.rot_mask, c["mask"]) and np.array_equal(r.intra, c["intra"]), name
        assert all(np.array_equal(a, b) for a, b in zip(r.moving, c["sets"]))
        # the neighbour lists are the pair list seen from both atoms
        pairs = {(i, int(j)) for i in range(r.n_atoms) for j in r.intra_atom[r.intra_start[i]:r.intra_start[i + 1]]}
        assert pairs == {tuple(p) for p in c["intra"].tolist()} | {tuple(p[::-1]) for p in c["intra"].tolist()}
        assert r.intra_start[-1] == 2 * len(c["intra"]) == len(r.intra_atom)
    c = cases["P2_A257_L6_T2"]
    assert c["lig_active"][5] == 0 and 5 in c["sets"][1] and c["rot"].tolist() == [[2, 1], [2, 3]]      # the hydrogen moves with its side


def test_argument_validation(cases):
    from physdock_amd.refine import MAX_TORSIONS, VinaRefine
    from physdock_amd.scoring import VinaScore
    c = cases["P2_A257_L6_T2"]
    v = VinaScore.from_types(c["types"], c["lig_idx"], c["rec_mask"], 2.0, ligand_active=c["lig_active"])
    with pytest.raises(ValueError, match="leaves the 6 atoms"):
        VinaRefine.from_vina(v, [(0, 6)])
    with pytest.raises(ValueError, match="bond orders"):
        VinaRefine.from_vina(v, c["bonds"], [1.0])
    # a comb of 62 backbone atoms, each with a side atom: 61 rotatable bonds
    n = 62
    bonds = [(i, i + 1) for i in range(n - 1)] + [(i, n + i) for i in range(n)]
    A = 2 * n + 1
    big = VinaScore.from_types(np.zeros(A, dtype=np.uint8), np.arange(2 * n), np.r_[np.zeros(2 * n), 1], 0.0)
    with pytest.raises(ValueError, match=f"up to {MAX_TORSIONS}"):
        VinaRefine.from_vina(big, bonds)
    r = VinaRefine.from_vina(v, c["bonds"])
    import torch
    for bad in (dict(max_iters=-1), dict(grad_tol=-1.0), dict(max_step=0.0), dict(grad_tol=float("nan"))):
        with pytest.raises(ValueError, match="VinaRefine.refine"):
            r.refine(torch.zeros(1, 257, 3), **bad)
    with pytest.raises(ValueError, match="pose atoms"):
        r.energy(torch.zeros(1, 256, 3))
    rigid = VinaRefine.from_vina(VinaScore.from_types(c["types"], c["lig_idx"][:1], c["rec_mask"], 0.0), [])
    assert rigid.n_torsions == 0 and rigid.rot.shape == (0, 2) and len(rigid.intra) == 0                 # L = 1 is legal


def test_abi_version_and_symbols():
    from physdock_amd import VinaRefine, _lib  # noqa: F401
    assert _lib.ABI_VERSION == 11
    new = {"pd_vina_refine", "pd_vina_refine_energy", "pd_vina_refine_workspace_numel"}
    assert new <= set(_lib.header_symbols())
    L = _lib.lib()
    assert new <= set(_lib.SYMBOLS) and all(hasattr(L, s) for s in new)
    assert L.pd_vina_refine_workspace_numel(3, 12, 3) == 3 * (81 + 36)
    assert L.pd_vina_refine_workspace_numel(1, 1025, 0) == -3 and L.pd_vina_refine_workspace_numel(1, 12, 59) == -3
    assert L.pd_vina_refine_workspace_numel(0, 12, 3) == -1


# ------------------------------------------------------------------ the restatement
def test_the_cases_are_the_shapes_that_take_every_path(cases):
    shapes = {name: (c["x"].shape[0], c["x"].shape[1], len(c["lig_idx"]), len(c["rot"])) for name, c in cases.items()}
    assert shapes == {"P3_A300_L12_T3": (3, 300, 12, 3), "P2_A257_L6_T2": (2, 257, 6, 2), "P2_A65_L1_T0": (2, 65, 1, 0),
                      "P2_A300_L12_far": (2, 300, 12, 3)}
    lig = cases["P3_A300_L12_T3"]["lig_idx"]
    assert 299 in lig and (lig >= 256).any() and np.diff(lig).max() > 1
    for name, c in cases.items():
        for p in range(c["x"].shape[0]):
            xp, y = pose(c, p)
            assert ref.evaluate(c, xp, y)["margin"] >= ref.MARGIN, (name, p)
    # pose 0 clashes by 0.5 A, pose 1 touches, pose 2 is 3 A out
    c = cases["P3_A300_L12_T3"]
    lig, rec = c["lig_idx"], np.nonzero(c["rec_mask"])[0]
    rad = ref.RADII[c["types"] & 15]
    gaps = []
    for p in range(3):
        xp, y = pose(c, p)
        gaps.append((np.sqrt(((y[:, None] - xp[rec][None]) ** 2).sum(-1)) - rad[lig][:, None] - rad[rec][None]).min())
    assert abs(gaps[0] + 0.5) < 0.02 and 0.0 <= gaps[1] < 0.3 and 3.0 <= gaps[2] < 3.3, gaps
    # the far case: no pair of any kind inside the cutoff
    c = cases["P2_A300_L12_far"]
    for p in range(2):
        xp, y = pose(c, p)
        ev = ref.evaluate(c, xp, y)
        assert ev["n_pairs"] == 0 and ev["energy"] == 0.0 and not ev["grad"].any() and not ev["ggrad"].any()


def test_inter_is_the_energy_of_vina_ref(cases):
    for name, c in cases.items():
        want = vina_ref.vina(c["x"], c["lig_idx"], c["types"], c["rec_mask"], c["lig_active"], 0.0)
        for p in range(c["x"].shape[0]):
            xp, y = pose(c, p)
            ev = ref.evaluate(c, xp, y)
            scale = np.abs(vina_ref.WEIGHTS * want["terms"][p]).sum()
            assert abs(ev["inter"] - want["inter"][p]) <= 64 * 2.0 ** -53 * max(scale, 1.0), (name, p)
            # the receptor part of the gradient is minus the force of vina_ref
            only_inter = dict(c, intra=np.zeros((0, 2), dtype=np.int32))
            g = ref.evaluate(only_inter, xp, y)["grad"]
            assert np.abs(g + want["forces"][p]).max() <= 1e-12 * max(np.abs(g).max(), 1.0)


def test_gradients_against_central_differences(cases):
    for name, c in cases.items():
        for p in range(c["x"].shape[0]):
            xp, y = pose(c, p)
            ev = ref.evaluate(c, xp, y)
            tol = FD_TOL
            assert ev["margin"] >= LEVER * H_FD and np.abs(y - y.mean(0)).max() <= LEVER or ev["n_pairs"] == 0
            n = 6 + len(c["rot"])
            fd = np.zeros(n)
            for k in range(n):
                e = np.zeros(n)
                e[k] = H_FD
                fd[k] = (ref.evaluate(c, xp, ref.move(c, y, e))["energy"] - ref.evaluate(c, xp, ref.move(c, y, -e))["energy"]) / (2 * H_FD)
            assert np.abs(fd - ev["ggrad"]).max() <= tol, (name, p, np.abs(fd - ev["ggrad"]).max())
            fdc = np.zeros_like(y)
            for i in range(len(y)):
                for a in range(3):
                    yp, ym = y.copy(), y.copy()
                    yp[i, a] += H_FD
                    ym[i, a] -= H_FD
                    fdc[i, a] = (ref.evaluate(c, xp, yp)["energy"] - ref.evaluate(c, xp, ym)["energy"]) / (2 * H_FD)
            assert np.abs(fdc - ev["grad"]).max() <= tol, (name, p, np.abs(fdc - ev["grad"]).max())
            assert not ev["grad"][c["lig_active"] == 0].any()


def test_move_is_an_isometry_of_every_rigid_fragment(cases):
    rng = np.random.default_rng(5)
    for name, c in cases.items():
        L = len(c["lig_idx"])
        _, y = pose(c, 0)
        frag = np.zeros(L, dtype=np.int64)                                           # atoms with the same membership pattern are one fragment
        for k, m in enumerate(c["sets"]):
            frag[m] |= 1 << k
        s = np.concatenate([rng.uniform(-2, 2, 3), rng.uniform(-1.5, 1.5, 3), rng.uniform(-3, 3, len(c["rot"]))])
        z = ref.move(c, y, s)
        same = frag[:, None] == frag[None, :]
        for (a, b) in c["rot"]:                                                       # the two atoms of an axis belong to both sides
            same[a, frag == frag[b]] = same[frag == frag[b], a] = True
        d0, d1 = np.sqrt(((y[:, None] - y[None]) ** 2).sum(-1)), np.sqrt(((z[:, None] - z[None]) ** 2).sum(-1))
        assert np.abs(d1 - d0)[same].max() <= 1e-12, name
        if len(c["rot"]):
            assert np.abs(d1 - d0).max() > 1e-3                                       # ... and the torsions did turn
        assert np.abs(ref.move(c, y, np.zeros_like(s)) - y).max() <= 1e-14
        # a pure translation and a pure rotation
        t = ref.move(c, y, np.r_[1.0, -2.0, 0.5, np.zeros(3 + len(c["rot"]))])
        assert np.abs(t - y - [1.0, -2.0, 0.5]).max() <= 1e-14
        r = ref.move(c, y, np.r_[np.zeros(3), 0.0, 0.0, np.pi / 2, np.zeros(len(c["rot"]))])
        cen = y.mean(0)
        assert np.abs((r - cen)[:, 0] + (y - cen)[:, 1]).max() <= 1e-13 and np.abs((r - cen)[:, 1] - (y - cen)[:, 0]).max() <= 1e-13


@pytest.fixture(scope="module")
def runs(cases):
    """the reference minimiser on every pose of every case at max_iters 3 and 20, forward and with reversed summation order"""
    out = {}
    for name, c in cases.items():
        for mi in (3, 20):
            for p in range(c["x"].shape[0]):
                xp = c["x"][p].astype(np.float64)
                out[name, mi, p] = (ref.refine(c, xp, max_iters=mi), ref.refine(c, xp, max_iters=mi, order=-1))
    return out


def test_the_minimiser_descends(cases, runs):
    for (name, mi, p), (a, _) in runs.items():
        assert (np.diff(a["trace"]) <= 0).all() and a["trace"][0] == a["energy_start"] and a["trace"][-1] == a["energy"], (name, mi, p)
        assert a["energy"] <= a["energy_start"] and a["evaluations"] >= a["iterations"] + 1 and a["iterations"] <= mi
    c = cases["P3_A300_L12_T3"]
    xp, y = pose(c, 0)
    for mi in (3, 20):
        a = runs["P3_A300_L12_T3", mi, 0][0]
        assert a["energy"] < a["energy_start"] and ref.repulsion(c, xp, a["y"]) < ref.repulsion(c, xp, y)
    assert ref.repulsion(c, xp, y) > 0.25                                            # the 0.5 A clash: one pair at d = -0.5
    for p in range(2):
        a = runs["P2_A300_L12_far", 20, p][0]
        xp, y = pose(cases["P2_A300_L12_far"], p)
        assert a["iterations"] == 0 and a["status"] == 0 and a["evaluations"] == 1 and np.array_equal(a["y"], y) and a["moved"] == 0.0
    one = runs["P2_A65_L1_T0", 20, 1][0]
    assert one["status"] == 0 and 0 < one["iterations"] < 20                          # a single atom converges on grad_tol


def test_conditioning_guard(cases, runs):
    """the inputs of the GPU trajectory test are well conditioned: reversing every summation moves no coordinate by 1e-8 A, changes no
    count, and moves the final energy by at most a quarter of the energy bound at the end point (the GPU test holds the device's
    final energy to that bound; a case whose own restatement cannot reproduce it is replaced, not excused)"""
    for (name, mi, p), (a, b) in runs.items():
        c = cases[name]
        bound = ref.evaluate(c, c["x"][p].astype(np.float64), a["y"], bounds=True)["bound"]["energy"]
        assert abs(a["energy"] - b["energy"]) <= 0.25 * bound, (name, mi, p, abs(a["energy"] - b["energy"]), bound)
        assert np.abs(a["y"] - b["y"]).max() <= 1e-8, (name, mi, p, np.abs(a["y"] - b["y"]).max())
        assert (a["iterations"], a["evaluations"], a["status"]) == (b["iterations"], b["evaluations"], b["status"]), (name, mi, p)
