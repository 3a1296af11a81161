"""FlexRefine on the host: the side-chain torsion tables of physdock_amd/flex.py against the chi table and a brute-force graph search,
`select`, the package's tables against the restatement tests/flex_refine_ref.py, the ABI, the driver keyword's argument check, and
the restatement itself - its gradients against central differences, `move` as an isometry of everything bonded, the exclusion
guard of the `excluded` case, the behavioural case, and the conditioning guard of the GPU trajectory test: the reference run with
reversed summation order must end within 1e-8 A of itself with the same counts and reproduce its final energy within a quarter of
the energy bound (a condition on the seeded inputs, not a tolerance on the kernel).

Central differences: the accounting of tests/test_vina_refine_cpu.py (FD_TOL there: h = 1e-5, truncation h^2 D3 / 6 with at most 40
pairs of one atom in the gaussian's range and a lever of 8 A per radian, rounding u |E| / h) - a side-chain atom lies within 8 A of
its chi axes, and the ligand rows within 8 A of their centroid (asserted)."""
import numpy as np
import pytest

import flex_refine_ref as ref
import vina_refine_ref as vrr

H_FD = 1e-5
LEVER = 8.0
D3 = 0.0356 * 67.0 * 40.0 * LEVER ** 3
FD_TOL = H_FD ** 2 * D3 / 6.0 + 2.0 ** -53 * 10.0 / H_FD


@pytest.fixture(scope="module")
def cases():
    return {name: ref.make_case(name) for name in ref.CASES}


def pose(c, p):
    xp = c["x"][p].astype(np.float64)
    return xp, xp[c["mov_idx"]]


# ------------------------------------------------------------------ side-chain torsions by name
ORDER = {"GLY": [], "ALA": ["CB"], "SER": ["CB", "OG"], "CYS": ["CB", "SG"], "VAL": ["CB", "CG1", "CG2"], "THR": ["CB", "OG1", "CG2"],
         "LEU": ["CB", "CG", "CD1", "CD2"], "ILE": ["CB", "CG1", "CG2", "CD1"], "MET": ["CB", "CG", "SD", "CE"], "PRO": ["CB", "CG", "CD"],
         "PHE": ["CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ"], "TYR": ["CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ", "OH"],
         "TRP": ["CB", "CG", "CD1", "CD2", "NE1", "CE2", "CE3", "CZ2", "CZ3", "CH2"], "ASP": ["CB", "CG", "OD1", "OD2"],
         "GLU": ["CB", "CG", "CD", "OE1", "OE2"], "ASN": ["CB", "CG", "OD1", "ND2"], "GLN": ["CB", "CG", "CD", "OE1", "NE2"],
         "HIS": ["CB", "CG", "ND1", "CD2", "CE1", "NE2"], "LYS": ["CB", "CG", "CD", "CE", "NZ"],
         "ARG": ["CB", "CG", "CD", "NE", "CZ", "NH1", "NH2"]}


def peptide(kinds, drop=()):
    """names of a chain of residues, one after the other: (res_names, atom_names, residue_of); drop: (residue, atom name) left out"""
    res, names, rid = [], [], []
    for s, k in enumerate(kinds):
        for a in ["N", "CA", "C", "O"] + ORDER[k]:
            if (s, a) not in drop:
                res.append(k); names.append(a); rid.append(s)
    return res, names, np.asarray(rid)


def test_side_chain_torsions_of_all_twenty_residues():
    from physdock_amd.flex import side_chain_torsions_from_names
    from physdock_amd.receptor_geometry import _CHI, residue_bonds_from_names
    kinds = list(ORDER)
    assert set(kinds) == set(_CHI) and len(kinds) == 20
    res, names, rid = peptide(kinds)
    t = side_chain_torsions_from_names(res, names, rid, range(20))
    none = {"PRO", "GLY", "ALA"}
    assert [kinds[s] for s in t["residues"]] == [k for k in kinds if k not in none]
    assert sorted(t["skipped"]) == sorted((kinds.index(k), "no torsions") for k in none)
    bonds = residue_bonds_from_names(res, names, rid)
    assert np.array_equal(t["bonds"], bonds)
    n = len(names)
    dist = np.full((n, n), np.inf)
    np.fill_diagonal(dist, 0)
    for i, j in bonds:
        dist[i, j] = dist[j, i] = 1
    for k in range(n):
        dist = np.minimum(dist, dist[:, k:k + 1] + dist[k:k + 1, :])
    idx = {(int(r), a): i for i, (r, a) in enumerate(zip(rid, names))}
    for s in t["residues"]:
        k = kinds[s]
        assert len(t["torsions"][s]) == len(_CHI[k]), k                                # one torsion per chi
        chain = ["CA", "CB"] + _CHI[k]
        assert t["torsions"][s] == [(idx[s, chain[j]], idx[s, chain[j + 1]]) for j in range(len(_CHI[k]))], k     # the chis' central bonds
        side = [idx[s, a] for a in ORDER[k]]
        for (a, b), m in zip(t["torsions"][s], t["moving"][s]):
            want = sorted(i for i in side if dist[b, i] < dist[a, i])                 # a tree beyond CA: the atoms nearer to b than to a
            assert m.tolist() == want, (k, names[a], names[b])
            assert a not in m and b in m
        assert t["atoms"][s] == [idx[s, "CA"]] + sorted(side)
    lys = kinds.index("LYS")
    assert [len(m) for m in t["moving"][lys]] == [5, 4, 3, 2]
    phe = kinds.index("PHE")
    assert [len(m) for m in t["moving"][phe]] == [7, 6]                              # chi2 turns the whole ring


def test_missing_atoms_and_a_disulfide_are_skipped():
    from physdock_amd.flex import side_chain_torsions_from_names
    kinds = ["CYS", "LYS", "CYS", "LEU", "SER"]
    res, names, rid = peptide(kinds, drop={(1, "CE"), (4, "CB")})
    sg = [i for i, (r, a) in enumerate(zip(rid, names)) if a == "SG"]
    t = side_chain_torsions_from_names(res, names, rid, [3, 0, 1, 2, 4, 9], extra_bonds=[sg])
    assert t["residues"] == [3]
    assert t["skipped"] == [(0, "ring"), (1, "missing atom"), (2, "ring"), (4, "missing atom"), (9, "no torsions")]
    free = side_chain_torsions_from_names(res, names, rid, [0, 2])                     # without the disulfide both are eligible
    assert free["residues"] == [0, 2] and not free["skipped"]
    # a mask takes an atom away like a missing name does
    m = np.ones(len(names))
    m[[i for i, (r, a) in enumerate(zip(rid, names)) if (r, a) == (3, "CD1")]] = 0
    assert side_chain_torsions_from_names(res, names, rid, [3], mask=m)["skipped"] == [(3, "missing atom")]


def test_select_orders_by_distance_and_cuts_at_the_limit():
    from physdock_amd.flex import SELECT_CUTOFF, FlexRefine
    assert SELECT_CUTOFF == 4.0
    kinds = ["LYS", "ALA", "LEU", "ARG", "SER", "GLY", "MET"]
    res, names, rid = peptide(kinds)
    x = np.zeros((len(names), 3))
    x[:, 0] = 100.0 + 10.0 * np.arange(len(names))                                     # everything far from the ligand and apart
    at = lambda s, a: [i for i, (r, n) in enumerate(zip(rid, names)) if (r, n) == (s, a)][0]
    lig = np.zeros((2, 3))
    x[at(0, "NZ")] = [3.0, 0, 0]                                                       # LYS 3.0, LEU 2.0, ARG 3.9, MET 4.5 (out)
    x[at(2, "CD2")] = [0, 2.0, 0]
    x[at(3, "NH1")] = [0, 0, 3.9]
    x[at(6, "CE")] = [0, 4.5, 0]
    x[at(4, "CB")] = [1.0, 0, 0]                                                       # SER: only CB is close - CB does not count
    x[at(1, "CB")] = [0, 1.0, 0]                                                       # ALA: no torsions
    sel = FlexRefine.select(lig, x, res, names, rid)
    assert sel["residues"] == [2, 0, 3] and sel["cut"] == []
    assert sel["distance"] == {2: 2.0, 0: 3.0, 3: 3.9}
    assert (1, "no torsions") in sel["skipped"] and (5, "no torsions") in sel["skipped"]
    cut = FlexRefine.select(lig, x, res, names, rid, max_torsions=7)                  # LEU 2 + LYS 4 = 6; ARG's 4 do not fit
    assert cut["residues"] == [2, 0] and cut["cut"] == [3]
    assert FlexRefine.select(lig, x, res, names, rid, max_torsions=1) == dict(sel, residues=[], cut=[2, 0, 3])
    wide = FlexRefine.select(lig, x, res, names, rid, cutoff=5.0)
    assert wide["residues"] == [2, 0, 3, 6]
    assert FlexRefine.select(lig, x, res, names, rid, residues=[0, 3])["residues"] == [0, 3]


# ------------------------------------------------------------------ the package's tables
def flex_refine_of(c, device=None):
    from physdock_amd.flex import FlexRefine
    return FlexRefine.from_tables(c["types"], c["lig_idx"], c["rec_mask"], c["lig_active"], c["n_rot"], c["rot"][:c["T"]], c["sets"][:c["T"]],
                                  c["intra"], c["rec_bonds"], c["residues"], device=device)


def test_the_package_builds_the_tables_of_the_restatement(cases):
    for name, c in cases.items():
        f = flex_refine_of(c)
        assert (f.n_atoms, f.n_flex_atoms, f.n_torsions, f.n_flex_torsions) == (c["L"], c["F"], c["T"] + c["S"], c["S"]), name
        for k in ("mov_idx", "fixed_mask", "active", "rot", "pairs", "flex_idx"):
            assert np.array_equal(getattr(f, k), c[k]), (name, k)
        assert np.array_equal(f.rot_mask, c["mask"]) and all(np.array_equal(a, b) for a, b in zip(f.moving, c["sets"]))
        lists = ref.csr(c)
        for k in lists:
            assert np.array_equal(getattr(f, k), lists[k]) and getattr(f, k).dtype == np.int32, (name, k)
        assert all(np.array_equal(a, b) for a, b in zip(f.excl, c["excl"])) and all(np.array_equal(a, b) for a, b in zip(f.residue_rows, c["residue_rows"]))
        assert len(f.describe()) == len(c["residues"]) and f.skipped == ()
    shapes = {n: (c["x"].shape[0], c["L"], c["F"], c["T"], c["S"]) for n, c in cases.items()}
    assert shapes == {"small": (3, 12, 10, 2, 4), "rigid_ligand": (2, 6, 5, 0, 3), "no_flex": (2, 6, 0, 2, 0), "full_chart": (2, 12, 84, 2, 56),
                      "over_block": (2, 12, 292, 2, 2), "excluded": (2, 12, 3, 2, 1), "across": (2, 12, 6, 2, 4)}
    assert cases["full_chart"]["T"] + cases["full_chart"]["S"] == 58 and cases["over_block"]["L"] + cases["over_block"]["F"] > 256
    assert min(len(m) for m in cases["over_block"]["sets"][2:]) >= 144               # few torsions, large moving sets


def test_the_pair_and_exclusion_lists_equal_a_brute_force_graph_search(cases):
    for name in ("small", "full_chart", "excluded", "over_block"):
        c = cases[name]
        A, L, F = c["x"].shape[1], c["L"], c["F"]
        dist = np.full((A, A), np.inf)
        np.fill_diagonal(dist, 0)
        for i, j in c["rec_bonds"]:
            dist[i, j] = dist[j, i] = 1
        for k in range(A):                                                           # Floyd - Warshall
            dist = np.minimum(dist, dist[:, k:k + 1] + dist[k:k + 1, :])
        flex, fixed = c["flex_idx"], c["fixed_mask"] > 0
        assert np.array_equal(fixed, (c["rec_mask"] > 0) & ~np.isin(np.arange(A), flex))
        for k, a in enumerate(flex):
            assert c["excl"][L + k].tolist() == [j for j in range(A) if fixed[j] and dist[a, j] <= 3], (name, k)
        assert all(len(e) == 0 for e in c["excl"][:L])
        want = {tuple(p) for p in c["intra"].tolist()} | {(i, L + k) for i in range(L) if c["active"][i] for k in range(F)}
        want |= {(L + k, L + m) for k in range(F) for m in range(k + 1, F) if dist[flex[k], flex[m]] > 3}
        assert {tuple(p) for p in c["pairs"].tolist()} == want and len(c["pairs"]) == len(want), name
    c = cases["small"]                                                               # a hydrophobic and a donor - acceptor (ligand, flexible) pair in range
    xp, y = pose(c, 0)
    t = c["types"][c["mov_idx"]].astype(int)
    L = c["L"]
    close = [(i, j) for i, j in c["pairs"] if i < L <= j and np.sqrt(((y[i] - y[j]) ** 2).sum()) < 8.0]
    assert any(t[i] & t[j] & 16 for i, j in close) and any((t[i] & 32 and t[j] & 64) or (t[i] & 64 and t[j] & 32) for i, j in close)


def test_argument_validation(cases):
    import torch
    from physdock_amd.flex import FlexRefine
    c = cases["small"]
    f = flex_refine_of(c)
    for bad in (dict(max_iters=-1), dict(grad_tol=-1.0), dict(max_step=0.0), dict(grad_tol=float("nan"))):
        with pytest.raises(ValueError, match="FlexRefine.refine"):
            f.refine(torch.zeros(1, c["x"].shape[1], 3), **bad)
    with pytest.raises(ValueError, match="pose atoms"):
        f.energy(torch.zeros(1, c["x"].shape[1] - 1, 3))
    args = [c["types"], c["lig_idx"], c["rec_mask"], c["lig_active"], c["n_rot"], c["rot"][:2], c["sets"][:2], c["intra"]]
    a, b = c["residues"][0][0]
    with pytest.raises(ValueError, match="ring"):
        tip = [int(i) for i in c["flex_idx"][1:3] if i != b][0]                        # G of the first residue: CA - CB - G - CA
        FlexRefine.from_tables(*args, list(c["rec_bonds"]) + [(tip, a)], c["residues"])
    with pytest.raises(ValueError, match="two residues"):
        FlexRefine.from_tables(*args, c["rec_bonds"], [c["residues"][0], c["residues"][0]])
    holes = c["rec_mask"].copy()
    holes[b] = 0
    with pytest.raises(ValueError, match="rec_mask"):
        FlexRefine.from_tables(c["types"], c["lig_idx"], holes, *args[3:], c["rec_bonds"], c["residues"])
    big = cases["full_chart"]
    with pytest.raises(ValueError, match="up to 58"):
        FlexRefine.from_tables(big["types"], big["lig_idx"], big["rec_mask"], big["lig_active"], 3.0, vrr.tables(12, vrr.LIG12_BONDS)["rot"],
                               vrr.tables(12, vrr.LIG12_BONDS)["sets"], big["intra"], big["rec_bonds"], big["residues"])


def test_abi_version_and_symbols():
    from physdock_amd import FlexRefine, _lib  # noqa: F401
    assert _lib.ABI_VERSION == 11
    new = {"pd_vina_flex_refine", "pd_vina_flex_energy", "pd_vina_flex_workspace_numel"}
    assert new <= set(_lib.header_symbols())
    L = _lib.lib()
    assert new <= set(_lib.SYMBOLS) and all(hasattr(L, s) for s in new)
    assert L.pd_vina_flex_workspace_numel(3, 22, 6) == 3 * (144 + 66)
    assert L.pd_vina_flex_workspace_numel(1, 1025, 0) == -3 and L.pd_vina_flex_workspace_numel(1, 12, 59) == -3
    assert L.pd_vina_flex_workspace_numel(0, 12, 3) == -1 and L.pd_vina_flex_workspace_numel(65536, 12, 3) == -3


def test_the_driver_keyword_is_checked_before_anything_is_sampled(cases):
    import inspect
    import torch
    from physdock_amd import driver
    c = cases["small"]
    f = flex_refine_of(c)
    A = c["x"].shape[1]

    class NoSampling:
        def sample_diffusion(self, *a, **k):
            raise AssertionError("sampled")

    batch = {"x_gt": torch.zeros(A + 1, 3)}
    with pytest.raises(ValueError, match=f"flex= was built over {A} pose atoms, the batch holds {A + 1}"):
        driver.redock(NoSampling(), batch, flex=f)
    with pytest.raises(ValueError, match="flex= takes a flex.FlexRefine"):
        driver.redock(NoSampling(), batch, flex=object())
    with pytest.raises(ValueError, match="flex= was built over"):
        driver.redock_many(NoSampling(), [(batch, {"flex": f})])
    driver.check_flex(None, batch)                                                   # without the keyword nothing is checked ...
    assert inspect.signature(driver.redock).parameters["flex"].default is None       # ... and nothing runs
    driver.check_flex(f, {"x_gt": torch.zeros(A, 3)})


# ------------------------------------------------------------------ the restatement
def test_no_flex_is_the_restatement_of_vina_refine(cases):
    c = cases["no_flex"]
    b = vrr.make_case(ref.CASES["no_flex"]["base"])
    for p in range(2):
        xp, y = pose(c, p)
        ev, want = ref.evaluate(c, xp, y), vrr.evaluate(b, xp, y)
        assert ev["receptor"] == 0.0 and all(np.array_equal(ev[k], want[k]) for k in ("energy", "inter", "intra", "grad", "ggrad"))
        a, w = ref.refine(c, xp, max_iters=20), vrr.refine(b, xp, max_iters=20)
        assert np.array_equal(a["y"], w["y"]) and all(a[k] == w[k] for k in ("energy", "iterations", "evaluations", "status", "moved"))
        assert a["moved_flex"] == 0.0


def test_gradients_against_central_differences(cases):
    for name in ref.FD_CASES:
        c = cases[name]
        L = c["L"]
        for p in range(c["x"].shape[0]):
            xp, y = pose(c, p)
            ev = ref.evaluate(c, xp, y)
            assert ev["margin"] >= max(ref.MARGIN, LEVER * H_FD), (name, p, ev["margin"])
            assert np.abs(y[:L] - y[:L].mean(0)).max() <= LEVER
            assert all(np.sqrt(((y[m] - y[a]) ** 2).sum(-1)).max() <= LEVER for (a, _), m in zip(c["rot"], c["sets"]))
            n = 6 + len(c["rot"])
            fd = np.zeros(n)
            for k in range(n):
                e = np.zeros(n)
                e[k] = H_FD
                fd[k] = (ref.evaluate(c, xp, ref.move(c, y, e))["energy"] - ref.evaluate(c, xp, ref.move(c, y, -e))["energy"]) / (2 * H_FD)
            assert np.abs(fd - ev["ggrad"]).max() <= FD_TOL, (name, p, np.abs(fd - ev["ggrad"]).max())
            fdc = np.zeros_like(y)
            for i in range(len(y)):
                for a in range(3):
                    yp, ym = y.copy(), y.copy()
                    yp[i, a] += H_FD
                    ym[i, a] -= H_FD
                    fdc[i, a] = (ref.evaluate(c, xp, yp)["energy"] - ref.evaluate(c, xp, ym)["energy"]) / (2 * H_FD)
            assert np.abs(fdc - ev["grad"]).max() <= FD_TOL, (name, p, np.abs(fdc - ev["grad"]).max())
            if c["S"]:
                assert np.abs(ev["ggrad"][6 + c["T"]:]).max() > 1e-3                  # the side chains feel a force


def bonded_and_13(c):
    """bool [M,M]: movable rows bonded or 1-3 to one another, in the ligand's and the receptor's bond graphs"""
    M, L = c["L"] + c["F"], c["L"]
    local = {int(a): k for k, a in enumerate(c["mov_idx"])}
    adj = np.zeros((M, M), dtype=bool)
    for i, j in c["bonds"]:
        adj[i, j] = adj[j, i] = True
    for i, j in c["rec_bonds"]:
        if i in local and j in local:
            adj[local[i], local[j]] = adj[local[j], local[i]] = True
    return adj | ((adj.astype(int) @ adj.astype(int)) > 0)


def test_move_preserves_every_bonded_and_13_distance(cases):
    rng = np.random.default_rng(11)
    for name, c in cases.items():
        xp, y = pose(c, 0)
        n = 6 + len(c["rot"])
        s = np.concatenate([rng.uniform(-2, 2, 3), rng.uniform(-1.5, 1.5, 3), rng.uniform(-3, 3, n - 6)])
        z = ref.move(c, y, s)
        keep = bonded_and_13(c)
        d0, d1 = np.sqrt(((y[:, None] - y[None]) ** 2).sum(-1)), np.sqrt(((z[:, None] - z[None]) ** 2).sum(-1))
        assert np.abs(d1 - d0)[keep].max() <= 1e-12 * max(1.0, d0[keep].max()), name
        assert np.abs(ref.move(c, y, np.zeros(n)) - y).max() <= 1e-14
        L = c["L"]
        t = ref.move(c, y, np.r_[1.0, -2.0, 0.5, np.zeros(n - 3)])                     # the translation moves the ligand rows alone
        assert np.abs(t[:L] - y[:L] - [1.0, -2.0, 0.5]).max() <= 1e-14 and np.array_equal(t[L:], y[L:])
        r = ref.move(c, y, np.r_[np.zeros(3), 0.3, -0.2, 0.9, np.zeros(n - 6)])
        assert np.array_equal(r[L:], y[L:]) and np.abs(r[:L] - y[:L]).max() > 1e-3
        for res_rows in c["residue_rows"]:                                           # the anchor CA (and with it the backbone) never moves
            assert np.array_equal(z[res_rows[0]], y[res_rows[0]])
        if c["S"]:
            assert np.abs(z[L:] - y[L:]).max() > 1e-3


def test_the_excluded_case_exercises_the_exclusion_list(cases):
    c = cases["excluded"]
    L = c["L"]
    cb = c["mov_idx"].tolist().index(c["residues"][0][0][1])                         # the row of CB: b of chi1
    for p in range(2):
        xp, y = pose(c, p)
        fixed = np.nonzero(c["fixed_mask"])[0]
        close = fixed[np.sqrt(((xp[fixed] - y[cb]) ** 2).sum(-1)) < 8.0]
        assert len(close) >= 3 and set(close.tolist()) <= set(c["excl"][cb].tolist())     # CB's close fixed neighbours are all within three bonds
        with_, without = ref.evaluate(c, xp, y), ref.evaluate(c, xp, y, exclusions=False)
        assert abs(with_["receptor"] - without["receptor"]) > 1.0 and with_["inter"] == without["inter"]
        assert np.abs(with_["grad"][cb] - without["grad"][cb]).max() > 1e-2


@pytest.fixture(scope="module")
def runs(cases):
    """the reference minimiser on every pose of every trajectory run, forward and with reversed summation order"""
    out = {}
    for name, mi in ref.RUNS:
        c = cases[name]
        for p in range(c["x"].shape[0]):
            xp = c["x"][p].astype(np.float64)
            out[name, mi, p] = (ref.refine(c, xp, max_iters=mi), ref.refine(c, xp, max_iters=mi, order=-1))
    return out


def test_the_minimiser_descends_and_the_side_chains_move(cases, runs):
    for (name, mi, p), (a, _) in runs.items():
        assert (np.diff(a["trace"]) <= 0).all() and a["trace"][0] == a["energy_start"] and a["trace"][-1] == a["energy"], (name, mi, p)
        assert a["energy"] < a["energy_start"] and a["evaluations"] >= a["iterations"] + 1 and 0 < a["iterations"] <= mi
        assert a["energy"] == (a["inter"] + a["intra"]) + a["receptor"]
        assert (a["moved_flex"] > 1e-3) == (cases[name]["S"] > 0), (name, mi, p)


def test_conditioning_guard(cases, runs):
    """the inputs of the GPU trajectory test are well conditioned (see tests/test_vina_refine_cpu.py::test_conditioning_guard)"""
    for (name, mi, p), (a, b) in runs.items():
        c = cases[name]
        xp = c["x"][p].astype(np.float64)
        assert ref.evaluate(c, xp, xp[c["mov_idx"]])["margin"] >= ref.GPU_MARGIN
        bound = ref.evaluate(c, xp, a["y"], bounds=True)["bound"]["energy"]
        assert abs(a["energy"] - b["energy"]) <= 0.25 * bound, (name, mi, p, abs(a["energy"] - b["energy"]), bound)
        assert np.abs(a["y"] - b["y"]).max() <= 1e-8, (name, mi, p, np.abs(a["y"] - b["y"]).max())
        assert (a["iterations"], a["evaluations"], a["status"]) == (b["iterations"], b["evaluations"], b["status"]), (name, mi, p)


def test_flexible_side_chains_reach_a_lower_energy_than_the_rigid_refinement(cases, runs):
    """the behavioural case: a four-chi side chain laid across the ligand.  The rigid refinement (the same chart without the side-chain
    torsions: VinaRefine, up to the constant receptor part) ends higher, by more than 0.1 kcal/mol, in the SAME energy function"""
    c = cases["across"]
    mi = dict(ref.RUNS)["across"]
    for p in range(c["x"].shape[0]):
        xp, y = pose(c, p)
        flex = runs["across", mi, p][0]
        rigid = ref.refine(ref.frozen_side_chains(c), xp, max_iters=mi)
        assert np.array_equal(rigid["y"][c["L"]:], y[c["L"]:]) and rigid["moved_flex"] == 0.0
        e_rigid = ref.evaluate(c, xp, rigid["y"])["energy"]
        assert flex["energy"] < e_rigid - 0.1, (p, flex["energy"], e_rigid)
        assert flex["moved_flex"] > 0.1


def test_non_finite_input_ends_at_once(cases):
    c = cases["small"]
    L = c["L"]
    for row, moved_nan in ((3, True), (L + 2, False)):                               # a ligand row; a side-chain row of a moving set
        xp = c["x"][0].astype(np.float64)
        xp[c["mov_idx"][row]] = np.nan
        a = ref.refine(c, xp, max_iters=5)
        assert (a["status"], a["iterations"], a["evaluations"]) == (2, 0, 1) and np.isfinite(a["energy"]) and a["energy"] == a["energy_start"]
        assert np.array_equal(a["y"], xp[c["mov_idx"]], equal_nan=True) and np.isnan(a["moved"]) == moved_nan
    xp = c["x"][0].astype(np.float64)
    xp[np.nonzero(c["fixed_mask"])[0][0]] = np.inf                                   # a fixed atom merely drops out
    assert ref.refine(c, xp, max_iters=3)["iterations"] == 3
