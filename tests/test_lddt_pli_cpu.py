"""lDDT-PLI without a GPU: the float64 restatement (tests/lddt_pli_ref.py) against hand-computed answers, the host tables of
`LddtPli` against the restatement's naive loops, the argument checks, the header, and the condition the GPU tests rest on: for
every seeded case of tests/lddt_pli_cases.py the compares the margin DELTA leaves open are at most 1e-3 of all compares (one
`UNCERTAIN | ...` line per case, pytest -s: the source of the table in NOTES.md)."""
import re
import types

import numpy as np
import pytest
import torch

import lddt_pli_cases as cases
import lddt_pli_ref as ref

MAX_SHARE = 1e-3


# ------------------------------------------------------------------ the restatement against hand-computed answers
def three_contacts():
    """ligand atom 0 at the origin, receptor atoms on the axes at 3, 4 and 5 A, a fourth one 7 A away (no contact)"""
    x_gt = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [0, 0, 5], [0, -7, 0]], dtype=np.float32)
    return x_gt, [0], np.array([False, True, True, True, True])


def test_identical_pose_scores_one():
    x_gt, lig, rec = three_contacts()
    out = ref.lddt_pli(x_gt[None], x_gt, lig, rec)
    assert out["n_contacts"] == 3 and out["conserved"].tolist() == [[3, 3, 3, 3]]
    assert out["lddt_pli"].tolist() == [1.0] and out["per_atom"].tolist() == [[1.0]] and out["best_perm"].tolist() == [0]


def test_ligand_moved_ten_angstrom_scores_zero():
    x_gt, lig, rec = three_contacts()
    x = x_gt.copy()
    x[0] = [-10, 0, 0]                      # distances 13, sqrt(116), sqrt(125): every difference is above 4 A
    out = ref.lddt_pli(x[None], x_gt, lig, rec)
    assert out["conserved"].tolist() == [[0, 0, 0, 0]] and out["lddt_pli"].tolist() == [0.0]


def test_one_contact_moved_by_three_quarters_of_an_angstrom():
    x_gt = np.array([[0, 0, 0], [3, 0, 0]], dtype=np.float32)
    x = x_gt.copy()
    x[1] = [3.75, 0, 0]
    out = ref.lddt_pli(x[None], x_gt, [0], np.array([False, True]))
    assert out["n_contacts"] == 1 and out["conserved"].tolist() == [[0, 1, 1, 1]] and out["lddt_pli"].tolist() == [0.75]
    start, atom, dist = ref.contacts(x_gt, [0], np.array([False, True]))
    pc = ref.pair_counts(x[None], [0], start, atom, dist)
    assert pc["c"].tolist() == pc["lo"].tolist() == pc["hi"].tolist() == [[[[0, 1, 1, 1]]]]
    # a compare inside the margin is left open: the difference 0.75 against a threshold of 0.75 + DELTA / 2
    open_ = ref.pair_counts(x[None], [0], start, atom, dist, thresholds=(0.75 + ref.DELTA / 2, 1, 2, 4))
    assert open_["lo"][0, 0, 0, 0] == 0 and open_["hi"][0, 0, 0, 0] == 1


def test_no_contacts_scores_zero():
    x_gt, lig, rec = three_contacts()
    out = ref.lddt_pli(x_gt[None], x_gt, lig, np.zeros(5, bool))
    assert out["n_contacts"] == 0 and out["lddt_pli"].tolist() == [0.0] and out["per_atom"].tolist() == [[0.0]]


def phenyl():
    """(x_gt [A,3], lig, rec_mask, bonds, elements, orders): a phenyl ring (atoms 0 - 5) on an anchor atom (6) in a random pocket"""
    rng = np.random.default_rng(3)
    ring = np.array([[1.39 * np.cos(k * np.pi / 3), 1.39 * np.sin(k * np.pi / 3), 0.0] for k in range(6)])
    anchor = np.array([[1.39 + 1.5, 0.0, 0.0]])
    x_gt = np.concatenate([ring, anchor, rng.uniform(-7, 7, (80, 3))]).astype(np.float32)
    rec = np.ones(len(x_gt), bool)
    rec[:7] = False
    bonds = [(k, (k + 1) % 6) for k in range(6)] + [(0, 6)]
    return x_gt, list(range(7)), rec, bonds, [6] * 6 + [7], [1.5] * 6 + [1.0]


def test_flipped_phenyl_needs_the_symmetry_table():
    from physdock_amd import LigandSymmetry
    x_gt, lig, rec, bonds, el, orders = phenyl()
    sym = LigandSymmetry.from_bonds(7, bonds, el, orders)
    assert sym.perms.tolist() == [[0, 1, 2, 3, 4, 5, 6], [0, 5, 4, 3, 2, 1, 6]]
    x = x_gt.copy()
    x[[1, 2, 4, 5]] = x_gt[[5, 4, 2, 1]]           # the ring turned by 180 degrees about the axis through atoms 0 and 3
    plain = ref.lddt_pli(x[None], x_gt, lig, rec)
    with_sym = ref.lddt_pli(x[None], x_gt, lig, rec, perms=sym.perms)
    assert plain["n_contacts"] > 100 and plain["lddt_pli"][0] < 0.95
    assert with_sym["lddt_pli"].tolist() == [1.0] and with_sym["best_perm"].tolist() == [1]
    assert with_sym["conserved"].tolist() == [[plain["n_contacts"]] * 4] and (with_sym["per_atom"] == 1.0).all()
    # the unflipped pose keeps row 0: the smallest maximiser
    assert ref.lddt_pli(x_gt[None], x_gt, lig, rec, perms=sym.perms)["best_perm"].tolist() == [0]


# ------------------------------------------------------------------ the seeded cases and the condition of the GPU tests
@pytest.mark.parametrize("name", list(cases.CASES))
def test_seeded_cases_leave_few_compares_open(name):
    r = cases.reference(name)
    share, n = cases.uncertain_share(r)
    print(f"UNCERTAIN | {name} | P={r['x'].shape[0]} A={r['x'].shape[1]} L={len(r['lig'])} M={len(r['table_perms'])} "
          f"contacts={int(r['start'][-1])} candidates={int(r['cand_start'][-1])} | {n} | {int((r['hi'] - r['lo']).sum())} | {share:.2e} |")
    assert share <= MAX_SHARE and (r["lo"] <= r["c"]).all() and (r["c"] <= r["hi"]).all()
    assert np.abs(r["x"]).max() < cases.BOX and np.abs(r["x_gt"]).max() < cases.BOX
    if name not in ("empty",):
        # the rigidly moved copy stays in the box and, in float64, inside the same lo and hi
        moved = cases.rigid_copy(r["x"])
        assert np.abs(moved).max() < cases.BOX
        pc = ref.pair_counts(moved, r["lig"], r["start"], r["atom"], r["dist"], delta=0.0)["c"]
        c = ref.by_candidate(pc, r["table_perms"])
        assert (r["lo"] <= c).all() and (c <= r["hi"]).all()


def test_the_cases_have_the_shapes_they_are_there_for():
    from physdock_amd.lddt_pli import CONTACT_TILE, LDS_CANDIDATES
    r = {k: cases.reference(k) for k in cases.CASES}
    n_i = {k: np.diff(v["start"]) for k, v in r.items()}
    assert r["empty"]["x"].shape[:2] == (1, 5) and n_i["empty"].tolist() == [0]
    assert r["three"]["x"].shape[0] == 1 and n_i["three"].tolist() == [3]
    assert r["ring"]["x"].shape == (5, 333, 3) and r["ring"]["table_perms"].shape == (12, 12) and 30 <= n_i["ring"].mean() <= 50
    assert r["cf3"]["table_perms"].shape[0] == 1296 and 1296 > 4 * 256 and 1296 % 256
    assert n_i["dense"].tolist() == [700] and 700 > CONTACT_TILE and 700 > 2 * 256
    assert (~r["masked"]["lig_mask"]).sum() == 2 and n_i["masked"][[2, 9]].tolist() == [0, 0] and (n_i["masked"] > 0).sum() == 10
    assert int(r["wide"]["cand_start"][-1]) > LDS_CANDIDATES and r["wide"]["x"].shape[0] == 2
    # poses relabelled by a table row: the restatement finds rows other than the identity
    for k in ("ring", "cf3", "masked", "wide"):
        best = ref.select(r[k]["c"], r[k]["table_perms"], n_i[k])["best_perm"]
        assert (best != 0).any(), k
    # the constructed ties: two rows share the maximum, the smaller one is named
    s = ref.select(r["tie"]["c"], r["tie"]["table_perms"], n_i["tie"])
    t = s["totals"]
    assert t[0, 2] == t[0, 3] > max(t[0, 0], t[0, 1]) and t[0, 0] == t[0, 1] and t[1, 0] == t[1, 1] >= max(t[1, 2], t[1, 3])
    assert s["best_perm"].tolist() == [2, 0]
    for key in ("lo", "hi"):                          # ... whatever the open compares turn out to be
        u = ref.select(r["tie"][key], r["tie"]["table_perms"], n_i["tie"])["totals"]
        assert u[0, 2] == u[0, 3] and u[1, 0] == u[1, 1]


# ------------------------------------------------------------------ host tables
def tables_of(r, **kw):
    from physdock_amd import LddtPli, LigandSymmetry
    sym = None if r["perms"] is None else LigandSymmetry.from_permutations(r["perms"])
    return LddtPli.from_arrays(r["x_gt"], r["lig"], r["rec_mask"], sym, ligand_mask=r["lig_mask"], **kw)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_host_tables_against_the_naive_loops(name):
    r = cases.reference(name)
    t = tables_of(r)
    L, M = len(r["lig"]), len(r["table_perms"])
    assert (t.n_atoms, t.n_perms, t.n_pose_atoms, t.n_contacts) == (L, M, r["x"].shape[1], int(r["start"][-1]))
    assert t.contact_start.dtype == np.int32 and t.contact_start.tolist() == r["start"].tolist()
    assert t.contact_atom.dtype == np.int32 and t.contact_atom.tolist() == r["atom"].tolist()
    assert t.contact_dist.dtype == np.float32 and np.array_equal(t.contact_dist, r["dist"])
    assert t.atom_contacts.tolist() == np.diff(r["start"]).tolist() and t.ligand_idx.tolist() == r["lig"].tolist()
    # candidates: the distinct images, ascending; slot_t names the image of every row, atom-major as LigandSymmetry's table
    assert t.cand_start.tolist() == r["cand_start"].tolist() and t.cand_atom.tolist() == r["cand_atom"].tolist()
    assert t.slot_t.dtype == np.uint16 and t.slot_t.shape == (L, M) and t.slot_t.flags["C_CONTIGUOUS"]
    assert np.array_equal(t.slot_t, r["slot"])
    for i in range(L):
        own = t.cand_atom[t.cand_start[i]:t.cand_start[i + 1]]
        assert own.tolist() == sorted(set(r["table_perms"][:, i].tolist()))
        assert np.array_equal(own[t.slot_t[i]], r["table_perms"][:, i])
    assert t.n_candidates == int(r["cand_start"][-1]) and t.symmetry_complete is True


def test_tables_are_uploaded_once_per_device_with_the_host_dtypes():
    from physdock_amd import ops
    assert ops.resolve_device("cpu") == torch.device("cpu")
    assert ops.resolve_device(torch.device("cuda", 0)) == torch.device("cuda", 0)
    r = cases.reference("ring")
    t = tables_of(r)
    d = t.tables("cpu")
    assert t.tables(torch.device("cpu")) is d and list(t._tables) == [torch.device("cpu")]
    L, M, n, c = len(r["lig"]), len(r["table_perms"]), int(r["start"][-1]), int(r["cand_start"][-1])
    want = {"ligand_idx": (torch.int32, (L,)), "contact_start": (torch.int32, (L + 1,)), "contact_atom": (torch.int32, (n,)),
            "contact_dist": (torch.float32, (n,)), "cand_start": (torch.int32, (L + 1,)), "cand_atom": (torch.int32, (c,)),
            "slot_t": (torch.int16, (L, M)), "atom_contacts": (torch.int32, (L,))}
    assert list(d) == list(want)
    for k, (dtype, shape) in want.items():
        assert d[k].dtype == dtype and tuple(d[k].shape) == shape and d[k].is_contiguous(), k
        host = t.slot_t.view(np.int16) if k == "slot_t" else getattr(t, k)
        assert np.array_equal(d[k].numpy(), host), k


def test_masked_atoms_are_left_out_of_the_tables():
    r = cases.reference("masked")
    t = tables_of(r)
    everything = ref.contacts(r["x_gt"], r["lig"], np.ones(len(r["x_gt"]), bool))
    lig = set(r["lig"].tolist())
    hidden = [j for j in range(len(r["x_gt"])) if not r["rec_mask"][j] and j not in lig]
    assert len(hidden) == 8 and all(j in everything[1] for j in hidden), "every masked receptor atom would be a contact"
    assert not set(hidden) & set(t.contact_atom.tolist()) and not lig & set(t.contact_atom.tolist())
    n_all = np.diff(everything[0])
    assert n_all[2] > 0 and n_all[9] > 0 and t.atom_contacts[[2, 9]].tolist() == [0, 0]
    # a receptor mask that names ligand atoms changes nothing: ligand atoms never count
    from physdock_amd import LddtPli
    loud = LddtPli.from_arrays(r["x_gt"], r["lig"], np.ones(len(r["x_gt"])), ligand_mask=np.ones(12))
    assert not lig & set(loud.contact_atom.tolist()) and loud.contact_start.tolist() == everything[0].tolist()


def test_from_batch_takes_the_ligand_and_the_masks_of_the_batch():
    from physdock_amd import LddtPli
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.synthetic import make_batch
    batch = make_batch(20, 4, 9, 4, seed=6)
    is_lig = ligand_atom_mask(batch).numpy()
    lig = np.nonzero(is_lig)[0]
    t = LddtPli.from_batch(batch)
    assert t.ligand_idx.tolist() == lig.tolist() and t.n_pose_atoms == len(is_lig) and t.n_perms == 1 and t._tables == {}
    start, atom, dist = ref.contacts(batch["x_gt"].numpy(), lig, ~is_lig)
    assert t.contact_start.tolist() == start.tolist() and t.contact_atom.tolist() == atom.tolist() and np.array_equal(t.contact_dist, dist)
    assert t.n_contacts > 0
    # a_mask hides a receptor atom, x_exists a ligand atom
    b2 = dict(batch, a_mask=batch["a_mask"].clone(), x_exists=batch["x_exists"].clone())
    gone = int(atom[0])
    b2["a_mask"][gone] = 0
    b2["x_exists"][lig[1]] = 0
    t2 = LddtPli.from_batch(b2)
    rec2 = ~is_lig
    rec2[gone] = False
    s2, a2, _ = ref.contacts(batch["x_gt"].numpy(), lig, rec2, lig_mask=np.arange(len(lig)) != 1)
    assert t2.contact_start.tolist() == s2.tolist() and t2.contact_atom.tolist() == a2.tolist() and gone not in a2
    assert t2.atom_contacts[1] == 0


def test_constructor_parameters_and_the_cut_table():
    from physdock_amd import LddtPli, LigandSymmetry
    r = cases.reference("ring")
    t = tables_of(r, radius=4.5, thresholds=(0.25, 0.75, 1.5, 3.0))
    start, atom, dist = ref.contacts(r["x_gt"], r["lig"], r["rec_mask"], radius=4.5)
    assert t.contact_atom.tolist() == atom.tolist() and t.n_contacts < int(r["start"][-1]) and t.thresholds == (0.25, 0.75, 1.5, 3.0)
    assert t.radius == 4.5
    cut = LddtPli.from_arrays(r["x_gt"], r["lig"], r["rec_mask"], LigandSymmetry.from_permutations(r["perms"][:5], complete=False))
    assert cut.symmetry_complete is False and cut.n_perms == 5


def test_value_errors():
    from physdock_amd import LddtPli, LigandSymmetry
    from physdock_amd.lddt_pli import MAX_ATOMS, MAX_PERMS
    x = np.zeros((1100, 3), np.float32)
    rec = np.ones(1100)
    assert (MAX_ATOMS, MAX_PERMS) == (1024, 65535)
    with pytest.raises(ValueError, match="ligand atoms"):
        LddtPli.from_arrays(x, np.arange(MAX_ATOMS + 1), rec)
    with pytest.raises(ValueError, match="ligand atoms"):
        LddtPli.from_arrays(x, np.arange(0), rec)
    big = types.SimpleNamespace(n_atoms=2, perms=np.zeros((MAX_PERMS + 1, 2), np.int32), complete=True)
    with pytest.raises(ValueError, match="permutations"):
        LddtPli.from_arrays(x, [0, 1], rec, big)
    with pytest.raises(ValueError, match="table over 3 atoms"):
        LddtPli.from_arrays(x, [0, 1], rec, LigandSymmetry.from_permutations([[0, 1, 2]]))
    with pytest.raises(ValueError, match="four"):
        LddtPli.from_arrays(x, [0, 1], rec, thresholds=(0.5, 1, 2))
    with pytest.raises(ValueError, match="four"):
        LddtPli.from_arrays(x, [0, 1], rec, thresholds=(0.5, 1, 2, 4, 8))
    with pytest.raises(ValueError, match="distinct"):
        LddtPli.from_arrays(x, [0, 0], rec)
    with pytest.raises(ValueError, match="distinct"):
        LddtPli.from_arrays(x, [0, 1100], rec)
    with pytest.raises(ValueError, match="receptor_mask"):
        LddtPli.from_arrays(x, [0, 1], rec[:-1])
    with pytest.raises(ValueError, match="ligand_mask"):
        LddtPli.from_arrays(x, [0, 1], rec, ligand_mask=[1])
    with pytest.raises(ValueError, match=r"\[A,3\]"):
        LddtPli.from_arrays(x[:, :2], [0, 1], rec)
    t = LddtPli.from_arrays(x, [0, 1], rec)
    with pytest.raises(ValueError, match="pose atoms"):
        t.score(torch.zeros(2, 1099, 3))


# ------------------------------------------------------------------ header, binding, package
def test_header_declares_the_launchers_and_the_abi_stays_11():
    import physdock_amd
    from physdock_amd import _lib, lddt_pli
    assert physdock_amd.LddtPli is lddt_pli.LddtPli
    assert _lib.ABI_VERSION == 11
    assert {"pd_lddt_pli_counts", "pd_lddt_pli_select"} <= set(_lib.header_symbols())
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "physdock_hip.h")).read()
    define = lambda name: eval(re.search(rf"#define\s+{name}\s+(.+)", hdr).group(1))
    assert define("PD_LDDT_PLI_TILE") == lddt_pli.CONTACT_TILE and define("PD_LDDT_PLI_LDS_CAND") == lddt_pli.LDS_CANDIDATES
    assert define("PD_LDDT_PLI_MAX_CONTACTS") == lddt_pli.MAX_CONTACTS and 4 * lddt_pli.MAX_CONTACTS < 2 ** 31
    src = open(_lib.os.path.join(_lib._HERE, "csrc", "lddt_pli.hip")).read()
    assert "PD_EXPORT int pd_lddt_pli_counts(" in src and "PD_EXPORT int pd_lddt_pli_select(" in src


def test_the_built_library_exports_and_binds_the_launchers():
    from physdock_amd import _lib
    L = _lib.lib()
    assert L.pd_abi_version() == 11
    for name, n_args in (("pd_lddt_pli_counts", 18), ("pd_lddt_pli_select", 13)):
        assert hasattr(L, name) and len(_lib.SYMBOLS[name].argtypes) == n_args
