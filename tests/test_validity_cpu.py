"""PoseValidity's host tables on hand-built molecules, the float64 restatement (tests/validity_ref.py) against hand-computed answers,
rank_by_confidence(valid=) on CPU tensors, the argument errors and the C ABI of pd_pose_validity."""
import math
import os
import re

import numpy as np
import pytest
import torch

import validity_ref as ref
from conftest import REPO

BUTANE = [(0, 1), (1, 2), (2, 3)]
RING = [(i, (i + 1) % 6) for i in range(6)]
#: C0=C1 with substituents 2, 3 on C0 and 4, 5 on C1
ETHENE = [(0, 1), (0, 2), (0, 3), (1, 4), (1, 5)]
ETHENE_ORDERS = [2.0, 1.0, 1.0, 1.0, 1.0]


def build(n, bonds, n_extra=0, elements=None, **kw):
    """PoseValidity of an n-atom ligand that is the LAST n of n + n_extra pose atoms, random reference conformer"""
    from physdock_amd.validity import PoseValidity
    rng = np.random.default_rng(n + len(bonds))
    el = [6] * (n + n_extra) if elements is None else elements
    return PoseValidity.from_bonds(n, bonds, rng.standard_normal((n, 3)) * 2, el, np.arange(n_extra, n_extra + n), **kw)


def far_pairs(v):
    return sorted((int(i), int(j)) for i, j in zip(*np.nonzero(v.far)) if i < j)


# ------------------------------------------------------------------ topological classes
def test_butane_and_hexane_classes():
    v = build(4, BUTANE)
    assert v.pair12.tolist() == [[0, 1], [1, 2], [2, 3]] and v.pair13.tolist() == [[0, 2], [1, 3]] and far_pairs(v) == []
    assert v.pair12.dtype == np.int32 and v.d12_ref.dtype == np.float32 and v.far.dtype == np.uint8 and v.far.shape == (4, 4)
    h = build(6, [(i, i + 1) for i in range(5)])
    assert far_pairs(h) == [(0, 4), (0, 5), (1, 5)] and np.array_equal(h.far, h.far.T) and not h.far.diagonal().any()
    assert len(h.pair12) == 5 and len(h.pair13) == 4


def test_reference_distances_come_from_the_conformer():
    from physdock_amd.validity import PoseValidity
    x = np.array([[0, 0, 0], [1.5, 0, 0], [1.5, 2.0, 0], [1.5, 2.0, 1.0]], dtype=np.float64)
    v = PoseValidity.from_bonds(4, BUTANE, x, [6] * 4, [0, 1, 2, 3])
    assert np.allclose(v.d12_ref, [1.5, 2.0, 1.0]) and np.allclose(v.d13_ref, [2.5, math.sqrt(5.0)])


def test_benzene_classes_and_ring_group():
    v = build(6, RING, bond_orders=[1.5] * 6)
    assert len(v.pair12) == 6 and len(v.pair13) == 6 and far_pairs(v) == []          # para atoms are three bonds apart
    assert v.planar.tolist() == [[0, 1, 2, 3, 4, 5, -1, -1]] and v.planar.dtype == np.int32
    assert build(6, RING).planar.shape == (0, 8)                                      # no orders: no groups
    assert build(6, RING, bond_orders=[1.0] * 6).planar.shape == (0, 8)               # cyclohexane
    assert build(6, RING, bond_orders=[1.5] * 6, planar_groups=[(0, 1, 2, 3)]).planar.tolist() == [[0, 1, 2, 3, -1, -1, -1, -1]]


def test_fused_and_five_rings():
    from physdock_amd.validity import planar_groups_from_bonds
    # indole-like: a six-ring 0..5 fused over the bond (4, 5) with a five-ring 4, 5, 6, 7, 8; the nine-atom perimeter is no group
    bonds = RING + [(5, 6), (6, 7), (7, 8), (8, 4)]
    groups = planar_groups_from_bonds(9, bonds, [1.5] * len(bonds))
    assert groups == [(0, 1, 2, 3, 4, 5), (4, 5, 6, 7, 8)]


def test_double_bond_group():
    v = build(6, ETHENE, bond_orders=ETHENE_ORDERS)
    assert v.planar.tolist() == [[0, 1, 2, 3, 4, 5, -1, -1]]
    assert build(6, ETHENE).planar.shape == (0, 8)
    # a degree-4 end (not sp2) defines no group; a bare C=C of two atoms defines none either
    assert build(7, ETHENE + [(1, 6)], bond_orders=ETHENE_ORDERS + [1.0]).planar.shape == (0, 8)
    assert build(2, [(0, 1)], bond_orders=[2.0]).planar.shape == (0, 8)


def test_two_fragments_are_far_from_each_other():
    v = build(6, BUTANE + [(4, 5)])
    assert far_pairs(v) == [(a, b) for a in range(4) for b in (4, 5)]
    assert v.pair12.tolist() == [[0, 1], [1, 2], [2, 3], [4, 5]] and v.pair13.tolist() == [[0, 2], [1, 3]]


# ------------------------------------------------------------------ radii, masks
def test_radii_and_overrides():
    el = [1, 6, 7, 8, 9, 15, 16, 17, 35, 53, 26, 5]
    v = build(4, BUTANE, n_extra=8, elements=el)
    assert np.allclose(v.radius, [1.2, 1.7, 1.6, 1.55, 1.5, 1.95, 1.8, 1.8, 1.9, 2.1, 2.0, 2.0]) and v.radius.dtype == np.float32
    w = build(4, BUTANE, n_extra=8, elements=el, radii={26: 1.4, 6: 1.75})
    assert np.allclose(w.radius, [1.2, 1.75, 1.6, 1.55, 1.5, 1.95, 1.8, 1.8, 1.9, 2.1, 1.4, 2.0])


def test_heavy_only_masks():
    from physdock_amd.validity import PoseValidity
    #            receptor: C  H  N  (masked) O | ligand: C  H  C  C  (scattered: pose atoms 1, 4, 6, 7 ... see ligand_idx)
    el = [6, 6, 1, 7, 1, 8, 6, 6]
    lig = [1, 4, 6, 7]
    a_mask = [1, 1, 1, 0, 1, 1, 1, 1]
    x = np.random.default_rng(0).standard_normal((4, 3))
    v = PoseValidity.from_bonds(4, BUTANE, x, el, lig, a_mask=a_mask)
    assert v.rec_mask.tolist() == [1, 0, 0, 0, 0, 1, 0, 0] and v.lig_active.tolist() == [1, 0, 1, 1]
    assert v.ligand_idx.tolist() == lig and v.rec_mask.dtype == np.uint8 and v.lig_active.dtype == np.uint8
    w = PoseValidity.from_bonds(4, BUTANE, x, el, lig, a_mask=a_mask, heavy_only=False)
    assert w.rec_mask.tolist() == [1, 0, 1, 0, 0, 1, 0, 0] and w.lig_active.tolist() == [1, 1, 1, 1]
    assert len(v.pair12) == 3                         # the hydrogen keeps its bond


def test_from_batch_reads_elements_and_ligand_atoms():
    from physdock_amd.synthetic import make_batch
    from physdock_amd.validity import PoseValidity
    b = make_batch(5, 3, 6, 4, seed=2)
    b["a_mask"] = b["a_mask"].clone()
    b["a_mask"][2] = 0.0
    bonds = [(i, i + 1) for i in range(5)]
    v = PoseValidity.from_batch(b, bonds)
    A = 5 * 3 + 6
    el = (b["ref_feat"][:, 4:132].argmax(-1) + 1).numpy()
    assert v.n_pose_atoms == A and v.n_atoms == 6 and v.ligand_idx.tolist() == list(range(15, 21))
    table = {1: 1.2, 6: 1.7, 7: 1.6, 8: 1.55, 9: 1.5, 15: 1.95, 16: 1.8}
    assert np.allclose(v.radius, [table.get(int(z), 2.0) for z in el])
    expect = np.ones(A, bool)
    expect[15:] = False
    expect[2] = False
    expect &= el != 1
    assert v.rec_mask.tolist() == expect.astype(int).tolist()
    assert v.lig_active.tolist() == (el[15:] != 1).astype(int).tolist()
    assert np.allclose(v.d12_ref, (b["ref_pos"][15:20] - b["ref_pos"][16:21]).norm(dim=-1).numpy())


def test_from_mmff_terms_reads_the_bond_rows():
    from physdock_amd.validity import PoseValidity

    from physdock_amd import mmff

    class Terms:                                  # what from_mmff_terms reads of an mmff.MMFFTerms
        n_atoms = 4
        idx = {mmff.BOND: np.asarray(BUTANE, dtype=np.int32)}
    v = PoseValidity.from_mmff_terms(Terms, np.random.default_rng(1).standard_normal((4, 3)), [6] * 4, [0, 1, 2, 3])
    assert v.pair12.tolist() == [[0, 1], [1, 2], [2, 3]] and v.pair13.tolist() == [[0, 2], [1, 3]]


# ------------------------------------------------------------------ the restatement against hand-computed answers
def tables(L, A, **kw):
    t = dict(lig_idx=np.arange(L), radius=np.full(A, 1.5, np.float32), rec_mask=np.zeros(A, np.uint8), lig_active=np.ones(L, np.uint8),
             pair12=np.zeros((0, 2), int), d12_ref=np.zeros(0, np.float32), pair13=np.zeros((0, 2), int), d13_ref=np.zeros(0, np.float32),
             far=np.zeros((L, L), np.uint8), planar=-np.ones((0, 8), int))
    t.update(kw)
    return t


def test_lifted_square_has_the_analytic_planarity():
    # a square (+-1, +-1, 0) with the corner (1, 1) lifted by h.  Centred on (0, 0, h/4) the scatter matrix has the eigenvector
    # (1, -1, 0) (eigenvalue 4) and, in the basis u = (1, 1, 0) / sqrt(2), z, the block [[4, h sqrt(2)], [h sqrt(2), 3 h^2 / 4]]: a
    # 2x2 problem with the closed form below.  The normal is a u + b z; the centred atoms have (u, z) components
    # (sqrt(2), 3h/4), (0, -h/4), (-sqrt(2), -h/4), (0, -h/4).
    for h in (0.4, 1.0):
        sq = np.array([[1, 1, h], [1, -1, 0], [-1, -1, 0], [-1, 1, 0]], dtype=np.float32)
        r = ref.pose_validity(sq[None], **tables(4, 4, planar=[[0, 1, 2, 3, -1, -1, -1, -1]]))
        h = float(np.float32(h))
        q = 0.75 * h * h
        lam = ((4 + q) - math.sqrt((4 - q) ** 2 + 8 * h * h)) / 2
        a, b = h * math.sqrt(2), lam - 4
        n = math.hypot(a, b)
        expect = max(abs(a * math.sqrt(2) + b * 0.75 * h), abs(b * 0.25 * h), abs(-a * math.sqrt(2) - b * 0.25 * h)) / n
        assert r["val"][0, 7] == pytest.approx(expect, abs=1e-12) and 0.2 * h < expect < 0.3 * h
        d, w = ref.plane_distance(sq)
        assert w[1] > 0.1
    flat = np.array([[1, 1, 0], [1, -1, 0], [-1, -1, 0], [-1, 1, 0]], dtype=np.float32)
    assert ref.pose_validity(flat[None], **tables(4, 4, planar=[[0, 1, 2, 3, -1, -1, -1, -1]]))["val"][0, 7] < 1e-12


def test_collinear_and_coincident_groups_report_zero():
    line = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3.5, 3.5, 3.5]], dtype=np.float32)
    point = np.ones((4, 3), dtype=np.float32)
    for pts in (line, point):
        assert ref.pose_validity(pts[None], **tables(4, 4, planar=[[0, 1, 2, 3, -1, -1, -1, -1]]))["val"][0, 7] == 0.0


def test_two_atoms_at_a_known_distance():
    x = np.array([[[0, 0, 0], [3, 4, 0], [0, 0, 6]]], dtype=np.float32)         # ligand atoms 0, 1; pose atom 2 is receptor
    rad = np.array([1.5, 1.0, 2.5], np.float32)
    t = tables(2, 3, radius=rad, rec_mask=np.array([0, 0, 1], np.uint8), pair12=[[0, 1]], d12_ref=[4.0], pair13=[[0, 1]], d13_ref=[10.0],
               far=np.array([[0, 1], [1, 0]], np.uint8))
    for fp32 in (False, True):
        r = ref.pose_validity(x, **t, fp32=fp32)
        d1 = math.sqrt(9 + 16 + 36)
        assert np.allclose(r["val"][0], [1.25, 1.25, 0.5, 0.5, 2.0, 6 / 4.0, 6.0, 0.0], rtol=1e-6)
        assert r["worst"].tolist() == [[0, 2]] and r["rec"][0, 1, 2] == pytest.approx(d1 / 3.5, rel=1e-6) and np.isinf(r["rec"][0, 0, 0])
    # nothing to look at: the neutral values, no flag
    r = ref.pose_validity(x, **tables(2, 3))
    assert r["val"][0].tolist() == [1, 1, 1, 1, np.inf, np.inf, np.inf, 0] and r["worst"].tolist() == [[-1, -1]] and ref.flags(r["val"]).tolist() == [0]
    # an inactive ligand atom and a masked receptor atom do not count; ties go to the smallest (a, j)
    x2 = np.array([[[0, 0, 0], [0, 0, 2], [0, 0, 1], [0, 0, 1]]], dtype=np.float32)
    t2 = tables(2, 4, rec_mask=np.array([0, 0, 1, 1], np.uint8))
    assert ref.pose_validity(x2, **t2)["worst"].tolist() == [[0, 2]]
    t2["lig_active"] = np.array([0, 1], np.uint8)
    assert ref.pose_validity(x2, **t2)["worst"].tolist() == [[1, 2]]
    t2["rec_mask"] = np.array([0, 0, 0, 1], np.uint8)
    assert ref.pose_validity(x2, **t2)["worst"].tolist() == [[1, 3]]


def test_flags_of_the_restatement():
    good = np.array([[1.0, 1.0, 1.0, 1.0, 1.2, 1.1, 3.5, 0.01]])
    assert ref.flags(good).tolist() == [0]
    for col, value, bit in ((0, 0.7, 1), (1, 1.3, 1), (2, 0.7, 2), (3, 1.3, 2), (4, 0.69, 4), (5, 0.74, 8), (7, 0.26, 16), (6, 8.5, 32)):
        v = good.copy()
        v[0, col] = value
        assert ref.flags(v).tolist() == [bit], col
    v = good.copy()
    v[0, 4:7] = np.inf
    assert ref.flags(v).tolist() == [0]
    assert ref.flags(good, {"bond_lo": 1.01}).tolist() == [1]


# ------------------------------------------------------------------ ranking
def test_rank_by_confidence_with_a_validity_mask():
    from physdock_amd.ranking import rank_by_confidence
    rc = torch.tensor([0.5, 0.9, 0.5, 0.1, 0.9, 0.5])
    pl = torch.tensor([70.0, 60.0, 80.0, 90.0, 60.0, 80.0])
    scores = {"ranking_confidence": rc, "mean_plddt": pl}
    plain = rank_by_confidence(scores)
    assert plain.tolist() == [1, 4, 2, 5, 0, 3] and torch.equal(rank_by_confidence(scores, valid=None), plain)
    valid = torch.tensor([True, False, False, True, True, True])
    order = rank_by_confidence(scores, valid=valid)
    assert order.tolist() == [4, 5, 0, 3, 1, 2] and order.dtype == torch.long
    assert rank_by_confidence(scores, valid=torch.ones(6, dtype=torch.bool)).tolist() == plain.tolist()
    assert rank_by_confidence(scores, valid=torch.zeros(6, dtype=torch.bool)).tolist() == plain.tolist()
    with pytest.raises(ValueError, match="bool"):
        rank_by_confidence(scores, valid=valid.float())
    with pytest.raises(ValueError, match="6 poses"):
        rank_by_confidence(scores, valid=valid[:5])


# ------------------------------------------------------------------ argument errors
def test_argument_errors():
    from physdock_amd.validity import PoseValidity
    x = np.random.default_rng(3).standard_normal((4, 3))
    with pytest.raises(ValueError, match=r"4 ligand atoms, ligand_idx holds 3"):
        PoseValidity.from_bonds(4, BUTANE, x, [6] * 8, [1, 2, 3])
    with pytest.raises(ValueError, match=r"4 ligand atoms, x_ref_lig has shape \(3, 3\)"):
        PoseValidity.from_bonds(4, BUTANE, x[:3], [6] * 8, [1, 2, 3, 4])
    with pytest.raises(ValueError, match="distinct atom indices below 8"):
        PoseValidity.from_bonds(4, BUTANE, x, [6] * 8, [1, 2, 3, 8])
    with pytest.raises(ValueError, match="distinct"):
        PoseValidity.from_bonds(4, BUTANE, x, [6] * 8, [1, 2, 3, 3])
    with pytest.raises(ValueError, match="bond"):
        PoseValidity.from_bonds(4, [(0, 4)], x, [6] * 8, [1, 2, 3, 4])
    with pytest.raises(ValueError, match="3 bonds but 2 bond orders"):
        PoseValidity.from_bonds(4, BUTANE, x, [6] * 8, [1, 2, 3, 4], bond_orders=[1, 1])
    with pytest.raises(ValueError, match="planar group 0"):
        PoseValidity.from_bonds(4, BUTANE, x, [6] * 8, [1, 2, 3, 4], planar_groups=[(0, 1, 2)])
    with pytest.raises(ValueError, match="planar group 0"):
        PoseValidity.from_bonds(12, [], np.random.default_rng(4).standard_normal((12, 3)), [6] * 12, range(12), planar_groups=[range(9)])
    with pytest.raises(ValueError, match="unknown thresholds"):
        PoseValidity.from_bonds(4, BUTANE, x, [6] * 8, [1, 2, 3, 4], thresholds={"bond_low": 0.5})
    with pytest.raises(ValueError, match="a_mask for 7"):
        PoseValidity.from_bonds(4, BUTANE, x, [6] * 8, [1, 2, 3, 4], a_mask=[1] * 7)
    with pytest.raises(ValueError, match="1025 ligand atoms"):
        PoseValidity.from_bonds(1025, [], np.random.default_rng(5).standard_normal((1025, 3)), [6] * 1025, range(1025))
    v = PoseValidity.from_bonds(4, BUTANE, x, [6] * 8, [1, 2, 3, 4], thresholds={"bond_lo": 0.9})
    assert v.thresholds["bond_lo"] == 0.9 and v.thresholds["bond_hi"] == 1.25 and v._thr.bond_lo == np.float32(0.9)
    with pytest.raises(ValueError, match=r"8 pose atoms, x_pred has shape \(2, 9, 3\)"):
        v.check(torch.zeros(2, 9, 3))
    assert PoseValidity.check_names(0) == [] and PoseValidity.check_names(torch.tensor(41)) == ["bond_lengths", "receptor_clash", "detached"]
    assert PoseValidity.check_names(63) == list(ref.CHECK_NAMES)


def test_defaults_match_the_restatement():
    from physdock_amd import PoseValidity, validity
    assert validity.DEFAULT_THRESHOLDS == ref.DEFAULT_THRESHOLDS and list(validity.DEFAULT_THRESHOLDS) == list(ref.DEFAULT_THRESHOLDS)
    assert validity.CHECK_NAMES == ref.CHECK_NAMES and PoseValidity is validity.PoseValidity
    assert "not been validated" in validity.__doc__


# ------------------------------------------------------------------ C ABI
def test_header_declares_the_launcher_and_the_binding_matches():
    import ctypes as C
    from physdock_amd import _lib
    hdr = open(os.path.join(REPO, "include", "physdock_hip.h")).read()
    assert {"pd_pose_validity", "pd_pose_validity_workspace_numel"} <= set(_lib.header_symbols())
    src = open(os.path.join(REPO, "physdock_amd", "_lib.py")).read()
    n_hdr = len(re.search(r"int\s+pd_pose_validity\s*\(([^;]*)\)\s*;", hdr).group(1).split(","))
    n_sig = len(re.search(r'sig\("pd_pose_validity",([^\n#]*)\)', src).group(1).split(","))
    assert n_hdr == n_sig == 23
    fields = re.search(r"typedef struct pd_validity_thresholds \{([^}]*)\}", hdr).group(1)
    names = [n.strip() for n in fields.replace("float", "").replace(";", "").split(",")]
    assert names == [f[0] for f in _lib.ValidityThresholds._fields_] == list(ref.DEFAULT_THRESHOLDS)
    assert C.sizeof(_lib.ValidityThresholds) == 32
    from physdock_amd import validity
    assert int(re.search(r"#define\s+PD_VALIDITY_REC_TILE\s+(\d+)", hdr).group(1)) == validity.REC_TILE
    L = _lib.lib()
    assert hasattr(L, "pd_pose_validity")
    assert L.pd_pose_validity_workspace_numel(3, 2 * validity.REC_TILE + 1) == 3 * 3 * 2
    assert L.pd_pose_validity_workspace_numel(0, 5) == -1 and L.pd_pose_validity_workspace_numel(65536, 5) == -3
