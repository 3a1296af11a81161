"""tests/shape_overlap_ref.py (the written definition of ShapeOverlap) against closed forms, the host side of physdock_amd/shape.py and
the argument checks of the driver and PoseClusters - nothing here needs a GPU."""
import numpy as np
import pytest
import torch

import shape_overlap_cases as cases
import shape_overlap_ref as ref


def one_atom(R=1.7, at=(0.0, 0.0, 0.0)):
    return ref.prepare(np.asarray([at]), [R], [])


def test_one_atom_self_overlap_and_volume():
    for R in (1.2, 1.7, 2.1):
        a = ref.KAPPA / R ** 2
        assert one_atom(R)["O"] == pytest.approx(ref.P ** 2 * (np.pi / (2 * a)) ** 1.5, rel=1e-14)
        assert ref.P * (np.pi / a) ** 1.5 == pytest.approx(4.0 * np.pi * R ** 3 / 3.0, rel=1e-14)      # pins KAPPA
    assert ref.P2 == pytest.approx(ref.P ** 2, rel=1e-15)


@pytest.mark.parametrize("d", [0.0, 0.7, 2.5, 9.0])
def test_two_equal_atoms(d):
    a = ref.KAPPA / 1.7 ** 2
    s = ref.score(one_atom(), one_atom(at=(d, 0.0, 0.0)))
    assert s["O_AB"] == pytest.approx(8.0 * np.exp(-a * d * d / 2.0) * (np.pi / (2 * a)) ** 1.5, rel=1e-13)
    assert s["color_tanimoto"] == 0.0 and s["combo"] == s["shape_tanimoto"]
    if d == 0.0:
        assert s["shape_tanimoto"] == 1.0


def test_far_pair_underflows_to_zero_and_nan_structure():
    s = ref.score(one_atom(), one_atom(at=(400.0, 0.0, 0.0)))
    assert s["O_AB"] == 0.0 and s["shape_tanimoto"] == 0.0 and s["combo"] == 0.0
    bad = ref.prepare(np.asarray([[np.nan, 0, 0]]), [1.7], [])
    assert all(np.isnan(ref.score(bad, one_atom())[k]) for k in ("O_AB", "shape_tanimoto", "color_tanimoto", "combo"))


def test_invariance_under_rigid_motion_and_permutation():
    ya, ra, fa = ref.molecule(14, 3)
    yb, rb, fb = ref.molecule(11, 4)
    base = ref.score(ref.prepare(ya, ra, fa), ref.prepare(yb, rb, fb))
    _, R, t = cases.rigid(ya, 0)
    mv = lambda y: np.asarray(y, dtype=np.float64) @ R.T + t
    moved = ref.score(ref.prepare(mv(ya), ra, fa), ref.prepare(mv(yb), rb, fb))
    perm = np.random.default_rng(0).permutation(14)
    inv = np.argsort(perm)
    permuted = ref.score(ref.prepare(ya[perm], ra[perm], [(k, tuple(int(inv[i]) for i in m)) for k, m in fa]), ref.prepare(yb, rb, fb))
    for k in ("O_AB", "C_AB", "shape_tanimoto", "color_tanimoto", "combo"):
        assert moved[k] == pytest.approx(base[k], rel=1e-11) and permuted[k] == pytest.approx(base[k], rel=1e-12), k
    assert base["C_AB"] > 0 and 0 < base["combo"] <= 2


def test_gradient_matches_central_differences():
    ya, ra, _ = ref.molecule(9, 5)
    yb, rb, _ = ref.molecule(7, 6)
    ya, yb = ya.astype(np.float64), yb.astype(np.float64)
    aa, ab = ref.alphas(ra), ref.alphas(rb)
    _, g, _ = ref.energy(ya, aa, yb, ab)
    h = 1e-5
    for i in range(9):
        for c in range(3):
            p, m = ya.copy(), ya.copy()
            p[i, c] += h; m[i, c] -= h
            fd = (ref.energy(p, aa, yb, ab)[0] - ref.energy(m, aa, yb, ab)[0]) / (2 * h)
            assert fd == pytest.approx(g[i, c], rel=1e-6, abs=1e-8)


@pytest.mark.parametrize("name", list(cases.OVERLAY_CASES))
def test_overlay_cases_keep_their_margins(name):
    c = cases.overlay_case(name)
    o = ref.overlay(c["A"], c["B"], max_iters=c["max_iters"])
    for k, floor in cases.MARGINS.items():
        assert o["margin"][k] >= floor, (name, k, o["margin"][k])
    assert o["overlap"] >= o["overlap_start"] and o["overlap"] >= -o["runs"][4]["energy"]
    assert o["status"] == (1 if name.endswith("short") else 0)
    # the conditioning guard: B's atoms summed in reverse order, the same decisions and the same fit
    M = len(c["xb"])
    B2 = ref.prepare(c["xb"][::-1].copy(), c["rb"][::-1].copy(), [(k, tuple(M - 1 - i for i in m)) for k, m in c["fb"]])
    o2 = ref.overlay(c["A"], B2, max_iters=c["max_iters"])
    assert all(o[k] == o2[k] for k in ("iterations", "evaluations", "status", "best_start")) and np.abs(o["y"] - o2["y"]).max() < 1e-8


def test_overlay_of_a_moved_copy_recovers_the_motion():
    c = cases.overlay_case("L12_M12")
    moved, R, t = cases.rigid(c["xa"], 1)
    o = ref.overlay(c["A"], ref.prepare(moved, c["ra"], c["fa"]))
    assert abs(o["shape_tanimoto"] - 1.0) < 1e-9 and np.abs(o["y"] - moved).max() < 1e-3


# ------------------------------------------------------------------ the host side of the package
DRAWN = dict(elements=["C"] * 6 + ["C", "O", "O", "C", "N", "O"],
             bonds=[(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 6), (6, 7), (6, 8), (3, 9), (9, 10), (4, 11)],
             orders=[1.5] * 6 + [1, 2, 1, 1, 1, 1])


def test_feature_table_of_a_drawn_molecule():
    from physdock_amd import shape
    spec = shape.ShapeSpec.from_bonds(DRAWN["elements"], DRAWN["bonds"], DRAWN["orders"])
    # a benzene ring with a carboxylic acid on atom 0, an aminomethyl on 3, a hydroxyl on 4; the ring's carbons are no hydrophobes
    assert spec.features == [("donor", (8,)), ("donor", (10,)), ("donor", (11,)), ("acceptor", (7,)), ("acceptor", (8,)), ("acceptor", (11,)),
                             ("cation", (10,)), ("anion", (7,)), ("anion", (8,)), ("ring", (0, 1, 2, 3, 4, 5))]
    assert spec.n_atoms == 12 and (spec.radii == 1.7).all() and shape.FEATURE_NAMES == ref.FEATURE_NAMES
    vdw = shape.ShapeSpec.from_bonds(DRAWN["elements"], DRAWN["bonds"], DRAWN["orders"], radii="vdw")
    assert vdw.radii.tolist() == [1.7] * 7 + [1.55, 1.55, 1.7, 1.6, 1.55]
    assert shape.KAPPA == pytest.approx(ref.KAPPA, rel=1e-15) and shape.COLOR_ALPHA == pytest.approx(ref.COLOR_ALPHA, rel=1e-15)
    with pytest.raises(AttributeError):
        spec.radii = None
    with pytest.raises(ValueError):
        spec.radii[0] = 2.0


def test_from_sdf_record():
    from physdock_amd import shape
    rec = dict(elements=DRAWN["elements"], bonds=np.asarray(DRAWN["bonds"]), bond_orders=np.asarray(DRAWN["orders"], dtype=np.float64),
               charges=np.zeros(12, dtype=np.int64), coords=np.zeros((12, 3)))
    spec = shape.ShapeSpec.from_sdf(rec)
    assert spec.n_atoms == 12 and ("ring", (0, 1, 2, 3, 4, 5)) in spec.features and spec.ligand_idx is None


def test_tversky_and_apply():
    from physdock_amd import shape
    res = dict(O_AB=torch.tensor([[2.0, 3.0]], dtype=torch.float64), O_AA=torch.tensor([4.0], dtype=torch.float64),
               O_BB=torch.tensor([8.0, 6.0], dtype=torch.float64))
    assert torch.equal(shape.tversky(res, 1.0), torch.tensor([[0.5, 0.75]], dtype=torch.float64))
    assert torch.equal(shape.tversky(res, 0.0), torch.tensor([[0.25, 0.5]], dtype=torch.float64))
    assert shape.tversky(res, 0.5)[0, 0].item() == pytest.approx(ref.tversky(2.0, 4.0, 8.0, 0.5))
    one = dict(O_AB=torch.tensor([2.0, 3.0], dtype=torch.float64), O_AA=torch.tensor([4.0, 6.0], dtype=torch.float64),
               O_BB=torch.tensor([8.0], dtype=torch.float64))                           # the vectors of to_reference: [P], [P], [1]
    assert torch.equal(shape.tversky(one, 1.0), torch.tensor([0.5, 0.5], dtype=torch.float64))
    assert torch.equal(shape.tversky(one, 0.5), torch.tensor([2.0 / 6.0, 3.0 / 7.0], dtype=torch.float64))
    x = torch.tensor([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
    q = torch.tensor([np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)])                         # a quarter turn about z
    got = shape.apply(x, q, torch.tensor([0.5, 0.0, -1.0]))
    assert got.dtype == torch.float64 and torch.allclose(got, torch.tensor([[0.5, 1.0, -1.0], [-1.5, 0.0, -1.0]], dtype=torch.float64), atol=1e-7)
    assert np.allclose(ref.apply(x.numpy(), q.numpy(), [0.5, 0.0, -1.0]), got.numpy(), atol=1e-7)


def test_host_value_errors():
    from physdock_amd import shape
    S = shape.ShapeSpec
    with pytest.raises(ValueError):
        S.from_tables(0)
    with pytest.raises(ValueError):
        S.from_tables(shape.MAX_ATOMS + 1)
    with pytest.raises(ValueError):
        S.from_tables(3, [("donor", (3,))])                                           # an index outside the molecule
    with pytest.raises(ValueError):
        S.from_tables(3, [("donor", ())])
    with pytest.raises(ValueError):
        S.from_tables(3, [("sticky", (0,))])
    with pytest.raises(ValueError):
        S.from_tables(3, [(6, (0,))])
    with pytest.raises(ValueError):
        S.from_tables(3, radii=[1.7, 1.7])
    with pytest.raises(ValueError):
        S.from_tables(3, radii=[1.7, -1.0, 1.7])
    with pytest.raises(ValueError):
        S.from_tables(3, radii="covalent")
    with pytest.raises(ValueError):
        S.from_tables(3, ligand_idx=[0, 1])
    with pytest.raises(ValueError):
        S.from_tables(2, [("ring", (0, 1))] * (shape.MAX_FEATURES + 1))
    with pytest.raises(ValueError):
        shape.ShapeOverlap("spec")
    so = shape.ShapeOverlap(S.from_tables(3))
    with pytest.raises(ValueError):
        so.pairwise(torch.zeros(2, 3, 3))                                              # not on the device
    with pytest.raises(ValueError):
        so.overlay(torch.zeros(2, 3, 3), so.spec, torch.zeros(2, 3, 3), max_step=0.0)
    big = shape.ShapeOverlap(S.from_tables(shape.MAX_OVERLAY_ATOMS + 1))
    with pytest.raises(ValueError):
        big.overlay(torch.zeros(1, 257, 3), big.spec, torch.zeros(1, 257, 3))


def test_driver_and_clusters_refuse_before_sampling():
    from physdock_amd import shape
    from physdock_amd.clustering import PoseClusters, check_redock_prerequisites
    from physdock_amd.driver import redock, redock_many
    from physdock_amd.synthetic import small_batch
    assert PoseClusters(cutoff=0.3, metric="shape").metric == "shape"
    with pytest.raises(ValueError, match="needs shape="):
        check_redock_prerequisites(PoseClusters(metric="shape"))
    batch = small_batch(0)
    n = int(batch["is_ligand"][batch["atom_id_to_token_id"].long()].sum())

    class Model:                                                                       # sampling would raise: the checks come first
        def sample_diffusion(self, *a, **k):
            raise AssertionError("sampled")

    wrong = shape.ShapeOverlap(shape.ShapeSpec.from_tables(n + 1))
    for bad in (wrong, "shape", (shape.ShapeOverlap(shape.ShapeSpec.from_tables(n)), "ref")):
        with pytest.raises(ValueError, match="shape="):
            redock(Model(), batch, shape=bad)
    with pytest.raises(ValueError, match="needs shape="):
        redock(Model(), batch, clusters=PoseClusters(metric="shape"))
    with pytest.raises(ValueError, match="shape="):
        redock_many(Model(), [(batch, dict(shape=wrong))])


def test_abi_exports():
    from physdock_amd import _lib
    declared = set(_lib.header_symbols())
    assert {"pd_shape_prepare", "pd_shape_overlap", "pd_shape_overlay"} <= declared
    L = _lib.lib()
    for name in ("pd_shape_workspace_numel", "pd_shape_prepare", "pd_shape_overlap", "pd_shape_overlay_workspace_numel", "pd_shape_overlay"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.pd_shape_workspace_numel(3, 5, 2) == 3 * (15 + 6 + 2) and L.pd_shape_overlay_workspace_numel(2, 3, 7) == 2 * 3 * 5 * (16 + 21)
    assert L.pd_shape_workspace_numel(1, 1025, 0) == -3 and L.pd_shape_workspace_numel(0, 4, 0) == -1
