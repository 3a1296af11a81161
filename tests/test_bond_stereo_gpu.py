"""pd_bond_stereo (csrc/bond_stereo.hip) against its written definition (tests/bond_stereo_ref.py), the conformers of marked
ligands end to end, and the bond_stereo keywords of redock.  Inputs are random ligand-like coordinates plus entries whose dihedral is set
by construction, at least 1 degree from 90 and from max_twist, so no decision sits on a threshold."""
import numpy as np
import pytest
import torch

import bond_stereo_ref as ref

pytestmark = pytest.mark.gpu

MAX_TWIST = 30.0
#: one fp32 ulp at 180 degrees
ULP_180 = 2.0 ** -16
#: dihedrals and out-of-plane bends of the second substituents (degrees): the four pairs of an entry stand at phi, phi - bend_a,
#: phi + bend_d and phi + bend_d - bend_a (mod 180), each at least 5 degrees from +-30, +-90 and +-150 (`compare` checks the float64 values)
PHIS = (0.0, 8.0, -15.0, 50.0, -70.0, 110.0, -130.0, 165.0, 172.0, 180.0, -45.0)
BENDS = (0.0, 4.0, -6.0)


def make_case(n, P, A=None, first=0, seconds="some", seed=0):
    """-> (x fp32 [P,A,3], quads int32 [n,6], expect uint8 [n]): entry k owns six atoms from `first` on; seconds: which entries have
    a2 / d2 ("some": every second entry a2, every third d2; "all"; "none")"""
    rng = np.random.default_rng(seed)
    A = first + 6 * n if A is None else A
    assert first + 6 * n <= A
    x = rng.uniform(-8.0, 8.0, (P, A, 3))
    quads = np.full((n, 6), -1, dtype=np.int32)
    for k in range(n):
        base = first + 6 * k
        has_a2 = seconds == "all" or (seconds == "some" and k % 2 == 0)
        has_d2 = seconds == "all" or (seconds == "some" and k % 3 == 0)
        quads[k] = (base, base + 1, base + 2, base + 3, base + 4 if has_a2 else -1, base + 5 if has_d2 else -1)
        for p in range(P):
            phi, ba, bd = PHIS[(k + 3 * p) % len(PHIS)], BENDS[(k + p) % 3], BENDS[(2 * k + p) % 3]
            pts = ref.place(phi, rng, la=rng.uniform(1.2, 1.6), lc=rng.uniform(1.2, 1.6), t1=rng.uniform(110, 128), t2=rng.uniform(110, 128),
                            bend_a=ba, bend_d=bd)
            x[p, base:base + 6] = pts
    expect = rng.integers(1, 3, n).astype(np.uint8)
    return x.astype(np.float32), quads, expect


def run(x, quads, expect, max_twist=MAX_TWIST):
    from physdock_amd.bond_stereo import BondStereo
    spec = BondStereo.from_tables(quads, expect, max_twist=max_twist)
    return spec, spec.check(torch.from_numpy(x).cuda())


def compare(got, want, n_entries):
    g = {k: v.cpu().numpy() for k, v in got.items()}
    # no constructed decision sits on a threshold
    t64 = want["twist64"][np.isfinite(want["twist64"])]
    d64 = want["dihedral64"][np.isfinite(want["dihedral64"])]
    assert (np.abs(t64 - MAX_TWIST) > 0.5).all() and (np.abs(np.abs(d64) - 90.0) > 0.5).all()
    for k in ("state", "n_wrong", "n_twisted", "ok"):
        assert g[k].dtype == want[k].dtype and np.array_equal(g[k], want[k]), k
    for k in ("dihedral", "twist"):
        assert np.array_equal(np.isnan(g[k]), np.isnan(want[k]))
        fin = ~np.isnan(want[k])
        err = np.abs(g[k][fin].astype(np.float64) - want[k][fin].astype(np.float64))
        print(k, "largest difference to the rounded float64 value, in ulps at 180:", float(err.max() / ULP_180) if err.size else 0.0)
        assert (err <= ULP_180).all(), (k, float(err.max()))
    # the maximum is exact: the kernel's own twist row, bit for bit
    own = np.where(np.isnan(g["twist"]).any(1), np.float32(np.nan), np.nan_to_num(g["twist"], nan=0.0).max(1))
    assert g["max_twist_seen"].tobytes() == own.astype(np.float32).tobytes()


@pytest.mark.parametrize("n, P, A, first, seconds", [
    (1, 1, None, 0, "none"),         # minimal
    (64, 1, None, 0, "some"),        # one full wave
    (65, 1, None, 0, "some"),        # the stride loop
    (130, 3, None, 0, "some"),       # two full rounds and a tail, several poses
    (3, 3, 40, 17, "all"),           # ligand indices offset into the pose
    (7, 2, None, 5, "none"),
])
def test_kernel_against_the_definition(n, P, A, first, seconds):
    x, quads, expect = make_case(n, P, A, first, seconds, seed=n + P)
    spec, got = run(x, quads, expect)
    want = ref.check(x, quads, expect, MAX_TWIST)
    assert (want["n_wrong"] > 0).any() or n == 1
    compare(got, want, n)
    # two launches give equal bits
    again = spec.check(torch.from_numpy(x).cuda())
    assert all(got[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes() for k in got)
    # a label-only run: the same states, the undefined entries counted
    label = spec.label(torch.from_numpy(x).cuda())
    assert torch.equal(label, got["state"])


def test_undefined_entries_and_batch_independence():
    from physdock_amd.bond_stereo import BondStereo
    x, quads, expect = make_case(66, 3, seconds="some", seed=5)
    x[1, quads[2, 3], 0] = np.nan                                   # a coordinate that is not finite: entry 2 of pose 1
    x[1, quads[65, :3]] = np.asarray([[1.0, 2.0, 3.0], [2.0, 2.0, 3.0], [3.0, 2.0, 3.0]])       # a, b, c of entry 65 on one line, exactly
    x[1, quads[4, 4], 1] = np.inf                                   # a2 of entry 4: the main dihedral stays defined, the twist does not
    spec, got = run(x, quads, expect)
    want = ref.check(x, quads, expect, MAX_TWIST)
    assert want["state"][1, 2] == 0 and want["state"][1, 65] == 0 and want["state"][1, 4] != 0 and np.isnan(want["twist"][1, 4])
    assert np.isnan(want["max_twist_seen"][1]) and np.isfinite(want["max_twist_seen"][[0, 2]]).all()
    assert want["n_twisted"][1] >= 3 and want["ok"][1] == 0
    compare(got, want, 66)
    # a pose alone and the same pose inside the batch: equal bits
    for p in range(3):
        alone = spec.check(torch.from_numpy(x[p:p + 1]).cuda())
        for k in got:
            assert alone[k][0].cpu().numpy().tobytes() == got[k][p].cpu().numpy().tobytes(), (k, p)
    # expect = NULL labels only: n_wrong counts the undefined entries
    lab = BondStereo.from_tables(quads, None).check(torch.from_numpy(x).cuda())
    assert lab["n_wrong"].tolist() == [0, 2, 0] and lab["ok"].tolist() == [1, 0, 1] and torch.equal(lab["state"], got["state"])


def test_refusals_before_a_launch():
    from physdock_amd import ops
    from physdock_amd.bond_stereo import BondStereo
    x = torch.zeros(2, 12, 3, device="cuda")
    with pytest.raises(ValueError, match="1025 entries"):
        BondStereo.from_tables(np.tile([0, 1, 2, 3, -1, -1], (1025, 1)), None)
    with pytest.raises(ValueError, match="reach atom 12"):
        BondStereo.from_tables([[0, 1, 2, 12, -1, -1]], [1]).check(x)
    with pytest.raises(ValueError, match="reach atom 12"):
        BondStereo.from_tables([[0, 1, 2, 3, -1, 12]], [1]).label(x)
    with pytest.raises(ValueError, match="negative"):
        BondStereo.from_tables([[0, -1, 2, 3, -1, -1]], [1])
    with pytest.raises(ValueError, match="negative"):
        BondStereo.from_tables([[0, 1, 2, 3, -2, -1]], [1])
    with pytest.raises(ValueError, match="kind"):
        BondStereo.from_tables([[0, 1, 2, 3, -1, -1]], [3])
    with pytest.raises(ValueError, match="poses must be"):
        BondStereo.from_tables([[0, 1, 2, 3, -1, -1]], [1]).check(x[0])
    # the C entry point refuses what it can see: too many entries or poses (-3), a missing output or count (-1)
    L_ = ops._lib.init()
    q = torch.zeros(1, 6, dtype=torch.int32, device="cuda")
    o = torch.zeros(2, 1, device="cuda")
    s = torch.zeros(2, 1, dtype=torch.uint8, device="cuda")
    call = lambda P, n, state=s: L_.pd_bond_stereo(ops.ptr(x), ops.ptr(q), None, 30.0, ops.ptr(o), ops.ptr(o), ops.ptr(state) if state is not None else None,
                                                   None, None, None, None, P, 12, n, ops.stream())
    assert call(2, 1025) == -3 and call(65536, 1) == -3 and call(0, 1) == -1 and call(2, 0) == -1 and call(2, 1, None) == -1
    # without entries nothing is launched and every pose passes
    none = BondStereo.from_tables(np.zeros((0, 6)), np.zeros(0))
    out = none.check(x)
    assert out["state"].shape == (2, 0) and out["ok"].tolist() == [1, 1] and none.accept(x).tolist() == [True, True]


def test_describe_and_from_ligand():
    from physdock_amd.bond_stereo import BondStereo
    from physdock_amd.ligand import Ligand
    lig = Ligand.from_smiles("C/C=C/C=C\\C")
    idx = np.arange(6) + 17
    spec = BondStereo.from_ligand(lig, idx)
    assert spec.entries.tolist() == [[17, 18, 19, 20, 2, -1, -1], [19, 20, 21, 22, 1, -1, -1]] and spec.n_atoms == 6 and spec.n_entries == 2
    x = np.zeros((1, 40, 3), dtype=np.float32)
    x[0, 17:21] = ref.place(170.0)                                  # trans as written, 10 degrees of twist
    x[0, 21] = x[0, 20] + (x[0, 19] - x[0, 18])                     # the second bond cannot be judged from here: set it trans, 0 twist
    x[0, 22] = x[0, 21] + (x[0, 20] - x[0, 19])
    res = spec.check(torch.from_numpy(x).cuda())
    assert res["state"][0].tolist() == [2, 2] and res["n_wrong"].tolist() == [1] and not spec.accept(torch.from_numpy(x).cuda()).any()
    d = spec.describe(res, 0)
    assert [it["entry"] for it in d] == [0, 1] and d[0]["found"] == "trans" and d[1]["expected"] == "cis" and d[1]["found"] == "trans"
    assert abs(d[0]["twist"] - 10.0) < 1e-3 and not d[0]["twisted"]


# ---------------------------------------------------------------------- end to end: the conformers of marked ligands
@pytest.mark.parametrize("smiles", ["C/C=C/C", "C/C=C\\C", "OC(=O)/C=C/C(=O)O", "OC(=O)/C=C\\C(=O)O", "C/C=C/C=C\\C"])
def test_conformers_obey_the_marks(smiles):
    """The definition alone (tests/conformers_ref.py on the host) accepts 32 of 32 starts for each of these ligands."""
    from physdock_amd.bond_stereo import BondStereo
    from physdock_amd.conformers import ConformerEnsemble, ideal_bounds
    from physdock_amd.ligand import Ligand
    lig = Ligand.from_smiles(smiles)
    t = ideal_bounds(lig)
    ens = ConformerEnsemble.from_tables(t["lo"], t["up"], t["centres"], t["vol_lo"], t["vol_hi"], bond_stereo=t["stereo_bonds"])
    out = ens.embed(32, 0, keep=None, device="cuda")
    ok = out["ok"].bool().cpu().numpy()
    print(smiles, "accepted", int(ok.sum()), "of 32")
    assert ok.sum() >= 16
    spec = BondStereo.from_ligand(lig)
    state = spec.label(out["x"]).cpu().numpy()
    kinds = lig.bond_stereo[:, 4]
    assert (state[ok] == kinds[None]).all() and out["stereo_ok"].cpu().numpy()[ok].all()
    # the twist an accepted conformer can show: what its bounds allow when each may be violated by the conformer's own largest violation
    twist = spec.check(out["x"])["twist"].cpu().numpy()
    viol = out["max_violation"].cpu().numpy()
    for c in np.nonzero(ok)[0]:
        for k, row in enumerate(lig.bond_stereo.tolist()):
            bound = ref.twist_bound(t["lo"], t["up"], row[:4], float(viol[c]) + 1e-6)
            assert twist[c, k] <= bound + 1e-3, (c, k, float(twist[c, k]), bound)
    print(smiles, "largest twist of an accepted conformer", float(twist[ok].max()))
    # the chosen reference conformer is the written isomer too
    chosen = lig.embed_reference(seed=0, C=32, device="cuda")
    assert (spec.label(chosen["ref_pos"][None]).cpu().numpy()[0] == kinds).all()
    # the unmarked ligand's pool is told nothing and reports nothing
    assert "stereo_ok" not in ConformerEnsemble.from_tables(t["lo"], t["up"]).embed(2, 0, keep=None, device="cuda")


def test_from_sdf_labels_from_the_coordinates():
    from physdock_amd.ligand import Ligand
    for smiles in ("C/C=C/C", "C/C=C\\C", "C/C=C(/CC)C"):
        lig = Ligand.from_smiles(smiles)
        pos = lig.embed_reference(seed=0, C=8, device="cuda")["ref_pos"].cpu().numpy()
        record = {"title": smiles, "elements": lig.symbols(), "coords": pos.astype(np.float64), "bonds": lig.bonds, "bond_orders": lig.bond_orders,
                  "charges": lig.charges}
        assert Ligand.from_sdf(record).bond_stereo.shape == (0, 7)
        assert Ligand.from_sdf(record, stereo="coords").bond_stereo.tolist() == lig.bond_stereo.tolist()
    # aromatisation carries the table through
    cinnamic = Ligand.from_smiles("OC(=O)/C=C/C1=CC=CC=C1")
    assert cinnamic.aromatized("cuda").bond_stereo.tolist() == cinnamic.bond_stereo.tolist() and len(cinnamic.bond_stereo) == 1


# ---------------------------------------------------------------------- the keywords of redock
@pytest.fixture(scope="module")
def small(small_model_inputs):
    from physdock_amd import PhysDock
    cfg, P_, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P_, strict=True)
    return model.cuda().eval(), {k: v.cuda() for k, v in batch.items()}, cfg


def test_redock_reports_bond_stereo_and_changes_nothing_else(small):
    from physdock_amd import driver
    from physdock_amd.bond_stereo import BondStereo
    model, dbatch, _ = small
    lig = torch.nonzero(driver.ligand_atom_mask(dbatch)).flatten().tolist()
    assert len(lig) >= 4
    spec = BondStereo(np.asarray([lig[:4] + [-1, -1]]), [1], n_atoms=len(lig))
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, dbatch, **kw)
    out = driver.redock(model, dbatch, bond_stereo=spec, **kw)
    assert set(out) == set(plain) | {"bond_stereo"} and set(out["bond_stereo"]) == {"state", "dihedral", "twist", "n_wrong", "n_twisted", "ok"}
    assert all(torch.equal(out[k], plain[k]) for k in ("poses",)) and out["rounds"] == plain["rounds"]
    direct = spec.check(out["poses"])
    assert all(torch.equal(out["bond_stereo"][k], direct[k]) or k in ("dihedral", "twist") for k in out["bond_stereo"])
    assert all(out["bond_stereo"][k].cpu().numpy().tobytes() == direct[k].cpu().numpy().tobytes() for k in ("dihedral", "twist"))
    want = ref.check(out["poses"].cpu().numpy(), spec.quads, spec.expect, spec.max_twist)
    assert np.array_equal(out["bond_stereo"]["state"].cpu().numpy(), want["state"])
    many = driver.redock_many(model, [(dbatch, {"bond_stereo": spec})], group=1, **kw)
    assert set(many[0]) == set(out) and torch.equal(many[0]["bond_stereo"]["state"], spec.check(many[0]["poses"])["state"])
    # a spec over another atom count, or reaching past the batch, is refused before anything is sampled
    with pytest.raises(ValueError, match="ligand atoms"):
        driver.redock(model, dbatch, bond_stereo=BondStereo(np.asarray([lig[:4] + [-1, -1]]), [1], n_atoms=len(lig) + 1), **kw)
    with pytest.raises(ValueError, match="reaches atom"):
        driver.redock(model, dbatch, bond_stereo=BondStereo.from_tables([[0, 1, 2, 10 ** 6, -1, -1]], [1]), **kw)
    with pytest.raises(ValueError, match="needs bond_stereo="):
        driver.redock(model, dbatch, bond_stereo_filter=True, **kw)


def test_bond_stereo_filter_rejects_where_chirality_does(small):
    from physdock_amd import driver
    from physdock_amd.bond_stereo import BondStereo
    from physdock_amd.synthetic import reference_conformers
    model, dbatch, _ = small
    lig = torch.nonzero(driver.ligand_atom_mask(dbatch)).flatten().tolist()
    confs = reference_conformers({k: t.cpu() for k, t in dbatch.items()}, n_conf=6, seed=1).cuda()
    kw = dict(ref_mol_poses=confs, physics_correction=True, max_samples=3, max_rounds=2, num_samples_per_round=3, steps=6, seed=2)
    plain = driver.redock(model, dbatch, **kw)
    quad = lig[:4] + [-1, -1]
    # round 0 is seeded: sample it again and read the planted geometry off it
    x0 = model.sample_diffusion(dbatch, num_sample=3, steps=6, seed=2, align_ref_pos=False, karras_noise_schedule_power=1000,
                                mmff_gamma_0_factor=6.0, ode_step_scale_eta=1.5)
    found = BondStereo.from_tables([quad], None).label(x0)[:, 0].tolist()
    assert all(s in (1, 2) for s in found)
    kind = found[0]
    same = BondStereo(np.asarray([quad]), [kind], n_atoms=len(lig))
    opposite = BondStereo(np.asarray([quad]), [3 - kind], n_atoms=len(lig))
    out = driver.redock(model, dbatch, bond_stereo=same, bond_stereo_filter=True, **kw)
    assert out["rounds"][0]["accepted"] == sum(s == kind for s in found)
    out = driver.redock(model, dbatch, bond_stereo=opposite, bond_stereo_filter=True, **kw)
    assert out["rounds"][0]["accepted"] == sum(s == 3 - kind for s in found)
    # a spec no pose can meet (the same bond expected cis and trans): every pose of every round is rejected
    never = BondStereo(np.asarray([quad, quad]), [1, 2], n_atoms=len(lig))
    out = driver.redock(model, dbatch, bond_stereo=never, bond_stereo_filter=True, **kw)
    assert [r["accepted"] for r in out["rounds"]] == [0, 0] and out["accepted"] == 0 and plain["accepted"] == 3
    assert out["gamma_factor"] == pytest.approx(max(max(6.0 * 0.7, 1.0) * 0.7, 1.0))
    assert not out["bond_stereo"]["ok"].any()
    # reported but not filtered: the rounds are those of the plain call
    rep = driver.redock(model, dbatch, bond_stereo=never, **kw)
    assert rep["rounds"] == plain["rounds"] and torch.equal(rep["poses"], plain["poses"])
