"""pd_distogram_* (csrc/distogram_score.hip) through DistogramScore, PhysDock.predict_distogram, and the distogram keyword of redock /
redock_many.

The yardstick is the float64 definition tests/distogram_score_ref.py.  Every integer output must EQUAL it.  Every fp32 output must lie
within one fp32 ulp of the definition's value rounded to fp32: the arithmetic is float64 on both sides and of the same terms - only exp
and log differ in the last bits of a double and the device sums in a fixed tree, about 1e-15 relative over at most T^2 non-negative
terms, which can move a value across one fp32 rounding boundary and no further.  Forces sum terms of both signs, so they get the
larger of one ulp of the value and 1e-12 of abs_force, the magnitude of what they are summed from.

Shapes: T = 24 (16 receptor tokens of 4 to 5 atoms, 8 ligand tokens of one atom: two tiles of four rows per pose), P = 5, K = 39;
T = 17 gives 289 pairs: one full 256-pair block of the table kernel and a tail; K = 8 and K = 64 (the limit, above the default LDS of
a block); the reference of a case is computed once and shared."""
import numpy as np
import pytest
import torch

import distogram_score_ref as ref

pytestmark = pytest.mark.gpu

FLOATS = ("nll_interface", "nll_ligand", "nll_receptor", "nll", "token_nll", "expected_error", "contact_recovery", "contact_precision")
INTS = ("n_pairs", "n_contacts", "ok", "bins")


def within_ulps(got, want, n=1, floor=None):
    """|got - want| <= n fp32 ulps of want (or `floor`, whichever is larger), NaN exactly where want is NaN; returns the worst excess"""
    g, w = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert g.shape == w.shape, (g.shape, w.shape)
    assert np.array_equal(np.isnan(g), np.isnan(w)), "NaN in other places"
    ok = ~np.isnan(w)
    tol = n * np.spacing(np.abs(w[ok])).astype(np.float64)
    if floor is not None:
        tol = np.maximum(tol, np.broadcast_to(np.asarray(floor, np.float64), w.shape)[ok])
    err = np.abs(g[ok].astype(np.float64) - w[ok].astype(np.float64))
    return float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0


def cases():
    base = ref.make_case()
    signs = dict(base, logits=np.where(base["logits"] > 0, np.float32(80), np.float32(-80)))
    masked = dict(base, pb=base["pb"].copy(), s_mask=base["s_mask"].copy())
    masked["pb"][2], masked["s_mask"][5], masked["s_mask"][20] = -1, 0, 0
    broken = dict(base, x=base["x"].copy())
    broken["x"][1, base["pb"][0], 1] = np.nan                     # an active pseudo-beta atom: ok = 0
    broken["x"][3, base["pb"][18], 2] = np.inf                    # a ligand token's
    broken["x"][2, base["pb"][0] + 1, 0] = np.nan                 # nobody's pseudo-beta atom: unaffected
    edge, _ = ref.edge_pairs_case()
    return {
        "base": (base, {}),
        "T17": (ref.make_case(T_rec=12, T_lig=5, seed=1), {}),
        "K8": (ref.make_case(K=8, seed=2), {}),
        "K64": (ref.make_case(K=64, seed=3), {}),
        "P1": (ref.make_case(P=1, seed=4), {}),
        "logits80": (signs, {}),
        "masked": (masked, {}),
        "no_ligand": (dict(base, is_ligand=np.zeros(24, np.float32)), {}),
        "receptor": (base, {"receptor": True}),
        "no_ligand_receptor": (dict(base, is_ligand=np.zeros(24, np.float32)), {"receptor": True}),
        "edge_pairs": (edge, {}),
        "not_finite": (broken, {}),
        "cutoff_below_the_first_edge": (base, {"contact_cutoff": 3.0, "max_expected": 12.0}),
    }


CASES = cases()


@pytest.fixture(scope="module")
def restated():
    """a case's definition-side spec and results, computed once and left unchanged"""
    memo = {}

    def get(name):
        if name not in memo:
            c, kw = CASES[name]
            spec = ref.Spec(c["logits"], c["pb"], c["is_ligand"], c["s_mask"], **kw)
            memo[name] = (spec, spec.score(c["x"], detail=True), spec.potential(c["x"], forces=True))
        return memo[name]
    return get


def device_spec(c, **kw):
    from physdock_amd import DistogramScore
    batch = {"token_id_to_pseudo_beta_atom_id": torch.from_numpy(c["pb"]), "is_ligand": torch.from_numpy(c["is_ligand"]),
             "s_mask": torch.from_numpy(c["s_mask"]), "x_gt": torch.from_numpy(c["x"][0])}
    return DistogramScore.from_logits(torch.from_numpy(c["logits"]).cuda(), batch, **kw)


def host(d):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_every_output_against_the_definition(name, restated):
    c, kw = CASES[name]
    spec, want, want_pot = restated(name)
    dev = device_spec(c, **kw)
    x = torch.from_numpy(c["x"]).cuda()
    t = dev.tables("cuda")
    lse = t["lse"].cpu().numpy()
    assert np.isfinite(lse).all() and np.abs(lse - spec.lse).max() <= 1e-14 * np.abs(spec.lse).max()
    print(name, "tables: expected", within_ulps(t["expected"].cpu().numpy(), spec.expected), "p_contact",
          within_ulps(t["p_contact"].cpu().numpy(), spec.p_contact), "ulp")
    assert within_ulps(t["expected"].cpu().numpy(), spec.expected) <= 1 and within_ulps(t["p_contact"].cpu().numpy(), spec.p_contact) <= 1
    got = host(dev.score(x, detail=True))
    assert set(got) == set(FLOATS) | set(INTS)
    for k in INTS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    for k in FLOATS:
        worst = within_ulps(got[k], want[k])
        print(name, k, f"{worst:.2f} ulp")
        assert worst <= 1, (k, worst)
    assert "bins" not in dev.score(x)
    pot = host(dev.potential(x, forces=True))
    assert set(pot) == {"potential", "forces", "abs_force"} and set(dev.potential(x)) == {"potential"}
    wp, wf, wa = within_ulps(pot["potential"], want_pot["potential"]), None, within_ulps(pot["abs_force"], want_pot["abs_force"])
    floor = 1e-12 * np.nan_to_num(want_pot["abs_force"].astype(np.float64))[..., None]
    wf = within_ulps(pot["forces"], want_pot["forces"], floor=floor)
    print(name, f"potential {wp:.2f} ulp, abs_force {wa:.2f} ulp, forces {wf:.2f} of max(1 ulp, 1e-12 abs_force)")
    assert wp <= 1 and wa <= 1 and wf <= 1
    if name == "logits80":
        # (a mean: about half of a pose's pairs sit in a bin 160 below the largest logit of their row)
        assert np.isfinite(got["nll_interface"]).all() and got["nll_interface"].min() > 40
    if name == "masked":
        assert list(got["n_pairs"]) == [7 * 14, 21, 0] and (got["bins"][:, :, [2, 5, 20]] == 255).all()
    if name.startswith("no_ligand"):
        assert np.isnan(got["nll_interface"]).all() and np.isnan(got["nll_ligand"]).all() and list(got["n_pairs"][:2]) == [0, 0]
        assert np.isnan(pot["potential"]).all() and pot["forces"].shape == (5, 0, 3) and (got["ok"] == 1).all()
        assert np.isnan(got["nll"]).all() == (name == "no_ligand") and got["n_pairs"][2] == (0 if name == "no_ligand" else 276)
    if name == "edge_pairs":
        assert list(got["bins"][0, :, 0]) == [0, 1, 38, 0]
    if name == "not_finite":
        assert list(got["ok"]) == [1, 0, 1, 0, 1] and np.isnan(pot["forces"][[1, 3]]).all() and np.isfinite(pot["forces"][[0, 2, 4]]).all()
        clean = host(device_spec(CASES["base"][0]).score(torch.from_numpy(CASES["base"][0]["x"]).cuda(), detail=True))
        assert all(np.array_equal(got[k][2], clean[k][2], equal_nan=True) for k in FLOATS + ("n_contacts", "bins")), "pose 2 is unaffected"


def test_the_kernels_refuse_what_they_do_not_take():
    from physdock_amd import DistogramScore, ops
    c = CASES["base"][0]
    with pytest.raises(ValueError, match="2 .. 64 bins"):
        device_spec(dict(c, logits=np.zeros((24, 24, 65), np.float32)))
    L = ops._lib.init()
    dev = device_spec(c)
    t = dev.tables("cuda")
    lse = torch.full((24, 24), -7.0, dtype=torch.float64, device="cuda")
    big = torch.zeros(24, 24, 65, device="cuda")
    centres = (ops.C.c_double * 65)(*range(65))
    P = ops.ptr
    assert L.pd_distogram_tables(P(big), centres, 3, P(lse), P(t["expected"]), P(t["p_contact"]), 24, 65, ops.stream()) == -3
    assert L.pd_distogram_tables(P(big), centres, 3, P(lse), P(t["expected"]), P(t["p_contact"]), 4097, 39, ops.stream()) == -3
    torch.cuda.synchronize()
    assert bool((lse == -7.0).all()), "a refused call wrote"


def test_a_pose_gives_the_same_bits_whatever_the_batch(restated):
    c, _ = CASES["base"]
    dev = device_spec(c, receptor=True)
    x = torch.from_numpy(c["x"]).cuda()
    whole, again, head = (host(dict(dev.score(v, detail=True), **dev.potential(v, forces=True))) for v in (x, x.clone(), x[:2]))
    mid = host(dict(dev.score(x[3:4], detail=True), **dev.potential(x[3:4], forces=True)))
    for k in whole:
        if k == "n_pairs":
            continue
        a, b, h, m = (v[k].view(np.uint8) if v[k].dtype == np.uint8 else v[k].view(np.int32) for v in (whole, again, head, mid))
        assert np.array_equal(a, b), f"{k}: two identical calls differ"
        assert np.array_equal(a[:2], h), f"{k}: poses [0:2] differ from the rows of the call with P = 5"
        assert np.array_equal(a[3:4], m), f"{k}: pose 3 alone differs from its row"


# ------------------------------------------------------------------ the small model: logits at inference, redock, redock_many
@pytest.fixture(scope="module")
def small(small_model_inputs):
    from physdock_amd import PhysDock
    cfg, P_, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P_, strict=True)
    return model.cuda().eval(), {k: v.cuda() for k, v in batch.items()}, cfg


def same_result(u, w):
    """the same keys and, tensor by tensor, the same bits (a NaN equals itself)"""
    if isinstance(u, torch.Tensor):
        raw = lambda t: t.detach().contiguous().view(-1).view(torch.uint8)
        return isinstance(w, torch.Tensor) and u.dtype == w.dtype and u.shape == w.shape and torch.equal(raw(u), raw(w))
    if isinstance(u, dict):
        return isinstance(w, dict) and set(u) == set(w) and all(same_result(u[k], w[k]) for k in u)
    if isinstance(u, (list, tuple)):
        return len(u) == len(w) and all(same_result(a, b) for a, b in zip(u, w))
    return u == w or (isinstance(u, float) and isinstance(w, float) and u != u and w != w)


def test_predict_distogram_is_forwards_head(small):
    model, batch, cfg = small
    torch.manual_seed(0)
    want = model.forward(batch)["p_distogram"]
    T = batch["target_feat"].shape[0]
    assert want.shape == (T, T, cfg.loss.distogram_loss["no_bins"]) and want.dtype == torch.float32
    got = model.predict_distogram(batch)
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))
    _, cond = model.sample_diffusion(batch, num_sample=1, steps=2, seed=0, return_conditioning=True)
    for c in (cond, cond[2:]):
        again = model.predict_distogram(batch, conditioning=c)
        assert torch.equal(again.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got, got.transpose(0, 1)), "symmetrised"
    with pytest.raises(ValueError, match="the conditioning's z has shape"):
        model.predict_distogram(batch, conditioning=(cond[2], cond[3][:-1]))


def test_redock_ranks_by_the_distogram_and_changes_nothing_else(small):
    from physdock_amd import DistogramScore, PoseClusters, driver
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.ranking import rank_by_score
    from physdock_amd.sdfio import SdfTemplate, parse_sdf
    from physdock_amd.validity import PoseValidity
    model, batch, _ = small
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, batch, **kw)
    assert set(plain) == {"poses", "accepted", "rounds", "gamma_factor", "ranking"}
    assert same_result(driver.redock(model, batch, **kw), plain), "two calls without the keyword: the same keys, the same bits"
    out = driver.redock(model, batch, distogram=True, **kw)
    assert set(out) == set(plain) | {"distogram", "order_distogram"}
    assert same_result({k: out[k] for k in plain}, plain), "unchanged key for key"
    d = out["distogram"]
    assert set(d) == set(driver.DISTOGRAM_KEYS) and d["nll_interface"].shape == (4,) and d["token_nll"].shape == (4, batch["is_ligand"].shape[0])
    nll = d["nll_interface"].cpu()
    order = out["order_distogram"].cpu().tolist()
    assert sorted(order) == [0, 1, 2, 3] and out["order_distogram"].is_cuda and bool(torch.isfinite(nll).all())
    assert all(nll[order[i]] <= nll[order[i + 1]] for i in range(3)) and torch.equal(out["order_distogram"], rank_by_score(d["nll_interface"]))
    direct = DistogramScore.from_batch(model, batch)
    sc = direct.score(out["poses"])
    assert all(torch.equal(d[k].view(torch.int32), sc[k].view(torch.int32)) for k in driver.DISTOGRAM_KEYS[:-1])
    assert torch.equal(d["potential"], direct.potential(out["poses"])["potential"])
    worst = direct.describe(d, order[0])
    assert len(worst) == int(batch["is_ligand"].sum()) and worst[0][1] >= worst[-1][1]
    # validity, clusters and the SD item
    n = int(ligand_atom_mask(batch).sum())
    chain = [(i, i + 1) for i in range(n - 1)]
    t = SdfTemplate.from_batch(batch, chain, title="small")
    full = driver.redock(model, batch, distogram={"receptor": True, "contact_cutoff": 10.0}, sdf=t, validity=PoseValidity.from_batch(batch, chain),
                         clusters=PoseClusters(2.0, by="distogram"), **kw)
    assert set(full) == set(plain) | {"distogram", "order_distogram", "order_distogram_valid", "validity", "clusters", "sdf"}
    assert torch.equal(full["poses"], plain["poses"])
    assert torch.equal(full["order_distogram_valid"], rank_by_score(full["distogram"]["nll_interface"], valid=full["validity"]["valid"]))
    assert torch.equal(full["distogram"]["nll_interface"], d["nll_interface"]), "the interface does not see the receptor class"
    back = parse_sdf("".join(SdfTemplate.split(full["sdf"])))
    assert len(back) == 4
    for p, r in enumerate(back):
        assert float(r["properties"]["distogram_nll"]) == pytest.approx(float(nll[p]), rel=1e-4, abs=1e-4)
    # redock_many: the sequential, the two-stream and the grouped route
    many = driver.redock_many(model, [(batch, {"distogram": True})], **kw)
    assert same_result(many[0], out)
    two = driver.redock_many(model, [(batch, {"distogram": True}), (batch, {})], streams=2, **kw)
    assert same_result(two[0], out) and same_result(two[1], plain)
    grouped = driver.redock_many(model, [(batch, {"distogram": True}), (batch, {})], group=2, **kw)
    bare = driver.redock_many(model, [(batch, {}), (batch, {})], group=2, **kw)
    assert set(grouped[0]) == set(out) and set(grouped[1]) == set(plain) == set(bare[0])
    assert same_result(grouped[1], bare[1]) and same_result({k: grouped[0][k] for k in plain}, bare[0]), "the grouped route without the keyword"
    g = grouped[0]["distogram"]
    assert set(g) == set(driver.DISTOGRAM_KEYS) and sorted(grouped[0]["order_distogram"].cpu().tolist()) == [0, 1, 2, 3]
    assert torch.equal(grouped[0]["order_distogram"], rank_by_score(g["nll_interface"])) and bool(torch.isfinite(g["nll_interface"]).all())
