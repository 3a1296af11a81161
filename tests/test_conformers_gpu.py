"""csrc/conformers.hip against tests/conformers_ref.py, and `redock(conformers=)`."""
import functools

import numpy as np
import pytest
import torch

import conformers_ref as cr
from physdock_amd import conformers as pc, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
#: the kernel may differ from the reference by ten times what the reference differs from itself under a relabelling of the atoms
BOUND = 10.0 * cr.RELABEL_SPREAD


@functools.lru_cache(maxsize=None)
def _ens(name, mirror=False):
    c = cr.make_case(name)
    x = c["x_ref"] * np.array([1.0, 1.0, -1.0]) if mirror else c["x_ref"]
    return pc.ConformerEnsemble.from_bonds(c["n_atoms"], c["bonds"], x, c["elements"], bond_orders=c["bond_orders"],
                                           planar_groups=c["planar_groups"], centres=c["centres"], device=DEV)


@pytest.mark.parametrize("name,C", [("chain2", 6), ("chain3", 6), ("chain4", 6), ("centre5", 12), ("toluene7", 6), ("phenyl14", 64),
                                    ("chain63", 6), ("chain64", 6), ("chain65", 6), ("chain128", 6)])
def test_error_and_gradient_parity(name, C):
    t, ens = cr.case_tables(name), _ens(name)
    pts = cr.parity_points(name, C)
    for w_chi, w_4d in cr.STAGES:
        out = ens.error(torch.from_numpy(pts).to(DEV), w_chi, w_4d, gradients=True)
        e_dev, g_dev = out["err"].cpu().numpy(), out["grad"].cpu().numpy()
        only_e = ens.error(torch.from_numpy(pts).to(DEV), w_chi, w_4d)["err"].cpu().numpy()
        assert np.array_equal(only_e, e_dev)
        for k in range(C):
            e, g = cr.error_and_grad(t, pts[k], w_chi, w_4d)
            de, dg = abs(e_dev[k] - e), np.abs(g_dev[k] - g).max()
            print(f"{name} point {k} weights {w_chi, w_4d}: E {e:.6e} diff {de:.2e}; max|g| {np.abs(g).max():.3e} diff {dg:.2e}")
            assert de <= BOUND * abs(e) and dg <= BOUND * np.abs(g).max()


@pytest.mark.parametrize("name", ["centre5", "phenyl14", "chain65"])
def test_error_and_gradient_do_not_depend_on_the_batch(name):
    """C = 1 and C = 2 calls against the reference and, bit for bit, against the same points inside a C = 64 call"""
    t, ens = cr.case_tables(name), _ens(name)
    pts = cr.parity_points(name, 64)
    big = ens.error(torch.from_numpy(pts).to(DEV), 1.0, 0.1, gradients=True)
    for lo, hi in ((5, 6), (2, 4), (63, 64)):
        out = ens.error(torch.from_numpy(pts[lo:hi]).to(DEV), 1.0, 0.1, gradients=True)
        assert torch.equal(out["err"], big["err"][lo:hi]) and torch.equal(out["grad"], big["grad"][lo:hi])
        for k in range(lo, hi):
            e, g = cr.error_and_grad(t, pts[k], 1.0, 0.1)
            assert abs(float(out["err"][k - lo]) - e) <= BOUND * abs(e)
            assert np.abs(out["grad"][k - lo].cpu().numpy() - g).max() <= BOUND * np.abs(g).max()


@pytest.mark.parametrize("name,iters,kind", cr.SHORT_RUNS)
def test_short_runs_from_given_starts(name, iters, kind):
    t, x0, ref = cr.short_reference(name, iters, kind)
    if min(v for _, v in ref["margins"]) < cr.MARGIN_FLOOR:
        pytest.skip("a decision of the reference sits within 1e-9 of its threshold")
    ens = _ens(name)
    start = torch.from_numpy(np.stack([x0, x0])).to(DEV)
    out = ens.embed(2, seed=0, max_iters=iters, start=start, keep=None)
    assert out["iterations"].cpu().tolist() == [ref["iterations"]] * 2 and out["status"].cpu().tolist() == [ref["status"]] * 2
    scale = np.abs(ref["x4"]).max()
    x3 = ref["x4"][:, :3] - ref["x4"][:, :3].mean(0)
    err = out["err"].cpu().numpy()
    print(f"{name}: iterations {ref['iterations']} status {ref['status']} E {ref['err']:.6e} device {err[0]:.6e}")
    # 1e-9 of E, as the margins; E is a sum of squares of residuals that round at 1e-16, so below 1e-24 it holds no digits
    assert abs(err[0] - ref["err"]) <= 1e-9 * abs(ref["err"]) + 1e-24 and err[0] == err[1]
    assert abs(float(out["max_violation"][0]) - ref["max_violation"]) <= 1e-8 * scale
    assert bool(out["ok"][0]) == ref["ok"]
    # the 4-D point the run ended at, accepted or not: a few steps of float64 arithmetic on coordinates of this size
    x4 = out["x4"].cpu().numpy()
    dx = np.abs(x4[0] - ref["x4"]).max()
    print(f"{name}: max|x4 - reference| {dx:.2e} of size {scale:.2e}")
    assert dx <= 1e-8 * scale and np.array_equal(x4[0], x4[1])
    # and its gradient (stage 2's weights), by the parity yardstick at the device's own point; near a minimum the summands cancel,
    # so the scale is the sum of their magnitudes, which is max|g| where they do not
    g = cr.error_and_grad(t, x4[0], *cr.STAGES[1])[1]
    assert np.abs(out["grad4"][0].cpu().numpy() - g).max() <= BOUND * cr.gradient_scale(t, x4[0], *cr.STAGES[1])
    if ref["ok"]:                                   # fp32 rounding of coordinates that agree to 1e-8 of their size
        assert np.abs(out["x"][0].cpu().numpy().astype(np.float64) - x3).max() <= 2.0 ** -23 * scale + 1e-8 * scale
    else:
        assert not out["x"].any()


@functools.lru_cache(maxsize=None)
def _full(name, C=64, seed=11, mirror=False):
    out = _ens(name, mirror).embed(C, seed)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", ["chain4", "centre5", "toluene7", "phenyl14", "chain20"])
def test_full_runs_accept_only_valid_conformers(name):
    t, out = cr.case_tables(name), _full(name)
    assert out["x"].shape == (64, t["lo"].shape[0], 3) and out["poses"].shape[0] == out["ok"].sum()
    assert np.array_equal(out["poses"], out["x"][out["ok"] > 0])
    print(f"{name}: accepted {int(out['ok'].sum())} / 64, iterations mean {out['iterations'].mean(0)}, status counts "
          f"{[np.bincount(out['status'][:, s], minlength=3).tolist() for s in (0, 1)]}")
    for c in range(64):
        x = out["x"][c].astype(np.float64)
        if out["ok"][c]:
            viol, signs, _ = cr.accept_checks(t, x)
            eps = 4.0 * 2.0 ** -24 * np.abs(x).max() * np.sqrt(3.0)          # two endpoints, fp32 rounding of three coordinates
            assert viol <= 0.1 + eps and signs
            assert abs(viol - out["max_violation"][c]) <= eps and np.abs(x.mean(0)).max() <= 1e-5
        else:
            assert not x.any()
        assert set(out["status"][c]) <= {0, 1, 2} and (out["iterations"][c] <= 400).all()
    assert out["ok"].sum() > 0


def test_full_runs_reject_few_where_the_reference_accepts_all():
    checked = 0
    for name in ("chain4", "toluene7"):
        ref = cr.embed(cr.case_tables(name), 64, seed=11)
        if all(r["ok"] for r in ref):
            checked += 1
            assert 64 - int(_full(name)["ok"].sum()) <= 8, name
    assert checked, "the reference accepts all 64 in none of the cases"


def test_full_runs_are_deterministic_and_independent_of_the_batch():
    a = _full("phenyl14")
    b = {k: v.cpu().numpy() for k, v in _ens("phenyl14").embed(64, 11).items()}
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    five = {k: v.cpu().numpy() for k, v in _ens("phenyl14").embed(5, 11, keep=None).items()}
    for k in five:
        assert np.array_equal(five[k], a[k][:5], equal_nan=True), k
    other = _full("phenyl14", seed=12)
    both = (a["ok"] > 0) & (other["ok"] > 0)
    assert both.any() and all(not np.array_equal(a["x"][c], other["x"][c]) for c in np.nonzero(both)[0])


def test_start_is_the_stated_philox_draw():
    t, ens = cr.case_tables("centre5"), _ens("centre5")
    seed = (7 << 32) | 123
    given = torch.from_numpy(np.stack([cr.start(seed, c, 5, t["box"]) for c in range(3)])).to(DEV)
    a = ens.embed(3, seed, max_iters=2, keep=None)
    b = ens.embed(3, 99, max_iters=2, keep=None, start=given)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_mirror_reference_gives_the_other_handedness():
    t = cr.case_tables("phenyl14")
    a, b = _full("phenyl14"), _full("phenyl14", mirror=True)
    assert a["ok"].sum() and b["ok"].sum()
    for out, sign in ((a, 1.0), (b, -1.0)):
        for c in np.nonzero(out["ok"])[0]:
            assert (cr.signed_volumes(out["x"][c].astype(np.float64), t["centres"]) * t["vol_lo"] * sign > 0).all()


def test_refusals_and_exact_workspace():
    L_ = ops._lib.init()
    ens = _ens("centre5")
    t = ens.tables(DEV)
    C, L = 4, 5
    assert L_.pd_embed_conformers_workspace_numel(C, L) == C * (400 + 160)
    assert L_.pd_embed_conformers_workspace_numel(1, 129) == -3 and L_.pd_embed_conformers_workspace_numel(4097, 5) == -3
    assert L_.pd_embed_conformers_workspace_numel(0, 5) == -1
    numel = C * 560
    guard = 64
    ws = torch.full((numel + guard,), -7.25, device=DEV, dtype=torch.float64)
    f = lambda shape, dt, v: torch.full(shape, v, device=DEV, dtype=dt)
    out = dict(x=f((C, L, 3), torch.float32, -7.25), ok=f((C,), torch.uint8, 9), err=f((C,), torch.float64, -7.25),
               viol=f((C,), torch.float64, -7.25), it=f((C, 2), torch.int32, -9), st=f((C, 2), torch.int32, -9))
    p = ops.ptr

    def call(lo=p(t["lo"]), up=p(t["up"]), w=p(ws), n=numel, x=p(out["x"]), c=C, l=L, nc=1, it=50, box=ens.box, okp=p(out["ok"])):
        return L_.pd_embed_conformers(lo, up, p(t["centres"]), p(t["vol_lo"]), p(t["vol_hi"]), 3, it, 1e-4, box, w, n, x, okp,
                                      p(out["err"]), p(out["viol"]), p(out["it"]), p(out["st"]), None, c, l, nc, ops.stream())
    for rc, kw in ((-1, dict(lo=None)), (-1, dict(w=None)), (-1, dict(x=None)), (-1, dict(okp=None)), (-1, dict(n=numel - 1)),
                   (-1, dict(c=0)), (-1, dict(it=-1)), (-1, dict(box=0.0)), (-1, dict(lo=p(t["lo"]) + 4)), (-1, dict(x=p(out["x"]) + 2)),
                   (-3, dict(l=129)), (-3, dict(c=4097)), (-3, dict(nc=65))):
        assert call(**kw) == rc, kw
    torch.cuda.synchronize()
    assert (ws == -7.25).all() and (out["x"] == -7.25).all() and (out["ok"] == 9).all() and (out["it"] == -9).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (ws[numel:] == -7.25).all() and not (ws[:numel] == -7.25).all()
    ref = ens.embed(C, 3, max_iters=50, keep=None)
    assert torch.equal(out["x"], ref["x"]) and torch.equal(out["ok"], ref["ok"]) and torch.equal(out["it"], ref["iterations"])
    pos = torch.zeros(1, L, 4, device=DEV, dtype=torch.float64)
    e = torch.full((1,), -7.25, device=DEV, dtype=torch.float64)
    eg = lambda **k: L_.pd_dg_error_grad(k.get("lo", p(t["lo"])), p(t["up"]), p(t["centres"]), p(t["vol_lo"]), p(t["vol_hi"]),
                                         k.get("pos", p(pos)), 1.0, 0.1, k.get("e", p(e)), None, k.get("c", 1), k.get("l", L), 1, ops.stream())
    assert eg(lo=None) == -1 and eg(pos=None) == -1 and eg(e=None) == -1 and eg(c=0) == -1 and eg(l=129) == -3 and eg(c=4097) == -3
    torch.cuda.synchronize()
    assert float(e[0]) == -7.25


def test_redock_takes_its_pool_from_the_ensemble():
    from physdock_amd import PhysDock, param_shapes, redock, seeded_state_dict, small_config
    from physdock_amd.synthetic import small_batch
    cfg = small_config()
    model = PhysDock(cfg)
    model.load_state_dict(seeded_state_dict(param_shapes(cfg), seed=0), strict=True)
    model = model.to(DEV).eval()
    batch = {k: v.to(DEV) for k, v in small_batch(0).items()}
    kw = dict(physics_correction=True, max_rounds=2, num_samples_per_round=2, max_samples=2, steps=4, seed=5, ranking=False,
              accept_fn=lambda x: False)
    with pytest.raises(ValueError, match="ETKDG"):
        redock(model, batch, **kw)
    c = cr.make_case("chain6")
    ens = pc.ConformerEnsemble.from_bonds(6, c["bonds"], c["x_ref"], c["elements"], device=DEV)
    out = redock(model, batch, conformers=ens, **kw)
    log = out["conformers"]
    assert log["embedded"] == 128 and 0 < log["accepted"] <= 128 and log["max_violation"].shape == (128,)
    assert int(log["ok"].sum()) == log["accepted"] and out["poses"].shape[0] == 2 and len(out["rounds"]) == 2
    assert out["rounds"][1]["templates"] > 0
    with pytest.raises(ValueError, match="atoms"):
        redock(model, batch, conformers=_ens("centre5"), **kw)
    plain = redock(model, batch, steps=4, num_samples_per_round=2, max_samples=2, seed=5, ranking=False)
    assert "conformers" not in plain
