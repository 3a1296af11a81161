"""tests/loss_ref.py and tests/loss_cases.py on the reference alone (no GPU): the float64 definition the kernel-level loss tests
compare with is pinned to the existing restatement (test_loss_cpu.restate_f64), to the stored float64 gradients of the g16
fixtures, to torch float64 autograd and to central differences; every case meets the conditions the GPU comparison relies on; the
case table reaches the branches it names."""
import numpy as np
import pytest

import loss_cases as lc
import loss_ref as lr
from test_loss_cpu import CASES, load_case, restate_f64
from test_loss_grad_cpu import GRAD_CASES, load_grad

F64_BAR = 1e-10               # two float64 evaluations of one formula (tests/test_loss_cpu.py)
SETTINGS = dict(clamp=15.0, sd=16.0, eps=1e-9, min_bin=3.25, max_bin=50.75, no_bins=39)     # the fixtures' configuration


def aligned_f64(g):
    """(x_gt_aligned [B,A,3], weights [A]) of a fixture, the alignment as restate_f64 forms it (NaN where a sample is not finite)"""
    xd, xg, ex = (g[k].astype(np.float64) for k in ("x_denoised", "x_gt", "x_exists"))
    w = (1 + g["is_dna"] * 5.0 + g["is_rna"] * 5.0 + g["is_ligand"] * 10.0)[g["atom_id_to_token_id"]] * ex
    al = np.full_like(xd, np.nan)
    for b in range(xd.shape[0]):
        xp = xd[b] * ex[:, None]
        if not np.isfinite(xp).all():
            continue
        mu_p, mu_g = w @ xp / w.sum(), w @ xg / w.sum()
        U, _, Vh = np.linalg.svd((xg - mu_g).T @ (w[:, None] * (xp - mu_p)))
        R = U @ Vh
        if np.linalg.det(R) < 0:
            R = U @ np.diag([1.0, 1.0, -1.0]) @ Vh
        al[b] = (xg - mu_g) @ R + mu_p
    return al, w


def fixture_args(g):
    s = SETTINGS
    b2 = np.linspace(s["min_bin"], s["max_bin"], s["no_bins"] - 1) ** 2
    return dict(centre=(g["x_denoised"], g["x_gt"], g["token_id_to_centre_atom_id"], g["token_bonds"], g["is_key_res"], g["is_ligand"],
                        g["t_hat"], s["sd"], s["sd"], s["eps"]),
                smooth=(g["x_denoised"], g["x_gt"], g["x_exists"], s["clamp"]),
                disto=(g["p_distogram"], g["x_gt"], g["x_exists"], g["token_id_to_pseudo_beta_atom_id"], b2, s["no_bins"]))


@pytest.mark.parametrize("name", CASES)
def test_forward_equals_the_restatement_on_the_g15_fixtures(name):
    from physdock_amd import PhysDockConfig
    g = load_case(name)
    want = restate_f64(g, PhysDockConfig(model_name="medium").loss)
    a = fixture_args(g)
    al, w = aligned_f64(g)
    with np.errstate(invalid="ignore"):
        bond, key = lr.centre_pairs(*a["centre"])
        mine = {"weighted_mse_loss": lr.weighted_mse(g["x_denoised"], al, w, g["t_hat"]), "smooth_lddt_loss": lr.smooth_lddt(*a["smooth"]),
                "bond_loss": bond, "key_res_loss": key, "distogram_loss": lr.distogram(*a["disto"])}
    for t, v in want.items():
        print(f"{name} {t}: loss_ref {mine[t]!r} restate_f64 {v!r}")
        if np.isnan(v):
            assert np.isnan(mine[t]), t
        else:
            assert abs(mine[t] - v) <= F64_BAR * abs(v), t


#: max(0, |loss_ref - g64| - allowance) / max|g64| over all g16 cases, terms and stored rows: measured 7.95e-15 (cfg1, rows of
#: 2 048 pair terms), asserted with a factor of ten.  The fixtures' generator added the pair terms of a row with a BLAS product,
#: loss_ref adds them with numpy's own summation (no BLAS on this side), so the figure is the rounding of two summation orders
G16_MEASURED = 7.95e-15
G16_BAR = 10 * G16_MEASURED


@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradients_reproduce_the_stored_g64_rows(name):
    """Measured per case (worst term and row, relative to max|g64| of the sample): small 4.4e-16, ragged 1.1e-15, cfg1 8.0e-15,
    degenerate 4.5e-16, nan 1.2e-16, clamped 4.4e-16, shared-centre 4.4e-16, grad-only-p 1.2e-16: the two restatements differ by
    rounding only, nine orders of magnitude below the kernels' 2e-5 bar.  The recorded allowances agree to 1e-10."""
    g, inp = load_grad(name)
    rows, prow, tau = g["rows"], g["prow"], float(g["tau"])
    a = fixture_args(inp)
    B = inp["x_denoised"].shape[0]
    worst = 0.0

    def excess(mine, t, allow=None):
        absmax = np.asarray(g["absmax_" + t], dtype=np.float64)
        absmax = absmax[rows] if absmax.ndim else absmax
        d = np.abs(mine - g["g64_" + t]) - (allow[..., None] if allow is not None else 0.0)
        d = np.maximum(d, 0.0).reshape(len(mine), -1).max(1) if absmax.ndim else np.maximum(d, 0.0).max()
        return float(np.max(np.where(absmax > 0, d / np.where(absmax > 0, absmax, 1.0), np.where(d == 0, 0.0, np.inf))))
    if g["has_weighted_mse_loss"]:
        al, w = aligned_f64(inp)
        worst = max(worst, excess(lr.weighted_mse_grad(inp["x_denoised"], al, w, inp["t_hat"])[rows], "weighted_mse_loss"))
    if g["has_smooth_lddt_loss"]:
        mine, allow = lr.smooth_lddt_grad(*a["smooth"], tau, rows=rows)
        assert np.abs(allow - g["allow_smooth_lddt_loss"]).max() <= F64_BAR * max(np.abs(allow).max(), 1e-300)
        worst = max(worst, excess(mine, "smooth_lddt_loss", g["allow_smooth_lddt_loss"]))
    if g["has_bond_loss"] or g["has_key_res_loss"]:
        gb, gk, allow = lr.centre_pairs_grad(*a["centre"], tau, rows=rows)
        if g["has_bond_loss"]:
            worst = max(worst, excess(gb, "bond_loss"))
        if g["has_key_res_loss"]:
            worst = max(worst, excess(gk, "key_res_loss", g["allow_key_res_loss"]))
    if g["has_distogram_loss"]:
        worst = max(worst, excess(lr.distogram_grad(*a["disto"])[prow][None], "distogram_loss"))
    print(f"{name}: worst excess over max|g64| {worst:.3e} (B = {B})")
    assert worst <= G16_BAR
    assert G16_BAR <= 1e-3 * lc.TOL                       # three orders of magnitude below the kernels' bar, or the restatement is wrong


def _autograd(fn, leaf):
    import torch
    x = torch.tensor(np.asarray(leaf, dtype=np.float64), requires_grad=True)
    vals = fn(x)
    vals = vals if isinstance(vals, tuple) else (vals,)
    return [torch.autograd.grad(v, x, retain_graph=True)[0].numpy() for v in vals]


def test_closed_forms_equal_torch_autograd():
    """one small case per term; 65x5 holds two tokens predicted at one point (torch.norm at 0: zero direction) and 63x2-hi sits
    above the clamp of the weighted MSE (no gradient)"""
    c, r = lc.smooth("65x4"), lc.smooth_ref("65x4")
    (ga,) = _autograd(lambda x: lr.torch_smooth_lddt(x, c.x_gt, c.x_exists, lc.CLAMP), c.x_denoised)
    assert np.abs(ga - r.g).max() <= F64_BAR * np.abs(r.g).max()
    c, r = lc.centre("65x5"), lc.centre_ref("65x5")
    gb, gk = _autograd(lambda x: lr.torch_centre_pairs(x, *lc.centre_args(c)[1:]), c.x_denoised)
    assert np.abs(gb - r.g_bond).max() <= F64_BAR * np.abs(r.g_bond).max() and np.abs(gk - r.g_key).max() <= F64_BAR * np.abs(r.g_key).max()
    assert np.isfinite(gb).all() and np.isfinite(gk).all()
    for name in ("39x33", "2x16"):
        c, r = lc.disto(name), lc.disto_ref(name)
        (gp,) = _autograd(lambda p: lr.torch_distogram(p, *lc.disto_args(c)[1:]), c.p_distogram)
        assert np.abs(gp - r.g).max() <= F64_BAR * np.abs(r.g).max()
    for name in ("63x2-lo", "63x2-hi"):
        c, r = lc.mse(name), lc.mse_ref(name)
        (gm,) = _autograd(lambda x: lr.torch_weighted_mse(x, *lc.mse_args(c)[1:]), c.x_denoised)
        assert np.abs(gm - r.g).max() <= F64_BAR * max(np.abs(r.g).max(), 1e-300)
        assert (name.endswith("hi")) == (not np.abs(r.g).any())


def test_gradients_agree_with_central_differences():
    """h = 1e-6, at coordinates of atoms that sit in no pair with |d - d_gt| < 1e-3 (test_loss_grad_cpu's rule), one new case per
    term; the bar is that test's 1e-5 of max|g|"""
    h = 1e-6
    rng = np.random.RandomState(0)

    def fd(f, x, idx):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        return (f(xp) - f(xm)) / (2 * h)

    def away(xd, xg, atoms=None):
        ok = []
        for b in range(xd.shape[0]):
            xa, ga = (xd[b], xg) if atoms is None else (xd[b][atoms], xg[atoms])
            dl = np.abs(lr.pairdist(xa) - lr.pairdist(ga))
            np.fill_diagonal(dl, np.inf)
            ok += [(b, int(i if atoms is None else atoms[i])) for i in np.nonzero(dl.min(1) > 1e-3)[0]]
        return [ok[k] + (int(rng.randint(3)),) for k in rng.choice(len(ok), 6, replace=False)]
    c, r = lc.smooth("129x11"), lc.smooth_ref("129x11")
    xd = c.x_denoised.astype(np.float64)
    for idx in away(xd, c.x_gt.astype(np.float64)):
        d = fd(lambda x: lr.smooth_lddt(x, c.x_gt, c.x_exists, lc.CLAMP), xd, idx)
        assert abs(d - r.g[idx]) <= 1e-5 * np.abs(r.g).max(), ("smooth", idx, d, r.g[idx])
    c, r = lc.centre("130x9"), lc.centre_ref("130x9")
    xd = c.x_denoised.astype(np.float64)
    for idx in away(xd, c.x_gt.astype(np.float64), c.centre):
        db, dk = (fd(lambda x: lr.centre_pairs(x, *lc.centre_args(c)[1:])[k], xd, idx) for k in (0, 1))
        assert abs(db - r.g_bond[idx]) <= 1e-5 * np.abs(r.g_bond).max() and abs(dk - r.g_key[idx]) <= 1e-5 * np.abs(r.g_key).max(), idx
    c, r = lc.disto("38x17"), lc.disto_ref("38x17")
    p = c.p_distogram.astype(np.float64)
    for idx in [(0, 1, 0), (3, 7, 5), (10, 4, 37), (16, 16, 12), (4, 4, 20), (2, 5, 3)]:
        d = fd(lambda q: lr.distogram(q, *lc.disto_args(c)[1:]), p, idx)
        assert abs(d - r.g[idx]) <= 1e-5 * np.abs(r.g).max(), ("distogram", idx, d, r.g[idx])
    c, r = lc.mse("257x3-lo"), lc.mse_ref("257x3-lo")
    xd = c.x_denoised.astype(np.float64)
    for idx in [(0, 0, 0), (1, 1, 2), (2, 256, 1), (1, 100, 0)]:
        d = fd(lambda x: lr.weighted_mse(x, *lc.mse_args(c)[1:]), xd, idx)
        assert abs(d - r.g[idx]) <= 1e-5 * np.abs(r.g).max(), ("mse", idx, d, r.g[idx])
    assert r.g[1, 1].tolist() == [0.0, 0.0, 0.0] and c.weights[1] == 0


def _ratio(allow, g):
    l1 = np.abs(g).reshape(g.shape[0], -1).sum(1)
    return max(float(a.sum() / n) if n > 0 else (0.0 if a.sum() == 0 else np.inf) for a, n in zip(allow, l1))


@pytest.mark.parametrize("name", lc.SMOOTH_GRAD)
def test_smooth_lddt_cases_meet_their_conditions(name):
    c, r = lc.smooth(name), lc.smooth_ref(name)
    assert r.clamp_margin > 1e-5
    assert _ratio(r.allow, r.g) <= 0.01
    assert not r.allow.any()              # stricter than the cap: the cases are built without a sign tie (loss_cases.untie)
    assert np.isfinite(r.g).all() and np.isfinite(r.value) and r.value > 0
    dgt = lr.pairdist(c.x_gt.astype(np.float64))
    if c.A >= 257:
        assert (dgt < lc.CLAMP).any() and (dgt > lc.CLAMP).any()           # both sides of the clamp
    if name == "half":
        assert sorted(np.nonzero(c.x_exists == 0.5)[0].tolist()) == [3, 64]
    if name == "tile-off":
        assert not c.x_exists[64:128].any() and c.x_exists[:64].all() and c.x_exists[128:].all() and not np.abs(r.g[:, 64:128]).any()
    if name == "far-tile":
        assert (dgt[:128, 128:] > lc.CLAMP).all() and (dgt[128:, 128:] < lc.CLAMP).any()
    if c.near:
        i, j = c.near
        d = c.x_denoised[:, j].astype(np.float64) - c.x_denoised[:, i].astype(np.float64)
        assert (d == [float(np.float32(1e-20)), 0.0, 0.0]).all() and (c.x_denoised[:, i] == 0).all()
        assert np.float32(1e-20) ** 2 < np.finfo(np.float32).tiny and np.float32(1e-20) * np.float32(1e-20) > 0     # a subnormal d2
        assert c.x_exists[i] == c.x_exists[j] == 1 and dgt[i, j] < lc.CLAMP and i // 64 == (0 if name == "near-in" else j // 64 - 1)
        # the pair's own contribution is far above the bar: a kernel that drops it fails
        k = 1.0 / c.B / (1e-9 + lr.lddt_mask(c.x_gt, c.x_exists, lc.CLAMP)[1].sum())
        assert k * 2 * lr.deps4(dgt[i, j]) > 100 * lc.TOL * np.abs(r.g).reshape(c.B, -1).max(1).max()


def test_smooth_lddt_forward_only_case():
    r = lc.smooth_ref("2881x1", False)
    assert r.clamp_margin > 1e-5 and np.isfinite(r.value)


@pytest.mark.parametrize("name", lc.CENTRE)
def test_centre_cases_meet_their_conditions(name):
    c, r = lc.centre(name), lc.centre_ref(name)
    assert c.A == c.T + 7 and _ratio(r.allow, r.g_key) <= 0.01 and not r.allow.any()
    assert len(set(c.centre.tolist())) > 1 or c.T == 1
    if c.T > 2:
        assert (np.diff(c.centre) < 0).any() and (np.diff(c.centre) > 0).any()
    if name == "1x1":
        assert r.bond == 0.0 and r.key > 0 and not np.abs(r.g_bond).any() and not np.abs(r.g_key).any()
    if name == "63x3":
        assert not c.token_bonds.any() and not c.is_key_res.any() and r.bond == 0.0 and r.key == 0.0
    if name == "64x4":
        assert c.is_key_res[5] == c.is_ligand[5] == 1
    if name == "65x5":
        assert (c.x_denoised[:, c.centre[7]] == c.x_denoised[:, c.centre[40]]).all() and c.centre[7] != c.centre[40]
        assert c.token_bonds[7, 40] == 1 and c.token_bonds[40, 7] == 0 and c.is_key_res[7] == c.is_ligand[40] == 1
    if name == "257x2":
        assert c.centre[3] == c.centre[100] == c.centre[256] and 3 // 256 != 256 // 256
        assert len(set(c.centre.tolist())) == c.T - 2
    if c.T >= 64:
        assert (c.token_bonds != c.token_bonds.T).any() and r.bond > 0 and r.key > 0
        assert ((c.token_bonds + c.token_bonds.T) == 1).any()              # pairs bonded in one orientation only
    assert sum(lc.centre(n).T >= 64 and bool((lc.centre(n).token_bonds != lc.centre(n).token_bonds.T).any()) for n in lc.CENTRE) >= 2


@pytest.mark.parametrize("name", lc.DISTO)
def test_distogram_cases_meet_their_conditions(name):
    c, r = lc.disto(name), lc.disto_ref(name)
    assert r.bin_margin > 1e-5 and np.isfinite(r.g).all() and np.isfinite(r.value)
    assert np.array_equal(c.boundaries_sq, (np.linspace(lc.MIN_BIN, lc.MAX_BIN, c.no_bins - 1, dtype=np.float32) ** 2))
    if c.T >= 15:
        assert c.x_exists[c.pseudo_beta[2]] == 0 and (c.p_distogram[2] == np.float32(1e30)).all() and (c.p_distogram[:, 2] == np.float32(1e30)).all()
        assert c.x_exists[c.pseudo_beta[4]] == 0.5 and not np.abs(r.g[2]).any() and not np.abs(r.g[:, 2]).any()
        assert (np.diff(c.pseudo_beta) < 0).any() and (np.diff(c.pseudo_beta) > 0).any()


def test_distogram_table_covers_every_bin_count_and_size_twice():
    for nb in (2, 3, 38, 39, 62, 63):
        assert sum(s[0] == nb for s in lc.DISTO_SHAPES) >= 2, nb
    for T in (1, 15, 16, 17, 33):
        assert sum(s[1] == T for s in lc.DISTO_SHAPES) >= 2, T
    assert any(T * T % 256 == 0 for _, T in lc.DISTO_SHAPES) and any(T * T > 1024 for _, T in lc.DISTO_SHAPES)
    assert any(nb % 2 == 0 for nb, _ in lc.DISTO_SHAPES) and any((nb | 1) != nb for nb, _ in lc.DISTO_SHAPES)
    c = lc.disto("63x33")
    m = np.outer(c.x_exists[c.pseudo_beta], c.x_exists[c.pseudo_beta])
    assert {0.0, 0.25, 0.5, 1.0} <= set(np.unique(m).tolist())            # m, m^2 and m^3 differ where m = 0.5 or 0.25


@pytest.mark.parametrize("name", lc.MSE)
def test_weighted_mse_cases_meet_their_conditions(name):
    c, r = lc.mse(name), lc.mse_ref(name)
    assert abs(r.pre_clamp / 1e4 - 1.0) >= 1e-3                           # fp32 cannot cross the clamp
    assert (c.weights == 0).any() or c.A == 1
    assert c.weights.sum() > 0
    if c.side == "lo":
        assert 0.85e4 < r.pre_clamp < 0.95e4 and r.value == r.pre_clamp and np.abs(r.g).any()
    else:
        assert 1.05e4 < r.pre_clamp < 1.15e4 and r.value == 1e4 and not np.abs(r.g).any()
    if c.B > 1:
        assert c.t_hat.max() / c.t_hat.min() > (30 if c.B > 3 else 2)


def test_the_table_reaches_the_branches_it_names():
    ceil = lambda a, b: -(-a // b)
    shapes = lc.SMOOTH_SHAPES
    A_s, B_s = {a for a, _ in shapes}, {b for _, b in shapes}
    # smooth lDDT forward: LT = 64, LBC = 12, 1024 tile pairs per trip of the final pass, 64 samples per block of it
    assert lc.tile_pairs(2881) == 1081 > 1024 and ceil(2881, 64) == 46 and max(lc.tile_pairs(a) for a in A_s) <= 1024
    assert {1, 63, 64, 65} <= A_s and {1, 11, 12, 13, 25} <= B_s and max(B_s) > 64
    assert any(b % 12 == 1 and b > 12 for b in B_s)                       # a chunk holding one sample
    # gradient sweep: GB = 4, GQ = 4
    nts = {ceil(a, 64) for a in A_s}
    assert {1, 2, 3} <= nts and 5 in nts and ceil(257, 64) % 4 == 1 and ceil(513, 64) % 4 == 1 and ceil(513, 64) > 8
    assert {b % 4 for b in B_s} == {0, 1, 2, 3}
    assert max(a * b for a, b in shapes) == 513 * 25
    # centre pairs: lanes of 64, 4 samples per block, scatter blocks of 256
    T_s, B_c = {t for t, _ in lc.CENTRE_SHAPES}, {b for _, b in lc.CENTRE_SHAPES}
    assert {1, 63, 64, 65} <= T_s and max(T_s) > 256 and {b % 4 for b in B_c} == {0, 1, 2, 3}
    assert sum(b % 4 != 0 and b != 5 for b in B_c) >= 3
    # weighted MSE: 256 samples per trip of the second pass, 256 atoms per trip of a block
    assert any(b > 256 for _, b in lc.MSE_SHAPES) and any(a < 64 for a, _ in lc.MSE_SHAPES) and any(a > 256 for a, _ in lc.MSE_SHAPES)
    assert sum(b > 256 for _, b in lc.MSE_SHAPES) >= 2


def test_probes_move_the_scalar_by_far_more_than_the_bar():
    """one atom of one sample moved by 1 A, elsewhere x_denoised = x_gt.  The sample mean makes the value independent of WHICH
    sample holds the moved atom, so a kernel that drops a sample, a tile or the factor 2 of an off-diagonal tile returns the
    unmoved value or a fraction of the move.  Condition: the move is at least 10 bars, and the values of two probed atoms are
    more than 2 bars apart (two intervals of one bar cannot overlap)."""
    P = lc.PROBE_SMOOTH
    assert P.samples == (0, 11, P.B - 1) and P.atoms == (0, 63, 64, P.A - 1) and P.B > 12
    base = lc.probe_smooth_ref()
    vals = {a: [lc.probe_smooth_ref(a, s) for s in P.samples] for a in P.atoms}
    for a, v in vals.items():
        assert all(abs(x - base) >= 10 * lc.TOL * base for x in v), (a, v, base)
        assert max(v) - min(v) <= F64_BAR * base
    flat = sorted(v[0] for v in vals.values())
    assert all(b - a > 2 * lc.TOL * base for a, b in zip(flat, flat[1:])), flat
    P = lc.PROBE_CENTRE
    assert P.samples == (0, 3, P.B - 1) and P.tokens == (0, 63, 64, P.T - 1) and P.B > 4
    c = lc.probe_centre_base()
    assert (c.token_bonds != c.token_bonds.T).any()
    b0, k0 = lc.probe_centre_ref()
    assert b0 == 0.0 and k0 > 0                                            # unmoved: every |d - d_gt| is 0
    for k in (0, 1):
        vals = {t: [lc.probe_centre_ref(t, s)[k] for s in P.samples] for t in P.tokens}
        for t, v in vals.items():
            assert all(abs(x - (b0, k0)[k]) >= 10 * lc.TOL * x for x in v), (k, t, v)
        flat = sorted(v[0] for v in vals.values())
        assert all(b - a > 2 * lc.TOL * b for a, b in zip(flat, flat[1:])), (k, flat)
