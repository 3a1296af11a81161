"""The ten launchers of csrc/loss.hip and csrc/loss_grad.hip, called on the C ABI against the float64 definition tests/loss_ref.py
at the cases of tests/loss_cases.py (the table and the branch each case reaches are in that file's docstring;
tests/test_loss_ref_cpu.py checks the references and the cases' conditions without a GPU).

Bars (the project's own, tests/test_loss_gpu.py and tests/test_loss_grad_gpu.py): a value within 2e-5 of |f64|, exactly 0.0 where
f64 is 0 by construction; a gradient, per sample and element, within 2e-5 max|g64| of the sample plus the sign-tie allowance of
the element.  Every output and every workspace sits in front of a sentinel-filled guard that must come back untouched; the
workspace holds exactly pd_loss_workspace_numel / pd_loss_grad_workspace_numel floats, requested as physdock_amd.loss requests
them, is filled with NaN before a call, and a second call with other garbage in it must give the same bits."""
import numpy as np
import pytest
import torch

import loss_cases as lc

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
GUARD, SENT = 256, 1234.5
TOL = lc.TOL


def _ops():
    from physdock_amd import _lib as ops
    return ops, ops.init()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(n, fill):
    """n floats of `fill` in front of GUARD sentinels"""
    buf = torch.full((n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    buf[:n] = fill
    return buf


def guard_ok(buf, n):
    return bool((buf[n:] == SENT).all())


def numel(L, grad, B, A, T):
    n = (L.pd_loss_grad_workspace_numel if grad else L.pd_loss_workspace_numel)(B, A, T)
    assert n > 0
    return n


def fwd(kind, c, xd=None, ws_fill=float("nan")):
    """the term(s) of case c as a list of Python floats"""
    ops, L = _ops()
    p, s = ops.ptr, ops.stream()
    nout = 2 if kind == "centre" else 1
    out = guarded(nout, SENT)
    if kind == "smooth":
        nws = numel(L, False, c.B, c.A, 1)
        ws = guarded(nws, ws_fill)
        t = [dev(c.x_denoised if xd is None else xd), dev(c.x_gt), dev(c.x_exists)]
        rc = L.pd_loss_smooth_lddt(p(t[0]), p(t[1]), p(t[2]), lc.CLAMP, p(ws), p(out), c.B, c.A, s)
    elif kind == "centre":
        nws = numel(L, False, c.B, c.A, c.T)
        ws = guarded(nws, ws_fill)
        t = [dev(a) for a in (c.x_denoised if xd is None else xd, c.x_gt, c.centre, c.token_bonds, c.is_key_res, c.is_ligand, c.t_hat)]
        rc = L.pd_loss_centre_pairs(*(p(a) for a in t), lc.SD_BOND, lc.SD_KEY, lc.EPS, p(ws), p(out), c.B, c.A, c.T, s)
    elif kind == "disto":
        nws = numel(L, False, 1, c.A, c.T)
        ws = guarded(nws, ws_fill)
        t = [dev(a) for a in (c.p_distogram, c.x_gt, c.x_exists, c.pseudo_beta, c.boundaries_sq)]
        rc = L.pd_loss_distogram(*(p(a) for a in t), c.no_bins, p(ws), p(out), c.A, c.T, s)
    else:
        nws = numel(L, False, c.B, c.A, 1)
        ws = guarded(nws, ws_fill)
        t = [dev(a) for a in (c.x_denoised, c.x_gt_aligned, c.weights, c.t_hat)]
        rc = L.pd_loss_weighted_mse(*(p(a) for a in t), p(ws), p(out), c.B, c.A, s)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guard_ok(ws, nws), f"{kind} {c.name}: workspace guard written"
    assert guard_ok(out, nout), f"{kind} {c.name}: output guard written"
    return out[:nout].cpu().tolist()


def grad(kind, c, scale, accumulate=0, prefill=None, xd=None, p_in=None, ws_fill=float("nan")):
    """g_x [B,A,3] (g_p [T,T,bins] for the distogram) of case c as a CPU fp32 tensor; scale: float or (bond, key)"""
    ops, L = _ops()
    p, s = ops.ptr, ops.stream()
    shape = (c.T, c.T, c.no_bins) if kind == "disto" else (c.B, c.A, 3)
    n = int(np.prod(shape))
    g = guarded(n, SENT)
    if prefill is not None:
        g[:n] = prefill.reshape(-1).cuda()
    sc = torch.tensor(list(scale) if kind == "centre" else [scale], dtype=torch.float32, device="cuda")
    if kind == "smooth":
        nws = numel(L, True, c.B, c.A, 1)
        ws = guarded(nws, ws_fill)
        t = [dev(c.x_denoised if xd is None else xd), dev(c.x_gt), dev(c.x_exists)]
        rc = L.pd_loss_smooth_lddt_grad(p(t[0]), p(t[1]), p(t[2]), lc.CLAMP, p(sc), p(ws), p(g), c.B, c.A, accumulate, s)
    elif kind == "centre":
        nws = numel(L, True, c.B, c.A, c.T)
        ws = guarded(nws, ws_fill)
        t = [dev(a) for a in (c.x_denoised if xd is None else xd, c.x_gt, c.centre, c.token_bonds, c.is_key_res, c.is_ligand, c.t_hat)]
        rc = L.pd_loss_centre_pairs_grad(*(p(a) for a in t), lc.SD_BOND, lc.SD_KEY, lc.EPS, p(sc), p(ws), p(g), c.B, c.A, c.T, accumulate, s)
    elif kind == "disto":
        nws = numel(L, True, 1, c.A, c.T)
        ws = guarded(nws, ws_fill)
        t = [dev(a) for a in (c.p_distogram if p_in is None else p_in, c.x_gt, c.x_exists, c.pseudo_beta, c.boundaries_sq)]
        rc = L.pd_loss_distogram_grad(*(p(a) for a in t), c.no_bins, p(sc), p(ws), p(g), c.A, c.T, s)
    else:
        nws = numel(L, True, c.B, c.A, 1)
        ws = guarded(nws, ws_fill)
        t = [dev(a) for a in (c.x_denoised if xd is None else xd, c.x_gt_aligned, c.weights, c.t_hat)]
        rc = L.pd_loss_weighted_mse_grad(*(p(a) for a in t), p(sc), p(ws), p(g), c.B, c.A, accumulate, s)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guard_ok(ws, nws), f"{kind} {c.name}: workspace guard written"
    assert guard_ok(g, n), f"{kind} {c.name}: rows past the output written"
    return g[:n].cpu().reshape(shape)


def check_value(what, got, f64):
    rel = abs(got - f64) / abs(f64) if f64 else abs(got)
    print(f"{what}: hip {got!r} f64 {f64!r} rel {rel:.3e}")
    if f64 == 0.0:
        assert got == 0.0, what
    else:
        assert abs(got - f64) <= TOL * abs(f64), what


def check_grad(what, got, g64, allow=None):
    """per sample (first axis): |g - g64| <= TOL max|g64| + allowance; all finite"""
    got = got.double().numpy()
    assert np.isfinite(got).all(), f"{what}: non-finite gradient at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    worst = 0.0
    for b in range(g64.shape[0]):
        m = np.abs(g64[b]).max()
        bound = TOL * m + (allow[b][:, None] if allow is not None else 0.0)
        err = np.abs(got[b] - g64[b])
        worst = max(worst, float(err.max() / m) if m > 0 else float(err.max()))
        assert (err <= bound).all(), (what, b, float(err.max()), float(m), float((err - bound).max()))
    print(f"{what}: worst |g - g64| / max|g64| over samples {worst:.3e}")


def twice(f):
    """f(ws_fill) with NaN and with other garbage in the workspace: the same bits"""
    a, b = f(float("nan")), f(-3.0e38)
    if isinstance(a, torch.Tensor):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    else:
        assert [np.float32(x).tobytes() for x in a] == [np.float32(x).tobytes() for x in b]
    return a


# ------------------------------------------------------------------ forward parity
@pytest.mark.parametrize("name", lc.SMOOTH_FWD)
def test_smooth_lddt_forward(name):
    c = lc.smooth(name)
    (v,) = twice(lambda w: fwd("smooth", c, ws_fill=w))
    check_value(f"smooth lDDT {name}", v, (lc.smooth_ref(name, False) if name == "2881x1" else lc.smooth_ref(name)).value)


@pytest.mark.parametrize("name", lc.CENTRE)
def test_centre_pairs_forward(name):
    c, r = lc.centre(name), lc.centre_ref(name)
    b, k = twice(lambda w: fwd("centre", c, ws_fill=w))
    check_value(f"bond {name}", b, r.bond)
    check_value(f"key-res {name}", k, r.key)


@pytest.mark.parametrize("name", lc.DISTO)
def test_distogram_forward(name):
    c = lc.disto(name)
    (v,) = twice(lambda w: fwd("disto", c, ws_fill=w))
    check_value(f"distogram {name}", v, lc.disto_ref(name).value)


@pytest.mark.parametrize("name", lc.MSE)
def test_weighted_mse_forward(name):
    c, r = lc.mse(name), lc.mse_ref(name)
    (v,) = twice(lambda w: fwd("mse", c, ws_fill=w))
    check_value(f"weighted MSE {name} (pre-clamp {r.pre_clamp:.6g})", v, r.value)
    if c.side == "hi":
        assert v == 10000.0


# ------------------------------------------------------------------ probes
def test_smooth_lddt_probes():
    """x_denoised = x_gt, one atom of one sample moved by 1 A: the last column tile, the last sample of a chunk or the factor 2 of
    an off-diagonal tile cannot be dropped without moving the scalar by more than the bar (tests/test_loss_ref_cpu.py)"""
    P, c = lc.PROBE_SMOOTH, lc.probe_smooth_base()
    c.name = "probe"
    check_value("smooth lDDT probe base", fwd("smooth", c, xd=lc.probe_smooth_xd())[0], lc.probe_smooth_ref())
    for a in P.atoms:
        for s in P.samples:
            check_value(f"smooth lDDT probe atom {a} sample {s}", fwd("smooth", c, xd=lc.probe_smooth_xd(a, s))[0], lc.probe_smooth_ref(a, s))


def test_centre_pairs_probes():
    P, c = lc.PROBE_CENTRE, lc.probe_centre_base()
    c.name = "probe"
    b, k = fwd("centre", c, xd=lc.probe_centre_xd())
    assert b == 0.0
    check_value("key-res probe base", k, lc.probe_centre_ref()[1])
    for t in P.tokens:
        for s in P.samples:
            b, k = fwd("centre", c, xd=lc.probe_centre_xd(t, s))
            check_value(f"bond probe token {t} sample {s}", b, lc.probe_centre_ref(t, s)[0])
            check_value(f"key-res probe token {t} sample {s}", k, lc.probe_centre_ref(t, s)[1])


# ------------------------------------------------------------------ gradient parity
@pytest.mark.parametrize("name", lc.SMOOTH_GRAD)
def test_smooth_lddt_gradient(name):
    """near-in / near-edge: two predicted atoms 1e-20 apart have d2 = 1e-40, below the normal fp32 range, where v_rsq_f32 answers
    inf; before the fix in smooth_lddt_grad_kernel the rows of both atoms came back NaN"""
    c, r = lc.smooth(name), lc.smooth_ref(name)
    g = twice(lambda w: grad("smooth", c, 1.0, ws_fill=w))
    check_grad(f"smooth lDDT gradient {name}", g, r.g, r.allow)
    g = grad("smooth", c, -2.5)
    check_grad(f"smooth lDDT gradient {name} x -2.5", g, -2.5 * r.g, 2.5 * r.allow)


@pytest.mark.parametrize("name", lc.CENTRE)
def test_centre_pairs_gradient(name):
    c, r = lc.centre(name), lc.centre_ref(name)
    gb = twice(lambda w: grad("centre", c, (1.0, 0.0), ws_fill=w))
    check_grad(f"bond gradient {name}", gb, r.g_bond)
    gk = twice(lambda w: grad("centre", c, (0.0, 1.0), ws_fill=w))
    check_grad(f"key-res gradient {name}", gk, r.g_key, r.allow)
    both = grad("centre", c, (0.5, 3.0))
    check_grad(f"bond + key-res gradient {name}", both, 0.5 * r.g_bond + 3.0 * r.g_key, 3.0 * r.allow)


@pytest.mark.parametrize("name", lc.DISTO)
def test_distogram_gradient(name):
    c, r = lc.disto(name), lc.disto_ref(name)
    g = twice(lambda w: grad("disto", c, 1.0, ws_fill=w))
    check_grad(f"distogram gradient {name}", g.reshape(1, -1, c.no_bins), r.g.reshape(1, -1, c.no_bins))
    if c.T >= 15:
        assert not g[2].abs().any() and not g[:, 2].abs().any()             # the masked token with logits 1e30
    g = grad("disto", c, 0.03)
    check_grad(f"distogram gradient {name} x 0.03", g.reshape(1, -1, c.no_bins), 0.03 * r.g.reshape(1, -1, c.no_bins))


@pytest.mark.parametrize("name", lc.MSE)
def test_weighted_mse_gradient(name):
    c, r = lc.mse(name), lc.mse_ref(name)
    g = twice(lambda w: grad("mse", c, 1.0, ws_fill=w))
    check_grad(f"weighted MSE gradient {name}", g, r.g)
    if c.side == "hi":
        assert not g.view(torch.int32).any()                                # above the clamp: an exact zero


# ------------------------------------------------------------------ zero scale, accumulate
X_KINDS = (("smooth", "129x11"), ("centre", "130x9"), ("centre", "257x2"), ("mse", "257x3-lo"), ("mse", "40x300-lo"), ("smooth", "65x4"))


def _case(kind, name):
    return {"smooth": lc.smooth, "centre": lc.centre, "mse": lc.mse, "disto": lc.disto}[kind](name)


def _prefill(c):
    return torch.from_numpy(np.random.RandomState(7).uniform(0.5, 2.0, (c.B, c.A, 3)).astype(np.float32))


@pytest.mark.parametrize("kind,name", X_KINDS)
def test_zero_scale_writes_an_exact_zero(kind, name):
    """NaN in x_denoised and in the workspace: a zero scale writes +0.0 everywhere (accumulate = 0) or leaves g_x as it was
    (accumulate = 1), never 0 * NaN"""
    c = _case(kind, name)
    xd = c.x_denoised.copy()
    xd[0, 0, 1] = np.nan
    xd[-1, -1] = np.nan
    zero = (0.0, 0.0) if kind == "centre" else 0.0
    g = grad(kind, c, zero, xd=xd)
    assert not g.view(torch.int32).any(), f"{kind} {name}"
    pre = _prefill(c)
    g = grad(kind, c, zero, accumulate=1, prefill=pre, xd=xd)
    assert torch.equal(g.view(torch.int32), pre.view(torch.int32)), f"{kind} {name}"


@pytest.mark.parametrize("accumulate", (0, 1))
@pytest.mark.parametrize("name", ("64x4", "130x9", "257x2"))
def test_one_sided_zero_scale_of_the_centre_pairs(name, accumulate):
    """(s, 0): the key-residue term is skipped, so NaN in is_ligand (its mask, its denominator) must not reach g_x: the result is,
    bit for bit, that of the same call with the key and ligand masks zeroed.  (0, s) likewise with NaN in token_bonds against
    the call with no bonds.  A skipped term is one whose value was not finite, so this is the input a zero element meets."""
    import copy
    c = lc.centre(name)
    pre = _prefill(c) if accumulate else None
    hostile, clean = copy.copy(c), copy.copy(c)
    hostile.is_ligand = c.is_ligand.copy()
    hostile.is_ligand[np.nonzero(c.is_ligand)[0][:2]] = np.nan
    hostile.is_ligand[0] = np.nan
    clean.is_key_res, clean.is_ligand = np.zeros_like(c.is_key_res), np.zeros_like(c.is_ligand)
    got = grad("centre", hostile, (1.7, 0.0), accumulate=accumulate, prefill=pre)
    want = grad("centre", clean, (1.7, 0.0), accumulate=accumulate, prefill=pre)
    assert torch.isfinite(got).all() and want.abs().sum() > 0
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"bond only, {name}"
    hostile, clean = copy.copy(c), copy.copy(c)
    hostile.token_bonds = c.token_bonds.copy()
    hostile.token_bonds[np.nonzero(c.token_bonds)[0][0]] = np.nan            # a whole row of a bonded token
    hostile.token_bonds[:, 1] = np.nan
    clean.token_bonds = np.zeros_like(c.token_bonds)
    got = grad("centre", hostile, (0.0, 0.6), accumulate=accumulate, prefill=pre)
    want = grad("centre", clean, (0.0, 0.6), accumulate=accumulate, prefill=pre)
    assert torch.isfinite(got).all() and want.abs().sum() > 0
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"key-res only, {name}"


@pytest.mark.parametrize("name", ("39x33", "62x17", "2x16"))
def test_zero_scale_distogram(name):
    c = lc.disto(name)
    p = c.p_distogram.copy()
    p[0, 0, 0] = np.nan
    p[-1] = np.nan
    g = grad("disto", c, 0.0, p_in=p)
    assert not g.view(torch.int32).any()


@pytest.mark.parametrize("kind,name", X_KINDS)
def test_accumulate_adds_to_g_x(kind, name):
    c = _case(kind, name)
    scale = (0.7, 1.3) if kind == "centre" else 1.7
    fresh = grad(kind, c, scale)
    pre = _prefill(c)
    acc = grad(kind, c, scale, accumulate=1, prefill=pre)
    assert fresh.abs().sum() > 0
    assert torch.equal(acc, pre + fresh), f"{kind} {name}: max diff {(acc - (pre + fresh)).abs().max()}"


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched():
    ops, L = _ops()
    p, s = ops.ptr, ops.stream()
    out, ws = guarded(0, SENT), guarded(0, SENT)
    sc = torch.ones(2, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return guard_ok(out, 0) and guard_ok(ws, 0)
    # the distogram's bin count: 64 does not fit the LDS rows, 1 is no histogram
    c = lc.disto("63x16")
    keep = [dev(a) for a in (c.p_distogram, c.x_gt, c.x_exists, c.pseudo_beta, c.boundaries_sq)]
    t = [p(a) for a in keep]
    for nb, want in ((64, PD_ERR_UNSUPPORTED), (1, PD_ERR_ARG), (0, PD_ERR_ARG)):
        assert L.pd_loss_distogram(*t, nb, p(ws), p(out), c.A, c.T, s) == want
        assert L.pd_loss_distogram_grad(*t, nb, p(sc), p(ws), p(out), c.A, c.T, s) == want
    assert L.pd_loss_distogram(*t, c.no_bins, p(ws), p(out), c.A, 0, s) == PD_ERR_ARG
    assert L.pd_loss_distogram_grad(*t, c.no_bins, p(sc), p(ws), p(out), 0, c.T, s) == PD_ERR_ARG
    for k in range(5):
        u = list(t)
        u[k] = None
        assert L.pd_loss_distogram(*u, c.no_bins, p(ws), p(out), c.A, c.T, s) == PD_ERR_ARG
        assert L.pd_loss_distogram_grad(*u, c.no_bins, p(sc), p(ws), p(out), c.A, c.T, s) == PD_ERR_ARG
    for tail in ((None, p(ws), p(out)), (p(sc), None, p(out)), (p(sc), p(ws), None)):
        assert L.pd_loss_distogram_grad(*t, c.no_bins, *tail, c.A, c.T, s) == PD_ERR_ARG
    assert untouched()
    # smooth lDDT
    c = lc.smooth("65x4")
    keep = [dev(a) for a in (c.x_denoised, c.x_gt, c.x_exists)]
    t = [p(a) for a in keep]
    for B, A in ((0, c.A), (c.B, 0), (-1, c.A)):
        assert L.pd_loss_smooth_lddt(*t, lc.CLAMP, p(ws), p(out), B, A, s) == PD_ERR_ARG
        assert L.pd_loss_smooth_lddt_grad(*t, lc.CLAMP, p(sc), p(ws), p(out), B, A, 0, s) == PD_ERR_ARG
    for k in range(3):
        u = list(t)
        u[k] = None
        assert L.pd_loss_smooth_lddt(*u, lc.CLAMP, p(ws), p(out), c.B, c.A, s) == PD_ERR_ARG
        assert L.pd_loss_smooth_lddt_grad(*u, lc.CLAMP, p(sc), p(ws), p(out), c.B, c.A, 0, s) == PD_ERR_ARG
    assert L.pd_loss_smooth_lddt(*t, lc.CLAMP, None, p(out), c.B, c.A, s) == PD_ERR_ARG
    assert L.pd_loss_smooth_lddt(*t, lc.CLAMP, p(ws), None, c.B, c.A, s) == PD_ERR_ARG
    for tail in ((None, p(ws), p(out)), (p(sc), None, p(out)), (p(sc), p(ws), None)):
        assert L.pd_loss_smooth_lddt_grad(*t, lc.CLAMP, *tail, c.B, c.A, 0, s) == PD_ERR_ARG
    assert untouched()
    # centre pairs
    c = lc.centre("64x4")
    keep = [dev(a) for a in (c.x_denoised, c.x_gt, c.centre, c.token_bonds, c.is_key_res, c.is_ligand, c.t_hat)]
    t = [p(a) for a in keep]
    sd = (lc.SD_BOND, lc.SD_KEY, lc.EPS)
    for B, A, T in ((0, c.A, c.T), (c.B, 0, c.T), (c.B, c.A, 0)):
        assert L.pd_loss_centre_pairs(*t, *sd, p(ws), p(out), B, A, T, s) == PD_ERR_ARG
        assert L.pd_loss_centre_pairs_grad(*t, *sd, p(sc), p(ws), p(out), B, A, T, 0, s) == PD_ERR_ARG
    for k in range(7):
        u = list(t)
        u[k] = None
        assert L.pd_loss_centre_pairs(*u, *sd, p(ws), p(out), c.B, c.A, c.T, s) == PD_ERR_ARG
        assert L.pd_loss_centre_pairs_grad(*u, *sd, p(sc), p(ws), p(out), c.B, c.A, c.T, 0, s) == PD_ERR_ARG
    assert L.pd_loss_centre_pairs(*t, *sd, None, p(out), c.B, c.A, c.T, s) == PD_ERR_ARG
    assert L.pd_loss_centre_pairs(*t, *sd, p(ws), None, c.B, c.A, c.T, s) == PD_ERR_ARG
    for tail in ((None, p(ws), p(out)), (p(sc), None, p(out)), (p(sc), p(ws), None)):
        assert L.pd_loss_centre_pairs_grad(*t, *sd, *tail, c.B, c.A, c.T, 0, s) == PD_ERR_ARG
    assert untouched()
    # weighted MSE
    c = lc.mse("63x2-lo")
    keep = [dev(a) for a in (c.x_denoised, c.x_gt_aligned, c.weights, c.t_hat)]
    t = [p(a) for a in keep]
    for B, A in ((0, c.A), (c.B, 0)):
        assert L.pd_loss_weighted_mse(*t, p(ws), p(out), B, A, s) == PD_ERR_ARG
        assert L.pd_loss_weighted_mse_grad(*t, p(sc), p(ws), p(out), B, A, 0, s) == PD_ERR_ARG
    for k in range(4):
        u = list(t)
        u[k] = None
        assert L.pd_loss_weighted_mse(*u, p(ws), p(out), c.B, c.A, s) == PD_ERR_ARG
        assert L.pd_loss_weighted_mse_grad(*u, p(sc), p(ws), p(out), c.B, c.A, 0, s) == PD_ERR_ARG
    assert L.pd_loss_weighted_mse(*t, None, p(out), c.B, c.A, s) == PD_ERR_ARG
    assert L.pd_loss_weighted_mse(*t, p(ws), None, c.B, c.A, s) == PD_ERR_ARG
    for tail in ((None, p(ws), p(out)), (p(sc), None, p(out)), (p(sc), p(ws), None)):
        assert L.pd_loss_weighted_mse_grad(*t, *tail, c.B, c.A, 0, s) == PD_ERR_ARG
    assert untouched()
    for f in (L.pd_loss_workspace_numel, L.pd_loss_grad_workspace_numel):
        assert f(0, 1, 1) == f(1, 0, 1) == f(1, 1, 0) == PD_ERR_ARG
