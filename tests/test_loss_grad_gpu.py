"""PhysDockLoss gradients on the device against the reference's autograd (tests/golden/g16_loss_grad_*.npz,
tools/make_golden_loss_grad.py).

Bar, per sample and component: |g_hip - g64| <= tol * max|g64| + a_bi, tol = max(2e-5, 4 * e_ref).  2e-5 is the forward's bar
(tests/test_loss_gpu.py), whose rounding argument covers sums of up to 2e8 terms; a gradient element sums at most A of them.
e_ref is the reference fp32 gradient's own distance to g64 under the same metric; a_bi the sign-tie allowance of the fixture
(smooth lDDT, key-res; zero elsewhere)."""
import logging

import numpy as np
import pytest
import torch

from test_loss_cpu import TERMS
from test_loss_grad_cpu import GRAD_CASES, X_TERMS, load_grad

pytestmark = pytest.mark.gpu

OUT_KEYS = ("x_denoised", "t_hat", "p_distogram")


def to_dev(inp, need_x=True, need_p=True):
    from physdock_amd.synthetic import LOSS_FEAT_KEYS
    o = {k: torch.from_numpy(np.array(inp[k])).cuda() for k in OUT_KEYS}
    f = {k: torch.from_numpy(np.array(inp[k])).cuda() for k in LOSS_FEAT_KEYS}
    o["x_denoised"].requires_grad_(need_x)
    o["p_distogram"].requires_grad_(need_p)
    return o, f


def settings(cfg, t):
    return {k: v for k, v in cfg.loss[t].items() if k != "weight"}


def check_x(name, what, got, g64, absmax, allow, tol, rows):
    """got: the full [B,A,3] from the device; g64 / allow / absmax on the fixture's stored sample rows"""
    got = got.double().cpu().numpy()
    for r, b in enumerate(rows):
        bound = tol * absmax[r] + (allow[r][:, None] if allow is not None else 0.0)
        err = np.abs(got[b] - g64[r])
        worst = float((err - bound).max())
        print(f"{name} {what} sample {b}: max err {err.max():.3e} max|g64| {absmax[r]:.3e} tol {tol:.1e} excess {worst:.3e}")
        assert (err <= bound).all(), (name, what, b, worst)


def check_p(name, what, got, g64, absmax, tol, prow):
    got = got.double().cpu().numpy()[prow]
    err = np.abs(got - g64)
    print(f"{name} {what}: max err {err.max():.3e} max|g64| {absmax:.3e} tol {tol:.1e}")
    assert (err <= tol * absmax).all(), (name, what)


def checksums(name, what, got, g, t, tol):
    """full arrays of which only some rows are stored: sum and sum of squares within what the per-element bound allows"""
    got = got.double().cpu().numpy()
    M = float(np.max(g["absmax_" + t]))
    amax = float(g.get("allow_max_" + t, 0.0))
    e = tol * M + amax
    n = got.size
    s, s2 = g["sum_g64_" + t]
    print(f"{name} {what}: sum {got.sum()!r} vs {s!r}, sum sq {(got ** 2).sum()!r} vs {s2!r}")
    assert abs(got.sum() - s) <= n * tol * M + 3 * float(g.get("allow_sum_" + t, 0.0))
    assert abs((got ** 2).sum() - s2) <= n * e * (2 * M + e)


@pytest.mark.parametrize("name", GRAD_CASES)
def test_term_gradients_vs_reference(name):
    from physdock_amd import PhysDockConfig, loss
    cfg = PhysDockConfig(model_name="medium")
    g, inp = load_grad(name)
    rows, prow = g["rows"], g["prow"]
    done = 0
    for t in TERMS:
        if not g["has_" + t]:
            continue
        o, f = to_dev(inp)
        v = getattr(loss, t)(**o, **f, **settings(cfg, t))
        assert v.grad_fn is not None
        v.backward()
        tol = max(2e-5, 4 * float(g["e_ref_" + t]))
        if t == "distogram_loss":
            assert o["x_denoised"].grad is None
            check_p(name, t, o["p_distogram"].grad, g["g64_" + t], float(g["absmax_" + t]), tol, prow)
            if len(prow) < o["p_distogram"].shape[0]:
                checksums(name, t, o["p_distogram"].grad, g, t, tol)
        else:
            assert o["p_distogram"].grad is None
            absmax = np.asarray(g["absmax_" + t])[rows]
            check_x(name, t, o["x_denoised"].grad, g["g64_" + t], absmax, g.get("allow_" + t), tol, rows)
            if len(rows) < o["x_denoised"].shape[0]:
                checksums(name, t, o["x_denoised"].grad, g, t, tol)
        if name == "clamped" and t == "weighted_mse_loss":
            assert not o["x_denoised"].grad.abs().any()
        done += 1
    assert done >= 1


@pytest.mark.parametrize("name", GRAD_CASES)
def test_total_backward_vs_reference_and_grads_bits(name, caplog):
    from physdock_amd import PhysDockConfig, PhysDockLoss
    cfg = PhysDockConfig(model_name="medium")
    g, inp = load_grad(name)
    need_x = bool(g["need_x"])
    rows, prow, w = g["rows"], g["prow"], g["weights"]
    L = PhysDockLoss(cfg)
    o, f = to_dev(inp, need_x=need_x)
    with caplog.at_level(logging.WARNING):
        cum, losses = L(o, f)
    assert cum.grad_fn is not None and all(v.grad_fn is None for v in losses.values())
    # with grad enabled the values are the bits of the no-grad path
    o0, f0 = to_dev(inp, need_x=False, need_p=False)
    cum0, losses0 = L(o0, f0)
    assert cum0.grad_fn is None
    assert torch.equal(cum.detach(), cum0) and all(torch.equal(losses[k], losses0[k]) for k in losses0)
    cum.backward()
    # grads(): the same bits, no host read
    t5, g_x, g_p = L.grads(o0, f0)
    assert torch.equal(o["p_distogram"].grad, g_p)
    if need_x:
        assert torch.equal(o["x_denoised"].grad, g_x)
    else:
        assert o["x_denoised"].grad is None
    # against sum_t weight_t g64_t over the terms PhysDockLoss keeps
    if need_x:
        kept = [(k, t) for k, t in enumerate(X_TERMS) if g["has_" + t]]
        if not kept:                         # no finite x term (nan case): a zero gradient
            assert torch.isfinite(o["x_denoised"].grad).all() and not o["x_denoised"].grad.abs().any()
        else:
            tol = max(2e-5, 4 * float(g["e_ref_cum_x"]))
            g64 = sum(w[k] * g["g64_" + t] for k, t in kept)
            allow = sum(w[k] * g["allow_" + t] for k, t in kept if ("allow_" + t) in g)
            allow = None if isinstance(allow, (int, float)) else allow
            absmax = np.array([np.abs(g64[r]).max() for r in range(len(rows))])
            check_x(name, "cum", o["x_denoised"].grad, g64, absmax, allow, tol, rows)
    tol = max(2e-5, 4 * float(g["e_ref_cum_p"]))
    check_p(name, "cum", o["p_distogram"].grad, w[4] * g["g64_distogram_loss"], w[4] * float(g["absmax_distogram_loss"]), tol, prow)
    if name == "nan":
        assert any("Skipping" in r.getMessage() for r in caplog.records)
        assert torch.isfinite(o["p_distogram"].grad).all()


def test_other_inputs_requiring_grad_are_refused():
    from physdock_amd import PhysDockConfig, PhysDockLoss, loss
    g, inp = load_grad("small")
    for key in ("t_hat", "x_gt"):
        o, f = to_dev(inp)
        (o if key in o else f)[key].requires_grad_(True)
        with pytest.raises(NotImplementedError, match=key):
            PhysDockLoss(PhysDockConfig())(o, f)
    o, f = to_dev(inp)
    f["x_gt"].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="x_gt"):
        loss.smooth_lddt_loss(**o, **f, max_clamp_distance=15.0)


@pytest.mark.parametrize("name", ["small", "ragged"])
def test_bits_across_calls_streams_and_graph_replay(name):
    from physdock_amd import PhysDockConfig, PhysDockLoss
    g, inp = load_grad(name)
    o, f = to_dev(inp, need_x=False, need_p=False)
    L = PhysDockLoss(PhysDockConfig())
    a = L.grads(o, f)
    b = L.grads(o, f)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = L.grads(o, f)
    s.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    graph = torch.cuda.CUDAGraph()
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        L.grads(o, f)                                            # warm-up on the capture stream
    s2.synchronize()
    with torch.cuda.graph(graph, stream=s2):
        r = L.grads(o, f)
    for _ in range(2):
        for x in r:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(a, r):
            assert torch.equal(x, y)


def test_backward_memory_at_cfg1_shape():
    """B = 48, A = 2048, T = 256: one [48, 2048, 2048] fp32 tensor is 805 MB; the backward may add 64 MB (the forward's own
    bar in tests/test_loss_gpu.py; g_x is 1.2 MB, g_p 10.2 MB, the workspace 1.2 MB)"""
    from physdock_amd import PhysDockConfig, PhysDockLoss
    g, inp = load_grad("cfg1")
    o, f = to_dev(inp)
    L = PhysDockLoss(PhysDockConfig())
    L(o, f)[0].backward()                                        # library load, first-call state
    torch.cuda.synchronize()
    o["x_denoised"].grad = None
    o["p_distogram"].grad = None
    cum, _ = L(o, f)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    cum.backward()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"peak memory growth over the backward: {grown / 2 ** 20:.2f} MB (one B A A fp32 tensor: {48 * 2048 * 2048 * 4 / 2 ** 20:.0f} MB)")
    assert grown < 64 * 2 ** 20
