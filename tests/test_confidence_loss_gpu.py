"""The confidence losses on the device against the reference (tests/golden/g17_conf_loss_*.npz,
tools/make_golden_confidence_loss.py).  GPU only (-m gpu).

lDDT and every bin index: EXACT.  Each is a hard decision on a distance, the fixtures keep every decision 1e-4 A from its
threshold, and the lDDT ratio is one IEEE fp32 division of two exactly representable sums.
Values: |hip - f64| <= max(2e-5, 4 ref_vs_f64_rel) |f64|, the bar tests/test_loss_gpu.py derived for sums of up to 2e8 terms; these
are sums of at most 5e4 non-negative cross entropies.  Gradients: |g_hip - g64| <= max(2e-5, 4 e_ref) max|g64|, the metric of
tests/test_loss_grad_gpu.py (no sign-tie allowance: a softmax has none)."""
import ctypes

import numpy as np
import pytest
import torch

from test_confidence_loss_cpu import CONF_CASES, LOGITS, SETTINGS, TERMS, load_conf

pytestmark = pytest.mark.gpu

W = {"plddt": 1e-4, "pde": 1e-4, "pae": 2e-4}          # a non-zero PAE weight so that all three terms enter the total


def config():
    from physdock_amd import PhysDockConfig
    cfg = PhysDockConfig(model_name="medium")
    cfg.loss.pae_loss.weight = W["pae"]
    assert cfg.loss.plddt_loss.weight == W["plddt"] and cfg.loss.pde_loss.weight == W["pde"]
    return cfg


def to_dev(g, grad=False, frames=True):
    from physdock_amd.synthetic import CONF_FEAT_KEYS
    o = {k: torch.from_numpy(np.array(g[k])).cuda() for k in ("p_plddt", "p_pde", "p_pae", "x_pred")}
    f = {k: torch.from_numpy(np.array(g[k])).cuda() for k in CONF_FEAT_KEYS if frames or "frame" not in k}
    for k in LOGITS.values():
        o[k].requires_grad_(grad)
    return o, f


def call_term(t, o, f):
    from physdock_amd import loss
    return getattr(loss, t + "_loss")(**o, **f, **SETTINGS[t])


def value_ok(name, what, got, g, t):
    f64, got = float(g["f64_" + t]), got.detach()
    tol = max(2e-5, 4 * float(g["ref_vs_f64_rel_" + t]))
    print(f"{name} {what} {t}: hip {float(got)!r} f64 {f64!r} rel {abs(float(got) - f64) / abs(f64):.3e} tol {tol:.1e}")
    assert abs(float(got) - f64) <= tol * abs(f64), (name, what, t)


def grad_ok(name, what, got, g, t):
    got = got.double().cpu().numpy().reshape(-1, got.shape[-1])
    M, tol = float(g["absmax_" + t]), max(2e-5, 4 * float(g["e_ref_" + t]))
    err = np.abs(got[g["grow_" + t]] - g["g64_" + t])
    s, s2 = g["sum_g64_" + t]
    print(f"{name} {what} {t}: max err {err.max():.3e} max|g64| {M:.3e} tol {tol:.1e}; sum {got.sum()!r} vs {s!r}, sum sq {(got ** 2).sum()!r} vs {s2!r}")
    assert (err <= tol * M).all(), (name, what, t)
    e = tol * M
    assert abs(got.sum() - s) <= got.size * e and abs((got ** 2).sum() - s2) <= got.size * e * (2 * M + e)


def row_mask(g, t):
    ex = torch.from_numpy(g["x_exists"])
    return ex if t == "plddt" else torch.outer(ex[g["token_id_to_centre_atom_id"]], ex[g["token_id_to_centre_atom_id"]]).reshape(-1)


def masked_rows_zero(g, t, got):
    m = row_mask(g, t)
    rows = got.cpu().reshape(m.shape[0], -1)[m == 0]
    assert rows.shape[0] >= 1 and not rows.any() and not torch.signbit(rows).any()


@pytest.mark.parametrize("name", CONF_CASES)
def test_lddt_and_bins_equal_the_reference_exactly(name):
    from physdock_amd import loss
    g = load_conf(name)
    o, f = to_dev(g)
    poly = f["is_ligand"] == 0
    got = loss.cal_lddt(o["x_pred"], f["x_gt"], f["is_dna"], f["is_rna"], poly, f["token_id_to_centre_atom_id"]).cpu().numpy()
    ref = g["ref_lddt"]
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got.view(np.uint32)[~np.isnan(ref)], ref.view(np.uint32)[~np.isnan(ref)])
    one = loss.cal_lddt(o["x_pred"][1], f["x_gt"], f["is_dna"], f["is_rna"], poly.float(), f["token_id_to_centre_atom_id"])
    assert one.shape == (ref.shape[1],) and np.array_equal(one.cpu().numpy(), got[1], equal_nan=True)
    with np.errstate(invalid="ignore"):
        v = got[0] * np.float32(50)
    bins = np.where(np.isnan(v), 0, np.clip(np.trunc(np.nan_to_num(v)), 0, 49)).astype(np.int64)
    assert np.array_equal(bins, g["bins_plddt"].astype(np.int64))
    # the bins the kernels form, read off the gradient: with zero logits g = coef (1 / nb - onehot), negative at the target only
    z = {k: torch.zeros_like(o[k]).requires_grad_(True) for k in LOGITS.values()}
    for t in TERMS:
        call_term(t, {**o, **z}, f).backward()
        gr = z[LOGITS[t]].grad.cpu().reshape(-1, z[LOGITS[t]].shape[-1])
        live = (gr != 0).any(-1)
        want = torch.from_numpy(g["bins_" + t].astype(np.int64)).reshape(-1)
        assert ((gr < 0).sum(-1)[live] == 1).all()
        assert torch.equal(gr.argmin(-1)[live], want[live]), t
        assert torch.equal(live, row_mask(g, t) != 0)                             # masked rows: no gradient at all


@pytest.mark.parametrize("name", CONF_CASES)
def test_values_and_gradients_vs_reference(name):
    from physdock_amd import ConfidenceLoss
    g = load_conf(name)
    L = ConfidenceLoss(config())
    # each term alone
    alone, galone = {}, {}
    for t in TERMS:
        o, f = to_dev(g, grad=True)
        v = call_term(t, o, f)
        assert v.shape == () and v.dtype == torch.float32 and v.is_cuda and v.grad_fn is not None
        value_ok(name, "alone", v, g, t)
        v.backward()
        grad_ok(name, "alone", o[LOGITS[t]].grad, g, t)
        masked_rows_zero(g, t, o[LOGITS[t]].grad)
        assert all(o[LOGITS[u]].grad is None for u in TERMS if u != t)
        o0, f0 = to_dev(g)
        v0 = call_term(t, o0, f0)
        assert v0.grad_fn is None and torch.equal(v0, v.detach())
        alone[t], galone[t] = v0, o[LOGITS[t]].grad
    # through the module
    o, f = to_dev(g, grad=True)
    cum, losses = L(o, f)
    assert set(losses) == {"plddt_loss", "pde_loss", "pae_loss", "loss"} and all(v.grad_fn is None for v in losses.values())
    assert cum.grad_fn is not None and torch.equal(cum.detach(), losses["loss"])
    for t in TERMS:
        assert torch.equal(losses[t + "_loss"], alone[t])                         # the same bits as the function alone
        value_ok(name, "module", losses[t + "_loss"], g, t)
    f64 = sum(W[t] * float(g["f64_" + t]) for t in TERMS)
    tol = max(2e-5, 4 * max(float(g["ref_vs_f64_rel_" + t]) for t in TERMS))
    assert abs(float(cum.detach()) - f64) <= tol * abs(f64)
    cum.backward()
    o0, f0 = to_dev(g)
    t3, *gs = L.grads(o0, f0)
    assert torch.equal(t3, torch.stack([alone[t] for t in TERMS])) and torch.equal(L.terms(o0, f0), t3)
    for t, gg in zip(TERMS, gs):
        got = o[LOGITS[t]].grad
        assert torch.equal(got, gg), t                                            # backward() and grads(): the same bits
        gw = {k: (v * W[t] if k.startswith(("g64_", "absmax_")) else v * np.array([W[t], W[t] ** 2]) if k.startswith("sum_g64_") else v)
              for k, v in g.items()}
        grad_ok(name, "module", got, gw, t)
        masked_rows_zero(g, t, got)
    # grad_scale scales linearly (a power of two: exactly)
    _, *g4 = L.grads(o0, f0, grad_scale=torch.tensor(4.0, device="cuda"))
    assert all(torch.equal(a * 4, b) for a, b in zip(gs, g4))
    _, *g3 = L.grads(o0, f0, grad_scale=torch.tensor(3.0, device="cuda"))
    for t, a, b in zip(TERMS, gs, g3):
        assert float((a.double() * 3 - b.double()).abs().max()) <= 1e-6 * 3 * W[t] * float(g["absmax_" + t])


def test_pae_without_frame_keys_and_other_inputs_requiring_grad():
    from physdock_amd import ConfidenceLoss, PhysDockConfig
    g = load_conf("small")
    o, f = to_dev(g, grad=True, frames=False)
    L = ConfidenceLoss(PhysDockConfig(model_name="medium"))                       # pae_loss.weight = 0
    cum, losses = L(o, f)
    assert set(losses) == {"plddt_loss", "pde_loss", "pae_loss", "loss"} and float(losses["pae_loss"]) == 0.0
    cum.backward()
    assert o["p_pae"].grad is None and o["p_plddt"].grad is not None and o["p_pde"].grad is not None
    o0, f0 = to_dev(g, frames=False)
    t3, gl, gd, ga = L.grads(o0, f0)
    assert ga is None and float(t3[2]) == 0.0 and torch.equal(gl, o["p_plddt"].grad) and torch.equal(gd, o["p_pde"].grad)
    with pytest.raises(KeyError, match="token_id_to_frame_atom_id"):
        ConfidenceLoss(config())(o0, f0)
    # with the keys and a zero weight the term is computed and its gradient is an exact zero
    o1, f1 = to_dev(g)
    t3b, _, _, ga = L.grads(o1, f1)
    assert float(t3b[2]) > 0 and ga is not None and not ga.any()
    for key in ("x_pred", "x_gt"):
        o2, f2 = to_dev(g, grad=True)
        (o2 if key in o2 else f2)[key].requires_grad_(True)
        with pytest.raises(NotImplementedError, match=key):
            L(o2, f2)
        with pytest.raises(NotImplementedError, match=key):
            call_term("pde", o2, f2)
    before = torch.cuda.memory_allocated()
    v = call_term("pde", o1, f1)
    assert v.grad_fn is None and torch.cuda.memory_allocated() - before < o1["p_pde"].numel() * 4       # no gradient buffer


@pytest.mark.parametrize("name", ["small", "ragged"])
def test_bits_across_calls_streams_and_graph_replay(name):
    from physdock_amd import ConfidenceLoss
    from physdock_amd import _lib as ops
    g = load_conf(name)
    o, f = to_dev(g)
    L = ConfidenceLoss(config())
    a = L.grads(o, f)
    b = L.grads(o, f)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = L.grads(o, f)                                        # also the warm-up of the capture stream
    s.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    del c, x, y, z                                               # their blocks go back to the capture stream's pool: no allocation below
    # the launches of grads() captured with the library's own graph helpers replay to the eager bits
    lib = ops.init()
    with torch.cuda.stream(s):
        ops.check(lib.pd_graph_begin(s.cuda_stream), "graph_begin")
        r = L.grads(o, f)
        ex = ctypes.c_void_p()
        ops.check(lib.pd_graph_end(s.cuda_stream, ctypes.byref(ex)), "graph_end")
        for _ in range(2):
            for x in r:
                x.zero_()
            ops.check(lib.pd_graph_launch(ex, s.cuda_stream), "graph_launch")
            s.synchronize()
            for x, y in zip(a, r):
                assert torch.equal(x, y)
        ops.check(lib.pd_graph_destroy(ex), "graph_destroy")


def test_end_to_end_confidence_module_into_the_loss():
    """ConfidenceModule at the small configuration (seeded weights, the s / z / x_pred of the small confidence case) -> its three
    logits -> ConfidenceLoss: a finite positive loss and finite gradients of the logits' shapes"""
    from physdock_amd import ConfidenceLoss, ConfidenceModule, small_config
    from physdock_amd.synthetic import frame_atom_ids, loss_features
    from test_confidence_cpu import confidence_case
    cm, batch, inp, sd, _ = confidence_case("small")
    cfg = small_config()
    mod = ConfidenceModule.from_config(cfg)
    mod.load_state_dict(sd, strict=True)
    mod = mod.cuda().eval()
    db = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    x_pred = inp["x_pred"].cuda()
    p_pae, p_pde, p_plddt = mod(db, inp["s"].cuda(), inp["z"].cuda(), x_pred)
    feats = loss_features(batch, seed=1, n_dna=2, n_rna=2)
    for k, v in enumerate(frame_atom_ids(feats)):
        feats[f"token_id_to_frame_atom_id_{k}"] = v
    feats = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in feats.items()}
    cfg.loss.pae_loss.weight = 1e-4
    out = {"p_plddt": p_plddt.requires_grad_(True), "p_pde": p_pde.requires_grad_(True), "p_pae": p_pae.requires_grad_(True), "x_pred": x_pred}
    cum, losses = ConfidenceLoss(cfg)(out, feats)
    assert torch.isfinite(cum) and float(cum.detach()) > 0 and all(torch.isfinite(v) and float(v) > 0 for v in losses.values())
    cum.backward()
    A, T = x_pred.shape[1], p_pde.shape[0]
    assert p_plddt.grad.shape == (A, 50) and p_pde.grad.shape == (T, T, 64) and p_pae.grad.shape == (T, T, 64)
    for p in (p_plddt, p_pde, p_pae):
        assert torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0
