"""PhysDockLoss on the device against the reference's values (tests/golden/g15_loss_*.npz, tools/make_golden_loss.py).

The bar is relative and set against the reference, not against this code: all five terms are sums of non-negative fp32
terms, and |hip - f64| / |f64| <= max(2e-5, 4 * ref_vs_f64_rel).  2e-5 is about (log2 of 2e8 terms + the distance
cancellation at 50 A) x 2^-24 with a factor of ten; the factor 4 over the reference's own fp32 distance to float64 allows
another summation order."""
import ctypes
import logging

import numpy as np
import pytest
import torch

from test_loss_cpu import CASES, TERMS, load_case

pytestmark = pytest.mark.gpu

OUT_KEYS = ("x_denoised", "t_hat", "p_distogram")


def to_dev(g):
    from physdock_amd.synthetic import LOSS_FEAT_KEYS
    o = {k: torch.from_numpy(g[k]).cuda() for k in OUT_KEYS}
    f = {k: torch.from_numpy(g[k]).cuda() for k in LOSS_FEAT_KEYS}
    return o, f


def settings(cfg, t):
    return {k: v for k, v in cfg.loss[t].items() if k != "weight"}


@pytest.mark.parametrize("name", CASES)
def test_terms_and_total_vs_reference(name, caplog):
    from physdock_amd import PhysDockConfig, PhysDockLoss, loss
    cfg = PhysDockConfig(model_name="medium")
    g = load_case(name)
    o, f = to_dev(g)
    with caplog.at_level(logging.WARNING):
        cum, losses = PhysDockLoss(cfg)(o, f)
    assert set(losses) == set(TERMS) | {"loss"}
    for k, v in losses.items():
        assert v.is_cuda and v.dtype == torch.float32 and v.dim() == 0, k
    assert cum.is_cuda and cum.dim() == 0 and float(cum) == float(losses["loss"])
    for t in TERMS:
        single = float(getattr(loss, t)(**o, **f, **settings(cfg, t)))        # the function alone, reference call shape
        ref, f64, tol = float(g["ref_" + t]), float(g["f64_" + t]), max(2e-5, 4 * float(g["ref_vs_f64_rel_" + t]))
        got = float(losses[t])
        print(f"{name} {t}: hip {got!r} alone {single!r} f64 {f64!r} ref {ref!r} rel {abs(got - f64) / abs(f64) if f64 else 0.0:.3e} tol {tol:.1e}")
        if np.isnan(ref):            # the reference's skip-and-warn path: NaN term -> zero, with a warning
            assert np.isnan(single) and got == 0.0, t
            assert any(t in r.getMessage() for r in caplog.records), t
            continue
        assert single == got, t
        assert abs(got - f64) <= tol * abs(f64), t
    tot, f64 = float(losses["loss"]), float(g["f64_loss"])
    print(f"{name} loss: hip {tot!r} f64 {f64!r} rel {abs(tot - f64) / abs(f64):.3e}")
    assert abs(tot - f64) <= max(2e-5, 4 * float(g["ref_vs_f64_rel_loss"])) * abs(f64)
    if not np.isnan([float(g["ref_" + t]) for t in TERMS]).any():
        assert not caplog.records


def test_x_exists_falls_back_to_a_mask():
    from physdock_amd import PhysDockConfig, PhysDockLoss
    o, f = to_dev(load_case("small"))
    want = PhysDockLoss(PhysDockConfig())(o, f)[0]
    f["a_mask"] = f.pop("x_exists")
    assert torch.equal(PhysDockLoss(PhysDockConfig())(o, f)[0], want)


@pytest.mark.parametrize("name", ["small", "ragged"])
def test_bit_reproducible_and_stream_independent(name):
    from physdock_amd import PhysDockConfig, PhysDockLoss
    o, f = to_dev(load_case(name))
    L = PhysDockLoss(PhysDockConfig())
    a = L.terms(o, f)
    b = L.terms(o, f)
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = L.terms(o, f)
    s.synchronize()
    assert torch.equal(a, c)


def test_memory_at_cfg1_shape():
    """B = 48, A = 2048, T = 256: one [48, 2048, 2048] fp32 tensor would be 805 MB; the call may allocate 64 MB"""
    from physdock_amd import PhysDockConfig, PhysDockLoss
    g = load_case("cfg1")
    assert g["x_denoised"].shape == (48, 2048, 3)
    o, f = to_dev(g)
    L = PhysDockLoss(PhysDockConfig())
    L(o, f)                                                   # library load, first-call state
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    L(o, f)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"peak memory growth over the loss call: {grown / 2 ** 20:.2f} MB")
    assert grown < 64 * 2 ** 20


def test_forward_return_loss(small_model_inputs):
    from physdock_amd import PhysDock, PhysDockLoss
    from physdock_amd.synthetic import loss_features
    cfg, P, batch = small_model_inputs
    model = PhysDock(cfg); model.load_state_dict(P); model = model.cuda().eval()
    feats = {k: v.cuda() for k, v in loss_features(batch, seed=1, n_dna=2, n_rna=2, n_key=4, masked_atoms=(7,)).items()}
    out = model(feats)
    assert isinstance(out, dict) and set(out) == {"x_denoised", "x_hat", "t_hat", "p_distogram"}
    outputs, cum, losses = model(feats, return_loss=True)
    assert set(outputs) == set(out)
    cum2, losses2 = PhysDockLoss(cfg)(outputs, feats)
    assert torch.equal(cum, cum2) and set(losses) == set(losses2) == set(TERMS) | {"loss"}
    for k in losses:
        assert torch.equal(losses[k], losses2[k]), k
    assert torch.isfinite(cum) and float(cum) > 0


def test_forward_return_loss_ragged_system():
    """T = 23 / A = 91 runs padded inside forward(); outputs and loss use the real sizes"""
    from physdock_amd import PhysDock, PhysDockLoss, param_shapes, seeded_state_dict, small_config
    from physdock_amd.synthetic import loss_features, make_batch
    cfg = small_config()
    model = PhysDock(cfg); model.load_state_dict(seeded_state_dict(param_shapes(cfg), seed=0)); model = model.cuda().eval()
    feats = {k: v.cuda() for k, v in loss_features(make_batch(17, 5, 6, 8, seed=2), seed=3, n_key=3).items()}
    outputs, cum, losses = model(feats, return_loss=True)
    assert outputs["x_denoised"].shape[1:] == (91, 3) and outputs["p_distogram"].shape == (23, 23, 39)
    cum2, _ = PhysDockLoss(cfg)(outputs, feats)
    assert torch.equal(cum, cum2) and torch.isfinite(cum)


def test_five_launches_in_one_graph_replay_to_the_same_bits():
    from physdock_amd import PhysDockConfig, _lib as ops, loss
    cfg = PhysDockConfig()
    o, f = to_dev(load_case("ragged"))
    both = {**o, **f}
    B, A, T = o["x_denoised"].shape[0], o["x_denoised"].shape[1], f["is_ligand"].shape[0]
    L = ops.init()
    c = cfg.loss
    # everything a launch needs exists before the capture: no allocation inside it
    ws = torch.empty(L.pd_loss_workspace_numel(B, A, T), device="cuda")
    al = torch.empty(B, A, 3, device="cuda")
    w = loss.mse_weights(f["is_dna"], f["is_rna"], f["is_ligand"], 5.0, 5.0, 10.0, f["atom_id_to_token_id"], f["x_exists"])
    b2 = loss.distogram_boundaries_sq(c.distogram_loss.min_bin, c.distogram_loss.max_bin, c.distogram_loss.no_bins, "cuda")

    def launches(out):
        loss.weighted_mse_loss(**both, **settings(cfg, "weighted_mse_loss"), _ws_buf=ws, _out=out[0:1], _aligned=al, _weights=w)
        loss.smooth_lddt_loss(**both, **settings(cfg, "smooth_lddt_loss"), _ws_buf=ws, _out=out[1:2])
        loss._centre_pairs(o["x_denoised"], f["x_gt"], o["t_hat"], f["token_bonds"], f["is_key_res"], f["is_ligand"],
                           f["token_id_to_centre_atom_id"], 16.0, 16.0, 1e-9, _ws_buf=ws, _out=out[2:4])
        loss.distogram_loss(**both, **settings(cfg, "distogram_loss"), _ws_buf=ws, _out=out[4:5], _bounds=b2)

    eager = torch.zeros(5, device="cuda")
    launches(eager)
    torch.cuda.synchronize()
    replay = torch.zeros(5, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.check(L.pd_graph_begin(ops.stream()), "graph_begin")
        launches(replay)
        ex = ctypes.c_void_p()
        ops.check(L.pd_graph_end(ops.stream(), ctypes.byref(ex)), "graph_end")
        assert float(replay.abs().sum().cpu()) == 0.0            # captured, not run
        for _ in range(2):
            replay.zero_()
            ops.check(L.pd_graph_launch(ex, ops.stream()), "graph_launch")
            s.synchronize()
            assert torch.equal(replay, eager)
        L.pd_graph_destroy(ex)
    assert torch.isfinite(eager).all()
