"""The confidence head over several poses on the HIP kernels: ConfidenceModule.forward_poses / score_poses (Engine.confidence_poses,
csrc/confidence.hip *_poses kernels), ranking.rank_by_confidence and the confidence= keyword of driver.redock, against the
single-pose path (bit for bit), the G19 vectors of the reference and get_metrics.  GPU only (-m gpu).

Shapes: small T 36 / A 52 / P 5 (no padding; 1296 pair rows per pose are not whole row tiles, so the exit projections run pose by
pose), ragged T 23 / A 91 / P 3 (padded to 24 / 92; 576 pair rows = whole 64-row tiles: ONE exit launch per chunk), and P = 1."""
import numpy as np
import pytest
import torch

import physdock_oracle as orc
from test_confidence_poses_cpu import CASES, TOL, bound, check_logits, poses_case

pytestmark = pytest.mark.gpu
SCORE_KEYS = ("ranking_confidence", "ptm", "iptm", "has_clash", "mean_plddt", "plddt")
_state = {}


def hip_case(name):
    """module on the device, device batch / inputs, and forward_poses of all poses - computed once per case, left unchanged"""
    if name not in _state:
        from physdock_amd.confidence import ConfidenceModule
        cm, batch, inp, sd, g = poses_case(name)
        mod = ConfidenceModule(**cm)
        mod.load_state_dict(sd, strict=True)
        mod = mod.cuda().eval()
        db = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        di = {k: v.cuda() for k, v in inp.items()}
        out = mod.forward_poses(db, di["s"], di["z"], di["x_pred"])
        torch.cuda.synchronize()
        _state[name] = (mod, db, di, out, g)
    return _state[name]


def same_scores(a, b):
    return all(torch.equal(a[k], b[k]) for k in SCORE_KEYS)


@pytest.mark.parametrize("name", list(CASES))
def test_forward_poses_is_bit_equal_to_the_single_pose_path(name):
    mod, db, di, out, g = hip_case(name)
    T, A, P = CASES[name]
    assert out[0].shape == (P, T, T, 64) and out[1].shape == (P, T, T, 64) and out[2].shape == (P, A, 50)
    assert all(o.is_contiguous() and torch.isfinite(o).all() for o in out)
    for p in range(P):
        one = mod(db, di["s"], di["z"], di["x_pred"][p:p + 1])
        for k in range(3):
            assert torch.equal(out[k][p], one[k]), (name, p, k)
    assert not torch.equal(out[0][0], out[0][1])                               # the poses do differ
    # pose 0 alone (P = 1), and forward itself still reads pose 0 only
    p1 = mod.forward_poses(db, di["s"], di["z"], di["x_pred"][:1])
    fw = mod(db, di["s"], di["z"], di["x_pred"])
    assert all(p1[k].shape[0] == 1 and torch.equal(p1[k][0], out[k][0]) and torch.equal(fw[k], out[k][0]) for k in range(3))


def test_forward_poses_subset_out_of_order():
    mod, db, di, out, g = hip_case("small")
    for poses in ([3, 0], torch.tensor([3, 0], device="cuda")):
        sub = mod.forward_poses(db, di["s"], di["z"], di["x_pred"], poses=poses)
        assert all(sub[k].shape[0] == 2 and torch.equal(sub[k][0], out[k][3]) and torch.equal(sub[k][1], out[k][0]) for k in range(3))


@pytest.mark.parametrize("name", list(CASES))
def test_logits_and_scores_vs_reference(name):
    """logits: TOL = 2e-4 of the largest logit (tests/test_confidence_gpu.py); ptm / iptm / mean_plddt: max(4 e32, 8 ulp32) against the
    float64 evaluation (tests/test_metrics_gpu.py), e32 = what the reference's own fp32 run of the same inputs costs; has_clash exact"""
    mod, db, di, out, g = hip_case(name)
    P = CASES[name][2]
    for p in range(P):
        check_logits(tuple(o[p].cpu() for o in out), g, p, TOL)
    sc = mod.score_poses(db, di["s"], di["z"], di["x_pred"])
    assert sc["has_clash"].dtype == torch.int64 and sc["has_clash"].cpu().tolist() == g["ref_has_clash"].tolist()
    assert sc["plddt"].shape == (P, CASES[name][1]) and sc["atom_plddts"] is sc["plddt"]
    bad = []
    for q in ("ptm", "iptm", "mean_plddt"):
        assert sc[q].shape == (P,) and sc[q].dtype == torch.float32 and sc[q].is_cuda
        err = float(np.abs(sc[q].double().cpu().numpy() - g["f64_" + q].numpy()).max())
        dref = float(np.abs(sc[q].double().cpu().numpy() - g["ref_" + q].double().numpy()).max())
        print(f"{name} {q}: max |hip - f64| {err:.3e}  |hip - ref| {dref:.3e}  e32 {float(g['e32_' + q]):.3e}  bound {bound(g, q):.3e}")
        if err > bound(g, q):
            bad.append((q, err, bound(g, q)))
    assert not bad, bad


@pytest.mark.parametrize("name", list(CASES))
def test_score_poses_equals_get_metrics_of_forward_poses_for_every_chunk(name):
    from physdock_amd import get_metrics
    mod, db, di, out, g = hip_case(name)
    P = CASES[name][2]
    m = get_metrics({"p_plddt": out[2], "p_pae": out[0], "x_pred": di["x_pred"]}, db, all_poses=True)
    want = dict(m, plddt=m["atom_plddts"])
    for chunk in (1, 2, P, None):
        sc = mod.score_poses(db, di["s"], di["z"], di["x_pred"], chunk=chunk)
        assert same_scores(sc, want), (name, chunk)
    one = mod.score_poses(db, di["s"], di["z"], di["x_pred"][:1])               # P = 1
    assert all(torch.equal(one[k], want[k][:1]) for k in SCORE_KEYS)
    ms = get_metrics({"p_plddt": out[2], "p_pae": out[0], "x_pred": di["x_pred"]}, db, all_poses=True, skip_self_pairs=True)
    assert torch.equal(mod.score_poses(db, di["s"], di["z"], di["x_pred"], skip_self_pairs=True)["has_clash"], ms["has_clash"])
    with pytest.raises(ValueError, match="chunk"):
        mod.score_poses(db, di["s"], di["z"], di["x_pred"], chunk=0)


@pytest.mark.parametrize("name", list(CASES))
def test_ranking_reproduces_the_reference_order(name):
    from physdock_amd.ranking import rank_by_confidence
    mod, db, di, out, g = hip_case(name)
    order = rank_by_confidence(mod.score_poses(db, di["s"], di["z"], di["x_pred"]))
    assert order.is_cuda and order.dtype == torch.int64 and order.cpu().tolist() == g["order"].tolist()


def test_rank_by_confidence_tie_rule_on_the_device():
    from physdock_amd.ranking import rank_by_confidence
    s = {"ranking_confidence": torch.tensor([0.5, 0.7, 0.5, 0.7, -0.3, 0.5]).cuda(), "mean_plddt": torch.tensor([10.0, 20.0, 30.0, 20.0, 99.0, 10.0]).cuda()}
    assert rank_by_confidence(s).cpu().tolist() == [1, 3, 2, 0, 5, 4]


def test_pose_kernels_vs_torch_and_single_calls():
    """pd_confidence_pair_init_poses / pd_pair_symmetrize_poses / pd_atom_dist_embed_poses against the reference expressions and,
    bit for bit, against P calls of the single-pose launchers; pose 2 puts centre distances EXACTLY on bin midpoints"""
    from physdock_amd import ops
    L = ops._lib.init()
    g = torch.Generator().manual_seed(7)
    T, C, A, Cap, P = 37, 32, 53, 8, 3
    z, si, sj = torch.randn(T * T, C, generator=g), torch.randn(T, C, generator=g), torch.randn(T, C, generator=g)
    Wd = torch.randn(C, 13, generator=g)
    x = 12 * torch.randn(P, A, 3, generator=g)
    ctr = torch.randperm(A, generator=g)[:T]
    v = torch.linspace(3.375, 24.375, 13)
    x[2] = 0.0                                                # centres on a line: |x_i - x_0| = the 12 bin midpoints, exact in fp32
    x[2, ctr[1:13], 0] = v[:-1] + 0.875
    xc = x[:, ctr]
    d = torch.norm(xc[:, :, None] - xc[:, None], dim=-1)
    assert d[2, 0, 1:13].tolist() == (v[:-1] + 0.875).tolist()
    onehot = orc.one_hot_nearest(d, v)
    bins = onehot.argmax(-1)
    assert len(torch.unique(bins)) == 13 and bins[2, 0, 1:13].tolist() == list(range(12))      # argmin: the first of two equal bins
    want = z.reshape(T, T, C) + si[:, None] + sj[None] + onehot @ Wd.t()
    dz, dsi, dsj, dW, dx, dc = z.cuda(), si.cuda(), sj.cuda(), Wd.t().contiguous().cuda(), x.cuda(), ctr.cuda()
    NAN = float("nan")
    out = torch.full((P * T * T * C + 64,), NAN, device="cuda")
    ops.check(L.pd_confidence_pair_init_poses(ops.ptr(dz), ops.ptr(dsi), ops.ptr(dsj), ops.ptr(dW), ops.ptr(dx), ops.ptr(dc),
                                              ops.ptr(out), T, C, P, 3 * A, ops.stream()), "pair_init_poses")
    assert torch.isnan(out[P * T * T * C:]).all()
    out = out[:P * T * T * C].reshape(P, T * T, C)
    assert torch.equal(out.cpu().reshape(P, T, T, C), want)
    single = torch.empty(T * T, C, device="cuda")
    sym = torch.full((P * T * T * C + 64,), NAN, device="cuda")
    ops.check(L.pd_pair_symmetrize_poses(ops.ptr(out), ops.ptr(sym), T, C, P, ops.stream()), "sym_poses")
    assert torch.isnan(sym[P * T * T * C:]).all()
    sym = sym[:P * T * T * C].reshape(P, T * T, C)
    assert torch.equal(sym.cpu().reshape(P, T, T, C), want + want.transpose(1, 2))
    w, b = torch.randn(Cap, 1, generator=g).cuda(), torch.randn(Cap, generator=g).cuda()
    ap = torch.full((P * A * A * Cap + 64,), NAN, device="cuda")
    ops.check(L.pd_atom_dist_embed_poses(ops.ptr(dx), ops.ptr(w), ops.ptr(b), ops.ptr(ap), A, Cap, P, 3 * A, ops.stream()), "dist_embed_poses")
    assert torch.isnan(ap[P * A * A * Cap:]).all()
    ap = ap[:P * A * A * Cap].reshape(P, A * A, Cap)
    want_ap = torch.norm(x[:, None] - x[:, :, None], dim=-1)[..., None] * w.cpu()[:, 0] + b.cpu()
    torch.testing.assert_close(ap.cpu().reshape(P, A, A, Cap), want_ap, rtol=1e-6, atol=1e-6)
    one_ap, one_sym = torch.empty(A * A, Cap, device="cuda"), torch.empty(T * T, C, device="cuda")
    for p in range(P):
        ops.check(L.pd_confidence_pair_init(ops.ptr(dz), ops.ptr(dsi), ops.ptr(dsj), ops.ptr(dW), ops.ptr(dx[p]), ops.ptr(dc),
                                            ops.ptr(single), T, C, ops.stream()), "pair_init")
        ops.check(L.pd_pair_symmetrize(ops.ptr(single), ops.ptr(one_sym), T, C, ops.stream()), "sym")
        ops.check(L.pd_atom_dist_embed(ops.ptr(dx[p]), ops.ptr(w), ops.ptr(b), ops.ptr(one_ap), A, Cap, ops.stream()), "dist_embed")
        assert torch.equal(single, out[p]) and torch.equal(one_sym, sym[p]) and torch.equal(one_ap, ap[p]), p
    assert L.pd_pair_symmetrize_poses(ops.ptr(out), ops.ptr(out), T, C, P, ops.stream()) != 0          # in-place is refused
    assert L.pd_confidence_pair_init_poses(ops.ptr(dz), ops.ptr(dsi), ops.ptr(dsj), ops.ptr(dW), ops.ptr(dx), ops.ptr(dc), ops.ptr(out), T, 30, P,
                                           3 * A, ops.stream()) == -3


def test_state_stream_sync_and_allocations():
    """second call = first call; on a non-default stream; no synchronisation (the call is captured in a graph and replayed on new
    poses, as tests/test_metrics_gpu.py does for get_metrics); no fresh logit allocation in the second call"""
    mod, db, di, out, g = hip_case("small")
    T, A, P = CASES["small"]
    first = mod.score_poses(db, di["s"], di["z"], di["x_pred"], chunk=2)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    second = mod.score_poses(db, di["s"], di["z"], di["x_pred"], chunk=2)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    assert same_scores(first, second)
    result_bytes = sum(second[k].numel() * second[k].element_size() for k in SCORE_KEYS)
    one_pose_logits = 4 * (2 * T * T * 64 + A * 50)
    print(f"memory_allocated grew by {grown} bytes over the second call (results {result_bytes}, logits of one pose {one_pose_logits})")
    assert grown <= result_bytes + 8 * 512 < one_pose_logits                    # the results (512-byte allocator blocks), nothing else
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = mod.score_poses(db, di["s"], di["z"], di["x_pred"], chunk=2)
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    assert same_scores(side, first)
    x = di["x_pred"].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        captured = mod.score_poses(db, di["s"], di["z"], x, chunk=2)
    new = torch.flip(di["x_pred"], dims=(0,)).contiguous()
    eager = mod.score_poses(db, di["s"], di["z"], new, chunk=2)
    torch.cuda.synchronize()
    x.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    assert same_scores(captured, eager)
    assert all(torch.equal(eager[k], torch.flip(first[k], dims=(0,))) for k in SCORE_KEYS)


def test_redock_with_confidence(small_model_inputs):
    from physdock_amd import PhysDock, driver
    from physdock_amd.confidence import ConfidenceModule
    from physdock_amd.params import confidence_param_shapes, seeded_state_dict
    cfg, P, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P, strict=True)
    model = model.cuda().eval()
    dbatch = {k: v.cuda() for k, v in batch.items()}
    cm = dict(cfg.model.confidence_module)
    conf = ConfidenceModule(**cm)
    conf.load_state_dict(seeded_state_dict(confidence_param_shapes(**cm), seed=3), strict=True)
    conf = conf.cuda().eval()
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, dbatch, **kw)
    assert set(plain) == {"poses", "accepted", "rounds", "gamma_factor", "ranking"}
    out = driver.redock(model, dbatch, confidence=conf, **kw)
    assert set(out) == set(plain) | {"confidence", "order_confidence"}
    assert torch.equal(out["poses"], plain["poses"]) and out["ranking"]["order"] == plain["ranking"]["order"]
    assert out["ranking"]["rmsd"] == plain["ranking"]["rmsd"]
    n = out["poses"].shape[0]
    assert sorted(out["order_confidence"].cpu().tolist()) == list(range(n)) and out["order_confidence"].is_cuda
    _, cond = model.sample_diffusion(dbatch, num_sample=1, steps=2, seed=0, return_conditioning=True)
    s, z = driver.conditioning_s_z(cond[2:], batch["target_feat"].shape[0])
    chunk = batch["token_id_to_chunk_sizes"].long().cuda()
    db = dict(dbatch, token_id_to_centre_atom_id=torch.cumsum(chunk, 0) - chunk, s_mask=torch.ones(batch["target_feat"].shape[0], device="cuda"))
    direct = conf.score_poses(db, s, z, out["poses"])
    assert torch.equal(direct["ranking_confidence"], out["confidence"]["ranking_confidence"])
    many = driver.redock_many(model, [dbatch], confidence=conf, **kw)          # one system: the sequential path
    assert torch.equal(many[0]["confidence"]["ranking_confidence"], out["confidence"]["ranking_confidence"])
