"""get_metrics on the device against the reference (tests/golden/g18_metrics_*.npz, tools/make_golden_metrics.py).  GPU only (-m gpu).

Values: |hip - f64| <= max(4 e32, 8 ulp32(max |f64|)) per quantity, the `4 E + 8 ulp32` rule of tests/test_sampler_kernels_gpu.py
(e32: what a plain fp32 numpy evaluation costs on the same input; the generator asserts that the reference itself meets the
bound).  Decisions - the argmax rows of pTM / ipTM, has_clash of every pose in both loop modes - are exact: the fixtures keep the
argmax gap >= 1e-4 and every inter-chain distance 1e-4 A from 1.1."""
import numpy as np
import pytest
import torch

from test_metrics_cpu import FEAT_KEYS, METRICS_CASES, QUANTITIES, bound, centres, load_metrics

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
SHAPES = {"atom_plddts": "PA", "mean_plddt": "P", "pae": "PTT", "ptm": "P", "iptm": "P", "has_clash": "P", "ranking_confidence": "P"}


def to_dev(g, a_mask=None):
    o = {k: torch.from_numpy(np.array(g[k])).cuda() for k in ("p_plddt", "p_pae", "x_pred")}
    f = {k: torch.from_numpy(np.array(g[k])).cuda() for k in FEAT_KEYS}
    if a_mask is not None:
        f["a_mask"] = torch.from_numpy(np.array(a_mask)).cuda()
    return o, f


def same_bits(a, b):
    return all(torch.equal(a[k], b[k]) for k in SHAPES) and set(a) == set(b) == set(SHAPES)


@pytest.mark.parametrize("name", METRICS_CASES)
def test_values_and_decisions_vs_reference(name):
    from physdock_amd import get_metrics, predicted_tm_score
    g = load_metrics(name)
    o, f = to_dev(g)
    m = get_metrics(o, f)
    P, A, T = g["f64_ptm"].shape[0], g["a_mask"].shape[0], g["s_mask"].shape[0]
    dims = {"P": P, "A": A, "T": T}
    for k, s in SHAPES.items():
        assert m[k].shape == tuple(dims[c] for c in s) and m[k].is_cuda, k
        assert m[k].dtype == (torch.int64 if k == "has_clash" else torch.float32), k
    for q in QUANTITIES:
        got = m[q].double().cpu().numpy()
        if q == "pae":
            s, s2 = g["sum_f64_pae"]
            e = bound(g, q)
            assert abs(got.sum() - s) <= got.size * e and abs((got ** 2).sum() - s2) <= got.size * e * (2 * np.abs(g["f64_pae"]).max() + e)
            got = got[:, g["pae_rows"]]
        err = np.abs(got - g["f64_" + q]).max()
        print(f"{name} {q}: max |hip - f64| {err:.3e}  e32 {float(g['e32_' + q]):.3e}  bound {bound(g, q):.3e}")
        assert err <= bound(g, q), (name, q)
    # decisions, exact
    lg = o["p_pae"]
    for q, interface in enumerate((False, True)):
        val, row, per = predicted_tm_score(lg, f["s_mask"], f["asym_id"], interface=interface, return_row=True)
        assert row.cpu().reshape(-1).tolist() == g["f64_rows"][:, q].tolist(), (name, interface)
        assert torch.equal(val.reshape(-1), m["iptm" if interface else "ptm"])
        assert torch.equal(per.reshape(P, T)[torch.arange(P, device="cuda"), row.reshape(-1).long()].reshape(-1), val.reshape(-1))
        assert torch.equal(predicted_tm_score(lg, f["s_mask"], f["asym_id"], interface=interface).reshape(-1), val.reshape(-1))
    nposes = P if P > 1 else 1
    assert m["has_clash"].cpu().tolist() == g["ref_has_clash"][:nposes].tolist()
    ms = get_metrics(o, f, skip_self_pairs=True)
    assert ms["has_clash"].cpu().tolist() == g["f64_has_clash_skip"][:nposes].tolist()
    if P == 1:
        for skip, want in ((False, g["ref_has_clash"]), (True, g["f64_has_clash_skip"])):
            ma = get_metrics(o, f, all_poses=True, skip_self_pairs=skip)
            assert ma["has_clash"].cpu().tolist() == want.tolist(), (name, skip)
            rc = 0.8 * ma["iptm"].double() + 0.2 * ma["ptm"].double() - ma["has_clash"].double()
            assert ma["ranking_confidence"].shape == (len(want),) and float((ma["ranking_confidence"].double() - rc).abs().max()) <= 1.2e-7
            assert all(torch.equal(ma[k], m[k]) for k in ("atom_plddts", "mean_plddt", "pae", "ptm", "iptm"))
    if name == "onechain":
        assert float(m["iptm"]) == 0.0
    if name == "chains3":
        assert m["has_clash"].tolist() == [1] and ms["has_clash"].tolist() == [0]
        assert abs(float(ms["ranking_confidence"]) - float(m["ranking_confidence"]) - 1.0) <= 1.2e-7


def test_clash_rules_per_pose_and_public_pieces():
    """each pose of `clash` under its own atom mask (ratio rule alone, count rule alone, the boundary 100 / 200, masked and ligand
    atoms only), through get_metrics and through get_has_clash; compute_plddt / compute_predicted_aligned_error return get_metrics' bits"""
    from physdock_amd import compute_plddt, compute_predicted_aligned_error, get_has_clash, get_metrics
    g = load_metrics("clash")
    o, f = to_dev(g)
    a2t = f["atom_id_to_token_id"]
    for b in range(5):
        ob, fb = to_dev(g, a_mask=g["a_mask_pose"][b])
        ob["x_pred"] = ob["x_pred"][b:b + 1]
        for skip, want in ((False, g["ref_has_clash_pose"]), (True, g["f64_has_clash_pose_skip"])):
            assert get_metrics(ob, fb, skip_self_pairs=skip)["has_clash"].tolist() == [int(want[b])], (b, skip)
        for dtype in (torch.bool, torch.float32, torch.int64):      # `is_ligand == 0` for every dtype
            poly = (fb["is_ligand"].to(dtype) == 0)[a2t]
            got = get_has_clash(ob["x_pred"][0], fb["a_mask"], fb["asym_id"][a2t], poly.to(dtype))
            assert got.shape == () and got.dtype == torch.int64 and int(got) == int(g["ref_has_clash_pose"][b])
    allp = get_has_clash(o["x_pred"], f["a_mask"], f["asym_id"][a2t], (f["is_ligand"] == 0)[a2t])
    assert allp.tolist() == g["ref_has_clash"].tolist()
    fl = dict(f, is_ligand=f["is_ligand"].float())                  # a float is_ligand, which the reference's `~` refuses
    m, mf = get_metrics(o, f), get_metrics(o, fl)
    assert same_bits(m, mf)
    assert torch.equal(compute_plddt(o["p_plddt"]), m["atom_plddts"][0])
    r = compute_predicted_aligned_error(o["p_pae"])
    assert torch.equal(r["predicted_aligned_error"], m["pae"][0])
    assert float(r["max_predicted_aligned_error"]) == float(np.float32(centres(64)[-1]))


def test_first_maximal_row_wins_a_tie():
    """rows 3 and 7 of p_pae bit-identical and the best: the chosen row is 3, per_alignment of the two rows is bit-equal"""
    from physdock_amd import predicted_tm_score
    g = load_metrics("small")
    o, f = to_dev(g)
    assert float(f["s_mask"][3]) == float(f["s_mask"][7]) == 1.0 and int(f["asym_id"][3]) == int(f["asym_id"][7])
    lg = o["p_pae"].clone()
    lg[3] = -0.5 * torch.arange(64, device="cuda")[None, :].float() + 0.25 * lg[3]     # mass on the low-error bins: the best row
    lg[7] = lg[3]
    # the two rows see the same inter-chain mask only where columns 3 and 7 agree too, which they do: same chain
    for interface in (False, True):
        val, row, per = predicted_tm_score(lg, f["s_mask"], f["asym_id"], interface=interface, return_row=True)
        assert int(row) == 3, (interface, int(row))
        assert torch.equal(per[3], per[7]) and float(per[3]) == float(val)
        assert float(per[3]) > float(torch.cat([per[:3], per[4:7], per[8:]]).max())
    lg[3], lg[7] = o["p_pae"][3], lg[3].clone()                                         # only row 7 left: it wins
    assert int(predicted_tm_score(lg, f["s_mask"], f["asym_id"], return_row=True)[1]) == 7


def test_unbatched_equals_each_slice_of_the_stacked_call():
    from physdock_amd import get_metrics
    g = load_metrics("mid")
    o, f = to_dev(g)
    m = get_metrics(o, f)
    again = get_metrics(o, f)
    assert same_bits(m, again)                                       # determinism: two calls, identical bits
    for p in range(3):
        one = get_metrics({"p_plddt": o["p_plddt"][p], "p_pae": o["p_pae"][p], "x_pred": o["x_pred"][p:p + 1]}, f)
        for k in SHAPES:
            assert torch.equal(one[k], m[k][p:p + 1]), (p, k)
    with pytest.raises(ValueError, match="x_pred with 3 rows"):
        get_metrics(dict(o, x_pred=o["x_pred"][:2]), f)


def test_all_poses_equals_single_pose_calls():
    from physdock_amd import get_metrics
    g = load_metrics("clash")
    o, f = to_dev(g)
    ma = get_metrics(o, f, all_poses=True)
    assert ma["has_clash"].shape == (5,) and ma["ranking_confidence"].shape == (5,) and ma["ptm"].shape == (1,)
    for b in range(5):
        one = get_metrics(dict(o, x_pred=o["x_pred"][b:b + 1]), f)
        assert torch.equal(one["has_clash"], ma["has_clash"][b:b + 1]) and torch.equal(one["ranking_confidence"], ma["ranking_confidence"][b:b + 1])
        assert all(torch.equal(one[k], ma[k]) for k in ("atom_plddts", "mean_plddt", "pae", "ptm", "iptm"))
    assert "_metrics_chain" in f and f["_metrics_chain"][2] == 3     # the cached chain index: three chains


def test_buffers_and_masking():
    """the launchers write the real [P,A] / [P,T,T] extents only (sentinel-filled, one row longer), and a token with s_mask = 0
    contributes nothing to pTM: its logits can change without changing a bit of the other rows"""
    from physdock_amd import _lib as ops
    from physdock_amd import metrics
    g = load_metrics("small")
    o, f = to_dev(g)
    L = ops.init()
    A, T = 61, 24
    NAN = float("nan")
    atom = torch.full((A + 7,), NAN, device="cuda")
    mean = torch.full((2,), NAN, device="cuda")
    ops.check(L.pd_metrics_plddt(ops.ptr(o["p_plddt"]), ops.ptr(atom), ops.ptr(mean), 1, A, 50, ops.stream()), "plddt")
    pae = torch.full((T * T + T,), NAN, device="cuda")
    ptm, iptm = torch.full((2,), NAN, device="cuda"), torch.full((2,), NAN, device="cuda")
    rows = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    per = torch.full((2 * T + 5,), NAN, device="cuda")
    ws = torch.full((L.pd_metrics_workspace_numel(1, T) + 3,), NAN, device="cuda")
    asym = f["asym_id"].to(torch.int32)
    ops.check(L.pd_metrics_pae_tm(ops.ptr(o["p_pae"]), ops.ptr(metrics.bin_centres("cuda")), ops.ptr(f["s_mask"]), ops.ptr(asym), ops.ptr(ws),
                                  ops.ptr(pae), ops.ptr(ptm), ops.ptr(iptm), ops.ptr(rows), ops.ptr(per), 1, T, 64, ops.stream()), "pae_tm")
    m = metrics.get_metrics(o, f)
    assert torch.equal(atom[:A], m["atom_plddts"][0]) and torch.isnan(atom[A:]).all() and torch.equal(mean[:1], m["mean_plddt"]) and torch.isnan(mean[1:]).all()
    assert torch.equal(pae[:T * T].reshape(T, T), m["pae"][0]) and torch.isnan(pae[T * T:]).all()
    assert torch.equal(ptm[:1], m["ptm"]) and torch.equal(iptm[:1], m["iptm"]) and torch.isnan(ptm[1:]).all() and torch.isnan(iptm[1:]).all()
    assert rows.tolist()[:2] == g["f64_rows"][0].tolist() and rows.tolist()[2:] == [-7, -7]
    assert not torch.isnan(per[:2 * T]).any() and torch.isnan(per[2 * T:]).all() and torch.isnan(ws[-3:]).all()
    # masked tokens: per_alignment of a masked row is 0; another logit row / column there changes nothing else
    masked = torch.nonzero(f["s_mask"] == 0).reshape(-1)
    assert len(masked) >= 3 and not per[:2 * T].reshape(2, T)[:, masked].any()
    lg = o["p_pae"].clone()
    lg[masked] = 3.0 - lg[masked]
    lg[:, masked] = 1.0 - lg[:, masked]
    m2 = metrics.get_metrics(dict(o, p_pae=lg), f)
    assert torch.equal(m2["ptm"], m["ptm"]) and torch.equal(m2["iptm"], m["iptm"]) and torch.equal(m2["ranking_confidence"], m["ranking_confidence"])
    keep = torch.ones(T, dtype=torch.bool, device="cuda")
    keep[masked] = False
    assert torch.equal(m2["pae"][0][keep][:, keep], m["pae"][0][keep][:, keep]) and not torch.equal(m2["pae"], m["pae"])


def test_graph_capture_and_replay():
    from physdock_amd import get_metrics
    g = load_metrics("small")
    o, f = to_dev(g)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        get_metrics(o, f)                                            # warm-up: fills the chain-index and bin-centre caches
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        captured = get_metrics(o, f)
    new = {"p_plddt": 0.5 - o["p_plddt"], "p_pae": torch.flip(o["p_pae"], dims=(0,)).contiguous(), "x_pred": o["x_pred"] + 0.25}
    eager = get_metrics(new, f)
    torch.cuda.synchronize()
    for k in new:
        o[k].copy_(new[k])
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, eager)
    assert not torch.equal(eager["pae"], get_metrics({k: torch.from_numpy(np.array(g[k])).cuda() for k in new}, f)["pae"])


def test_launcher_guards():
    from physdock_amd import _lib as ops
    from physdock_amd import metrics
    L = ops.init()
    g = load_metrics("small")
    o, f = to_dev(g)
    A, T, st = 61, 24, ops.stream()
    SENT = -3.0
    buf = lambda n, dt=torch.float32: torch.full((n,), SENT, dtype=dt, device="cuda")
    atom, mean, pae, ptm, iptm, per = buf(A), buf(1), buf(T * T), buf(1), buf(1), buf(2 * T)
    rows, ws, cnt, has, rank = buf(2, torch.int32), buf(L.pd_metrics_workspace_numel(1, T)), buf(9, torch.int32), buf(1, torch.int64), buf(1)
    lp, la, cen, w, asym = o["p_plddt"], o["p_pae"], metrics.bin_centres("cuda"), f["s_mask"], f["asym_id"].to(torch.int32)
    x, am = o["x_pred"], f["a_mask"]
    chain, poly, n = metrics._dense_chain(f["asym_id"][f["atom_id_to_token_id"]])[0], (f["is_ligand"] == 0)[f["atom_id_to_token_id"]].float(), 3
    P = ops.ptr
    assert L.pd_metrics_plddt(P(lp), P(atom), P(mean), 1, A, 65, st) == PD_ERR_UNSUPPORTED
    assert L.pd_metrics_plddt(P(lp), P(atom), P(mean), 1, 0, 50, st) == PD_ERR_ARG
    assert L.pd_metrics_plddt(P(lp), P(atom), P(mean), 0, A, 50, st) == PD_ERR_ARG
    assert L.pd_metrics_plddt(None, P(atom), P(mean), 1, A, 50, st) == PD_ERR_ARG
    assert L.pd_metrics_plddt(P(lp), None, P(mean), 1, A, 50, st) == PD_ERR_ARG
    args = [P(la), P(cen), P(w), P(asym), P(ws), P(pae), P(ptm), P(iptm), P(rows), P(per), 1, T, 64, st]
    def pae_tm(**kw):
        a = list(args)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.pd_metrics_pae_tm(*a)
    assert pae_tm(_12=65) == PD_ERR_UNSUPPORTED and pae_tm(_10=65536) == PD_ERR_UNSUPPORTED
    assert pae_tm(_11=0) == PD_ERR_ARG and pae_tm(_11=-4) == PD_ERR_ARG and pae_tm(_12=0) == PD_ERR_ARG and pae_tm(_10=0) == PD_ERR_ARG
    for k in (0, 1, 2, 4, 6, 7, 8):                              # asym_id, pae and per_alignment are nullable
        assert pae_tm(**{f"_{k}": None}) == PD_ERR_ARG, k
    cargs = [P(x), P(am), P(chain), P(poly), P(cnt), P(ptm), P(iptm), 0, P(has), P(rank), 1, A, n, 0, st]
    def clash(**kw):
        a = list(cargs)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.pd_metrics_clash(*a)
    assert clash(_12=65) == PD_ERR_UNSUPPORTED and clash(_11=46341) == PD_ERR_UNSUPPORTED
    assert clash(_12=0) == PD_ERR_ARG and clash(_11=0) == PD_ERR_ARG and clash(_10=0) == PD_ERR_ARG and clash(_7=2) == PD_ERR_ARG
    for k in (0, 1, 2, 3, 4, 8):
        assert clash(**{f"_{k}": None}) == PD_ERR_ARG, k
    assert clash(_5=None) == PD_ERR_ARG                          # a ranking output needs ptm and iptm
    assert L.pd_metrics_workspace_numel(1, 0) == PD_ERR_ARG and L.pd_metrics_workspace_numel(65535, 46340) == PD_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for t in (atom, mean, pae, ptm, iptm, per, ws, rank):        # nothing was launched
        assert (t == SENT).all()
    assert (rows == -3).all() and (cnt == -3).all() and (has == -3).all()
    with pytest.raises(ValueError, match="at most 64 chains"):
        metrics._clash(x, am, chain, poly, 65, False)
    # the valid calls still work afterwards, with the nullable outputs left out
    assert pae_tm(_3=None, _5=None, _9=None) == 0 and clash(_5=None, _6=None, _9=None) == 0
    torch.cuda.synchronize()
    assert float(iptm) == 0.0 and rows.tolist()[1] == 0 and (pae == SENT).all() and has.tolist() == g["ref_has_clash"][:1].tolist()
