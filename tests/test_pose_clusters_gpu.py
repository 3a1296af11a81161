"""pd_pose_clusters (csrc/cluster.hip) straight on the C ABI, PoseClusters, and the clusters keyword of redock / redock_many.

The yardstick is tests/pose_clusters_ref.py fed the same fp32 matrix.  Every integer output must EQUAL the restatement and every float
output must hold the same BITS: each is a copy of an entry of D, an exact fp32 maximum, or an IEEE fp64 sum in the stated order followed
by one fp64 division and one rounding to fp32 - nothing is left to a tolerance.  Output buffers are one element longer than needed and
pre-filled with a sentinel (-7777 / -7777.0; NaN is a legitimate output here).

Shapes: n = 1; the hand-worked n = 5; 70 is no multiple of a wave; 257 is one sweep of the 1024 threads with a tail, 1030 two sweeps with
a tail (and two pieces of `order`); planted modes interleave in pose id under a seeded non-identity order; one cluster; n singletons
(K = n, the longest chain of leaders); entries exactly at the cutoff; a NaN pair; the best pose invalid; all invalid; tied scores; no
score.  Out-of-range entries of `order` are not fed to the device: that guard is specified, not exercised here."""
import numpy as np
import pytest
import torch

import pose_clusters_ref as ref

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
SENT = -7777
NAMES = ("labels", "dist_to_leader", "leader", "size", "radius", "medoid", "spread", "mean_score", "n_clusters")


@pytest.fixture(scope="module")
def L():
    from physdock_amd import ops
    return ops._lib.init()


def P(t):
    from physdock_amd import ops
    return ops.ptr(t)


def S():
    from physdock_amd import ops
    return ops.stream()


def up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def buffers(n):
    dt = lambda k: torch.int32 if k in ref.INT_KEYS else torch.float32
    return {k: torch.full(((1 if k == "n_clusters" else n) + 1,), SENT, dtype=dt(k), device="cuda") for k in NAMES}


def untouched(t):
    return bool((t == SENT).all())


def launch(L, c, ws_extra=1):
    """one pd_pose_clusters call into sentinel buffers -> (numpy dict of the outputs, the raw buffers)"""
    n = c["D"].shape[0]
    assert c["D"].shape == (n, n) and c["D"].dtype == np.float32 and c["order"].shape == (n,) and c["order"].dtype == np.int32
    assert 0 <= c["order"].min() and c["order"].max() < n, "no out-of-range entry goes to the device"
    D, order, valid, score = up(c["D"]), up(c["order"]), up(c["valid"]), up(c["score"])
    numel = L.pd_pose_clusters_workspace_numel(n)
    assert numel == n
    ws = torch.full((numel + ws_extra,), float(SENT), dtype=torch.float64, device="cuda")
    b = buffers(n)
    rc = L.pd_pose_clusters(P(D), P(order), float(c["cutoff"]), P(valid), P(score), P(ws), numel, *(P(b[k]) for k in NAMES), n, S())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all(untouched(v[-1:]) for v in b.values()) and untouched(ws[numel:]), "an element behind an output was written"
    assert not any((v[:-1] == SENT).any() for v in b.values()) and not (ws[:numel] == SENT).any(), "an output element kept its sentinel"
    return {k: v[:-1].cpu().numpy() for k, v in b.items()}, b


def differing(got, want):
    return [k for k in ref.INT_KEYS if not np.array_equal(got[k], want[k])] + [k for k in ref.FLOAT_KEYS if not ref.same_bits(got[k], want[k])]


# ------------------------------------------------------------------ the C ABI against the restatement
@pytest.mark.parametrize("name", list(ref.CASES))
def test_kernel_equals_the_restatement(L, name):
    c = ref.make_case(name)
    want = ref.restate(c["D"], c["order"], c["cutoff"], valid=c["valid"], score=c["score"])
    got, raw = launch(L, c)
    print(f"CASE | {name} | n {c['D'].shape[0]} | clusters {int(got['n_clusters'][0])} (restatement {int(want['n_clusters'][0])}) | "
          f"largest {int(got['size'].max())}")
    assert differing(got, want) == [], name
    ref.check_invariants(c["D"], c["order"], c["cutoff"], got, valid=c["valid"])
    again, raw2 = launch(L, c)
    assert all(torch.equal(raw[k].view(torch.int32), raw2[k].view(torch.int32)) for k in NAMES), "two calls on the same input give identical bytes"


def test_the_hand_worked_case_against_its_literals(L):
    got, _ = launch(L, ref.hand_case())
    for k, v in ref.HAND.items():
        head = got[k] if k in ref.INT_KEYS or k == "dist_to_leader" else got[k][:2]
        assert ref.same_bits(head, np.asarray(v, np.float32)) if k in ref.FLOAT_KEYS else head.tolist() == v, k
    assert all(np.isnan(got[k][2:]).all() for k in ("radius", "spread", "mean_score"))


def test_shapes_at_the_sweep_boundary(L):
    """n = 1023, 1024, 1025: the last column of a sweep, a full sweep and one column into the second"""
    for n in (1023, 1024, 1025):
        c = dict(D=ref.planted(n, modes=5, seed=n), order=ref.permutation(n, n + 1), cutoff=2.0, valid=None, score=None)
        got, _ = launch(L, c)
        assert differing(got, ref.restate(c["D"], c["order"], c["cutoff"])) == [], n


def test_argument_handling(L):
    c = ref.make_case("n70_planted")
    n = 70
    D, order, score = up(c["D"]), up(c["order"]), up(c["score"])
    valid = torch.ones(n, dtype=torch.uint8, device="cuda")
    ws = torch.full((n,), float(SENT), dtype=torch.float64, device="cuda")
    b = buffers(n)
    outs = [P(b[k]) for k in NAMES]

    def call(D_=P(D), order_=P(order), cutoff=2.0, valid_=P(valid), score_=P(score), ws_=P(ws), numel=n, outs_=outs, n_=n):
        return L.pd_pose_clusters(D_, order_, cutoff, valid_, score_, ws_, numel, *outs_, n_, S())

    rcs = {"n=0": call(n_=0), "n=-1": call(n_=-1), "cutoff<0": call(cutoff=-1.0), "cutoff nan": call(cutoff=float("nan")),
           "cutoff inf": call(cutoff=float("inf")), "short workspace": call(numel=n - 1), "null D": call(D_=None),
           "null order": call(order_=None), "null ws": call(ws_=None), "misaligned D": call(D_=P(D) + 2),
           "misaligned order": call(order_=P(order) + 2), "misaligned score": call(score_=P(score) + 2), "misaligned ws": call(ws_=P(ws) + 4)}
    for k, name in enumerate(NAMES):
        args = list(outs)
        args[k] = None
        rcs["null " + name] = call(outs_=args)
        args[k] = outs[k] + 2
        rcs["misaligned " + name] = call(outs_=args)
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), rcs
    assert call(n_=8193) == PD_ERR_UNSUPPORTED, "n = 8193 is refused before any buffer (these hold 70 poses) is looked at"
    assert L.pd_pose_clusters_workspace_numel(0) == PD_ERR_ARG and L.pd_pose_clusters_workspace_numel(8193) == PD_ERR_UNSUPPORTED
    assert L.pd_pose_clusters_workspace_numel(8192) == 8192
    torch.cuda.synchronize()
    assert all(untouched(v) for v in b.values()) and untouched(ws), "a rejected call wrote"
    assert call() == 0 and call(valid_=None, score_=None) == 0
    torch.cuda.synchronize()
    assert not any((v[:-1] == SENT).any() for v in b.values())


# ------------------------------------------------------------------ PoseClusters
def to_np(res):
    return {k: res[k].cpu().numpy() for k in ref.KEYS}


def test_cluster_agrees_with_the_c_abi_and_captures_into_a_graph(L):
    from physdock_amd import PoseClusters
    c = ref.make_case("n257_score_ties")
    raw, _ = launch(L, c)
    spec = PoseClusters(cutoff=c["cutoff"])
    D, order, score = up(c["D"]), up(c["order"]), up(c["score"])
    out = spec.cluster(D, order=order, scores=score)
    assert set(out) == set(ref.KEYS) and all(t.is_cuda for t in out.values())
    assert all(out[k].dtype == torch.int32 for k in ref.INT_KEYS) and all(out[k].dtype == torch.float32 for k in ref.FLOAT_KEYS)
    assert differing(to_np(out), raw) == []
    assert differing(to_np(spec.cluster(D, order=order.long(), scores={"score": score.double()})), raw) == [], "int64 order, a dict of scores"
    # the order from the scores: ascending, ties by pose id (rank_by_score); without either, the pose ids
    by_score = np.lexsort((np.arange(257), c["score"])).astype(np.int32)
    assert differing(to_np(spec.cluster(D, scores=score)), ref.restate(c["D"], by_score, c["cutoff"], score=c["score"])) == []
    assert differing(to_np(spec.cluster(D)), ref.restate(c["D"], np.arange(257, dtype=np.int32), c["cutoff"])) == []
    valid = torch.from_numpy(np.random.default_rng(1).random(257) < 0.8).cuda()
    want = ref.restate(c["D"], c["order"], c["cutoff"], valid=valid.cpu().numpy(), score=c["score"])
    assert differing(to_np(spec.cluster(D, order=order, scores=score, valid=valid)), want) == []
    told = spec.summary(out)
    K = int(raw["n_clusters"][0])
    assert len(told) == K == 5 and [m["leader"] for m in told] == raw["leader"][:K].tolist()
    assert all(m["members"] == np.nonzero(raw["labels"] == k)[0].tolist() and m["size"] == len(m["members"]) for k, m in enumerate(told))
    assert torch.equal(spec.representatives(out, per="medoid"), out["medoid"]) and spec.representatives(out) is out["leader"]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    Ds = D.clone()
    with torch.cuda.stream(st):
        spec.cluster(Ds, order=order, scores=score)
    st.synchronize()
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        captured = spec.cluster(Ds, order=order, scores=score)
    c2 = ref.make_case("n257_planted")
    Ds.copy_(up(c2["D"]))
    graph.replay()
    torch.cuda.synchronize()
    assert differing(to_np(captured), ref.restate(c2["D"], c["order"], c["cutoff"], score=c["score"])) == []


def symmetric_ligand_poses():
    """10 receptor atoms and a 6-atom ligand whose atoms 4 and 5 are exchanged by its one automorphism and lie 4 A apart.  Pose 0; pose 1
    = pose 0 with those two exchanged plus noise of 0.05 A; pose 2 = pose 0, the whole complex rotated and moved."""
    rng = np.random.default_rng(31)
    rec = rng.uniform(-8, 8, size=(10, 3))
    lig = np.array([[0, 0, 0], [1.5, 0, 0], [3.0, 0, 0], [4.5, 0, 0], [5.5, 2.0, 0], [5.5, -2.0, 0]], dtype=np.float64)
    a = np.concatenate([rec, lig])
    b = a.copy()
    b[[14, 15]] = a[[15, 14]]
    b[10:] += rng.uniform(-0.05, 0.05, size=(6, 3)) / np.sqrt(3.0)
    t = 0.7
    R = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1.0]])
    c = a @ R.T + np.array([3.0, -2.0, 5.0])
    x = torch.from_numpy(np.stack([a, b, c]).astype(np.float32)).cuda()
    w = torch.cat([torch.ones(10), torch.zeros(6)]).cuda()
    return x, torch.arange(10, 16, dtype=torch.int32, device="cuda"), w


def test_binding_modes_and_the_ligand_symmetry():
    from physdock_amd import LigandSymmetry, PoseClusters
    x, lig, w = symmetric_ligand_poses()
    sym = LigandSymmetry.from_permutations(np.array([[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 5, 4]], dtype=np.int32))
    spec = PoseClusters()                                              # 2.0 A

    def modes(**kw):
        out = spec.binding_modes(x, lig, **kw)
        D = out["dist"].cpu().numpy()
        assert out["dist"].shape == (3, 3) and out["x_common"].shape == x.shape
        order = kw.get("order")
        want = ref.restate(D, np.arange(3, dtype=np.int32) if order is None else order.cpu().numpy().astype(np.int32), 2.0)
        assert differing(to_np(out), want) == []
        return out, D

    out, D = modes(align_weights=w)
    assert abs(D[0, 1] - np.sqrt(2 * 16 / 6)) < 0.1 and D[0, 1] > 2.0 and D[0, 2] < 1e-3, "plain RMSD: the exchanged pose is 2.31 A away"
    assert out["labels"].tolist() == [0, 1, 0] and int(out["n_clusters"]) == 2
    out, D = modes(align_weights=w, symmetry=sym)
    assert D[0, 1] < 0.1 and out["labels"].tolist() == [0, 0, 0] and int(out["n_clusters"]) == 1 and int(out["size"][0]) == 3
    out, D = modes()                                                   # as they are: the moved complex is a mode of its own
    assert torch.equal(out["x_common"], x) and out["labels"].tolist() == [0, 1, 2]
    out, D = modes(symmetry=sym)
    assert out["labels"].tolist() == [0, 0, 1]
    out, D = modes(align_weights=w, symmetry=sym, order=torch.tensor([2, 1, 0], device="cuda"))
    assert int(out["leader"][0]) == 2 and torch.allclose(out["x_common"][2], x[2], atol=1e-3), "the default anchor is the first pose of the order"
    out, D = modes(align_weights=w, anchor=1)
    assert torch.allclose(out["x_common"][1], x[1], atol=1e-3)


# ------------------------------------------------------------------ redock, redock_many
@pytest.fixture(scope="module")
def small(small_model_inputs):
    from physdock_amd import PhysDock
    cfg, P_, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P_, strict=True)
    return model.cuda().eval(), {k: v.cuda() for k, v in batch.items()}, cfg


def same_result(a, b):
    def eq(u, w):
        if isinstance(u, torch.Tensor):
            return isinstance(w, torch.Tensor) and torch.equal(u, w)
        if isinstance(u, dict):
            return isinstance(w, dict) and set(u) == set(w) and all(eq(u[k], w[k]) for k in u)
        return u == w
    return eq(a, b)


def same_clusters(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) or ref.same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in a)


KW = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)


def test_redock_reports_the_clusters_and_changes_nothing_else(small):
    from physdock_amd import PoseClusters, driver
    model, dbatch, _ = small
    plain = driver.redock(model, dbatch, **KW)
    spec = PoseClusters(cutoff=2.0)
    out = driver.redock(model, dbatch, clusters=spec, **KW)
    assert "x_gt" in dbatch and set(out) == set(plain) | {"clusters"}
    assert same_result({k: out[k] for k in plain}, plain)
    cl = out["clusters"]
    assert set(cl) == set(ref.KEYS) | {"dist", "leader_rmsd"} and cl["dist"] is out["ranking"]["dist"], "the ranking's matrix is reused"
    D = cl["dist"].cpu().numpy()
    want = ref.restate(D, np.arange(4, dtype=np.int32), 2.0)
    assert differing(to_np(cl), want) == []
    K = int(want["n_clusters"][0])
    r = out["ranking"]["rmsd_all"].cpu().numpy()
    lr = cl["leader_rmsd"].cpu().numpy()
    assert ref.same_bits(lr[:K], r[want["leader"][:K]]) and np.isnan(lr[K:]).all()
    # without the ranking the matrix is computed here: the same values, no leader_rmsd
    bare = driver.redock(model, dbatch, clusters=spec, ranking=False, **KW)
    assert bare["ranking"] is None and set(bare["clusters"]) == set(ref.KEYS) | {"dist"}
    assert same_clusters(bare["clusters"], {k: v for k, v in cl.items() if k != "leader_rmsd"})
    many = driver.redock_many(model, [(dbatch, {"clusters": spec})], **KW)               # one system: the sequential path
    assert same_result({k: many[0][k] for k in plain}, plain) and same_clusters(many[0]["clusters"], cl)
    two = driver.redock_many(model, [(dbatch, {}), (dbatch, {"clusters": PoseClusters(0.5)})], streams=1, **KW)     # a per-system keyword
    assert same_result(two[0], plain) and same_result({k: two[1][k] for k in plain}, plain)
    assert differing(to_np(two[1]["clusters"]), ref.restate(D, np.arange(4, dtype=np.int32), 0.5)) == []
    grouped = driver.redock_many(model, [(dbatch, {"clusters": spec})], group=1, **KW)
    assert set(grouped[0]) == set(out)
    g = grouped[0]["clusters"]
    assert g["dist"] is grouped[0]["ranking"]["dist"]
    assert differing(to_np(g), ref.restate(g["dist"].cpu().numpy(), np.arange(4, dtype=np.int32), 2.0)) == []


def test_redock_orders_by_vina_and_clusters_interactions(small):
    from physdock_amd import PoseClusters, driver
    from physdock_amd.interactions import InteractionFingerprint
    from physdock_amd.scoring import VinaScore
    from physdock_amd.validity import PoseValidity
    model, dbatch, _ = small
    bonds = [(i, i + 1) for i in range(int(driver.ligand_atom_mask(dbatch).sum()) - 1)]
    vs, fp, pv = VinaScore.from_batch(dbatch, bonds), InteractionFingerprint.from_batch(dbatch, bonds), PoseValidity.from_batch(dbatch, bonds)
    tools = dict(vina=vs, interactions=fp, validity=pv)
    base = driver.redock(model, dbatch, **tools, **KW)
    out = driver.redock(model, dbatch, clusters=PoseClusters(1.0, by="vina"), **tools, **KW)
    assert set(out) == set(base) | {"clusters"} and same_result({k: out[k] for k in base}, base)
    cl = out["clusters"]
    score = out["vina"]["score"].cpu().numpy()
    order = out["order_vina"].cpu().numpy().astype(np.int32)
    assert order.tolist() == np.lexsort((np.arange(4), score)).tolist()
    valid = out["validity"]["valid"].cpu().numpy()
    want = ref.restate(cl["dist"].cpu().numpy(), order, 1.0, valid=valid, score=score)
    assert differing(to_np(cl), want) == []
    if valid[order[0]]:
        assert int(cl["leader"][0]) == int(order[0]), "mode 0 is led by the pose with the best score"
    inter = driver.redock(model, dbatch, clusters=PoseClusters(0.5, metric="interactions"), **tools, **KW)
    assert same_result({k: inter[k] for k in base}, base)
    ci = inter["clusters"]
    D = 1.0 - fp.pairwise(inter["interactions"]["bits"])
    assert torch.equal(ci["dist"], D) and not D.diagonal().any() and "leader_rmsd" in ci
    assert differing(to_np(ci), ref.restate(D.cpu().numpy(), np.arange(4, dtype=np.int32), 0.5, valid=valid, score=score)) == []
    many = driver.redock_many(model, [(dbatch, dict(tools, clusters=PoseClusters(1.0, by="vina")))], **KW)
    assert same_result({k: many[0][k] for k in base}, base) and same_clusters(many[0]["clusters"], cl)
