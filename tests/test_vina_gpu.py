"""pd_vina_score (csrc/vina.hip) straight on the C ABI, VinaScore.score, and the vina keyword of redock / redock_many.

The yardstick is the float64 restatement tests/vina_ref.py, which also derives the fp32 error bound of every output element from the
rounding of the distance, of each term's own arithmetic, of expf (1 ulp) and of the sums (its docstring); the device must satisfy
|dev - ref| <= bound element by element, with nothing multiplied on.  The seeded cases keep every pair 1e-4 A clear of the cutoff
and of the kinks (tests/test_vina_cpu.py checks that on the CPU; it is asserted again here).  One `ENVELOPE | pd_vina_score | ...`
line is printed per output (pytest -s): largest |reference|, largest error, the bound at the element with the largest err / bound,
and that ratio - the source of the table in NOTES.md.  Output buffers are one row longer than needed and pre-filled with NaN."""
import numpy as np
import pytest
import torch

import vina_ref as ref

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN = float("nan")
OUTPUTS = ("atom_terms", "terms", "inter", "score", "per_atom", "forces")


# ------------------------------------------------------------------ sentinels, plumbing
def sentinel(*shape):
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), NAN, device="cuda")


def body(buf):
    torch.cuda.synchronize()
    assert torch.isnan(buf[-1]).all(), "the row behind the output was written"
    assert not torch.isnan(buf[:-1]).any(), "an output element kept its sentinel"
    return buf[:-1]


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


def tables(c):
    """a case's tables on the device, every index the kernel would follow checked to be inside its array first"""
    A = c["x"].shape[1]
    assert 0 <= c["lig_idx"].min() and c["lig_idx"].max() < A and len(c["types"]) == A == len(c["rec_mask"])
    assert len(c["lig_active"]) == len(c["lig_idx"]) and not c["rec_mask"][c["lig_idx"]].any()
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()
    return dict(lig_idx=up(c["lig_idx"], np.int32), types=up(c["types"], np.uint8), rec_mask=up(c["rec_mask"], np.uint8),
                lig_active=up(c["lig_active"], np.uint8))


def launch(L, x, c, d=None, forces=True):
    """one pd_vina_score call into sentinel buffers -> dict of the bodies"""
    d = d or tables(c)
    x = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    n, A, Lg = x.shape[0], x.shape[1], len(c["lig_idx"])
    assert A == len(c["types"])
    buf = dict(atom_terms=sentinel(n, Lg, 5), terms=sentinel(n, 5), inter=sentinel(n), score=sentinel(n), per_atom=sentinel(n, Lg))
    if forces:
        buf["forces"] = sentinel(n, Lg, 3)
    rc = L.pd_vina_score(P(x), P(d["lig_idx"]), P(d["types"]), P(d["rec_mask"]), P(d["lig_active"]), float(c["n_rot"]), P(buf["atom_terms"]),
                         P(buf["terms"]), P(buf["inter"]), P(buf["score"]), P(buf["per_atom"]), P(buf["forces"]) if forces else None,
                         n, A, Lg, S())
    assert rc == 0, rc
    return {k: body(v) for k, v in buf.items()}


def oracle(c, x=None):
    return ref.vina(c["x"] if x is None else x, c["lig_idx"], c["types"], c["rec_mask"], c["lig_active"], c["n_rot"])


def check(case, out, want):
    """every output of the device against the restatement, element by element under its derived bound"""
    for k in OUTPUTS:
        if k not in out:
            continue
        dev, r, b = out[k].cpu().double().numpy(), want[k], want["bound"][k]
        assert dev.shape == r.shape == b.shape, (case, k, dev.shape, r.shape)
        err = np.abs(dev - r)
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
        worst = np.unravel_index(np.argmax(ratio), ratio.shape) if ratio.ndim else ()
        print(f"ENVELOPE | pd_vina_score | {case} {k} | {np.abs(r).max():.2e} | {err.max():.2e} | {b[worst]:.2e} | {ratio.max():.2f} |")
        assert (err <= b).all(), (case, k, "err", err.max(), "bound", b[worst], "ratio", ratio.max())


def same(a, b, keys=None):
    return all(torch.equal(a[k], b[k]) for k in (keys or a))


# ------------------------------------------------------------------ cases 1 - 3: accuracy and exactness
def test_the_cases_are_the_shapes_that_take_every_path():
    shapes = {(n, A, len(lig)) for n, A, lig, _, _ in ref.CASES.values()}
    assert shapes == {(3, 300, 5), (2, 65, 1), (2, 257, 3)}
    n, A, lig, inactive, _ = ref.CASES["P3_A300_L5"]
    assert A - 1 in lig and 256 in lig and inactive is not None and sorted(lig) == list(lig) and np.diff(lig).max() > 1
    c = ref.make_case("P3_A300_L5")
    assert set((c["types"] & 15).tolist()) == set(range(10)) and set((c["types"] >> 4).tolist()) == set(range(8))
    assert (c["rec_mask"] == 0).sum() > len(lig)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_kernel_against_float64(L, name):
    c = ref.make_case(name)
    want = oracle(c)
    assert want["margin"] >= ref.MARGIN and (want["terms"] > 0).all(), "the case must keep clear of the kinks and use every term"
    d = tables(c)
    out = launch(L, c["x"], c, d)
    check(name, out, want)
    n = c["x"].shape[0]
    # bit-identical from launch to launch
    assert same(launch(L, c["x"], c, d), out)
    # a pose scored alone is the pose scored inside the batch
    for p in range(n):
        one = launch(L, c["x"][p:p + 1], c, d)
        assert all(torch.equal(one[k][0], out[k][p]) for k in out), (name, p)
    # reversing the poses reverses the outputs
    rev = launch(L, c["x"][::-1], c, d)
    assert all(torch.equal(rev[k].flip(0), out[k]) for k in out), name
    # without the forces the other outputs are what they were
    bare = launch(L, c["x"], c, d, forces=False)
    assert "forces" not in bare and same(bare, out, list(bare))
    # inactive ligand atoms report exact zeros
    off = torch.from_numpy(c["lig_active"] == 0).cuda()
    assert not out["atom_terms"][:, off].any() and not out["forces"][:, off].any() and not out["per_atom"][:, off].any()


def test_a_ligand_beyond_the_cutoff_scores_exactly_zero(L):
    c = ref.make_case("P3_A300_L5")
    x = c["x"].copy()
    x[1, c["lig_idx"]] += np.float32([60.0, 0.0, 0.0])                # pose 1: the ligand 60 A away; poses 0 and 2 as they were
    want = oracle(c, x)
    assert want["n_pairs"][1] == 0 and want["n_pairs"][0] > 0 and want["margin"] >= ref.MARGIN
    out = launch(L, x, c)
    for k in out:
        assert not out[k][1].any(), k
    check("far ligand", out, want)
    assert same({k: v[[0, 2]] for k, v in out.items()}, {k: v[[0, 2]] for k, v in launch(L, c["x"], c).items()})


def test_a_coincident_pair_is_finite_and_contributes_no_force(L):
    c = ref.make_case("P2_A257_L3")
    x = c["x"].copy()
    j = int(np.nonzero(c["rec_mask"])[0][5])
    i = 1
    x[0, j] = x[0, c["lig_idx"][i]]                                    # pose 0: receptor atom j sits exactly on ligand atom i
    want = oracle(c, x)
    assert want["margin"] >= ref.MARGIN
    rsum = ref.CLASS_RADII[c["types"][c["lig_idx"][i]] & 15] + ref.CLASS_RADII[c["types"][j] & 15]
    assert want["pair_terms"][2, 0, i, j] == pytest.approx(rsum ** 2) and not want["pair_force"][0, i, j].any()
    out = launch(L, x, c)
    assert all(torch.isfinite(v).all() for v in out.values())
    check("coincident pair", out, want)                                # the repulsion of the pair is in atom_terms and terms
    # moving the coincident receptor atom away adds a force: without it the force of atom i is that of the other pairs alone
    c2 = dict(c, rec_mask=c["rec_mask"].copy())
    c2["rec_mask"][j] = 0
    without = launch(L, x, c2)
    assert torch.equal(without["forces"][0, i], out["forces"][0, i])
    assert float(out["atom_terms"][0, i, 2] - without["atom_terms"][0, i, 2]) == pytest.approx(rsum ** 2, rel=1e-5)


# ------------------------------------------------------------------ argument handling
def test_argument_handling(L):
    c = ref.make_case("P2_A65_L1")
    d = tables(c)
    x = torch.from_numpy(c["x"]).cuda()
    n, A, Lg = 2, 65, 1
    bufs = [sentinel(n, Lg, 5), sentinel(n, 5), sentinel(n), sentinel(n), sentinel(n, Lg), sentinel(n, Lg, 3)]
    names = ["x", "lig_idx", "type", "rec_mask", "lig_active", "n_rot", "atom_terms", "terms", "inter", "score", "per_atom", "forces"]
    good = [P(x), P(d["lig_idx"]), P(d["types"]), P(d["rec_mask"]), P(d["lig_active"]), 3.0] + [P(b) for b in bufs]
    rcs = {}
    for k, name in enumerate(names):
        if name not in ("n_rot", "forces"):
            args = list(good)
            args[k] = None
            rcs["null " + name] = L.pd_vina_score(*args, n, A, Lg, S())
    for k, name in enumerate(["P", "A", "L"]):
        sz = [n, A, Lg]
        sz[k] = 0
        rcs[name + "=0"] = L.pd_vina_score(*good, *sz, S())
        sz[k] = -1
        rcs[name + "<0"] = L.pd_vina_score(*good, *sz, S())
    for k, name in enumerate(names):
        if name in ("x", "lig_idx", "atom_terms", "terms", "inter", "score", "per_atom", "forces"):
            args = list(good)
            args[k] = good[k] + 2                                      # a float / int pointer off its 4-byte alignment
            rcs["misaligned " + name] = L.pd_vina_score(*args, n, A, Lg, S())
    rcs["n_rot<0"] = L.pd_vina_score(*good[:5], -1.0, *good[6:], n, A, Lg, S())
    rcs["n_rot nan"] = L.pd_vina_score(*good[:5], NAN, *good[6:], n, A, Lg, S())
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), rcs
    unsupported = {"L": L.pd_vina_score(*good, n, A, 1025, S()), "A": L.pd_vina_score(*good, n, (1 << 22) + 1, Lg, S()),
                   "P": L.pd_vina_score(*good, 65536, A, Lg, S())}
    assert all(rc == PD_ERR_UNSUPPORTED for rc in unsupported.values()), unsupported
    torch.cuda.synchronize()
    assert all(torch.isnan(b).all() for b in bufs), "a rejected call wrote"
    assert L.pd_vina_score(*good[:-1], None, n, A, Lg, S()) == 0      # forces may be NULL
    for b in bufs[:-1]:
        body(b)
    assert torch.isnan(bufs[-1]).all()


# ------------------------------------------------------------------ VinaScore.score, graph capture
def vina_of(c, device="cuda"):
    from physdock_amd.scoring import VinaScore
    rec = c["rec_mask"].copy()
    return VinaScore.from_types(c["types"], c["lig_idx"], rec, c["n_rot"], ligand_active=c["lig_active"], device=device)


def test_score_agrees_with_the_c_abi_and_captures_into_a_graph(L):
    c = ref.make_case("P3_A300_L5")
    v = vina_of(c)
    assert np.array_equal(v.rec_mask, c["rec_mask"]) and np.array_equal(v.lig_active, c["lig_active"])
    x = torch.from_numpy(c["x"]).cuda()
    raw = launch(L, c["x"], c)
    out = v.score(x, forces=True)
    assert set(out) == {"score", "inter", "terms", "per_atom", "forces"} and all(t.is_cuda and t.dtype == torch.float32 for t in out.values())
    assert out["score"].shape == (3,) and out["terms"].shape == (3, 5) and out["per_atom"].shape == (3, 5) and out["forces"].shape == (3, 5, 3)
    assert same(out, raw, list(out))
    plain = v.score(x)
    assert set(plain) == {"score", "inter", "terms", "per_atom"} and same(plain, raw, list(plain))
    with pytest.raises(ValueError, match="pose atoms"):
        v.score(x[:, :-1])
    # capture, then replay on other coordinates
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    xs = x.clone()
    with torch.cuda.stream(s):
        v.score(xs, forces=True)
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        captured = v.score(xs, forces=True)
    xs.copy_(x.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(captured[k], out[k].flip(0)) for k in out)
    check("VinaScore.score", {k: t for k, t in out.items()}, oracle(c))


# ------------------------------------------------------------------ redock, redock_many
@pytest.fixture(scope="module")
def small(small_model_inputs):
    from physdock_amd import PhysDock
    cfg, P_, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P_, strict=True)
    return model.cuda().eval(), {k: v.cuda() for k, v in batch.items()}, cfg


def chain_bonds(batch):
    from physdock_amd.driver import ligand_atom_mask
    return [(i, i + 1) for i in range(int(ligand_atom_mask(batch).sum()) - 1)]


def same_result(a, b):
    """two redock results: the same keys, bit-equal tensors, equal everything else"""
    def eq(u, w):
        if isinstance(u, torch.Tensor):
            return isinstance(w, torch.Tensor) and torch.equal(u, w)
        if isinstance(u, dict):
            return isinstance(w, dict) and set(u) == set(w) and all(eq(u[k], w[k]) for k in u)
        return u == w
    return eq(a, b)


def test_redock_reports_the_score_and_changes_nothing_else(small):
    from physdock_amd import driver
    from physdock_amd.ranking import rank_by_score
    from physdock_amd.scoring import VinaScore
    from physdock_amd.validity import PoseValidity
    model, dbatch, _ = small
    bonds = chain_bonds(dbatch)
    vina = VinaScore.from_batch(dbatch, bonds)
    validity = PoseValidity.from_batch(dbatch, bonds)
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, dbatch, **kw)
    assert same_result(plain, driver.redock(model, dbatch, **kw)), "the path without the keyword is deterministic"
    out = driver.redock(model, dbatch, vina=vina, **kw)
    assert set(out) == set(plain) | {"vina", "order_vina"}
    assert same_result({k: out[k] for k in plain}, plain)
    assert same(out["vina"], vina.score(out["poses"])) and out["vina"]["score"].shape == (4,) and out["order_vina"].is_cuda
    assert torch.equal(out["order_vina"], rank_by_score(out["vina"]))
    sc = out["vina"]["score"].cpu().tolist()
    assert out["order_vina"].tolist() == sorted(range(4), key=lambda p: (sc[p], p))
    both = driver.redock(model, dbatch, vina=vina, validity=validity, **kw)
    assert set(both) == set(plain) | {"vina", "order_vina", "validity", "order_vina_valid"}
    assert same(both["vina"], out["vina"]) and torch.equal(both["order_vina"], out["order_vina"])
    vl = both["validity"]["valid"].cpu().tolist()
    order = both["order_vina"].tolist()
    assert both["order_vina_valid"].tolist() == [p for p in order if vl[p]] + [p for p in order if not vl[p]]
    # the score of the kept poses against the restatement
    host = dict(x=out["poses"].cpu().numpy(), lig_idx=vina.ligand_idx, types=vina.types, rec_mask=vina.rec_mask, lig_active=vina.lig_active,
                n_rot=vina.n_rot)
    want = oracle(host)
    if want["margin"] >= ref.MARGIN:
        check("redock poses", out["vina"], want)
    many = driver.redock_many(model, [(dbatch, {"vina": vina})], **kw)               # one system: the sequential path
    assert same_result(many[0], out)
    grouped = driver.redock_many(model, [(dbatch, {"vina": vina, "validity": validity})], group=1, **kw)
    assert same(grouped[0]["vina"], vina.score(grouped[0]["poses"])) and "order_vina_valid" in grouped[0]
