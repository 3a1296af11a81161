"""pd_vina_refine_energy and pd_vina_refine (csrc/vina_refine.hip) straight on the C ABI, VinaRefine.refine / .energy, and the refine
keyword of redock / redock_many.

The yardstick is the float64 restatement tests/vina_refine_ref.py.  The energy kernel must satisfy |dev - ref| <= bound element by
element, the bound derived there from float64 roundoff, the pair counts and the device exp's documented 1 ulp, nothing multiplied
on.  The refinement must take the reference's trajectory: equal iterations, evaluations and status, ligand coordinates within 1e-6 A
plus one fp32 ulp of the largest coordinate (the guard in tests/test_vina_refine_cpu.py holds the reference to 1e-8 A against its own
reversed summation).  One `ENVELOPE | pd_vina_refine_energy | ...` line is printed per output (pytest -s), and one
`TRAJECTORY | ...` line per case with the largest coordinate difference.  Output buffers are one row longer than needed and
pre-filled with a sentinel."""
import numpy as np
import pytest
import torch

import vina_ref
import vina_refine_ref as ref

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN = float("nan")
I_SENTINEL = -77


def sentinel(*shape, dtype=torch.float64):
    fill = NAN if dtype.is_floating_point else I_SENTINEL
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), fill, device="cuda", dtype=dtype)


def untouched(buf):
    return bool(torch.isnan(buf).all()) if buf.dtype.is_floating_point else bool((buf == I_SENTINEL).all())


def body(buf):
    torch.cuda.synchronize()
    assert untouched(buf[-1]), "the row behind the output was written"
    if buf.dtype.is_floating_point:
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


@pytest.fixture(scope="module")
def cases():
    return {name: ref.make_case(name) for name in ref.CASES}


def tables(c):
    """a case's tables on the device, every index the kernel would follow checked to be inside its array first"""
    A, Lg, T = c["x"].shape[1], len(c["lig_idx"]), len(c["rot"])
    assert 0 <= c["lig_idx"].min() and c["lig_idx"].max() < A and len(c["types"]) == A == len(c["rec_mask"])
    assert len(c["lig_active"]) == Lg and not c["rec_mask"][c["lig_idx"]].any()
    assert c["rot"].shape == (T, 2) and (T == 0 or (0 <= c["rot"].min() and c["rot"].max() < Lg)) and c["mask"].shape == (T, (Lg + 31) // 32)
    both = np.concatenate([c["intra"], c["intra"][:, ::-1]], 0).astype(np.int64)
    both = both[np.lexsort((both[:, 1], both[:, 0]))] if len(both) else both
    start = np.concatenate([[0], np.cumsum(np.bincount(both[:, 0], minlength=Lg))]).astype(np.int32)
    assert len(start) == Lg + 1 and start[-1] == len(both) and (len(both) == 0 or (0 <= both.min() and both.max() < Lg))
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()
    return dict(lig_idx=up(c["lig_idx"], np.int32), types=up(c["types"], np.uint8), rec_mask=up(c["rec_mask"], np.uint8),
                lig_active=up(c["lig_active"], np.uint8), rot=up(c["rot"], np.int32), mask=up(c["mask"].view(np.int32), np.int32),
                intra_start=up(start, np.int32), intra_atom=up(both[:, 1] if len(both) else np.zeros(0), np.int32), n_intra=len(c["intra"]))


def head(x, d, T):
    return [P(x), P(d["lig_idx"]), P(d["types"]), P(d["rec_mask"]), P(d["lig_active"]), P(d["rot"]) if T else None,
            P(d["mask"]) if T else None, P(d["intra_start"]), P(d["intra_atom"]) if d["n_intra"] else None, d["n_intra"]]


def launch_energy(L, x, c, d=None):
    d = d or tables(c)
    x = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    n, A, Lg, T = x.shape[0], x.shape[1], len(c["lig_idx"]), len(c["rot"])
    buf = dict(energy=sentinel(n), inter=sentinel(n), intra=sentinel(n), grad=sentinel(n, Lg, 3), ggrad=sentinel(n, 6 + T))
    rc = L.pd_vina_refine_energy(*head(x, d, T), P(buf["energy"]), P(buf["inter"]), P(buf["intra"]), P(buf["grad"]), P(buf["ggrad"]),
                                 n, A, Lg, T, S())
    assert rc == 0, rc
    return {k: body(v) for k, v in buf.items()}


def launch_refine(L, x, c, d=None, max_iters=20, grad_tol=1e-4, max_step=1.0, trace=True):
    d = d or tables(c)
    x = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    n, A, Lg, T = x.shape[0], x.shape[1], len(c["lig_idx"]), len(c["rot"])
    numel = L.pd_vina_refine_workspace_numel(n, Lg, T)
    assert numel == n * ((6 + T) ** 2 + 3 * Lg)
    ws = sentinel(numel)
    i32 = torch.int32
    buf = dict(x_refined=sentinel(n, A, 3, dtype=torch.float32), energy_start=sentinel(n), energy=sentinel(n), iterations=sentinel(n, dtype=i32),
               evaluations=sentinel(n, dtype=i32), status=sentinel(n, dtype=i32), moved=sentinel(n))
    if trace:
        buf["energy_trace"] = sentinel(n, max_iters + 1)
    rc = L.pd_vina_refine(*head(x, d, T), max_iters, grad_tol, max_step, P(ws), numel, P(buf["x_refined"]), P(buf["energy_start"]),
                          P(buf["energy"]), P(buf["iterations"]), P(buf["evaluations"]), P(buf["status"]), P(buf["moved"]),
                          P(buf["energy_trace"]) if trace else None, n, A, Lg, T, S())
    assert rc == 0, rc
    out = {k: body(v) for k, v in buf.items()}
    assert untouched(ws[-1:]), "the element behind the workspace was written"
    assert not (out["iterations"] == I_SENTINEL).any() and not (out["status"] == I_SENTINEL).any()
    return out


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------ the energy kernel
def oracle(c):
    outs = [ref.evaluate(c, c["x"][p].astype(np.float64), c["x"][p].astype(np.float64)[c["lig_idx"]], bounds=True) for p in range(c["x"].shape[0])]
    keys = ("energy", "inter", "intra", "grad", "ggrad")
    return ({k: np.stack([np.asarray(o[k]) for o in outs]) for k in keys}, {k: np.stack([np.asarray(o["bound"][k]) for o in outs]) for k in keys},
            min(o["margin"] for o in outs))


def check(case, out, want, bound):
    for k in want:
        dev, r, b = out[k].cpu().numpy(), want[k], bound[k]
        assert dev.dtype == np.float64 and dev.shape == r.shape == b.shape, (case, k, dev.shape, r.shape)
        err = np.abs(dev - r)
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
        worst = np.unravel_index(np.argmax(ratio), ratio.shape) if ratio.ndim else ()
        print(f"ENVELOPE | pd_vina_refine_energy | {case} {k} | {np.abs(r).max():.2e} | {err.max():.2e} | {b[worst]:.2e} | {ratio.max():.2f} |")
        assert (err <= b).all(), (case, k, "err", err.max(), "bound", b[worst], "ratio", ratio.max())


@pytest.mark.parametrize("name", list(ref.CASES))
def test_energy_kernel_against_float64(L, cases, name):
    c = cases[name]
    want, bound, margin = oracle(c)
    assert margin >= ref.MARGIN
    d = tables(c)
    out = launch_energy(L, c["x"], c, d)
    check(name, out, want, bound)
    assert same(launch_energy(L, c["x"], c, d), out)                                   # launch to launch
    for p in range(c["x"].shape[0]):                                                   # alone and inside the batch
        one = launch_energy(L, c["x"][p:p + 1], c, d)
        assert all(torch.equal(one[k][0], out[k][p]) for k in out), (name, p)
    assert not out["grad"][:, torch.from_numpy(c["lig_active"] == 0).cuda()].any()
    assert torch.equal(out["energy"], out["inter"] + out["intra"])
    if name.endswith("far"):
        assert not any(v.any() for v in out.values())                                  # exact zeros
    # every output may be NULL
    x = torch.from_numpy(c["x"]).cuda()
    n, T = c["x"].shape[0], len(c["rot"])
    e = sentinel(n)
    assert L.pd_vina_refine_energy(*head(x, d, T), P(e), None, None, None, None, n, x.shape[1], len(c["lig_idx"]), T, S()) == 0
    assert torch.equal(body(e), out["energy"])


@pytest.mark.parametrize("name", list(ref.CASES))
def test_inter_against_pd_vina_score(L, cases, name):
    c = cases[name]
    d = tables(c)
    out = launch_energy(L, c["x"], c, d)
    x = torch.from_numpy(c["x"]).cuda()
    n, A, Lg = x.shape[0], x.shape[1], len(c["lig_idx"])
    new = lambda *s: torch.empty(*s, device="cuda")
    inter = new(n)
    assert L.pd_vina_score(P(x), P(d["lig_idx"]), P(d["types"]), P(d["rec_mask"]), P(d["lig_active"]), 0.0, P(new(n, Lg, 5)), P(new(n, 5)),
                           P(inter), P(new(n)), P(new(n, Lg)), None, n, A, Lg, S()) == 0
    b32 = vina_ref.vina(c["x"], c["lig_idx"], c["types"], c["rec_mask"], c["lig_active"], 0.0)["bound"]["inter"]
    err = np.abs(out["inter"].cpu().numpy() - inter.cpu().double().numpy())
    print(f"ENVELOPE | inter vs pd_vina_score | {name} | {err.max():.2e} | {b32.max():.2e} |")
    assert (err <= b32 + oracle(c)[1]["inter"]).all(), (name, err, b32)


# ------------------------------------------------------------------ the refinement
@pytest.fixture(scope="module")
def reference_runs(cases):
    return {(name, mi): [ref.refine(c, c["x"][p].astype(np.float64), max_iters=mi) for p in range(c["x"].shape[0])]
            for name, c in cases.items() for mi in (3, 20)}


@pytest.fixture(scope="module")
def device_runs(L, cases):
    return {(name, mi): launch_refine(L, c["x"], c, max_iters=mi) for name, c in cases.items() for mi in (3, 20)}


@pytest.mark.parametrize("mi", [3, 20])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_refinement_takes_the_reference_trajectory(cases, reference_runs, device_runs, name, mi):
    c, want, out = cases[name], reference_runs[name, mi], device_runs[name, mi]
    for k in ("iterations", "evaluations", "status"):
        assert out[k].cpu().tolist() == [w[k] for w in want], (name, mi, k, out[k].cpu().tolist(), [w[k] for w in want])
    lig = torch.from_numpy(c["lig_idx"].astype(np.int64)).cuda()
    y = out["x_refined"][:, lig].cpu().double().numpy()
    yr = np.stack([w["y"] for w in want])
    ulp = float(np.spacing(np.float32(np.abs(yr).max())))
    diff = np.abs(y - yr).max()
    print(f"TRAJECTORY | {name} max_iters {mi} | largest coordinate difference {diff:.3e} | fp32 ulp {ulp:.3e} | moved {max(w['moved'] for w in want):.3f} |")
    assert diff <= 1e-6 + ulp, (name, mi, diff)
    assert np.abs(out["moved"].cpu().numpy() - [w["moved"] for w in want]).max() <= np.sqrt(3.0) * 1e-6     # an RMSD of such differences


@pytest.mark.parametrize("mi", [3, 20])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_refined_energy_within_the_energy_bound(cases, reference_runs, device_runs, name, mi):
    c, want, out = cases[name], reference_runs[name, mi], device_runs[name, mi]
    for p, w in enumerate(want):
        b = ref.evaluate(c, c["x"][p].astype(np.float64), w["y"], bounds=True)["bound"]["energy"]
        err = abs(float(out["energy"][p]) - w["energy"])
        print(f"ENVELOPE | pd_vina_refine energy | {name} max_iters {mi} pose {p} | {abs(w['energy']):.2e} | {err:.2e} | {b:.2e} | {err / b if b else 0:.2f} |")
        assert err <= b, (name, mi, p, err, b)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_rigidity(cases, device_runs, name):
    c, out = cases[name], device_runs[name, 20]
    x = torch.from_numpy(c["x"]).cuda()
    lig = c["lig_idx"].astype(np.int64)
    rest = torch.from_numpy(np.setdiff1d(np.arange(x.shape[1]), lig)).cuda()
    assert torch.equal(out["x_refined"][:, rest], x[:, rest]), "a receptor row changed"
    Lg = len(lig)
    adj = np.zeros((Lg, Lg), dtype=bool)
    for i, j in c["bonds"]:
        adj[i, j] = adj[j, i] = True
    frag = np.zeros(Lg, dtype=np.int64)
    for k, m in enumerate(c["sets"]):
        frag[m] |= 1 << k
    rigid = adj | ((adj.astype(int) @ adj.astype(int)) > 0) | (frag[:, None] == frag[None, :])          # bonded, 1-3, same fragment
    y0, y1 = c["x"][:, lig].astype(np.float64), out["x_refined"][:, torch.from_numpy(lig).cuda()].cpu().double().numpy()
    d0 = np.sqrt(((y0[:, :, None] - y0[:, None]) ** 2).sum(-1))
    d1 = np.sqrt(((y1[:, :, None] - y1[:, None]) ** 2).sum(-1))
    tol = 4.0 * float(np.spacing(np.float32(max(np.abs(y0).max(), np.abs(y1).max()))))
    assert np.abs(d1 - d0)[:, rigid].max() <= tol, (name, np.abs(d1 - d0)[:, rigid].max(), tol)
    if not name.endswith("far"):
        assert float(out["moved"].max()) > 0.05


def test_descent(cases, device_runs):
    for (name, mi), out in device_runs.items():
        tr = out["energy_trace"]
        assert (tr[:, 1:] <= tr[:, :-1]).all() and torch.equal(tr[:, 0], out["energy_start"]) and torch.equal(tr[:, -1], out["energy"])
        assert (out["energy"] <= out["energy_start"]).all(), (name, mi)
    clash = device_runs["P3_A300_L12_T3", 20]
    assert float(clash["energy"][0]) < float(clash["energy_start"][0]) and int(clash["iterations"][0]) > 0
    c = cases["P2_A300_L12_far"]
    for mi in (3, 20):
        far = device_runs["P2_A300_L12_far", mi]
        assert torch.equal(far["x_refined"], torch.from_numpy(c["x"]).cuda())
        assert far["iterations"].tolist() == [0, 0] and far["status"].tolist() == [0, 0] and far["evaluations"].tolist() == [1, 1]
        assert not far["moved"].any() and not far["energy"].any()


@pytest.mark.parametrize("name", ["P3_A300_L12_T3", "P2_A257_L6_T2"])
def test_independence(L, cases, device_runs, name):
    c, out = cases[name], device_runs[name, 20]
    d = tables(c)
    assert same(launch_refine(L, c["x"], c, d), out)                                   # two launches
    rev = launch_refine(L, c["x"][::-1], c, d)
    assert all(torch.equal(rev[k].flip(0), out[k]) for k in out), name
    for p in range(c["x"].shape[0]):
        one = launch_refine(L, c["x"][p:p + 1], c, d)
        assert all(torch.equal(one[k][0], out[k][p]) for k in out), (name, p)
    bare = launch_refine(L, c["x"], c, d, trace=False)                                  # the trace is optional
    assert "energy_trace" not in bare and all(torch.equal(bare[k], out[k]) for k in bare)


def test_error_codes(L, cases):
    c = cases["P2_A257_L6_T2"]
    d = tables(c)
    x = torch.from_numpy(c["x"]).cuda()
    n, A, Lg, T = 2, 257, 6, 2
    numel = L.pd_vina_refine_workspace_numel(n, Lg, T)
    i32 = torch.int32
    ws = sentinel(numel)
    bufs = [sentinel(n, A, 3, dtype=torch.float32), sentinel(n), sentinel(n), sentinel(n, dtype=i32), sentinel(n, dtype=i32), sentinel(n, dtype=i32),
            sentinel(n), sentinel(n, 4)]
    h = head(x, d, T)

    def call(h=h, mi=3, gt=1e-4, ms=1.0, ws_=P(ws), wn=numel, outs=None, sizes=(n, A, Lg, T)):
        outs = [P(b) for b in bufs] if outs is None else outs
        return L.pd_vina_refine(*h, mi, gt, ms, ws_, wn, *outs, *sizes, S())

    rcs = {}
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 8):                                              # x .. intra_atom
        hh = list(h)
        hh[k] = None
        rcs[f"null table {k}"] = call(h=hh)
    for k in (0, 1, 5, 6, 7, 8):                                                        # float / int tables off their alignment
        hh = list(h)
        hh[k] = h[k] + 2
        rcs[f"misaligned table {k}"] = call(h=hh)
    for k in range(7):                                                                  # the required outputs
        outs = [P(b) for b in bufs]
        outs[k] = None
        rcs[f"null output {k}"] = call(outs=outs)
    for k in range(8):
        outs = [P(b) for b in bufs]
        outs[k] = outs[k] + (2 if bufs[k].dtype != torch.float64 else 4)
        rcs[f"misaligned output {k}"] = call(outs=outs)
    rcs["null ws"] = call(ws_=None)
    rcs["misaligned ws"] = call(ws_=P(ws) + 4)
    rcs["short ws"] = call(wn=numel - 1)
    rcs["max_iters<0"] = call(mi=-1)
    rcs["grad_tol<0"] = call(gt=-1e-4)
    rcs["grad_tol nan"] = call(gt=NAN)
    rcs["max_step 0"] = call(ms=0.0)
    rcs["max_step<0"] = call(ms=-1.0)
    for k in range(3):
        sz = [n, A, Lg, T]
        sz[k] = 0
        rcs[f"size {k} = 0"] = call(sizes=sz)
    rcs["T<0"] = call(sizes=(n, A, Lg, -1))
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), rcs
    unsupported = {"L": call(sizes=(n, A, 1025, T)), "T": call(sizes=(n, A, Lg, 59)), "P": call(sizes=(65536, A, Lg, T)),
                   "A": call(sizes=(n, (1 << 22) + 1, Lg, T))}
    assert all(rc == PD_ERR_UNSUPPORTED for rc in unsupported.values()), unsupported
    # the energy entry point: the same table checks
    e = sentinel(n)
    ecall = lambda h=h, e_=P(e), sizes=(n, A, Lg, T): L.pd_vina_refine_energy(*h, e_, None, None, None, None, *sizes, S())
    hh = list(h)
    hh[7] = None
    assert ecall(h=hh) == PD_ERR_ARG and ecall(e_=P(e) + 4) == PD_ERR_ARG and ecall(sizes=(0, A, Lg, T)) == PD_ERR_ARG
    assert ecall(sizes=(n, A, Lg, 59)) == PD_ERR_UNSUPPORTED and ecall(sizes=(n, A, 1025, T)) == PD_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(untouched(b) for b in bufs) and untouched(ws) and untouched(e), "a rejected call wrote"
    assert call() == 0
    for b in bufs:
        body(b)


# ------------------------------------------------------------------ VinaRefine
def vina_refine_of(c):
    from physdock_amd import VinaRefine
    from physdock_amd.scoring import VinaScore
    v = VinaScore.from_types(c["types"], c["lig_idx"], c["rec_mask"], c["n_rot"], ligand_active=c["lig_active"], device="cuda")
    return VinaRefine.from_vina(v, c["bonds"], device="cuda")


def test_python_surface(L, cases, device_runs):
    c = cases["P3_A300_L12_T3"]
    r = vina_refine_of(c)
    x = torch.from_numpy(c["x"]).cuda()
    out = r.refine(x, max_iters=20, trace=True)
    assert set(out) == {"x_refined", "energy_start", "energy", "iterations", "evaluations", "status", "moved", "energy_trace", "score_start", "score"}
    assert all(t.is_cuda for t in out.values())
    f64, f32, i32 = torch.float64, torch.float32, torch.int32
    dtypes = dict(x_refined=f32, energy_start=f64, energy=f64, iterations=i32, evaluations=i32, status=i32, moved=f64, energy_trace=f64,
                  score_start=f32, score=f32)
    assert {k: t.dtype for k, t in out.items()} == dtypes
    assert out["x_refined"].shape == (3, 300, 3) and out["energy_trace"].shape == (3, 21) and all(out[k].shape == (3,) for k in dtypes if k not in ("x_refined", "energy_trace"))
    raw = device_runs["P3_A300_L12_T3", 20]
    assert all(torch.equal(out[k], raw[k]) for k in raw)
    assert torch.equal(out["score"], r.vina.score(out["x_refined"])["score"]) and torch.equal(out["score_start"], r.vina.score(x)["score"])
    assert "energy_trace" not in r.refine(x, max_iters=3)
    e = r.energy(x, gradients=True)
    assert set(e) == {"energy", "inter", "intra", "grad", "ggrad"} and all(t.is_cuda and t.dtype == f64 for t in e.values())
    assert e["grad"].shape == (3, 12, 3) and e["ggrad"].shape == (3, 9) and e["energy"].shape == (3,)
    assert same(e, launch_energy(L, c["x"], c))
    assert set(r.energy(x)) == {"energy", "inter", "intra"} and torch.equal(r.energy(x)["energy"], e["energy"])
    with pytest.raises(ValueError, match="pose atoms"):
        r.refine(x[:, :-1])
    one = vina_refine_of(cases["P2_A65_L1_T0"])                                         # T = 0 and no intramolecular pair
    o1 = one.refine(torch.from_numpy(cases["P2_A65_L1_T0"]["x"]).cuda(), max_iters=20)
    assert torch.equal(o1["x_refined"], device_runs["P2_A65_L1_T0", 20]["x_refined"])


@pytest.fixture(scope="module")
def small(small_model_inputs):
    from physdock_amd import PhysDock
    cfg, P_, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P_, strict=True)
    return model.cuda().eval(), {k: v.cuda() for k, v in batch.items()}, cfg


def same_result(u, w):
    if isinstance(u, torch.Tensor):
        return isinstance(w, torch.Tensor) and torch.equal(u, w)
    if isinstance(u, dict):
        return isinstance(w, dict) and set(u) == set(w) and all(same_result(u[k], w[k]) for k in u)
    return u == w


def test_redock_reports_the_refinement_and_changes_nothing_else(small):
    from physdock_amd import VinaRefine, driver
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.ranking import rank_by_score
    from physdock_amd.validity import PoseValidity
    model, dbatch, _ = small
    bonds = [(i, i + 1) for i in range(int(ligand_atom_mask(dbatch).sum()) - 1)]
    refine = VinaRefine.from_batch(dbatch, bonds)
    validity = PoseValidity.from_batch(dbatch, bonds)
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, dbatch, **kw)
    assert set(plain) == {"poses", "accepted", "rounds", "gamma_factor", "ranking"}      # the keys of the parent commit
    out = driver.redock(model, dbatch, refine=refine, **kw)
    assert set(out) == set(plain) | {"refined"} and same_result({k: out[k] for k in plain}, plain)
    assert same_result(out["refined"], refine.refine(out["poses"]))
    assert out["refined"]["x_refined"].shape == out["poses"].shape and (out["refined"]["energy"] <= out["refined"]["energy_start"]).all()
    full = driver.redock(model, dbatch, refine=refine, vina=refine.vina, validity=validity, **kw)
    assert set(full) == set(plain) | {"refined", "order_vina_refined", "vina", "order_vina", "validity", "order_vina_valid"}
    assert same_result(full["refined"]["validity"], validity.check(full["refined"]["x_refined"]))
    assert torch.equal(full["order_vina_refined"], rank_by_score({"score": full["refined"]["score"]}))
    assert torch.equal(full["refined"]["score_start"], full["vina"]["score"]) and torch.equal(full["poses"], plain["poses"])
    assert same_result({k: v for k, v in full["refined"].items() if k != "validity"}, out["refined"])
    many = driver.redock_many(model, [(dbatch, {"refine": refine})], **kw)
    assert same_result(many[0], out)
    grouped = driver.redock_many(model, [(dbatch, {"refine": refine, "vina": refine.vina})], group=1, **kw)
    assert same_result(grouped[0]["refined"], refine.refine(grouped[0]["poses"])) and "order_vina_refined" in grouped[0]
