"""pd_vina_search, pd_vina_search_select and pd_vina_search_workspace_numel (csrc/vina_refine.hip) straight on the C ABI,
VinaRefine.search, and the search keyword of redock / redock_many.

The yardstick is the float64 definition tests/vina_search_ref.py on the (case, seed, settings) tuples `GPU_CASES`, whose conditioning
tests/test_vina_search_cpu.py guards on the CPU: the device must take every decision of the reference - entity, accept, iterations
and status of every descent, best_step, accepted, evaluations, best_chain - and end within the project's figure for ONE refinement,
1e-6 A plus one fp32 ulp of the largest coordinate; the figure is not widened for the chain.  One `TRAJECTORY | pd_vina_search | ...`
line per case is printed under pytest -s.  Output buffers are one row longer than needed and pre-filled with a sentinel, and the
element behind the workspace is checked, with the helpers of tests/test_vina_refine_gpu.py.

The proposal alone (steps = 1, max_iters = 0, temperature = inf).  x_chains holds each chain's BEST conformation, so it shows the
proposal move(y_start, s) where the proposal lowers the energy - there it must agree with the reference's to one fp32 ulp at each
coordinate's magnitude, the rounding of the output - and the start, bit for bit, where it does not; the CPU guard sees to it that
the first happens, and takes the decision E_new < E_start out of roundoff's reach."""
import numpy as np
import pytest
import torch

import test_vina_refine_gpu as rg
import vina_refine_ref as ref
import vina_search_ref as sr

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN, INF = float("nan"), float("inf")
sentinel, body, untouched, P, S = rg.sentinel, rg.body, rg.untouched, rg.P, rg.S
OUTS = ("x_chains", "energy_chains", "energy_start", "best_step", "accepted", "evaluations")
TRACES = ("trace_energy", "trace_entity", "trace_accept", "trace_iterations", "trace_status")
SELECTED = ("best_chain", "energy", "x_search")
PROPOSAL = dict(steps=1, max_iters=0, temperature=INF)


@pytest.fixture(scope="module")
def L():
    from physdock_amd import ops
    return ops._lib.init()


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in sr.GPU_CASES:
        c = ref.make_case(name)
        out[name] = (c, rg.tables(c))
    return out


def settings(name, **over):
    seed, st = sr.GPU_CASES[name]
    return dict(dict(st, seed=seed, grad_tol=1e-4, max_step=1.0), **over)


def launch_search(L, c, d, x=None, splits=None, pose0=0, trace=True, *, chains, steps, seed, temperature, translate_amp, rotate_amp, max_iters,
                  grad_tol, max_step):
    """the search of the poses x (default: the case's) in launches of `splits` steps (default: one launch), then the selection"""
    x = torch.from_numpy(np.array(c["x"] if x is None else x, dtype=np.float32)).cuda()
    n, A, Lg, T, K = x.shape[0], x.shape[1], len(c["lig_idx"]), len(c["rot"]), chains
    numel = L.pd_vina_search_workspace_numel(n, K, Lg, T)
    assert numel == n * K * ((6 + T) ** 2 + 9 * Lg + 8)
    ws = sentinel(numel)
    i32, f32 = torch.int32, torch.float32
    buf = dict(x_chains=sentinel(n, K, Lg, 3, dtype=f32), energy_chains=sentinel(n, K), energy_start=sentinel(n, K), best_step=sentinel(n, K, dtype=i32),
               accepted=sentinel(n, K, dtype=i32), evaluations=sentinel(n, K, dtype=i32))
    if trace:
        buf.update(trace_energy=sentinel(n, K, steps + 1), **{k: sentinel(n, K, steps, dtype=i32) for k in TRACES[1:]})
    splits = [steps] if splits is None else list(splits)
    assert sum(splits) == steps
    step0 = 0
    for ns in splits:
        rc = L.pd_vina_search(*rg.head(x, d, T), max_iters, grad_tol, max_step, seed, pose0, step0, ns, steps, temperature, translate_amp, rotate_amp,
                              P(ws), numel, *[P(buf[k]) for k in OUTS], *[P(buf[k]) if trace else None for k in TRACES], n, K, A, Lg, T, S())
        assert rc == 0, rc
        step0 += ns
    out = {k: body(v) for k, v in buf.items()}
    assert untouched(ws[-1:]), "the element behind the workspace was written"
    for k in ("best_step", "accepted", "evaluations") + (TRACES[1:] if trace else ()):
        assert not (out[k] == rg.I_SENTINEL).any(), k
    sel = dict(best_chain=sentinel(n, dtype=i32), energy=sentinel(n), x_search=sentinel(n, A, 3, dtype=f32))
    rc = L.pd_vina_search_select(P(x), P(d["lig_idx"]), P(out["x_chains"]), P(out["energy_chains"]), P(sel["best_chain"]), P(sel["energy"]),
                                 P(sel["x_search"]), n, K, A, Lg, S())
    assert rc == 0, rc
    out.update({k: body(v) for k, v in sel.items()})
    assert not (out["best_chain"] == rg.I_SENTINEL).any()
    return out


def same(a, b, keys=None):
    return all(torch.equal(a[k], b[k]) for k in (keys or a))


@pytest.fixture(scope="module")
def reference_runs(cases):
    """(case, kind) -> the reference search, computed once"""
    out = {}
    for name, (seed, st) in sr.GPU_CASES.items():
        out[name, "trajectory"] = sr.search(cases[name][0], seed=seed, **st)
        out[name, "proposal"] = sr.search(cases[name][0], seed=seed, **dict(st, **PROPOSAL))
    return out


@pytest.fixture(scope="module")
def device_runs(L, cases):
    return {name: launch_search(L, c, d, **settings(name)) for name, (c, d) in cases.items()}


def per_chain(run, key):
    return [[r[key] for r in row] for row in run["chains"]]


# ------------------------------------------------------------------ 1. steps = 0 is pd_vina_refine
@pytest.mark.parametrize("name", list(sr.GPU_CASES))
def test_zero_steps_is_refine_bit_for_bit(L, cases, name):
    c, d = cases[name]
    st = settings(name, steps=0)
    out = launch_search(L, c, d, **st)
    want = rg.launch_refine(L, c["x"], c, d, max_iters=st["max_iters"], trace=False)
    lig = torch.from_numpy(c["lig_idx"].astype(np.int64)).cuda()
    for k in range(st["chains"]):
        assert torch.equal(out["x_chains"][:, k], want["x_refined"][:, lig]), (name, k)
        assert torch.equal(out["energy_chains"][:, k], want["energy"]) and torch.equal(out["energy_start"][:, k], want["energy"])
        assert torch.equal(out["evaluations"][:, k], want["evaluations"])
    assert torch.equal(out["trace_energy"][:, :, 0], out["energy_start"]) and out["trace_entity"].numel() == 0
    assert not out["best_step"].any() and not out["accepted"].any() and not out["best_chain"].any()
    assert torch.equal(out["x_search"], want["x_refined"]) and torch.equal(out["energy"], want["energy"])


# ------------------------------------------------------------------ 2. the proposal alone
@pytest.mark.parametrize("name", list(sr.GPU_CASES))
def test_the_proposal_alone(L, cases, reference_runs, name):
    c, d = cases[name]
    want = reference_runs[name, "proposal"]
    out = launch_search(L, c, d, **settings(name, **PROPOSAL))
    assert out["trace_entity"][:, :, 0].cpu().tolist() == [[e[0] for e in row] for row in per_chain(want, "entity")]
    assert out["best_step"].cpu().tolist() == per_chain(want, "best_step")
    assert out["accepted"].cpu().tolist() == [[1] * len(row) for row in want["chains"]]            # temperature = inf
    assert out["evaluations"].cpu().tolist() == [[2] * len(row) for row in want["chains"]]         # max_iters = 0: one evaluation per descent
    got = out["x_chains"].cpu().numpy()
    start = c["x"][:, c["lig_idx"]]
    shown = 0
    for p, row in enumerate(want["chains"]):
        for k, r in enumerate(row):
            if r["best_step"] == 1:
                y = r["proposals"][0]
                ulp = np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)
                assert (np.abs(got[p, k].astype(np.float64) - y) <= ulp).all(), (name, p, k, np.abs(got[p, k] - y).max())
                shown += 1
            else:
                assert np.array_equal(got[p, k], start[p]), (name, p, k)
    assert shown >= 1, name


# ------------------------------------------------------------------ 3. the trajectory
@pytest.mark.parametrize("name", list(sr.GPU_CASES))
def test_search_takes_the_reference_trajectory(cases, reference_runs, device_runs, name):
    """Measured on an MI355X (TRAJECTORY lines, also in NOTES.md): see NOTES.md "VinaSearch"."""
    c, _ = cases[name]
    want, out = reference_runs[name, "trajectory"], device_runs[name]
    for dev, key in (("trace_entity", "entity"), ("trace_accept", "accept"), ("trace_iterations", "iterations"), ("trace_status", "status"),
                     ("best_step", "best_step"), ("accepted", "accepted"), ("evaluations", "evaluations")):
        assert out[dev].cpu().tolist() == per_chain(want, key), (name, dev, out[dev].cpu().tolist(), per_chain(want, key))
    assert out["best_chain"].cpu().tolist() == want["best_chain"], name
    yr = np.asarray(per_chain(want, "y_best"))
    y = out["x_chains"].cpu().double().numpy()
    ulp = float(np.spacing(np.float32(np.abs(yr).max())))
    diff = float(np.abs(y - yr).max())
    ediff = float(np.abs(out["trace_energy"].cpu().numpy() - np.asarray(per_chain(want, "trace_energy"))).max())
    print(f"TRAJECTORY | pd_vina_search | {name} | {diff:.3e} | {ediff:.3e} |")
    assert diff <= 1e-6 + ulp, (name, diff)
    lig = torch.from_numpy(c["lig_idx"].astype(np.int64)).cuda()
    assert np.abs(out["x_search"][:, lig].cpu().double().numpy() - want["y"]).max() <= 1e-6 + ulp


# ------------------------------------------------------------------ 4. resumable
@pytest.mark.parametrize("name", list(sr.GPU_CASES))
def test_a_search_cut_into_launches_is_the_same_search(L, cases, device_runs, name):
    c, d = cases[name]
    st = settings(name)
    assert st["steps"] == 6
    cut = launch_search(L, c, d, splits=(1, 2, 3), **st)
    assert same(cut, device_runs[name]), [k for k in cut if not torch.equal(cut[k], device_runs[name][k])]
    assert same(launch_search(L, c, d, splits=(0, 6, 0), **st), cut)                    # an empty launch changes nothing


# ------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("name", ["P3_A300_L12_T3", "P2_A257_L6_T2"])
def test_independence(L, cases, device_runs, name):
    c, d = cases[name]
    st, out = settings(name), device_runs[name]
    assert same(launch_search(L, c, d, **st), out)                                      # launch to launch
    per = OUTS + TRACES
    for K in (1, 2):
        few = launch_search(L, c, d, **dict(st, chains=K))
        assert all(torch.equal(few[k], out[k][:, :K]) for k in per), (name, K)
    for q in range(c["x"].shape[0]):                                                    # alone under its pose id, and inside the batch
        one = launch_search(L, c, d, x=c["x"][q:q + 1], pose0=q, **st)
        assert all(torch.equal(one[k][0], out[k][q]) for k in per + SELECTED), (name, q)
    bare = launch_search(L, c, d, trace=False, **st)                                    # the traces are optional
    assert not set(bare) & set(TRACES) and same(bare, out, OUTS + SELECTED)
    other = launch_search(L, c, d, **dict(st, seed=st["seed"] + 1))
    assert not torch.equal(other["trace_entity"], out["trace_entity"])
    assert torch.equal(other["energy_start"], out["energy_start"])                      # the start does not draw


# ------------------------------------------------------------------ 6. the outputs among themselves
@pytest.mark.parametrize("name", list(sr.GPU_CASES))
def test_outputs_are_consistent(cases, reference_runs, device_runs, name):
    c, _ = cases[name]
    st, out, want = settings(name), device_runs[name], reference_runs[name, "trajectory"]
    tr = out["trace_energy"].cpu().numpy()
    assert np.isfinite(tr).all()
    assert np.array_equal(out["energy_chains"].cpu().numpy(), np.where(np.isfinite(tr), tr, np.inf).min(-1))
    assert np.array_equal(out["energy_start"].cpu().numpy(), tr[:, :, 0])
    acc = out["trace_accept"].cpu().numpy()
    u4 = np.asarray(per_chain(want, "u4"))
    for p in range(tr.shape[0]):
        for k in range(tr.shape[1]):
            cur, best, best_step = tr[p, k, 0], tr[p, k, 0], 0
            for m in range(1, st["steps"] + 1):
                e = tr[p, k, m]
                prob = float(np.exp((cur - e) / st["temperature"]))
                assert abs(u4[p, k, m - 1] - prob) >= sr.U_MARGIN, (name, p, k, m)          # no step is left out
                rule = bool(np.isfinite(e) and (e < cur or u4[p, k, m - 1] < prob))
                assert bool(acc[p, k, m - 1]) == rule, (name, p, k, m)
                cur = e if rule else cur
                if e < best:
                    best, best_step = e, m
            assert int(out["best_step"][p, k]) == best_step and int(out["accepted"][p, k]) == int(acc[p, k].sum())
    e = out["energy_chains"].cpu().numpy()
    assert np.array_equal(out["energy"].cpu().numpy(), e.min(-1)) and np.array_equal(out["best_chain"].cpu().numpy(), e.argmin(-1))
    assert (out["energy"][:, None] <= out["energy_start"]).all()
    x = torch.from_numpy(c["x"]).cuda()
    lig = c["lig_idx"].astype(np.int64)
    rest = torch.from_numpy(np.setdiff1d(np.arange(x.shape[1]), lig)).cuda()
    assert torch.equal(out["x_search"][:, rest], x[:, rest]), "a receptor row changed"
    pick = out["x_chains"][torch.arange(x.shape[0]).cuda(), out["best_chain"].long()]
    assert torch.equal(out["x_search"][:, torch.from_numpy(lig).cuda()], pick)


# ------------------------------------------------------------------ 7. refusals
def test_error_codes(L, cases):
    name = "P2_A257_L6_T2"
    c, d = cases[name]
    x = torch.from_numpy(c["x"]).cuda()
    n, K, A, Lg, T, steps = 2, 3, 257, 6, 2, 2
    numel = L.pd_vina_search_workspace_numel(n, K, Lg, T)
    i32, f32 = torch.int32, torch.float32
    ws = sentinel(numel)
    bufs = [sentinel(n, K, Lg, 3, dtype=f32), sentinel(n, K), sentinel(n, K), sentinel(n, K, dtype=i32), sentinel(n, K, dtype=i32), sentinel(n, K, dtype=i32),
            sentinel(n, K, steps + 1)] + [sentinel(n, K, steps, dtype=i32) for _ in range(4)]
    h = rg.head(x, d, T)
    base = dict(mi=3, gt=1e-4, ms=1.0, seed=5, pose0=0, step0=0, ns=steps, total=steps, temp=1.2, ta=2.0, ra=1.0)

    def call(h=h, ws_=P(ws), wn=numel, outs=None, sizes=(n, K, A, Lg, T), **over):
        a = dict(base, **over)
        outs = [P(b) for b in bufs] if outs is None else outs
        return L.pd_vina_search(*h, a["mi"], a["gt"], a["ms"], a["seed"], a["pose0"], a["step0"], a["ns"], a["total"], a["temp"], a["ta"], a["ra"],
                                ws_, wn, *outs, *sizes, S())

    rcs = {}
    for k in range(9):                                                                  # x .. intra_atom
        hh = list(h)
        hh[k] = None
        rcs[f"null table {k}"] = call(h=hh)
    for k in (0, 1, 5, 6, 7, 8):
        hh = list(h)
        hh[k] = h[k] + 2
        rcs[f"misaligned table {k}"] = call(h=hh)
    for k in range(6):                                                                  # the required outputs
        outs = [P(b) for b in bufs]
        outs[k] = None
        rcs[f"null output {k}"] = call(outs=outs)
    for k in range(len(bufs)):
        outs = [P(b) for b in bufs]
        outs[k] = outs[k] + (2 if bufs[k].dtype != torch.float64 else 4)
        rcs[f"misaligned output {k}"] = call(outs=outs)
    rcs["null ws"] = call(ws_=None)
    rcs["misaligned ws"] = call(ws_=P(ws) + 4)
    rcs["short ws"] = call(wn=numel - 1)
    for key, bad in (("mi", -1), ("gt", -1e-4), ("gt", NAN), ("ms", 0.0), ("ms", -1.0), ("ns", -1), ("step0", -1), ("pose0", -1), ("total", 1),
                     ("temp", 0.0), ("temp", -1.0), ("temp", NAN), ("ta", -1.0), ("ta", NAN), ("ra", -0.5), ("ra", NAN)):
        rcs[f"{key}={bad}"] = call(**{key: bad})
    rcs["step0 + n_steps > steps_total"] = call(step0=1, ns=2)
    for k in range(4):
        sz = [n, K, A, Lg, T]
        sz[k] = 0
        rcs[f"size {k} = 0"] = call(sizes=sz)
    rcs["T<0"] = call(sizes=(n, K, A, Lg, -1))
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), rcs
    unsupported = {"L": call(sizes=(n, K, A, 1025, T)), "T": call(sizes=(n, K, A, Lg, 59)), "A": call(sizes=(n, K, (1 << 22) + 1, Lg, T)),
                   "K": call(sizes=(n, 65, A, Lg, T)), "P K": call(sizes=(21846, 3, A, Lg, T)), "P": call(sizes=(65536, 1, A, Lg, T))}
    assert all(rc == PD_ERR_UNSUPPORTED for rc in unsupported.values()), unsupported
    # the selection
    sel = [sentinel(n, dtype=i32), sentinel(n), sentinel(n, A, 3, dtype=f32)]
    xc, ec = torch.zeros(n, K, Lg, 3, device="cuda"), torch.zeros(n, K, device="cuda", dtype=torch.float64)
    args = [P(x), P(d["lig_idx"]), P(xc), P(ec)] + [P(b) for b in sel]

    def select(args=args, sizes=(n, K, A, Lg)):
        return L.pd_vina_search_select(*args, *sizes, S())

    rcs = {}
    for k in range(7):
        for bad, what in ((None, "null"), (args[k] + (4 if k in (3, 5) else 2), "misaligned")):
            aa = list(args)
            aa[k] = bad
            rcs[f"select {what} {k}"] = select(args=aa)
    for k in range(4):
        sz = [n, K, A, Lg]
        sz[k] = 0
        rcs[f"select size {k} = 0"] = select(sizes=sz)
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), rcs
    unsupported = {"K": select(sizes=(n, 65, A, Lg)), "L": select(sizes=(n, K, A, 1025)), "A": select(sizes=(n, K, (1 << 22) + 1, Lg)),
                   "P": select(sizes=(65536, K, A, Lg))}
    assert all(rc == PD_ERR_UNSUPPORTED for rc in unsupported.values()), unsupported
    torch.cuda.synchronize()
    assert all(untouched(b) for b in bufs + sel) and untouched(ws), "a rejected call wrote"
    assert call() == 0 and select() == 0
    for b in bufs + sel:
        body(b)
    assert untouched(ws[-1:])


# ------------------------------------------------------------------ 8. VinaRefine.search and redock(search=)
def test_python_surface(L, cases, device_runs):
    name = "P3_A300_L12_T3"
    c, _ = cases[name]
    r = rg.vina_refine_of(c)
    x = torch.from_numpy(c["x"]).cuda()
    st = settings(name)
    out = r.search(x, trace=True, **st)
    f64, f32, i32 = torch.float64, torch.float32, torch.int32
    n, K, A, steps = 3, 3, 300, st["steps"]
    want = dict(x_search=(f32, (n, A, 3)), energy=(f64, (n,)), best_chain=(i32, (n,)), x_chains=(f32, (n, K, A, 3)), energy_chains=(f64, (n, K)),
                energy_start=(f64, (n, K)), best_step=(i32, (n, K)), accepted=(i32, (n, K)), evaluations=(i32, (n, K)), moved=(f64, (n,)),
                score_start=(f32, (n,)), score=(f32, (n,)), trace_energy=(f64, (n, K, steps + 1)), trace_entity=(i32, (n, K, steps)),
                trace_accept=(i32, (n, K, steps)), trace_iterations=(i32, (n, K, steps)), trace_status=(i32, (n, K, steps)))
    assert {k: (t.dtype, tuple(t.shape)) for k, t in out.items()} == want and all(t.is_cuda for t in out.values())
    raw = device_runs[name]
    assert all(torch.equal(out[k], raw[k]) for k in raw if k != "x_chains")
    lig = torch.from_numpy(c["lig_idx"].astype(np.int64)).cuda()
    rest = torch.from_numpy(np.setdiff1d(np.arange(A), c["lig_idx"])).cuda()
    assert torch.equal(out["x_chains"][:, :, lig], raw["x_chains"]) and torch.equal(out["x_chains"][:, :, rest], x[:, None, rest].expand(n, K, -1, 3))
    assert torch.equal(out["score"], r.vina.score(out["x_search"])["score"]) and torch.equal(out["score_start"], r.vina.score(x)["score"])
    moved = ((out["x_search"][:, lig].double() - x[:, lig].double()) ** 2).sum(-1).mean(-1).sqrt()
    assert torch.equal(out["moved"], moved) and float(moved.max()) > 0.05
    plain = r.search(x, **st)
    assert set(plain) == set(want) - set(TRACES) and same(plain, out, plain)
    assert same(r.search(x, steps_per_launch=4, **st), plain) and same(r.search(x, steps_per_launch=1, trace=True, **st), out)
    shifted = r.search(x[1:], pose0=1, **st)
    assert all(torch.equal(shifted[k], plain[k][1:]) for k in plain)
    auto = r.search(x, **dict(st, rotate_amp=None))                                     # the default amplitude, from the first pose
    assert same(auto, r.search(x, **dict(st, rotate_amp=r.default_rotate_amp(x, st["translate_amp"]))))
    assert abs(r.default_rotate_amp(x) - sr.default_rotate_amp(c, c["x"][0])) <= 1e-6     # fp32 poses on the device


def test_pose_chunking_changes_nothing(cases, device_runs, monkeypatch):
    from physdock_amd import refine as refine_module
    name = "P3_A300_L12_T3"
    c, _ = cases[name]
    r = rg.vina_refine_of(c)
    x = torch.from_numpy(c["x"]).cuda()
    st = settings(name)
    whole = r.search(x, trace=True, **st)
    monkeypatch.setattr(refine_module, "MAX_SEARCH_BLOCKS", 2 * st["chains"] + 1)        # two poses per launch: 2 + 1
    assert same(r.search(x, trace=True, **st), whole)
    monkeypatch.setattr(refine_module, "MAX_SEARCH_BLOCKS", st["chains"])                # one pose per launch
    assert same(r.search(x, trace=True, steps_per_launch=4, **st), whole)


@pytest.fixture(scope="module")
def small(small_model_inputs):
    from physdock_amd import PhysDock
    cfg, P_, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P_, strict=True)
    return model.cuda().eval(), {k: v.cuda() for k, v in batch.items()}, cfg


def test_redock_reports_the_search_and_changes_nothing_else(small):
    from physdock_amd import VinaRefine, driver
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.ranking import rank_by_score
    from physdock_amd.validity import PoseValidity
    model, dbatch, _ = small
    bonds = [(i, i + 1) for i in range(int(ligand_atom_mask(dbatch).sum()) - 1)]
    refine = VinaRefine.from_batch(dbatch, bonds)
    validity = PoseValidity.from_batch(dbatch, bonds)
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    spec = dict(chains=2, steps=2, max_iters=3, seed=11)
    base = driver.redock(model, dbatch, refine=refine, **kw)
    out = driver.redock(model, dbatch, refine=refine, search=spec, **kw)
    assert set(out) == set(base) | {"searched"} and rg.same_result({k: out[k] for k in base}, base)
    n, A = out["poses"].shape[0], out["poses"].shape[1]
    direct = refine.search(out["poses"], **spec)
    assert rg.same_result(out["searched"], direct)
    assert set(direct) == {"x_search", "energy", "best_chain", "x_chains", "energy_chains", "energy_start", "best_step", "accepted", "evaluations",
                           "moved", "score_start", "score"}
    assert direct["x_search"].shape == (n, A, 3) and direct["x_chains"].shape == (n, 2, A, 3) and direct["energy_chains"].shape == (n, 2)
    assert (direct["energy"][:, None] <= direct["energy_start"]).all()
    assert torch.equal(direct["energy_start"][:, 0], refine.refine(out["poses"], max_iters=3)["energy"])
    assert rg.same_result(refine.search(out["poses"], steps_per_launch=1, **spec), direct)
    full = driver.redock(model, dbatch, refine=refine, vina=refine.vina, validity=validity, search=spec, **kw)
    assert {"searched", "order_vina_searched", "refined", "order_vina_refined"} <= set(full)
    assert rg.same_result(full["searched"]["validity"], validity.check(full["searched"]["x_search"]))
    order = full["order_vina_searched"]
    assert torch.equal(order, rank_by_score({"score": full["searched"]["score"]})) and sorted(order.tolist()) == list(range(n))
    assert torch.equal(full["poses"], base["poses"])
    assert rg.same_result({k: v for k, v in full["searched"].items() if k != "validity"}, out["searched"])
    off = driver.redock(model, dbatch, refine=refine, search=None, **kw)
    assert rg.same_result(off, base)
    many = driver.redock_many(model, [(dbatch, {"refine": refine, "search": spec})], **kw)
    assert rg.same_result(many[0], out)
    grouped = driver.redock_many(model, [(dbatch, {"refine": refine, "search": True})], group=1, **kw)
    assert rg.same_result(grouped[0]["searched"], refine.search(grouped[0]["poses"]))
    assert grouped[0]["searched"]["energy_chains"].shape == (n, 8)
    with pytest.raises(ValueError, match="refine="):
        driver.redock(model, dbatch, search=True, **kw)
