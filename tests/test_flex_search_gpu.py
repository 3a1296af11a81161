"""pd_vina_flex_search, pd_vina_flex_search_select and pd_vina_flex_search_workspace_numel (csrc/vina_flex.hip) straight on the C ABI,
FlexRefine.search, and the flex_search keyword of redock / redock_many.

The yardstick is the float64 definition tests/flex_search_ref.py on the (case, seed, settings) tuples `GPU_CASES`, whose conditioning
tests/test_flex_search_cpu.py guards on the CPU: the device must take every decision of the reference - entity, accept, iterations and
status of every descent, best_step, accepted, evaluations, best_chain - and end within the project's figure for ONE refinement, 1e-6 A
plus one fp32 ulp of the largest coordinate; the figure is not widened for the chain.  One `TRAJECTORY | pd_vina_flex_search | ...`
line per case is printed under pytest -s.  Output buffers are one row longer than needed and pre-filled with a sentinel, and the
element behind the workspace is checked, with the helpers of tests/test_flex_refine_gpu.py.

The proposal alone (steps = 1, max_iters = 0, temperature = inf): x_chains holds each chain's BEST conformation, so it shows the
proposal move(y_start, s) where the proposal lowers the energy - there it must agree with the reference's to one fp32 ulp at each
coordinate's magnitude - and the start, bit for bit, where it does not (tests/test_vina_search_gpu.py); the CPU guard sees to it that
a side-chain proposal is among those shown."""
import numpy as np
import pytest
import torch

import flex_refine_ref as ref
import flex_search_ref as fs
import test_flex_refine_gpu as fg
import vina_refine_ref as vrr

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN, INF = float("nan"), float("inf")
sentinel, body, untouched, P, S = fg.sentinel, fg.body, fg.untouched, fg.P, fg.S
OUTS = ("x_chains", "energy_chains", "energy_start", "best_step", "accepted", "evaluations")
TRACES = ("trace_energy", "trace_entity", "trace_accept", "trace_iterations", "trace_status")
SELECTED = ("best_chain", "energy", "inter", "intra", "receptor", "x_search", "moved", "moved_flex")
PROPOSAL = dict(steps=1, max_iters=0, temperature=INF)


@pytest.fixture(scope="module")
def L():
    from physdock_amd import ops
    return ops._lib.init()


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in fs.GPU_CASES:
        c = ref.make_case(name)
        out[name] = (c, fg.tables(c))
    return out


def settings(name, **over):
    seed, st = fs.GPU_CASES[name]
    return dict(dict(st, seed=seed, grad_tol=1e-4, max_step=1.0), **over)


def launch_search(L, c, d, x=None, splits=None, pose0=0, trace=True, finite=True, *, chains, steps, seed, temperature, translate_amp, rotate_amp,
                  chi_amp, max_iters, grad_tol, max_step):
    """the search of the poses x (default: the case's) in launches of `splits` steps (default: one launch), then the selection"""
    x = torch.from_numpy(np.array(c["x"] if x is None else x, dtype=np.float32)).cuda()
    n, A, M, N, K = x.shape[0], x.shape[1], c["L"] + c["F"], c["T"] + c["S"], chains
    numel = L.pd_vina_flex_search_workspace_numel(n, K, M, N)
    assert numel == n * K * ((6 + N) ** 2 + 9 * M + 8)
    ws = sentinel(numel)
    i32, f32 = torch.int32, torch.float32
    buf = dict(x_chains=sentinel(n, K, M, 3, dtype=f32), energy_chains=sentinel(n, K), energy_start=sentinel(n, K), best_step=sentinel(n, K, dtype=i32),
               accepted=sentinel(n, K, dtype=i32), evaluations=sentinel(n, K, dtype=i32))
    if trace:
        buf.update(trace_energy=sentinel(n, K, steps + 1), **{k: sentinel(n, K, steps, dtype=i32) for k in TRACES[1:]})
    splits = [steps] if splits is None else list(splits)
    assert sum(splits) == steps
    sz = (n, K) + fg.sizes(c, n)[1:]
    step0 = 0
    for ns in splits:
        rc = L.pd_vina_flex_search(*fg.head(x, d), max_iters, grad_tol, max_step, seed, pose0, step0, ns, steps, temperature, translate_amp,
                                   rotate_amp, chi_amp, P(ws), numel, *[P(buf[k]) for k in OUTS], *[P(buf[k]) if trace else None for k in TRACES],
                                   *sz, S())
        assert rc == 0, rc
        step0 += ns
    out = {k: body(v, finite) for k, v in buf.items()}
    assert untouched(ws[-1:]), "the element behind the workspace was written"
    for k in ("best_step", "accepted", "evaluations") + (TRACES[1:] if trace else ()):
        assert not (out[k] == fg.I_SENTINEL).any(), k
    sel = dict(best_chain=sentinel(n, dtype=i32), energy=sentinel(n), inter=sentinel(n), intra=sentinel(n), receptor=sentinel(n),
               x_search=sentinel(n, A, 3, dtype=f32), moved=sentinel(n), moved_flex=sentinel(n))
    rc = L.pd_vina_flex_search_select(*fg.head(x, d), P(ws), numel, *[P(sel[k]) for k in SELECTED], *sz, S())
    assert rc == 0, rc
    out.update({k: body(v, finite) for k, v in sel.items()})
    assert not (out["best_chain"] == fg.I_SENTINEL).any() and untouched(ws[-1:])
    n2 = (6 + N) ** 2                                                                  # the chains' float64 best, as the workspace holds them
    out["best64"] = ws[:numel].view(n, K, n2 + 9 * M + 8)[:, :, n2 + 6 * M:n2 + 9 * M].reshape(n, K, M, 3).clone()
    return out


def same(a, b, keys=None):
    return all(torch.equal(a[k], b[k]) for k in (keys or a))


@pytest.fixture(scope="module")
def reference_runs(cases):
    """(case, kind) -> the reference search, computed once"""
    out = {}
    for name, (seed, st) in fs.GPU_CASES.items():
        out[name, "trajectory"] = fs.search(cases[name][0], seed=seed, **st)
        out[name, "proposal"] = fs.search(cases[name][0], seed=seed, **dict(st, **PROPOSAL))
    return out


@pytest.fixture(scope="module")
def device_runs(L, cases):
    return {name: launch_search(L, c, d, **settings(name)) for name, (c, d) in cases.items()}


def per_chain(run, key):
    return [[r[key] for r in row] for row in run["chains"]]


# ------------------------------------------------------------------ 1. steps = 0 is pd_vina_flex_refine
@pytest.mark.parametrize("name", list(fs.GPU_CASES))
def test_zero_steps_is_flex_refine_bit_for_bit(L, cases, name):
    c, d = cases[name]
    st = settings(name, steps=0)
    out = launch_search(L, c, d, **st)
    want = fg.launch_refine(L, c["x"], c, d, max_iters=st["max_iters"], trace=False)
    mov = torch.from_numpy(c["mov_idx"].astype(np.int64)).cuda()
    for k in range(st["chains"]):
        assert torch.equal(out["x_chains"][:, k], want["x_refined"][:, mov]), (name, k)
        assert torch.equal(out["energy_chains"][:, k], want["energy"]) and torch.equal(out["energy_start"][:, k], want["energy"])
        assert torch.equal(out["evaluations"][:, k], want["evaluations"])
    assert torch.equal(out["trace_energy"][:, :, 0], out["energy_start"]) and out["trace_entity"].numel() == 0
    assert not out["best_step"].any() and not out["accepted"].any() and not out["best_chain"].any()
    assert torch.equal(out["x_search"], want["x_refined"])
    for k in ("energy", "inter", "intra", "receptor", "moved", "moved_flex"):
        assert torch.equal(out[k], want[k]), (name, k)


# ------------------------------------------------------------------ 2. the proposal alone
def test_the_proposal_alone(L, cases, reference_runs):
    side_chain_shown = 0
    for name in fs.GPU_CASES:
        c, d = cases[name]
        want = reference_runs[name, "proposal"]
        out = launch_search(L, c, d, **settings(name, **PROPOSAL))
        assert out["trace_entity"][:, :, 0].cpu().tolist() == [[e[0] for e in row] for row in per_chain(want, "entity")], name
        assert out["best_step"].cpu().tolist() == per_chain(want, "best_step"), name
        assert out["accepted"].cpu().tolist() == [[1] * len(row) for row in want["chains"]]        # temperature = inf
        assert out["evaluations"].cpu().tolist() == [[2] * len(row) for row in want["chains"]]     # max_iters = 0: one evaluation per descent
        got = out["x_chains"].cpu().numpy()
        start = c["x"][:, c["mov_idx"]]
        for p, row in enumerate(want["chains"]):
            for k, r in enumerate(row):
                if r["best_step"] == 1:
                    y = r["proposals"][0]
                    ulp = np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)
                    assert (np.abs(got[p, k].astype(np.float64) - y) <= ulp).all(), (name, p, k, np.abs(got[p, k] - y).max())
                    side_chain_shown += int(r["entity"][0] >= 2 + c["T"])
                else:
                    assert np.array_equal(got[p, k], start[p]), (name, p, k)
    assert side_chain_shown >= 1


# ------------------------------------------------------------------ 3. the trajectory
@pytest.mark.parametrize("name", list(fs.GPU_CASES))
def test_search_takes_the_reference_trajectory(cases, reference_runs, device_runs, name):
    """Measured on an MI355X (TRAJECTORY lines): see NOTES.md "FlexSearch"."""
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
    # the winner's energy within the envelope of flex_refine_ref.evaluate at the winner: the float64 conformation the device ended at
    # (the workspace's `best`, whose fp32 rounding is x_search).  At the REFERENCE's end point the envelope of one evaluation cannot
    # hold: the reference's own twin run ends up to 3e-12 kcal/mol away from it, the end point's wander through the descents
    mov = torch.from_numpy(c["mov_idx"].astype(np.int64)).cuda()
    win = out["best64"][torch.arange(len(want["y"])).cuda(), out["best_chain"].long()]
    assert torch.equal(win.float(), out["x_search"][:, mov])
    evs = [ref.evaluate(c, c["x"][p].astype(np.float64), win[p].cpu().numpy(), bounds=True) for p in range(len(want["y"]))]
    errs, bounds = [abs(float(out["energy"][p]) - ev["energy"]) for p, ev in enumerate(evs)], [ev["bound"]["energy"] for ev in evs]
    wander = max(abs(float(out["energy"][p]) - want["energy"][p]) for p in range(len(want["y"])))
    print(f"TRAJECTORY | pd_vina_flex_search | {name} | {diff:.3e} | {ediff:.3e} | winner's energy {max(errs):.3e} | its bound {min(bounds):.3e} | "
          f"from the reference's end point {wander:.3e} |")
    assert diff <= 1e-6 + ulp, (name, diff)
    assert np.abs(out["x_search"][:, mov].cpu().double().numpy() - want["y"]).max() <= 1e-6 + ulp
    for p, (err, b) in enumerate(zip(errs, bounds)):
        assert err <= b, (name, p, err, b)
    for k in ("moved", "moved_flex"):
        w = [want["chains"][p][b][k] for p, b in enumerate(want["best_chain"])]
        assert np.abs(out[k].cpu().numpy() - w).max() <= np.sqrt(3.0) * 1e-6, k


# ------------------------------------------------------------------ 4. resumable, and cut by the workspace
@pytest.mark.parametrize("name", ["small", "over_block"])
def test_a_search_cut_into_launches_is_the_same_search(L, cases, device_runs, name):
    c, d = cases[name]
    st = settings(name)
    for per in (1, 2):                                                                  # steps_per_launch = 1, 2
        splits = [per] * (st["steps"] // per) + ([st["steps"] % per] if st["steps"] % per else [])
        cut = launch_search(L, c, d, splits=splits, **st)
        assert same(cut, device_runs[name]), (per, [k for k in cut if not torch.equal(cut[k], device_runs[name][k])])
    assert same(launch_search(L, c, d, splits=(0, st["steps"], 0), **st), device_runs[name])     # an empty launch changes nothing
    f = fg.flex_refine_of(c)
    x = torch.from_numpy(c["x"]).cuda()
    whole = f.search(x, trace=True, **st)
    assert same(whole, device_runs[name], [k for k in device_runs[name] if k not in ("x_chains", "best64")])
    assert same(f.search(x, trace=True, workspace_bytes=1, **st), whole)                 # one pose per launch
    assert same(f.search(x, trace=True, workspace_bytes=1, steps_per_launch=1, **st), whole)
    assert same(f.search(x, trace=True, steps_per_launch=2, **st), whole)


# ------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("name", ["small", "rigid_ligand"])
def test_independence(L, cases, device_runs, name):
    c, d = cases[name]
    st, out = settings(name), device_runs[name]
    assert same(launch_search(L, c, d, **st), out)                                      # two identical launches
    per = OUTS + TRACES
    few = launch_search(L, c, d, **dict(st, chains=1))                                  # chain 0 of K = 1 and of K = 3
    assert all(torch.equal(few[k], out[k][:, :1]) for k in per), name
    for q in range(c["x"].shape[0]):                                                    # alone under its pose id, and inside the batch
        one = launch_search(L, c, d, x=c["x"][q:q + 1], pose0=q, **st)
        assert all(torch.equal(one[k][0], out[k][q]) for k in per + SELECTED), (name, q)
    shifted = launch_search(L, c, d, x=c["x"][::-1], pose0=5, **st)                     # the pose ids 5, 6, ...: other draws ...
    back = launch_search(L, c, d, x=c["x"][-1:], pose0=5, **st)                         # ... that follow the id, not the place
    assert all(torch.equal(back[k][0], shifted[k][0]) for k in per + SELECTED)
    assert not torch.equal(shifted["trace_entity"].flip(0), out["trace_entity"])
    bare = launch_search(L, c, d, trace=False, **st)                                    # the traces are optional
    assert not set(bare) & set(TRACES) and same(bare, out, OUTS + SELECTED)
    other = launch_search(L, c, d, **dict(st, seed=st["seed"] + 1))
    assert not torch.equal(other["trace_entity"], out["trace_entity"]) and torch.equal(other["energy_start"], out["energy_start"])


# ------------------------------------------------------------------ 6. no flexible residue: pd_vina_search
def test_no_flex_agrees_with_pd_vina_search(L, cases, device_runs):
    import test_vina_refine_gpu as rg
    import test_vina_search_gpu as sg
    c, _ = cases["no_flex"]
    b = vrr.make_case(ref.CASES["no_flex"]["base"])
    st = settings("no_flex")
    rigid = sg.launch_search(L, b, rg.tables(b), **{k: v for k, v in st.items() if k != "chi_amp"})
    out = device_runs["no_flex"]
    for k in ("best_step", "accepted", "evaluations", "best_chain") + TRACES[1:]:
        assert torch.equal(out[k], rigid[k]), k
    diff, ulp, ok = fg.close_coordinates(out["x_chains"].cpu().double().numpy(), rigid["x_chains"].cpu().double().numpy())
    assert ok and fg.close_coordinates(out["x_search"].cpu().double().numpy(), rigid["x_search"].cpu().double().numpy())[2], diff
    print(f"AGREEMENT | no_flex vs pd_vina_search | coordinates {diff:.3e} | bit-equal {torch.equal(out['x_chains'], rigid['x_chains'])} |")
    assert not out["receptor"].any() and not out["moved_flex"].any()


# ------------------------------------------------------------------ 7. invariants of x_search and x_chains
@pytest.mark.parametrize("name", list(fs.GPU_CASES))
def test_invariants_of_x_search_and_x_chains(cases, device_runs, name):
    c, _ = cases[name]
    out = device_runs[name]
    x = torch.from_numpy(c["x"]).cuda()
    n, A, K = x.shape[0], x.shape[1], out["x_chains"].shape[1]
    mov = torch.from_numpy(c["mov_idx"].astype(np.int64)).cuda()
    rest = torch.from_numpy(np.setdiff1d(np.arange(A), c["mov_idx"])).cuda()
    assert torch.equal(out["x_search"][:, rest], x[:, rest]), "a fixed row changed"
    full = x[:, None].expand(n, K, A, 3).contiguous()
    full[:, :, mov] = out["x_chains"]
    pick = out["x_chains"][torch.arange(n).cuda(), out["best_chain"].long()]
    assert torch.equal(out["x_search"][:, mov], pick)
    poses = torch.cat([out["x_search"][:, None], full], 1)                              # [n, 1 + K, A, 3]
    if c["F"]:                                                                       # the anchors never move
        ca = torch.from_numpy(np.asarray([c["mov_idx"][r[0]] for r in c["residue_rows"]], dtype=np.int64)).cuda()
        assert torch.equal(poses[:, :, ca], x[:, None, ca].expand(n, 1 + K, -1, 3))
    adj = np.zeros((A, A), dtype=bool)
    lig = c["lig_idx"].astype(np.int64)
    for i, j in c["bonds"]:
        adj[lig[i], lig[j]] = adj[lig[j], lig[i]] = True
    rec = np.zeros((A, A), dtype=bool)
    for i, j in c["rec_bonds"]:
        rec[i, j] = rec[j, i] = True
    keep = adj | rec | ((rec.astype(int) @ rec.astype(int)) > 0)                        # ligand bonds; receptor bonds and 1-3
    np.fill_diagonal(keep, False)
    ii, jj = np.nonzero(np.triu(keep))
    x0, x1 = c["x"].astype(np.float64), poses.cpu().double().numpy()
    d0 = np.sqrt(((x0[:, ii] - x0[:, jj]) ** 2).sum(-1))
    d1 = np.sqrt(((x1[:, :, ii] - x1[:, :, jj]) ** 2).sum(-1))
    tol = 2.0 * float(np.spacing(np.float32(max(np.abs(x0).max(), np.abs(x1).max()))))     # (test_invariants_of_x_refined's)
    worst = np.abs(d1 - d0[:, None]).max()
    assert worst <= tol, (name, worst, tol)
    assert torch.equal(out["energy"], (out["inter"] + out["intra"]) + out["receptor"])
    e = out["energy_chains"].cpu().numpy()
    assert np.array_equal(out["energy"].cpu().numpy(), e.min(1)) and np.array_equal(out["best_chain"].cpu().numpy(), e.argmin(1))
    assert (out["energy"][:, None] <= out["energy_start"]).all()
    tr = out["trace_energy"].cpu().numpy()
    assert np.isfinite(tr).all() and np.array_equal(e, tr.min(-1)) and np.array_equal(out["energy_start"].cpu().numpy(), tr[:, :, 0])


# ------------------------------------------------------------------ 8. a non-finite movable coordinate
def test_a_non_finite_coordinate_ends_as_the_reference_says(L, cases, device_runs):
    """E stays finite (a pair at a non-finite distance is no pair), so the Metropolis test goes on; every descent of the pose ends
    before its first step.  tests/test_flex_search_cpu.py guards the reference's decisions for exactly these inputs."""
    c, d = cases["small"]
    st = settings("small")
    clean = device_runs["small"]
    for row in (3, c["L"] + 2):                                                      # a ligand row; a side-chain row of a moving set
        x = c["x"].copy()
        x[0, c["mov_idx"][row]] = np.nan
        want = fs.search(c, x=x[:1], seed=st["seed"], **fs.GPU_CASES["small"][1])["chains"][0]
        out = launch_search(L, c, d, x=x, finite=False, **st)
        assert not out["trace_iterations"][0].any() and bool((out["trace_status"][0] == 2).all())
        assert out["evaluations"][0].cpu().tolist() == [st["steps"] + 1] * st["chains"] == [r["evaluations"] for r in want]
        for dev, key in (("trace_entity", "entity"), ("trace_accept", "accept")):
            assert out[dev][0].cpu().tolist() == [r[key] for r in want], (row, dev)
        for key in ("best_step", "accepted"):
            assert out[key][0].cpu().tolist() == [r[key] for r in want], (row, key)
        assert bool(torch.isfinite(out["trace_energy"][0]).all())
        assert np.abs(out["trace_energy"][0].cpu().numpy() - np.asarray([r["trace_energy"] for r in want])).max() <= 1e-9
        assert all(torch.equal(out[k][1:], clean[k][1:]) for k in OUTS + TRACES + SELECTED), "the poses beside it changed"


# ------------------------------------------------------------------ 9. refusals
def test_error_codes(L, cases):
    c, d = cases["small"]
    x = torch.from_numpy(c["x"]).cuda()
    n, A, Lg, F, T, S_ = fg.sizes(c, 3)
    K, M, steps = 3, Lg + F, 2
    numel = L.pd_vina_flex_search_workspace_numel(n, K, M, T + S_)
    i32, f32 = torch.int32, torch.float32
    ws = sentinel(numel)
    bufs = [sentinel(n, K, M, 3, dtype=f32), sentinel(n, K), sentinel(n, K), sentinel(n, K, dtype=i32), sentinel(n, K, dtype=i32), sentinel(n, K, dtype=i32),
            sentinel(n, K, steps + 1)] + [sentinel(n, K, steps, dtype=i32) for _ in range(4)]
    h = fg.head(x, d)
    base = dict(mi=3, gt=1e-4, ms=1.0, seed=5, pose0=0, step0=0, ns=steps, total=steps, temp=1.2, ta=2.0, ra=1.0, ca=3.0)

    def call(h=h, ws_=P(ws), wn=numel, outs=None, sizes=(n, K, A, Lg, F, T, S_), **over):
        a = dict(base, **over)
        outs = [P(b) for b in bufs] if outs is None else outs
        return L.pd_vina_flex_search(*h, a["mi"], a["gt"], a["ms"], a["seed"], a["pose0"], a["step0"], a["ns"], a["total"], a["temp"], a["ta"],
                                     a["ra"], a["ca"], ws_, wn, *outs, *sizes, S())

    rcs = {}
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11):                                       # x .. excl_atom
        hh = list(h)
        hh[k] = None
        rcs[f"null table {k}"] = call(h=hh)
    for k in (0, 1, 5, 6, 7, 8, 10, 11):
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
                     ("temp", 0.0), ("temp", -1.0), ("temp", NAN), ("ta", -1.0), ("ta", NAN), ("ra", -0.5), ("ra", NAN), ("ca", -0.5), ("ca", NAN)):
        rcs[f"{key}={bad}"] = call(**{key: bad})
    rcs["step0 + n_steps > steps_total"] = call(step0=1, ns=2)
    for k in range(4):
        sz = [n, K, A, Lg, F, T, S_]
        sz[k] = 0
        rcs[f"size {k} = 0"] = call(sizes=sz)
    rcs["F<0"], rcs["T<0"], rcs["S<0"] = call(sizes=(n, K, A, Lg, -1, T, S_)), call(sizes=(n, K, A, Lg, F, -1, S_)), call(sizes=(n, K, A, Lg, F, T, -1))
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), rcs
    unsupported = {"L + F": call(sizes=(n, K, A, Lg, 1025 - Lg, T, S_)), "T + S": call(sizes=(n, K, A, Lg, F, T, 59 - T)),
                   "A": call(sizes=(n, K, (1 << 22) + 1, Lg, F, T, S_)), "K": call(sizes=(n, 65, A, Lg, F, T, S_)),
                   "P K": call(sizes=(21846, 3, A, Lg, F, T, S_)), "P": call(sizes=(65536, 1, A, Lg, F, T, S_))}
    assert all(rc == PD_ERR_UNSUPPORTED for rc in unsupported.values()), unsupported
    # the selection
    sel = [sentinel(n, dtype=i32)] + [sentinel(n) for _ in range(4)] + [sentinel(n, A, 3, dtype=f32), sentinel(n), sentinel(n)]

    def select(h=h, ws_=P(ws), wn=numel, outs=None, sizes=(n, K, A, Lg, F, T, S_)):
        outs = [P(b) for b in sel] if outs is None else outs
        return L.pd_vina_flex_search_select(*h, ws_, wn, *outs, *sizes, S())

    rcs = {}
    for k in (0, 1, 2, 3, 4, 7, 10):
        hh = list(h)
        hh[k] = None
        rcs[f"select null table {k}"] = select(h=hh)
    for k in (0, 1, 5, 6):                                                              # best_chain, energy, x_search, moved
        outs = [P(b) for b in sel]
        outs[k] = None
        rcs[f"select null output {k}"] = select(outs=outs)
    for k in range(len(sel)):
        outs = [P(b) for b in sel]
        outs[k] = outs[k] + (2 if sel[k].dtype != torch.float64 else 4)
        rcs[f"select misaligned output {k}"] = select(outs=outs)
    rcs["select null ws"], rcs["select misaligned ws"], rcs["select short ws"] = select(ws_=None), select(ws_=P(ws) + 4), select(wn=numel - 1)
    for k in range(4):
        sz = [n, K, A, Lg, F, T, S_]
        sz[k] = 0
        rcs[f"select size {k} = 0"] = select(sizes=sz)
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), rcs
    unsupported = {"K": select(sizes=(n, 65, A, Lg, F, T, S_)), "L + F": select(sizes=(n, K, A, Lg, 1025 - Lg, T, S_)),
                   "T + S": select(sizes=(n, K, A, Lg, F, T, 59 - T)), "P K": select(sizes=(21846, 3, A, Lg, F, T, S_))}
    assert all(rc == PD_ERR_UNSUPPORTED for rc in unsupported.values()), unsupported
    torch.cuda.synchronize()
    assert all(untouched(b) for b in bufs + sel) and untouched(ws), "a rejected call wrote"
    assert call() == 0 and select() == 0
    for b in bufs + sel:
        body(b)
    assert untouched(ws[-1:])


# ------------------------------------------------------------------ 10. FlexRefine.search
def test_python_surface(cases, device_runs):
    name = "small"
    c, _ = cases[name]
    f = fg.flex_refine_of(c)
    x = torch.from_numpy(c["x"]).cuda()
    st = settings(name)
    out = f.search(x, trace=True, **st)
    f64, f32, i32 = torch.float64, torch.float32, torch.int32
    n, K, A, steps, R = 3, 3, 96, st["steps"], 3
    want = dict(x_search=(f32, (n, A, 3)), energy=(f64, (n,)), inter=(f64, (n,)), intra=(f64, (n,)), receptor=(f64, (n,)), best_chain=(i32, (n,)),
                x_chains=(f32, (n, K, A, 3)), energy_chains=(f64, (n, K)), energy_start=(f64, (n, K)), best_step=(i32, (n, K)),
                accepted=(i32, (n, K)), evaluations=(i32, (n, K)), moved=(f64, (n,)), moved_flex=(f64, (n,)), residue_moved=(f64, (n, R)),
                score_start=(f32, (n,)), score=(f32, (n,)), trace_energy=(f64, (n, K, steps + 1)), trace_entity=(i32, (n, K, steps)),
                trace_accept=(i32, (n, K, steps)), trace_iterations=(i32, (n, K, steps)), trace_status=(i32, (n, K, steps)))
    assert {k: (t.dtype, tuple(t.shape)) for k, t in out.items()} == want and all(t.is_cuda for t in out.values())
    raw = device_runs[name]
    assert all(torch.equal(out[k], raw[k]) for k in raw if k not in ("x_chains", "best64"))
    mov = torch.from_numpy(c["mov_idx"].astype(np.int64)).cuda()
    rest = torch.from_numpy(np.setdiff1d(np.arange(A), c["mov_idx"])).cuda()
    assert torch.equal(out["x_chains"][:, :, mov], raw["x_chains"]) and torch.equal(out["x_chains"][:, :, rest], x[:, None, rest].expand(n, K, -1, 3))
    assert torch.equal(out["score"], f.vina.score(out["x_search"])["score"]) and torch.equal(out["score_start"], f.vina.score(x)["score"])
    disp = (out["x_search"].double() - x.double()).pow(2).sum(-1).sqrt().cpu().numpy()
    assert np.array_equal(out["residue_moved"].cpu().numpy(), np.stack([disp[:, c["mov_idx"][r].astype(np.int64)].max(1) for r in c["residue_rows"]], 1))
    assert torch.equal(out["energy_start"][:, 0], f.refine(x, max_iters=st["max_iters"])["energy"])
    plain = f.search(x, **st)
    assert set(plain) == set(want) - set(TRACES) and same(plain, out, plain)
    shifted = f.search(x[1:], pose0=1, **st)
    assert all(torch.equal(shifted[k], plain[k][1:]) for k in plain)
    from physdock_amd import VinaRefine
    auto = f.search(x, **dict(st, rotate_amp=None))                                     # the default amplitude, from the first pose
    assert same(auto, f.search(x, **dict(st, rotate_amp=VinaRefine.default_rotate_amp(f, x, st["translate_amp"]))))
    assert same(f.search(x, **{k: v for k, v in st.items() if k != "chi_amp"}), plain)    # chi_amp defaults to pi


# ------------------------------------------------------------------ 11. redock(flex=, flex_search=)
def test_redock_reports_the_flexible_search_and_changes_nothing_else(small_model_inputs):
    from physdock_amd import FlexRefine, PhysDock, VinaRefine, driver
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.ranking import rank_by_score
    from physdock_amd.receptor_geometry import ReceptorGeometry
    from physdock_amd.validity import PoseValidity
    cfg, P_, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P_, strict=True)
    model, dbatch = model.cuda().eval(), {k: v.cuda() for k, v in batch.items()}
    lig = ligand_atom_mask(dbatch).cpu().numpy()
    rid = dbatch["atom_id_to_token_id"].cpu().numpy()
    atoms, seen = [], {}
    for r in rid:                                                                    # every protein token a serine without its O
        atoms.append(("N", "CA", "C", "CB", "OG")[seen.get(r, 0) % 5])
        seen[r] = seen.get(r, 0) + 1
    res = ["LIG" if l else "SER" for l in lig]
    bonds = [(i, i + 1) for i in range(int(lig.sum()) - 1)]
    refine = VinaRefine.from_batch(dbatch, bonds)
    rec_ok = np.asarray(refine.vina.rec_mask).reshape(-1) > 0
    protein = [t for t in sorted(set(rid[~lig].tolist())) if rec_ok[rid == t].all() and (rid == t).sum() == 5]
    flex = FlexRefine.from_refine(refine, res, atoms, rid, protein[:3], device="cuda")
    geometry = ReceptorGeometry.from_names(res, atoms, rid, dbatch["x_gt"], n_residues=int(dbatch["is_ligand"].shape[0]), device="cuda")
    validity = PoseValidity.from_batch(dbatch, bonds)
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    spec = dict(chains=2, steps=2, max_iters=3, seed=11)
    base = driver.redock(model, dbatch, flex=flex, **kw)
    out = driver.redock(model, dbatch, flex=flex, flex_search=spec, **kw)
    assert set(out) == set(base) | {"flex_searched"} and fg.same_result({k: out[k] for k in base}, base)
    n, A = out["poses"].shape[0], out["poses"].shape[1]
    direct = flex.search(out["poses"], **spec)
    assert fg.same_result(out["flex_searched"], direct)
    assert direct["x_search"].shape == (n, A, 3) and direct["x_chains"].shape == (n, 2, A, 3) and (direct["energy"][:, None] <= direct["energy_start"]).all()
    assert torch.equal(direct["energy_start"][:, 0], flex.refine(out["poses"], max_iters=3)["energy"])
    full = driver.redock(model, dbatch, flex=flex, vina=refine.vina, validity=validity, receptor_geometry=geometry, flex_search=spec, **kw)
    assert {"flex_searched", "order_vina_flex_searched", "flex_refined", "order_vina_flex"} <= set(full)
    xs = full["flex_searched"]["x_search"]
    assert fg.same_result(full["flex_searched"]["validity"], validity.check(xs))
    assert fg.same_result(full["flex_searched"]["receptor_geometry"], geometry.check(xs))
    order = full["order_vina_flex_searched"]
    assert torch.equal(order, rank_by_score({"score": full["flex_searched"]["score"]})) and sorted(order.tolist()) == list(range(n))
    assert torch.equal(full["poses"], base["poses"])
    assert fg.same_result(driver.redock(model, dbatch, flex=flex, flex_search=None, **kw), base)
    many = driver.redock_many(model, [(dbatch, {"flex": flex, "flex_search": spec})], **kw)
    assert fg.same_result(many[0], out)
    with pytest.raises(ValueError, match="flex="):
        driver.redock(model, dbatch, flex_search=True, **kw)
