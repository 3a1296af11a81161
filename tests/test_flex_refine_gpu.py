"""pd_vina_flex_energy and pd_vina_flex_refine (csrc/vina_flex.hip) straight on the C ABI, FlexRefine.refine / .energy, and the flex
keyword of redock / redock_many.

The yardstick is the float64 restatement tests/flex_refine_ref.py.  The energy kernel must satisfy |dev - ref| <= bound element by
element, the bound derived there, nothing multiplied on.  The refinement must take the reference's trajectory: equal iterations,
evaluations and status, movable coordinates within 1e-6 A plus one fp32 ulp of the largest coordinate (the criterion of
tests/test_vina_refine_gpu.py; the guard in tests/test_flex_refine_cpu.py holds the reference to 1e-8 A against its own reversed
summation).  One `ENVELOPE | pd_vina_flex_energy | ...` line is printed per output (pytest -s) and one `TRAJECTORY | ...` line per
run.  Output buffers are one row longer than needed and pre-filled with a sentinel."""
import numpy as np
import pytest
import torch

import flex_refine_ref as ref
import vina_refine_ref as vrr

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN = float("nan")
I_SENTINEL = -77
ENERGY_KEYS = ("energy", "inter", "intra", "receptor", "grad", "ggrad")


def sentinel(*shape, dtype=torch.float64):
    fill = NAN if dtype.is_floating_point else I_SENTINEL
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), fill, device="cuda", dtype=dtype)


def untouched(buf):
    return bool(torch.isnan(buf).all()) if buf.dtype.is_floating_point else bool((buf == I_SENTINEL).all())


def body(buf, finite=True):
    torch.cuda.synchronize()
    assert untouched(buf[-1]), "the row behind the output was written"
    if buf.dtype.is_floating_point and finite:
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


def sizes(c, n):
    return (n, c["x"].shape[1], c["L"], c["F"], c["T"], c["S"])


def tables(c):
    """a case's tables on the device, every index the kernel would follow checked to be inside its array first"""
    A, Lg, M, N = c["x"].shape[1], c["L"], c["L"] + c["F"], c["T"] + c["S"]
    lists = ref.csr(c)
    assert len(c["mov_idx"]) == M and 0 <= c["mov_idx"].min() and c["mov_idx"].max() < A and len(set(c["mov_idx"].tolist())) == M
    assert len(c["types"]) == A == len(c["fixed_mask"]) and len(c["active"]) == M and not c["fixed_mask"][c["mov_idx"]].any()
    assert c["rot"].shape == (N, 2) and (N == 0 or (0 <= c["rot"].min() and c["rot"].max() < M)) and c["mask"].shape == (N, (M + 31) // 32)
    assert all(len(m) and 0 <= m.min() and m.max() < M for m in c["sets"])                # (the mask's bits are those of the sets)
    ps, pa, es, ea = lists["pair_start"], lists["pair_atom"], lists["excl_start"], lists["excl_atom"]
    assert len(ps) == M + 1 and ps[0] == 0 and (np.diff(ps) >= 0).all() and ps[-1] == len(pa) and (len(pa) == 0 or (0 <= pa.min() and pa.max() < M))
    assert len(es) == M + 1 and es[0] == 0 and (np.diff(es) >= 0).all() and es[-1] == len(ea) and (len(ea) == 0 or (0 <= ea.min() and ea.max() < A))
    assert M <= 1024 and N <= 58
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()
    return dict(mov_idx=up(c["mov_idx"], np.int32), types=up(c["types"], np.uint8), fixed_mask=up(c["fixed_mask"], np.uint8),
                active=up(c["active"], np.uint8), rot=up(c["rot"], np.int32), mask=up(c["mask"].view(np.int32), np.int32), pair_start=up(ps, np.int32),
                pair_atom=up(pa, np.int32), excl_start=up(es, np.int32), excl_atom=up(ea, np.int32), n_pair=len(pa), n_excl=len(ea), N=N)


def head(x, d):
    return [P(x), P(d["mov_idx"]), P(d["types"]), P(d["fixed_mask"]), P(d["active"]), P(d["rot"]) if d["N"] else None,
            P(d["mask"]) if d["N"] else None, P(d["pair_start"]), P(d["pair_atom"]) if d["n_pair"] else None, d["n_pair"],
            P(d["excl_start"]), P(d["excl_atom"]) if d["n_excl"] else None, d["n_excl"]]


def launch_energy(L, x, c, d=None):
    d = d or tables(c)
    x = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    n, M = x.shape[0], c["L"] + c["F"]
    buf = dict(energy=sentinel(n), inter=sentinel(n), intra=sentinel(n), receptor=sentinel(n), grad=sentinel(n, M, 3), ggrad=sentinel(n, 6 + d["N"]))
    rc = L.pd_vina_flex_energy(*head(x, d), *[P(buf[k]) for k in ENERGY_KEYS], *sizes(c, n), S())
    assert rc == 0, rc
    return {k: body(v) for k, v in buf.items()}


REFINE_KEYS = ("x_refined", "energy_start", "energy", "inter", "intra", "receptor", "iterations", "evaluations", "status", "moved", "moved_flex")


def launch_refine(L, x, c, d=None, max_iters=20, grad_tol=1e-4, max_step=1.0, trace=True, finite=True):
    d = d or tables(c)
    x = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    n, A, M = x.shape[0], x.shape[1], c["L"] + c["F"]
    numel = L.pd_vina_flex_workspace_numel(n, M, d["N"])
    assert numel == n * ((6 + d["N"]) ** 2 + 3 * M)
    ws = sentinel(numel)
    i32 = torch.int32
    buf = dict(x_refined=sentinel(n, A, 3, dtype=torch.float32), energy_start=sentinel(n), energy=sentinel(n), inter=sentinel(n), intra=sentinel(n),
               receptor=sentinel(n), iterations=sentinel(n, dtype=i32), evaluations=sentinel(n, dtype=i32), status=sentinel(n, dtype=i32),
               moved=sentinel(n), moved_flex=sentinel(n))
    if trace:
        buf["energy_trace"] = sentinel(n, max_iters + 1)
    rc = L.pd_vina_flex_refine(*head(x, d), max_iters, grad_tol, max_step, P(ws), numel, *[P(buf[k]) for k in REFINE_KEYS],
                               P(buf["energy_trace"]) if trace else None, *sizes(c, n), S())
    assert rc == 0, rc
    out = {k: body(v, finite) for k, v in buf.items()}
    assert untouched(ws[-1:]), "the element behind the workspace was written"
    assert not (out["iterations"] == I_SENTINEL).any() and not (out["status"] == I_SENTINEL).any()
    return out


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------ the energy kernel
def oracle(c):
    outs = [ref.evaluate(c, c["x"][p].astype(np.float64), c["x"][p].astype(np.float64)[c["mov_idx"]], bounds=True) for p in range(c["x"].shape[0])]
    return ({k: np.stack([np.asarray(o[k]) for o in outs]) for k in ENERGY_KEYS},
            {k: np.stack([np.asarray(o["bound"][k]) for o in outs]) for k in ENERGY_KEYS}, min(o["margin"] for o in outs))


@pytest.mark.parametrize("name", list(ref.CASES))
def test_energy_kernel_against_float64(L, cases, name):
    c = cases[name]
    want, bound, margin = oracle(c)
    assert margin >= ref.GPU_MARGIN
    d = tables(c)
    out = launch_energy(L, c["x"], c, d)
    for k in want:
        dev, r, b = out[k].cpu().numpy(), want[k], bound[k]
        assert dev.dtype == np.float64 and dev.shape == r.shape == b.shape, (name, k, dev.shape, r.shape)
        err = np.abs(dev - r)
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
        worst = np.unravel_index(np.argmax(ratio), ratio.shape) if ratio.ndim else ()
        print(f"ENVELOPE | pd_vina_flex_energy | {name} {k} | {np.abs(r).max():.2e} | {err.max():.2e} | {b[worst]:.2e} | {ratio.max():.2f} |")
        assert (err <= b).all(), (name, k, "err", err.max(), "bound", b[worst], "ratio", ratio.max())
    assert same(launch_energy(L, c["x"], c, d), out)                                   # launch to launch
    for p in range(c["x"].shape[0]):                                                   # alone and inside the batch
        one = launch_energy(L, c["x"][p:p + 1], c, d)
        assert all(torch.equal(one[k][0], out[k][p]) for k in out), (name, p)
    assert torch.equal(out["energy"], (out["inter"] + out["intra"]) + out["receptor"])
    x = torch.from_numpy(c["x"]).cuda()                                                # every output may be NULL
    n = c["x"].shape[0]
    e = sentinel(n)
    assert L.pd_vina_flex_energy(*head(x, d), P(e), None, None, None, None, None, *sizes(c, n), S()) == 0
    assert torch.equal(body(e), out["energy"])


# ------------------------------------------------------------------ the refinement
@pytest.fixture(scope="module")
def reference_runs(cases):
    return {(name, mi): [ref.refine(cases[name], cases[name]["x"][p].astype(np.float64), max_iters=mi) for p in range(cases[name]["x"].shape[0])]
            for name, mi in ref.RUNS}


@pytest.fixture(scope="module")
def device_runs(L, cases):
    return {(name, mi): launch_refine(L, cases[name]["x"], cases[name], max_iters=mi) for name, mi in ref.RUNS}


def close_coordinates(y, yr):
    ulp = float(np.spacing(np.float32(np.abs(yr).max())))
    diff = float(np.abs(y - yr).max())
    return diff, ulp, diff <= 1e-6 + ulp


@pytest.mark.parametrize("name,mi", ref.RUNS)
def test_refinement_takes_the_reference_trajectory(cases, reference_runs, device_runs, name, mi):
    c, want, out = cases[name], reference_runs[name, mi], device_runs[name, mi]
    for k in ("iterations", "evaluations", "status"):
        assert out[k].cpu().tolist() == [w[k] for w in want], (name, mi, k, out[k].cpu().tolist(), [w[k] for w in want])
    mov = torch.from_numpy(c["mov_idx"].astype(np.int64)).cuda()
    y = out["x_refined"][:, mov].cpu().double().numpy()
    diff, ulp, ok = close_coordinates(y, np.stack([w["y"] for w in want]))
    print(f"TRAJECTORY | {name} max_iters {mi} | largest coordinate difference {diff:.3e} | fp32 ulp {ulp:.3e} | moved "
          f"{max(w['moved'] for w in want):.3f} | moved_flex {max(w['moved_flex'] for w in want):.3f} |")
    assert ok, (name, mi, diff)
    for k in ("moved", "moved_flex"):
        assert np.abs(out[k].cpu().numpy() - [w[k] for w in want]).max() <= np.sqrt(3.0) * 1e-6
    tr = out["energy_trace"]                                                           # the trace is non-increasing
    assert (tr[:, 1:] <= tr[:, :-1]).all() and torch.equal(tr[:, 0], out["energy_start"]) and torch.equal(tr[:, -1], out["energy"])
    assert torch.equal(out["energy"], (out["inter"] + out["intra"]) + out["receptor"])
    for p, w in enumerate(want):
        # the final energy within the energy bound, as for pd_vina_refine (the guard on the CPU keeps a quarter of it for the end point's
        # own wander).  Its three parts are not stationary at the end point, so they are held to the identity above, not to a bound
        b = ref.evaluate(c, c["x"][p].astype(np.float64), w["y"], bounds=True)["bound"]["energy"]
        err = abs(float(out["energy"][p]) - w["energy"])
        print(f"ENVELOPE | pd_vina_flex_refine energy | {name} max_iters {mi} pose {p} | {abs(w['energy']):.2e} | {err:.2e} | {b:.2e} |")
        assert err <= b, (name, mi, p, err, b)


def test_the_device_reproduces_the_behavioural_case(cases, reference_runs, device_runs):
    """tests/test_flex_refine_cpu.py shows with the reference alone that the flexible refinement of `across` ends lower than the rigid
    one; the device takes that trajectory (above) and so ends lower as well, in its own numbers"""
    c = cases["across"]
    mi = dict(ref.RUNS)["across"]
    out = device_runs["across", mi]
    for p in range(c["x"].shape[0]):
        xp = c["x"][p].astype(np.float64)
        rigid = ref.refine(ref.frozen_side_chains(c), xp, max_iters=mi)
        e_rigid = ref.evaluate(c, xp, rigid["y"])["energy"]
        assert float(out["energy"][p]) < e_rigid - 0.1 and float(out["moved_flex"][p]) > 0.1


def test_no_flex_agrees_with_pd_vina_refine(L, cases, device_runs):
    c = cases["no_flex"]
    b = vrr.make_case(ref.CASES["no_flex"]["base"])
    out = device_runs["no_flex", 20]
    x = torch.from_numpy(b["x"]).cuda()
    n, A, Lg, T = x.shape[0], x.shape[1], len(b["lig_idx"]), len(b["rot"])
    both = np.concatenate([b["intra"], b["intra"][:, ::-1]], 0).astype(np.int64)
    both = both[np.lexsort((both[:, 1], both[:, 0]))]
    start = np.concatenate([[0], np.cumsum(np.bincount(both[:, 0], minlength=Lg))]).astype(np.int32)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()
    t = [up(b["lig_idx"], np.int32), up(b["types"], np.uint8), up(b["rec_mask"], np.uint8), up(b["lig_active"], np.uint8), up(b["rot"], np.int32),
         up(b["mask"].view(np.int32), np.int32), up(start, np.int32), up(both[:, 1], np.int32)]
    numel = L.pd_vina_refine_workspace_numel(n, Lg, T)
    ws = torch.empty(numel, device="cuda", dtype=torch.float64)
    f64, i32 = (lambda *s: torch.empty(*s, device="cuda", dtype=torch.float64)), (lambda *s: torch.empty(*s, device="cuda", dtype=torch.int32))
    o = dict(x_refined=torch.empty_like(x), energy_start=f64(n), energy=f64(n), iterations=i32(n), evaluations=i32(n), status=i32(n), moved=f64(n))
    assert L.pd_vina_refine(P(x), *[P(v) for v in t], len(b["intra"]), 20, 1e-4, 1.0, P(ws), numel, *[P(v) for v in o.values()], None,
                            n, A, Lg, T, S()) == 0
    torch.cuda.synchronize()
    for k in ("iterations", "evaluations", "status"):
        assert torch.equal(out[k], o[k]), k
    diff, ulp, ok = close_coordinates(out["x_refined"].cpu().double().numpy(), o["x_refined"].cpu().double().numpy())
    assert ok, diff
    for p in range(n):
        y = o["x_refined"][p].cpu().double().numpy()[c["mov_idx"]]
        bound = ref.evaluate(c, c["x"][p].astype(np.float64), y, bounds=True)["bound"]["energy"]
        for k in ("energy", "energy_start"):
            assert abs(float(out[k][p]) - float(o[k][p])) <= bound, (k, p)
    print(f"AGREEMENT | no_flex vs pd_vina_refine | coordinates {diff:.3e} | bit-equal {torch.equal(out['x_refined'], o['x_refined'])} |")
    assert not out["receptor"].any() and not out["moved_flex"].any()


@pytest.mark.parametrize("name,mi", ref.RUNS)
def test_invariants_of_x_refined(cases, device_runs, name, mi):
    c, out = cases[name], device_runs[name, mi]
    x = torch.from_numpy(c["x"]).cuda()
    A = x.shape[1]
    rest = torch.from_numpy(np.setdiff1d(np.arange(A), c["mov_idx"])).cuda()
    assert torch.equal(out["x_refined"][:, rest], x[:, rest]), "a fixed row changed"
    if c["F"]:                                                                       # the anchors never move either
        ca = torch.from_numpy(np.asarray([c["mov_idx"][r[0]] for r in c["residue_rows"]], dtype=np.int64)).cuda()
        assert torch.equal(out["x_refined"][:, ca], x[:, ca])
    adj = np.zeros((A, A), dtype=bool)
    lig = c["lig_idx"].astype(np.int64)
    for i, j in c["bonds"]:
        adj[lig[i], lig[j]] = adj[lig[j], lig[i]] = True
    keep = adj.copy()                                                                # ligand: bonded distances
    rec = np.zeros((A, A), dtype=bool)
    for i, j in c["rec_bonds"]:
        rec[i, j] = rec[j, i] = True
    keep |= rec | ((rec.astype(int) @ rec.astype(int)) > 0)                           # receptor: bonds and 1-3
    np.fill_diagonal(keep, False)
    x0, x1 = c["x"].astype(np.float64), out["x_refined"].cpu().double().numpy()
    d0 = np.sqrt(((x0[:, :, None] - x0[:, None]) ** 2).sum(-1))
    d1 = np.sqrt(((x1[:, :, None] - x1[:, None]) ** 2).sum(-1))
    tol = 2.0 * float(np.spacing(np.float32(max(np.abs(x0).max(), np.abs(x1).max()))))
    worst = np.abs(d1 - d0)[:, keep].max()
    assert worst <= tol, (name, worst, tol)
    assert float(out["moved"].max()) > 0.05 and (float(out["moved_flex"].max()) > 1e-3) == (c["S"] > 0)


@pytest.mark.parametrize("name", ["small", "over_block"])
def test_determinism(L, cases, device_runs, name):
    c = cases[name]
    mi = [m for n_, m in ref.RUNS if n_ == name][0]
    out = device_runs[name, mi]
    d = tables(c)
    assert same(launch_refine(L, c["x"], c, d, max_iters=mi), out)                    # two launches
    rev = launch_refine(L, c["x"][::-1], c, d, max_iters=mi)
    assert all(torch.equal(rev[k].flip(0), out[k]) for k in out), name
    for p in range(c["x"].shape[0]):
        one = launch_refine(L, c["x"][p:p + 1], c, d, max_iters=mi)
        assert all(torch.equal(one[k][0], out[k][p]) for k in out), (name, p)
    bare = launch_refine(L, c["x"], c, d, max_iters=mi, trace=False)                  # the trace is optional
    assert "energy_trace" not in bare and all(torch.equal(bare[k], out[k]) for k in bare)


def test_a_non_finite_coordinate_terminates_as_the_reference_says(L, cases):
    c = cases["small"]
    Lg = c["L"]
    for row in (3, Lg + 2):                                                          # a ligand row; a side-chain row of a moving set
        x = c["x"][:2].copy()
        x[0, c["mov_idx"][row]] = np.nan
        want = ref.refine(c, x[0].astype(np.float64), max_iters=5)
        assert (want["status"], want["iterations"], want["evaluations"]) == (2, 0, 1)
        out = launch_refine(L, x, c, max_iters=5, finite=False)
        assert (int(out["status"][0]), int(out["iterations"][0]), int(out["evaluations"][0])) == (2, 0, 1)
        xd = torch.from_numpy(x).cuda()
        assert torch.equal(torch.nan_to_num(out["x_refined"][0], nan=7.0), torch.nan_to_num(xd[0], nan=7.0))      # returned as it came
        far = x[0].astype(np.float64)                                                # the same pairs, the atom out of everyone's range: a finite bound
        far[c["mov_idx"][row]] = 1e4
        twin = ref.evaluate(c, far, far[c["mov_idx"]], bounds=True)
        assert twin["energy"] == want["energy"]
        assert abs(float(out["energy"][0]) - want["energy"]) <= twin["bound"]["energy"] and torch.equal(out["energy"][0], out["energy_start"][0])
        assert bool(torch.isnan(out["moved"][0])) == bool(np.isnan(want["moved"]))
        clean = ref.refine(c, x[1].astype(np.float64), max_iters=5)                   # the pose beside it is untouched by it
        assert (int(out["status"][1]), int(out["iterations"][1]), int(out["evaluations"][1])) == (clean["status"], clean["iterations"], clean["evaluations"])


def test_error_codes(L, cases):
    c = cases["small"]
    d = tables(c)
    x = torch.from_numpy(c["x"]).cuda()
    n, A, Lg, F, T, S_ = sizes(c, 3)
    M = Lg + F
    numel = L.pd_vina_flex_workspace_numel(n, M, T + S_)
    i32 = torch.int32
    ws = sentinel(numel)
    bufs = [sentinel(n, A, 3, dtype=torch.float32)] + [sentinel(n) for _ in range(5)] + [sentinel(n, dtype=i32) for _ in range(3)] + \
        [sentinel(n), sentinel(n), sentinel(n, 4)]
    h = head(x, d)

    def call(h=h, mi=3, gt=1e-4, ms=1.0, ws_=P(ws), wn=numel, outs=None, sz=(n, A, Lg, F, T, S_)):
        outs = [P(b) for b in bufs] if outs is None else outs
        return L.pd_vina_flex_refine(*h, mi, gt, ms, ws_, wn, *outs, *sz, S())

    rcs = {}
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11):                                       # x .. excl_atom
        hh = list(h)
        hh[k] = None
        rcs[f"null table {k}"] = call(h=hh)
    for k in (0, 1, 5, 6, 7, 8, 10, 11):                                                # float / int tables off their alignment
        hh = list(h)
        hh[k] = h[k] + 2
        rcs[f"misaligned table {k}"] = call(h=hh)
    for k in (0, 1, 2, 6, 7, 8, 9):                                                     # the required outputs
        outs = [P(b) for b in bufs]
        outs[k] = None
        rcs[f"null output {k}"] = call(outs=outs)
    for k in range(12):
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
    for k in range(3):
        sz = [n, A, Lg, F, T, S_]
        sz[k] = 0
        rcs[f"size {k} = 0"] = call(sz=sz)
    rcs["F<0"], rcs["T<0"], rcs["S<0"] = call(sz=(n, A, Lg, -1, T, S_)), call(sz=(n, A, Lg, F, -1, S_)), call(sz=(n, A, Lg, F, T, -1))
    hh = list(h)
    hh[9] = -1
    rcs["n_pair<0"] = call(h=hh)
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), rcs
    unsupported = {"M": call(sz=(n, A, Lg, 1025 - Lg, T, S_)), "N": call(sz=(n, A, Lg, F, T, 59 - T)), "P": call(sz=(65536, A, Lg, F, T, S_)),
                   "A": call(sz=(n, (1 << 22) + 1, Lg, F, T, S_))}
    assert all(rc == PD_ERR_UNSUPPORTED for rc in unsupported.values()), unsupported
    # the energy entry point: the same table checks
    e = sentinel(n)
    ecall = lambda h=h, e_=P(e), sz=(n, A, Lg, F, T, S_): L.pd_vina_flex_energy(*h, e_, None, None, None, None, None, *sz, S())
    hh = list(h)
    hh[7] = None
    assert ecall(h=hh) == PD_ERR_ARG and ecall(e_=P(e) + 4) == PD_ERR_ARG and ecall(sz=(0, A, Lg, F, T, S_)) == PD_ERR_ARG
    assert ecall(sz=(n, A, Lg, F, T, 59 - T)) == PD_ERR_UNSUPPORTED and ecall(sz=(n, A, Lg, 1025 - Lg, T, S_)) == PD_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(untouched(b) for b in bufs) and untouched(ws) and untouched(e), "a rejected call wrote"
    assert call() == 0
    for b in bufs:
        body(b)
    assert untouched(ws[-1:])


# ------------------------------------------------------------------ FlexRefine
def flex_refine_of(c):
    from physdock_amd import FlexRefine
    return FlexRefine.from_tables(c["types"], c["lig_idx"], c["rec_mask"], c["lig_active"], c["n_rot"], c["rot"][:c["T"]], c["sets"][:c["T"]],
                                  c["intra"], c["rec_bonds"], c["residues"], device="cuda")


def test_python_surface(L, cases, device_runs):
    c = cases["small"]
    f = flex_refine_of(c)
    x = torch.from_numpy(c["x"]).cuda()
    out = f.refine(x, max_iters=12, trace=True)
    raw = device_runs["small", 12]
    assert set(out) == set(raw) | {"residue_moved", "score_start", "score"} and all(t.is_cuda for t in out.values())
    assert all(torch.equal(out[k], raw[k]) for k in raw)
    f64, f32 = torch.float64, torch.float32
    assert out["residue_moved"].shape == (3, 3) and out["residue_moved"].dtype == f64 and out["score"].dtype == f32
    mov = c["mov_idx"].astype(np.int64)
    disp = (out["x_refined"].double() - x.double()).pow(2).sum(-1).sqrt().cpu().numpy()
    assert np.array_equal(out["residue_moved"].cpu().numpy(), np.stack([disp[:, mov[r]].max(1) for r in c["residue_rows"]], 1))
    assert torch.equal(out["score"], f.vina.score(out["x_refined"])["score"]) and torch.equal(out["score_start"], f.vina.score(x)["score"])
    assert "energy_trace" not in f.refine(x, max_iters=3)
    e = f.energy(x, gradients=True)
    assert set(e) == set(ENERGY_KEYS) and all(t.is_cuda and t.dtype == f64 for t in e.values())
    assert e["grad"].shape == (3, 22, 3) and e["ggrad"].shape == (3, 12)
    assert same(e, launch_energy(L, c["x"], c))
    assert set(f.energy(x)) == {"energy", "inter", "intra", "receptor"} and torch.equal(f.energy(x)["energy"], e["energy"])
    with pytest.raises(ValueError, match="pose atoms"):
        f.refine(x[:, :-1])
    none = flex_refine_of(cases["no_flex"])                                            # no flexible residue: VinaRefine.refine
    from physdock_amd import VinaRefine
    b = vrr.make_case(ref.CASES["no_flex"]["base"])
    xb = torch.from_numpy(b["x"]).cuda()
    o0, o1 = none.refine(xb, max_iters=20), VinaRefine.from_vina(none.vina, b["bonds"], device="cuda").refine(xb, max_iters=20)
    assert all(torch.equal(o0[k], o1[k]) for k in ("iterations", "evaluations", "status")) and o0["residue_moved"].shape == (2, 0)
    assert close_coordinates(o0["x_refined"].cpu().double().numpy(), o1["x_refined"].cpu().double().numpy())[2]


def same_result(u, w):
    if isinstance(u, torch.Tensor):
        return isinstance(w, torch.Tensor) and torch.equal(u, w)
    if isinstance(u, dict):
        return isinstance(w, dict) and set(u) == set(w) and all(same_result(u[k], w[k]) for k in u)
    return u == w


def test_redock_reports_the_flexible_refinement_and_changes_nothing_else(small_model_inputs):
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
    flex = FlexRefine.from_refine(refine, res, atoms, rid, protein[:3] + [int(rid[lig][0])], device="cuda")
    assert flex.n_flex_torsions == 3 and flex.n_flex_atoms == 9 and flex.skipped == ((int(rid[lig][0]), "no torsions"),)
    geometry = ReceptorGeometry.from_names(res, atoms, rid, dbatch["x_gt"], n_residues=int(dbatch["is_ligand"].shape[0]), device="cuda")
    validity = PoseValidity.from_batch(dbatch, bonds)
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, dbatch, **kw)
    out = driver.redock(model, dbatch, flex=flex, **kw)
    assert set(out) == set(plain) | {"flex_refined"} and same_result({k: out[k] for k in plain}, plain)
    assert same_result(out["flex_refined"], flex.refine(out["poses"]))
    assert out["flex_refined"]["x_refined"].shape == out["poses"].shape and (out["flex_refined"]["energy"] <= out["flex_refined"]["energy_start"]).all()
    full = driver.redock(model, dbatch, flex=flex, vina=refine.vina, validity=validity, receptor_geometry=geometry, **kw)
    assert {"flex_refined", "order_vina_flex", "vina", "validity", "receptor_geometry"} <= set(full)
    xr = full["flex_refined"]["x_refined"]
    assert same_result(full["flex_refined"]["validity"], validity.check(xr))
    assert same_result(full["flex_refined"]["receptor_geometry"], geometry.check(xr))
    assert torch.equal(full["order_vina_flex"], rank_by_score({"score": full["flex_refined"]["score"]}))
    assert torch.equal(full["poses"], plain["poses"])
    many = driver.redock_many(model, [(dbatch, {"flex": flex})], **kw)
    assert same_result(many[0], out)
    with pytest.raises(ValueError, match="flex= was built over"):
        driver.redock(model, {**dbatch, "x_gt": dbatch["x_gt"][:-1]}, flex=flex, **kw)
