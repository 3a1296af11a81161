"""pd_pocket_grid (csrc/pocket.hip) straight on the C ABI, PocketGrid, and the pocket keyword of redock / redock_many.

The yardstick is the float64 restatement tests/pocket_ref.py and its acceptance rule (its docstring): every seeded case is closed - no
solid, inside or near flag differs between the thresholds moved by -1e-9 A and +1e-9 A (tests/test_pocket_cpu.py asserts it on the
CPU; it is asserted again here) - so every integer of the device must EQUAL the restatement.  Floats are compared with the float64
value computed from the device's own counts, within one rounding (volumes) or two (fractions).  Output buffers and the workspace are
one row longer than needed and pre-filled with a sentinel (-7777, 171).

Shapes: n = 9 is odd, below one 32-bit word per row and below one block of eight row-words per slab; n = 16 and n = 33 give several blocks,
n = 33 rows of two words; A = 530 is more than two runs of 256 atoms; case d is a serpentine one point wide (the hard case of label
propagation), case h plants atoms 1e-6 A from a threshold - inside any fp32 guard band, outside the float64 margin."""
import time

import numpy as np
import pytest
import torch

import pocket_ref as ref

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
INT, BYTE = -7777, 171
BYTES = ("ok", "classes", "buried", "truncated", "atom_class", "atom_buried")
INTS = ("counts", "lining_points", "lining_residues")
KEYS = set(BYTES) | set(INTS) | set(ref.VALUE_NAMES) | {"centre"}


# ------------------------------------------------------------------ sentinels, plumbing
def sentinel(shape, dtype):
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), BYTE if dtype == torch.uint8 else INT, dtype=dtype, device="cuda")


def untouched(buf):
    return bool((buf == (BYTE if buf.dtype == torch.uint8 else INT)).all())


def body(buf):
    torch.cuda.synchronize()
    assert untouched(buf[-1]), "the row behind the output was written"
    head = buf[:-1]
    assert not (head == (BYTE if buf.dtype == torch.uint8 else INT)).any(), "an output element kept its sentinel"
    return head


@pytest.fixture(scope="module")
def L():
    from physdock_amd import ops
    return ops._lib.init()


@pytest.fixture(scope="module")
def restated():
    """the seeded cases and their restatements, computed once and left unchanged"""
    memo = {}

    def get(name):
        if name not in memo:
            c = ref.make_case(name)
            memo[name] = (c, ref.restate(c))
        return memo[name]
    return get


def P(t):
    from physdock_amd import ops
    return ops.ptr(t)


def S():
    from physdock_amd import ops
    return ops.stream()


def tables(c):
    """a case's tables on the device, every index the kernels would follow checked to be inside its array first"""
    A, R = c["x"].shape[1], int(c["n_residues"])
    start, atom = ref.csr(c)
    cls = ref.classes(c)
    lig = np.asarray(c["lig_idx"])
    assert 0 <= lig.min() and lig.max() < A and len(set(lig.tolist())) == len(lig) <= 1024 and len(cls) == A == len(c["radius"])
    assert not (cls[lig] == 1).any() and 1 <= R <= 4096 and 8 <= c["n"] <= 48
    assert len(start) == R + 1 and start[0] == 0 and (np.diff(start) >= 0).all() and start[-1] == len(atom) <= A
    assert len(atom) == 0 or (0 <= atom.min() and atom.max() < A and len(set(atom.tolist())) == len(atom))
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()
    return dict(cls=up(cls, np.uint8), radius=up(c["radius"], np.float32), lig_idx=up(lig, np.int32), res_start=up(start, np.int32),
                res_atom=up(atom if len(atom) else [0], np.int32), N=len(atom))


def buffers(L, n_pose, A, Lg, R, n):
    numel = L.pd_pocket_grid_workspace_numel(n_pose, n, A)
    assert numel == n_pose * (2 * n ** 3 + 2 * n * n * ((n + 31) // 32))
    b = dict(centre_used=sentinel((n_pose, 3), torch.float32), ok=sentinel((n_pose,), torch.uint8), classes=sentinel((n_pose, n ** 3), torch.uint8),
             buried=sentinel((n_pose, n ** 3), torch.uint8), counts=sentinel((n_pose, 8), torch.int32), truncated=sentinel((n_pose,), torch.uint8),
             values=sentinel((6, n_pose), torch.float32), atom_class=sentinel((n_pose, Lg), torch.uint8), atom_buried=sentinel((n_pose, Lg), torch.uint8),
             lining_points=sentinel((n_pose, R), torch.int32), lining_residues=sentinel((n_pose,), torch.int32))
    ws = torch.full((numel + 64,), INT, dtype=torch.int32, device="cuda")
    return b, ws, numel


def steps_of(c):
    import ctypes
    return (ctypes.c_int * 7)(*ref.step_table(c["reach"], c["h"]))


def launch(L, x, c, d=None, centre="case"):
    """one pd_pocket_grid call into sentinel buffers -> dict of the outputs as PocketGrid.measure names them"""
    d = d or tables(c)
    x = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    n_pose, A, Lg, R, n = x.shape[0], x.shape[1], len(c["lig_idx"]), int(c["n_residues"]), int(c["n"])
    assert A == len(c["radius"]) and x.shape[2] == 3
    centre = c["centre"] if isinstance(centre, str) else centre
    ctr = None if centre is None else torch.from_numpy(np.asarray(centre, dtype=np.float32)).cuda()
    assert ctr is None or tuple(ctr.shape) in ((3,), (n_pose, 3))
    b, ws, numel = buffers(L, n_pose, A, Lg, R, n)
    rc = L.pd_pocket_grid(P(x), P(d["cls"]), P(d["radius"]), P(d["lig_idx"]), P(d["res_start"]), P(d["res_atom"]), P(ctr),
                          0 if ctr is None or ctr.dim() == 1 else 3, int(c["snap"]), float(c["h"]), n, float(c["probe"]), float(c["lining"]), steps_of(c),
                          int(c["min_enclosed"]), P(ws), numel, *[P(v) for v in b.values()], n_pose, A, Lg, R, d["N"], S())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert untouched(ws[numel:]), "the workspace was written behind its end"
    out = {k: body(v) for k, v in b.items()}
    values = out.pop("values")
    out.update({k: values[i] for i, k in enumerate(ref.VALUE_NAMES)})
    out["centre"] = out.pop("centre_used")
    return out


def grid_of(c, device="cuda", **kw):
    from physdock_amd.pocket import PocketGrid
    args = dict(n_residues=c["n_residues"], a_mask=c["a_mask"], ligand_active=c["lig_active"], h=c["h"], n=c["n"], probe=c["probe"],
                lining=c["lining"], reach=c["reach"], min_enclosed=c["min_enclosed"], snap=c["snap"], device=device)
    args.update(kw)
    if not np.array_equal(c["radius"], ref.radii_of(c["elements"])):
        args["radii"] = {6: float(c["radius"][0])}                   # case d: one radius for its one element
    return PocketGrid.from_arrays(c["elements"], c["lig_idx"], c["receptor_mask"], c["residue_of"], **args)


def check(case, c, out, want):
    """the device against the restatement: every integer exactly, floats against float64 from the device's own integers"""
    for k in BYTES + INTS:
        dev = out[k].cpu().numpy().astype(np.int64)
        assert dev.shape == want[k].shape and np.array_equal(dev, want[k]), (case, k, int((dev != want[k]).sum()))
    centre = out["centre"].cpu().double().numpy()
    assert np.array_equal(centre, want["centre"], equal_nan=True), (case, "centre")
    good = want["ok"] == 1
    vals = ref.values_of(c, out["counts"].cpu().numpy(), out["atom_buried"].cpu().numpy())
    for k in ref.VALUE_NAMES:
        dev, (val, bound) = out[k].cpu().double().numpy(), vals[k]
        assert dev.shape == val.shape and np.isnan(dev[~good]).all() and np.isfinite(dev[good]).all(), (case, k)
        err = np.abs(dev - val)[good]
        print(f"ENVELOPE | pd_pocket_grid | {case} {k} | {np.abs(val[good]).max(initial=0):.3e} | {err.max(initial=0):.2e} | {bound[good].max(initial=0):.2e} |")
        assert (err <= bound[good]).all(), (case, k, err.max())


def same(a, b, keys=None):
    eq = lambda u, w: torch.equal(u, w) if u.dtype != torch.float32 else bool(((u == w) | (torch.isnan(u) & torch.isnan(w))).all())
    return all(a[k].shape == b[k].shape and eq(a[k], b[k]) for k in (keys or a))


# ------------------------------------------------------------------ the seeded cases
@pytest.mark.parametrize("name", list(ref.CASES))
def test_kernel_against_float64(L, restated, name):
    c, want = restated(name)
    assert want["open_flags"] == 0, "the case must be closed"
    d = tables(c)
    out = launch(L, c["x"], c, d)
    check(name, c, out, want)
    assert same(launch(L, c["x"], c, d), out), "two runs of one call are bit-identical"
    g = grid_of(c)
    got = g.measure(torch.from_numpy(c["x"]).cuda(), centre="ligand" if c["centre"] is None else c["centre"])
    assert set(got) == KEYS and all(t.is_cuda for t in got.values()) and same(got, out), "PocketGrid gives what the C ABI gives"
    assert all(got[k].dtype == torch.uint8 for k in BYTES) and all(got[k].dtype == torch.int32 for k in INTS)
    assert all(got[k].shape == (c["x"].shape[0],) and got[k].dtype == torch.float32 for k in ref.VALUE_NAMES)
    lean = g.measure(torch.from_numpy(c["x"]).cuda(), centre="ligand" if c["centre"] is None else c["centre"], maps=False)
    assert set(lean) == KEYS - {"classes", "buried"} and same(lean, out, lean)
    assert np.array_equal(g.lining(got).cpu().numpy(), want["lining_points"] >= 1) and g.lining(got).dtype == torch.bool
    told = g.describe(got, 0)
    row = want["lining_points"][0]
    assert [r for r, _ in told] == sorted(np.nonzero(row)[0].tolist(), key=lambda r: (-row[r], r)) and len(told) == want["lining_residues"][0]


def test_a_winding_tunnel_is_labelled_within_a_time_limit(restated):
    """case d: 77 points in a serpentine one point wide - a labelling that needs a sweep per point would crawl; the union-find needs
    none.  The call is polled, not waited for: a labelling that does not converge fails here after 20 s instead of hanging the suite."""
    c, want = restated("d")
    g = grid_of(c)
    x = torch.from_numpy(c["x"]).cuda()
    g.measure(x, centre=c["centre"])
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    t0 = time.monotonic()
    out = g.measure(x, centre=c["centre"])
    done.record()
    while not done.query():
        assert time.monotonic() - t0 < 20.0, "the labelling did not converge within 20 s"
    assert out["counts"][0].tolist() == want["counts"][0].tolist() and out["counts"][0, 3] == len(ref.tunnel_points()) >= 60
    assert out["counts"][0, 6] == 1 and np.array_equal(out["classes"].cpu().numpy(), want["classes"])


def test_the_planted_structures(L, restated):
    c, want = restated("a")
    out = launch(L, c["x"], c)
    f = out["filled_fraction"]
    assert bool((out["counts"][:, 3] > 0).all()) and bool((f > 0).all()) and bool((f < 1).all()), "a: a site filled in part"
    c, want = restated("b")
    out = launch(L, c["x"], c)
    assert int(out["counts"][0, 6]) >= 2 and int(out["counts"][0, 7]) == 1, "b: two cavities, the ligand in one"
    c, want = restated("e")
    out = launch(L, c["x"], c)
    assert not out["counts"][:, [0, 2, 3, 4, 6, 7]].any() and bool((out["atom_class"] == 1).all()) and bool((out["atom_buried"] == 0).all())
    for k in ref.VALUE_NAMES:
        assert bool((out[k] == 0).all()), (k, "0 and not NaN")
    assert not out["lining_points"].any() and not out["lining_residues"].any() and not out["truncated"].any() and bool((out["ok"] == 1).all())
    c, want = restated("f")
    out = launch(L, c["x"], c)
    assert int(out["truncated"][0]) == 1 and int(out["counts"][0, 3]) > 0, "f: the site reaches a face of the lattice"


def test_special_atoms_and_a_pose_with_a_nan(L, restated):
    c, want = restated("g")
    d = tables(c)
    base = launch(L, c["x"], c, d)
    assert bool((base["atom_class"][:, [ref.G_INACTIVE, ref.G_OUTSIDE]] == 255).all()) and bool((base["atom_buried"][:, [ref.G_INACTIVE, ref.G_OUTSIDE]] == 255).all())
    x = c["x"].copy()
    x[ref.G_NAN[0], ref.G_NAN[1], 1] = np.nan
    bad = ref.restate(c, x)
    assert bad["open_flags"] == 0 and bad["ok"].tolist() == [1, 0, 1]
    out = launch(L, x, c, d)
    check("g with a NaN", c, out, bad)
    p = ref.G_NAN[0]
    assert int(out["ok"][p]) == 0 and not out["counts"][p].any() and int(out["truncated"][p]) == 0 and int(out["lining_residues"][p]) == 0
    assert all(bool((out[k][p] == 255).all()) for k in ("classes", "buried", "atom_class", "atom_buried")) and not out["lining_points"][p].any()
    assert all(bool(torch.isnan(out[k][p]).all()) for k in ref.VALUE_NAMES + ("centre",))
    keep = [q for q in range(3) if q != p]
    assert same({k: v[keep] for k, v in out.items()}, {k: v[keep] for k, v in base.items()}), "the other poses are bit-equal to their values without it"
    x = c["x"].copy()
    x[0, ref.G_HOLE] = np.nan                                        # a NaN in an ignored atom is not looked at
    x[2, c["lig_idx"][ref.G_INACTIVE]] = np.inf
    assert same(launch(L, x, c, d), base)
    x[2, c["lig_idx"][0]] = np.inf                                   # ... in an active ligand atom it is: the centre is not finite either
    out = launch(L, x, c, d)
    assert out["ok"].tolist() == [1, 1, 0] and same({k: v[:2] for k, v in out.items()}, {k: v[:2] for k, v in base.items()})


def test_a_pose_does_not_depend_on_the_batch(L, restated):
    c, want = restated("a")
    d = tables(c)
    base = launch(L, c["x"], c, d)
    for p in range(3):
        alone = launch(L, c["x"][p:p + 1], c, d)
        assert same({k: v[0] for k, v in alone.items()}, {k: v[p] for k, v in base.items()}), ("alone", p)
    flipped = launch(L, c["x"][::-1], c, d)
    assert same({k: v.flip(0) for k, v in flipped.items()}, base), "reversed"
    five = launch(L, c["x"][[1, 2, 0, 2, 1]], c, d)
    assert same({k: v[[2, 0, 1]] for k, v in five.items()}, base) and same({k: v[[3, 4]] for k, v in five.items()}, {k: v[[2, 1]] for k, v in base.items()})


def test_an_explicit_centre_and_no_snap(L, restated):
    c, _ = restated("a")
    ctr = ref.CENTRE + np.array([0.3, 0.2, -0.4])
    for snap in (False, True):
        cc = dict(c, snap=snap)
        want = ref.restate(cc, centre=ctr)
        assert want["open_flags"] == 0
        out = launch(L, c["x"], cc, centre=ctr)
        check(f"centre [3] snap={snap}", cc, out, want)
        assert out["centre"].cpu().tolist() == [np.float32(ctr if not snap else np.rint(ctr)).tolist()] * 3
        assert same(grid_of(cc).measure(torch.from_numpy(c["x"]).cuda(), centre=ctr), out)
    per_pose = np.stack([ctr, ref.CENTRE, ctr + 1.0])
    cc = dict(c, snap=False)
    want = ref.restate(cc, centre=per_pose)
    assert want["open_flags"] == 0
    out = launch(L, c["x"], cc, centre=per_pose)
    check("centre [P,3]", cc, out, want)
    assert same(grid_of(cc).measure(torch.from_numpy(c["x"]).cuda(), centre=torch.from_numpy(per_pose)), out)
    free = dict(c, snap=False)                                       # the ligand's own centre, not snapped
    want = ref.restate(free)
    assert want["open_flags"] == 0
    check("ligand centre, no snap", free, launch(L, c["x"], free), want)


def test_other_reach_threshold_and_probe(L, restated):
    c, base = restated("a")
    cc = dict(c, reach=3.0, min_enclosed=3, probe=ref.F32(1.0))
    want = ref.restate(cc)
    assert want["open_flags"] == 0 and (want["counts"][:, 6] > 1).all() and not np.array_equal(want["counts"], base["counts"])
    out = launch(L, c["x"], cc)
    check("reach 3, min_enclosed 3, probe 1", cc, out, want)
    assert same(grid_of(cc).measure(torch.from_numpy(c["x"]).cuda()), out)


# ------------------------------------------------------------------ argument handling
def test_return_codes(L, restated):
    c, _ = restated("a")
    d = tables(c)
    x = torch.from_numpy(c["x"]).cuda()
    n_pose, A, Lg, R, N, n = 3, 70, 9, int(c["n_residues"]), d["N"], 9
    b, ws, numel = buffers(L, n_pose, A, Lg, R, n)
    ins = [P(x), P(d["cls"]), P(d["radius"]), P(d["lig_idx"]), P(d["res_start"]), P(d["res_atom"])]
    outs = [P(v) for v in b.values()]

    def call(ins=ins, outs=outs, n=n, sizes=(n_pose, A, Lg, R, N), h=1.0, probe=c["probe"], lining=c["lining"], steps=None, min_enclosed=5,
             ws_ptr=P(ws), ws_numel=numel, stride=0):
        return L.pd_pocket_grid(*ins, None, stride, 1, h, n, probe, lining, steps_of(c) if steps is None else steps, min_enclosed, ws_ptr, ws_numel,
                                *outs, *sizes, S())
    import ctypes
    unsupported = {"n=7": call(n=7), "n=49": call(n=49), "L": call(sizes=(n_pose, A, 1025, R, N)), "R": call(sizes=(n_pose, A, Lg, 4097, N)),
                   "P": call(sizes=(65536, A, Lg, R, N)), "edge": call(h=600.0)}
    assert all(rc == PD_ERR_UNSUPPORTED for rc in unsupported.values()), unsupported
    rcs = {}
    for k, name in enumerate(["x", "cls", "radius", "lig_idx", "res_start", "res_atom"]):
        args = list(ins)
        args[k] = None
        rcs["null " + name] = call(ins=args)
        if name != "cls":
            args[k] = ins[k] + 2
            rcs["misaligned " + name] = call(ins=args)
    for k, name in enumerate(b):
        args = list(outs)
        args[k] = None
        rcs["null " + name] = call(outs=args)
    rcs["null ws"] = call(ws_ptr=None)
    rcs["short ws"] = call(ws_numel=numel - 1)
    for k, name in enumerate(["P", "A", "L", "R"]):
        sz = [n_pose, A, Lg, R, N]
        sz[k] = 0
        rcs[f"{name}=0"] = call(sizes=sz)
    rcs["N>A"] = call(sizes=(n_pose, A, Lg, R, A + 1))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rcs[f"h {bad}"] = call(h=bad)
    for bad in (-1.0, float("nan"), float("inf")):
        rcs[f"probe {bad}"], rcs[f"lining {bad}"] = call(probe=bad), call(lining=bad)
    rcs["min_enclosed 8"], rcs["min_enclosed -1"], rcs["stride"] = call(min_enclosed=8), call(min_enclosed=-1), L.pd_pocket_grid(
        *ins, P(x), 2, 1, 1.0, n, c["probe"], c["lining"], steps_of(c), 5, P(ws), numel, *outs, n_pose, A, Lg, R, N, S())
    rcs["steps -1"] = call(steps=(ctypes.c_int * 7)(12, 12, -1, 6, 6, 6, 6))
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), rcs
    torch.cuda.synchronize()
    assert all(untouched(v) for v in b.values()) and untouched(ws), "a rejected call wrote"
    assert call() == 0
    for v in b.values():
        body(v)


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


def test_redock_reports_the_pocket_and_changes_nothing_else(small):
    from physdock_amd import driver
    from physdock_amd.pocket import PocketGrid
    model, dbatch, _ = small
    g = PocketGrid.from_batch(dbatch, n=16)
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, dbatch, **kw)
    out = driver.redock(model, dbatch, pocket=g, **kw)
    assert "x_gt" in dbatch and set(out) == set(plain) | {"pocket", "pocket_gt"}
    assert same_result({k: out[k] for k in plain}, plain), "unchanged key for key"
    assert set(out["pocket"]) == set(driver.POCKET_KEYS) == set(out["pocket_gt"]) and out["pocket"]["counts"].shape == (4, 8)
    assert out["pocket"]["atom_buried"].shape == (4, g.n_atoms) and out["pocket"]["lining_points"].shape == (4, g.n_residues)
    assert same(out["pocket"], g.measure(out["poses"]), driver.POCKET_KEYS)
    direct = g.measure(dbatch["x_gt"].float()[None])
    assert same(out["pocket_gt"], direct, driver.POCKET_KEYS) and out["pocket_gt"]["site_volume"].shape == (1,)
    assert bool((out["pocket"]["ok"] == 1).all()) and bool(torch.isfinite(out["pocket"]["filled_fraction"]).all())
    many = driver.redock_many(model, [(dbatch, {"pocket": g})], **kw)               # one system: the sequential path
    assert same_result(many[0], out)
    grouped = driver.redock_many(model, [(dbatch, {"pocket": g})], group=1, **kw)
    assert set(grouped[0]) == set(out) and same(grouped[0]["pocket"], g.measure(grouped[0]["poses"]), driver.POCKET_KEYS)
    assert same(grouped[0]["pocket_gt"], out["pocket_gt"])
    other = PocketGrid.from_arrays([6] * 8, [1], np.ones(8), [0, 0, 1, 1, 2, 2, 3, 3])
    with pytest.raises(ValueError, match="pocket= was built over 8 pose atoms"):
        driver.redock(model, dbatch, pocket=other, **kw)
