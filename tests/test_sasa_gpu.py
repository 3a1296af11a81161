"""pd_buried_surface (csrc/sasa.hip) straight on the C ABI, BuriedSurface, and the surface keyword of redock / redock_many.

The yardstick is the float64 restatement tests/sasa_ref.py and its acceptance rule (its docstring): every seeded case is closed - no
flag of any point differs between the covering radii moved by -1e-4 A and +1e-4 A (tests/test_sasa_cpu.py asserts it on the CPU; it
is asserted again here) - so the device's integer counts must EQUAL the restatement.  Areas and sums are compared with the float64
value computed from the device's own counts, within the derived rounding bound (nothing multiplied on).  Output buffers are one row
longer than needed and pre-filled with a sentinel (NaN, -7777).

Shapes: A = 70 is no multiple of the 256 atoms of a scan run; n = 96 fills one and a half waves of points (two groups of threads
share the list), n = 257 gives two points per thread and a tail (one group), n = 1 a single lane (four groups); case g puts
LIST + 5 atoms within reach of one atom, spread so that the list is walked twice."""
import numpy as np
import pytest
import torch

import sasa_ref as ref

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN, INT = float("nan"), -7777
CASE_A = "a_P3_A70_L9_n96"
INTS = ("free_points", "buried_points", "interface_residues")
FLOATS = ("per_atom", "residue_buried") + ref.TOTAL_NAMES


# ------------------------------------------------------------------ sentinels, plumbing
def sentinel(shape, dtype):
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), NAN if dtype == torch.float32 else INT, dtype=dtype, device="cuda")


def untouched(buf):
    return bool(torch.isnan(buf).all()) if buf.dtype == torch.float32 else bool((buf == INT).all())


def body(buf):
    torch.cuda.synchronize()
    assert untouched(buf[-1]), "the row behind the output was written"
    head = buf[:-1]
    assert not (torch.isnan(head).any() if buf.dtype == torch.float32 else (head == INT).any()), "an output element kept its sentinel"
    return head


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
    """a case's tables on the device, every index the kernels would follow checked to be inside its array first"""
    A, R, n = c["x"].shape[1], int(c["n_residues"]), int(c["n_points"])
    start, atom = ref.csr(c)
    cls = ref.classes(c)
    lig = np.asarray(c["lig_idx"])
    assert 0 <= lig.min() and lig.max() < A and len(set(lig.tolist())) == len(lig) <= 1024 and len(cls) == A == len(c["radius"])
    assert not (cls[lig] == 1).any() and len(c["polar"]) == len(lig) and 1 <= R <= A and 1 <= n <= 1024
    assert len(start) == R + 1 and start[0] == 0 and (np.diff(start) >= 0).all() and start[-1] == len(atom) <= A
    assert len(atom) == 0 or (0 <= atom.min() and atom.max() < A and len(set(atom.tolist())) == len(atom))
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()
    unit = ref.sphere_points(n).astype(np.float32)
    assert unit.shape == (n, 3)
    return dict(cls=up(cls, np.uint8), radius=up(c["radius"], np.float32), unit=up(unit, np.float32), lig_idx=up(lig, np.int32),
                polar=up(c["polar"], np.uint8), res_start=up(start, np.int32), res_atom=up(atom if len(atom) else [0], np.int32), N=len(atom))


def buffers(n, A, Lg, R):
    return dict(ws_free=sentinel((n, A), torch.int32), free_points=sentinel((n, Lg), torch.int32), buried_points=sentinel((n, A), torch.int32),
                per_atom=sentinel((n, Lg), torch.float32), totals=sentinel((8, n), torch.float32), residue_buried=sentinel((n, R), torch.float32),
                interface_residues=sentinel((n,), torch.int32))


def launch(L, x, c, d=None):
    """one pd_buried_surface call into sentinel buffers -> dict of the outputs as BuriedSurface.measure names them (+ ws_free)"""
    d = d or tables(c)
    x = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    n, A, Lg, R = x.shape[0], x.shape[1], len(c["lig_idx"]), int(c["n_residues"])
    assert A == len(c["radius"]) and x.shape[2] == 3
    b = buffers(n, A, Lg, R)
    rc = L.pd_buried_surface(P(x), P(d["cls"]), P(d["radius"]), P(d["unit"]), P(d["lig_idx"]), P(d["polar"]), P(d["res_start"]), P(d["res_atom"]),
                             float(c["probe"]), P(b["ws_free"]), P(b["free_points"]), P(b["buried_points"]), P(b["per_atom"]), P(b["totals"]),
                             P(b["residue_buried"]), P(b["interface_residues"]), n, A, Lg, R, d["N"], int(c["n_points"]), S())
    assert rc == 0, rc
    out = {k: body(v) for k, v in b.items()}
    totals = out.pop("totals")
    out.update({k: totals[i] for i, k in enumerate(ref.TOTAL_NAMES)})
    return out


def check(case, c, out, want):
    """the device against the restatement: counts exactly, floats against float64 from the device's own counts"""
    lig = np.asarray(c["lig_idx"])
    free, buried = out["free_points"].cpu().numpy(), out["buried_points"].cpu().numpy()
    assert np.array_equal(buried, want["n_buried"]), (case, "buried_points", int((buried != want["n_buried"]).sum()))
    assert np.array_equal(free, want["n_free"][:, lig]), (case, "free_points", int((free != want["n_free"][:, lig]).sum()))
    assert np.array_equal(out["ws_free"].cpu().numpy()[:, ref.classes(c) == 2], want["n_free"][:, ref.classes(c) == 2])
    a = ref.areas(c, free, buried)
    assert np.array_equal(out["interface_residues"].cpu().numpy(), a["interface_residues"]), (case, "interface_residues")
    for k in FLOATS:
        dev, (val, bound) = out[k].cpu().double().numpy(), a[k]
        assert dev.shape == val.shape and np.isfinite(dev).all(), (case, k)
        err = np.abs(dev - val)
        ratio = (err / np.where(bound > 0, bound, 1.0))[bound > 0].max() if (bound > 0).any() else 0.0
        print(f"ENVELOPE | pd_buried_surface | {case} {k} | {np.abs(val).max():.3e} | {err.max():.2e} | {bound.max():.2e} | {ratio:.2f} |")
        assert (err <= bound).all(), (case, k, err.max(), ratio)


def same(a, b, keys=None):
    return all(torch.equal(a[k], b[k]) for k in (keys or a))


# ------------------------------------------------------------------ the seeded cases
@pytest.mark.parametrize("name", list(ref.CASES))
def test_kernel_against_float64(L, name):
    c = ref.make_case(name)
    want = ref.restate(c)
    assert want["open_flags"] == 0, "the case must be closed"
    d = tables(c)
    out = launch(L, c["x"], c, d)
    check(name, c, out, want)
    assert same(launch(L, c["x"], c, d), out), "two runs of one call are bit-identical"
    cls = ref.classes(c)
    assert not out["buried_points"][:, torch.from_numpy(cls == 0).cuda()].any(), "an ignored atom reports 0"
    off = torch.from_numpy(cls[c["lig_idx"]] == 0).cuda()
    assert not out["free_points"][:, off].any() and not out["per_atom"][:, off].any()
    assert bool((out["buried_fraction"] >= 0).all()) and bool((out["buried_fraction"] <= 1).all())


def test_special_atoms(L):
    c = ref.make_case("f_P3_A70_L9_n96_special")
    out = launch(L, c["x"], c)
    n = c["n_points"]
    assert not out["buried_points"][:, ref.F_HOLE].any() and not out["ws_free"][:, ref.F_HOLE].any(), "the atom a_mask removes"
    assert not out["free_points"][:, ref.F_INACTIVE].any() and not out["buried_points"][:, int(c["lig_idx"][ref.F_INACTIVE])].any()
    assert not out["buried_points"][:, ref.F_FAR].any(), "a receptor atom no ligand atom reaches: exactly 0"
    first, second = ref.F_TWIN
    assert bool((out["ws_free"][:, second] == 0).all()), "the twin with the smaller radius lies inside the other's sphere"
    want = ref.restate(c)
    assert np.array_equal(out["ws_free"][:, first].cpu().numpy(), want["n_free"][:, first]) and (want["n_free"][:, first] <= n).all()


def test_enclosed_ligand_atom_and_the_walked_list(L):
    for name in ("d_P3_A70_L1_n96", "g_P1_A530_L1_n96_cluster"):
        c = ref.make_case(name)
        out = launch(L, c["x"], c)
        assert bool((out["free_points"] == c["n_points"]).all()) and bool((out["buried_points"][:, int(c["lig_idx"][0])] == c["n_points"]).all())
        assert bool((out["ligand_bound"] == 0).all()) and bool((out["buried_fraction"] == 1.0).all()) and bool((out["buried_apolar"] + out["buried_polar"] > 0).all())


def test_a_ligand_far_away_buries_nothing(L):
    c = ref.make_case(CASE_A)
    x = c["x"].copy()
    x[1, c["lig_idx"]] += np.float32([30.0, 0.0, 0.0])                # pose 1: the ligand 30 A away; poses 0 and 2 as they were
    want = ref.restate(c, x)
    assert want["open_flags"] == 0 and not want["n_buried"][1].any() and want["n_buried"][0].any() and np.abs(x).max() <= 64
    out = launch(L, x, c)
    check("far ligand", c, out, want)
    assert not out["buried_points"][1].any() and float(out["buried_fraction"][1]) == 0.0 and int(out["interface_residues"][1]) == 0
    assert float(out["ligand_buried"][1]) == 0.0 and float(out["receptor_buried"][1]) == 0.0 and float(out["interface_area"][1]) == 0.0
    assert not out["residue_buried"][1].any() and float(out["ligand_free"][1]) > 0 and float(out["ligand_free"][1]) == float(out["ligand_bound"][1])
    base = launch(L, c["x"], c)
    assert same({k: v[[0, 2]] for k, v in out.items()}, {k: v[[0, 2]] for k, v in base.items()})


def test_an_all_inactive_ligand_has_fraction_zero_and_no_nan(L):
    c = ref.make_case(CASE_A)
    c["lig_active"] = np.zeros_like(c["lig_active"])
    want = ref.restate(c)
    assert want["open_flags"] == 0
    out = launch(L, c["x"], c)
    check("inactive ligand", c, out, want)
    for k in ("ligand_free", "ligand_bound", "ligand_buried", "buried_fraction", "receptor_buried", "interface_area"):
        assert bool((out[k] == 0).all()), k
    assert not out["free_points"].any() and not out["buried_points"].any() and not out["interface_residues"].any()


def test_a_pose_does_not_depend_on_the_batch(L):
    for name in (CASE_A, "b_P3_A70_L9_n257", "e_P3_A70_L9_n96_rim"):
        c = ref.make_case(name)
        d = tables(c)
        five = launch(L, c["x"][[1, 2, 0, 2, 1]], c, d)
        alone = launch(L, c["x"][0:1], c, d)
        assert all(torch.equal(five[k][2], alone[k][0]) for k in five), (name, "the pose at row 2 of 5 is the pose measured alone")
        assert all(torch.equal(five[k][1], five[k][3]) and torch.equal(five[k][0], five[k][4]) for k in five), name


# ------------------------------------------------------------------ argument handling
def test_argument_handling(L):
    c = ref.make_case("d_P3_A70_L1_n96")
    d = tables(c)
    x = torch.from_numpy(c["x"]).cuda()
    n, A, Lg, R, N, npts = 3, 70, 1, int(c["n_residues"]), d["N"], 96
    b = buffers(n, A, Lg, R)
    names = ["x", "cls", "radius", "unit", "lig_idx", "polar", "res_start", "res_atom"] + list(b)
    ptrs = [P(x), P(d["cls"]), P(d["radius"]), P(d["unit"]), P(d["lig_idx"]), P(d["polar"]), P(d["res_start"]), P(d["res_atom"])] + [P(v) for v in b.values()]
    call = lambda p=ptrs, probe=1.4, sizes=(n, A, Lg, R, N, npts): L.pd_buried_surface(*p[:8], probe, *p[8:], *sizes, S())
    rcs = {}
    for k, name in enumerate(names):
        args = list(ptrs)
        args[k] = None
        rcs["null " + name] = call(args)
        if name not in ("cls", "polar"):
            args[k] = ptrs[k] + 2                                      # a float / int pointer off its 4-byte alignment
            rcs["misaligned " + name] = call(args)
    for k, name in enumerate(["P", "A", "L", "R", "N", "n_points"]):
        for v in (0, -1):
            if name == "N" and v == 0:
                continue
            sz = [n, A, Lg, R, N, npts]
            sz[k] = v
            rcs[f"{name}={v}"] = call(sizes=sz)
    rcs["N>A"] = call(sizes=(n, A, Lg, R, A + 1, npts))
    for bad in (-1.0, NAN, float("inf")):
        rcs[f"probe {bad}"] = call(probe=bad)
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), rcs
    unsupported = {"n_points": call(sizes=(n, A, Lg, R, N, 1025)), "L": call(sizes=(n, A, 1025, R, N, npts)),
                   "A": call(sizes=(n, (1 << 22) + 1, Lg, R, N, npts)), "P": call(sizes=(65536, A, Lg, R, N, npts)),
                   "R>A": call(sizes=(n, A, Lg, A + 1, N, npts))}
    assert all(rc == PD_ERR_UNSUPPORTED for rc in unsupported.values()), unsupported
    torch.cuda.synchronize()
    assert all(untouched(v) for v in b.values()), "a rejected call wrote"
    assert call() == 0
    for v in b.values():
        body(v)


# ------------------------------------------------------------------ BuriedSurface, graph capture
def surface_of(c, device="cuda"):
    from physdock_amd.surface import BuriedSurface
    return BuriedSurface.from_arrays(c["elements"], c["lig_idx"], c["receptor_mask"], c["residue_of"], n_residues=c["n_residues"],
                                     a_mask=c["a_mask"], ligand_active=c["lig_active"], probe=c["probe"], n_points=c["n_points"], device=device)


def test_the_class_agrees_with_the_c_abi_and_captures_into_a_graph(L):
    c = ref.make_case("e_P3_A70_L9_n96_rim")
    s = surface_of(c)
    x = torch.from_numpy(c["x"]).cuda()
    raw = launch(L, c["x"], c)
    raw.pop("ws_free")
    out = s.measure(x)
    assert set(out) == set(INTS) | set(FLOATS) and all(t.is_cuda for t in out.values())
    assert all(out[k].dtype == torch.int32 for k in INTS) and all(out[k].dtype == torch.float32 for k in FLOATS)
    assert out["free_points"].shape == (3, 9) and out["buried_points"].shape == (3, 70) and out["residue_buried"].shape == (3, 8)
    assert all(out[k].shape == (3,) and out[k].is_contiguous() for k in ref.TOTAL_NAMES + ("interface_residues",))
    assert same(out, raw)
    assert bool((out["buried_fraction"] > 0.3).all()) and bool((out["buried_fraction"] < 0.8).all()), "the half-exposed ligand"
    row = out["residue_buried"][0].cpu().numpy()
    told = s.describe(out["residue_buried"][0])
    assert [r for r, _ in told] == sorted(np.nonzero(row)[0].tolist(), key=lambda r: (-row[r], r)) and len(told) == int(out["interface_residues"][0])
    with pytest.raises(ValueError, match="pose atoms"):
        s.measure(x[:, :-1])
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    xs = x.clone()
    with torch.cuda.stream(st):
        s.measure(xs)
    st.synchronize()
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        captured = s.measure(xs)
    xs.copy_(x.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(captured[k], out[k].flip(0)) for k in out)


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


def test_redock_reports_the_surface_and_changes_nothing_else(small):
    from physdock_amd import driver
    from physdock_amd.surface import BuriedSurface
    model, dbatch, _ = small
    s = BuriedSurface.from_batch(dbatch)
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, dbatch, **kw)
    out = driver.redock(model, dbatch, surface=s, **kw)
    assert "x_gt" in dbatch and set(out) == set(plain) | {"surface", "surface_gt"}
    assert same_result({k: out[k] for k in plain}, plain)
    assert set(out["surface"]) == set(INTS) | set(FLOATS) and out["surface"]["buried_points"].shape == (4, s.n_pose_atoms)
    assert same(out["surface"], s.measure(out["poses"]))
    assert same(out["surface_gt"], s.measure(dbatch["x_gt"].float()[None])) and out["surface_gt"]["ligand_free"].shape == (1,)
    assert bool(torch.isfinite(out["surface"]["buried_fraction"]).all()) and bool((out["surface"]["ligand_free"] > 0).all())
    many = driver.redock_many(model, [(dbatch, {"surface": s})], **kw)               # one system: the sequential path
    assert same_result(many[0], out)
    grouped = driver.redock_many(model, [(dbatch, {"surface": s})], group=1, **kw)
    assert set(grouped[0]) == set(out) and same(grouped[0]["surface"], s.measure(grouped[0]["poses"]))
    assert same(grouped[0]["surface_gt"], out["surface_gt"])
