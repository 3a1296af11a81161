"""pd_shape_prepare, pd_shape_overlap and pd_shape_overlay (csrc/shape_overlap.hip) straight on the C ABI, and ShapeOverlap / redock(shape=)
through the Python surface.

The yardstick is the float64 definition tests/shape_overlap_ref.py.  Float64 outputs must satisfy |dev - ref| <= bound element by
element, the bound derived there from float64 roundoff and the operation counts, nothing multiplied on; fp32 scores one fp32 ulp
more.  One `ENVELOPE | pd_shape_overlap | ...` line is printed per output (pytest -s).  The overlay must take the reference's decisions
(cases with asserted margins, tests/shape_overlap_cases.py): equal counts, status and start, fitted coordinates within 1e-6 A plus one
fp32 ulp of the largest coordinate; its overlap is held to the derived bound alone, both against the reference evaluated at the
device's own fitted atoms (`x_fit`) and against the reference's own optimum.  Buffers are one row longer than needed and pre-filled with a sentinel."""
import numpy as np
import pytest
import torch

import shape_overlap_cases as cases
import shape_overlap_ref as ref

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN = float("nan")
I_SENTINEL = -77
KEYS = ("O_AB", "C_AB", "shape_tanimoto", "color_tanimoto", "combo")
F32 = ("shape_tanimoto", "color_tanimoto", "combo")


def sentinel(*shape, dtype=torch.float64):
    fill = 12345.0 if dtype.is_floating_point else I_SENTINEL                          # (NaN is a legitimate output here)
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), fill, device="cuda", dtype=dtype)


def untouched(buf):
    return bool((buf == (12345.0 if buf.dtype.is_floating_point else I_SENTINEL)).all())


def body(buf):
    torch.cuda.synchronize()
    assert untouched(buf[-1]), "the row behind the output was written"
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


def up(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()


class Side:
    """n structures of one molecule, prepared on the device and in the reference"""

    def __init__(self, L, xs, radii, feats):
        self.xs, self.radii, self.feats = np.asarray(xs, dtype=np.float32), np.asarray(radii, dtype=np.float64), feats
        self.n, self.L, self.F = self.xs.shape[0], self.xs.shape[1], len(feats)
        start = np.concatenate([[0], np.cumsum([len(m) for _, m in feats])]).astype(np.int32)
        atom = np.asarray([i for _, m in feats for i in m], dtype=np.int32)
        assert atom.size == 0 or (0 <= atom.min() and atom.max() < self.L)              # every index the kernel follows
        self.alpha, self.kind = up(ref.alphas(radii), np.float64), up([k for k, _ in feats], np.int32)
        self.start, self.atom = up(start, np.int32), up(atom, np.int32)
        self.lig = up(np.arange(self.L), np.int32)
        self.x = up(self.xs, np.float32)
        self.numel = L.pd_shape_workspace_numel(self.n, self.L, self.F)
        assert self.numel == self.n * (3 * (self.L + self.F) + 2)
        self.wsbuf = sentinel(self.numel)
        assert self.prepare(L, P(self.wsbuf), self.numel) == 0
        self.ws = body(self.wsbuf)
        self.ref = [ref.prepare(x, radii, feats) for x in self.xs]

    def prepare(self, L, ws, numel, x=None, n=None, Lg=None, F=None):
        F = self.F if F is None else F
        return L.pd_shape_prepare(P(self.x) if x is None else x, P(self.lig), P(self.alpha), P(self.start) if F else None,
                                  P(self.atom) if F else None, P(self.kind) if F else None, ref.COLOR_ALPHA, ws, numel,
                                  self.n if n is None else n, self.L, self.L if Lg is None else Lg, F, S())

    def args(self):
        return [P(self.ws), self.numel, P(self.alpha), P(self.kind) if self.F else None, self.n, self.L, self.F]


def launch_overlap(L, a, b, pairwise=False, share=False, only=None):
    buf = {k: sentinel(a.n, b.n, dtype=torch.float32 if k in F32 else torch.float64) for k in KEYS if only is None or k in only}
    sh = sentinel(a.n, a.L) if share else None
    rc = L.pd_shape_overlap(*a.args(), *b.args(), ref.COLOR_ALPHA, 1 if pairwise else 0, *(P(buf.get(k)) for k in KEYS), P(sh), S())
    assert rc == 0, rc
    out = {k: body(v) for k, v in buf.items()}
    if share:
        out["atom_share"] = body(sh)
    for v in out.values():
        assert not (v == 12345.0).any(), "an output element kept its sentinel"
    return out


def oracle(a, b, share=False):
    got = [[ref.score(A, B, per_atom=share) for B in b.ref] for A in a.ref]
    want = {k: np.array([[g[k] for g in row] for row in got]) for k in KEYS}
    bound = {k: np.array([[g["bound"][k] for g in row] for row in got]) for k in KEYS}
    if share:
        want["atom_share"] = np.stack([row[0]["atom_share"] for row in got])
        bound["atom_share"] = np.stack([row[0]["bound"]["atom_share"] for row in got])
    return want, bound


def check(case, out, want, bound):
    for k in out:
        dev, r, b = out[k].cpu().double().numpy(), want[k], bound[k]
        assert dev.shape == r.shape, (case, k, dev.shape, r.shape)
        assert (np.isnan(dev) == np.isnan(r)).all(), (case, k)
        if k in F32:
            b = b + np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)       # one fp32 ulp
        err = np.nan_to_num(np.abs(dev - r))
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
        print(f"ENVELOPE | pd_shape_overlap | {case} {k} | {np.nanmax(np.abs(r)):.2e} | {err.max():.2e} | {ratio.max():.3f} |")
        assert (err <= b).all(), (case, k, "err", err.max(), "ratio", ratio.max())


def bits(t):
    """the bit patterns: NaN outputs compare equal to themselves"""
    view = {torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype)
    return t.contiguous().view(view) if view is not None else t


def same(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


def stack(Lg, n, seed, **kw):
    """n structures of one molecule of Lg atoms: seeded rigid motions of it, so that the overlaps with a neighbour are neither 0 nor 1"""
    y, radii, feats = ref.molecule(Lg, seed, **kw)
    xs = np.stack([y] + [cases.rigid(y, 10 * seed + p)[0] for p in range(1, n)])
    return xs, radii, feats


# ------------------------------------------------------------------ the overlap kernel
SHAPES = [(1, 1), (3, 7), (33, 64), (65, 300), (257, 7), (257, 300), (65, 1)]


@pytest.mark.parametrize("Lg,M", SHAPES)
def test_cross_against_float64(L, Lg, M):
    a = Side(L, *stack(Lg, 3, Lg))
    b = Side(L, *stack(M, 18, 1000 + M, n_feats=min(M, 40)))                              # 18 columns: two tiles of 16
    out = launch_overlap(L, a, b)
    check(f"L{Lg}_M{M}", out, *oracle(a, b))
    assert same(launch_overlap(L, a, b), out)                                          # launch to launch
    one = Side(L, a.xs[1:2], a.radii, a.feats)                                         # a row alone, a column alone
    assert all(torch.equal(bits(launch_overlap(L, one, b)[k][0]), bits(out[k][1])) for k in KEYS)
    col = Side(L, b.xs[16:17], b.radii, b.feats)
    alone = launch_overlap(L, a, col, share=True)
    assert all(torch.equal(bits(alone[k][:, 0]), bits(out[k][:, 16])) for k in KEYS)
    want, bound = oracle(a, col, share=True)
    check(f"L{Lg}_M{M} share", {"atom_share": alone["atom_share"]}, want, bound)
    for k in KEYS:                                                                     # every output may be NULL
        assert torch.equal(bits(launch_overlap(L, a, b, only=(k,))[k]), bits(out[k]))
    assert untouched(a.wsbuf[-1:]) and untouched(b.wsbuf[-1:])


def test_no_features_no_shared_kind_ring_and_far_pair(L):
    y, radii, _ = ref.molecule(9, 1)
    bare = Side(L, y[None], radii, [])
    donors = Side(L, y[None], radii, [(0, (0,)), (0, (3,))])
    rings = Side(L, y[None] + np.float32(0.5), radii, [(5, (0, 1, 2, 3, 4, 5)), (1, (2,))])
    far = Side(L, y[None] + np.float32(400.0), radii, [(0, (0,))])
    for name, a, b in (("bare-bare", bare, bare), ("bare-donors", bare, donors), ("no shared kind", donors, rings), ("rings", rings, rings),
                       ("far", donors, far)):
        out = launch_overlap(L, a, b)
        check(name, out, *oracle(a, b))
        if name != "rings":
            assert float(out["C_AB"]) == 0.0 and float(out["color_tanimoto"]) == 0.0
    out = launch_overlap(L, donors, far)
    assert all(float(out[k]) == 0.0 for k in KEYS)                                     # underflow to exact zeros, not NaN
    assert float(launch_overlap(L, rings, rings)["color_tanimoto"]) == 1.0


def test_pairwise_is_symmetric_with_unit_diagonal_and_nan_rows(L):
    xs, radii, feats = stack(33, 19, 7)
    a = Side(L, xs, radii, feats)
    out = launch_overlap(L, a, a, pairwise=True)
    check("pairwise", out, *oracle(a, a))
    for k in KEYS:
        assert torch.equal(bits(out[k]), bits(out[k].T)), k
    assert torch.equal(out["shape_tanimoto"].diagonal(), torch.ones(19, device="cuda"))
    full = launch_overlap(L, a, a)                                                     # the cross form of the same side
    assert torch.equal(bits(torch.triu(out["O_AB"])), bits(torch.triu(full["O_AB"])))
    xs2 = xs.copy()
    xs2[4, 2, 1] = np.inf
    b = Side(L, xs2, radii, feats)
    bad = launch_overlap(L, b, b, pairwise=True)
    keep = torch.ones(19, 19, dtype=torch.bool, device="cuda")
    keep[4], keep[:, 4] = False, False
    for k in KEYS:
        assert torch.isnan(bad[k][4]).all() and torch.isnan(bad[k][:, 4]).all()
        assert torch.equal(bits(bad[k][keep]), bits(out[k][keep])), k
    # per-atom shares follow the same rule: a NaN row is NaN in all its atoms, a NaN reference column (here through an infinite
    # coordinate, whose pair terms underflow to 0) makes every row's shares NaN
    good_col, bad_col = Side(L, xs[7:8], radii, feats), Side(L, xs2[4:5], radii, feats)
    sh, clean = launch_overlap(L, b, good_col, share=True)["atom_share"], launch_overlap(L, a, good_col, share=True)["atom_share"]
    rows = torch.arange(19, device="cuda") != 4
    assert torch.isnan(sh[4]).all() and torch.equal(bits(sh[rows]), bits(clean[rows]))
    assert torch.isnan(launch_overlap(L, a, bad_col, share=True)["atom_share"]).all()
    want, _ = oracle(b, good_col, share=True)
    assert (np.isnan(want["atom_share"]) == torch.isnan(sh).cpu().numpy()).all()


def test_argument_errors_leave_outputs_untouched(L):
    a = Side(L, *stack(5, 2, 1))
    b = Side(L, *stack(6, 3, 2))
    ws = sentinel(a.numel)
    assert a.prepare(L, P(ws), a.numel - 1) == PD_ERR_ARG                               # a short workspace
    assert a.prepare(L, None, a.numel) == PD_ERR_ARG and a.prepare(L, P(ws), a.numel, x=0) == PD_ERR_ARG
    assert a.prepare(L, P(ws), a.numel, n=0) == PD_ERR_ARG and a.prepare(L, P(ws), a.numel, n=65536) == PD_ERR_UNSUPPORTED
    assert a.prepare(L, P(ws), 10 ** 9, Lg=1025) == PD_ERR_UNSUPPORTED and a.prepare(L, P(ws), 10 ** 9, F=1025) == PD_ERR_UNSUPPORTED
    o = sentinel(2, 3)
    f = lambda aa, bb, pw=0, sh=None: L.pd_shape_overlap(*aa, *bb, ref.COLOR_ALPHA, pw, P(o), None, None, None, None, sh, S())
    short = a.args(); short[1] -= 1
    null = a.args(); null[0] = None
    noalpha = b.args(); noalpha[2] = None
    nokind = b.args(); nokind[3] = None
    bigL = a.args(); bigL[5] = 1025
    for args, code in (((short, b.args()), PD_ERR_ARG), ((null, b.args()), PD_ERR_ARG), ((a.args(), noalpha), PD_ERR_ARG),
                       ((a.args(), nokind), PD_ERR_ARG), ((bigL, b.args()), PD_ERR_UNSUPPORTED), ((a.args(), b.args(), 1), PD_ERR_ARG),
                       ((a.args(), b.args(), 0, P(o)), PD_ERR_ARG)):
        assert f(*args) == code, args
    tr, sc, i32 = sentinel(2, 3, 7), sentinel(2, 3, 3, dtype=torch.float32), torch.int32
    ov, os_, ints = sentinel(2, 3), sentinel(2, 3), [sentinel(2, 3, dtype=i32) for _ in range(4)]
    numel = L.pd_shape_overlay_workspace_numel(2, 3, a.L)
    assert L.pd_shape_overlay_workspace_numel(2, 3, 257) == PD_ERR_UNSUPPORTED and L.pd_shape_overlay_workspace_numel(0, 3, 5) == PD_ERR_ARG
    wo = sentinel(numel)
    g = lambda aa, bb, ws=P(wo), n=numel, mi=5, step=1.0, t=P(tr): L.pd_shape_overlay(*aa, *bb, ref.COLOR_ALPHA, mi, 1e-4, step, ws, n, t, None, P(sc),
                                                                                  P(ov), P(os_), *(P(v) for v in ints), S())
    big = a.args(); big[5] = 257
    assert g(a.args(), b.args(), n=numel - 1) == PD_ERR_ARG and g(a.args(), b.args(), ws=None) == PD_ERR_ARG
    assert g(a.args(), b.args(), mi=-1) == PD_ERR_ARG and g(a.args(), b.args(), step=0.0) == PD_ERR_ARG
    assert g(a.args(), b.args(), t=None) == PD_ERR_ARG and g(big, b.args()) == PD_ERR_UNSUPPORTED and g(short, b.args()) == PD_ERR_ARG
    torch.cuda.synchronize()
    assert all(untouched(v) for v in [ws, o, tr, sc, ov, os_, wo] + ints)


# ------------------------------------------------------------------ the overlay
def launch_overlay(L, a, b, max_iters=50, grad_tol=1e-4, max_step=1.0):
    n, C, i32 = a.n, b.n, torch.int32
    numel = L.pd_shape_overlay_workspace_numel(n, C, a.L)
    assert numel == n * C * 5 * (16 + 3 * a.L)
    ws = sentinel(numel)
    buf = dict(transform=sentinel(n, C, 7), x_fit=sentinel(n, C, a.L, 3), scores=sentinel(n, C, 3, dtype=torch.float32), overlap=sentinel(n, C), overlap_start=sentinel(n, C),
               best_start=sentinel(n, C, dtype=i32), iterations=sentinel(n, C, dtype=i32), evaluations=sentinel(n, C, dtype=i32),
               status=sentinel(n, C, dtype=i32))
    rc = L.pd_shape_overlay(*a.args(), *b.args(), ref.COLOR_ALPHA, max_iters, grad_tol, max_step, P(ws), numel, *(P(v) for v in buf.values()), S())
    assert rc == 0, rc
    out = {k: body(v) for k, v in buf.items()}
    assert untouched(ws[-1:]), "the element behind the workspace was written"
    assert all(not (v == (12345.0 if v.dtype.is_floating_point else I_SENTINEL)).any() for v in out.values())
    return out


def fitted(x, tr):
    return ref.apply(x, tr[:4], tr[4:])


@pytest.fixture(scope="module")
def overlay_runs(L):
    runs = {}
    for name in cases.OVERLAY_CASES:
        c = cases.overlay_case(name)
        a, b = Side(L, c["xa"][None], c["ra"], c["fa"]), Side(L, c["xb"][None], c["rb"], c["fb"])
        runs[name] = (c, a, b, ref.overlay(c["A"], c["B"], max_iters=c["max_iters"]), launch_overlay(L, a, b, max_iters=c["max_iters"]))
    return runs


@pytest.mark.parametrize("name", list(cases.OVERLAY_CASES))
def test_overlay_takes_the_reference_decisions(L, overlay_runs, name):
    c, a, b, want, out = overlay_runs[name]
    for k, floor in cases.MARGINS.items():
        assert want["margin"][k] >= floor, (name, k, want["margin"][k])
    for k in ("iterations", "evaluations", "status", "best_start"):
        assert int(out[k]) == want[k], (name, k, int(out[k]), want[k])
    tr = out["transform"][0, 0].cpu().numpy()
    y = fitted(c["xa"], tr)
    tol = 1e-6 + float(np.spacing(np.float32(np.abs(want["y"]).max())))
    print(f"TRAJECTORY | pd_shape_overlay | {name} | {np.abs(y - want['y']).max():.2e} | {tol:.2e} |")
    assert np.abs(y - want["y"]).max() <= tol
    # the overlap against the derived bound alone: the reference's overlap AT THE DEVICE'S OWN fitted atoms (x_fit, float64, the
    # conformation the kernel evaluated last) and that evaluation's bound - nothing added for the path that led there.  The
    # transform must reproduce those atoms to the same tolerance as the reference's.
    x_fit = out["x_fit"][0, 0].cpu().numpy()
    assert np.abs(y - x_fit).max() <= tol and np.abs(x_fit - want["y"]).max() <= tol
    e_fit, _, b_fit = ref.energy(x_fit, c["A"]["alpha"], c["B"]["y"], c["B"]["alpha"])
    err = abs(float(out["overlap"]) + e_fit)
    print(f"ENVELOPE | pd_shape_overlay | {name} overlap | {-e_fit:.2e} | {err:.2e} | {b_fit:.2e} | {err / b_fit:.3f} | vs the reference's own "
          f"optimum {abs(float(out['overlap']) - want['overlap']):.2e} of {want['bound']:.2e}")
    assert err <= b_fit, (name, err, b_fit)
    assert abs(float(out["overlap"]) - want["overlap"]) <= want["bound"]               # and against the reference's own optimum, its bound alone
    assert float(out["overlap"]) >= float(out["overlap_start"])
    assert abs(float(np.sqrt((tr[:4] ** 2).sum())) - 1.0) < 1e-14 and tr[0] >= 0.0
    inplace = launch_overlap(L, a, b)
    assert float(out["overlap_start"]) == pytest.approx(float(inplace["O_AB"]), abs=2 * ref.score(c["A"], c["B"])["bound"]["O_AB"])
    sc = out["scores"][0, 0].cpu().numpy()
    assert sc[0] >= float(inplace["shape_tanimoto"]) - 1e-7                             # never worse than in place (start 4)
    at_fit = ref.score(dict(c["A"], y=x_fit, fp=ref.feature_points(x_fit, c["fa"])[0]), c["B"])    # the scores at those atoms
    for i, k in enumerate(F32):
        tol32 = at_fit["bound"][k] + float(np.spacing(np.float32(abs(at_fit[k]))))      # the bound and one fp32 ulp, as the overlap kernel's
        print(f"ENVELOPE | pd_shape_overlay | {name} {k} | {at_fit[k]:.2e} | {abs(sc[i] - at_fit[k]):.2e} | {tol32:.2e} |")
        assert abs(sc[i] - at_fit[k]) <= tol32, (name, k, sc[i], at_fit[k])
    assert same(launch_overlay(L, a, b, max_iters=c["max_iters"]), out)                # launch to launch


def test_overlay_batch_equals_alone_and_nan(L, overlay_runs):
    c, a, b, want, out = overlay_runs["L6_M9_a"]
    xs = np.stack([c["xa"], cases.rigid(c["xa"], 3)[0], c["xa"]])
    xs[2, 1, 0] = np.nan
    ys = np.stack([c["xb"], cases.rigid(c["xb"], 4)[0]])
    A3, B2 = Side(L, xs, c["ra"], c["fa"]), Side(L, ys, c["rb"], c["fb"])
    got = launch_overlay(L, A3, B2)
    for k in out:
        assert torch.equal(bits(got[k][0, 0]), bits(out[k][0, 0])), k                  # inside a batch: the same bits
    assert torch.isnan(got["overlap"][2]).all() and torch.isnan(got["scores"][2]).all() and (got["status"][2] == 2).all()
    assert torch.isnan(got["x_fit"][2]).all() and torch.isnan(got["transform"][2]).all()
    assert not torch.isnan(got["overlap"][:2]).any() and (got["overlap"][:2] >= got["overlap_start"][:2]).all()


def test_overlay_of_a_moved_copy(L):
    c = cases.overlay_case("L12_M12")
    moved, R, t = cases.rigid(c["xa"], 1)
    a, b = Side(L, c["xa"][None], c["ra"], c["fa"]), Side(L, moved[None], c["ra"], c["fa"])
    out = launch_overlay(L, a, b)
    want = ref.overlay(c["A"], b.ref[0])
    # shape Tanimoto 1 within the bound of the Tanimoto and, the score being fp32, one fp32 ulp of 1
    assert abs(float(out["scores"][0, 0, 0]) - 1.0) <= ref.score(c["A"], c["A"])["bound"]["shape_tanimoto"] + 2.0 ** -23
    assert float(out["scores"][0, 0, 1]) == pytest.approx(1.0, abs=1e-5) and int(out["status"]) == want["status"]
    y = fitted(c["xa"], out["transform"][0, 0].cpu().numpy())
    # grad_tol 1e-4 over a curvature of order |O| / A^2 ~ 10^2: the fit is within 1e-4 A of the copy (fp32 rounding of the copy: 1e-6)
    assert np.abs(y - moved).max() < 1e-4
    Rm = ref.quat_to_matrix(out["transform"][0, 0, :4].cpu().numpy())
    assert np.abs(Rm - R).max() < 1e-4 and np.abs(out["transform"][0, 0, 4:].cpu().numpy() - t).max() < 1e-3


# ------------------------------------------------------------------ the Python surface
def test_python_surface_matches_the_kernels(L):
    from physdock_amd import shape
    xs, radii, feats = stack(12, 4, 3)
    ys, radii2, feats2 = stack(9, 3, 4)
    rng = np.random.default_rng(0)
    A, lig = 20, np.sort(rng.permutation(20)[:12])
    pose = rng.normal(size=(4, A, 3)).astype(np.float32)
    pose[:, lig] = xs
    spec = shape.ShapeSpec.from_tables(12, feats, radii, ligand_idx=lig)
    other = shape.ShapeSpec.from_tables(9, feats2, radii2)
    so = shape.ShapeOverlap(spec)
    x, y = torch.from_numpy(pose).cuda(), torch.from_numpy(ys).cuda()
    a, b = Side(L, xs, radii, feats), Side(L, ys, radii2, feats2)
    raw = launch_overlap(L, a, b)
    got = so.cross(x, other, y)
    assert all(torch.equal(bits(got[k]), bits(raw[k])) for k in KEYS)
    pw = so.pairwise(x)
    assert torch.equal(bits(pw["combo"]), bits(launch_overlap(L, a, a, pairwise=True)["combo"]))
    tr = so.to_reference(x, other, y[1], per_atom=True)
    assert torch.equal(bits(tr["combo"]), bits(raw["combo"][:, 1])) and tr["atom_share"].shape == (4, 12)
    assert torch.allclose(tr["atom_share"].sum(1), tr["O_AB"], rtol=1e-12)
    tv = shape.tversky(got, 0.3)
    assert tv.shape == (4, 3) and torch.allclose(tv, got["O_AB"] / (0.3 * got["O_AA"][:, None] + 0.7 * got["O_BB"][None]))
    ov = so.overlay(x, other, y, max_iters=10)
    assert ov["quat"].shape == (4, 3, 4) and ov["x_fit"].shape == (4, 3, 12, 3) and (ov["overlap"] >= ov["overlap_start"]).all()
    tv1 = shape.tversky(tr, 0.3)                                                       # the vectors of to_reference
    assert tv1.shape == (4,) and torch.equal(bits(tv1), bits(tv[:, 1]))
    moved = shape.apply(x[:, None, torch.from_numpy(lig).cuda()], ov["quat"], ov["t"])   # [4,3,12,3]
    o = ref.score(ref.prepare(moved[1, 2].cpu().numpy(), radii, feats), b.ref[2])
    assert float(ov["overlap"][1, 2]) == pytest.approx(o["O_AB"], rel=1e-9) and float(ov["combo"][1, 2]) == pytest.approx(o["combo"], abs=1e-6)
    with pytest.raises(ValueError):
        so.cross(x[:, :5], other, y)
    with pytest.raises(ValueError):
        so.cross(x, other, y[:, :5])


def test_redock_shape_keyword():
    from physdock_amd import PhysDock, param_shapes, seeded_state_dict, shape, small_config
    from physdock_amd.clustering import PoseClusters
    from physdock_amd.driver import ligand_atom_mask, redock
    from physdock_amd.synthetic import small_batch
    cfg = small_config()
    model = PhysDock(cfg)
    model.load_state_dict(seeded_state_dict(param_shapes(cfg), seed=0), strict=True)
    model = model.to("cuda:0").eval()
    batch = {k: v.to("cuda:0") for k, v in small_batch(0).items()}
    n = int(ligand_atom_mask(batch).sum())
    bonds = [(i, i + 1) for i in range(n - 1)]
    so = shape.ShapeOverlap(shape.ShapeSpec.from_batch(batch, bonds))
    kw = dict(steps=4, seed=5, num_samples_per_round=3, max_samples=3)
    plain = redock(model, batch, **kw)
    got = redock(model, batch, shape=so, clusters=PoseClusters(cutoff=0.5, metric="shape"), **kw)
    assert set(got) - set(plain) == {"shape", "order_shape", "clusters"}
    assert all(torch.equal(bits(v), bits(got[k])) for k, v in plain.items() if isinstance(v, torch.Tensor))
    assert all(torch.equal(bits(v), bits(got["ranking"][k])) for k, v in plain["ranking"].items() if isinstance(v, torch.Tensor))
    sh = got["shape"]
    assert set(sh) == {"shape_tanimoto", "color_tanimoto", "combo", "pairwise"} and sh["combo"].shape == (3,)
    assert torch.equal(got["order_shape"], torch.sort(-sh["combo"], stable=True).indices)
    assert torch.equal(sh["pairwise"]["shape_tanimoto"].diagonal(), torch.ones(3, device="cuda"))
    assert torch.equal(got["clusters"]["dist"], 1.0 - sh["pairwise"]["shape_tanimoto"])
    lig = torch.nonzero(ligand_atom_mask(batch)).flatten()
    other = shape.ShapeSpec.from_tables(n)
    again = redock(model, batch, shape=(so, (other, batch["x_gt"].float()[lig])), **kw)
    assert torch.equal(again["shape"]["shape_tanimoto"], sh["shape_tanimoto"])         # the same atoms and radii named another way


def test_redock_many_validity_order_and_sdf_items():
    from physdock_amd import PhysDock, param_shapes, seeded_state_dict, shape, small_config
    from physdock_amd.driver import ligand_atom_mask, redock, redock_many
    from physdock_amd.ranking import rank_by_score
    from physdock_amd.sdfio import SdfTemplate, parse_sdf
    from physdock_amd.synthetic import small_batch
    from physdock_amd.validity import PoseValidity
    cfg = small_config()
    model = PhysDock(cfg)
    model.load_state_dict(seeded_state_dict(param_shapes(cfg), seed=0), strict=True)
    model = model.to("cuda:0").eval()
    batch = {k: v.to("cuda:0") for k, v in small_batch(0).items()}
    n = int(ligand_atom_mask(batch).sum())
    chain = [(i, i + 1) for i in range(n - 1)]
    so = shape.ShapeOverlap(shape.ShapeSpec.from_batch(batch, chain))
    kw = dict(steps=4, seed=5, num_samples_per_round=4, max_samples=4, validity=PoseValidity.from_batch(batch, chain))
    t = SdfTemplate.from_batch(batch, chain, title="small")
    one = redock(model, batch, shape=so, sdf=t, **kw)
    sh, valid = one["shape"], one["validity"]["valid"]
    # valid poses first, each group by descending combo
    assert torch.equal(one["order_shape"], rank_by_score(-sh["combo"], valid=valid))
    order = one["order_shape"].tolist()
    flags, combo = valid[one["order_shape"]].tolist(), sh["combo"][one["order_shape"]].tolist()
    assert flags == sorted(flags, reverse=True) and sorted(order) == [0, 1, 2, 3]
    assert all(combo[i] >= combo[i + 1] for i in range(3) if flags[i] == flags[i + 1])
    # the SD records carry the two items, as the scores print
    back = parse_sdf("".join(SdfTemplate.split(one["sdf"])))
    assert len(back) == 4
    for p, r in enumerate(back):
        assert float(r["properties"]["shape_tanimoto"]) == pytest.approx(float(sh["shape_tanimoto"][p]), rel=1e-4, abs=1e-6)
        assert float(r["properties"]["tanimoto_combo"]) == pytest.approx(float(sh["combo"][p]), rel=1e-4, abs=1e-6)
    # redock_many: the sequential and the grouped path give what redock gives
    for extra in ({}, {"group": 1}):
        many = redock_many(model, [(batch, {"shape": so, "sdf": t})], **extra, **kw)[0]
        assert set(many) == set(one) and torch.equal(many["poses"], one["poses"]) and torch.equal(many["order_shape"], one["order_shape"])
        assert all(torch.equal(bits(many["shape"][k]), bits(sh[k])) for k in ("shape_tanimoto", "color_tanimoto", "combo"))
        assert torch.equal(bits(many["shape"]["pairwise"]["combo"]), bits(sh["pairwise"]["combo"]))
        assert SdfTemplate.split(many["sdf"]) == SdfTemplate.split(one["sdf"])
