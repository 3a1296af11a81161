"""pd_torsion_prepare, pd_torsion_tfd and pd_torsion_deviation (csrc/torsion.hip) straight on the C ABI, and TorsionFingerprint /
redock(torsions=) / PoseClusters(metric="torsion").

The yardstick is the float64 numpy definition tests/torsion_ref.py, and the tolerance is the rule it carries:

    B = 4 E + (Nq + T + 64) 2^-52 max_t (180 / max_dev_t),   E = the disagreement of the atan2 and the acos form of every angle on that
    input, propagated through the definition;   |D_dev - TFD_ref| <= B + 1 ulp32(TFD_ref)

best_perm: the reference's TFD at the device's row is within B of the reference minimum.  Angles are compared circularly.  One
`ENVELOPE | pd_torsion_tfd | ...` line is printed per comparison (pytest -s): the source of the table in NOTES.md.  Output buffers are
one row too long and pre-filled with sentinels, the workspace is one element too long.  Ligands sit 60 - 100 A from the origin, every
bond angle of a named quadruple lies between 90 and 150 degrees (tests/torsion_cases.py; tests/test_torsion_cpu.py asserts that E is
a few ulp on every case).  The kernel does not need its table to be a group: the kernel cases use random tables, the identity first.
No test passes an index outside a structure.

The column tile TJ of the kernel is 64 (M <= 4), 16 (M <= 16), 4 (M <= 64) or 1, quartered until (TJ + 1) (Q | 1) doubles fit 65280
bytes of LDS; for Q >= 4080 the row's angles stay in global memory.  torsion_cases.KERNEL_CASES holds nb = TJ - 1 and TJ + 1 for each
tile (nb = 1 and 2 for TJ = 1), reached both by M and by the LDS budget; tests/test_torsion_cpu.py checks that the list covers every
axis value the issue names.  Every test here calls the new entry points."""
import math

import numpy as np
import pytest
import torch

import pose_clusters_ref as pcr
import torsion_cases as tc
import torsion_ref as ref

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN = float("nan")


# ------------------------------------------------------------------ sentinels, plumbing
def sentinel(*shape, dtype=torch.float32):
    fill = NAN if dtype.is_floating_point else -7
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")


def is_sentinel(t):
    return torch.isnan(t) if t.dtype.is_floating_point else t == -7


def body(buf):
    torch.cuda.synchronize()
    assert is_sentinel(buf[-1]).all(), "the row behind the output was written"
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


def dev(t):
    return None if t is None else torch.as_tensor(t).cuda().contiguous()


def upload(t):
    """the tables of torsion_cases.tables on the device (the uint16 image as int16 storage)"""
    return dict(quads=dev(t["quads"]), image=dev(np.ascontiguousarray(t["image"]).view(np.int16)), qstart=dev(t["qstart"]), w=dev(t["w"]),
                inv=dev(t["inv"]))


def prepare(L, x, idx, Lg, t, d, M, angles=False, expect=0):
    """one pd_torsion_prepare call -> (ws [n,Q] view of a buffer one element too long, the angles buffer with its tail row)"""
    x, idx = dev(x), dev(idx)
    n, A = x.shape[:2]
    Q, Nq = t["quads"].shape[0], t["image"].shape[0]
    numel = L.pd_torsion_workspace_numel(n, Q)
    assert numel == n * Q
    ws = torch.full((numel + 1,), 12345.0, dtype=torch.float64, device="cuda")
    ang = sentinel(n, Nq) if angles else None
    rc = L.pd_torsion_prepare(P(x), P(idx), P(d["quads"]), P(d["image"]), P(ws), numel, P(ang), n, A, Lg, Q, Nq, M, S())
    assert rc == expect, rc
    torch.cuda.synchronize()
    assert float(ws[-1]) == 12345.0
    return ws[:-1].view(n, Q), ang


def tfd(L, ws_a, ws_b, t, d, M, detail=True, symmetric=False, expect=0):
    na, nb = ws_a.shape[0], (ws_a if symmetric else ws_b).shape[0]
    Q, Nq, T = t["quads"].shape[0], t["image"].shape[0], t["w"].shape[0]
    D, bp = sentinel(na, nb), sentinel(na, nb, dtype=torch.int32)
    rc = L.pd_torsion_tfd(P(ws_a), None if symmetric else P(ws_b), P(d["qstart"]), P(d["w"]), P(d["inv"]), P(d["image"]), P(D),
                          P(bp) if detail else None, na, nb, Q, T, Nq, M, 1 if symmetric else 0, S())
    assert rc == expect, rc
    return D, bp


def run_case(L, c, detail=True):
    t, M = c["tables"], c["perms"].shape[0]
    d = upload(t)
    ws_a, ang = prepare(L, c["xa"], c["idx_a"], c["Lg"], t, d, M, angles=True)
    ws_b, _ = prepare(L, c["xb"], c["idx_b"], c["Lg"], t, d, M)
    D, bp = tfd(L, ws_a, ws_b, t, d, M, detail)
    return D, bp, ang, ws_a, ws_b, d


def check_against_reference(tag, res, D, bp):
    """every element of a rectangular call against the definition; prints one ENVELOPE line (the worst element)"""
    Dh, bph = body(D).cpu().numpy().astype(np.float64), body(bp).cpu().numpy()
    worst = (0.0, 0.0, 0.0, 0.0)
    for i, row in enumerate(res):
        for j, r in enumerate(row):
            assert np.isfinite(Dh[i, j]) and 0 <= bph[i, j] < len(r["per_m"]), (tag, i, j, Dh[i, j], bph[i, j])
            err, bound = abs(Dh[i, j] - r["tfd"]), ref.value_bound(r["B"], r["tfd"])
            if err / bound >= worst[3]:
                worst = (r["E"], err, bound, err / bound)
            assert err <= bound, (tag, i, j, "E", r["E"], "err", err, "bound", bound)
            assert r["per_m"][bph[i, j]] - r["tfd"] <= r["B"], (tag, i, j, "row", bph[i, j], r["row"])
    print(f"ENVELOPE | pd_torsion_tfd | {tag} | {worst[0]:.2e} | {worst[1]:.2e} | {worst[2]:.2e} | {worst[3]:.2f} |")


def circ(a, b):
    d = np.abs(a - b)
    return np.where(d > 180.0, 360.0 - d, d)


# ------------------------------------------------------------------ kernels against float64
@pytest.mark.parametrize("k", range(len(tc.KERNEL_CASES)))
def test_kernel_against_float64(L, k):
    c = tc.kernel_case(k)
    D, bp, ang, ws_a, _, d = run_case(L, c)
    check_against_reference(c["tag"], c["ref"], D, bp)
    # the fp32 angles of the base quadruples, circularly, against the reference's: half an ulp32 of 180 plus float64 noise
    base = [q for e in c["ents"] for q in e["quads"]]
    xa = ref.gather(c["xa"], c["idx_a"], c["Lg"])
    want = np.array([ref.angles(x, base) for x in xa])
    got = body(ang).cpu().numpy().astype(np.float64)
    assert got.shape == want.shape and (circ(got, want) <= 2.0 ** -17 + 1e-10).all(), circ(got, want).max()
    # the workspace holds the same angles in float64, at the base quadruples' own ids
    own = torch.from_numpy(c["tables"]["image"][:, 0].astype(np.int64)).cuda()
    assert (circ(ws_a[:, own].cpu().numpy(), want) <= 1e-10).all()
    # the per-entry deviations at the device's row
    if k in (1, 4, 7):
        ws_ref, _ = prepare(L, c["xb"][:1], c["idx_b"], c["Lg"], c["tables"], d, c["perms"].shape[0])
        rows = body(bp)[:, 0].contiguous()
        T = len(c["ents"])
        out = sentinel(ws_a.shape[0], T)
        t = c["tables"]
        assert L.pd_torsion_deviation(P(ws_a), P(ws_ref), P(rows), P(d["qstart"]), P(d["inv"]), P(d["image"]), P(out), ws_a.shape[0],
                                      t["quads"].shape[0], T, t["image"].shape[0], c["perms"].shape[0], S()) == 0
        got_dev = body(out).cpu().numpy().astype(np.float64)
        amp = ref.amplification(c["ents"])
        for i in range(ws_a.shape[0]):
            r = c["ref"][i][0]
            want_dev = r["dev"][int(rows[i])]
            assert (np.abs(got_dev[i] - want_dev) <= r["B"] * amp + 2.0 ** -24).all(), (i, np.abs(got_dev[i] - want_dev).max())


def test_no_entries_gives_zeros_and_deviation_writes_nothing(L):
    D, bp = sentinel(5, 3), sentinel(5, 3, dtype=torch.int32)
    assert L.pd_torsion_tfd(None, None, None, None, None, None, P(D), P(bp), 5, 3, 0, 0, 0, 1, 0, S()) == 0
    assert (body(D) == 0).all() and (body(bp) == 0).all()
    Ds = sentinel(4, 4)
    assert L.pd_torsion_tfd(None, None, None, None, None, None, P(Ds), None, 4, 4, 0, 0, 0, 3, 1, S()) == 0
    assert (body(Ds) == 0).all()
    out = sentinel(2, 1)
    assert L.pd_torsion_deviation(None, None, None, None, None, None, P(out), 2, 0, 0, 0, 1, S()) == 0
    torch.cuda.synchronize()
    assert is_sentinel(out).all()


def test_one_missing_angle_touches_only_what_names_it(L):
    """a NaN coordinate and a collinear triple: NaN for the pairs whose quadruples name them (under the table row in question), and a
    NaN never wins the minimum"""
    c = dict(tc.block_case(na=3, nb=4, nblocks=6, T=2, M=3, scattered=False, seed=9))
    t = tc.tables(c["ents"], c["w"], c["perms"])
    named_0 = sorted({int(q[0]) // 4 for q in t["quads"][t["image"][:, 0]]})          # blocks the rows read (m = 0)
    free = [b for b in range(6) if b not in {int(q[0]) // 4 for q in t["quads"]}]
    xa, xb = c["xa"].copy(), c["xb"].copy()
    xa[1, 4 * named_0[0] + 2, 0] = np.nan                                              # row 1 loses a base angle: NaN whatever m
    for s_, step in enumerate(([0, 0, 0], [1, 0.5, 0.25], [2, 1, 0.5])):                 # column 2: an exactly collinear triple in a block m = 0 reads
        xb[2, 4 * named_0[0] + s_] = np.float32([64, 32, 16]) + np.float32(step)
    if free:
        xb[0, 4 * free[0]] = np.nan                                                    # an atom no quadruple names
    c.update(xa=xa, xb=xb, tables=t)
    res = ref.cross(xa, None, xb, None, c["ents"], c["w"], c["perms"], c["Lg"])
    D, bp, *_ = run_case(L, c)
    Dh, bph = body(D).cpu().numpy(), body(bp).cpu().numpy()
    want = ref.field(res, "tfd")
    assert np.isnan(want[1]).all() and np.isfinite(want[[0, 2]][:, [0, 1, 3]]).all() and np.isnan(res[0][2]["per_m"][0])
    assert np.array_equal(np.isnan(Dh), np.isnan(want)) and np.array_equal(bph < 0, np.isnan(want))
    for i in range(3):
        for j in range(4):
            r = res[i][j]
            if np.isfinite(r["tfd"]):
                assert abs(Dh[i, j] - r["tfd"]) <= ref.value_bound(r["B"], r["tfd"]) and np.isfinite(r["per_m"][bph[i, j]])
    # symmetric mode: a NaN row has a NaN diagonal, a finite row an exact zero
    d = upload(t)
    ws, _ = prepare(L, xa, None, c["Lg"], t, d, 3)
    Ds = body(tfd(L, ws, None, t, d, 3, detail=False, symmetric=True)[0]).cpu().numpy()
    want_s, _ = ref.pairwise(xa, None, c["ents"], c["w"], c["perms"], c["Lg"])
    assert np.array_equal(np.isnan(Ds), np.isnan(want_s)) and np.isnan(Ds[1, 1]) and np.isnan(Ds[1, 2]) and np.isnan(Ds[2, 1])
    assert Ds[0, 0] == 0 and Ds[2, 2] == 0 and np.isfinite(Ds[0, 2])          # (pose 1 as a COLUMN is NaN only through the rows that read its gap)


def test_best_perm_is_the_smallest_row_of_the_minimum(L):
    """rows 2 and 5 of the table are the same permutation and give the minimum: row 2 wins"""
    c = dict(tc.block_case(na=2, nb=3, nblocks=8, T=3, M=7, scattered=True, seed=4))
    perms = c["perms"].copy()
    perms[5] = perms[2]
    # plant the minimum: column j of side b becomes row structure 0 seen through perms[2]^-1, so that TFD(x_0, y_j o perms[2]) = 0
    lig_a = ref.gather(c["xa"], c["idx_a"], c["Lg"])[0]
    inv = np.argsort(perms[2])
    xb = c["xb"].copy()
    xb[1, c["idx_b"]] = lig_a[inv].astype(np.float32)
    c.update(perms=perms, xb=xb, tables=tc.tables(c["ents"], c["w"], perms))
    D, bp, *_ = run_case(L, c)
    res = ref.cross(c["xa"], c["idx_a"], xb, c["idx_b"], c["ents"], c["w"], perms, c["Lg"])
    assert res[0][1]["row"] == 2 and res[0][1]["tfd"] == 0.0
    assert int(body(bp)[0, 1]) == 2 and float(body(D)[0, 1]) <= 1e-12          # (the device may read a quadruple back to front)
    check_against_reference("planted rows 2 = 5", res, D, bp)


@pytest.mark.parametrize("k", [1, 3, 5, 7])
def test_symmetric_mode(L, k):
    """bit-equal to the rectangular call on (x, x) on the upper triangle (the same (row, column, m) work items), mirrored, with an
    exact zero diagonal"""
    c = tc.kernel_case(k)
    t, M = c["tables"], c["perms"].shape[0]
    d = upload(t)
    x = c["xb"][:min(6, c["xb"].shape[0])] if c["xb"].shape[0] >= 3 else np.concatenate([c["xb"], c["xb"][::-1] + np.float32(0.25)])
    ws, _ = prepare(L, x, c["idx_b"], c["Lg"], t, d, M)
    n = ws.shape[0]
    Ds = body(tfd(L, ws, None, t, d, M, detail=False, symmetric=True)[0])
    Dr = body(tfd(L, ws, ws, t, d, M, detail=False)[0])
    iu = torch.triu_indices(n, n, 1)
    assert torch.equal(Ds[iu[0], iu[1]].view(torch.int32), Dr[iu[0], iu[1]].view(torch.int32))
    assert torch.equal(Ds, Ds.T) and (torch.diagonal(Ds) == 0).all() and not torch.isnan(Ds).any() and n >= 2
    want, B = ref.pairwise(x, c["idx_b"], c["ents"], c["w"], c["perms"], c["Lg"])
    got = Ds.cpu().numpy().astype(np.float64)
    assert all(abs(got[i, j] - want[i, j]) <= ref.value_bound(B[i, j], want[i, j]) for i in range(n) for j in range(n))


def test_a_value_does_not_depend_on_the_batch(L):
    c = tc.kernel_case(1)
    t, M = c["tables"], 3
    d = upload(t)
    ws_b, _ = prepare(L, c["xb"][:7], c["idx_b"], c["Lg"], t, d, M)
    ws_5, a5 = prepare(L, c["xa"], c["idx_a"], c["Lg"], t, d, M, angles=True)
    D5, bp5 = (body(b) for b in tfd(L, ws_5, ws_b, t, d, M))
    for i in (0, 3):
        ws_1, a1 = prepare(L, c["xa"][i:i + 1], c["idx_a"], c["Lg"], t, d, M, angles=True)
        D1, bp1 = (body(b) for b in tfd(L, ws_1, ws_b[2:5].contiguous(), t, d, M))
        assert torch.equal(ws_1.view(torch.int64), ws_5[i:i + 1].view(torch.int64)) and torch.equal(body(a1), body(a5)[i:i + 1])
        assert torch.equal(D1.view(torch.int32), D5[i:i + 1, 2:5].view(torch.int32)) and torch.equal(bp1, bp5[i:i + 1, 2:5])


def test_argument_handling(L):
    c = tc.kernel_case(3)
    t, M = c["tables"], c["perms"].shape[0]
    d = upload(t)
    Q, Nq, T, Lg = t["quads"].shape[0], t["image"].shape[0], len(c["ents"]), c["Lg"]
    x, idx = dev(c["xa"]), dev(c["idx_a"])
    n, A = x.shape[:2]
    assert L.pd_torsion_workspace_numel(0, 4) == PD_ERR_ARG and L.pd_torsion_workspace_numel(4, 0) == PD_ERR_ARG
    assert L.pd_torsion_workspace_numel(65536, 4) == PD_ERR_UNSUPPORTED and L.pd_torsion_workspace_numel(4, 4097) == PD_ERR_UNSUPPORTED
    assert L.pd_torsion_workspace_numel(65535, 4096) == 65535 * 4096
    ws = torch.full((n * Q + 1,), 12345.0, dtype=torch.float64, device="cuda")
    ang = sentinel(n, Nq)

    def prep(x_=x, idx_=idx, quads=d["quads"], image=d["image"], ws_=ws, numel=n * Q, ang_=ang, n_=n, A_=A, L_=Lg, Q_=Q, Nq_=Nq, M_=M):
        return L.pd_torsion_prepare(P(x_), P(idx_), P(quads), P(image), P(ws_), numel, P(ang_), n_, A_, L_, Q_, Nq_, M_, S())

    for kw in (dict(x_=None), dict(quads=None), dict(ws_=None), dict(image=None), dict(numel=n * Q - 1), dict(n_=0), dict(A_=0), dict(L_=0),
               dict(Q_=0), dict(M_=0), dict(idx_=None, A_=Lg - 1), dict(ws_=ws[1:].view(torch.uint8)[4:]), dict(Nq_=0)):
        assert prep(**kw) == PD_ERR_ARG, kw
    for kw in (dict(L_=1025), dict(Q_=4097, numel=n * 4097), dict(M_=65536), dict(n_=65536, numel=65536 * Q), dict(Nq_=9217)):
        assert prep(**kw) == PD_ERR_UNSUPPORTED, kw
    torch.cuda.synchronize()
    assert (ws == 12345.0).all() and is_sentinel(ang).all()
    assert prep() == 0
    wsv = ws[:-1].view(n, Q)
    D, bp, out = sentinel(n, n), sentinel(n, n, dtype=torch.int32), sentinel(n, T)

    def call(a=wsv, b=wsv, qstart=d["qstart"], w=d["w"], inv=d["inv"], image=d["image"], D_=D, bp_=bp, na=n, nb=n, Q_=Q, T_=T, Nq_=Nq, M_=M,
             sym=0):
        return L.pd_torsion_tfd(P(a), P(b), P(qstart), P(w), P(inv), P(image), P(D_), P(bp_), na, nb, Q_, T_, Nq_, M_, sym, S())

    for kw in (dict(a=None), dict(b=None), dict(qstart=None), dict(w=None), dict(inv=None), dict(image=None), dict(D_=None), dict(na=0),
               dict(nb=0), dict(Q_=0), dict(T_=-1), dict(Nq_=0), dict(M_=0), dict(sym=1), dict(sym=1, bp_=None, nb=n + 1),
               dict(sym=1, bp_=None, b=wsv[1:]), dict(D_=D.view(-1).view(torch.uint8)[2:])):
        assert call(**kw) == PD_ERR_ARG, kw
    for kw in (dict(Q_=4097), dict(T_=1025), dict(Nq_=9217), dict(M_=65536), dict(na=65536), dict(nb=65536)):
        assert call(**kw) == PD_ERR_UNSUPPORTED, kw
    rows = torch.zeros(n, dtype=torch.int32, device="cuda")

    def devi(a=wsv, r=wsv[:1], rows_=rows, qstart=d["qstart"], inv=d["inv"], image=d["image"], out_=out, na=n, Q_=Q, T_=T, Nq_=Nq, M_=M):
        return L.pd_torsion_deviation(P(a), P(r), P(rows_), P(qstart), P(inv), P(image), P(out_), na, Q_, T_, Nq_, M_, S())

    for kw in (dict(a=None), dict(r=None), dict(qstart=None), dict(inv=None), dict(image=None), dict(out_=None), dict(na=0), dict(Q_=0),
               dict(T_=-1), dict(Nq_=0), dict(M_=0)):
        assert devi(**kw) == PD_ERR_ARG, kw
    for kw in (dict(Q_=4097), dict(T_=1025), dict(Nq_=9217), dict(M_=65536), dict(na=65536)):
        assert devi(**kw) == PD_ERR_UNSUPPORTED, kw
    torch.cuda.synchronize()
    assert is_sentinel(D).all() and is_sentinel(bp).all() and is_sentinel(out).all()
    assert call(sym=1, bp_=None, b=None) == 0 and devi(rows_=None) == 0
    # a table row outside 0 .. M-1 (the -1 of best_perm) gives NaN deviations
    rows[1] = -1
    assert devi() == 0
    got = body(out)
    assert torch.isnan(got[1]).all() and not torch.isnan(got[[0]]).any()


# ------------------------------------------------------------------ the host API
@pytest.fixture(scope="module")
def host_case():
    from physdock_amd.symmetry import LigandSymmetry
    from physdock_amd.torsions import TorsionFingerprint
    mol, _ = tc.biphenyl(40.0)
    rng = np.random.default_rng(8)
    A = 14 + 9
    idx = rng.permutation(A)[:14].astype(np.int64)
    x = (rng.standard_normal((6, A, 3)) * 3 + 70).astype(np.float32)
    for i, psi in enumerate((40.0, 220.0, 75.0, 130.0, -20.0, 40.0)):
        x[i, idx] = tc.moved(tc.biphenyl(psi)[1], seed=i)
    sym = LigandSymmetry.from_bonds(14, mol["bonds"], mol["elements"], mol["orders"])
    spec = TorsionFingerprint.from_bonds(14, mol["bonds"], mol["orders"], ligand_idx=idx, symmetry=sym)
    ents = ref.entries(14, mol["bonds"], mol["orders"])
    return spec, sym, x, idx, ents, ref.weights(14, mol["bonds"], ents)


def test_cross_to_reference_and_pairwise(host_case):
    spec, sym, x, idx, ents, w = host_case
    xd = dev(x)
    targets = xd[[1, 3, 0, 3]]                                   # columns 1 and 3 are the same structure: the smaller index wins
    got = spec.cross(xd, targets, detail=True)
    res = ref.cross(x, idx, x[[1, 3, 0, 3]], idx, ents, w, sym.perms, 14)
    Dh = got["D"].cpu().numpy().astype(np.float64)
    assert all(abs(Dh[i, j] - res[i][j]["tfd"]) <= ref.value_bound(res[i][j]["B"], res[i][j]["tfd"]) for i in range(6) for j in range(4))
    key = np.where(np.isnan(Dh), np.inf, Dh)
    assert got["nearest"].tolist() == [int(np.argmin(r)) for r in key] and got["nearest"].dtype == torch.int64
    assert int(got["nearest"][3]) == 1 and float(got["nearest_tfd"][3]) == 0.0
    assert torch.equal(got["nearest_tfd"], got["D"].gather(1, got["nearest"][:, None])[:, 0]) and got["best_perm"].shape == (6, 4)
    # the ring flip (poses 0 and 1) is no difference with the table, the whole difference without
    from physdock_amd.torsions import TorsionFingerprint
    mol = tc.biphenyl(0.0)[0]
    bare = TorsionFingerprint.from_bonds(14, mol["bonds"], mol["orders"], ligand_idx=idx)
    assert float(got["D"][0, 0]) < 5e-5 and int(got["best_perm"][0, 0]) > 0 and float(bare.cross(xd, targets)["D"][0, 0]) > 0.3
    # targets given as the ligand alone, and from the host
    lig_only = spec.cross(xd, targets[:, torch.from_numpy(idx).cuda()].cpu())
    assert torch.equal(lig_only["D"], got["D"])
    with pytest.raises(ValueError, match="on the GPU of the poses"):          # targets on a device that is neither the poses' nor the host
        spec.cross(xd, torch.zeros(1, 23, 3, device="meta"))
    # a NaN pose: -1 and NaN for its row, and it never wins as a target
    x2 = xd.clone()
    x2[2, int(idx[0]), 1] = NAN
    nan = spec.cross(x2, x2[[2, 0]])
    assert int(nan["nearest"][2]) == -1 and math.isnan(float(nan["nearest_tfd"][2])) and nan["nearest"][[0, 1, 3, 4, 5]].tolist() == [1] * 5
    # to_reference = cross with one target, plus the per-entry deviations
    to = spec.to_reference(xd, xd[2])
    one = spec.cross(xd, xd[2:3], detail=True)
    assert torch.equal(to["tfd"], one["D"][:, 0]) and torch.equal(to["best_perm"], one["best_perm"][:, 0])
    assert to["deviation"].shape == (6, 3) and to["deviation"].dtype == torch.float32 and [to["worst_entry"].tolist()[i] for i in (0, 1, 3, 4, 5)] == [0] * 5
    devs = to["deviation"].cpu().numpy().astype(np.float64)
    for i in range(6):
        r = ref.tfd(x[i, idx], x[2, idx], ents, w, sym.perms)
        assert (np.abs(devs[i] - r["dev"][int(to["best_perm"][i])]) <= r["B"] * ref.amplification(ents) + 2.0 ** -24).all()
    assert "ring" in spec.describe(to["deviation"][0]) and spec.describe(to["deviation"][0]).splitlines()[1].split()[1] == "bond"
    # angles: fp32 degrees of every base quadruple, one representative per rotatable bond
    ang = spec.angles(xd)
    base = [q for e in ents for q in e["quads"]]
    want = np.array([ref.angles(p[idx], base) for p in x])
    assert ang.shape == (6, 16) and (circ(ang.cpu().numpy().astype(np.float64), want) <= 2.0 ** -17 + 1e-10).all()
    assert torch.equal(spec.entry_angles(xd), ang[:, :1])
    # pairwise: symmetric, zero diagonal, the definition, and what PoseClusters.cluster takes
    from physdock_amd.clustering import PoseClusters
    Dp = spec.pairwise(xd)
    Dref, Bp = ref.pairwise(x, idx, ents, w, sym.perms, 14)
    assert torch.equal(Dp, Dp.T) and (torch.diagonal(Dp) == 0).all()
    assert all(abs(float(Dp[i, j]) - Dref[i, j]) <= ref.value_bound(Bp[i, j], Dref[i, j]) for i in range(6) for j in range(6))
    modes = PoseClusters(cutoff=0.05, metric="torsion").cluster(Dp)
    want_modes = pcr.restate(Dp.cpu().numpy(), np.arange(6), 0.05)
    assert modes["labels"].tolist() == want_modes["labels"].tolist() and int(modes["labels"][1]) == 0 and int(modes["labels"][5]) == 0
    # no entries: zeros everywhere
    empty = TorsionFingerprint.from_bonds(14, [(0, 1)], ligand_idx=idx)
    assert (empty.pairwise(xd) == 0).all() and empty.angles(xd).shape == (6, 0) and empty.to_reference(xd, xd[0])["worst_entry"].tolist() == [-1] * 6


def test_amide_flip_is_the_worst_entry_on_the_device():
    from physdock_amd.torsions import TorsionFingerprint
    mol, trans = tc.amide_ligand(180.0)
    spec = TorsionFingerprint.from_bonds(25, mol["bonds"], mol["orders"])
    x = dev(np.stack([tc.moved(tc.amide_ligand(0.0)[1], 1), tc.moved(trans, 2)]))
    to = spec.to_reference(x, dev(tc.moved(trans, 3)))
    amide = [t for t, e in enumerate(spec.entries) if e.atoms == (11, 12)][0]
    assert to["worst_entry"].tolist()[0] == amide and abs(float(to["deviation"][0, amide]) - 1.0) < 5e-5
    assert float(to["tfd"][1]) < 5e-4 and float(to["tfd"][0]) > 10 * float(to["tfd"][1])
    assert spec.describe(to["deviation"][0]).splitlines()[1].split()[0] == str(amide)


def test_redock_reports_torsions_and_changes_nothing_else(small_model_inputs):
    from physdock_amd import PhysDock, TorsionFingerprint, driver
    from physdock_amd.clustering import PoseClusters
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.sdfio import SdfTemplate, parse_sdf
    cfg, P_, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P_, strict=True)
    model, dbatch = model.cuda().eval(), {k: v.cuda() for k, v in batch.items()}
    n_lig = int(ligand_atom_mask(dbatch).sum())
    chain = [(i, i + 1) for i in range(n_lig - 1)]
    spec = TorsionFingerprint.from_batch(dbatch, chain)
    assert spec.n_entries == max(0, n_lig - 3)
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, dbatch, **kw)
    out = driver.redock(model, dbatch, torsions=spec, **kw)
    assert set(out) == set(plain) | {"torsions"}
    assert torch.equal(out["poses"], plain["poses"]) and out["rounds"] == plain["rounds"] and out["accepted"] == plain["accepted"]
    assert all(torch.equal(out["ranking"][k], plain["ranking"][k]) for k in ("x_aligned", "dist", "rmsd_all"))
    got = out["torsions"]
    assert set(got) == {"pairwise", "to_gt", "deviation"} and got["pairwise"].shape == (4, 4) and got["to_gt"].shape == (4,)
    assert got["deviation"].shape == (4, spec.n_entries)
    assert torch.equal(got["pairwise"], spec.pairwise(out["poses"]))
    assert torch.equal(got["to_gt"], spec.to_reference(out["poses"], dbatch["x_gt"].float())["tfd"])
    bare = driver.redock(model, dbatch, torsions=TorsionFingerprint.from_bonds(n_lig, chain), **kw)      # no ligand_idx: redock gathers
    assert torch.equal(bare["torsions"]["pairwise"], got["pairwise"]) and torch.equal(bare["torsions"]["to_gt"], got["to_gt"])
    t = SdfTemplate.from_batch(dbatch, chain, title="small")
    modes = driver.redock(model, dbatch, torsions=spec, clusters=PoseClusters(0.3, metric="torsion"), sdf=t, **kw)
    assert torch.equal(modes["clusters"]["dist"], got["pairwise"])
    assert modes["clusters"]["labels"].tolist() == pcr.restate(got["pairwise"].cpu().numpy(), np.arange(4), 0.3)["labels"].tolist()
    back = parse_sdf("".join(SdfTemplate.split(modes["sdf"])))
    assert len(back) == 4
    for p, r in enumerate(back):
        text = r["properties"]["tfd"]                        # printed with the SD writer's default decimals: half a unit of the last
        assert abs(float(text) - float(got["to_gt"][p])) <= 0.5 * 10.0 ** -len(text.split(".")[1]) + 1e-7, (text, float(got["to_gt"][p]))
    assert "tfd" not in parse_sdf("".join(SdfTemplate.split(driver.redock(model, dbatch, sdf=t, **kw)["sdf"])))[0]["properties"]
    pool = torch.randn(6, n_lig, 3, generator=torch.Generator().manual_seed(5)) * 2
    gp = driver.redock(model, dbatch, torsions=spec, ref_mol_poses=pool, **kw)["torsions"]
    assert set(gp) == {"pairwise", "to_gt", "deviation", "nearest_template", "nearest_template_tfd"} and gp["nearest_template"].shape == (4,)
    many = driver.redock_many(model, [(dbatch, {"torsions": spec})], **kw)
    assert torch.equal(many[0]["poses"], plain["poses"]) and torch.equal(many[0]["torsions"]["pairwise"], got["pairwise"])
    grouped = driver.redock_many(model, [(dbatch, {"torsions": spec, "seed": 3})], group=1, **{k: v for k, v in kw.items() if k != "seed"})
    assert set(grouped[0]["torsions"]) == {"pairwise", "to_gt", "deviation"}
    with pytest.raises(ValueError, match="ligand atoms"):
        driver.redock(model, dbatch, torsions=TorsionFingerprint.from_bonds(n_lig + 1, chain), **kw)
    with pytest.raises(ValueError, match="torsions="):
        driver.redock(model, dbatch, clusters=PoseClusters(0.3, metric="torsion"), **kw)
