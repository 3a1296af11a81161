"""pd_pose_validity (csrc/validity.hip) straight on the C ABI, PoseValidity.check, and the validity keywords of redock / redock_many.

The yardstick is the float64 numpy restatement tests/validity_ref.py.  The fp32 columns (0 - 6) follow the rule of
tests/test_sym_rmsd_gpu.py: with ref64 the float64 value and ref32 the same formula evaluated in fp32 by numpy,
E = max|ref32 - ref64| is what fp32 arithmetic alone costs on that input, and the device must satisfy

    |dev - ref64| <= TOL_FACTOR * E + TOL_FLOOR_ULPS * ulp32(max|ref64|)

per column (infinite entries - an empty set - must agree exactly and are left out of E and the maximum).  Column 7 is computed in
double on coordinates of at most 50 A, so its rounding is ~1e-13; it is stored as fp32 (relative 6e-8) and bounded by PLANE_TOL =
1e-6 A, five orders below the 0.25 A threshold.  One `ENVELOPE | ...` line is printed per comparison (pytest -s): the source of
the table in NOTES.md.  Output buffers are one row longer than needed and pre-filled with a sentinel (NaN, -7 for integers)."""
import math

import numpy as np
import pytest
import torch

import validity_ref as ref

pytestmark = pytest.mark.gpu

TOL_FACTOR = 4.0
TOL_FLOOR_ULPS = 8.0
PLANE_TOL = 1e-6
PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN = float("nan")
REC_TILE = 256                      # pose atoms per block of the kernel's receptor pass (physdock_amd.validity.REC_TILE)
TABLE_KEYS = ("lig_idx", "radius", "rec_mask", "lig_active", "pair12", "d12_ref", "pair13", "d13_ref", "far", "planar")
COLUMNS = ("bond min", "bond max", "angle min", "angle max", "internal", "receptor", "distance", "planarity")


# ------------------------------------------------------------------ rule, sentinels, plumbing
def _ulp32(v):
    s = np.float32(abs(v))
    return float(np.nextafter(s, np.float32(np.inf)) - s)


def rule_bound(r32, r64):
    """(bound, E) of one column; entries that are infinite in the float64 value are left out (they must agree exactly)"""
    r32, r64 = np.asarray(r32, dtype=np.float64), np.asarray(r64, dtype=np.float64)
    fin = np.isfinite(r64)
    if not fin.any():
        return 0.0, 0.0
    E = float(np.abs(r32[fin] - r64[fin]).max())
    return TOL_FACTOR * E + TOL_FLOOR_ULPS * _ulp32(float(np.abs(r64[fin]).max())), E


def check_val(case, dev, r32, r64):
    """val [P,8] of the device against the restatement, column by column -> the bounds of the columns [8]"""
    dev = dev.detach().cpu().double().numpy()
    assert dev.shape == r64.shape, (case, dev.shape, r64.shape)
    bounds = np.zeros(8)
    for c in range(8):
        fin = np.isfinite(r64[:, c])
        assert np.array_equal(dev[~fin, c], r64[~fin, c]), (case, COLUMNS[c], dev[:, c], r64[:, c])
        if c == 7:
            bound, E = PLANE_TOL, 0.0
        else:
            bound, E = rule_bound(r32[:, c], r64[:, c])
        bounds[c] = bound
        if not fin.any():
            continue
        err = float(np.abs(dev[fin, c] - r64[fin, c]).max())
        print(f"ENVELOPE | pd_pose_validity | {case} {COLUMNS[c]} | {E:.2e} | {err:.2e} | {bound:.2e} | {err / bound if bound else 0.0:.2f} |")
        assert err <= bound, (case, COLUMNS[c], "E", E, "err", err, "bound", bound)
    return bounds


def sentinel(*shape, dtype=torch.float32):
    fill = NAN if dtype.is_floating_point else -7
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")


def is_sentinel(t):
    return torch.isnan(t) if t.dtype.is_floating_point else t == -7


def body(buf, written=True):
    torch.cuda.synchronize()
    assert is_sentinel(buf[-1]).all(), "the row behind the output was written"
    if written:
        assert not is_sentinel(buf[:-1]).any(), "an output element kept its sentinel"
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


def thresholds(**kw):
    from physdock_amd._lib import ValidityThresholds
    t = dict(ref.DEFAULT_THRESHOLDS)
    t.update(kw)
    return ValidityThresholds(*[t[k] for k in ref.DEFAULT_THRESHOLDS])


DTYPES = dict(lig_idx=np.int32, radius=np.float32, rec_mask=np.uint8, lig_active=np.uint8, pair12=np.int32, d12_ref=np.float32,
              pair13=np.int32, d13_ref=np.float32, far=np.uint8, planar=np.int32)


def launch(L, x, t, thr=None):
    """one pd_pose_validity call into sentinel buffers -> (val, worst, flags) buffers (tail row included)"""
    x = torch.as_tensor(x).cuda().contiguous()
    n, A = x.shape[0], x.shape[1]
    d = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(t[k], dtype=DTYPES[k]))).cuda() for k in TABLE_KEYS}
    n12, n13, G = len(t["pair12"]), len(t["pair13"]), len(t["planar"])
    check_tables(t, A)
    ws = torch.empty(L.pd_pose_validity_workspace_numel(n, A), dtype=torch.int64, device="cuda")
    val, worst, flags = sentinel(n, 8), sentinel(n, 2, dtype=torch.int32), sentinel(n, dtype=torch.int32)
    rc = L.pd_pose_validity(P(x), P(d["lig_idx"]), P(d["radius"]), P(d["rec_mask"]), P(d["lig_active"]), P(d["pair12"]) if n12 else None,
                            P(d["d12_ref"]) if n12 else None, P(d["pair13"]) if n13 else None, P(d["d13_ref"]) if n13 else None,
                            P(d["far"]), P(d["planar"]) if G else None, thr or thresholds(), P(ws), P(val), P(worst), P(flags),
                            n, A, len(t["lig_idx"]), n12, n13, G, S())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return val, worst, flags


def check_tables(t, A):
    """the kernel trusts its tables: every index it would follow is inside its array"""
    Lg = len(t["lig_idx"])
    assert 0 <= np.min(t["lig_idx"]) and np.max(t["lig_idx"]) < A and len(t["radius"]) == A == len(t["rec_mask"])
    assert len(t["lig_active"]) == Lg and np.asarray(t["far"]).shape == (Lg, Lg)
    for k, r in (("pair12", "d12_ref"), ("pair13", "d13_ref")):
        p = np.asarray(t[k]).reshape(-1, 2)
        assert len(p) == len(t[r]) and (p.size == 0 or (0 <= p.min() and p.max() < Lg))
    g = np.asarray(t["planar"]).reshape(-1, 8)
    assert g.size == 0 or (-1 <= g.min() and g.max() < Lg)


def host_flags(val, **kw):
    """the thresholds, as the fp32 numbers the kernel is given, applied to the device's own val"""
    return ref.flags(val.detach().cpu().numpy().astype(np.float32), kw)


# ------------------------------------------------------------------ kernel cases
def kernel_case(n, Lg, n_rec, with12=True, with13=True, groups=(), seed=0):
    """n poses of a chain-bonded ligand of Lg atoms scattered through a pose of Lg + n_rec + 3 atoms (three atoms are neither
    ligand nor receptor); coordinates within +-25 A, the ligand in a box of +-4 A around a centre the receptor surrounds.
    `groups`: sizes of the planar groups (consecutive ligand atoms)."""
    rng = np.random.default_rng(23000 + seed + 1000 * n + 10 * Lg + n_rec)
    A = Lg + n_rec + 3
    perm = rng.permutation(A)
    lig_idx, rec_idx = perm[:Lg], np.sort(perm[Lg:Lg + n_rec])
    x = rng.uniform(-25, 25, (n, A, 3))
    x[:, lig_idx] = rng.uniform(-15, 15, (n, 1, 3)) + rng.uniform(-4, 4, (n, Lg, 3))
    rec_mask = np.zeros(A, np.uint8)
    rec_mask[rec_idx] = 1
    active = (rng.random(Lg) < 0.8).astype(np.uint8)
    active[rng.integers(Lg)] = 1
    i = np.arange(Lg)
    p12 = np.stack([i[:-1], i[1:]], -1) if with12 and Lg > 1 else np.zeros((0, 2), np.int64)
    p13 = np.stack([i[:-2], i[2:]], -1) if with13 and Lg > 2 else np.zeros((0, 2), np.int64)
    far = (np.abs(i[:, None] - i[None, :]) >= 4).astype(np.uint8)
    planar = -np.ones((len(groups), 8), np.int64)
    start = 0
    for g, size in enumerate(groups):
        planar[g, :size] = (start + np.arange(size)) % Lg
        start += 3
    t = dict(lig_idx=lig_idx, radius=rng.choice([1.2, 1.55, 1.6, 1.7, 1.8, 2.0], A).astype(np.float32), rec_mask=rec_mask, lig_active=active,
             pair12=p12, d12_ref=rng.uniform(1.2, 1.6, len(p12)).astype(np.float32), pair13=p13,
             d13_ref=rng.uniform(2.2, 2.6, len(p13)).astype(np.float32), far=far, planar=planar)
    return x.astype(np.float32), t


#: (poses, ligand atoms, receptor atoms, bonded pairs, 1-3 pairs, planar group sizes): every value of each axis the issue lists
CASES = [
    (1, 1, 0, True, True, ()), (1, 1, 65, True, True, ()), (3, 3, 1, True, True, ()), (1, 3, 64, False, True, ()),
    (3, 33, 63, True, True, (4, 8)), (1, 33, 0, True, False, (8,)), (3, 33, REC_TILE + 1, True, True, ()), (1, 65, 64, True, True, (4,)),
    (3, 65, 65, False, False, (8, 4, 6)), (1, 65, REC_TILE + 1, True, True, (4, 8)), (3, 65, 2 * REC_TILE + 1, True, True, (5,)),
    (1, 33, 1, True, True, (4,)),
]


def test_the_case_list_covers_every_axis_value():
    from physdock_amd import validity
    assert validity.REC_TILE == REC_TILE
    assert {c[0] for c in CASES} == {1, 3} and {c[1] for c in CASES} == {1, 3, 33, 65}
    assert {c[2] for c in CASES} >= {0, 1, 63, 64, 65, REC_TILE + 1}
    assert {c[3] for c in CASES} == {False, True} == {c[4] for c in CASES}
    sizes = [s for c in CASES for s in c[5]]
    assert 4 in sizes and 8 in sizes and any(not c[5] for c in CASES)


@pytest.mark.parametrize("n,Lg,n_rec,with12,with13,groups", CASES)
def test_kernel_against_float64(L, n, Lg, n_rec, with12, with13, groups):
    x, t = kernel_case(n, Lg, n_rec, with12, with13, groups)
    assert np.abs(x).max() <= 25.0
    r64, r32 = ref.pose_validity(x, **t), ref.pose_validity(x, **t, fp32=True)
    assert r64["eig"].size == 0 or r64["eig"][..., 1].min() >= 0.1, "a test group is close to collinear"
    val, worst, flags = launch(L, x, t)
    tag = f"P={n} L={Lg} rec={n_rec} n12={len(t['pair12'])} n13={len(t['pair13'])} G={len(groups)}"
    v = body(val)
    bounds = check_val(tag, v, r32["val"], r64["val"])
    if not len(t["pair12"]):
        assert (v[:, 0:2] == 1).all()
    if not len(t["pair13"]):
        assert (v[:, 2:4] == 1).all()
    if not groups:
        assert (v[:, 7] == 0).all()
    # worst: it attains column 5 in the restatement within the bound, and is the restatement's argmin wherever the runner-up is
    # more than twice the bound away
    w = body(worst).cpu().numpy()
    if n_rec == 0:
        assert (w == -1).all() and torch.isinf(v[:, 5:7]).all() and (v[:, 5:7] > 0).all()
    else:
        for p in range(n):
            a, j = w[p]
            assert 0 <= a < Lg and t["rec_mask"][j] == 1 and t["lig_active"][a] == 1
            assert abs(r64["rec"][p, a, j] - r64["val"][p, 5]) <= bounds[5], (tag, p, w[p])
            flat = np.sort(r64["rec"][p].reshape(-1))
            if len(flat) < 2 or flat[1] - flat[0] > 2 * bounds[5]:
                assert tuple(w[p]) == tuple(r64["worst"][p]), (tag, p)
    # the flags are the thresholds applied to the values as stored - exactly
    assert body(flags).cpu().tolist() == host_flags(v).tolist()
    # bit-identical from launch to launch, and a pose does not see its neighbours
    val2, worst2, flags2 = launch(L, x, t)
    assert torch.equal(body(val2), v) and torch.equal(body(worst2), body(worst)) and torch.equal(body(flags2), body(flags))
    if n > 1:
        for p in range(n):
            v1, w1, f1 = launch(L, x[p:p + 1], t)
            assert torch.equal(body(v1)[0], v[p]) and torch.equal(body(w1)[0], body(worst)[p]) and int(body(f1)[0]) == int(body(flags)[p])


# ------------------------------------------------------------------ properties a wrong kernel fails
def test_masked_receptor_atom_and_inactive_ligand_atom_do_not_count(L):
    x, t = kernel_case(3, 33, 65, seed=1)
    t["lig_active"][:] = 1
    masked = np.setdiff1d(np.arange(x.shape[1]), np.concatenate([t["lig_idx"], np.nonzero(t["rec_mask"])[0]]))[0]
    base = body(launch(L, x, t)[0]).clone()
    x1 = x.copy()
    x1[:, masked] = x[:, t["lig_idx"][5]] + np.float32([0.1, 0, 0])            # 0.1 A from a ligand atom, but rec_mask is 0
    near = body(launch(L, x1, t)[0])
    assert torch.equal(near, base)
    t1 = dict(t, rec_mask=t["rec_mask"].copy())
    t1["rec_mask"][masked] = 1                                                  # ... and it does count once the mask says so
    seen = body(launch(L, x1, t1)[0])
    assert (seen[:, 5] < 0.1).all() and (seen[:, 6] < 0.101).all() and (base[:, 5] > 0.1).all()
    # an inactive ligand atom (a hydrogen under heavy_only) 0.1 A from a receptor atom: columns 4 - 6 do not see it, the bonds do
    t2 = dict(t, lig_active=t["lig_active"].copy())
    t2["lig_active"][7] = 0
    rec0 = np.nonzero(t["rec_mask"])[0][0]
    x2 = x.copy()
    x2[:, t["lig_idx"][7]] = x[:, rec0] + np.float32([0, 0.1, 0])
    v2 = body(launch(L, x2, t2)[0])
    r64, r32 = ref.pose_validity(x2, **t2), ref.pose_validity(x2, **t2, fp32=True)
    check_val("inactive ligand atom", v2, r32["val"], r64["val"])
    assert (v2[:, 5] > 0.1).all() and (v2[:, 6] > 0.2).all()
    assert (body(launch(L, x2, t)[0])[:, 6] < 0.101).all()                      # active, it is seen
    assert not torch.equal(v2[:, 0:4], base[:, 0:4])                            # its bonds and angles moved with it


def test_worst_names_the_last_atom_of_the_last_tile_and_the_smaller_index_of_a_tie(L):
    Lg, A = 9, 2 * REC_TILE
    rng = np.random.default_rng(5)
    lig_idx = np.arange(100, 100 + Lg)
    x = rng.uniform(-25, 25, (2, A, 3)).astype(np.float32)
    x[:, lig_idx] = rng.uniform(-2, 2, (2, Lg, 3)).astype(np.float32)
    rec_mask = np.ones(A, np.uint8)
    rec_mask[lig_idx] = 0
    i = np.arange(Lg)
    t = dict(lig_idx=lig_idx, radius=np.full(A, 1.7, np.float32), rec_mask=rec_mask, lig_active=np.ones(Lg, np.uint8),
             pair12=np.stack([i[:-1], i[1:]], -1), d12_ref=np.full(Lg - 1, 1.5, np.float32), pair13=np.zeros((0, 2), int),
             d13_ref=np.zeros(0, np.float32), far=np.zeros((Lg, Lg), np.uint8), planar=-np.ones((0, 8), int))
    d = np.linalg.norm(x[:, lig_idx][:, :, None].astype(np.float64) - x[:, None].astype(np.float64), axis=-1)[:, :, rec_mask > 0]
    assert d.min() > 0.5, "the random receptor must stay clear of the planted contact"
    x[:, A - 1] = x[:, lig_idx[4]] + np.float32([0, 0, 0.25])                  # the closest receptor atom: last atom, last tile
    val, worst, _ = launch(L, x, t)
    assert body(worst).cpu().tolist() == [[4, A - 1]] * 2
    r64, r32 = ref.pose_validity(x, **t), ref.pose_validity(x, **t, fp32=True)
    check_val("closest atom last in its tile", body(val), r32["val"], r64["val"])
    # two receptor atoms at exactly the same coordinates with the same radius: the smaller index is named, wherever they sit
    for twin in (A - 2, 3, REC_TILE - 1, REC_TILE):
        x2 = x.copy()
        x2[:, twin] = x2[:, A - 1]
        val2, worst2, _ = launch(L, x2, t)
        assert body(worst2).cpu().tolist() == [[4, min(twin, A - 1)]] * 2, twin
        assert torch.equal(body(val2)[:, 5:7], body(val)[:, 5:7])
    # two LIGAND atoms at the same place, equally far from the receptor atom: the smaller ligand index
    x3 = x.copy()
    x3[:, lig_idx[2]] = x3[:, lig_idx[4]]
    assert body(launch(L, x3, t)[1]).cpu().tolist() == [[2, A - 1]] * 2


# ------------------------------------------------------------------ flags on constructed poses
def toluene_like():
    """(reference conformer [11,3], bonds, bond orders): a benzene ring 0 - 5 in the xy plane, a zigzag chain 6 - 9 on atom 0 in the
    same plane, and a chloride (atom 10) as a second fragment 4.5 A beyond the chain's end"""
    ring = [[1.39 * math.cos(k * math.pi / 3), 1.39 * math.sin(k * math.pi / 3), 0.0] for k in range(6)]
    chain, pos, ang = [], np.array([1.39, 0.0, 0.0]), 0.0
    for k in range(4):
        ang = math.radians(34.5) * (1 if k % 2 == 0 else -1)                    # 111 degrees between successive bonds
        pos = pos + (1.51 if k == 0 else 1.53) * np.array([math.cos(ang), math.sin(ang), 0.0])
        chain.append(pos.tolist())
    cl = (np.array(chain[-1]) + np.array([4.5, 0.0, 0.0])).tolist()
    bonds = [(i, (i + 1) % 6) for i in range(6)] + [(0, 6), (6, 7), (7, 8), (8, 9)]
    return np.array(ring + chain + [cl]), bonds, [1.5] * 6 + [1.0] * 4


def constructed_poses(device="cuda"):
    """(x [7,A,3] fp32, PoseValidity): a good pose and six poses with one defect each, in flag-bit order"""
    from physdock_amd.validity import PoseValidity
    lig, bonds, orders = toluene_like()
    n_lig = len(lig)
    # receptor: carbons on two sheets 4 A above and below the ligand's plane, and three atoms that do not count
    gx, gy = np.meshgrid(np.arange(-4.0, 13.0, 2.0), np.arange(-4.0, 5.0, 2.0))
    sheet = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], -1)
    rec = np.concatenate([sheet + [0, 0, 4.0], sheet - [0, 0, 4.0]])
    A = len(rec) + n_lig
    order = np.random.default_rng(11).permutation(A)                            # the ligand scattered through the pose
    lig_idx, rec_idx = order[:n_lig], order[n_lig:]
    elements = np.full(A, 6)
    elements[lig_idx[10]] = 17
    good = np.zeros((A, 3))
    good[lig_idx], good[rec_idx] = lig, rec
    v = PoseValidity.from_bonds(n_lig, bonds, lig, elements, lig_idx, bond_orders=orders, device=device)
    poses = [good.copy() for _ in range(7)]
    a = lambda k: lig_idx[k]
    unit = lambda u: u / np.linalg.norm(u)
    poses[1][a(9)] = good[a(8)] + 1.4 * (good[a(9)] - good[a(8)])               # one bond stretched x 1.4
    u, w = unit(good[a(7)] - good[a(8)]), good[a(9)] - good[a(8)]
    side = unit(w - (w @ u) * u)
    poses[2][a(9)] = good[a(8)] + 1.53 * (math.cos(math.radians(70)) * u + math.sin(math.radians(70)) * side)   # angle 7-8-9 closed to 70
    poses[3][a(10)] = good[a(9)] + 0.5 * (1.7 + 1.8) * unit(good[a(9)] - good[a(8)])                           # two far atoms at half the vdW sum
    poses[4][rec_idx[0]] = good[a(3)] + 0.5 * (1.7 + 1.7) * np.array([-1.0, 0.0, 0.0])                         # a receptor atom at half the vdW sum
    poses[5][a(3)] = good[a(3)] + [0, 0, 0.6]                                    # a ring atom lifted 0.6 A
    poses[6][lig_idx] = good[lig_idx] + [0, 30.0, 0]                             # the ligand 30 A away
    return np.stack(poses).astype(np.float32), v


def host_tables(v):
    return dict(lig_idx=v.ligand_idx, radius=v.radius, rec_mask=v.rec_mask, lig_active=v.lig_active, pair12=v.pair12, d12_ref=v.d12_ref,
                pair13=v.pair13, d13_ref=v.d13_ref, far=v.far, planar=v.planar)


def test_flags_of_constructed_poses(L):
    x, v = constructed_poses()
    t = host_tables(v)
    assert v.planar.tolist() == [[0, 1, 2, 3, 4, 5, -1, -1]] and len(v.pair12) == 10 and v.far[9, 10] == 1
    r64, r32 = ref.pose_validity(x, **t), ref.pose_validity(x, **t, fp32=True)
    bounds = np.array([rule_bound(r32["val"][:, c], r64["val"][:, c])[0] if c < 7 else PLANE_TOL for c in range(8)])
    margin = ref.margins(r64["val"])
    assert (margin >= 10 * bounds[None, :]).all(), ("a constructed value sits too close to its threshold", margin.min(0), bounds)
    expect = ref.flags(r64["val"])
    assert expect.tolist() == [0, 1, 2, 4, 8, 16, 32]                           # a good pose, then each defect its own bit
    val, worst, flags = launch(L, x, t)
    check_val("constructed poses", body(val), r32["val"], r64["val"])
    assert body(flags).cpu().tolist() == expect.tolist() == host_flags(body(val)).tolist()
    out = v.check(torch.from_numpy(x).cuda())
    assert out["flags"].cpu().tolist() == expect.tolist() and out["valid"].cpu().tolist() == [True] + [False] * 6
    assert [v.check_names(f) for f in out["flags"].cpu()] == [[]] + [[n] for n in ref.CHECK_NAMES]
    assert r64["val"][1, 1] == pytest.approx(1.4, abs=1e-5) and r64["val"][3, 4] == pytest.approx(0.5, abs=1e-5)
    assert r64["val"][4, 5] == pytest.approx(0.5, abs=1e-5) and r64["val"][6, 6] > 20


def test_thresholds_are_taken_from_the_struct(L):
    x, t = kernel_case(3, 33, 63, groups=(4, 8))
    loose = dict(bond_lo=0.0, bond_hi=1e9, angle_lo=0.0, angle_hi=1e9, internal_clash=0.0, receptor_clash=0.0, planarity=1e9, detached=1e9)
    assert body(launch(L, x, t, thresholds(**loose))[2]).cpu().tolist() == [0, 0, 0]
    for bit, (k, value) in enumerate([("bond_lo", 1e9), ("angle_hi", 0.0), ("internal_clash", 1e9), ("receptor_clash", 1e9), ("planarity", 0.0),
                                      ("detached", 0.0)]):
        kw = dict(loose, **{k: value})
        val, _, flags = launch(L, x, t, thresholds(**kw))
        assert body(flags).cpu().tolist() == [1 << bit] * 3 == host_flags(body(val), **kw).tolist(), k


# ------------------------------------------------------------------ argument handling
def test_argument_handling(L):
    x, t = kernel_case(2, 5, 4, groups=(4,))
    xd = torch.from_numpy(x).cuda()
    d = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(t[k], dtype=DTYPES[k]))).cuda() for k in TABLE_KEYS}
    A = x.shape[1]
    ws = torch.empty(L.pd_pose_validity_workspace_numel(2, A), dtype=torch.int64, device="cuda")
    val, worst, flags = sentinel(2, 8), sentinel(2, 2, dtype=torch.int32), sentinel(2, dtype=torch.int32)
    names = ["x", "lig_idx", "radius", "rec_mask", "lig_active", "pair12", "d12_ref", "pair13", "d13_ref", "far", "planar", "thr", "ws", "val",
             "worst", "flags"]
    good = [P(xd)] + [P(d[k]) for k in TABLE_KEYS] + [thresholds(), P(ws), P(val), P(worst), P(flags)]
    sizes = [2, A, 5, 4, 3, 1]
    rcs = {}
    for k, name in enumerate(names):
        if name != "thr":
            args = list(good)
            args[k] = None
            rcs["null " + name] = L.pd_pose_validity(*args, *sizes, S())
    for k, name in enumerate(["P", "A", "L"]):
        sz = list(sizes)
        sz[k] = 0
        rcs[name + "=0"] = L.pd_pose_validity(*good, *sz, S())
    rcs["n12<0"] = L.pd_pose_validity(*good, 2, A, 5, -1, 3, 1, S())
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), rcs
    # the optional tables may be NULL exactly when their count is 0
    opt = list(good)
    for k in (5, 6, 7, 8, 10):
        opt[k] = None
    unsupported = {"L": L.pd_pose_validity(*good, 2, A, 1025, 4, 3, 1, S()), "G": L.pd_pose_validity(*good, 2, A, 5, 4, 3, 257, S()),
                   "A": L.pd_pose_validity(*good, 2, (1 << 22) + 1, 5, 4, 3, 1, S()), "P": L.pd_pose_validity(*good, 65536, A, 5, 4, 3, 1, S())}
    assert all(rc == PD_ERR_UNSUPPORTED for rc in unsupported.values()), unsupported
    torch.cuda.synchronize()
    assert is_sentinel(val).all() and is_sentinel(worst).all() and is_sentinel(flags).all()
    assert L.pd_pose_validity(*opt, 2, A, 5, 0, 0, 0, S()) == 0
    assert (body(val)[:, 0:4] == 1).all() and (body(val)[:, 7] == 0).all() and not is_sentinel(body(flags)).any()


# ------------------------------------------------------------------ PoseValidity.check, redock, redock_many
def chain_bonds(n):
    return [(i, i + 1) for i in range(n - 1)]


def validity_for(batch, **kw):
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.validity import PoseValidity
    return PoseValidity.from_batch(batch, chain_bonds(int(ligand_atom_mask(batch).sum())), **kw)


def same_check(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_check_on_a_synthetic_batch_agrees_with_the_c_abi(L):
    from physdock_amd.synthetic import make_batch
    batch = {k: v.cuda() for k, v in make_batch(20, 4, 9, 4, seed=6).items()}
    v = validity_for(batch, planar_groups=[(0, 1, 2, 3), (2, 3, 4, 5, 6, 7, 8)])
    g = torch.Generator().manual_seed(7)
    x = (batch["x_gt"].cpu()[None] + 0.3 * torch.randn(5, batch["x_gt"].shape[0], 3, generator=g)).cuda()
    out = v.check(x)
    assert set(out) == {"valid", "flags", "bond_ratio", "angle_ratio", "internal_clash", "receptor_clash", "receptor_distance", "planarity",
                        "worst_pair"}
    assert out["valid"].dtype == torch.bool and out["flags"].dtype == torch.int32 and out["worst_pair"].dtype == torch.int32
    assert all(t.is_cuda for t in out.values()) and out["bond_ratio"].shape == (5, 2) and out["worst_pair"].shape == (5, 2)
    val, worst, flags = launch(L, x.cpu().numpy(), host_tables(v))
    val, worst, flags = body(val), body(worst), body(flags)
    assert torch.equal(out["flags"], flags) and torch.equal(out["worst_pair"], worst) and torch.equal(out["valid"], flags == 0)
    got = torch.cat([out["bond_ratio"], out["angle_ratio"], out["internal_clash"][:, None], out["receptor_clash"][:, None],
                     out["receptor_distance"][:, None], out["planarity"][:, None]], 1)
    assert torch.equal(got, val)
    t = host_tables(v)
    check_val("PoseValidity.check", val, ref.pose_validity(x.cpu().numpy(), **t, fp32=True)["val"], ref.pose_validity(x.cpu().numpy(), **t)["val"])
    with pytest.raises(ValueError, match="pose atoms"):
        v.check(x[:, :-1])


@pytest.fixture(scope="module")
def small(small_model_inputs):
    from physdock_amd import PhysDock
    cfg, P_, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P_, strict=True)
    return model.cuda().eval(), {k: v.cuda() for k, v in batch.items()}, cfg


def same_ranking(a, b):
    return (a["order"] == b["order"] and a["rmsd"] == b["rmsd"]
            and all(torch.equal(a[k], b[k]) for k in ("x_aligned", "dist", "rmsd_all")) and set(a) == set(b))


def test_redock_reports_validity_and_changes_nothing_else(small):
    from physdock_amd import driver
    model, dbatch, _ = small
    v = validity_for(dbatch)
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, dbatch, **kw)
    out = driver.redock(model, dbatch, validity=v, **kw)
    assert set(out) == set(plain) | {"validity"}
    assert torch.equal(out["poses"], plain["poses"]) and out["rounds"] == plain["rounds"] and out["accepted"] == plain["accepted"]
    assert same_ranking(out["ranking"], plain["ranking"]) and out["gamma_factor"] == plain["gamma_factor"]
    assert same_check(out["validity"], v.check(out["poses"])) and out["validity"]["flags"].shape == (4,)
    # without physics correction there is no accept / reject, so the filter has nothing to reject and logs nothing
    filt = driver.redock(model, dbatch, validity=v, validity_filter=True, **kw)
    assert torch.equal(filt["poses"], plain["poses"]) and filt["rounds"] == plain["rounds"]
    many = driver.redock_many(model, [(dbatch, {"validity": v})], **kw)              # one system: the sequential path
    assert torch.equal(many[0]["poses"], plain["poses"]) and same_check(many[0]["validity"], out["validity"])
    assert many[0]["rounds"] == plain["rounds"] and same_ranking(many[0]["ranking"], plain["ranking"])


def test_validity_filter_rejects_where_chirality_does(small):
    from physdock_amd import driver
    from physdock_amd.synthetic import reference_conformers
    model, dbatch, _ = small
    confs = reference_conformers({k: t.cpu() for k, t in dbatch.items()}, n_conf=6, seed=1).cuda()
    # a random small model's ligand is nowhere near its conformer: no pose keeps every bond within 0.1 % of its reference
    strict = validity_for(dbatch, thresholds={"bond_lo": 0.999, "bond_hi": 1.001})
    kw = dict(ref_mol_poses=confs, physics_correction=True, max_samples=3, max_rounds=2, num_samples_per_round=3, steps=6, seed=2)
    plain = driver.redock(model, dbatch, **kw)
    out = driver.redock(model, dbatch, validity=strict, validity_filter=True, **kw)
    assert [r["invalid"] for r in out["rounds"]] == [r["sampled"] for r in out["rounds"]] == [3, 3]
    assert [r["accepted"] for r in out["rounds"]] == [0, 0] and out["accepted"] == 0
    assert out["gamma_factor"] == pytest.approx(max(max(6.0 * 0.7, 1.0) * 0.7, 1.0))
    assert all("invalid" not in r for r in plain["rounds"]) and plain["accepted"] == 3
    # the restatement agrees that every returned (rejected, topped-up) pose fails the bond check, far from the thresholds
    r64 = ref.pose_validity(out["poses"].cpu().numpy(), **host_tables(strict))
    assert (ref.flags(r64["val"], strict.thresholds) & 1).all() and out["validity"]["flags"].cpu().numpy().astype(int).tolist() == \
        ref.flags(r64["val"], strict.thresholds).tolist()
    assert min(abs(r64["val"][:, 0] - 0.999).min(), abs(r64["val"][:, 1] - 1.001).min()) > 1e-3
    # reported but not filtered: the rounds are those of the plain call
    rep = driver.redock(model, dbatch, validity=strict, **kw)
    assert rep["rounds"] == plain["rounds"] and torch.equal(rep["poses"], plain["poses"]) and not rep["validity"]["valid"].any()
    # default thresholds through the filter: the log counts exactly the poses check() fails (round 0 is seeded: sample it again)
    loose = validity_for(dbatch)
    x0 = model.sample_diffusion(dbatch, num_sample=3, steps=6, seed=2, align_ref_pos=False, karras_noise_schedule_power=1000,
                                mmff_gamma_0_factor=6.0, ode_step_scale_eta=1.5)
    out2 = driver.redock(model, dbatch, validity=loose, validity_filter=True, **kw)
    n_bad = int((~loose.check(x0)["valid"]).sum())
    assert out2["rounds"][0]["invalid"] == n_bad and out2["rounds"][0]["accepted"] == 3 - n_bad


def test_redock_many_takes_a_validity_per_system(small):
    from physdock_amd import driver
    from physdock_amd.synthetic import make_batch
    model, _, _ = small
    batches = [{k: v.cuda() for k, v in make_batch(n, 5, nl, 8, seed=70 + i).items()} for i, (n, nl) in enumerate([(18, 6), (14, 5)])]
    vs = [validity_for(b) for b in batches]
    assert vs[0].n_atoms != vs[1].n_atoms
    common = dict(num_samples_per_round=3, max_samples=3, steps=4)
    systems = [(b, {"validity": v, "seed": 100 + i}) for i, (b, v) in enumerate(zip(batches, vs))]
    bare = driver.redock_many(model, [(b, {"seed": 100 + i}) for i, b in enumerate(batches)], group=2, **common)
    for path in (dict(group=2), dict(streams=1), dict(streams=2)):
        res = driver.redock_many(model, systems, **path, **common)
        for v, r, r0 in zip(vs, res, bare):
            assert same_check(r["validity"], v.check(r["poses"])), path
            assert r["rounds"] == r0["rounds"] and "validity" not in r0
            if "group" in path:
                assert torch.equal(r["poses"], r0["poses"])
    one = [driver.redock(model, b, validity=v, seed=100 + i, **common) for i, (b, v) in enumerate(zip(batches, vs))]
    seq = driver.redock_many(model, systems, streams=1, **common)
    for a, b in zip(one, seq):
        assert torch.equal(a["poses"], b["poses"]) and same_check(a["validity"], b["validity"]) and a["rounds"] == b["rounds"]


def test_order_confidence_valid_puts_valid_poses_first(small):
    from physdock_amd import driver
    from physdock_amd.confidence import ConfidenceModule
    from physdock_amd.params import confidence_param_shapes, seeded_state_dict
    from physdock_amd.ranking import rank_by_confidence
    model, dbatch, cfg = small
    cm = dict(cfg.model.confidence_module)
    conf = ConfidenceModule(**cm)
    conf.load_state_dict(seeded_state_dict(confidence_param_shapes(**cm), seed=3), strict=True)
    conf = conf.cuda().eval()
    kw = dict(num_samples_per_round=6, max_samples=6, steps=4, seed=3)
    base = driver.redock(model, dbatch, validity=validity_for(dbatch), **kw)
    # a bond window set between the poses' own smallest ratios, so that some poses pass and some fail
    lo = base["validity"]["bond_ratio"][:, 0].cpu().double().sort().values
    cut = float((lo[2] + lo[3]) / 2)
    assert lo[3] - lo[2] > 1e-4, "the poses' bond ratios must be told apart"
    v = validity_for(dbatch, thresholds={"bond_lo": cut, "bond_hi": 1e9, "angle_lo": 0.0, "angle_hi": 1e9, "internal_clash": 0.0,
                                         "receptor_clash": 0.0, "planarity": 1e9, "detached": 1e9})
    with_conf = driver.redock(model, dbatch, confidence=conf, **kw)
    out = driver.redock(model, dbatch, confidence=conf, validity=v, **kw)
    assert set(out) == set(with_conf) | {"validity", "order_confidence_valid"}
    assert torch.equal(out["order_confidence"], with_conf["order_confidence"]) and torch.equal(out["poses"], with_conf["poses"])
    valid = out["validity"]["valid"]
    assert int(valid.sum()) == 3
    order, both = out["order_confidence"].tolist(), out["order_confidence_valid"]
    assert both.is_cuda and torch.equal(both, rank_by_confidence(out["confidence"], valid=valid))
    vl = valid.cpu().tolist()
    assert both.tolist() == [i for i in order if vl[i]] + [i for i in order if not vl[i]]
