"""pd_plif_rings (csrc/plif_rings.hip) straight on the C ABI, RingInteractions, and the ring_interactions keyword of redock /
redock_many.

The yardstick is the float64 restatement tests/plif_rings_ref.py and its acceptance rule (its docstring): lo <= dev <= hi bit by bit
for `bits`, `ligand_bits` and `ring_bits`, where lo / hi are the fingerprints with every distance threshold lowered / raised by 1e-4 A
and every cosine window shrunk / widened by 1e-4; `counts` are the popcounts of the device's own bits; `centroid`, `normal` and
`min_centroid_dist` lie within the derived float64 / fp32 rounding bounds element by element, with nothing multiplied on, and +inf
matches exactly.  In every seeded case lo == hi (tests/test_plif_rings_cpu.py asserts it on the CPU; it is asserted again here), so
the device must equal the restatement.  Output buffers are one row longer than needed and pre-filled with a sentinel (bytes 0xA5 -
bit 7 is never set by the kernel -, NaN, -7777).

Case d crosses every block and stride of the kernels - FRAME_BLOCK = 64 rings per block of plif_rings_frame_kernel (70 rings),
RECEPTOR_BLOCK = 256 receptor entities per block of plif_rings_receptor_kernel (68 rings + 672 list entries: three blocks, the
first holds rings and entries), the stride LIGAND_BLOCK = 64 of plif_rings_ligand_kernel (68 receptor rings, 672 entries, 273
acceptors among them), the stride FOLD_BLOCK = 64 of plif_rings_fold_kernel (97 residues, 72 ligand atoms).  No kernel tiles the
poses: a pose is a grid index, and case e has 66 of them."""
import ctypes

import numpy as np
import pytest
import torch

import plif_ref
import plif_rings_ref as ref

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN = float("nan")
BYTE, INT = 0xA5, -7777
CASE_A = "a_P3_L16_R14"
BYTES = ("bits", "ligand_bits", "ring_bits")
OUT = BYTES + ("centroid", "normal", "min_centroid_dist", "counts")
DTYPES = dict(bits=torch.uint8, ligand_bits=torch.uint8, ring_bits=torch.uint8, centroid=torch.float64, normal=torch.float64,
              min_centroid_dist=torch.float32, counts=torch.int32)


# ------------------------------------------------------------------ sentinels, plumbing
def sentinel(shape, dtype):
    fill = {torch.uint8: BYTE, torch.int32: INT, torch.float32: NAN, torch.float64: NAN}[dtype]
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")


def untouched(buf):
    return bool(torch.isnan(buf).all()) if buf.is_floating_point() else bool((buf == (BYTE if buf.dtype == torch.uint8 else INT)).all())


def body(buf, nan_ok=False):
    torch.cuda.synchronize()
    assert untouched(buf[-1]), "the row behind the output was written"
    head = buf[:-1]
    if not nan_ok:
        assert not (torch.isnan(head).any() if buf.is_floating_point() else (head == (BYTE if buf.dtype == torch.uint8 else INT)).any()), \
            "an output element kept its sentinel"
    return head


@pytest.fixture(scope="module")
def L():
    from physdock_amd import ops
    return ops._lib.init()


def P(t):
    from physdock_amd import ops
    return ops.ptr(t) if t is not None and t.numel() else None


def S():
    from physdock_amd import ops
    return ops.stream()


def thr(values):
    """the eight doubles the entry takes from a case's thresholds: five distances, then the cosines of the three angles"""
    return (ctypes.c_double * 8)(*values[:5], *[float(np.cos(np.deg2rad(v))) for v in values[5:]])


def tables(c):
    """a case's tables on the device, every index the kernels would follow checked to be inside its array first"""
    A, R, Lg = c["x"].shape[1], int(c["n_residues"]), len(c["lig_idx"])
    start, atom = ref.csr(c)
    ring_start, ring_atom, ring_residue, halogen = ref.ring_tables(c)
    Gl, Gr = len(c["lig_rings"]), len(c["rec_rings"])
    assert 0 <= c["lig_idx"].min() and c["lig_idx"].max() < A and len(c["types"]) == A == len(c["charges"]) == len(c["rec_mask"])
    assert len(c["lig_active"]) == Lg <= 1024 and not c["rec_mask"][c["lig_idx"]].any() and 1 <= R <= A
    assert len(start) == R + 1 and start[0] == 0 and (np.diff(start) >= 0).all() and start[-1] == len(atom) <= A
    assert len(atom) == 0 or (0 <= atom.min() and atom.max() < A and len(set(atom.tolist())) == len(atom))
    assert len(ring_start) == Gl + Gr + 1 and ring_start[0] == 0 and ring_start[-1] == len(ring_atom) and Gl <= 64 and Gr <= 4096
    assert Gl + Gr == 0 or (3 <= np.diff(ring_start).min() and np.diff(ring_start).max() <= 8 and 0 <= ring_atom.min() and ring_atom.max() < A)
    assert (ring_residue[:Gl] == -1).all() and (np.diff(ring_residue[Gl:]) >= 0).all() and (Gr == 0 or (0 <= ring_residue[Gl] and ring_residue[-1] < R))
    assert len(halogen) <= 64 and (len(halogen) == 0 or (0 <= halogen.min() and halogen.max() < Lg))
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()
    return dict(lig_idx=up(c["lig_idx"], np.int32), types=up(c["types"], np.uint8), charges=up(c["charges"], np.uint8),
                lig_active=up(c["lig_active"], np.uint8), res_start=up(start, np.int32), res_atom=up(atom, np.int32),
                ring_start=up(ring_start, np.int32), ring_atom=up(ring_atom, np.int32), ring_residue=up(ring_residue, np.int32),
                halogen=up(halogen, np.int32), N=len(atom), Gl=Gl, Gr=Gr, H=len(halogen), Lg=Lg, R=R)


def shapes(n, d):
    return dict(bits=(n, d["R"]), ligand_bits=(n, d["Lg"]), ring_bits=(n, d["Gl"]), centroid=(n, d["Gl"] + d["Gr"], 3),
                normal=(n, d["Gl"] + d["Gr"], 3), min_centroid_dist=(n, d["R"]), counts=(n, 5))


def raw_call(L, x, d, t, ws, ws_bytes, buf):
    n, A = x.shape[0], x.shape[1]
    G = d["Gl"] + d["Gr"]
    return L.pd_plif_rings(P(x), P(d["lig_idx"]), P(d["types"]), P(d["charges"]), P(d["lig_active"]), P(d["res_start"]), P(d["res_atom"]),
                           P(d["ring_start"]) if G else None, P(d["ring_atom"]), P(d["ring_residue"]), d["Gl"], d["Gr"], P(d["halogen"]), d["H"],
                           t, P(ws), ws_bytes, P(buf["bits"]), P(buf["ligand_bits"]), P(buf["ring_bits"]), P(buf["centroid"]),
                           P(buf["normal"]), P(buf["min_centroid_dist"]), P(buf["counts"]), n, A, d["Lg"], d["R"], d["N"], S())


def launch(L, x, c, d=None):
    """one pd_plif_rings call into sentinel buffers -> dict of the bodies"""
    d = d or tables(c)
    x = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    n = x.shape[0]
    assert x.shape[1] == len(c["types"])
    nbytes = L.pd_plif_rings_workspace(n, d["Lg"], d["N"], d["Gl"], d["Gr"], d["H"])
    assert nbytes > 0 and nbytes % 8 == 0
    ws = sentinel((nbytes // 8,), torch.float64)
    buf = {k: sentinel(s, DTYPES[k]) for k, s in shapes(n, d).items()}
    rc = raw_call(L, x, d, thr(c["thresholds"]), ws, nbytes, buf)
    assert rc == 0, rc
    body(ws, nan_ok=True)                                              # nothing behind the workspace was written
    return {k: body(v, nan_ok=k == "centroid") for k, v in buf.items()}


def check(case, out, want):
    """the device against the restatement under the acceptance rule"""
    dev_bits = {}
    for k in BYTES:
        dev, lo, hi = out[k].cpu().numpy(), want["lo"][k], want["hi"][k]
        assert dev.shape == lo.shape and dev.dtype == np.uint8, (case, k)
        assert not (lo & ~dev).any() and not (dev & ~hi).any(), (case, k, "lo <= dev <= hi fails in", int(((lo & ~dev) | (dev & ~hi) > 0).sum()), "bytes")
        assert not (dev >> 5).any(), "bits 5 to 7 are always 0"
        dev_bits[k] = dev
    assert np.array_equal(out["counts"].cpu().numpy(), ref.popcounts(dev_bits["bits"])), (case, "counts are the popcounts of the device's own bits")
    mid = want["mid"]
    for k, bound in (("centroid", want["centroid_bound"]), ("normal", want["normal_bound"])):
        dev, w = out[k].cpu().numpy(), mid[k]
        assert dev.shape == w.shape and np.array_equal(np.isnan(dev), np.isnan(w)), (case, k, "NaN only where the restatement has one")
        ok = np.broadcast_to(mid["ok"][..., None], w.shape)
        if k == "normal":
            assert not dev[~ok].any(), "a degenerate ring reports the normal 0"
            dev = dev * np.where((dev * w).sum(-1, keepdims=True) < 0, -1.0, 1.0)       # the sign of a normal is not defined
        err = np.abs(dev - w)[ok]
        lim = np.broadcast_to(bound, w.shape)[ok]
        if err.size:
            print(f"ENVELOPE | pd_plif_rings | {case} {k} | {np.abs(w[ok]).max():.2e} | {err.max():.2e} | {lim.max():.2e} | {(err / lim).max():.2f} |")
        assert (err <= lim).all(), (case, k, err.max())
    dev, m, b = out["min_centroid_dist"].cpu().double().numpy(), mid["min_centroid_dist"], want["min_bound"]
    assert np.array_equal(np.isinf(dev), np.isinf(m)) and (dev[np.isinf(dev)] > 0).all() and not np.isnan(dev).any(), (case, "+inf must match exactly")
    fin = np.isfinite(m)
    if fin.any():
        err = np.abs(dev[fin] - m[fin])
        print(f"ENVELOPE | pd_plif_rings | {case} min_centroid_dist | {m[fin].max():.2e} | {err.max():.2e} | {b[fin].max():.2e} | {(err / b[fin]).max():.2f} |")
        assert (err <= b[fin]).all(), (case, "min_centroid_dist", err.max())


def same(a, b, keys=None):
    """bit-equal tensors (NaN equal to NaN: a ring with a NaN coordinate reports a NaN centroid)"""
    eq = lambda u, w: torch.equal(torch.nan_to_num(u, nan=-1e300), torch.nan_to_num(w, nan=-1e300)) if u.is_floating_point() else torch.equal(u, w)
    return all(eq(a[k], b[k]) for k in (keys or a))


# ------------------------------------------------------------------ cases a - f
@pytest.mark.parametrize("name", ref.CASES)
def test_kernel_against_float64(L, name):
    c = ref.make_case(name)
    want = ref.restate(c)
    assert want["open_bytes"] == 0, "the case must leave no bit open"
    d = tables(c)
    out = launch(L, c["x"], c, d)
    check(name, out, want)
    assert all(np.array_equal(out[k].cpu().numpy(), want["lo"][k]) for k in BYTES)
    n = c["x"].shape[0]
    # bit-identical from launch to launch
    assert same(launch(L, c["x"], c, d), out)
    # a pose fingerprinted alone is the pose inside the batch
    for p in sorted({0, 1, n // 2, n - 1}):
        one = launch(L, c["x"][p:p + 1], c, d)
        assert same({k: v[0] for k, v in one.items()}, {k: v[p] for k, v in out.items()}), (name, p)
    # reversing the poses reverses the outputs
    rev = launch(L, c["x"][::-1], c, d)
    assert same({k: v.flip(0) for k, v in rev.items()}, out), name
    # inactive ligand atoms report 0
    off = torch.from_numpy(c["lig_active"] == 0).cuda()
    assert not out["ligand_bits"][:, off].any()


def test_case_a_shows_and_misses_every_kind(L):
    c = ref.make_case(CASE_A)
    out = launch(L, c["x"], c)
    bits = out["bits"].cpu().numpy()
    for k in range(5):
        shown = (bits >> k & 1).astype(bool)
        assert shown.any() and not shown.all() and (shown.any(0) & ~shown.all(0)).any(), ref.RING_KIND_NAMES[k]
    assert bits[0, [2, 3, 5, 7]].tolist() == [0, 0, 0, 0] and bits[0, [0, 1, 4, 6, 8]].tolist() == [1, 2, 4, 16, 8]
    m = out["min_centroid_dist"].cpu().numpy()
    ringed = np.zeros(14, dtype=bool)
    ringed[c["rec_ring_residue"]] = True
    assert np.isfinite(m[:, ringed]).all() and np.isinf(m[:, ~ringed]).all()


def test_the_empty_forms(L):
    for name in ("b_no_ligand_ring", "b_no_receptor_ring", "c_no_receptor_atom"):
        c = ref.make_case(name)
        out = launch(L, c["x"], c)
        assert bool(torch.isinf(out["min_centroid_dist"]).all()) and not (out["bits"] & 3).any(), name
        assert out["centroid"].shape[1] == len(c["lig_rings"]) + len(c["rec_rings"])
    assert not out["bits"].any() and not out["ligand_bits"].any() and not out["ring_bits"].any() and not out["counts"].any()


def test_degenerate_and_nan_rings_show_nothing_and_touch_nothing_else(L):
    c = ref.make_case("f_degenerate_and_nan")
    out = launch(L, c["x"], c)
    p = ref.F_NAN_POSE
    assert not out["ring_bits"][:, 2].any() and not out["normal"][:, 2].any(), "three collinear atoms"
    assert not out["ring_bits"][p, 0].any() and not out["normal"][p, 0].any() and bool(out["ring_bits"][0, 0] != 0), "the ring with the NaN"
    assert bool(torch.isnan(out["centroid"][p, 0]).any()) and not torch.isnan(out["centroid"][[0, 2]]).any()
    assert not torch.isnan(out["min_centroid_dist"]).any() and not torch.isnan(out["normal"]).any()
    clean = c["x"].copy()
    clean[p] = c["x"][0]
    base = launch(L, clean, c)
    keep = [q for q in range(3) if q != p]
    assert same({k: v[keep] for k, v in out.items()}, {k: v[keep] for k, v in base.items()}), "the other poses are untouched"
    assert bool(out["ring_bits"][p, 1] == out["ring_bits"][0, 1]) and bool(out["ring_bits"][p, 1] != 0), "the other ring of the pose is untouched"
    lig = c["lig_idx"]
    five = torch.from_numpy(np.asarray([int(a) - int(lig[0]) for a in c["lig_rings"][1]])).cuda()
    assert bool((out["ligand_bits"][p, five] == out["ring_bits"][p, 1]).all())


def test_rotating_or_reversing_a_ring_changes_no_byte(L):
    c = ref.make_case(CASE_A)
    out = launch(L, c["x"], c)
    for which in ("lig_rings", "rec_rings"):
        for g in range(len(c[which])):
            ring = list(c[which][g])
            for new in (ring[2:] + ring[:2], ring[::-1]):
                moved = dict(c, **{which: c[which][:g] + [new] + c[which][g + 1:]})
                got = launch(L, c["x"], moved)
                assert same(got, out, BYTES + ("counts",)), (which, g, new)
                check(f"{which} {g} moved", got, ref.restate(moved))


def test_a_rigid_motion_of_a_pose_changes_no_byte(L):
    c = ref.make_case(CASE_A)
    out = launch(L, c["x"], c)
    Rm, t = ref.rotation([0.3, -1.0, 0.6], 77.0), np.array([11.0, -7.5, 4.25])
    x = c["x"].astype(np.float64)
    x[0] = x[0] @ Rm.T + t                                             # pose 0 moves as a whole; poses 1 and 2 stay
    x = x.astype(np.float32)
    want = ref.restate(c, x)
    assert want["open_bytes"] == 0
    got = launch(L, x, c)
    check("moved pose", got, want)
    assert same(got, out, BYTES + ("counts",))
    assert same({k: v[[1, 2]] for k, v in got.items()}, {k: v[[1, 2]] for k, v in out.items()})


def test_a_ligand_far_away_shows_nothing_and_keeps_finite_distances(L):
    c = ref.make_case(CASE_A)
    x = c["x"].copy()
    x[0, c["lig_idx"]] += np.float32([60.0, 0.0, 0.0])                # pose 0: the ligand 60 A away; poses 1 and 2 as they were
    want = ref.restate(c, x)
    assert want["open_bytes"] == 0 and not want["lo"]["bits"][0].any() and want["lo"]["bits"][2].any()
    out = launch(L, x, c)
    assert not out["bits"][0].any() and not out["ligand_bits"][0].any() and not out["ring_bits"][0].any() and not out["counts"][0].any()
    ringed = torch.zeros(14, dtype=torch.bool)
    ringed[c["rec_ring_residue"]] = True
    assert torch.isfinite(out["min_centroid_dist"][0, ringed.cuda()]).all() and (out["min_centroid_dist"][0, ringed.cuda()] > 30).all()
    check("far ligand", out, want)
    base = launch(L, c["x"], c)
    assert same({k: v[[1, 2]] for k, v in out.items()}, {k: v[[1, 2]] for k, v in base.items()})


def test_thresholds_are_arguments(L):
    c = ref.make_case(CASE_A)
    base = launch(L, c["x"], c)
    zero = dict(c, thresholds=(0.0,) * 5 + ref.THRESHOLDS[5:])
    out = launch(L, c["x"], zero)
    assert not out["bits"].any() and not out["ligand_bits"].any() and not out["ring_bits"].any()
    assert same(out, base, ("centroid", "normal", "min_centroid_dist")), "the frames do not depend on the thresholds"
    wide = dict(c, thresholds=(7.0, 3.5, 7.0, 5.0, 5.0, 50.0, 40.0, 95.0))
    want = ref.restate(wide)
    assert want["open_bytes"] == 0 and want["lo"]["counts"].sum() > ref.restate(c)["lo"]["counts"].sum()
    got = launch(L, c["x"], wide)
    check("widened", got, want)
    assert all(np.array_equal(got[k].cpu().numpy(), want["lo"][k]) for k in BYTES)
    assert bool((got["bits"][0, [2, 3, 5, 7]] != 0).all()), "the four designed near misses of pose 0 now show"


# ------------------------------------------------------------------ argument handling
def test_argument_handling(L):
    c = ref.make_case(CASE_A)
    d = tables(c)
    x = torch.from_numpy(c["x"]).cuda()
    n, A = x.shape[0], x.shape[1]
    nbytes = L.pd_plif_rings_workspace(n, d["Lg"], d["N"], d["Gl"], d["Gr"], d["H"])
    ws = sentinel((nbytes // 8,), torch.float64)
    buf = {k: sentinel(s, DTYPES[k]) for k, s in shapes(n, d).items()}
    names = ["x", "lig_idx", "type", "charge", "lig_active", "res_start", "res_atom", "ring_start", "ring_atom", "ring_residue", "G_l", "G_r",
             "halogen", "H", "thresholds", "workspace", "workspace_bytes", "bits", "ligand_bits", "ring_bits", "centroid", "normal",
             "min_centroid_dist", "counts", "P", "A", "L", "R", "N"]
    good = [P(x), P(d["lig_idx"]), P(d["types"]), P(d["charges"]), P(d["lig_active"]), P(d["res_start"]), P(d["res_atom"]), P(d["ring_start"]),
            P(d["ring_atom"]), P(d["ring_residue"]), d["Gl"], d["Gr"], P(d["halogen"]), d["H"], thr(c["thresholds"]), P(ws), nbytes] + \
           [P(buf[k]) for k in OUT] + [n, A, d["Lg"], d["R"], d["N"]]
    at = names.index

    def call(**change):
        args = list(good)
        for k, v in change.items():
            args[at(k)] = v
        return L.pd_plif_rings(*args, S())
    pointers = [k for k in names if k not in ("G_l", "G_r", "H", "workspace_bytes", "P", "A", "L", "R", "N")]
    rcs = {"null " + k: call(**{k: None}) for k in pointers}
    for k in ("P", "A", "L", "R"):
        for v in (0, -1):
            rcs[f"{k}={v}"] = call(**{k: v})
    for k in ("N", "G_l", "G_r", "H"):
        rcs[f"{k}=-1"] = call(**{k: -1})
    rcs["N>A"] = call(N=A + 1)
    for k in ("x", "lig_idx", "res_start", "res_atom", "ring_start", "ring_atom", "ring_residue", "halogen", "min_centroid_dist", "counts"):
        rcs["misaligned " + k] = call(**{k: good[at(k)] + 2})
    for k in ("workspace", "centroid", "normal"):
        rcs["misaligned " + k] = call(**{k: good[at(k)] + 4})
    for k in range(8):
        for bad in ((-1.0, NAN, float("inf"), -0.5e-30) if k < 5 else (1.5, -1.5, NAN, float("inf"))):
            t = list(thr(c["thresholds"]))
            t[k] = bad
            rcs[f"threshold {k} {bad}"] = call(thresholds=(ctypes.c_double * 8)(*t))
    rcs["workspace one byte short"] = call(workspace_bytes=nbytes - 1)
    rcs["no workspace"] = call(workspace_bytes=0)
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), {k: v for k, v in rcs.items() if v != PD_ERR_ARG}
    unsupported = {"L": call(L=1025), "A": call(A=(1 << 22) + 1), "P": call(P=65536), "R>A": call(R=A + 1), "G_l": call(G_l=65),
                   "G_r": call(G_r=4097), "H": call(H=65)}
    assert all(rc == PD_ERR_UNSUPPORTED for rc in unsupported.values()), unsupported
    torch.cuda.synchronize()
    assert all(untouched(b) for b in list(buf.values()) + [ws]), "a rejected call wrote"
    assert call() == 0
    for k, b in buf.items():
        body(b)
    # the forms without rings, halogens or receptor atoms: their arrays may be NULL
    for name in ("b_no_ligand_ring", "b_no_receptor_ring", "c_no_receptor_atom"):
        c2 = ref.make_case(name)
        d2 = tables(c2)
        assert (d2["Gl"] == 0) or (d2["Gr"] == 0)
        check(name + " NULL arrays", launch(L, c2["x"], c2, d2), ref.restate(c2))          # `launch` passes NULL for every empty array
    c3 = dict(ref.make_case("c_no_receptor_atom"), lig_rings=[], halogens=[])
    d3 = tables(c3)
    assert d3["Gl"] == d3["Gr"] == d3["H"] == d3["N"] == 0
    out = launch(L, c3["x"], c3, d3)
    assert not out["bits"].any() and not out["ligand_bits"].any() and not out["counts"].any() and bool(torch.isinf(out["min_centroid_dist"]).all())


# ------------------------------------------------------------------ RingInteractions, graph capture
def ri_of(c, device="cuda"):
    from physdock_amd.ring_interactions import RingInteractions
    local = {int(a): i for i, a in enumerate(c["lig_idx"])}
    return RingInteractions.from_tables(c["types"], c["charges"], c["lig_idx"], c["rec_mask"], c["residue_of"],
                                        ligand_rings=[[local[int(a)] for a in r] for r in c["lig_rings"]], receptor_rings=c["rec_rings"],
                                        halogens=c["halogens"], n_residues=c["n_residues"], ligand_active=c["lig_active"],
                                        thresholds=c["thresholds"], device=device)


def within_one_ulp(dev, want):
    dev, want = np.asarray(dev, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return bool((np.abs(dev.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all())


def test_the_class_agrees_with_the_c_abi_and_captures_into_a_graph(L):
    c = ref.make_case("e_P66")
    f = ri_of(c)
    x = torch.from_numpy(c["x"]).cuda()
    raw = launch(L, c["x"], c)
    out = f.fingerprint(x)
    assert set(out) == set(OUT) and all(t.is_cuda for t in out.values()) and all(out[k].dtype == DTYPES[k] for k in OUT)
    assert all(tuple(out[k].shape) == s for k, s in shapes(66, tables(c)).items())
    assert same(out, raw)
    with pytest.raises(ValueError, match="pose atoms"):
        f.fingerprint(x[:, :-1])
    # compare, pairwise and satisfies on ring bytes: the integer numpy of tests/plif_ref.py
    host = out["bits"].cpu().numpy()
    for kinds, mask in ((None, 31), (("pi_parallel", "pi_tshaped"), 3), ("halogen_bond", 16)):
        t = f.pairwise(out["bits"], kinds=kinds)
        assert t.shape == (66, 66) and torch.equal(t, t.T) and bool((t.diagonal() == 1.0).all())
        assert within_one_ulp(t.cpu().numpy(), plif_ref.pairwise(host, mask)), kinds
        for p in (0, 17, 65):
            got, want = f.compare(out["bits"], out["bits"][p], kinds=kinds), plif_ref.compare(host, host[p], mask)
            assert np.array_equal(got["shared"].cpu().numpy(), want["shared"]) and np.array_equal(got["n_pose"].cpu().numpy(), want["n_pose"])
            assert int(got["n_reference"]) == want["n_reference"] and within_one_ulp(got["recovery"].cpu().numpy(), want["recovery"])
            assert within_one_ulp(got["tanimoto"].cpu().numpy(), want["tanimoto"]) and torch.equal(got["tanimoto"], t[p])
    by_x = f.compare(out["bits"], x[0])
    assert same(by_x, f.compare(out["bits"], out["bits"][0])) and same(by_x, f.compare(out["bits"], host[0]))
    shown = [(int(s), ref.RING_KIND_NAMES[k]) for s in range(14) for k in range(5) if host[0, s] >> k & 1]
    ok = f.satisfies(out["bits"], shown)
    assert len(shown) == 5 and ok.dtype == torch.bool and ok.is_cuda and bool(ok[0]) and not bool(ok.all())
    assert ok.tolist() == [bool(((host[p] & host[0]) == host[0]).all()) for p in range(66)]
    assert f.satisfies(out["bits"], [(0, "pi_parallel")]).tolist() == [bool(host[p, 0] & 1) for p in range(66)]
    assert f.satisfies(out["bits"], []).tolist() == [True] * 66
    assert f.describe(out["bits"][0]) == [(s, [ref.RING_KIND_NAMES[k] for k in range(5) if host[0, s] >> k & 1]) for s in range(14) if host[0, s]]
    # combined: the six kinds and the five side by side; pairwise over the concatenated rows is the Tanimoto over all eleven
    rng = np.random.default_rng(5)
    six = torch.from_numpy((rng.integers(0, 64, host.shape) & rng.integers(0, 64, host.shape)).astype(np.uint8)).cuda()
    both = f.combined(six, out["bits"])
    assert both.shape == (66, 28) and torch.equal(both[:, :14], six) and torch.equal(both[:, 14:], out["bits"])
    t11 = f.pairwise_combined(six, out["bits"])
    rows = np.concatenate([six.cpu().numpy(), host], 1).astype(np.int64)
    shared = plif_ref.popcount8(rows[:, None, :] & rows[None, :, :]).sum(-1)
    cnt = plif_ref.popcount8(rows).sum(-1)
    assert within_one_ulp(t11.cpu().numpy(), plif_ref.ratio(shared, cnt[:, None] + cnt[None, :] - shared))
    raw_t = torch.empty(66, 66, device="cuda")
    assert L.pd_plif_pairwise(P(both.contiguous()), 63, P(raw_t), 66, 28, S()) == 0 and torch.equal(raw_t, t11)
    # capture, then replay on other coordinates
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    xs = x.clone()
    with torch.cuda.stream(s):
        f.fingerprint(xs)
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        captured = f.fingerprint(xs)
    xs.copy_(x.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    assert same(captured, {k: v.flip(0) for k, v in out.items()})


# ------------------------------------------------------------------ redock, redock_many
@pytest.fixture(scope="module")
def small(small_model_inputs):
    from physdock_amd import PhysDock
    cfg, P_, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P_, strict=True)
    return model.cuda().eval(), {k: v.cuda() for k, v in batch.items()}, cfg


def same_result(a, b):
    """two redock results: the same keys, bit-equal tensors, equal everything else"""
    def eq(u, w):
        if isinstance(u, torch.Tensor):
            return isinstance(w, torch.Tensor) and torch.equal(u, w)
        if isinstance(u, dict):
            return isinstance(w, dict) and set(u) == set(w) and all(eq(u[k], w[k]) for k in u)
        return u == w
    return eq(a, b)


def test_redock_reports_the_ring_interactions_and_changes_nothing_else(small):
    from physdock_amd import driver
    from physdock_amd.interactions import InteractionFingerprint
    from physdock_amd.ring_interactions import RingInteractions
    model, dbatch, _ = small
    n_lig = int(driver.ligand_atom_mask(dbatch).sum())
    bonds = [(i, i + 1) for i in range(n_lig - 1)]
    fp = InteractionFingerprint.from_batch(dbatch, bonds)
    # the fixture carries no names: the ligand's first atoms as a ring, the first receptor residue with three atoms or more as one,
    # every receptor oxygen-like atom an acceptor and every fifth receptor atom a cation, so that every family of pairs runs
    heavy = np.nonzero(fp.lig_active)[0]
    assert len(heavy) >= 4
    sizes = np.diff(fp.res_start)
    s0 = int(np.nonzero(sizes >= 3)[0][0])
    rec_ring = fp.res_atom[fp.res_start[s0]:fp.res_start[s0] + min(int(sizes[s0]), 6)].tolist()
    types, charges = fp.types.copy(), fp.charges.copy()
    rec = np.nonzero(fp.rec_mask)[0]
    types[rec[::3]] |= ref.ACCEPTOR
    charges[rec[::5]] |= ref.CATION
    charges[fp.ligand_idx[heavy[-1]]] = ref.CATION
    ri = RingInteractions.from_tables(types, charges, fp.ligand_idx, fp.rec_mask, fp.residue_of, ligand_rings=[heavy[:3].tolist()],
                                      receptor_rings=[rec_ring], halogens=[(int(heavy[3]), int(heavy[2]))], n_residues=fp.n_residues,
                                      ligand_active=fp.lig_active, device="cuda")
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, dbatch, **kw)
    out = driver.redock(model, dbatch, ring_interactions=ri, **kw)
    assert "x_gt" in dbatch and set(out) == set(plain) | {"ring_interactions", "ring_interaction_recovery"}
    assert same_result({k: out[k] for k in plain}, plain)
    assert set(out["ring_interactions"]) == set(OUT) and out["ring_interactions"]["bits"].shape == (4, ri.n_residues)
    assert same(out["ring_interactions"], ri.fingerprint(out["poses"]))
    assert same(out["ring_interaction_recovery"], ri.compare(out["ring_interactions"]["bits"], dbatch["x_gt"].float()))
    assert set(out["ring_interaction_recovery"]) == {"shared", "n_pose", "n_reference", "recovery", "tanimoto"}
    # the kept poses against the restatement (acceptance rule; a byte may be open here: the poses are not designed)
    host = dict(x=out["poses"].cpu().numpy(), lig_idx=ri.ligand_idx, types=ri.types, charges=ri.charges, lig_active=ri.lig_active,
                rec_mask=ri.rec_mask, residue_of=ri.residue_of, n_residues=ri.n_residues, thresholds=ri.threshold_values,
                lig_rings=[ri.ligand_idx[heavy[:3]].tolist()], rec_rings=[rec_ring], rec_ring_residue=[s0], halogens=ri.halogens.tolist())
    check("redock poses", out["ring_interactions"], ref.restate(host))
    both = driver.redock(model, dbatch, ring_interactions=ri, interactions=fp, **kw)
    assert set(both) == set(plain) | {"ring_interactions", "ring_interaction_recovery", "interactions", "interaction_recovery"}
    assert same(both["ring_interactions"], out["ring_interactions"]) and same(both["ring_interaction_recovery"], out["ring_interaction_recovery"])
    six = driver.redock(model, dbatch, interactions=fp, **kw)
    assert same(both["interactions"], six["interactions"]) and same(both["interaction_recovery"], six["interaction_recovery"])
    many = driver.redock_many(model, [(dbatch, {"ring_interactions": ri})], **kw)    # one system: the sequential path
    assert same_result({k: many[0][k] for k in plain}, plain) and same(many[0]["ring_interactions"], out["ring_interactions"])
    assert same(many[0]["ring_interaction_recovery"], out["ring_interaction_recovery"])
    grouped = driver.redock_many(model, [(dbatch, {"ring_interactions": ri})], group=1, **kw)
    assert set(grouped[0]) == set(out) and same(grouped[0]["ring_interactions"], ri.fingerprint(grouped[0]["poses"]))
    assert same(grouped[0]["ring_interaction_recovery"], ri.compare(grouped[0]["ring_interactions"]["bits"], dbatch["x_gt"].float()))
