"""pd_place_hydrogens and pd_hydrogen_bonds (csrc/hydrogens.hip) straight on the C ABI, Hydrogens.place / .hbonds / .compare /
.pdb_template, and the hydrogens keyword of redock / redock_many.

The yardstick is the float64 restatement tests/hydrogens_ref.py.  `placed` and `rotor_choice` are compared exactly.  `x_h` is compared
with the restatement rounded to fp32 and may differ by at most ONE fp32 ulp of the coordinate: both sides compute in float64 with
errors near 1e-15, so only the final rounding can fall the other way (the largest difference seen is printed, one `ULP | ...` line
per case, pytest -s).  The bytes and counts of pd_hydrogen_bonds are compared exactly with the restatement FED THE DEVICE'S OWN x_h;
tests/test_hydrogens_cpu.py asserts that no rotor of a case is within 1e-6 A of a tie and no bond condition within 1e-9 of its
threshold, and the second is asserted again here on the device's hydrogens.  Output buffers are one row longer than needed and
pre-filled with a sentinel (bytes 0xA5 - the kernels set bits 0 and 1 only -, NaN, -7777).

Case c crosses every block and stride of the kernels: more rows than PLACE_BLOCK = 128, more acceptors on either side than the 64
lanes that stride them, more residues, ligand atoms and rows than the 64 threads of the fold, rotor groups of one and three."""
import ctypes

import numpy as np
import pytest
import torch

import hydrogens_ref as ref

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN = float("nan")
BYTE, INT = 0xA5, -7777
PLACE_OUT = dict(x_h=torch.float32, placed=torch.uint8, rotor_choice=torch.int32)
BOND_OUT = dict(bits=torch.uint8, ligand_bits=torch.uint8, h_bits=torch.uint8, counts=torch.int32)


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
    return (ctypes.c_double * 2)(float(values[0]), float(np.cos(np.deg2rad(values[1]))))


def tables(c):
    """a case's tables on the device, every index the kernels would follow checked to be inside its array first"""
    t, d = c["table"], ref.derived(c)
    A, R, Lg, H = c["x"].shape[1], int(c["n_residues"]), len(c["lig_idx"]), len(c["table"]["parent"])
    G, NA, HP = len(d["group_h"]), d["NA_r"] + d["NA_l"], d["HP_l"] + d["HP_r"]
    assert 1 <= H <= 65535 and 0 <= t["parent"].min() and t["parent"].max() < A and -1 <= t["ref"].min() and t["ref"].max() < A
    assert t["ref"].shape == (H, 3) and t["mode"].max() <= 3 and all(len(t[k]) == H for k in ("mode", "length", "a", "b", "group"))
    assert d["group_h"].shape == (G, 3) and d["group_h"].max(initial=-1) < H and (d["group_h"][:, 0] >= 0).all() and G <= H
    assert len(d["acc"]) == NA <= A and (NA == 0 or (0 <= d["acc"].min() and d["acc"].max() < A)) and d["NA_l"] <= 1024
    assert len(d["polar"]) == HP <= H and (HP == 0 or (0 <= d["polar"].min() and d["polar"].max() < H))
    assert len(d["polar_slot"]) == H and d["polar_slot"].max(initial=-1) < HP and len(d["lig_acc_slot"]) == Lg <= 1024 and d["lig_acc_slot"].max(initial=-1) < d["NA_l"]
    for start, n in ((d["racc_start"], d["NA_r"]), (d["rh_start"], d["HP_r"])):
        assert len(start) == R + 1 and start[0] == 0 and start[-1] == n and (np.diff(start) >= 0).all()
    assert 0 <= c["lig_idx"].min() and c["lig_idx"].max() < A and 1 <= R <= A
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()
    dev = {k: up(t[k], dt) for k, dt in (("parent", np.int32), ("ref", np.int32), ("mode", np.uint8), ("length", np.float32), ("a", np.float32),
                                         ("b", np.float32))}
    dev.update({k: up(d[k], np.uint8 if k == "side" else np.int32) for k in ("side", "group_h", "acc", "racc_start", "lig_acc_slot", "polar",
                                                                            "rh_start", "polar_slot")})
    dev.update(lig_idx=up(c["lig_idx"], np.int32), G=G, H=H, R=R, Lg=Lg, A=A, NA_r=d["NA_r"], NA_l=d["NA_l"], HP_l=d["HP_l"], HP_r=d["HP_r"])
    return dev


def place_call(L, poses, d, buf, d_da=4.1, orient=1, **over):
    a = dict(G=d["G"], NA_r=d["NA_r"], NA_l=d["NA_l"], P=poses.shape[0], A=poses.shape[1], H=d["H"], parent=P(d["parent"]), x_h=P(buf["x_h"]),
             group_h=P(d["group_h"]), rotor_choice=P(buf["rotor_choice"]), acc=P(d["acc"]), x=P(poses))
    a.update(over)
    return L.pd_place_hydrogens(a["x"], a["parent"], P(d["ref"]), P(d["mode"]), P(d["length"]), P(d["a"]), P(d["b"]), P(d["side"]), a["group_h"],
                                a["G"], a["acc"], a["NA_r"], a["NA_l"], d_da, orient, a["x_h"], P(buf["placed"]), a["rotor_choice"], a["P"],
                                a["A"], a["H"], S())


def place(L, x, c, d, orient=1):
    """one pd_place_hydrogens call into sentinel buffers -> (device x, dict of the bodies)"""
    x = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    n = x.shape[0]
    buf = {"x_h": sentinel((n, d["H"], 3), torch.float32), "placed": sentinel((n, d["H"]), torch.uint8),
           "rotor_choice": sentinel((n, d["G"]), torch.int32)}
    rc = place_call(L, x, d, buf, float(c["thresholds"][0]), orient)
    assert rc == 0, rc
    return x, {k: body(v, nan_ok=k == "x_h") for k, v in buf.items()}


def bonds_call(lib, poses, h, d, t, ws, ws_bytes, buf, **over):
    a = dict(HP_l=d["HP_l"], HP_r=d["HP_r"], NA_r=d["NA_r"], NA_l=d["NA_l"], P=poses.shape[0], A=poses.shape[1], H=d["H"], L=d["Lg"], R=d["R"], x=P(poses),
             bits=P(buf["bits"]), polar=P(d["polar"]), acc=P(d["acc"]), workspace=P(ws), counts=P(buf["counts"]))
    a.update(over)
    return lib.pd_hydrogen_bonds(a["x"], P(h["x_h"]), P(h["placed"]), P(d["parent"]), a["polar"], a["HP_l"], a["HP_r"], P(d["polar_slot"]), a["acc"],
                               a["NA_r"], a["NA_l"], P(d["racc_start"]), P(d["rh_start"]), P(d["lig_idx"]), P(d["lig_acc_slot"]), t, a["workspace"],
                               ws_bytes, a["bits"], P(buf["ligand_bits"]), P(buf["h_bits"]), a["counts"], a["P"], a["A"], a["H"], a["L"], a["R"], S())


def bond_buffers(n, d):
    return {"bits": sentinel((n, d["R"]), torch.uint8), "ligand_bits": sentinel((n, d["Lg"]), torch.uint8),
            "h_bits": sentinel((n, d["H"]), torch.uint8), "counts": sentinel((n, 2), torch.int32)}


def bonds(L, x, h, c, d):
    """one pd_hydrogen_bonds call on the device's own hydrogens h (contiguous copies of the bodies) into sentinel buffers"""
    n = x.shape[0]
    h = {k: h[k].contiguous() for k in ("x_h", "placed")}
    nbytes = L.pd_hydrogen_bonds_workspace(n, d["HP_l"], d["HP_r"], d["NA_r"], d["NA_l"])
    assert nbytes >= 8 and nbytes % 8 == 0
    ws = sentinel((nbytes // 8,), torch.float64)
    buf = bond_buffers(n, d)
    rc = bonds_call(L, x, h, d, thr(c["thresholds"]), ws, nbytes, buf)
    assert rc == 0, rc
    body(ws, nan_ok=True)                                              # nothing behind the workspace was written
    return {k: body(v) for k, v in buf.items()}


def ulps(dev, want):
    """the largest |dev - want| in units of the fp32 spacing at want, over the finite entries; NaN must match NaN"""
    dev, want = np.asarray(dev, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert np.array_equal(np.isnan(dev), np.isnan(want)), "NaN exactly where the restatement has one"
    ok = ~np.isnan(want)
    return float((np.abs(dev[ok].astype(np.float64) - want[ok].astype(np.float64)) / np.spacing(np.abs(want[ok])).astype(np.float64)).max()) if ok.any() else 0.0


def same(a, b, keys=None):
    """bit-equal tensors (NaN equal to NaN: a hydrogen that is not placed)"""
    eq = lambda u, w: torch.equal(torch.nan_to_num(u, nan=-1e30), torch.nan_to_num(w, nan=-1e30)) if u.is_floating_point() else torch.equal(u, w)
    return all(eq(a[k], b[k]) for k in (keys or a))


def check_bonds(case, c, x_h, placed, out):
    """the device's bytes and counts against the restatement fed the device's own hydrogens"""
    want = ref.hbonds(c, x_h.cpu().numpy(), placed.cpu().numpy())
    assert want["margin"] >= 1e-9, (case, "a bond condition of the device's hydrogens is at its threshold", want["margin"])
    for k in BOND_OUT:
        dev = out[k].cpu().numpy()
        assert dev.shape == want[k].shape and dev.dtype == want[k].dtype and np.array_equal(dev, want[k]), (case, k)
    assert not (out["bits"] >> 2).any() and not (out["ligand_bits"] >> 2).any() and not (out["h_bits"] >> 2).any()
    return want


# ------------------------------------------------------------------ cases a - c on the C ABI
@pytest.mark.parametrize("name", ref.CASES)
def test_kernels_against_float64(L, name):
    c, want = ref.make_case(name), ref.reference(name)
    d = tables(c)
    x, h = place(L, c["x"], c, d)
    assert np.array_equal(h["placed"].cpu().numpy(), want["placed"]) and np.array_equal(h["rotor_choice"].cpu().numpy(), want["rotor_choice"])
    u = ulps(h["x_h"].cpu().numpy(), want["x_h"])
    print(f"ULP | pd_place_hydrogens | {name} | largest difference {u:.2f} fp32 ulp |")
    assert u <= 1.0, (name, u)
    off = h["placed"] == 0
    assert bool(torch.isnan(h["x_h"][off]).all()) and not bool(torch.isnan(h["x_h"][~off]).any()), "NaN exactly where nothing is placed"
    out = bonds(L, x, h, c, d)
    check_bonds(name, c, h["x_h"], h["placed"], out)
    assert not out["h_bits"][off].any(), "a hydrogen that is not placed appears in no bit"
    assert not out["ligand_bits"][:, torch.from_numpy(c["lig_active"] == 0).cuda()].any()
    # bit-identical from launch to launch
    x2, h2 = place(L, c["x"], c, d)
    assert same(h2, h) and same(bonds(L, x2, h2, c, d), out)
    # the default angles: no rotor turns, everything else is where it was
    _, plain = place(L, c["x"], c, d, orient=0)
    want0 = ref.place(c, orient=False)
    assert not plain["rotor_choice"].any() and torch.equal(plain["placed"], h["placed"]) and ulps(plain["x_h"].cpu().numpy(), want0["x_h"]) <= 1.0
    fixed = torch.from_numpy(c["table"]["group"] < 0).cuda()
    assert same({"x_h": plain["x_h"][:, fixed]}, {"x_h": h["x_h"][:, fixed]})
    check_bonds(name + " default angles", c, plain["x_h"], plain["placed"], bonds(L, x, plain, c, d))


@pytest.mark.parametrize("name", ref.CASES)
def test_a_pose_alone_is_the_pose_inside_a_batch(L, name):
    c = ref.make_case(name)
    d = tables(c)
    n = c["x"].shape[0]
    x, h = place(L, c["x"], c, d)
    out = bonds(L, x, h, c, d)
    for p in range(n):
        x1, h1 = place(L, c["x"][p:p + 1], c, d)
        o1 = bonds(L, x1, h1, c, d)
        trio = np.stack([c["x"][(p + 1) % n], c["x"][p], c["x"][(p + 1) % n]])
        x3, h3 = place(L, trio, c, d)
        o3 = bonds(L, x3, h3, c, d)
        for a, b in ((h1, h), (o1, out)):
            assert same({k: v[0] for k, v in a.items()}, {k: v[p] for k, v in b.items()}), (name, p, "alone")
        for a, b in ((h3, h), (o3, out)):
            assert same({k: v[1] for k, v in a.items()}, {k: v[p] for k, v in b.items()}), (name, p, "as row 1 of 3")


def test_case_a_finds_what_it_was_built_for(L):
    c = ref.make_case("a_hand_P2")
    d = tables(c)
    x, h = place(L, c["x"], c, d)
    out = bonds(L, x, h, c, d)
    assert h["rotor_choice"].tolist() == [[ref.A_OH_CHOICE[p], ref.A_NH3_CHOICE[p]] for p in range(2)] and bool(h["placed"].all())
    assert out["bits"].tolist() == [[2, 1, 0]] * 2 and out["counts"].tolist() == [[1, 1]] * 2
    assert out["ligand_bits"].tolist() == [[0, 0, 0, 0, 0, 0, 1, 0, 0, 2]] * 2 and out["h_bits"][:, 7].tolist() == [1, 1]
    # an angle no bond reaches: every byte is 0; a distance nothing reaches: no rotor turns
    tight = dict(c, thresholds=(4.1, 180.0))
    assert not any(v.any() for v in bonds(L, x, h, tight, d).values())
    _, near = place(L, c["x"], dict(c, thresholds=(1.0, 100.0)), d)
    assert not near["rotor_choice"].any()


def test_the_empty_forms(L):
    """no rotor group, no acceptor, no polar row: the arrays may be NULL, every byte is 0"""
    c = ref.make_case("a_hand_P2")
    t = c["table"]
    bare = dict(c, types=(c["types"] & 15).astype(np.uint8), table=dict(t, group=np.full_like(t["group"], -1)))
    d = tables(bare)
    assert d["G"] == 0 and d["NA_r"] == d["NA_l"] == 0 and d["HP_l"] > 0
    x, h = place(L, bare["x"], bare, d)
    assert h["rotor_choice"].shape == (2, 0) and np.array_equal(h["placed"].cpu().numpy(), ref.place(bare)["placed"])
    assert ulps(h["x_h"].cpu().numpy(), ref.place(bare)["x_h"]) <= 1.0
    out = bonds(L, x, h, bare, d)
    assert not any(v.any() for v in out.values())
    carbon = dict(bare, types=np.zeros_like(c["types"]))
    d2 = tables(carbon)
    assert d2["HP_l"] == d2["HP_r"] == 0
    assert not any(v.any() for v in bonds(L, x, h, carbon, d2).values())


def test_error_codes(L):
    c = ref.make_case("a_hand_P2")
    d = tables(c)
    x = torch.from_numpy(c["x"]).cuda()
    n = x.shape[0]
    buf = {"x_h": sentinel((n, d["H"], 3), torch.float32), "placed": sentinel((n, d["H"]), torch.uint8), "rotor_choice": sentinel((n, d["G"]), torch.int32)}
    for over, code in ((dict(P=0), PD_ERR_ARG), (dict(A=0), PD_ERR_ARG), (dict(H=0), PD_ERR_ARG), (dict(G=-1), PD_ERR_ARG), (dict(NA_r=-1), PD_ERR_ARG),
                       (dict(G=d["H"] + 1), PD_ERR_ARG), (dict(NA_r=16, NA_l=1), PD_ERR_ARG), (dict(x=None), PD_ERR_ARG), (dict(x_h=None), PD_ERR_ARG),
                       (dict(group_h=None), PD_ERR_ARG), (dict(rotor_choice=None), PD_ERR_ARG), (dict(acc=None), PD_ERR_ARG),
                       (dict(parent=P(d["parent"]) + 2), PD_ERR_ARG), (dict(x_h=P(buf["x_h"]) + 1), PD_ERR_ARG),
                       (dict(H=65536), PD_ERR_UNSUPPORTED), (dict(P=65536), PD_ERR_UNSUPPORTED), (dict(A=(1 << 22) + 1), PD_ERR_UNSUPPORTED)):
        assert place_call(L, x, d, buf, **over) == code, over
    for d_da in (-1.0, NAN, float("inf")):
        assert place_call(L, x, d, buf, d_da=d_da) == PD_ERR_ARG
    torch.cuda.synchronize()
    assert all(untouched(v) for v in buf.values()), "a rejected call writes nothing"
    assert place_call(L, x, d, buf) == 0
    h = {k: body(v, nan_ok=True).contiguous() for k, v in buf.items()}
    nbytes = L.pd_hydrogen_bonds_workspace(n, d["HP_l"], d["HP_r"], d["NA_r"], d["NA_l"])
    ws = sentinel((nbytes // 8,), torch.float64)
    out = bond_buffers(n, d)
    t = thr(c["thresholds"])
    call = lambda t_=t, nb=nbytes, **over: bonds_call(L, x, h, d, t_, ws, nb, out, **over)
    for over, code in ((dict(P=0), PD_ERR_ARG), (dict(L=0), PD_ERR_ARG), (dict(R=0), PD_ERR_ARG), (dict(H=0), PD_ERR_ARG), (dict(HP_l=-1), PD_ERR_ARG),
                       (dict(NA_l=-1), PD_ERR_ARG), (dict(NA_r=16, NA_l=1), PD_ERR_ARG), (dict(x=None), PD_ERR_ARG), (dict(bits=None), PD_ERR_ARG),
                       (dict(polar=None), PD_ERR_ARG), (dict(acc=None), PD_ERR_ARG), (dict(workspace=None), PD_ERR_ARG), (dict(workspace=P(ws) + 4), PD_ERR_ARG),
                       (dict(counts=P(out["counts"]) + 2), PD_ERR_ARG), (dict(HP_l=d["H"], HP_r=1), PD_ERR_UNSUPPORTED), (dict(L=1025), PD_ERR_UNSUPPORTED),
                       (dict(R=17), PD_ERR_UNSUPPORTED), (dict(P=65536), PD_ERR_UNSUPPORTED), (dict(H=65536), PD_ERR_UNSUPPORTED)):
        assert call(**over) == code, over
    assert call(nb=nbytes - 8) == PD_ERR_ARG, "a short workspace"
    for bad in ((-1.0, 0.0), (NAN, 0.0), (4.1, 1.5), (4.1, NAN)):
        assert call(t_=(ctypes.c_double * 2)(*bad)) == PD_ERR_ARG, bad
    torch.cuda.synchronize()
    assert all(untouched(v) for v in out.values()) and untouched(ws), "a rejected call writes nothing"
    assert call() == 0
    check_bonds("after the refusals", c, h["x_h"], h["placed"], {k: body(v) for k, v in out.items()})


# ------------------------------------------------------------------ the class
def hy_of(c, device="cuda"):
    from physdock_amd.hydrogens import Hydrogens
    return Hydrogens.from_tables(c["types"], c["lig_idx"], c["rec_mask"], c["residue_of"], c["table"], n_residues=c["n_residues"],
                                 ligand_active=c["lig_active"], thresholds=c["thresholds"], device=device)


@pytest.mark.parametrize("name", ref.CASES)
def test_the_class_is_the_kernels(L, name):
    c = ref.make_case(name)
    d = tables(c)
    x, h = place(L, c["x"], c, d)
    out = bonds(L, x, h, c, d)
    hy = hy_of(c)
    got = hy.place(x)
    A, H = x.shape[1], d["H"]
    assert set(got) == {"x_h", "placed", "rotor_choice", "x_all"} and same(got, h, PLACE_OUT)
    assert got["x_all"].shape == (x.shape[0], A + H, 3) and same({"a": got["x_all"][:, :A], "h": got["x_all"][:, A:]}, {"a": x, "h": h["x_h"]})
    full = hy.hbonds(x)
    assert set(full) == set(BOND_OUT) | set(got) and same(full, out, BOND_OUT) and same(full, got, got)
    assert same(hy.hbonds(x, placed=got), out, BOND_OUT)
    plain = hy.place(x, orient=False)
    assert not plain["rotor_choice"].any() and same(plain, place(L, c["x"], c, d, orient=0)[1], PLACE_OUT)
    with pytest.raises(ValueError, match="what `place` returned"):
        hy.hbonds(x, placed={"x_h": got["x_h"][:1], "placed": got["placed"][:1]})
    # compare: against a row, and against reference coordinates (pose 0 as the "ground truth"), which are given hydrogens first
    bits = full["bits"]
    vs = hy.compare(bits, c["x"][0])
    row = hy.compare(bits, bits[0])
    assert same(vs, row) and set(vs) == {"shared", "n_pose", "n_reference", "recovery", "tanimoto"}
    b = bits.cpu().numpy()
    pop = lambda v: np.unpackbits(v, axis=-1).sum(-1)
    assert vs["shared"].tolist() == pop(b & b[0]).tolist() and int(vs["n_reference"]) == int(pop(b[0])) > 0
    assert float(vs["recovery"][0]) == 1.0 and float(vs["tanimoto"][0]) == 1.0
    donors = hy.compare(bits, bits[0], kinds=("hbond_donor",))
    assert donors["n_pose"].tolist() == (b & 1).sum(1).tolist()
    assert bool(hy.satisfies(bits, [(int(np.nonzero(b[0] & 1)[0][0]), "hbond_donor")])[0])
    pw = hy.pairwise(bits)
    assert pw.shape == (b.shape[0], b.shape[0]) and bool((pw.diagonal() == 1).all())


def test_protonated_poses_through_the_pdb_template():
    from physdock_amd.hydrogens import Hydrogens, receptor_hydrogens_from_names
    from physdock_amd.pdbio import PdbTemplate
    from physdock_amd.scoring import receptor_types_from_names
    ser, gly = ["N", "CA", "C", "O", "CB", "OG"], ["N", "CA", "C", "O"]
    z_of = {"C": 6, "N": 7, "O": 8}
    conf = {"SER": {"ref_atom_name_chars": ser, "ref_element": [z_of[a[0]] - 1 for a in ser]},
            "GLY": {"ref_atom_name_chars": gly, "ref_element": [z_of[a[0]] - 1 for a in gly]},
            "LIG": {"ref_atom_name_chars": ["C1", "C2", "O1"], "ref_element": [5, 5, 7]}}
    meta = {"ccds": ["SER", "GLY", "LIG"], "atom_id_to_conformer_atom_id": np.array(list(range(6)) + list(range(4)) + [0, 1, 2]),
            "conformer_id_to_chunk_sizes": np.array([6, 4, 3]), "CHAIN_CLASS": ["protein", "protein", "ligand"], "CONF_META_DATA": conf,
            "residue_index": np.array([6, 7, 0]), "asym_id": np.array([0, 0, 1])}
    res, names, residue_of = ["SER"] * 6 + ["GLY"] * 4 + ["LIG"] * 3, ser + gly + ["C1", "C2", "O1"], [0] * 6 + [1] * 4 + [2] * 3
    elements = [z_of[a[0]] for a in names]
    rec = receptor_hydrogens_from_names(res[:10], names[:10], residue_of[:10])
    hy = Hydrogens.from_bonds(elements, [(0, 1), (1, 2)], [10, 11, 12], residue_of, receptor_types=receptor_types_from_names(res, names, elements),
                              receptor_hydrogens=rec, device="cuda")
    assert hy.n_hydrogens == 4 + 3 + 6
    x = torch.from_numpy(np.random.default_rng(5).normal(0.0, 4.0, (2, 13, 3)).astype(np.float32)).cuda()
    got = hy.place(x)
    assert bool(got["placed"].all())
    base = PdbTemplate(meta, device="cuda")
    full = hy.pdb_template(base)
    assert full.rows.is_cuda and (full.n_atoms, full.n_records) == (26, 26)
    blocks, heavy = full.blocks(got["x_all"]), base.blocks(x)
    x_h = got["x_h"].cpu().numpy()
    for p in range(2):
        lines, old = blocks[p].split("\n"), heavy[p].split("\n")
        assert lines[:14] == old[:14] and lines[27:] == old[14:], "the heavy-atom records and the frame are the template's, byte for byte"
        for k, line in enumerate(lines[14:27]):
            assert line[76:78] == " H" and int(line[6:11]) == 14 + k and line[:6] == ("ATOM  " if k < 7 else "HETATM")
            assert [line[30:38], line[38:46], line[46:54]] == [f"{v:8.3f}" for v in x_h[p, k]]
    hole = got["x_all"].clone()
    hole[1, 20, 0] = NAN
    with pytest.raises(ValueError, match="not finite"):
        full.blocks(hole)


# ------------------------------------------------------------------ the hydrogens keyword of redock
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


def test_redock_reports_the_hydrogens_and_changes_nothing_else(small):
    from physdock_amd import driver
    from physdock_amd.hydrogens import BISECT, Hydrogens, join_hydrogen_tables
    model, dbatch, _ = small
    n_lig = int(driver.ligand_atom_mask(dbatch).sum())
    chain = [(i, i + 1) for i in range(n_lig - 1)]
    lig = Hydrogens.from_batch(dbatch, chain)
    assert lig.receptor_typing == "elements" and lig.side.all() and lig.n_receptor_acceptors == 0
    # the fixture carries no names: every third receptor atom an acceptor, every ligand atom one too, and an N-H in the plane of
    # its two neighbours on the first atom of every residue of three atoms or more, so that both kinds of bond can form
    types = lig.types.copy()
    rec = np.nonzero(lig.rec_mask)[0]
    types[rec[::3]] |= ref.ACCEPTOR
    types[lig.ligand_idx] |= ref.ACCEPTOR
    order = rec[np.argsort(lig.residue_of[rec], kind="stable")]
    start = np.concatenate([[0], np.cumsum(np.bincount(lig.residue_of[rec], minlength=lig.n_residues))])
    trios = [order[start[s]:start[s] + 3] for s in range(lig.n_residues) if start[s + 1] - start[s] >= 3]
    assert len(trios) >= 2
    types[[t[0] for t in trios]] = ref.CLASS_N
    k = len(trios)
    rows = {"parent": np.array([t[0] for t in trios]), "ref": np.array([[t[1], t[2], -1] for t in trios]), "mode": np.full(k, BISECT),
            "length": np.full(k, 1.01), "a": np.zeros(k), "b": np.zeros(k), "group": np.full(k, -1)}
    hy = Hydrogens.from_tables(types, lig.ligand_idx, lig.rec_mask, lig.residue_of, join_hydrogen_tables(rows, lig.table), n_residues=lig.n_residues,
                               ligand_active=lig.lig_active, device="cuda")
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, dbatch, **kw)
    out = driver.redock(model, dbatch, hydrogens=hy, **kw)
    assert "x_gt" in dbatch and set(out) == set(plain) | {"hydrogens", "hbond_recovery"}
    assert same_result({k_: out[k_] for k_ in plain}, plain)
    assert set(out["hydrogens"]) == {"x_h", "placed", "bits", "counts"} and out["hydrogens"]["bits"].shape == (4, hy.n_residues)
    direct = hy.hbonds(out["poses"])
    assert same(out["hydrogens"], direct, out["hydrogens"])
    assert same(out["hbond_recovery"], hy.compare(direct["bits"], dbatch["x_gt"].float()))
    assert set(out["hbond_recovery"]) == {"shared", "n_pose", "n_reference", "recovery", "tanimoto"}
    # the kept poses against the restatement, fed the device's hydrogens
    host = dict(x=out["poses"].cpu().numpy(), lig_idx=hy.ligand_idx, lig_active=hy.lig_active, rec_mask=hy.rec_mask, residue_of=hy.residue_of,
                n_residues=hy.n_residues, types=hy.types, table=hy.table, thresholds=hy.threshold_values)
    want = ref.place(host)
    assert np.array_equal(direct["placed"].cpu().numpy(), want["placed"]) and ulps(direct["x_h"].cpu().numpy(), want["x_h"]) <= 1.0
    assert np.array_equal(direct["rotor_choice"].cpu().numpy(), want["rotor_choice"]) or want["rotor_margin"].min() < 1e-6
    bonds_want = ref.hbonds(host, direct["x_h"].cpu().numpy(), direct["placed"].cpu().numpy())
    assert bonds_want["margin"] < 1e-9 or all(np.array_equal(direct[k_].cpu().numpy(), bonds_want[k_]) for k_ in BOND_OUT)
    many = driver.redock_many(model, [(dbatch, {"hydrogens": hy})], **kw)            # one system: the sequential path
    assert same_result({k_: many[0][k_] for k_ in plain}, plain) and same(many[0]["hydrogens"], out["hydrogens"])
    assert same(many[0]["hbond_recovery"], out["hbond_recovery"])
    grouped = driver.redock_many(model, [(dbatch, {"hydrogens": hy})], group=1, **kw)
    assert set(grouped[0]) == set(out) and same(grouped[0]["hydrogens"], hy.hbonds(grouped[0]["poses"]), grouped[0]["hydrogens"])
    # a table over another number of atoms is refused before anything is sampled
    with pytest.raises(ValueError, match="pose atoms"):
        driver.redock(model, dbatch, hydrogens=hy_of(ref.make_case("a_hand_P2")), **kw)
    with pytest.raises(ValueError, match="pose atoms"):
        driver.redock_many(model, [(dbatch, {"hydrogens": hy_of(ref.make_case("a_hand_P2"))})], group=1, **kw)
