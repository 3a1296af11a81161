"""pd_receptor_geometry / pd_receptor_dihedrals (csrc/receptor_geometry.hip) straight on the C ABI, ReceptorGeometry.check / dihedrals /
chi_recovery, and redock(receptor_geometry=).

The yardstick is the float64 numpy restatement tests/receptor_geometry_ref.py.  The fp32 ratio columns (0 - 4) and the bond / 1-3 term
values follow the rule of tests/test_validity_gpu.py: |dev - ref64| <= 4 E + 8 ulp32(max|ref64|) with E = max|ref32 - ref64|; the
plane column uses PLANE_TOL = 1e-6; dihedrals, the twist column and the signed volumes are double arithmetic stored as fp32 and bounded
by one ulp32 of 180 degrees.  Integer outputs, flags, bits and worst_pair must be equal exactly - each case first asserts on the
restatement that no value lies within its bound of its threshold and that the minimal clash pair is unique beyond it
(receptor_geometry_cases.margins_hold).  One `ENVELOPE | ...` line is printed per column (pytest -s).  Output buffers are one row
longer than needed and pre-filled with a sentinel (NaN, -7 for integers)."""
import numpy as np
import pytest
import torch

import receptor_geometry_cases as cases
import receptor_geometry_ref as ref

pytestmark = pytest.mark.gpu

TOL_FACTOR, TOL_FLOOR_ULPS = 4.0, 8.0
PLANE_TOL = 1e-6
DOUBLE_TOL = float(np.nextafter(np.float32(180.0), np.float32(np.inf)) - np.float32(180.0))          # 1.53e-5
PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN = float("nan")
COLUMNS = ("bond min", "bond max", "angle min", "angle max", "clash", "planarity", "twist", "wrong centres")
TABLES = ("radius_signed", "excl_start", "excl_atom", "term_atoms", "term_ref", "res_term_start", "res_term", "res_atom_start", "res_atom")


def _ulp32(v):
    s = np.float32(abs(v))
    return float(np.nextafter(s, np.float32(np.inf)) - s)


def rule_bound(r32, r64):
    r32, r64 = np.asarray(r32, dtype=np.float64), np.asarray(r64, dtype=np.float64)
    fin = np.isfinite(r64)
    if not fin.any():
        return 0.0, 0.0
    E = float(np.abs(r32[fin] - r64[fin]).max())
    return TOL_FACTOR * E + TOL_FLOOR_ULPS * _ulp32(float(np.abs(r64[fin]).max())), E


def sentinel(*shape, dtype=torch.float32):
    fill = NAN if dtype.is_floating_point else (249 if dtype == torch.uint8 else -7)
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")


def is_sentinel(t):
    return torch.isnan(t) if t.dtype.is_floating_point else t == (249 if t.dtype == torch.uint8 else -7)


def body(buf, written=True):
    torch.cuda.synchronize()
    assert is_sentinel(buf[-1]).all(), "the row behind the output was written"
    if written and buf[:-1].numel():
        assert not is_sentinel(buf[:-1]).any(), "an output element kept its sentinel"
    return buf[:-1]


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


def thresholds(**kw):
    from physdock_amd._lib import ReceptorThresholds
    t = dict(ref.DEFAULT_THRESHOLDS)
    t.update(kw)
    return ReceptorThresholds(*[t[k] for k in list(ref.DEFAULT_THRESHOLDS)[:8]])


def check_tables(g, A):
    """the kernels trust their tables: every index they would follow is inside its array"""
    R, T = g.n_residues, g.n_terms
    assert len(g.radius_signed) == A and len(g.excl_start) == A + 1 and g.excl_start[0] == 0 and g.excl_start[-1] == len(g.excl_atom)
    assert (np.diff(g.excl_start) >= 0).all() and (g.excl_atom.size == 0 or (0 <= g.excl_atom.min() and g.excl_atom.max() < A))
    assert g.term_atoms.shape == (T, 10) and len(g.term_ref) == T == sum(g.term_counts)
    assert T == 0 or (-1 <= g.term_atoms.min() and g.term_atoms.max() < A)
    nb, na, nc, npep, ng = g.term_counts
    assert (g.term_atoms[:nb + na, :2] >= 0).all() and (g.term_atoms[nb + na:nb + na + nc + npep, :4] >= 0).all()
    assert (g.term_ref[:nb + na] > 0).all()
    for start, flat, n in ((g.res_term_start, g.res_term, T), (g.res_atom_start, g.res_atom, A)):
        assert len(start) == R + 1 and start[0] == 0 and start[-1] == len(flat) and (np.diff(start) >= 0).all()
        assert flat.size == 0 or (0 <= flat.min() and flat.max() < n)
    assert g.dih.shape == (R, 7, 4) and (g.dih.size == 0 or (-1 <= g.dih.min() and g.dih.max() < A))


def launch(L, g, x, thr=None):
    """one pd_receptor_geometry call into sentinel buffers -> dict of the buffers (tail row included)"""
    x = torch.as_tensor(x).cuda().contiguous()
    n, A, R, T = x.shape[0], x.shape[1], g.n_residues, g.n_terms
    assert A <= 4096 and R <= 4096 and x.dtype == torch.float32
    check_tables(g, A)
    d = {k: torch.from_numpy(np.ascontiguousarray(getattr(g, k))).cuda() for k in TABLES}
    ws = torch.empty(L.pd_receptor_geometry_workspace_numel(n, A), dtype=torch.int64, device="cuda")
    o = dict(val=sentinel(n, 8), worst=sentinel(n, 2, dtype=torch.int32), counts=sentinel(n, 7, dtype=torch.int32),
             flags=sentinel(n, dtype=torch.int32), residue_flags=sentinel(n, R, dtype=torch.uint8), atom_clash=sentinel(n, A, dtype=torch.uint8),
             term_val=sentinel(n, T), term_fail=sentinel(n, T, dtype=torch.uint8))
    rc = L.pd_receptor_geometry(P(x), P(d["radius_signed"]), P(d["excl_start"]), P(d["excl_atom"]), P(d["term_atoms"]), P(d["term_ref"]),
                                *g.term_counts, P(d["res_term_start"]), P(d["res_term"]), P(d["res_atom_start"]), P(d["res_atom"]),
                                thr or thresholds(), P(ws), P(o["val"]), P(o["worst"]), P(o["counts"]), P(o["flags"]), P(o["residue_flags"]),
                                P(o["atom_clash"]), P(o["term_val"]), P(o["term_fail"]), n, A, R, S())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return o


def launch_dihedrals(L, g, x):
    x = torch.as_tensor(x).cuda().contiguous()
    n, A, R = x.shape[0], x.shape[1], g.n_residues
    ang = sentinel(n, R, 7)
    ang[:-1] = 7777.0                                                   # NaN is a legitimate result here
    assert L.pd_receptor_dihedrals(P(x), P(torch.from_numpy(g.dih).cuda()), P(ang), n, A, R, S()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(ang[-1]).all() and not (ang[:-1] == 7777.0).any()
    return ang[:-1]


def angle_error(dev, r64):
    """largest difference of two angle arrays in degrees, across the +-180 seam; the NaN patterns must be equal"""
    assert np.array_equal(np.isnan(dev), np.isnan(r64))
    d = np.abs(np.remainder(dev - r64 + 180.0, 360.0) - 180.0)
    return float(np.nanmax(d)) if (~np.isnan(d)).any() else 0.0


def compare(tag, L, g, x, check_class=True):
    """every output of the device against the restatement -> (device outputs, float64 restatement)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    t = cases.host_tables(g)
    r64, r32 = ref.receptor_geometry(x, t), ref.receptor_geometry(x, t, fp32=True)
    nb, na, nc, npep, ng = g.term_counts
    ratio_terms = slice(0, nb + na)
    term_bound, _ = rule_bound(r32["term_val"][:, ratio_terms], r64["term_val"][:, ratio_terms])
    pair_bound, _ = rule_bound(r32["val"][:, 4], r64["val"][:, 4])
    margin = cases.margins_hold(r64, t, dict(ratio=max(term_bound, pair_bound, 8 * _ulp32(1.0)), double=DOUBLE_TOL))
    assert np.array_equal(r64["flags"], r32["flags"]) and np.array_equal(r64["worst"], r32["worst"])
    o = launch(L, g, x)
    val = body(o["val"]).cpu().double().numpy()
    for c in range(8):
        fin = np.isfinite(r64["val"][:, c])
        assert np.array_equal(val[~fin, c], r64["val"][~fin, c]), (tag, COLUMNS[c], val[:, c], r64["val"][:, c])
        bound, E = (PLANE_TOL, 0.0) if c == 5 else (DOUBLE_TOL, 0.0) if c == 6 else (0.0, 0.0) if c == 7 else rule_bound(r32["val"][:, c], r64["val"][:, c])
        if not fin.any():
            continue
        err = float(np.abs(val[fin, c] - r64["val"][fin, c]).max())
        print(f"ENVELOPE | pd_receptor_geometry | {tag} {COLUMNS[c]} | {E:.2e} | {err:.2e} | {bound:.2e} | {err / bound if bound else 0.0:.2f} |")
        assert err <= bound, (tag, COLUMNS[c], "E", E, "err", err, "bound", bound)
    tv = body(o["term_val"]).cpu().double().numpy()
    fin = np.isfinite(r64["term_val"])
    assert np.array_equal(tv[~fin], r64["term_val"][~fin]), tag
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(tv - r64["term_val"]), 0.0)
    for name, sl, bound in (("bond / 1-3 terms", ratio_terms, term_bound), ("signed volumes", slice(nb + na, nb + na + nc), DOUBLE_TOL),
                            ("twists", slice(nb + na + nc, nb + na + nc + npep), DOUBLE_TOL), ("plane terms", slice(nb + na + nc + npep, None), PLANE_TOL)):
        if err[:, sl].size:
            e = float(err[:, sl].max())
            print(f"ENVELOPE | pd_receptor_geometry | {tag} {name} | - | {e:.2e} | {bound:.2e} | {e / bound if bound else 0.0:.2f} |")
            assert e <= bound, (tag, name, e, bound)
    for k, rk in (("worst", "worst"), ("counts", "counts"), ("flags", "flags"), ("residue_flags", "residue_flags"), ("atom_clash", "atom_clash"),
                  ("term_fail", "term_fail")):
        assert np.array_equal(body(o[k]).cpu().numpy().astype(np.int64), r64[rk]), (tag, k, "margin", margin)
    ang = launch_dihedrals(L, g, x).cpu().double().numpy()
    a64 = np.stack([ref.dihedral(xp, g.dih) for xp in x])
    e = angle_error(ang, a64)
    print(f"ENVELOPE | pd_receptor_dihedrals | {tag} | - | {e:.2e} | {DOUBLE_TOL:.2e} | {e / DOUBLE_TOL:.2f} |")
    assert e <= DOUBLE_TOL, (tag, e)
    if check_class:
        xd = torch.from_numpy(x).cuda()
        out = g.check(xd)
        assert set(out) == {"val", "worst_pair", "counts", "flags", "valid", "residue_flags", "atom_clash", "term_val", "term_fail"}
        for k, b in (("val", "val"), ("worst_pair", "worst"), ("counts", "counts"), ("flags", "flags"), ("residue_flags", "residue_flags"),
                     ("atom_clash", "atom_clash"), ("term_val", "term_val"), ("term_fail", "term_fail")):
            assert out[k].is_cuda and torch.equal(out[k], body(o[b])), (tag, k)
        assert torch.equal(out["valid"], out["flags"] == 0) and out["valid"].dtype == torch.bool
        assert np.array_equal(g.dihedrals(xd).cpu().numpy(), ang.astype(np.float32), equal_nan=True)
    return {k: body(v) for k, v in o.items()}, r64, ang


# ------------------------------------------------------------------ the cases
def test_a_forty_residues_six_defects_over_three_poses(L):
    names, x_ref, poses = cases.combined_poses()
    assert poses.shape == (3, 335, 3) and 335 > 256 and 335 % 64
    g = cases.geometry(names, x_ref, device="cuda")
    o, r64, _ = compare("(a) 40 residues P=3", L, g, poses)
    flags = o["flags"].cpu().tolist()
    assert flags[0] == 0 and flags[1] & (4 | 8 | 32) == (4 | 8 | 32) and flags[2] & (16 | 1 | 64) == (16 | 1 | 64)
    rf = o["residue_flags"].cpu().numpy()
    assert rf[1, 2] & 4 and rf[1, 8] & 8 and rf[1, 9] & 8 and rf[1, 13] & 32 and rf[2, 27] & 16 and rf[2, 24] & 1 and rf[2, 10] & 64 and rf[2, 20] & 64
    lines = g.describe(o["residue_flags"][1])
    assert any(s.startswith("residue 2: ") and "chirality" in s for s in lines) and len(lines) == int((rf[1] > 0).sum())


def test_b_a_single_residue(L):
    res, atoms, rid, x = ref.build_peptide(("TRP",), oxt=True)
    g = cases.geometry((res, atoms, rid), x, device="cuda")
    assert g.term_counts[3] == 0 and g.n_residues == 1
    o, _, ang = compare("(b) one residue P=1", L, g, x[None])
    assert o["flags"].cpu().tolist() == [0] and np.isnan(ang[0, 0, :3]).all() and not np.isnan(ang[0, 0, 3:5]).any() and float(o["val"][0, 6]) == 0


def test_c_two_chains_unknown_residue_masked_atom_disulfide(L):
    names, x, mask, chain, number, at = cases.two_chain_case()
    g = cases.geometry(names, x, device="cuda", mask=mask, chain_of=chain, residue_number=number)
    assert g.untyped == 8 and len(g.peptides) == 6
    rng = np.random.default_rng(3)
    poses = np.stack([x, x + rng.normal(0, 0.03, x.shape), x])
    poses[2][at[7, "SG"]] += [0.0, 0.0, 1.0]                          # the disulfide stretched to 3.05 A: x 1.49
    poses[2][names[2] == 3] += 40.0                                    # the unknown residue may be anywhere ...
    poses[2][at[5, "CD2"]] = poses[2][at[0, "CA"]]                     # ... and the masked atom on top of another
    o, r64, _ = compare("(c) two chains P=3", L, g, poses)
    assert o["flags"].cpu().tolist()[0] == 0 and o["flags"].cpu().tolist()[2] & 1 and int(o["counts"][2, 6]) == r64["counts"][2, 6]
    rf = o["residue_flags"].cpu().numpy()
    assert rf[2, 1] & 1 and rf[2, 7] & 1 and rf[2, 3] == 0


def test_d_one_nan_coordinate(L):
    names, x_ref, at = cases.peptide40()
    g = cases.geometry(names, x_ref, device="cuda")
    poses = np.stack([x_ref, x_ref]).astype(np.float32)
    a = at[11, "CD"]
    poses[1, a, 2] = NAN
    o, r64, ang = compare("(d) NaN P=2", L, g, poses)
    assert o["flags"].cpu().tolist() == [0, 1 | 2 | 64] and o["worst"][1].cpu().tolist() == [0, a] and float(o["val"][1, 4]) == 0.0
    assert int(o["counts"][1, 6]) == 329 and int(o["atom_clash"][1].sum()) == 330 and np.isnan(ang[1, 11, 4:7]).all() and not np.isnan(ang[1, 11, 3])
    poses[1, a, 2] = np.inf
    o2 = launch(L, g, poses)
    assert torch.equal(body(o2["flags"]), o["flags"]) and torch.equal(body(o2["counts"]), o["counts"]) and torch.equal(body(o2["worst"]), o["worst"])


def test_e_empty_tables(L):
    from physdock_amd.receptor_geometry import ReceptorGeometry
    g = ReceptorGeometry.from_tables(np.zeros(5), np.ones(5), np.zeros(5, int), [], np.zeros((5, 3)), n_residues=2, device="cuda")
    assert g.n_terms == 0 and g.excl_atom.size == 0
    x = np.random.default_rng(0).normal(size=(2, 5, 3)).astype(np.float32)
    o, _, ang = compare("(e) empty P=2", L, g, x)
    assert o["val"].cpu().tolist() == [[1, 1, 1, 1, float("inf"), 0, 0, 0]] * 2 and o["worst"].cpu().tolist() == [[-1, -1]] * 2
    assert not o["flags"].any() and not o["counts"].any() and not o["residue_flags"].any() and np.isnan(ang).all()
    # atoms that take part but no term at all: only the clash check has something to say
    g2 = ReceptorGeometry.from_tables(np.ones(5), np.full(5, 1.7), np.arange(5) // 3, [], x[0] * 10, device="cuda")
    y = np.stack([x[0] * 10, x[0] * 10])
    y[1, 4] = y[1, 0] + np.float32([1.0, 0, 0])
    o, _, _ = compare("(e) no terms P=2", L, g2, y)
    assert o["flags"].cpu().tolist() == [0, 64] and o["worst"][1].cpu().tolist() == [0, 4] and o["residue_flags"][1].cpu().tolist() == [64, 64]


def test_f_a_pose_does_not_see_its_batch(L):
    names, x_ref, poses, _ = cases.single_defect_poses()
    g = cases.geometry(names, x_ref, device="cuda")
    five = poses[[0, 6, 2, 3, 1]]
    whole, again = launch(L, g, five), launch(L, g, five)
    da, db = launch_dihedrals(L, g, five), launch_dihedrals(L, g, five)
    assert torch.equal(da.view(torch.int32), db.view(torch.int32))
    for k in whole:
        assert torch.equal(body(whole[k]), body(again[k])), k          # (no NaN among these outputs: +-inf are the sentinels)
    for p in range(5):
        alone = launch(L, g, five[p:p + 1])
        for k in whole:
            assert torch.equal(body(alone[k])[0], body(whole[k])[p]), (k, p)
        assert torch.equal(launch_dihedrals(L, g, five[p:p + 1])[0].view(torch.int32), da[p].view(torch.int32))


def test_chi_recovery_on_the_device(L):
    names, x_ref, at = cases.peptide40()
    g = cases.geometry(names, x_ref, device="cuda")
    turned = ref.build_peptide(cases.SEQ40, oxt=True, chis={11: (55.0, 95.0, 60.0), 3: (-65.0, -80.0), 17: (-65.0, -60.0)})[3]   # LYS, ASP, TRP
    poses = np.stack([x_ref, turned]).astype(np.float32)
    out = g.chi_recovery(torch.from_numpy(poses).cuda())
    ang = np.stack([ref.dihedral(xp, g.dih) for xp in poses])
    m, c, ok = ref.chi_recovery(ang, g.chi_ref, g.pi_periodic)
    assert out["matched"].cpu().tolist() == m.tolist() and out["compared"].cpu().tolist() == c.tolist() and np.array_equal(out["rotamer_ok"].cpu().numpy(), ok)
    assert m[0] == c[0] == int((~np.isnan(g.chi_ref)).sum()) and c[1] == c[0] and m[1] == m[0] - 3       # LYS chi1 and chi3, TRP chi2 (155 off); ASP chi2 is 175 off, 5 modulo 180
    assert float(out["recovered"][0]) == 1.0 and not ok[1, 11] and ok[1, 3] and not ok[1, 17] and ok[1, 13] and not ok[1, 0]
    pocket = g.chi_recovery(torch.from_numpy(poses).cuda(), residues=[3, 11], tolerance=40.0, x_ref=x_ref)
    m2, c2, _ = ref.chi_recovery(ang, g.chi_ref, g.pi_periodic, residues=[3, 11])
    assert pocket["matched"].cpu().tolist() == m2.tolist() and pocket["compared"].cpu().tolist() == c2.tolist() == [6, 6]


def test_thresholds_are_taken_from_the_struct_and_arguments_are_checked(L):
    names, x_ref, poses = cases.combined_poses()
    g = cases.geometry(names, x_ref, device="cuda")
    loose = dict(bond_lo=0.0, bond_hi=1e9, angle_lo=0.0, angle_hi=1e9, clash=0.0, planarity=1e9, twist=1e9, cis=0.0)
    assert body(launch(L, g, poses, thresholds(**loose))["flags"]).cpu().tolist() == [0, 4, 4]        # (a wrong centre has no threshold)
    assert body(launch(L, g, poses, thresholds(**dict(loose, planarity=0.0)))["flags"]).cpu().tolist() == [32, 36, 36]
    assert body(launch(L, g, poses, thresholds(**dict(loose, clash=1e9)))["flags"]).cpu().tolist() == [64, 68, 68]
    x = torch.from_numpy(poses).cuda()
    d = {k: torch.from_numpy(np.ascontiguousarray(getattr(g, k))).cuda() for k in TABLES}
    ws = torch.empty(L.pd_receptor_geometry_workspace_numel(3, 335), dtype=torch.int64, device="cuda")
    outs = [sentinel(3, 8), sentinel(3, 2, dtype=torch.int32), sentinel(3, 7, dtype=torch.int32), sentinel(3, dtype=torch.int32),
            sentinel(3, 40, dtype=torch.uint8), sentinel(3, 335, dtype=torch.uint8), sentinel(3, g.n_terms), sentinel(3, g.n_terms, dtype=torch.uint8)]
    tables = [P(d[k]) for k in TABLES]
    def call(x_=P(x), counts=g.term_counts, sizes=(3, 335, 40), outs_=None, ws_=P(ws)):
        return L.pd_receptor_geometry(x_, *tables[:5], *counts, *tables[5:], thresholds(), ws_, *[P(b) for b in outs] if outs_ is None else outs_,
                                      *sizes, S())
    assert call(x_=None) == PD_ERR_ARG and call(ws_=None) == PD_ERR_ARG and call(sizes=(0, 335, 40)) == PD_ERR_ARG
    assert call(counts=(-1, 0, 0, 0, 0)) == PD_ERR_ARG and call(outs_=[None] + [P(b) for b in outs[1:]]) == PD_ERR_ARG
    assert call(sizes=(3, 4097, 40)) == PD_ERR_UNSUPPORTED and call(sizes=(3, 335, 4097)) == PD_ERR_UNSUPPORTED
    assert call(sizes=(65536, 335, 40)) == PD_ERR_UNSUPPORTED and call(counts=(1 << 20, 1, 0, 0, 0)) == PD_ERR_UNSUPPORTED
    assert L.pd_receptor_geometry_workspace_numel(0, 5) == PD_ERR_ARG and L.pd_receptor_geometry_workspace_numel(1, 4097) == PD_ERR_UNSUPPORTED
    assert L.pd_receptor_dihedrals(None, P(d["res_atom"]), P(outs[0]), 1, 5, 1, S()) == PD_ERR_ARG
    assert L.pd_receptor_dihedrals(P(x), P(d["res_atom"]), P(outs[0]), 1, 4097, 1, S()) == PD_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(is_sentinel(b).all() for b in outs)
    with pytest.raises(ValueError, match="pose atoms"):
        g.check(x[:, :-1])


# ------------------------------------------------------------------ redock
def synthetic_geometry(batch):
    """every protein token of a synthetic batch as an alanine (its five atoms N CA C O CB); the ligand's tokens have no table"""
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.receptor_geometry import ReceptorGeometry
    lig = ligand_atom_mask(batch).cpu().numpy()
    rid = batch["atom_id_to_token_id"].cpu().numpy()
    atoms, seen = [], {}
    for r in rid:
        atoms.append(("N", "CA", "C", "O", "CB")[seen.get(r, 0) % 5])
        seen[r] = seen.get(r, 0) + 1
    res = ["LIG" if l else "ALA" for l in lig]
    return ReceptorGeometry.from_names(res, atoms, rid, batch["x_gt"], n_residues=int(batch["is_ligand"].shape[0]), device="cuda")


def test_g_redock_reports_receptor_geometry_and_changes_nothing_else(small_model_inputs):
    from physdock_amd import PhysDock, driver
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.validity import PoseValidity
    cfg, P_, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P_, strict=True)
    model, dbatch = model.cuda().eval(), {k: v.cuda() for k, v in batch.items()}
    g = synthetic_geometry(dbatch)
    assert g.untyped == int(ligand_atom_mask(dbatch).sum()) and g.term_counts[0] == 18 * 4 + 17
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, dbatch, **kw)
    out = driver.redock(model, dbatch, receptor_geometry=g, **kw)
    assert set(out) == set(plain) | {"receptor_geometry"}
    assert torch.equal(out["poses"], plain["poses"]) and out["rounds"] == plain["rounds"] and out["accepted"] == plain["accepted"]
    assert all(torch.equal(out["ranking"][k], plain["ranking"][k]) for k in ("x_aligned", "dist", "rmsd_all")) and out["ranking"]["order"] == plain["ranking"]["order"]
    got = out["receptor_geometry"]
    assert set(got) == {"val", "flags", "valid", "counts", "residue_flags", "chi_recovery"}
    want = g.check(out["poses"])
    assert all(torch.equal(got[k], want[k]) for k in ("val", "flags", "valid", "counts", "residue_flags")) and got["flags"].shape == (4,)
    assert set(got["chi_recovery"]) == {"matched", "compared", "recovered", "rotamer_ok"} and got["chi_recovery"]["compared"].tolist() == [0] * 4
    n_lig = int(ligand_atom_mask(dbatch).sum())
    v = PoseValidity.from_batch(dbatch, [(i, i + 1) for i in range(n_lig - 1)])
    both = driver.redock(model, dbatch, receptor_geometry=g, validity=v, **kw)
    assert torch.equal(both["receptor_geometry"]["valid_both"], both["receptor_geometry"]["valid"] & both["validity"]["valid"])
    many = driver.redock_many(model, [(dbatch, {"receptor_geometry": g})], **kw)
    assert torch.equal(many[0]["poses"], plain["poses"]) and torch.equal(many[0]["receptor_geometry"]["val"], got["val"])
    from physdock_amd.receptor_geometry import ReceptorGeometry
    other = ReceptorGeometry.from_names(["GLY"] * 3, ["N", "CA", "C"], [0] * 3, np.eye(3))
    with pytest.raises(ValueError, match="pose atoms"):
        driver.redock(model, dbatch, receptor_geometry=other, **kw)
    with pytest.raises(ValueError, match="ReceptorGeometry"):
        driver.redock(model, dbatch, receptor_geometry=object(), **kw)
