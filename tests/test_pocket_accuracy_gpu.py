"""pd_pocket_accuracy (csrc/pocket_accuracy.hip) straight on the C ABI, PocketAccuracy.score, and the pocket_accuracy keyword of redock /
redock_many, against the float64 numpy restatement tests/pocket_accuracy_ref.py on the seeded cases of tests/pocket_accuracy_cases.py.

EXACT: conserved, swapped, ok and fit_ok.  The device counts in float64 from the same fp32 coordinates; two float64 evaluations of a
distance differ by a few ulp (about 1e-14 A inside the +-20 A box), and tests/test_pocket_accuracy_cpu.py checks on the restatement alone
that no compare of any case comes closer than 1e-9 A to its threshold and that no swap decision is a tie - a condition on the seeds.
TOLERANCES: lddt_lp and residue_lddt within 1 fp32 ulp of the restatement's quotient; RMSDs and t within 1e-6 + 1e-6 |v| A (float64 sums
of at most a few hundred terms below 1e3 A^2, rounded once to fp32: 6e-8 relative; near zero the deviations are differences of
coordinates below 64 A whose float64 error is about 1e-14 A); quat up to sign within 1e-6.

Output buffers are one row longer than needed and pre-filled with a sentinel (NaN, -7 for integers)."""
import numpy as np
import pytest
import torch

import pocket_accuracy_cases as cases
import pocket_accuracy_ref as ref

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN = float("nan")
OUT = ("lddt_lp", "residue_lddt", "conserved", "swapped", "rmsd", "residue_rmsd", "quat", "t", "ok", "fit_ok")


# ------------------------------------------------------------------ sentinels, plumbing
def sentinel(*shape, dtype=torch.float32):
    fill = NAN if dtype.is_floating_point else (249 if dtype == torch.uint8 else -7)
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")


def is_sentinel(t):
    return torch.isnan(t) if t.dtype.is_floating_point else t == (249 if t.dtype == torch.uint8 else -7)


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


def to_device(x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).cuda()


def bits(t):
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def device_tables(t):
    """the restatement's tables of a case as the kernel reads them, every index checked to be inside its array first"""
    A, Np, Rp, n = t["A"], len(t["patom"]), len(t["pocket"]), int(t["pair_start"][-1])
    assert 1 <= Rp <= Np <= A <= 4096 and len(t["res_atom_start"]) == Rp + 1 and len(t["pair_start"]) == Np + 1
    assert t["res_atom_start"][0] == 0 and t["res_atom_start"][-1] == Np and (np.diff(t["res_atom_start"]) >= 1).all()
    assert t["pair_start"][0] == 0 and (np.diff(t["pair_start"]) >= 0).all() and len(t["pair_atom"]) == n == len(t["pair_dist"])
    for k in ("patom", "pair_atom", "partner", "named"):
        assert len(t[k]) == 0 or (0 <= t[k].min() and t[k].max() < A), k
    assert len(t["partner"]) == A == len(t["atom_slot"]) and t["atom_slot"].min() >= -1 and t["atom_slot"].max() < Rp
    assert (t["atom_slot"][t["partner"] != np.arange(A)] >= 0).all() and Np <= len(t["named"]) <= A
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).cuda()
    return dict(patom=up(t["patom"], np.int32), patom_partner=up(t["partner"][t["patom"]], np.int32),
                patom_kind=up(t["patom_ca"] * 1 + t["patom_bb"] * 2, np.uint8), patom_ref=up(t["patom_ref"], np.float64),
                res_atom_start=up(t["res_atom_start"], np.int32), pair_start=up(t["pair_start"], np.int32),
                pair_atom=up(t["pair_atom"], np.int32), pair_dist=up(t["pair_dist"], np.float64), atom_partner=up(t["partner"], np.int32),
                atom_slot=up(t["atom_slot"], np.int32), named=up(t["named"], np.int32), A=A, Np=Np, Rp=Rp, n=n, n_named=len(t["named"]))


def buffers(n, Rp):
    return dict(lddt_lp=sentinel(n), residue_lddt=sentinel(n, Rp), conserved=sentinel(n, 4, dtype=torch.int32),
                swapped=sentinel(n, Rp, dtype=torch.int32), rmsd=sentinel(n, 3), residue_rmsd=sentinel(n, Rp),
                quat=sentinel(n, 4, dtype=torch.float64), t=sentinel(n, 3, dtype=torch.float64), ok=sentinel(n, dtype=torch.uint8),
                fit_ok=sentinel(n, dtype=torch.uint8))


def table_args(d):
    opt = lambda k: P(d[k]) if d[k].numel() else None
    return [P(d["patom"]), P(d["patom_partner"]), P(d["patom_kind"]), P(d["patom_ref"]), P(d["res_atom_start"]), P(d["pair_start"]),
            opt("pair_atom"), opt("pair_dist"), P(d["atom_partner"]), P(d["atom_slot"]), P(d["named"])]


def launch(L, x, d, thresholds=ref.THRESHOLDS):
    """the launcher into sentinel buffers -> dict of the bodies (NaN is a legitimate float output here: the row behind every output
    must keep its sentinel, and the integer outputs must lose theirs)"""
    x = to_device(x)
    n = x.shape[0]
    assert x.shape[1] == d["A"] and x.dtype == torch.float32
    n_ws = L.pd_pocket_accuracy_workspace_numel(n, d["Rp"])
    assert n_ws == 4 * n * d["Rp"]
    ws = torch.empty(n_ws, dtype=torch.int32, device="cuda")
    b = buffers(n, d["Rp"])
    rc = L.pd_pocket_accuracy(P(x), *table_args(d), *thresholds, P(ws), n_ws, *[P(b[k]) for k in OUT], n, d["A"], d["Np"], d["Rp"], d["n"],
                              d["n_named"], S())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for k, buf in b.items():
        assert is_sentinel(buf[-1]).all(), (k, "the row behind the output was written")
        if not buf.dtype.is_floating_point:
            assert not is_sentinel(buf[:-1]).any(), (k, "an output element kept its sentinel")
    return {k: buf[:-1] for k, buf in b.items()}


def one_ulp(dev, want):
    dev, want = np.asarray(dev, np.float32), np.asarray(want, np.float64).astype(np.float32)
    both_nan = np.isnan(dev) & np.isnan(want)
    return bool((both_nan | (dev == want) | (dev == np.nextafter(want, np.float32(np.inf))) | (dev == np.nextafter(want, np.float32(-np.inf)))).all())


def close(dev, want, tag):
    dev, want = np.asarray(dev, np.float64), np.asarray(want, np.float64)
    assert (np.isnan(dev) == np.isnan(want)).all(), (tag, "NaN pattern")
    m = ~np.isnan(want)
    err = np.abs(dev[m] - want[m])
    assert (err <= 1e-6 + 1e-6 * np.abs(want[m])).all(), (tag, float(err.max()))
    return float(err.max()) if m.any() else 0.0


def accept(tag, out, o):
    """the module docstring's rule on one launch against the restatement's scores o"""
    h = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("conserved", "swapped", "ok", "fit_ok"):
        assert h[k].astype(np.int64).tolist() == o[k].tolist(), (tag, k)
    assert one_ulp(h["lddt_lp"], o["lddt_lp"]) and one_ulp(h["residue_lddt"], o["residue_lddt"]), (tag, "lddt")
    e_rmsd = close(h["rmsd"], np.stack([o["ca_rmsd"], o["backbone_rmsd"], o["heavy_rmsd"]], 1), tag + " rmsd")
    e_res = close(h["residue_rmsd"], o["residue_rmsd"], tag + " residue_rmsd")
    e_t = close(h["t"], o["t"], tag + " t")
    sign = np.where((h["quat"] * o["quat"]).sum(-1, keepdims=True) < 0, -1.0, 1.0)
    assert (np.isnan(h["quat"]) == np.isnan(o["quat"])).all()
    e_q = float(np.nanmax(np.abs(h["quat"] * sign - o["quat"]), initial=0.0))
    assert e_q <= 1e-6, (tag, "quat", e_q)
    print(f"POCKET-ACCURACY | {tag} | poses {len(o['ok'])} | pairs {o['n_pairs']} | max err rmsd {max(e_rmsd, e_res):.2e} t {e_t:.2e} "
          f"quat {e_q:.2e} |")


def spec_of(r, **over):
    from physdock_amd import PocketAccuracy
    s = r["s"]
    return PocketAccuracy.from_names(s["res_names"], s["atom_names"], s["residue_of"], s["x_ref"], s["ligand_idx"], mask=s["mask"],
                                     device="cuda", **dict(r["kw"], **over))


def same_bits(a, b, keys=OUT):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in keys)


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", list(cases.CASES))
def test_kernel_against_float64(L, name):
    r = cases.reference(name)
    d = device_tables(r["tab"])
    out = launch(L, r["x"], d)
    accept(name, out, r["out"])
    # bit-identical from launch to launch, and a pose does not see its neighbours: alone, and inside a batch of 3
    assert same_bits(launch(L, r["x"], d), out)
    n = r["x"].shape[0]
    for p in range(min(n, 3)):
        one = launch(L, r["x"][p:p + 1], d)
        assert all(torch.equal(bits(one[k][0]), bits(out[k][p])) for k in OUT), (name, p)
    if n >= 3:
        three = launch(L, r["x"][[n - 1, 0, n - 2]], d)
        for row, p in enumerate((n - 1, 0, n - 2)):
            assert all(torch.equal(bits(three[k][row]), bits(out[k][p])) for k in OUT), (name, p)
    # PocketAccuracy.score: the same bits through the package's own tables
    obj = spec_of(r)
    sc = obj.score(to_device(r["x"]))
    assert set(sc) == set(OUT) | {"ca_rmsd", "backbone_rmsd", "heavy_rmsd", "n_pairs", "pocket_residues", "residue_labels"}
    assert all(sc[k].is_cuda and sc[k].dtype == out[k].dtype and sc[k].shape == out[k].shape for k in OUT) and same_bits(sc, out)
    assert all(torch.equal(bits(sc[k]), bits(sc["rmsd"][:, c])) for c, k in enumerate(("ca_rmsd", "backbone_rmsd", "heavy_rmsd")))
    assert sc["n_pairs"] == d["n"] and sc["pocket_residues"].cpu().tolist() == r["tab"]["pocket"].tolist()
    assert len(sc["residue_labels"]) == d["Rp"]


def test_the_special_poses_on_the_device(L):
    r = cases.reference("nine")
    out = {k: v.cpu().numpy() for k, v in launch(L, r["x"], device_tables(r["tab"])).items()}
    assert (out["lddt_lp"][:7] == 1.0).all() and out["swapped"][:7].sum(1).tolist() == [0, 1, 1, 2, 0, 0, 0]
    assert np.nonzero(out["swapped"][2])[0].tolist() == [5] and np.nonzero(out["swapped"][3])[0].tolist() == [3, 4]
    assert out["rmsd"][:5].max() <= 1e-6 and out["residue_rmsd"][:5].max() <= 1e-6          # the reference, swapped names, moved exactly
    assert out["rmsd"][6].min() > 1.0                                                       # mirrored
    q = out["quat"][4]
    assert np.abs(ref.rotation(q) - cases.QUARTER.T).max() <= 1e-6 and np.abs(out["t"][4] + cases.QUARTER.T @ cases.SHIFT).max() <= 1e-6


def test_small_pockets_no_pairs_and_tile_edges(L):
    for name, rp in (("one", 1), ("two", 2)):
        r = cases.reference(name)
        assert len(r["tab"]["pocket"]) == rp
        out = launch(L, r["x"], device_tables(r["tab"]))
        assert out["fit_ok"].cpu().tolist() == [0] * 3 and out["ok"].cpu().tolist() == [1] * 3
        assert torch.isnan(out["rmsd"]).all() and torch.isnan(out["quat"]).all() and torch.isnan(out["residue_rmsd"]).all()
        assert torch.isfinite(out["lddt_lp"]).all() and float(out["lddt_lp"][0]) == 1.0
    r = cases.reference("nopairs")
    assert r["out"]["n_pairs"] == 0 and r["x"].shape[0] == 1
    out = launch(L, r["x"], device_tables(r["tab"]))
    assert float(out["lddt_lp"][0]) == 0.0 and not out["residue_lddt"].any() and not out["conserved"].any() and not out["swapped"].any()
    for name, n in (("row1", 1), ("row256", 256), ("row257", 257)):
        assert np.diff(cases.reference(name)["tab"]["pair_start"])[0] == n         # (the comparison itself: test_kernel_against_float64)


def test_non_finite_coordinates(L):
    r = cases.reference("far")
    t, s = r["tab"], r["s"]
    assert t["A"] % 64 != 0
    pocket_atom, unnamed = int(t["patom"][3]), int(s["ligand_idx"][0])
    env_atom = int(next(j for j in t["pair_atom"] if t["atom_slot"][j] < 0))
    x = np.repeat(np.asarray(r["x"][:1], dtype=np.float32), 4, 0)
    x[1, pocket_atom, 0], x[2, env_atom, 2], x[3, unnamed, 1] = np.nan, np.inf, np.nan
    d = device_tables(t)
    out = launch(L, x, d)
    accept("far, non-finite", out, ref.score(t, x))
    assert out["ok"].cpu().tolist() == [1, 0, 0, 1]
    assert all(torch.equal(bits(out[k][3]), bits(out[k][0])) for k in OUT), "an atom no table names changes nothing"
    for p in (1, 2):
        assert all(torch.isnan(out[k][p]).all() for k in ("lddt_lp", "residue_lddt", "rmsd", "residue_rmsd", "quat", "t"))
        assert not out["conserved"][p].any() and not out["swapped"][p].any() and int(out["fit_ok"][p]) == 0


def test_thresholds_and_radii_are_the_constructors(L):
    r = cases.reference("nine")
    thr = (0.25, 0.75, 1.5, 3.0)
    kw = dict(pocket_radius=6.5, inclusion_radius=9.0)
    tab = cases.tables(r["s"], **kw)
    want = ref.score(tab, r["x"], thresholds=thr)
    assert want["margin"].min() >= 1e-9 and want["ties"].sum() == 0, "the seed condition for these thresholds"
    out = launch(L, r["x"], device_tables(tab), thr)
    accept("nine, radii 6.5 / 9, thresholds / 2 .. 3", out, want)
    sc = spec_of(r, thresholds=thr, **kw).score(to_device(r["x"]))
    assert same_bits(sc, out) and not torch.equal(out["conserved"], launch(L, r["x"], device_tables(r["tab"]))["conserved"])


def test_argument_handling(L):
    r = cases.reference("two")
    d = device_tables(r["tab"])
    x = to_device(r["x"])
    n = x.shape[0]
    ws = torch.full((4 * n * d["Rp"] + 4,), -7, dtype=torch.int32, device="cuda")
    b = buffers(n, d["Rp"])
    good = [P(x), *table_args(d), 0.5, 1.0, 2.0, 4.0, P(ws), 4 * n * d["Rp"], *[P(b[k]) for k in OUT]]
    size = [n, d["A"], d["Np"], d["Rp"], d["n"], d["n_named"]]
    call = lambda a=good, sz=size: L.pd_pocket_accuracy(*a, *sz, S())
    bad = {}
    for k in [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16] + list(range(18, 28)):
        a = list(good)
        a[k] = None
        bad[f"null {k}"] = call(a)
    for k, name in enumerate(["P", "A", "Np", "Rp"]):
        sz = list(size)
        sz[k] = 0
        bad[f"{name}=0"] = call(sz=sz)
    bad["n_pairs<0"] = call(sz=[n, d["A"], d["Np"], d["Rp"], -1, d["n_named"]])
    bad["Rp>Np"] = call(sz=[n, d["A"], d["Np"], d["Np"] + 1, d["n"], d["n_named"]])
    bad["n_named<Np"] = call(sz=[n, d["A"], d["Np"], d["Rp"], d["n"], d["Np"] - 1])
    bad["Np>A"] = call(sz=[n, d["A"], d["A"] + 1, d["Rp"], d["n"], d["A"] + 1])
    bad["short ws"] = call(good[:17] + [4 * n * d["Rp"] - 1] + good[18:])
    bad["ws unaligned"] = call(good[:16] + [P(ws) + 4] + good[17:])
    bad["threshold 0"] = call(good[:12] + [0.0] + good[13:])
    bad["threshold nan"] = call(good[:15] + [NAN] + good[16:])
    assert all(rc == PD_ERR_ARG for rc in bad.values()), bad
    uns = {"A": call(sz=[n, 4097, d["Np"], d["Rp"], d["n"], d["n_named"]]), "Rp": call(sz=[n, 4096, 2048, 1025, d["n"], 2048]),
           "P": call(sz=[65536] + size[1:])}
    assert all(rc == PD_ERR_UNSUPPORTED for rc in uns.values()), uns
    numel = L.pd_pocket_accuracy_workspace_numel
    assert numel(0, 3) == numel(3, 0) == PD_ERR_ARG and numel(65536, 3) == numel(3, 1025) == PD_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(is_sentinel(t).all() for t in list(b.values()) + [ws]), "a refused call wrote"


# ------------------------------------------------------------------ redock, redock_many
def synthetic_spec(batch):
    """every protein token of a synthetic batch as a five-atom residue; even tokens are named like a valine cut down to N CA C CG1 CG2, so
    that some residues can be swapped"""
    from physdock_amd import PocketAccuracy
    from physdock_amd.driver import ligand_atom_mask
    lig = ligand_atom_mask(batch).cpu().numpy()
    rid = batch["atom_id_to_token_id"].cpu().numpy()
    atoms, res, seen = [], [], {}
    for a, r in enumerate(rid):
        k = seen.get(r, 0)
        seen[r] = k + 1
        val = r % 2 == 0
        res.append("LIG" if lig[a] else ("VAL" if val else "ALA"))
        atoms.append((("N", "CA", "C", "CG1", "CG2") if val else ("N", "CA", "C", "O", "CB"))[k % 5])
    return PocketAccuracy.from_names(res, atoms, rid, batch["x_gt"], np.nonzero(lig)[0], device="cuda")


def test_redock_reports_pocket_accuracy_and_changes_nothing_else(small_model_inputs):
    from physdock_amd import PhysDock, PocketAccuracy, driver
    cfg, P_, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P_, strict=True)
    model, dbatch = model.cuda().eval(), {k: v.cuda() for k, v in batch.items()}
    obj = synthetic_spec(dbatch)
    assert obj.n_pairs > 0 and obj.swappable.any() and obj.n_ca >= 3
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, dbatch, **kw)
    again = driver.redock(model, dbatch, **kw)
    out = driver.redock(model, dbatch, pocket_accuracy=obj, **kw)
    assert set(plain) == set(again) and set(out) == set(plain) | {"pocket_accuracy"}
    for k, v in plain.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(out[k], v) and torch.equal(again[k], v), k
        elif isinstance(v, dict):
            assert set(out[k]) == set(v) and all(torch.equal(out[k][q], w) if isinstance(w, torch.Tensor) else out[k][q] == w
                                                 for q, w in v.items()), k
        else:
            assert out[k] == v, k
    got, n, Rp = out["pocket_accuracy"], out["poses"].shape[0], obj.n_pocket_residues
    shapes = dict(lddt_lp=(n,), residue_lddt=(n, Rp), conserved=(n, 4), swapped=(n, Rp), rmsd=(n, 3), ca_rmsd=(n,), backbone_rmsd=(n,),
                  heavy_rmsd=(n,), residue_rmsd=(n, Rp), quat=(n, 4), t=(n, 3), ok=(n,), fit_ok=(n,))
    assert all(got[k].is_cuda and tuple(got[k].shape) == s for k, s in shapes.items())
    direct = obj.score(out["poses"])
    assert same_bits(got, direct) and bool(got["ok"].all()) and bool(got["fit_ok"].all())
    assert bool(((got["lddt_lp"] >= 0) & (got["lddt_lp"] <= 1)).all())
    lines = obj.describe(got, 0)
    assert len(lines) == Rp and all("lddt" in ln for ln in lines)
    many = driver.redock_many(model, [(dbatch, {"pocket_accuracy": obj})], **kw)              # one system: the sequential path
    assert same_bits(many[0]["pocket_accuracy"], got)
    # refused before anything is sampled
    other = PocketAccuracy.from_names(["GLY"] * 3 + ["LIG"], ["N", "CA", "C", "C1"], [0, 0, 0, 1], np.eye(4, 3), [3])
    with pytest.raises(ValueError, match="pose atoms"):
        driver.redock(model, dbatch, pocket_accuracy=other, **kw)
    with pytest.raises(ValueError, match="x_gt"):
        driver.redock(model, {k: v for k, v in dbatch.items() if k != "x_gt"}, pocket_accuracy=obj, **kw)


def test_redock_items_gain_lddt_lp_and_pocket_ca_rmsd():
    from physdock_amd import sdfio
    out = {"poses": torch.zeros(2, 5, 3, device="cuda"), "ranking": None,
           "pocket_accuracy": {"lddt_lp": torch.tensor([0.5, 1.0], device="cuda"), "ca_rmsd": torch.tensor([[1.5, 0.0], [0.25, 0.0]], device="cuda")[:, 0]}}
    items = sdfio.redock_items(out)
    assert list(items)[-2:] == ["lddt_lp", "pocket_ca_rmsd"] and items["pocket_ca_rmsd"].is_contiguous()
    assert items["pocket_ca_rmsd"].tolist() == [1.5, 0.25] and "lddt_lp" not in sdfio.redock_items({"poses": out["poses"], "ranking": None})
