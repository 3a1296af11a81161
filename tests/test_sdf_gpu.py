"""pd_sdf_format (csrc/sdf.hip) through SdfTemplate.format / .blocks / .text / .write_sdf, `with_hydrogens` and the sdf keyword of redock
/ redock_many.  Every case compares the device buffer, cut at `offsets`, byte for byte with the reference writer tests/sdf_ref.py on the
same float32 inputs, and `offsets` with the cumulative lengths of the reference records exactly."""
import numpy as np
import pytest
import torch

import sdf_ref as ref

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
BLOCK = 256                                                                # threads per block of the write kernel and of the scan


def molecule(seed, na, nb, n_charged):
    rng = np.random.default_rng(seed)
    symbols = [["C", "N", "O", "S", "Cl", "Br", "F", "P"][i] for i in rng.integers(0, 8, na)]
    bonds = [(i, i + 1) for i in range(na - 1)]
    while len(bonds) < nb:
        i, j = sorted(rng.choice(na, 2, replace=False).tolist())
        if (i, j) not in bonds:
            bonds.append((i, j))
    orders = rng.choice([1.0, 1.5, 2.0, 3.0], len(bonds)).tolist()
    charges = np.zeros(na, dtype=np.int64)
    charges[rng.choice(na, n_charged, replace=False)] = rng.choice([-2, -1, 1, 2], n_charged)
    return dict(symbols=symbols, bonds=bonds, bond_orders=orders, charges=charges)


def template(mol, extra=4, **kw):
    """the molecule as the LAST atoms of a pose, in reverse order, behind `extra` receptor atoms"""
    from physdock_amd.sdfio import SdfTemplate
    na = len(mol["symbols"])
    A = na + extra
    lig = np.arange(A)[::-1][:na].copy()
    elements = ["Fe"] * A
    for s, a in zip(mol["symbols"], lig):
        elements[a] = s
    return SdfTemplate.from_bonds(elements, mol["bonds"], lig, mol["bond_orders"], mol["charges"], device="cuda", **kw)


def reference(t, mol, x, props=(), order=None, **kw):
    """the reference records of the poses x (host float32 [P,A,3]); props: (name, host values, decimals or None)"""
    return ref.records(mol["symbols"], x[:, t.atom], mol["bonds"], mol["bond_orders"], mol["charges"], props, order, **kw)


def as_properties(props):
    return {name: (torch.from_numpy(np.asarray(v)).cuda() if d is None else (torch.from_numpy(np.asarray(v)).cuda(), d)) for name, v, d in props}


def check(t, mol, x, props=(), order=None, **kw):
    """format on the device against the reference: the records byte for byte, the offsets exactly, nothing behind the file"""
    from physdock_amd.sdfio import SdfTemplate
    want = reference(t, mol, x, props, order, **kw)
    dev_order = None if order is None else torch.tensor(list(order), dtype=torch.int64, device="cuda")
    res = t.format(torch.from_numpy(x).cuda(), as_properties(props), dev_order)
    n = len(want)
    assert res["n_records"] == n and res["bytes"].dtype == torch.uint8 and res["offsets"].dtype == torch.int64 and res["bytes"].is_cuda
    offsets = res["offsets"].cpu().numpy()
    assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    fixed, longest = t.record_bytes(SdfTemplate.items(as_properties(props), x.shape[0]))
    assert res["bytes"].shape[0] == n * longest >= offsets[-1]
    got = SdfTemplate.split(res)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"record {r}"
    assert bytes(res["bytes"][:int(offsets[-1])].cpu().numpy()).decode("ascii") == "".join(want), "the buffer is the SD file as it stands"
    return got


def poses(seed, P, A, scale=20.0):
    return np.random.default_rng(seed).normal(0.0, scale, (P, A, 3)).astype(np.float32)


def varied_items(seed, P):
    """items whose text lengths differ from record to record"""
    rng = np.random.default_rng(seed)
    mag = (10.0 ** rng.uniform(-3, 9, P) * rng.choice([-1.0, 1.0], P)).astype(np.float32)
    return [("score", mag, 4), ("pose", rng.integers(-2 ** 31, 2 ** 31, P).astype(np.int64), None), ("whole", mag, 0),
            ("fine", (mag * np.float32(1e-3)).astype(np.float32), 8), ("flag", rng.integers(0, 2, P).astype(bool), None)]


# ------------------------------------------------------------------ molblock shapes
@pytest.mark.parametrize("na, nb, n_charged, title", [(1, 0, 0, "t" * 80), (3, 2, 1, "three atoms " * 5), (37, 40, 11, "")])
def test_molblock_shapes(na, nb, n_charged, title):
    mol = molecule(na, na, nb, n_charged)
    t = template(mol, title=title, comment="c" * (70 if na == 1 else 3))
    x = poses(na, 5, t.n_pose_atoms)
    got = check(t, mol, x, varied_items(na, 5), title=title, comment=t.comment)
    fixed, _ = t.record_bytes(())
    assert fixed > BLOCK and fixed % BLOCK != 0 and all(len(g) > BLOCK for g in got), "a record crosses block boundaries"
    assert len({len(g) for g in got}) > 1, "the records differ in length"


# ------------------------------------------------------------------ record counts: the scan carries across its chunks
@pytest.mark.parametrize("n", [1, 257, 600])
def test_record_counts(n):
    mol = molecule(7, 3, 2, 1)
    t = template(mol)
    x = poses(n, n, t.n_pose_atoms)
    got = check(t, mol, x, varied_items(n, n))
    assert len(got) == n and (n == 1 or len({len(g) for g in got}) > 8)


def test_no_items_is_the_fixed_length_path():
    mol = molecule(8, 37, 40, 11)
    t = template(mol)
    got = check(t, mol, poses(8, 300, t.n_pose_atoms))
    assert {len(g) for g in got} == {t.record_bytes(())[0]} and got[0].endswith("M  END\n$$$$\n")
    assert t.blocks(torch.from_numpy(poses(8, 300, t.n_pose_atoms)).cuda()) == got
    one = torch.from_numpy(poses(8, 300, t.n_pose_atoms)[0]).cuda()
    assert t.blocks(one) == got[:1], "a single pose [A,3]"


# ------------------------------------------------------------------ coordinates
LARGEST = float(np.nextafter(np.float32(100000.0), np.float32(0.0)))       # 99999.9921875
MOST_NEGATIVE = float(np.nextafter(np.float32(-10000.0), np.float32(0.0)))  # -9999.9990234375
COORDINATES = [0.0, -0.0, -0.00004, 0.00004, 0.03125, 0.09375, -0.03125, -0.09375, 9.99995, -9.99995, 99999.99, 0.99995, 99.99995, 999.99995,
               9999.99995, LARGEST, MOST_NEGATIVE, 1e-30, -1e-30, 1.0, -1.0, 12345.678, -1234.5678, 0.00005, 0.00015, 5e-5, 2.5e-4]


def test_coordinates():
    mol = molecule(9, 3, 2, 0)
    t = template(mol, extra=0)
    vals = np.asarray(COORDINATES + [0.0] * (-len(COORDINATES) % 9), dtype=np.float32)
    x = vals.reshape(-1, 3, 3)
    got = check(t, mol, x)
    text = "".join(got)
    for want in ("   -0.0000", "    0.0312", "    0.0938", "   -0.0312", "   -0.0938", "99999.9922", "-9999.9990", "   10.0000", "  -10.0000"):
        assert want in text, want
    assert f"{float(np.float32(9.99995)):10.4f}" == "   10.0000" and f"{LARGEST:10.4f}" == "99999.9922" and f"{MOST_NEGATIVE:10.4f}" == "-9999.9990"
    # random bit patterns of every magnitude that fits
    rng = np.random.default_rng(10)
    x = (10.0 ** rng.uniform(-6, 3.99, (40, 3, 3)) * rng.choice([-1.0, 1.0], (40, 3, 3))).astype(np.float32)
    check(t, mol, x)


@pytest.mark.parametrize("bad", [100000.0, -10000.0, NAN, INF, -INF, 99999.99995, -9999.99995])
def test_coordinate_overflow_raises_with_the_count(bad):
    mol = molecule(9, 3, 2, 0)
    t = template(mol)
    x = poses(11, 4, t.n_pose_atoms)
    receptor = x.copy()
    receptor[:, :4] = bad                                                  # atoms that are not written do not count
    check(t, mol, receptor)
    x[2, t.atom[1], 2] = bad
    with pytest.raises(ValueError, match=r"^1 numbers do not fit"):
        t.format(torch.from_numpy(x).cuda())
    x[0, t.atom[0], 0] = bad
    x[3, t.atom[2], 1] = bad
    with pytest.raises(ValueError, match=r"^3 numbers do not fit"):
        t.format(torch.from_numpy(x).cuda(), {"a": torch.zeros(4)})
    assert len(t.blocks(torch.from_numpy(x).cuda(), order=[1])) == 1, "a pose that is not written does not count"


# ------------------------------------------------------------------ values
def test_values():
    mol = molecule(12, 3, 2, 1)
    t = template(mol)
    ties = [0.5, 1.5, 2.5, -0.5, -1.5, 0.03125, 0.09375, -0.03125, 2.0 ** -9, 3 * 2.0 ** -9, 2.0 ** -27, 3 * 2.0 ** -27, 0.0, -0.0, -0.00004, 9.99995,
            0.99999999, 99999.99, 1e-30, 123456.789, -1e7, 9.9999998e10, -9.9999998e10, 6.5, 16777216.0]
    special = [NAN, -NAN, INF, -INF]
    v = np.asarray(ties + special, dtype=np.float32)
    P = len(v)
    ints = np.resize(np.asarray([-2 ** 31, 2 ** 31 - 1, 0, -1, 1, 9, 10, -10, 99, 100, 999999999, 1000000000, -999999999, -1000000000], dtype=np.int64), P)
    props = [("d0", v, 0), ("d4", v, 4), ("d8", (v * np.float32(2.0 ** -20)).astype(np.float32), 8), ("i", ints, None),
             ("small8", np.clip(v, -9e6, 9e6).astype(np.float32), 8), ("b", (np.arange(P) % 3 == 0), None)]
    x = poses(12, P, t.n_pose_atoms)
    got = check(t, mol, x, props)
    text = "".join(got)
    for want in ("\nnan\n", "\ninf\n", "\n-inf\n", "\n-2147483648\n", "\n2147483647\n", "\n-0.0000\n", "\n-0\n", "\n0.0312\n", "\n0.0938\n", "\n2\n", "\n-2\n",
                 "\n0.00195312\n", "\n0.00585938\n"):
        assert want in text, want
    # float64 and float16 inputs become float32, int64 and uint8 become int32
    d = t.blocks(torch.from_numpy(x).cuda(), {"a": torch.from_numpy(v.astype(np.float64)).cuda(), "h": (torch.tensor([0.5] * P, dtype=torch.float16), 1),
                                               "u": torch.arange(P, dtype=torch.uint8)})
    assert d == reference(t, mol, x, [("a", v, 4), ("h", np.full(P, 0.5, dtype=np.float32), 1), ("u", np.arange(P), None)])
    # 32 items, the limit
    many = [(f"item_{k}", (np.clip(v, -100.0, 100.0) * np.float32(k)).astype(np.float32), k % 9) for k in range(32)]
    check(t, mol, x, many)


def test_value_overflow_raises():
    mol = molecule(12, 3, 2, 1)
    t = template(mol)
    x = torch.from_numpy(poses(13, 3, t.n_pose_atoms)).cuda()
    fits = np.float32(9.9999998e10)
    assert float(fits) * 1e4 < 1e15
    t.format(x, {"a": (torch.tensor([1.0, float(fits), -float(fits)]), 4)})
    with pytest.raises(ValueError, match=r"^1 numbers do not fit"):
        t.format(x, {"a": (torch.tensor([1.0, 1e12, 2.0]), 4)})
    with pytest.raises(ValueError, match=r"^2 numbers do not fit"):
        t.format(x, {"a": (torch.tensor([1.0, 1e12, 2.0]), 4), "b": (torch.tensor([-1e7, 0.0, 2.0]), 8)})
    t.format(x, {"a": (torch.tensor([1.0, 1e12, 2.0]), 2)})


# ------------------------------------------------------------------ order
def test_order_and_position_do_not_change_a_record():
    mol = molecule(14, 37, 40, 11)
    t = template(mol)
    P = 9
    x = poses(14, P, t.n_pose_atoms)
    props = varied_items(14, P)
    all_ = check(t, mol, x, props)
    perm = [4, 8, 0, 3, 7, 1, 6, 2, 5]
    assert check(t, mol, x, props, order=perm) == [all_[p] for p in perm]
    subset = [7, 2]
    assert check(t, mol, x, props, order=subset) == [all_[p] for p in subset]
    assert check(t, mol, x, props, order=[5]) == [all_[5]]
    assert check(t, mol, x, props, order=[3, 3, 3]) == [all_[3]] * 3, "a pose may be written more than once"
    dx = torch.from_numpy(x).cuda()
    assert t.blocks(dx, as_properties(props), order=np.asarray(perm)) == [all_[p] for p in perm], "a host order"
    alone = t.blocks(dx[6:7], {k: (v[0][6:7], v[1]) if isinstance(v, tuple) else v[6:7] for k, v in as_properties(props).items()})
    assert alone == [all_[6]], "a pose alone is the pose inside a batch"
    with pytest.raises(ValueError, match="order names a pose"):
        t.format(dx, order=[0, P])
    with pytest.raises(ValueError, match="order names a pose"):
        t.format(dx, order=torch.tensor([0, P], device="cuda"))          # a device order is checked by the kernel: nothing is read first
    with pytest.raises(ValueError, match="records"):
        t.format(dx, order=[])
    with pytest.raises(ValueError, match="pose atoms"):
        t.format(dx[:, 1:])


def test_text_and_file(tmp_path):
    from physdock_amd.sdfio import parse_sdf
    mol = molecule(15, 3, 2, 1)
    t = template(mol, title="a ligand")
    x = poses(15, 4, t.n_pose_atoms)
    props = varied_items(15, 4)
    dx, dp = torch.from_numpy(x).cuda(), as_properties(props)
    want = "".join(reference(t, mol, x, props, [2, 0], title="a ligand"))
    assert t.text(dx, dp, order=[2, 0]) == want
    path = tmp_path / "poses.sdf"
    assert t.write_sdf(path, dx, dp, order=[2, 0]) == 2 and path.read_bytes() == want.encode("ascii")
    back = parse_sdf(path.read_text())
    assert [r["properties"]["pose"] for r in back] == [str(props[1][1][p]) for p in (2, 0)]
    assert np.abs(back[0]["coords"] - x[2][t.atom].astype(np.float64)).max() <= 5e-5


# ------------------------------------------------------------------ protonated records
def small_system():
    """SER - GLY and a three-atom ligand C - C - O: 13 pose atoms, 7 receptor hydrogens, 6 on the ligand"""
    from physdock_amd.hydrogens import Hydrogens, receptor_hydrogens_from_names
    from physdock_amd.scoring import receptor_types_from_names
    ser, gly = ["N", "CA", "C", "O", "CB", "OG"], ["N", "CA", "C", "O"]
    z_of = {"C": 6, "N": 7, "O": 8}
    res, names, residue_of = ["SER"] * 6 + ["GLY"] * 4 + ["LIG"] * 3, ser + gly + ["C1", "C2", "O1"], [0] * 6 + [1] * 4 + [2] * 3
    elements = [z_of[a[0]] for a in names]
    rec = receptor_hydrogens_from_names(res[:10], names[:10], residue_of[:10])
    hy = Hydrogens.from_bonds(elements, [(0, 1), (1, 2)], [10, 11, 12], residue_of, receptor_types=receptor_types_from_names(res, names, elements),
                              receptor_hydrogens=rec, device="cuda")
    return elements, hy


def test_protonated_records():
    from physdock_amd.sdfio import SdfTemplate, parse_sdf
    elements, hy = small_system()
    assert hy.n_hydrogens == 4 + 3 + 6
    base = SdfTemplate.from_bonds(elements, [(0, 1), (1, 2)], [10, 11, 12], [1.0, 1.0], title="protonated", device="cuda")
    full = base.with_hydrogens(hy)
    assert full.symbols == ["C", "C", "O"] + ["H"] * 6 and full.n_pose_atoms == 26 and full.atom.tolist() == [10, 11, 12] + list(range(13 + 7, 26))
    x = torch.from_numpy(np.random.default_rng(5).normal(0.0, 4.0, (2, 13, 3)).astype(np.float32)).cuda()
    got = hy.place(x)
    assert bool(got["placed"].all())
    x_all = got["x_all"]
    records = full.blocks(x_all, {"pose": torch.arange(2)})
    host = x_all.cpu().numpy()
    parents = (hy.parent[7:] - 10).tolist()
    bonds = [(0, 1), (1, 2)] + [(p, 3 + k) for k, p in enumerate(parents)]
    want = ref.records(full.symbols, host[:, full.atom], bonds, None, None, [("pose", np.arange(2), None)], title="protonated")
    assert records == want
    back = parse_sdf("".join(records))
    assert back[1]["elements"] == full.symbols and np.abs(back[1]["coords"][3:] - got["x_h"][1, 7:].double().cpu().numpy()).max() <= 5e-5
    assert base.blocks(x)[0].split("\n")[4:7] == records[0].split("\n")[4:7], "the heavy atoms are the unprotonated record's"
    hole = x_all.clone()
    hole[1, 13 + 9] = NAN                                                   # a ligand hydrogen that was not placed
    with pytest.raises(ValueError, match=r"^3 numbers do not fit"):
        full.blocks(hole)
    hole = x_all.clone()
    hole[1, 13 + 2] = NAN                                                   # a receptor hydrogen is not written
    assert full.blocks(hole, {"pose": torch.arange(2)}) == want


# ------------------------------------------------------------------ the sdf keyword of redock
@pytest.fixture(scope="module")
def small(small_model_inputs):
    from physdock_amd import PhysDock
    cfg, P_, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P_, strict=True)
    return model.cuda().eval(), {k: v.cuda() for k, v in batch.items()}


def same_result(a, b):
    def eq(u, w):
        if isinstance(u, torch.Tensor):
            return isinstance(w, torch.Tensor) and torch.equal(u, w)
        if isinstance(u, dict):
            return isinstance(w, dict) and set(u) == set(w) and all(eq(u[k], w[k]) for k in u)
        return u == w
    return eq(a, b)


def test_redock_writes_the_kept_poses(small):
    from physdock_amd import driver
    from physdock_amd.hydrogens import Hydrogens
    from physdock_amd.scoring import VinaScore
    from physdock_amd.sdfio import SdfTemplate, parse_sdf
    from physdock_amd.validity import PoseValidity
    model, dbatch = small
    lig = torch.nonzero(driver.ligand_atom_mask(dbatch)).flatten().cpu().numpy()
    n_lig = len(lig)
    chain = [(i, i + 1) for i in range(n_lig - 1)]
    t = SdfTemplate.from_batch(dbatch, chain, title="small")
    assert t.n_atoms == n_lig and t.atom.tolist() == lig.tolist() and t.n_pose_atoms == dbatch["x_gt"].shape[0]
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3, vina=VinaScore.from_batch(dbatch, chain),
              validity=PoseValidity.from_batch(dbatch, chain))
    plain = driver.redock(model, dbatch, **kw)
    out = driver.redock(model, dbatch, sdf=t, **kw)
    assert "sdf" not in plain and set(out) == set(plain) | {"sdf"} and same_result({k: out[k] for k in plain}, plain)
    assert set(out["sdf"]) == {"bytes", "offsets", "n_records"} and out["sdf"]["n_records"] == 4 and out["sdf"]["bytes"].is_cuda
    records = SdfTemplate.split(out["sdf"])
    back = parse_sdf("".join(records))
    kept = out["poses"].double().cpu().numpy()
    score, valid, rmsd = out["vina"]["score"].cpu().numpy(), out["validity"]["valid"].cpu().numpy(), out["ranking"]["rmsd_all"].cpu().numpy()
    assert len(back) == 4
    for p, r in enumerate(back):
        assert r["title"] == "small" and r["elements"] == t.symbols and r["bonds"].tolist() == [list(b) for b in chain]
        assert np.abs(r["coords"] - kept[p][lig]).max() <= 5e-5
        assert list(r["properties"].items()) == [("pose", str(p)), ("vina_score", f"{float(score[p]):.4f}"), ("valid", str(int(valid[p]))),
                                                 ("ligand_rmsd", f"{float(rmsd[p]):.4f}")]
    assert records == t.blocks(out["poses"], {"pose": torch.arange(4), "vina_score": out["vina"]["score"], "valid": out["validity"]["valid"],
                                              "ligand_rmsd": out["ranking"]["rmsd_all"]})
    # protonated: the hydrogens= object of the call, and a template made by with_hydrogens of it
    hy = Hydrogens.from_batch(dbatch, chain)
    th = t.with_hydrogens(hy)
    prot = driver.redock(model, dbatch, sdf=th, hydrogens=hy, ranking=False, num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    assert torch.equal(prot["poses"], plain["poses"])
    x_all = torch.cat([prot["poses"], prot["hydrogens"]["x_h"]], 1)
    assert SdfTemplate.split(prot["sdf"]) == th.blocks(x_all, {"pose": torch.arange(4)})
    assert parse_sdf(SdfTemplate.split(prot["sdf"])[0])[0]["elements"] == t.symbols + ["H"] * hy.n_hydrogens
    # redock_many: the sequential and the grouped path
    many = driver.redock_many(model, [(dbatch, {"sdf": t})], **kw)
    assert same_result({k: many[0][k] for k in plain}, plain) and SdfTemplate.split(many[0]["sdf"]) == records
    grouped = driver.redock_many(model, [(dbatch, {"sdf": t})], group=1, **kw)
    assert set(grouped[0]) == set(out) and len(parse_sdf("".join(SdfTemplate.split(grouped[0]["sdf"])))) == 4
    # a template over another atom count is refused before anything is sampled
    other = SdfTemplate.from_bonds([6] * 5, [(0, 1)], [0, 1])
    with pytest.raises(ValueError, match="sdf= was built over 5 pose atoms"):
        driver.redock(model, dbatch, sdf=other, **kw)
    with pytest.raises(ValueError, match="sdf= was protonated"):
        driver.redock(model, dbatch, sdf=th, **kw)
    with pytest.raises(ValueError, match="sdf= was protonated"):
        driver.redock(model, dbatch, sdf=th, hydrogens=Hydrogens.from_batch(dbatch, chain), **kw)
    with pytest.raises(ValueError, match="sdf= takes"):
        driver.redock(model, dbatch, sdf="text", **kw)
    with pytest.raises(ValueError, match="sdf= was built over 5 pose atoms"):
        driver.redock_many(model, [(dbatch, {"sdf": other})], group=1, **kw)
