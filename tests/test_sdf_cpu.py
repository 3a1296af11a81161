"""The SD file format of physdock_amd/sdfio.py without a GPU: the reference writer tests/sdf_ref.py against a record typed out by hand
(which pins the written definition itself to the CTfile V2000 specification), the reader `parse_sdf`, the host tables of `SdfTemplate`
(the molblock with blank coordinates, the byte map, the record lengths), `with_hydrogens`, every limit, and the declaration of
`pd_sdf_format`.  The byte-for-byte comparison of the device's output with the reference writer is tests/test_sdf_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch

import sdf_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a 3-atom molecule with one charge, one aromatic bond, one float item and one int item, typed out column by column
BY_HAND = (
    "by hand\n"
    "  physdock          3D\n"
    "\n"
    "  3  2  0  0  0  0  0  0  0  0999 V2000\n"
    "    1.5000   -2.2500    0.0000 C   0  0  0  0  0  0  0  0  0  0  0  0\n"
    "   -0.0312   10.0000   -0.0000 N   0  0  0  0  0  0  0  0  0  0  0  0\n"
    "  123.4568    0.0938    0.0001 Cl  0  0  0  0  0  0  0  0  0  0  0  0\n"
    "  1  2  4  0\n"
    "  2  3  1  0\n"
    "M  CHG  1   2   1\n"
    "M  END\n"
    ">  <score>\n"
    "-7.2500\n"
    "\n"
    ">  <pose>\n"
    "12\n"
    "\n"
    "$$$$\n")
HAND = dict(symbols=["C", "N", "Cl"], coords=[[1.5, -2.25, 0.0], [-0.03125, 9.99995, -0.00004], [123.45678, 0.09375, 0.00006]],
            bonds=[(0, 1), (1, 2)], bond_orders=[1.5, 1.0], charges=[0, 1, 0])


def test_the_reference_writer_is_the_specification():
    got = ref.record(HAND["symbols"], HAND["coords"], HAND["bonds"], HAND["bond_orders"], HAND["charges"],
                     items=[("score", -7.25, 4), ("pose", 12, None)], title="by hand")
    assert got == BY_HAND
    atom_lines = got.split("\n")[4:7]
    assert all(len(ln) == 69 for ln in atom_lines)
    assert ref.value_text(np.float32(2.5), 0) == "2" and ref.value_text(np.float32(-0.4), 0) == "-0" and ref.value_text(float("nan"), 4) == "nan"
    assert ref.value_text(float("-inf"), 2) == "-inf" and ref.value_text(-2 ** 31) == "-2147483648"


def test_eleven_charges_wrap_into_two_lines():
    text = ref.molblock(["N"] * 12, np.zeros((12, 3)), charges=[1, -1, 1, -1, 1, -1, 1, -1, 0, 2, -2, 15])
    chg = [ln for ln in text.split("\n") if ln.startswith("M  CHG")]
    assert chg == ["M  CHG  8   1   1   2  -1   3   1   4  -1   5   1   6  -1   7   1   8  -1", "M  CHG  3  10   2  11  -2  12  15"]


def random_molecule(seed, na, nb, n_charged):
    rng = np.random.default_rng(seed)
    symbols = [["C", "N", "O", "S", "Cl", "Br", "F", "P"][i] for i in rng.integers(0, 8, na)]
    bonds = [(i, i + 1) for i in range(na - 1)]
    while len(bonds) < nb:
        i, j = sorted(rng.choice(na, 2, replace=False).tolist())
        if (i, j) not in bonds:
            bonds.append((i, j))
    bonds = bonds[:nb]
    orders = rng.choice([1.0, 1.5, 2.0, 3.0], len(bonds)).tolist()
    charges = np.zeros(na, dtype=np.int64)
    charges[rng.choice(na, n_charged, replace=False)] = rng.choice([-2, -1, 1, 2], n_charged)
    return symbols, bonds, orders, charges


def test_parse_gives_back_what_was_written():
    from physdock_amd.sdfio import SdfTemplate, parse_sdf
    symbols, bonds, orders, charges = random_molecule(1, 37, 40, 11)
    poses = np.random.default_rng(2).normal(0.0, 30.0, (3, 37, 3)).astype(np.float32)
    props = [("score", np.array([-7.25, 0.5, 1e6], dtype=np.float32), 4), ("pose", np.array([0, 1, 2]), None),
             ("a.b_c", np.array([np.nan, np.inf, -0.0], dtype=np.float32), 2)]
    text = "".join(ref.records(symbols, poses, bonds, orders, charges, props, order=[2, 0, 1], title="t", comment="c"))
    got = parse_sdf(text)
    assert len(got) == 3
    for r, p in zip(got, (2, 0, 1)):
        assert r["title"] == "t" and r["elements"] == symbols and r["bonds"].tolist() == [list(b) for b in bonds]
        assert r["bond_orders"].tolist() == orders and r["charges"].tolist() == charges.tolist()
        assert r["coords"].dtype == np.float64 and np.abs(r["coords"] - poses[p].astype(np.float64)).max() <= 5e-5
        assert list(r["properties"].items()) == [(name, ref.value_text(v[p], d)) for name, v, d in props]
    # the result feeds from_bonds as it is, and the template's text is the text parsed
    r = got[0]
    t = SdfTemplate.from_bonds(r["elements"], r["bonds"], range(len(r["elements"])), r["bond_orders"], r["charges"], title="t", comment="c")
    assert t.molblock == ref.molblock(symbols, None, bonds, orders, charges, title="t", comment="c")
    assert parse_sdf(BY_HAND)[0]["charges"].tolist() == [0, 1, 0] and parse_sdf(BY_HAND)[0]["bond_orders"].tolist() == [1.5, 1.0]
    mol_only = ref.molblock(symbols, poses[0], bonds, orders, charges)            # a lone molfile: no $$$$
    assert len(parse_sdf(mol_only)) == 1 and parse_sdf(mol_only)[0]["properties"] == {}
    assert parse_sdf(text.replace("\n", "\r\n"))[1]["elements"] == symbols
    assert parse_sdf("") == []


def test_parse_refuses_what_it_does_not_read():
    from physdock_amd.sdfio import parse_sdf
    lines = BY_HAND.split("\n")
    v3000 = "\n".join(lines[:3] + ["  0  0  0     0  0            999 V3000"] + lines[4:])
    with pytest.raises(ValueError, match=r"line 4: a V3000"):
        parse_sdf(v3000)
    with pytest.raises(ValueError, match=r"line 7: the atom block is truncated"):
        parse_sdf("\n".join(lines[:6] + lines[7:]))                         # an atom line is gone: a bond line stands in its place
    with pytest.raises(ValueError, match=r"line 6: the file ends"):
        parse_sdf("\n".join(lines[:6]))
    with pytest.raises(ValueError, match=r"line 11: M  END is missing"):
        parse_sdf("\n".join(lines[:10] + lines[11:]))
    with pytest.raises(ValueError, match=r"line 10: M  END is missing"):
        parse_sdf("\n".join(lines[:10]))
    with pytest.raises(ValueError, match=r"line 8: bond type 8"):
        parse_sdf(BY_HAND.replace("  1  2  4  0", "  1  2  8  0"))
    with pytest.raises(ValueError, match=r"line 10: a property line other than M  CHG"):
        parse_sdf(BY_HAND.replace("M  CHG  1   2   1", "M  ISO  1   2  13"))
    with pytest.raises(ValueError, match=r"line 4: not a V2000"):
        parse_sdf(BY_HAND.replace(" V2000", ""))


@pytest.mark.parametrize("na, nb, n_charged", [(1, 0, 0), (3, 2, 1), (37, 40, 11)])
def test_the_host_tables(na, nb, n_charged):
    from physdock_amd import sdfio
    symbols, bonds, orders, charges = random_molecule(na, na, nb, n_charged)
    A = na + 5
    lig = np.arange(A)[::-1][:na].copy()                                   # the ligand's atoms are not the first and not in order
    elements = ["C"] * A
    for s, a in zip(symbols, lig):
        elements[a] = s
    t = sdfio.SdfTemplate.from_bonds(elements, bonds, lig, orders, charges, title="a title", comment="a comment")
    assert (t.n_atoms, t.n_bonds, t.n_pose_atoms) == (na, len(bonds), A) and t.atom.tolist() == lig.tolist() and t.symbols == symbols
    want = ref.molblock(symbols, None, bonds, orders, charges, title="a title", comment="a comment")
    assert t.molblock == want and bytes(t.tmpl) == want.encode("ascii") and t.molblock_bytes == len(want)
    # the reference text of a pose with the coordinate columns blanked is the template; every hole lies in columns 0 - 29 of an atom line
    pose = np.random.default_rng(na).normal(0.0, 9.0, (na, 3)).astype(np.float32)
    full = ref.molblock(symbols, pose, bonds, orders, charges, title="a title", comment="a comment")
    assert len(full) == len(want)
    blanked = bytearray(full.encode("ascii"))
    holes = np.nonzero(t.map >= 0)[0]
    assert len(holes) == 30 * na and t.map.shape == t.tmpl.shape and t.map.dtype == np.int32
    for i in holes:
        blanked[i] = 32
    assert bytes(blanked) == want.encode("ascii")
    line_start = [0] + [m.end() for m in re.finditer("\n", want)]
    for i in holes:
        ln = max(k for k, s in enumerate(line_start) if s <= i)
        slot, col = divmod(int(t.map[i]), 30)
        assert 4 <= ln < 4 + na and slot == ln - 4 and col == i - line_start[ln] and 0 <= col < 30
    assert t.atoms_at == line_start[4] and (t.map[t.map < 0] == -1).all()
    # the fixed record length and the capacity bound
    items = [("score", None, 4), ("pose", None, -1), ("x" * 64, None, 0)]
    fixed, longest = t.record_bytes(items)
    heads = sum(len(f">  <{name}>\n") + 2 for name, _, _ in items)
    assert fixed == len(want) + heads + len("$$$$\n") and longest == fixed + 18 + 11 + 18
    assert t.record_bytes(()) == (len(want) + 5, len(want) + 5)
    worst = ref.items_text([("score", np.float32(-999999986991104.0), 0), ("pose", -2 ** 31, None), ("x" * 64, np.float32(-9999999.0), 8)])
    assert len(want) + len(worst) <= longest and len(ref.value_text(np.float32(-9999999.0), 8)) == 17
    assert len(ref.value_text(np.float32(-999999986991104.0), 0)) == 16 and sdfio.FLOAT_TEXT_MAX == 18 and sdfio.INT_TEXT_MAX == 11


def test_items_from_properties():
    from physdock_amd.sdfio import SdfTemplate
    props = {"f": torch.tensor([1.0, 2.0], dtype=torch.float64), "g": (torch.tensor([1.0, 2.0]), 8), "i": torch.tensor([3, -4]),
             "b": torch.tensor([True, False]), "h": (np.array([0.5, 1.5], dtype=np.float16), 0), "l": [7, 8]}
    items = SdfTemplate.items(props, 2)
    assert [(n, d) for n, _, d in items] == [("f", 4), ("g", 8), ("i", -1), ("b", -1), ("h", 0), ("l", -1)]
    assert all(v.dtype == torch.int32 and v.shape == (2,) for _, v, _ in items)
    assert items[0][1].view(torch.float32).tolist() == [1.0, 2.0] and items[2][1].tolist() == [3, -4] and items[3][1].tolist() == [1, 0]
    assert SdfTemplate.items(None, 2) == []


def test_with_hydrogens_appends_atoms_and_bonds():
    from physdock_amd.hydrogens import BISECT, NERF, TRI, Hydrogens
    from physdock_amd.sdfio import SdfTemplate
    # pose atoms 0 .. 3 receptor (one residue), 4 .. 6 the ligand C - C - O; a hydrogen on receptor atom 0, three on the ligand
    types = np.zeros(7, dtype=np.uint8)
    table = {"parent": np.array([0, 4, 6, 4]), "ref": np.array([[1, 2, 3], [5, 6, -1], [5, 4, -1], [5, 6, -1]]),
             "mode": np.array([TRI, BISECT, NERF, BISECT]), "length": np.full(4, 1.0), "a": np.zeros(4), "b": np.zeros(4), "group": np.full(4, -1)}
    hy = Hydrogens.from_tables(types, [4, 5, 6], np.array([1, 1, 1, 1, 0, 0, 0]), np.array([0, 0, 0, 0, 1, 1, 1]), table, n_residues=2)
    base = SdfTemplate.from_bonds([7, 6, 6, 8, 6, 6, 8], [(0, 1), (1, 2)], [4, 5, 6], [1.0, 2.0], charges=[0, 0, -1], title="lig")
    full = base.with_hydrogens(hy)
    assert full.hydrogens is hy and base.hydrogens is None
    assert full.symbols == ["C", "C", "O", "H", "H", "H"] and full.n_pose_atoms == 7 + 4
    assert full.atom.tolist() == [4, 5, 6, 7 + 1, 7 + 2, 7 + 3], "the receptor's hydrogen (row 0) is not written"
    assert full.bonds.tolist() == [[0, 1], [1, 2], [0, 3], [2, 4], [0, 5]] and full.bond_types.tolist() == [1, 2, 1, 1, 1]
    assert full.charges.tolist() == [0, 0, -1, 0, 0, 0] and full.title == "lig"
    assert full.molblock == ref.molblock(full.symbols, None, full.bonds, [1, 2, 1, 1, 1], full.charges, title="lig")
    other = SdfTemplate.from_bonds([6] * 9, [], [0])
    with pytest.raises(ValueError, match="pose atoms"):
        other.with_hydrogens(hy)


def test_every_limit_raises():
    from physdock_amd.sdfio import SdfTemplate
    ok = lambda **kw: SdfTemplate.from_bonds(**{**dict(elements=[6, 7, 8], bonds=[(0, 1)], ligand_idx=[0, 1, 2]), **kw})
    ok()
    assert SdfTemplate.from_bonds([6] * 999, [(i, i + 1) for i in range(998)] + [(0, 2)], range(999)).n_bonds == 999
    for bad, match in ((dict(elements=[6] * 1000, ligand_idx=range(1000)), "1 .. 999"), (dict(ligand_idx=[]), "1 .. 999"),
                       (dict(elements=[6] * 50, ligand_idx=range(50), bonds=[(i, j) for i in range(50) for j in range(i + 1, 50)][:1000]), "at most 999"),
                       (dict(bond_orders=[2.5]), "1, 1.5, 2 or 3"), (dict(bond_orders=[0.0]), "1, 1.5, 2 or 3"), (dict(bond_orders=[1, 2]), "bond orders"),
                       (dict(bonds=[(0, 3)]), "leaves"), (dict(bonds=[(1, 1)]), "itself"), (dict(ligand_idx=[0, 1, 3]), "leaves"),
                       (dict(charges=[0, 1]), "formal charges"), (dict(charges=[0, 16, 0]), "formal charges"), (dict(elements=[6, 7, 0]), "atomic number"),
                       (dict(elements=["C", "N", "Xx"]), "element symbol"), (dict(title="x" * 81), "title"), (dict(title="a\nb"), "title"),
                       (dict(comment="\t"), "comment"), (dict(program="é"), "program")):
        with pytest.raises(ValueError, match=match):
            ok(**bad)
    v = torch.zeros(2)
    for name in ("", "1a", "a b", "a-b", "x" * 65, "é", 3):
        with pytest.raises(ValueError, match="name"):
            SdfTemplate.items({name: v}, 2)
    assert [n for n, _, _ in SdfTemplate.items({"x" * 64: v, "_a.b9": v}, 2)] == ["x" * 64, "_a.b9"]
    for props, match in (({"a": (v, 9)}, "decimals"), ({"a": (v, -1)}, "decimals"), ({"a": (v, 1.5)}, "decimals"), ({"a": (v, True)}, "decimals"),
                         ({"a": (torch.zeros(2, dtype=torch.int32), 2)}, "no decimals"), ({"a": torch.zeros(3)}, "2 poses"),
                         ({"a": torch.tensor([0, 2 ** 31])}, "int32"), ({"a": (v, 1, 2)}, "decimals"),
                         ({f"a{k}": v for k in range(33)}, "at most 32")):
        with pytest.raises(ValueError, match=match):
            SdfTemplate.items(props, 2)
    assert len(SdfTemplate.items({f"a{k}": v for k in range(32)}, 2)) == 32
    t = ok()
    with pytest.raises(RuntimeError, match="device only"):
        t.format(torch.zeros(1, 3, 3))


def test_the_declaration():
    import ctypes
    from physdock_amd import _lib
    header = open(os.path.join(REPO, "include", "physdock_hip.h")).read()
    assert int(re.search(r"#define\s+PD_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == _lib.ABI_VERSION
    assert "pd_sdf_format" in _lib.header_symbols()
    args = re.search(r"^int pd_sdf_format\((.*?)\);", header, flags=re.M | re.S).group(1)
    n_args = len(args.split(","))
    assert os.path.exists(_lib.LIB_PATH), "build the library first (python -m physdock_amd.build)"
    L = _lib.lib()
    fn = _lib.SYMBOLS["pd_sdf_format"]
    assert len(fn.argtypes) == n_args == 22 and fn.restype is ctypes.c_int and hasattr(L, "pd_sdf_format")
    assert int(re.search(r"#define\s+PD_SDF_MAX_ITEMS\s+(\d+)", header).group(1)) == 32
    import physdock_amd
    assert physdock_amd.SdfTemplate is physdock_amd.sdfio.SdfTemplate and physdock_amd.parse_sdf is physdock_amd.sdfio.parse_sdf
