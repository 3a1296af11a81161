"""Graph automorphisms for the symmetry-corrected ligand RMSD (physdock_amd/symmetry.py), the parts that need no GPU: group
orders and properties of hand-built heavy-atom graphs, truncation, table construction, the float64 restatement
(tests/sym_rmsd_ref.py) on poses that differ by a symmetry operation, and the C ABI of pd_sym_rmsd."""
import math
import os
import re
import warnings

import numpy as np
import pytest

import sym_rmsd_ref as ref
from physdock_amd.symmetry import LigandSymmetry, automorphisms

RING = [(i, (i + 1) % 6) for i in range(6)]
NEOPENTANE = dict(n_atoms=5, bonds=[(0, 1), (0, 2), (0, 3), (0, 4)], elements=[6] * 5)
CARBOXYLATE = dict(n_atoms=4, bonds=[(0, 1), (1, 2), (1, 3)], elements=[6, 6, 8, 8])
FRAGMENT = dict(n_atoms=3, bonds=[(0, 1), (1, 2)], elements=[6, 8, 6])                  # C-O-C: order 2

#: name -> (graph, expected group order)
GRAPHS = {
    "six-ring": (dict(n_atoms=6, bonds=RING, elements=[6] * 6), 12),
    "pyridine": (dict(n_atoms=6, bonds=RING, elements=[7] + [6] * 5, bond_orders=[1.5] * 6), 2),
    "toluene": (dict(n_atoms=7, bonds=RING + [(0, 6)], elements=[6] * 7), 2),
    "neopentane": (NEOPENTANE, 24),
    "biphenyl": (dict(n_atoms=12, bonds=RING + [(6 + i, 6 + (i + 1) % 6) for i in range(6)] + [(0, 6)], elements=[6] * 12), 8),
    "chain of different elements": (dict(n_atoms=4, bonds=[(0, 1), (1, 2), (2, 3)], elements=[6, 7, 8, 16]), 1),
    "carboxylate (2, 1)": (dict(CARBOXYLATE, bond_orders=[1, 2, 1]), 1),
    "carboxylate (1.5, 1.5)": (dict(CARBOXYLATE, bond_orders=[1, 1.5, 1.5]), 2),
    "carboxylate without orders": (CARBOXYLATE, 2),
    "two disjoint fragments": (dict(n_atoms=6, bonds=[(0, 1), (1, 2), (3, 4), (4, 5)], elements=[6, 8, 6, 6, 8, 6]), 2 * 2 ** 2),
}


def bond_map(g):
    orders = g.get("bond_orders") or [1.0] * len(g["bonds"])
    m = {}
    for (i, j), o in zip(g["bonds"], orders):
        m[(i, j)] = m[(j, i)] = float(o)
    return m


@pytest.mark.parametrize("name", list(GRAPHS))
def test_group_order_and_properties(name):
    g, order = GRAPHS[name]
    perms, complete = automorphisms(**g)
    n = g["n_atoms"]
    assert complete and perms.dtype == np.int32 and perms.shape == (order, n)
    assert perms[0].tolist() == list(range(n))
    rows = [tuple(r) for r in perms.tolist()]
    assert rows == sorted(set(rows)), "rows distinct and in lexicographic order"
    bm, el = bond_map(g), g["elements"]
    for r in rows:
        assert sorted(r) == list(range(n))
        assert all(el[r[a]] == el[a] for a in range(n))
        for a in range(n):
            for b in range(n):
                assert bm.get((a, b)) == bm.get((r[a], r[b])), (name, r, a, b)
    table = set(rows)
    for r in rows:                                           # a complete table is a group
        inv = [0] * n
        for a, b in enumerate(r):
            inv[b] = a
        assert tuple(inv) in table
        for s in rows:
            assert tuple(r[s[a]] for a in range(n)) in table
    assert automorphisms(**FRAGMENT)[0].shape[0] == 2        # (the fragment of the disjoint case)


def test_truncation_keeps_the_first_rows_and_warns_once():
    full, complete = automorphisms(**NEOPENTANE)
    assert complete and len(full) == 24
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        cut, complete = automorphisms(**NEOPENTANE, max_perms=5)
    assert len(w) == 1 and issubclass(w[0].category, RuntimeWarning) and w[0].filename == __file__
    assert not complete and np.array_equal(cut, full[:5])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        s = LigandSymmetry.from_bonds(**NEOPENTANE, max_perms=5)
    assert len(w) == 1 and w[0].filename == __file__
    assert not s.complete and s.n_perms == 5 and s.n_atoms == 5 and np.array_equal(s.perms, full[:5])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert automorphisms(**NEOPENTANE, max_perms=24)[1]          # exactly the group: complete, no warning
    assert not w


def test_from_permutations_checks_its_table():
    ok = LigandSymmetry.from_permutations(np.array([[0, 1, 2], [2, 1, 0]]))
    assert (ok.n_atoms, ok.n_perms, ok.complete) == (3, 2, True) and ok.perms.dtype == np.int32
    t = ok.table("cpu")
    assert tuple(t.shape) == (3, 2) and t.tolist() == [[0, 2], [1, 1], [2, 0]] and ok.table("cpu") is t      # atom-major, packed once
    with pytest.raises(ValueError, match="identity"):
        LigandSymmetry.from_permutations(np.array([[2, 1, 0], [0, 1, 2]]))
    with pytest.raises(ValueError, match="permutation"):
        LigandSymmetry.from_permutations(np.array([[0, 1, 2], [0, 0, 2]]))
    with pytest.raises(ValueError, match="permutation"):
        LigandSymmetry.from_permutations(np.array([[0, 1, 2], [0, 1, 3]]))
    with pytest.raises(ValueError):
        LigandSymmetry.from_permutations(np.zeros((0, 3), dtype=np.int64))


class _Atom:
    def __init__(self, z):
        self.z = z

    def GetAtomicNum(self):
        return self.z


class _Bond:
    def __init__(self, i, j, o):
        self.i, self.j, self.o = i, j, o

    def GetBeginAtomIdx(self):
        return self.i

    def GetEndAtomIdx(self):
        return self.j

    def GetBondTypeAsDouble(self):
        return self.o


class _Mol:
    """the six calls of an RDKit molecule that from_rdkit uses, and nothing else"""

    def __init__(self, g):
        orders = g.get("bond_orders") or [1.0] * len(g["bonds"])
        self.atoms = [_Atom(z) for z in g["elements"]]
        self.bonds = [_Bond(i, j, o) for (i, j), o in zip(g["bonds"], orders)]

    def GetAtoms(self):
        return iter(self.atoms)

    def GetBonds(self):
        return iter(self.bonds)


@pytest.mark.parametrize("name", ["pyridine", "biphenyl", "carboxylate (2, 1)", "carboxylate (1.5, 1.5)", "two disjoint fragments"])
def test_from_rdkit_duck_type_equals_from_bonds(name):
    g = GRAPHS[name][0]
    a, b = LigandSymmetry.from_rdkit(_Mol(g)), LigandSymmetry.from_bonds(**g)
    assert np.array_equal(a.perms, b.perms) and a.complete == b.complete and a.n_atoms == g["n_atoms"]
    assert a.n_perms == GRAPHS[name][1]


def ring_coordinates():
    return np.array([[1.39 * math.cos(k * math.pi / 3), 1.39 * math.sin(k * math.pi / 3), 0.0] for k in range(6)])


def tbutyl_coordinates():
    """C(central) - C(quaternary) with three methyls: tetrahedral, 1.53 A"""
    t = 1.53 / math.sqrt(3)
    return np.array([[-t, -t, -t], [0, 0, 0], [t, t, -t], [t, -t, t], [-t, t, t]], dtype=np.float64)


TBUTYL = dict(n_atoms=5, bonds=[(0, 1), (1, 2), (1, 3), (1, 4)], elements=[7, 6, 6, 6, 6])      # N-C(CH3)3


def test_restatement_on_symmetric_copies():
    ring = ring_coordinates()
    c, s = math.cos(math.pi / 3), math.sin(math.pi / 3)
    rotated = ring @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]).T
    perms, _ = automorphisms(6, RING, [6] * 6)
    assert ref.sym_rmsd(ring, rotated, perms) < 1e-12
    assert ref.plain_rmsd(ring, rotated) > 1.0
    tb = tbutyl_coordinates()
    swapped = tb[[0, 1, 3, 2, 4]]
    perms, _ = automorphisms(**TBUTYL)
    assert len(perms) == 6
    assert ref.sym_rmsd(tb, swapped, perms) < 1e-12
    assert ref.plain_rmsd(tb, swapped) > 1.0
    D, r, costs = ref.sym_rmsd_matrix(np.stack([tb, swapped]), None, tb, perms)
    assert D[0, 1] < 1e-12 and D[0, 0] == D[1, 1] == 0 and (r < 1e-12).all() and costs.shape == (2, 6)
    assert int(costs[1].argmin()) == [tuple(p) for p in perms.tolist()].index((0, 1, 3, 2, 4))


def test_abi_header_and_signature():
    from physdock_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "physdock_hip.h")).read()
    assert int(re.search(r"#define\s+PD_ABI_VERSION\s+(\d+)", hdr).group(1)) == 11 == _lib.ABI_VERSION
    assert "pd_sym_rmsd" in _lib.header_symbols()
    src = open(os.path.join(_lib._HERE, "_lib.py")).read()
    n_hdr = len(re.search(r"int\s+pd_sym_rmsd\s*\(([^;]*)\)\s*;", hdr).group(1).split(","))
    n_sig = len(re.search(r'sig\("pd_sym_rmsd",([^\n#]*)\)', src).group(1).split(","))
    assert n_hdr == n_sig == 12


def test_public_interface():
    import inspect
    import physdock_amd
    from physdock_amd import driver, ranking, symmetry
    assert physdock_amd.LigandSymmetry is symmetry.LigandSymmetry and physdock_amd.automorphisms is symmetry.automorphisms
    assert inspect.signature(ranking.pairwise_ligand_rmsd).parameters["symmetry"].default is None
    assert inspect.signature(ranking.rank_poses).parameters["symmetry"].default is None
    assert inspect.signature(driver.redock).parameters["ligand_symmetry"].default is None
    assert inspect.signature(driver._RedockState.__init__).parameters["ligand_symmetry"].default is None
