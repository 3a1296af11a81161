"""Graph automorphisms of a ligand, for the symmetry-corrected ligand RMSD of the ranking step (kernel `pd_sym_rmsd`).

The reference compares atom k of one pose with atom k of the other (redocking.py:382,389-390).  A phenyl ring flipped by 180
degrees, a carboxylate, a CF3 or t-butyl group or a symmetric linker is the same molecule in the same place, and the index-wise
RMSD reports 1 - 2.5 A for it.  The corrected value is the minimum over the automorphisms of the molecular graph (what `obrms`
and spyrmsd report): `automorphisms` enumerates them on the host, once per ligand, from the bond list alone (no RDKit), and
`LigandSymmetry` holds the table in the layout the kernel reads.  `ranking.pairwise_ligand_rmsd(..., symmetry=)`,
`ranking.rank_poses(..., symmetry=)` and `driver.redock(..., ligand_symmetry=)` take it; without it they do what the reference
does.
"""
from __future__ import annotations

import warnings
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .chirality import symmetry_classes

__all__ = ["automorphisms", "LigandSymmetry", "MAX_ATOMS", "MAX_PERMS"]

#: limits of the kernel (csrc/sym_rmsd.hip)
MAX_ATOMS = 1024
MAX_PERMS = 65535


def automorphisms(n_atoms: int, bonds: Iterable[Tuple[int, int]], elements: Optional[Sequence[int]] = None,
                  bond_orders: Optional[Sequence[float]] = None, max_perms: int = 4096, _stacklevel: int = 2):
    """The automorphisms of a molecular graph: (perms int32 [M, n_atoms], complete).  Row m maps atom a to atom perms[m, a]; every
    row keeps elements, adjacency and bond orders.  Backtracking search: atoms are assigned in index order, a candidate image lies
    in the atom's class of `chirality.symmetry_classes`, is unused, and has towards every atom assigned so far the bond (or the
    absence of a bond) the atom itself has.  Candidates are tried in ascending order, so the rows come out in lexicographic order:
    row 0 is the identity and the output is deterministic.  A disconnected graph needs no special case (identical fragments swap).

    A group of more than `max_perms` elements is cut to its first `max_perms` rows of that order and `complete` is False (one
    warning).  The minimum over a truncated table is then an UPPER BOUND of the symmetry-corrected RMSD; it is never above the
    index-wise RMSD, because the identity is always row 0."""
    n_atoms, max_perms = int(n_atoms), int(max_perms)
    if n_atoms < 1 or max_perms < 1:
        raise ValueError("automorphisms: n_atoms and max_perms must be positive")
    bonds = [(int(i), int(j)) for i, j in bonds]
    orders = [1.0] * len(bonds) if bond_orders is None else [round(float(o), 3) for o in bond_orders]
    cls = symmetry_classes(n_atoms, bonds, elements, bond_orders)          # (checks the lengths of elements / bond_orders)
    adj = [dict() for _ in range(n_atoms)]
    for (i, j), o in zip(bonds, orders):
        if not (0 <= i < n_atoms and 0 <= j < n_atoms) or i == j:
            raise ValueError(f"automorphisms: bond ({i}, {j}) of a graph of {n_atoms} atoms")
        adj[i][j] = o; adj[j][i] = o
    members = {}
    for a, c in enumerate(cls):
        members.setdefault(c, []).append(a)
    cand = [members[cls[a]] for a in range(n_atoms)]                         # ascending by construction
    lower = [sorted(b for b in adj[a] if b < a) for a in range(n_atoms)]     # bonds to the atoms assigned before a
    n_lower = [len(x) for x in lower]

    def fits(a, img, image):
        """does a -> img keep the bonds between a and the atoms 0 .. a-1?  Equal class means equal degree, so it is enough that
        every earlier neighbour's image is bonded to img with the same order and that img has no further bond into the images"""
        nb = adj[img]
        for b in lower[a]:
            if nb.get(image[b]) != adj[a][b]:
                return False
        return sum(1 for c in nb if used_by[c] < a) == n_lower[a]

    rows, complete = [], True
    image = [-1] * n_atoms
    used_by = [n_atoms] * n_atoms          # used_by[c]: the atom whose image c is (n_atoms: free)
    pos = [0] * n_atoms                    # next candidate of every depth
    a = 0
    while a >= 0:
        if a == n_atoms:
            if len(rows) == max_perms:
                complete = False
                break
            rows.append(list(image))
            a -= 1
            used_by[image[a]] = n_atoms
            continue
        found = False
        while pos[a] < len(cand[a]):
            img = cand[a][pos[a]]
            pos[a] += 1
            if used_by[img] == n_atoms and fits(a, img, image):
                image[a], used_by[img], found = img, a, True
                break
        if found:
            a += 1
            if a < n_atoms:
                pos[a] = 0
        else:
            a -= 1
            if a >= 0:
                used_by[image[a]] = n_atoms
    if not complete:
        warnings.warn(f"automorphisms: the graph has more than max_perms={max_perms} automorphisms; the table is cut to the first "
                      f"{max_perms} in lexicographic order and the corrected RMSD becomes an upper bound", RuntimeWarning,
                      stacklevel=_stacklevel)
    return np.asarray(rows, dtype=np.int32).reshape(len(rows), n_atoms), complete


class LigandSymmetry:
    """The permutation table of one ligand: `n_atoms`, `n_perms`, `complete` (False: the group was cut at max_perms), `perms`
    (host, int32 [M, n_atoms], identity first) and the table the kernel reads - atom-major unsigned 16-bit [n_atoms, M], packed
    once here and uploaded once per device (`table(device)`).  Atom a is the a-th LIGAND atom, i.e. position a of the
    `ligand_idx` the ranking functions use."""

    def __init__(self, perms, complete: bool = True, device=None):
        p = np.ascontiguousarray(np.asarray(perms))
        if p.ndim != 2 or p.shape[0] < 1 or p.shape[1] < 1 or p.dtype.kind not in "iu":
            raise ValueError("LigandSymmetry: perms must be an integer array [M, n_atoms] with at least one row")
        M, n = p.shape
        if n > MAX_ATOMS or M > MAX_PERMS:
            raise ValueError(f"LigandSymmetry: {n} atoms x {M} permutations; the kernel takes up to {MAX_ATOMS} x {MAX_PERMS}")
        if not np.array_equal(p[0], np.arange(n)):
            raise ValueError("LigandSymmetry: row 0 of the table must be the identity")
        if not np.array_equal(np.sort(p, axis=1), np.broadcast_to(np.arange(n), (M, n))):
            raise ValueError("LigandSymmetry: every row of the table must be a permutation of 0 .. n_atoms-1")
        self.perms = p.astype(np.int32)
        self.n_atoms, self.n_perms, self.complete = int(n), int(M), bool(complete)
        self._packed = np.ascontiguousarray(self.perms.T.astype(np.uint16))      # [n_atoms, M], the permutation index fastest
        self._tables = {}
        if device is not None:
            self.table(device)

    @staticmethod
    def from_bonds(n_atoms, bonds, elements=None, bond_orders=None, max_perms: int = 4096, device=None):
        perms, complete = automorphisms(n_atoms, bonds, elements, bond_orders, min(int(max_perms), MAX_PERMS), _stacklevel=3)
        return LigandSymmetry(perms, complete, device)

    @staticmethod
    def from_rdkit(ref_mol, max_perms: int = 4096, device=None):
        """from an RDKit molecule (or anything with its GetAtoms / GetBonds interface): atomic numbers and bonds with their
        orders as `GetBondTypeAsDouble` gives them (aromatic bonds 1.5).  Pass the molecule whose atoms are the ligand atoms of
        the poses in the same order - the heavy-atom `ref_mol` of the drivers."""
        elements = [int(a.GetAtomicNum()) for a in ref_mol.GetAtoms()]
        bonds, orders = [], []
        for b in ref_mol.GetBonds():
            bonds.append((int(b.GetBeginAtomIdx()), int(b.GetEndAtomIdx())))
            orders.append(float(b.GetBondTypeAsDouble()))
        perms, complete = automorphisms(len(elements), bonds, elements, orders, min(int(max_perms), MAX_PERMS), _stacklevel=3)
        return LigandSymmetry(perms, complete, device)

    @staticmethod
    def from_permutations(perms, complete: bool = True, device=None):
        """an explicit table (row 0 the identity, every row a permutation); it need not be a group"""
        return LigandSymmetry(perms, complete, device)

    def table(self, device) -> torch.Tensor:
        """the packed table on `device`: int16 storage [n_atoms, n_perms] of the unsigned 16-bit entries"""
        return ops.cached_upload(self._tables, device, lambda up: up(self._packed.view(np.int16)))

    def __repr__(self):
        return f"LigandSymmetry(n_atoms={self.n_atoms}, n_perms={self.n_perms}, complete={self.complete})"
