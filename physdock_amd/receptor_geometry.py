"""Is the RECEPTOR of a pose stereochemically sensible?  Checks of every sampled pose's protein on the device (kernels
`pd_receptor_geometry`, `pd_receptor_dihedrals`; csrc/receptor_geometry.hip).

The model is an all-atom co-folding sampler: every pose carries the receptor the model drew around the ligand, and every ligand measure
of this package (Vina score, burial, fingerprints) is computed against it.  The reference hands its output to PDBFixer and OpenMM
(PhysDock/data/relaxation.py), which repairs or fails on a broken receptor silently.  Here, with d the fp32 distance
sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))) and r a van der Waals radius (`validity.VDW_RADII`):

  bit 0  bond_lengths    a bond outside [0.75, 1.25] x its length in the reference structure
  bit 1  bond_angles     a 1-3 distance outside [0.75, 1.25] x its reference
  bit 2  chirality       V_pose sign(V_ref) <= 0 at a centre, V = (a - c) . ((b - c) x (e - c)) in double: CA of every non-GLY residue
                         (N, C, CB), CB of THR (CA, OG1, CG2) and of ILE (CA, CG1, CG2); centres with |V_ref| < 1e-3 A^3 are dropped
  bit 3  peptide_twist   min(|omega|, 180 - |omega|) > 30 degrees
  bit 4  cis_flip        |omega| < 30 degrees where |omega_ref| > 150 degrees
  bit 5  planarity       an atom more than 0.25 A off its group's least-squares plane (double, the method of validity.hip): the ring
                         or the carboxylate / amide / guanidinium group of PHE TYR TRP HIS ARG ASP GLU ASN GLN with the atom it hangs
                         on, and every peptide plane CA C O N' CA'
  bit 6  clash           an active pair i < j, more than three bonds apart and not already clashing in the reference structure, with
                         d / (r_i + r_j) < 0.7

The ratio defaults are those of `PoseValidity` (PoseBusters' ligand defaults); the angles are this package's own.  **None of them has
been validated for proteins.**  A non-finite coordinate fails every term and pair it enters (sentinels: +inf for a ratio, a twist or a
plane distance, -inf for a signed volume, 0 for a clash ratio).  Bonds come from a table of the 20 standard residues by atom name (no
RDKit), the peptide bond C(i) - N(i+1) by the "previous residue" rule of `receptor_hydrogens_from_names`, disulfides from SG - SG
within 2.5 A in the reference.  A residue without a table (nucleic acids, modified residues, ligands) is inactive: it takes part in
nothing and its atoms are counted in `untyped`.

`dihedrals(x_pred)` gives phi, psi, omega and chi1 - chi4 of every residue in degrees - atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3))
in double from the fp32 coordinates, rounded once, NaN where an atom is missing, a coordinate is not finite or a cross product is
shorter than 1e-6 - and `chi_recovery` counts the side-chain chis of a pose that lie within a tolerance of the reference's.

Out of scope: ideal-value libraries (Engh & Huber), Ramachandran or rotamer probabilities, hydrogens, nucleic acids and modified
residues, the LEU / VAL / ARG naming-swap symmetries in `chi_recovery`, repairing anything, rejecting poses while sampling.

`ReceptorGeometry` holds one system's tables, built once on the host; `check`, `dihedrals` and `chi_recovery` return device tensors
and never synchronise.  `driver.redock(..., receptor_geometry=)` reports them for the kept poses.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import ReceptorThresholds
from .scoring import _STANDARD, _SYMBOL_Z, _host, names_from_meta
from .validity import DEFAULT_RADIUS, VDW_RADII

__all__ = ["ReceptorGeometry", "CHECK_NAMES", "DEFAULT_THRESHOLDS", "ANGLE_NAMES", "MAX_ATOMS", "MAX_RESIDUES", "TERM_WIDTH",
           "residue_bonds_from_names", "dihedral_table_from_names", "dihedrals_host"]

#: limits of the kernels (csrc/receptor_geometry.hip)
MAX_ATOMS, MAX_RESIDUES, MAX_POSES, TERM_WIDTH = 4096, 4096, 65535, 10
#: failed-check names in flag-bit order
CHECK_NAMES = ("bond_lengths", "bond_angles", "chirality", "peptide_twist", "cis_flip", "planarity", "clash")
#: the first eight in the field order of pd_receptor_thresholds; `trans` (degrees: the reference omega counts as trans beyond it) is
#: used on the host
DEFAULT_THRESHOLDS = {"bond_lo": 0.75, "bond_hi": 1.25, "angle_lo": 0.75, "angle_hi": 1.25, "clash": 0.7, "planarity": 0.25, "twist": 30.0,
                      "cis": 30.0, "trans": 150.0}
#: the columns of `dihedrals`
ANGLE_NAMES = ("phi", "psi", "omega", "chi1", "chi2", "chi3", "chi4")
MIN_CHIRAL_VOLUME = 1e-3            # A^3
DISULFIDE = 2.5                     # A
_CHUNK = 256                        # rows of the reference-clash search held at a time

# heavy-atom bonds of the side chains beyond CB (the backbone N-CA, CA-C, C-O and CA-CB are added for every residue that has them)
_AROMATIC_6 = [("CB", "CG"), ("CG", "CD1"), ("CG", "CD2"), ("CD1", "CE1"), ("CD2", "CE2"), ("CE1", "CZ"), ("CE2", "CZ")]
_SIDE_BONDS = {
    "GLY": [], "ALA": [], "SER": [("CB", "OG")], "CYS": [("CB", "SG")], "VAL": [("CB", "CG1"), ("CB", "CG2")],
    "THR": [("CB", "OG1"), ("CB", "CG2")], "LEU": [("CB", "CG"), ("CG", "CD1"), ("CG", "CD2")],
    "ILE": [("CB", "CG1"), ("CB", "CG2"), ("CG1", "CD1")], "MET": [("CB", "CG"), ("CG", "SD"), ("SD", "CE")],
    "PRO": [("CB", "CG"), ("CG", "CD"), ("CD", "N")], "PHE": _AROMATIC_6, "TYR": _AROMATIC_6 + [("CZ", "OH")],
    "TRP": [("CB", "CG"), ("CG", "CD1"), ("CG", "CD2"), ("CD1", "NE1"), ("NE1", "CE2"), ("CD2", "CE2"), ("CD2", "CE3"), ("CE2", "CZ2"),
            ("CE3", "CZ3"), ("CZ2", "CH2"), ("CZ3", "CH2")],
    "ASP": [("CB", "CG"), ("CG", "OD1"), ("CG", "OD2")], "GLU": [("CB", "CG"), ("CG", "CD"), ("CD", "OE1"), ("CD", "OE2")],
    "ASN": [("CB", "CG"), ("CG", "OD1"), ("CG", "ND2")], "GLN": [("CB", "CG"), ("CG", "CD"), ("CD", "OE1"), ("CD", "NE2")],
    "HIS": [("CB", "CG"), ("CG", "ND1"), ("CG", "CD2"), ("ND1", "CE1"), ("CD2", "NE2"), ("CE1", "NE2")],
    "LYS": [("CB", "CG"), ("CG", "CD"), ("CD", "CE"), ("CE", "NZ")],
    "ARG": [("CB", "CG"), ("CG", "CD"), ("CD", "NE"), ("NE", "CZ"), ("CZ", "NH1"), ("CZ", "NH2")],
}
assert set(_SIDE_BONDS) == set(_STANDARD)
_BACKBONE = [("N", "CA"), ("CA", "C"), ("C", "O")]

# this package's own chi table: chi1 = N CA CB G, chi2 = CA CB G X, ...
_CHI = {
    "SER": ["OG"], "CYS": ["SG"], "THR": ["OG1"], "VAL": ["CG1"], "ILE": ["CG1", "CD1"], "LEU": ["CG", "CD1"], "PHE": ["CG", "CD1"],
    "TYR": ["CG", "CD1"], "TRP": ["CG", "CD1"], "ASN": ["CG", "OD1"], "ASP": ["CG", "OD1"], "HIS": ["CG", "ND1"], "PRO": ["CG", "CD"],
    "MET": ["CG", "SD", "CE"], "GLN": ["CG", "CD", "OE1"], "GLU": ["CG", "CD", "OE1"], "LYS": ["CG", "CD", "CE", "NZ"],
    "ARG": ["CG", "CD", "NE", "CZ"], "GLY": [], "ALA": [],
}
#: the chis compared modulo 180 degrees: (residue, chi number)
PI_PERIODIC = (("ASP", 2), ("GLU", 3), ("PHE", 2), ("TYR", 2))
_PLANAR = {
    "PHE": ("CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ"), "TYR": ("CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ", "OH"),
    "TRP": ("CB", "CG", "CD1", "CD2", "NE1", "CE2", "CE3", "CZ2", "CZ3", "CH2"), "HIS": ("CB", "CG", "ND1", "CD2", "CE1", "NE2"),
    "ARG": ("CD", "NE", "CZ", "NH1", "NH2"), "ASP": ("CB", "CG", "OD1", "OD2"), "GLU": ("CG", "CD", "OE1", "OE2"),
    "ASN": ("CB", "CG", "OD1", "ND2"), "GLN": ("CG", "CD", "OE1", "NE2"),
}
_CHIRAL_CB = {"THR": ("CB", "CA", "OG1", "CG2"), "ILE": ("CB", "CA", "CG1", "CG2")}


def residue_template_bonds(name: str) -> List[Tuple[str, str]]:
    """the heavy-atom bonds of one standard residue by atom name, without OXT ([] for a residue without a table)"""
    name = str(name).strip().upper()
    if name not in _SIDE_BONDS:
        return []
    return _BACKBONE + ([] if name == "GLY" else [("CA", "CB")]) + list(_SIDE_BONDS[name])


def _table_atoms(name: str) -> set:
    return {a for b in residue_template_bonds(name) for a in b} | ({"OXT"} if name in _SIDE_BONDS else set())


class _Residues:
    """atoms grouped into residues by name: `atoms[s]` {atom name: index}, `kind[s]` the residue name, `next_of(s)` the residue the
    peptide bond of s leads to (id one higher, same chain, numbered one higher) or None"""

    def __init__(self, res_names, atom_names, residue_of, mask=None, chain_of=None, residue_number=None, what="receptor geometry"):
        res = _host(residue_of, np.int64).reshape(-1)
        n = res.shape[0]
        if not len(res_names) == len(atom_names) == n:
            raise ValueError(f"{what}: {len(res_names)} residue names, {len(atom_names)} atom names, {n} residue ids")
        ok = np.ones(n, dtype=bool) if mask is None else _host(mask, np.float64).reshape(-1) > 0
        self.chain = None if chain_of is None else _host(chain_of, np.int64).reshape(-1)
        self.number = None if residue_number is None else _host(residue_number, np.int64).reshape(-1)
        if ok.shape[0] != n or (self.chain is not None and self.chain.shape[0] != n) or (self.number is not None and self.number.shape[0] != n):
            raise ValueError(f"{what}: {n} atoms, but a mask, chain_of or residue_number of another length")
        if n and res.min() < 0:
            raise ValueError(f"{what}: residue ids must not be negative")
        self.n, self.residue_of, self.mask = n, res, ok
        self.atoms: Dict[int, Dict[str, int]] = {}
        self.kind: Dict[int, str] = {}
        for a in range(n):
            if ok[a]:
                self.atoms.setdefault(int(res[a]), {}).setdefault(str(atom_names[a]).strip().upper(), a)
                self.kind.setdefault(int(res[a]), str(res_names[a]).strip().upper())

    def tabled(self):
        return [s for s in sorted(self.atoms) if self.kind[s] in _SIDE_BONDS]

    def next_of(self, s):
        """the tabled residue s + 1 when C of s and N of s + 1 exist and the chain and the numbering continue, else None"""
        cur, nxt = self.atoms.get(s, {}), self.atoms.get(s + 1, {})
        if self.kind.get(s) not in _SIDE_BONDS or self.kind.get(s + 1) not in _SIDE_BONDS or "C" not in cur or "N" not in nxt:
            return None
        c, n = cur["C"], nxt["N"]
        if self.chain is not None and self.chain[c] != self.chain[n]:
            return None
        if self.number is not None and self.number[c] + 1 != self.number[n]:
            return None
        return s + 1


def residue_bonds_from_names(res_names: Sequence[str], atom_names: Sequence[str], residue_of, mask=None, chain_of=None,
                             residue_number=None, extra_bonds=None) -> np.ndarray:
    """The heavy-atom bonds of a receptor by residue and atom names, int32 [n,2] (i < j, sorted) of indices into the arguments: the
    table of the 20 standard residues, OXT - C where OXT is present, and the peptide bond C(i) - N(i+1) by the "previous residue" rule
    of `receptor_hydrogens_from_names` (residue id one lower, the same chain when `chain_of` [n] is given, numbered one lower when
    `residue_number` [n] is).  Atoms with equal `residue_of` form a residue; `mask` [n] (default: all): 0 = the atom does not exist.  A
    missing atom drops its bonds, a residue without a table gets none.  `extra_bonds`: further (i, j) pairs (a disulfide, a
    cross-link).  Bonds inside a residue without OXT: GLY 3, ALA 4, SER 5, CYS 5, VAL 6, THR 6, LEU 7, ILE 7, MET 7, PRO 7, PHE 11, TYR
    12, TRP 15, ASP 7, GLU 8, ASN 7, GLN 8, HIS 10, LYS 8, ARG 10."""
    rs = _Residues(res_names, atom_names, residue_of, mask, chain_of, residue_number, "residue_bonds_from_names")
    bonds = set()
    for s in rs.tabled():
        atoms = rs.atoms[s]
        for a, b in residue_template_bonds(rs.kind[s]) + [("C", "OXT")]:
            if a in atoms and b in atoms:
                bonds.add((min(atoms[a], atoms[b]), max(atoms[a], atoms[b])))
        if rs.next_of(s) is not None:
            c, n = atoms["C"], rs.atoms[s + 1]["N"]
            bonds.add((min(c, n), max(c, n)))
    for i, j in (extra_bonds.tolist() if hasattr(extra_bonds, "tolist") else (extra_bonds or [])):
        i, j = int(i), int(j)
        if not (0 <= i < rs.n and 0 <= j < rs.n) or i == j:
            raise ValueError(f"residue_bonds_from_names: the extra bond ({i}, {j}) leaves the {rs.n} atoms or joins an atom to itself")
        bonds.add((min(i, j), max(i, j)))
    return np.asarray(sorted(bonds), dtype=np.int32).reshape(-1, 2)


def dihedral_table_from_names(res_names, atom_names, residue_of, n_residues=None, mask=None, chain_of=None, residue_number=None):
    """(dih int32 [R,7,4], pi_periodic bool [R,4]): the atoms of phi = C(i-1) N CA C, psi = N CA C N(i+1), omega = CA C N(i+1) CA(i+1)
    and chi1 - chi4 (this package's table: `_CHI`) of every residue, -1 where an atom is missing, the chain ends or the residue has no
    table; pi_periodic marks ASP chi2, GLU chi3, PHE chi2 and TYR chi2"""
    rs = _Residues(res_names, atom_names, residue_of, mask, chain_of, residue_number, "dihedral_table_from_names")
    R = int(n_residues) if n_residues is not None else (int(rs.residue_of.max()) + 1 if rs.n else 0)
    dih = -np.ones((R, 7, 4), dtype=np.int32)
    pi = np.zeros((R, 4), dtype=bool)
    for s in rs.tabled():
        if s >= R:
            raise ValueError(f"dihedral_table_from_names: residue id {s} with n_residues = {R}")
        at, name = rs.atoms[s], rs.kind[s]
        rows = {}
        if rs.next_of(s - 1) is not None:
            rows[0] = (rs.atoms[s - 1]["C"], at.get("N"), at.get("CA"), at.get("C"))
        if rs.next_of(s) is not None:
            nx = rs.atoms[s + 1]
            rows[1] = (at.get("N"), at.get("CA"), at.get("C"), nx.get("N"))
            rows[2] = (at.get("CA"), at.get("C"), nx.get("N"), nx.get("CA"))
        chain = ["N", "CA", "CB"] + _CHI[name]
        for k in range(len(_CHI[name])):
            rows[3 + k] = tuple(at.get(a) for a in chain[k:k + 4])
            pi[s, k] = (name, k + 1) in PI_PERIODIC
        for k, row in rows.items():
            if all(a is not None for a in row):
                dih[s, k] = row
    return dih, pi


def dihedrals_host(x, dih) -> np.ndarray:
    """the kernel's dihedral in numpy float64: x [..., A, 3] (rounded to fp32 first), dih [..., 4] indices -> degrees, NaN where undefined"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    dih = np.asarray(dih, dtype=np.int64)
    ok = (dih >= 0).all(-1)
    p = x[..., np.where(dih >= 0, dih, 0), :]
    b1, b2, b3 = p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 1, :], p[..., 3, :] - p[..., 2, :]
    with np.errstate(invalid="ignore"):
        m, n = np.cross(b1, b2), np.cross(b2, b3)
        w = np.degrees(np.arctan2(np.sqrt((b2 * b2).sum(-1)) * (b1 * n).sum(-1), (m * n).sum(-1)))
        ok = ok & np.isfinite(p).all((-1, -2)) & ((m * m).sum(-1) >= 1e-12) & ((n * n).sum(-1) >= 1e-12)
    return np.where(ok, w, np.nan)


def _csr(rows: List[Iterable[int]]) -> Tuple[np.ndarray, np.ndarray]:
    start = np.zeros(len(rows) + 1, dtype=np.int32)
    flat: List[int] = []
    for k, r in enumerate(rows):
        flat.extend(sorted(r))
        start[k + 1] = len(flat)
    return start, np.asarray(flat, dtype=np.int32)


def _thresholds(thresholds) -> Dict[str, float]:
    t = dict(DEFAULT_THRESHOLDS)
    unknown = set(thresholds or {}) - set(DEFAULT_THRESHOLDS)
    if unknown:
        raise ValueError(f"ReceptorGeometry: unknown thresholds {sorted(unknown)}; known: {sorted(DEFAULT_THRESHOLDS)}")
    t.update({k: float(v) for k, v in (thresholds or {}).items()})
    return t


_DEVICE_KEYS = ("radius_signed", "excl_start", "excl_atom", "term_atoms", "term_ref", "res_term_start", "res_term", "res_atom_start",
                "res_atom", "dih")


class ReceptorGeometry:
    """One system's tables for `pd_receptor_geometry` and `pd_receptor_dihedrals`: host copies (numpy: `active`, `radius`,
    `residue_of`, `pair12`, `d12_ref`, `pair13`, `d13_ref`, `centres`, `centre_sign`, `peptides`, `peptide_trans`, `groups`, `excl_start`,
    `excl_atom`, `reference_clashes`, `term_atoms`, `term_ref`, `res_term_start`, `res_term`, `res_atom_start`, `res_atom`, `dih`,
    `pi_periodic`, `chi_ref`, `thresholds`) and, uploaded once per device, what the kernels read.  `n_pose_atoms` is the A of the poses
    `check` takes, `n_residues` R, `untyped` the number of existing atoms that take no part."""

    def __init__(self, tables: Dict[str, np.ndarray], thresholds: Dict[str, float], residue_labels=None, device=None):
        self.__dict__.update(tables)
        self.thresholds = dict(thresholds)
        self.n_pose_atoms, self.n_residues = int(self.radius.shape[0]), int(self.dih.shape[0])
        self.n_terms = int(self.term_atoms.shape[0])
        self.term_counts = (len(self.pair12), len(self.pair13), len(self.centres), len(self.peptides), len(self.groups))
        self.residue_labels = list(residue_labels) if residue_labels is not None else [f"residue {r}" for r in range(self.n_residues)]
        if len(self.residue_labels) != self.n_residues:
            raise ValueError(f"ReceptorGeometry: {len(self.residue_labels)} residue labels for {self.n_residues} residues")
        self._thr = ReceptorThresholds(*[self.thresholds[k] for k in list(DEFAULT_THRESHOLDS)[:8]])
        self._tables = {}
        if device is not None:
            self.tables(device)

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_tables(active, radius, residue_of, bonds, x_ref, centres=(), peptides=(), groups=(), dih=None, pi_periodic=None,
                    n_residues: Optional[int] = None, n_existing: Optional[int] = None, thresholds: Optional[dict] = None,
                    residue_labels=None, device=None):
        """Everything explicit, in pose-atom indices: active [A] (1 = the atom takes part), radius [A] (A), residue_of [A], bonds
        [n,2] between active atoms, x_ref [A,3] the reference structure (finite on every active atom), centres [n,4] (centre, a, b, c),
        peptides [n,4] (CA, C, N', CA'), groups (4 .. 10 atoms each), dih [R,7,4] and pi_periodic [R,4] (`dihedral_table_from_names`).
        `n_existing`: the number of atoms that exist (default: the active ones), for `untyped`."""
        act = _host(active, np.float64).reshape(-1) > 0
        A = act.shape[0]
        rad = _host(radius, np.float32).reshape(-1)
        res = _host(residue_of, np.int64).reshape(-1)
        xr = _host(x_ref, np.float64)
        if rad.shape[0] != A or res.shape[0] != A or xr.shape != (A, 3):
            raise ValueError(f"ReceptorGeometry: active is given for {A} atoms, radius for {rad.shape[0]}, residue_of for {res.shape[0]}, "
                             f"x_ref has shape {tuple(xr.shape)}")
        if n_residues is not None:
            R = int(n_residues)
        else:
            R = int(np.asarray(dih).shape[0]) if dih is not None else (int(res.max()) + 1 if A else 0)
        if not 1 <= A <= MAX_ATOMS or R > MAX_RESIDUES:
            raise ValueError(f"ReceptorGeometry: {A} atoms in {R} residues; the kernels take 1 .. {MAX_ATOMS} atoms in up to {MAX_RESIDUES} "
                             "residues")
        if act.any() and (res[act].min() < 0 or res[act].max() >= R):
            raise ValueError(f"ReceptorGeometry: residue ids of atoms that take part must lie in 0 .. {R - 1}")
        if not np.isfinite(xr[act]).all():
            raise ValueError("ReceptorGeometry: the reference structure is not finite on every atom that takes part")
        if (rad[act] <= 0).any():
            raise ValueError("ReceptorGeometry: van der Waals radii must be positive")
        t = _thresholds(thresholds)

        def rows(what, table, lo, hi):
            out = []
            for row in (table.tolist() if hasattr(table, "tolist") else table):
                row = [int(a) for a in row if int(a) >= 0]
                if not lo <= len(row) <= hi or len(set(row)) != len(row) or min(row) < 0 or max(row) >= A or not act[row].all():
                    raise ValueError(f"ReceptorGeometry: a {what} holds {lo} .. {hi} distinct active atoms below {A}, got {row}")
                out.append(row)
            return out

        bonds = sorted({(min(i, j), max(i, j)) for i, j in rows("bond", bonds, 2, 2)})
        nb = [set() for _ in range(A)]
        for i, j in bonds:
            nb[i].add(j); nb[j].add(i)
        bonded = set(bonds)
        p13 = set()
        for b in range(A):
            for a in nb[b]:
                for c in nb[b]:
                    if a < c and (a, c) not in bonded:
                        p13.add((a, c))
        near = set(bonded) | p13
        for b, c in bonds:                                              # 1-4: the ends of every chain a - b - c - d
            for a in nb[b] - {c}:
                for d in nb[c] - {b}:
                    if a != d:
                        near.add((min(a, d), max(a, d)))
        pair12 = np.asarray(bonds, dtype=np.int32).reshape(-1, 2)
        pair13 = np.asarray(sorted(p13), dtype=np.int32).reshape(-1, 2)
        dist = lambda p: np.linalg.norm(xr[p[:, 0]] - xr[p[:, 1]], axis=-1).astype(np.float32)
        d12, d13 = dist(pair12), dist(pair13)
        if (d12 <= 0).any() or (d13 <= 0).any():
            raise ValueError("ReceptorGeometry: two bonded or 1-3 atoms of the reference structure coincide")
        # pairs that clash in the reference already: found in chunks of rows, never as an A x A matrix
        idx = np.nonzero(act)[0]
        xa, ra = xr[idx], rad[idx].astype(np.float64)
        ref_clash = []
        for k0 in range(0, len(idx), _CHUNK):
            d = np.linalg.norm(xa[k0:k0 + _CHUNK, None, :] - xa[None, :, :], axis=-1)
            hit = d / (ra[k0:k0 + _CHUNK, None] + ra[None, :]) < t["clash"]
            for a, b in zip(*np.nonzero(hit)):
                i, j = int(idx[k0 + a]), int(idx[b])
                if i < j and (i, j) not in near:
                    ref_clash.append((i, j))
        excl = [set() for _ in range(A)]
        for i, j in list(near) + ref_clash:
            excl[i].add(j)
        excl_start, excl_atom = _csr(excl)
        # chiral centres, peptide terms, planar groups
        cen = np.asarray(rows("chiral centre", centres, 4, 4), dtype=np.int32).reshape(-1, 4)
        v = xr[cen[:, 1:]] - xr[cen[:, :1]]
        vol = (v[:, 0] * np.cross(v[:, 1], v[:, 2])).sum(-1)
        keep = np.abs(vol) >= MIN_CHIRAL_VOLUME
        cen, sign = cen[keep], np.sign(vol[keep]).astype(np.float32)
        pep = np.asarray(rows("peptide term", peptides, 4, 4), dtype=np.int32).reshape(-1, 4)
        w_ref = dihedrals_host(xr, pep) if len(pep) else np.zeros(0)
        pep, w_ref = pep[~np.isnan(w_ref)], w_ref[~np.isnan(w_ref)]
        trans = (np.abs(w_ref) > t["trans"]).astype(np.float32)
        grp = rows("planar group", groups, 4, TERM_WIDTH)
        owner = lambda row: int(min(res[a] for a in row))

        def by_owner(table, *others):
            order = sorted(range(len(table)), key=lambda k: owner([a for a in table[k] if a >= 0]))
            return [np.asarray(o)[order] if len(order) else np.asarray(o) for o in (np.asarray(table),) + others]

        pair12, d12 = by_owner(pair12, d12)
        pair13, d13 = by_owner(pair13, d13)
        cen, sign = by_owner(cen, sign)
        pep, trans, w_ref = by_owner(pep, trans, w_ref)
        gtab = -np.ones((len(grp), TERM_WIDTH), dtype=np.int32)
        for g, row in enumerate(grp):
            gtab[g, :len(row)] = row
        gtab, = by_owner(gtab)
        gtab = gtab.reshape(-1, TERM_WIDTH)
        T = len(pair12) + len(pair13) + len(cen) + len(pep) + len(gtab)
        term_atoms = -np.ones((T, TERM_WIDTH), dtype=np.int32)
        term_ref = np.zeros(T, dtype=np.float32)
        at = 0
        for table, ref in ((pair12, d12), (pair13, d13), (cen, sign), (pep, trans), (gtab, np.zeros(len(gtab), np.float32))):
            if not len(ref):
                continue
            table = np.asarray(table, dtype=np.int32).reshape(len(ref), -1)
            term_atoms[at:at + len(ref), :table.shape[1]] = table
            term_ref[at:at + len(ref)] = ref
            at += len(ref)
        res_terms = [set() for _ in range(R)]
        for k in range(T):
            for a in term_atoms[k]:
                if a >= 0:
                    res_terms[res[a]].add(k)
        res_atoms = [set() for _ in range(R)]
        for a in idx:
            res_atoms[res[a]].add(int(a))
        res_term_start, res_term = _csr(res_terms)
        res_atom_start, res_atom = _csr(res_atoms)
        dih = -np.ones((R, 7, 4), dtype=np.int32) if dih is None else np.ascontiguousarray(np.asarray(dih, dtype=np.int32))
        pi = np.zeros((R, 4), dtype=bool) if pi_periodic is None else np.asarray(pi_periodic).astype(bool)
        if dih.shape != (R, 7, 4) or pi.shape != (R, 4) or (dih.size and (dih.min() < -1 or dih.max() >= A)):
            raise ValueError(f"ReceptorGeometry: dih is [{R},7,4] of atom indices below {A} (-1 = undefined), pi_periodic [{R},4]")
        if (dih >= 0).any() and not act[dih[dih >= 0]].all():
            raise ValueError("ReceptorGeometry: a dihedral names an atom that takes no part")
        tables = dict(active=act.astype(np.uint8), radius=rad, radius_signed=np.where(act, rad, -np.abs(rad) - (rad == 0)).astype(np.float32),
                      residue_of=res.astype(np.int32), pair12=pair12.reshape(-1, 2), d12_ref=d12, pair13=pair13.reshape(-1, 2), d13_ref=d13,
                      centres=cen.reshape(-1, 4), centre_sign=sign, peptides=pep.reshape(-1, 4), peptide_trans=trans, omega_ref=w_ref,
                      groups=gtab, excl_start=excl_start, excl_atom=excl_atom,
                      reference_clashes=np.asarray(sorted(ref_clash), dtype=np.int32).reshape(-1, 2), term_atoms=term_atoms, term_ref=term_ref,
                      res_term_start=res_term_start, res_term=res_term, res_atom_start=res_atom_start, res_atom=res_atom, dih=dih,
                      pi_periodic=pi, chi_ref=dihedrals_host(xr, dih)[:, 3:7] if R else np.zeros((0, 4)),
                      untyped=int((n_existing if n_existing is not None else act.sum()) - act.sum()))
        return ReceptorGeometry(tables, t, residue_labels, device)

    @staticmethod
    def from_names(res_names: Sequence[str], atom_names: Sequence[str], residue_of, x_ref, mask=None, chain_of=None, residue_number=None,
                   extra_bonds=None, n_residues: Optional[int] = None, radii: Optional[dict] = None, thresholds: Optional[dict] = None,
                   residue_labels=None, device=None):
        """from residue and atom names (one per pose atom): the bonds of `residue_bonds_from_names` plus the disulfides (CYS SG - SG
        within 2.5 A in `x_ref`), the centres, planar groups, peptide terms and dihedrals of the module's tables.  An atom takes part
        when `mask` says it exists and its residue's table names it; every other existing atom is counted in `untyped`.  The radius
        follows the element, read from the atom name's first letter (the tables hold C, N, O and S only); `radii={Z: r}` overrides."""
        rs = _Residues(res_names, atom_names, residue_of, mask, chain_of, residue_number, "ReceptorGeometry")
        xr = _host(x_ref, np.float64)
        if xr.shape != (rs.n, 3):
            raise ValueError(f"ReceptorGeometry: the names are over {rs.n} atoms, x_ref has shape {tuple(xr.shape)}")
        R = int(n_residues) if n_residues is not None else (int(rs.residue_of.max()) + 1 if rs.n else 0)
        if not 1 <= rs.n <= MAX_ATOMS or R > MAX_RESIDUES:
            raise ValueError(f"ReceptorGeometry: {rs.n} atoms in {R} residues; the kernels take 1 .. {MAX_ATOMS} atoms in up to "
                             f"{MAX_RESIDUES} residues")
        table = dict(VDW_RADII)
        table.update({int(z): float(r) for z, r in (radii or {}).items()})
        active = np.zeros(rs.n, dtype=bool)
        radius = np.full(rs.n, DEFAULT_RADIUS, dtype=np.float32)
        sg = []
        for s in rs.tabled():
            known = _table_atoms(rs.kind[s])
            for name, a in rs.atoms[s].items():
                if name in known:
                    active[a] = True
                    radius[a] = table.get(_SYMBOL_Z.get(name[0], 0), DEFAULT_RADIUS)
            if rs.kind[s] == "CYS" and "SG" in rs.atoms[s]:
                sg.append(rs.atoms[s]["SG"])
        if not np.isfinite(xr[active]).all():
            raise ValueError("ReceptorGeometry: the reference structure is not finite on every atom that takes part")
        extra = [(int(i), int(j)) for i, j in (extra_bonds.tolist() if hasattr(extra_bonds, "tolist") else (extra_bonds or []))]
        for k, i in enumerate(sg):
            for j in sg[k + 1:]:
                if np.linalg.norm(xr[i] - xr[j]) <= DISULFIDE:
                    extra.append((i, j))
        bonds = residue_bonds_from_names(res_names, atom_names, residue_of, mask, chain_of, residue_number, extra)
        if len(bonds) and not active[bonds].all():
            raise ValueError("ReceptorGeometry: an extra bond names an atom that takes no part")
        centres, peptides, groups = [], [], []
        for s in rs.tabled():
            at, name = rs.atoms[s], rs.kind[s]
            pick = lambda names, src=at: [src[a] for a in names] if all(a in src for a in names) else None
            for c in ([("CA", "N", "C", "CB")] if name != "GLY" else []) + ([_CHIRAL_CB[name]] if name in _CHIRAL_CB else []):
                if pick(c):
                    centres.append(pick(c))
            if name in _PLANAR and pick(_PLANAR[name]):
                groups.append(pick(_PLANAR[name]))
            if rs.next_of(s) is not None:
                nx = rs.atoms[s + 1]
                if "CA" in at and "CA" in nx:
                    peptides.append([at["CA"], at["C"], nx["N"], nx["CA"]])
                    if "O" in at:
                        groups.append([at["CA"], at["C"], at["O"], nx["N"], nx["CA"]])
        dih, pi = dihedral_table_from_names(res_names, atom_names, residue_of, R, mask, chain_of, residue_number)
        return ReceptorGeometry.from_tables(active, radius, rs.residue_of, bonds, xr, centres, peptides, groups, dih, pi, n_residues=R,
                                            n_existing=int(rs.mask.sum()), thresholds=thresholds, residue_labels=residue_labels, device=device)

    @staticmethod
    def from_batch(batch, infer_meta_data, x_ref=None, thresholds=None, **kw):
        """from a feature dict and the loader's naming tables (`scoring.names_from_meta`): a residue is a token, the receptor is every
        existing heavy atom (`a_mask`) that is not of a ligand token, chains and residue numbers come from the batch's `asym_id` /
        `residue_index`, `x_ref` defaults to `batch["x_gt"]`; the tables are uploaded to the batch's device."""
        from .driver import ligand_atom_mask
        from .interactions import residue_labels_from_meta
        res, names, z, _ = names_from_meta(infer_meta_data)
        rid = _host(batch["atom_id_to_token_id"], np.int64).reshape(-1)
        if len(res) != rid.shape[0]:
            raise ValueError(f"ReceptorGeometry: infer_meta_data names {len(res)} atoms, the batch holds {rid.shape[0]}")
        mask = (z != 1) & ~_host(ligand_atom_mask(batch), bool).reshape(-1)
        if batch.get("a_mask") is not None:
            mask &= _host(batch["a_mask"], np.float64).reshape(-1) > 0
        per_atom = lambda key: _host(batch[key], np.int64)[rid] if key in batch else None
        dev = batch["x_gt"].device
        R = int(batch["is_ligand"].shape[0])
        kw.setdefault("device", dev if dev.type == "cuda" else None)
        kw.setdefault("residue_labels", residue_labels_from_meta(infer_meta_data, rid, R))
        return ReceptorGeometry.from_names(res, names, rid, batch["x_gt"] if x_ref is None else x_ref, mask, chain_of=per_atom("asym_id"),
                                           residue_number=per_atom("residue_index"), n_residues=R, thresholds=thresholds, **kw)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernels' tables on `device` (uploaded once)"""
        names = (*_DEVICE_KEYS, "chi_ref", "pi_periodic")
        return ops.cached_upload(self._tables, device, lambda up: {k: up(getattr(self, k)) for k in names})

    def _poses(self, x_pred, what):
        if x_pred.dim() != 3 or x_pred.shape[1] != self.n_pose_atoms or x_pred.shape[2] != 3:
            raise ValueError(f"ReceptorGeometry.{what}: the tables are over {self.n_pose_atoms} pose atoms, x_pred has shape "
                             f"{tuple(x_pred.shape)}")
        if not 1 <= x_pred.shape[0] <= MAX_POSES:
            raise ValueError(f"ReceptorGeometry.{what}: {x_pred.shape[0]} poses; the kernels take 1 .. {MAX_POSES}")
        return x_pred.float().contiguous()

    def check(self, x_pred: torch.Tensor) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> dict of device tensors: val [P,8] (min, max bond ratio; min, max 1-3 ratio; min clash ratio; max
        plane distance, A; max peptide twist, degrees; number of wrong centres), worst_pair [P,2] int32 (the pair of the min clash
        ratio, -1 without pairs), counts [P,7] int32 (failing terms per check, failing pairs for the clash), flags [P] int32 (bit mask
        in CHECK_NAMES order), valid [P] bool, residue_flags [P,R] uint8, atom_clash [P,A] uint8, term_val [P,T] and term_fail [P,T]
        uint8 (every term's value and fail bits, in the order of `term_atoms`).  Empty sets give 1, +inf, 0, no bit.  Nothing is read
        back, nothing synchronises."""
        x = self._poses(x_pred, "check")
        L_ = ops._lib.init()
        P, A, R, T = x.shape[0], self.n_pose_atoms, self.n_residues, self.n_terms
        t = self.tables(x.device)
        n_ws = L_.pd_receptor_geometry_workspace_numel(P, A)
        ops.check(min(n_ws, 0), "pd_receptor_geometry_workspace_numel")
        dev = x.device
        ws = torch.empty(n_ws, dtype=torch.int64, device=dev)
        val = torch.empty(P, 8, device=dev)
        worst = torch.empty(P, 2, dtype=torch.int32, device=dev)
        counts = torch.empty(P, 7, dtype=torch.int32, device=dev)
        flags = torch.empty(P, dtype=torch.int32, device=dev)
        rflags = torch.empty(P, R, dtype=torch.uint8, device=dev)
        aclash = torch.empty(P, A, dtype=torch.uint8, device=dev)
        tval = torch.empty(P, T, device=dev)
        tfail = torch.empty(P, T, dtype=torch.uint8, device=dev)
        ptr = lambda k: ops.ptr(t[k]) if t[k].numel() else None
        out = lambda b: ops.ptr(b) if b.numel() else None
        ops.check(L_.pd_receptor_geometry(ops.ptr(x), ptr("radius_signed"), ptr("excl_start"), ptr("excl_atom"), ptr("term_atoms"),
                                          ptr("term_ref"), *self.term_counts, ptr("res_term_start"), ptr("res_term"), ptr("res_atom_start"),
                                          ptr("res_atom"), self._thr, ops.ptr(ws), ops.ptr(val), ops.ptr(worst), ops.ptr(counts),
                                          ops.ptr(flags), out(rflags), ops.ptr(aclash), out(tval), out(tfail), P, A, R, ops.stream()),
                  "pd_receptor_geometry")
        return {"val": val, "worst_pair": worst, "counts": counts, "flags": flags, "valid": flags == 0, "residue_flags": rflags,
                "atom_clash": aclash, "term_val": tval, "term_fail": tfail}

    def dihedrals(self, x_pred: torch.Tensor) -> torch.Tensor:
        """x_pred [P,A,3] (device) -> angles [P,R,7] fp32 degrees in ANGLE_NAMES order, NaN where undefined"""
        x = self._poses(x_pred, "dihedrals")
        P, R = x.shape[0], self.n_residues
        angles = torch.empty(P, R, 7, device=x.device)
        if R:
            ops.check(ops._lib.init().pd_receptor_dihedrals(ops.ptr(x), ops.ptr(self.tables(x.device)["dih"]), ops.ptr(angles), P,
                                                            self.n_pose_atoms, R, ops.stream()), "pd_receptor_dihedrals")
        return angles

    def chi_recovery(self, x_pred: torch.Tensor, x_ref=None, tolerance: float = 40.0, residues=None) -> Dict[str, torch.Tensor]:
        """How many side-chain rotamers does a pose recover?  A chi is compared where it is defined in the pose and in the reference
        (the structure the tables were built from, or `x_ref` [A,3]); it matches when the difference, wrapped to (-180, 180] - modulo
        180 for the pi-periodic chis - is at most `tolerance` degrees.  `residues`: ids or a bool mask [R] restricting the comparison
        (the pocket).  -> matched [P], compared [P] (int64), recovered [P] (their quotient, NaN when nothing is compared), rotamer_ok
        [P,R] bool (the residue has a compared chi and all of them match).  Device tensors, no read-back."""
        ang = self.dihedrals(x_pred)[:, :, 3:7].double()
        t = self.tables(ang.device)
        if x_ref is None:
            ref = t["chi_ref"]
        else:
            xr = _host(x_ref, np.float64)
            if xr.shape != (self.n_pose_atoms, 3):
                raise ValueError(f"ReceptorGeometry.chi_recovery: x_ref has shape {tuple(xr.shape)}, the tables are over {self.n_pose_atoms} atoms")
            ref = torch.from_numpy(dihedrals_host(xr, self.dih)[:, 3:7]).to(ang.device)
        sel = torch.ones(self.n_residues, dtype=torch.bool, device=ang.device)
        if residues is not None:
            r = torch.as_tensor(residues, device=ang.device)
            sel = r.bool() if r.dtype == torch.bool else torch.zeros_like(sel).index_fill_(0, r.long().reshape(-1), True)
            if sel.shape[0] != self.n_residues:
                raise ValueError(f"ReceptorGeometry.chi_recovery: a residue mask of {sel.shape[0]} for {self.n_residues} residues")
        diff = ang - ref[None]
        period = torch.where(t["pi_periodic"], 180.0, 360.0).double()[None]
        wrapped = torch.remainder(diff + period / 2, period) - period / 2
        compared = ~torch.isnan(diff) & sel[None, :, None]
        match = compared & (wrapped.abs() <= float(tolerance))
        n_match, n_comp = match.sum((1, 2)), compared.sum((1, 2))
        return {"matched": n_match, "compared": n_comp, "recovered": n_match.double() / n_comp.double(),
                "rotamer_ok": compared.any(-1) & (match == compared).all(-1)}

    # ------------------------------------------------------------------ reading a result
    @staticmethod
    def check_names(flags_row) -> list:
        """names of the failed checks of one flags value"""
        f = int(flags_row)
        return [n for b, n in enumerate(CHECK_NAMES) if f >> b & 1]

    def describe(self, row) -> List[str]:
        """one pose's residue_flags [R] (a row of `check`'s result; read back here) -> a line per failing residue: its label and the
        names of its failed checks"""
        row = _host(row, np.int64).reshape(-1)
        if row.shape[0] != self.n_residues:
            raise ValueError(f"ReceptorGeometry.describe: a row of {row.shape[0]} for {self.n_residues} residues")
        return [f"{self.residue_labels[r]}: {', '.join(self.check_names(row[r]))}" for r in np.nonzero(row)[0]]

    def __repr__(self):
        b, a, c, p, g = self.term_counts
        return (f"ReceptorGeometry(n_pose_atoms={self.n_pose_atoms}, n_residues={self.n_residues}, active={int(self.active.sum())}, "
                f"untyped={self.untyped}, bonds={b}, angles={a}, centres={c}, peptides={p}, planar_groups={g}, "
                f"reference_clashes={len(self.reference_clashes)})")
