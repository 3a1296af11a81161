"""Where are the hydrogens, and which of them make a hydrogen bond?  The model predicts heavy atoms only; the geometry of almost
every hydrogen follows from the heavy atoms it rides on.  `Hydrogens` places every hydrogen of the ligand and the receptor for every
pose on the device, turns the rotatable polar ones (OH, SH, NH3+) towards the partner molecule, and tests hydrogen bonds with the
donor - H ... acceptor angle (kernels `pd_place_hydrogens`, `pd_hydrogen_bonds`, csrc/hydrogens.hip - its header comment holds the same
definition, tests/hydrogens_ref.py restates it in float64 numpy).

One system: the tables of `InteractionFingerprint` - `ligand_idx [L]`, `rec_mask [A]`, `residue_of [A]` / `n_residues` R, the type
bytes of `VinaScore` (the ACCEPTOR bit, and the radius class, which tells N, O and S) - and a hydrogen table of H rows, built once on
the host: `parent` (the atom a hydrogen rides on), `ref [3]` (atoms n1, n2, n3; -1 where unused), `mode` (uint8), `length` (fp32, A),
`a`, `b` (fp32, radians), `group` (rotor id or -1) and `side` (0 receptor, 1 ligand).

Modes.  p is the parent's position, u_i = (n_i - p) / |n_i - p|, unit(v) = v / |v|; all arithmetic is float64 on the fp32
coordinates and the result is rounded once to fp32:

    TRI     three heavy neighbours (methine C-H, tertiary N+-H)   H = p + length unit(-(u1 + u2 + u3))
    BISECT  two heavy neighbours                                  bis = unit(-(u1 + u2)), w = unit(u1 x u2)
                                                                  H = p + length (cos a bis + sin a w)
            a = 0 for sp2 parents (aromatic C-H, amide and ring N-H), a = +-54.7356 deg for the two H of CH2 / NH2+
    NERF    one heavy neighbour n1, and n2 bonded to n1           bc = unit(p - n1), n = unit((n1 - n2) x bc), m = n x bc
                                                                  H = p + length (-cos a bc + sin a (cos b m + sin b n))
            a is the angle n1 - p - H, b the dihedral n2 - n1 - p - H (0 cis to n2, 180 deg trans): methyl a = 109.4712 deg, b = 60,
            180, 300 deg; OH / SH a = 109.5 deg, b = 180 deg; NH3+ three at 120 deg; terminal sp2 NH2 / =CH2 a = 120 deg, b = 0, 180 deg
    LINEAR  sp, one neighbour                                     H = p + length unit(p - n1)

A hydrogen is NOT PLACED when a vector about to be normalised is shorter than 1e-6, when a coordinate it reads is not finite or when
a ref its mode needs is -1: its `x_h` is NaN, `placed` 0, and it takes part in nothing.  Default lengths (`DEFAULT_LENGTHS`): C-H
1.09, N-H 1.01, O-H 0.96, S-H 1.34 A - THIS PACKAGE'S DEFAULTS; `lengths=` overrides them.

Rotor groups (`orient=True`).  A group is the hydrogens of one OH or SH (one H, 12 candidates) or of one NH3+ (three H, 4
candidates): NERF rows that share parent, n1 and n2.  Candidate k adds k * 30 deg to every b of the group; the group's acceptors are
the acceptor-typed heavy atoms A of the OTHER molecule with |A - p| <= d_da; the score of k is the smallest |A - H| over the group's
hydrogens and those acceptors; the smallest score wins, on a tie the smallest k, with no acceptor in range k = 0.  Every rotor looks
at heavy atoms only, so there is no order dependence.  `rotor_choice [P,G]` reports k.  Methyls are never rotated.

Hydrogen bond (PLIP's published conditions, as `RingInteractions` uses PLIP's): the donor is a placed hydrogen whose parent D is N, O
or S; the acceptor A is an acceptor-typed heavy atom of the other molecule; |D - A| <= d_da (4.1 A); the angle D - H ... A is at least
angle_min (100 deg), tested as (D - H) . (A - H) <= cos(angle_min) |D - H| |A - H| on the fp32 `x_h` as stored, so the result can be
recomputed from the outputs.  `thresholds=` overrides both numbers.  Bit 0 `hbond_donor`: the ligand donates to the residue; bit 1
`hbond_acceptor`: the ligand accepts from it (`HBOND_KIND_NAMES`).

`place(x_pred)` returns `x_h` fp32 [P,H,3], `placed` uint8 [P,H], `rotor_choice` int32 [P,G] and `x_all` [P,A+H,3] (the pose with the
hydrogens appended; a hydrogen that is not placed is NaN there too); `hbonds(x_pred)` adds `bits` uint8 [P,R], `ligand_bits` uint8
[P,L], `h_bits` uint8 [P,H] and `counts` int32 [P,2] (the (H, acceptor) pairs per kind).  `InteractionFingerprint` keeps its
distance-only `hbond_*` bits; these are a separate result.  `compare`, `pairwise`, `satisfies`, `required_row` and `describe` are
those of the other fingerprints; `pdb_template` makes `pdbio.PdbTemplate` write protonated poses; `driver.redock(..., hydrogens=)`
reports the kept poses'.

**Caveats.**  The charge states are fixed - LYS NH3+, ARG charged, ASP / GLU deprotonated, HIS neutral with the H on ND1, as
`receptor_charges_from_names` assumes - and there is no pKa model.  Lengths and thresholds are defaults that have not been validated
on real complexes.  HIS tautomers are not chosen.  There are no terminal NH3+ / COO-.  Hydrogens are placed on C, N, O and S only.
Out of scope: water, flipping ASN / GLN / HIS, and feeding the hydrogens into `VinaScore`, `BuriedSurface` or `PoseValidity` - those
are follow-ups behind their own keywords.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .interactions import MAX_POSES, InteractionFingerprint, _ByteRows, _mask_of, residue_labels_from_meta
from .scoring import (_STANDARD, _SYMBOL_Z, ACCEPTOR, _atomic_numbers, _bond_list, _host, _hydrogen_counts, names_from_meta,
                      receptor_types_from_names)

__all__ = ["Hydrogens", "HBOND_KIND_NAMES", "HBOND_THRESHOLD_NAMES", "DEFAULT_HBOND_THRESHOLDS", "DEFAULT_LENGTHS", "MODE_NAMES", "TRI",
           "BISECT", "NERF", "LINEAR", "hbond_kind_mask", "ligand_hydrogens_from_bonds", "receptor_hydrogens_from_names",
           "join_hydrogen_tables", "MAX_HYDROGENS"]

#: the two kinds in bit order
HBOND_KIND_NAMES = ("hbond_donor", "hbond_acceptor")
#: the two thresholds - the donor - acceptor distance (A) and the smallest D - H ... A angle (degrees) - and PLIP's defaults
HBOND_THRESHOLD_NAMES = ("d_da", "angle_min")
DEFAULT_HBOND_THRESHOLDS = {"d_da": 4.1, "angle_min": 100.0}
#: X - H bond lengths (A) by the parent's atomic number: this package's defaults
DEFAULT_LENGTHS = {6: 1.09, 7: 1.01, 8: 0.96, 16: 1.34}
#: the placement modes, in the order of their codes
MODE_NAMES = ("TRI", "BISECT", "NERF", "LINEAR")
TRI, BISECT, NERF, LINEAR = 0, 1, 2, 3
#: limit of the kernels (csrc/hydrogens.hip) beyond those of `interactions`
MAX_HYDROGENS = 65535

TETRAHEDRAL = math.acos(-1.0 / 3.0)                                  # 109.4712 deg
HALF_TETRAHEDRAL = TETRAHEDRAL / 2.0                                  # 54.7356 deg
_HYDROXYL, _TRIGONAL = math.radians(109.5), math.radians(120.0)
_DEG = math.pi / 180.0
_STAGGERED = (60.0 * _DEG, 180.0 * _DEG, 300.0 * _DEG, 0.0)
_POLAR_CLASSES = (1, 2, 4)                                            # the radius classes of N, O and S in a type byte (scoring.RADII)
_TABLE_KEYS = ("parent", "ref", "mode", "length", "a", "b", "group")

# the side chains of the 20 standard residues: (kind, parent, n1, n2[, n3]) - tri: TRI; ch2: two BISECT at +-54.7356 deg; ar: BISECT in
# the plane; me: a methyl; oh: a hydroxyl or thiol (a rotor); nh3: an ammonium (a rotor); nh2: a planar NH2, cis and trans to n2
_AROMATIC_6 = [("ar", "CD1", "CG", "CE1"), ("ar", "CD2", "CG", "CE2"), ("ar", "CE1", "CD1", "CZ"), ("ar", "CE2", "CD2", "CZ")]
_SIDE_CHAINS = {
    "GLY": [], "ALA": [("me", "CB", "CA", "N")],
    "SER": [("ch2", "CB", "CA", "OG"), ("oh", "OG", "CB", "CA")],
    "CYS": [("ch2", "CB", "CA", "SG"), ("oh", "SG", "CB", "CA")],
    "VAL": [("tri", "CB", "CA", "CG1", "CG2"), ("me", "CG1", "CB", "CA"), ("me", "CG2", "CB", "CA")],
    "THR": [("tri", "CB", "CA", "OG1", "CG2"), ("oh", "OG1", "CB", "CA"), ("me", "CG2", "CB", "CA")],
    "LEU": [("ch2", "CB", "CA", "CG"), ("tri", "CG", "CB", "CD1", "CD2"), ("me", "CD1", "CG", "CB"), ("me", "CD2", "CG", "CB")],
    "ILE": [("tri", "CB", "CA", "CG1", "CG2"), ("ch2", "CG1", "CB", "CD1"), ("me", "CG2", "CB", "CA"), ("me", "CD1", "CG1", "CB")],
    "MET": [("ch2", "CB", "CA", "CG"), ("ch2", "CG", "CB", "SD"), ("me", "CE", "SD", "CG")],
    "PRO": [("ch2", "CB", "CA", "CG"), ("ch2", "CG", "CB", "CD"), ("ch2", "CD", "CG", "N")],
    "PHE": [("ch2", "CB", "CA", "CG")] + _AROMATIC_6 + [("ar", "CZ", "CE1", "CE2")],
    "TYR": [("ch2", "CB", "CA", "CG")] + _AROMATIC_6 + [("oh", "OH", "CZ", "CE1")],
    "TRP": [("ch2", "CB", "CA", "CG"), ("ar", "CD1", "CG", "NE1"), ("ar", "NE1", "CD1", "CE2"), ("ar", "CE3", "CD2", "CZ3"),
            ("ar", "CZ2", "CE2", "CH2"), ("ar", "CZ3", "CE3", "CH2"), ("ar", "CH2", "CZ2", "CZ3")],
    "ASP": [("ch2", "CB", "CA", "CG")], "GLU": [("ch2", "CB", "CA", "CG"), ("ch2", "CG", "CB", "CD")],
    "ASN": [("ch2", "CB", "CA", "CG"), ("nh2", "ND2", "CG", "OD1")],
    "GLN": [("ch2", "CB", "CA", "CG"), ("ch2", "CG", "CB", "CD"), ("nh2", "NE2", "CD", "OE1")],
    "HIS": [("ch2", "CB", "CA", "CG"), ("ar", "ND1", "CG", "CE1"), ("ar", "CD2", "CG", "NE2"), ("ar", "CE1", "ND1", "NE2")],
    "LYS": [("ch2", "CB", "CA", "CG"), ("ch2", "CG", "CB", "CD"), ("ch2", "CD", "CG", "CE"), ("ch2", "CE", "CD", "NZ"),
            ("nh3", "NZ", "CE", "CD")],
    "ARG": [("ch2", "CB", "CA", "CG"), ("ch2", "CG", "CB", "CD"), ("ch2", "CD", "CG", "NE"), ("ar", "NE", "CD", "CZ"),
            ("nh2", "NH1", "CZ", "NE"), ("nh2", "NH2", "CZ", "NE")],
}
assert set(_SIDE_CHAINS) == set(_STANDARD)


def hbond_kind_mask(kinds: Optional[Iterable[str]] = None) -> int:
    """the byte mask of a sequence of hydrogen-bond kind names (default: both)"""
    return _mask_of(kinds, HBOND_KIND_NAMES)


def _lengths(lengths) -> Dict[int, float]:
    out = dict(DEFAULT_LENGTHS)
    for k, v in (lengths or {}).items():
        z = _SYMBOL_Z.get(k.strip().upper(), 0) if isinstance(k, str) else int(k)
        if z not in DEFAULT_LENGTHS or not math.isfinite(float(v)) or not float(v) > 0:
            raise ValueError(f"Hydrogens: lengths are positive values for C, N, O or S, got {k!r}: {v!r}")
        out[z] = float(v)
    return out


class _Rows:
    """a hydrogen table under construction"""

    def __init__(self):
        self.rows: List[tuple] = []
        self.n_groups = 0

    def add(self, parent, refs, mode, length, a=0.0, b=0.0, group=-1):
        refs = (list(refs) + [-1, -1, -1])[:3]
        self.rows.append((int(parent), tuple(int(r) for r in refs), int(mode), float(length), float(a), float(b), int(group)))

    def nerf(self, parent, n1, n2, length, a, bs, rotor=False):
        group = -1
        if rotor and n1 >= 0 and n2 >= 0:
            group, self.n_groups = self.n_groups, self.n_groups + 1
        for b in bs:
            self.add(parent, (n1, n2), NERF, length, a, b, group)

    def table(self) -> Dict[str, np.ndarray]:
        cols = list(zip(*self.rows)) if self.rows else [[], [], [], [], [], [], []]
        return {"parent": np.asarray(cols[0], dtype=np.int32), "ref": np.asarray(cols[1], dtype=np.int32).reshape(-1, 3),
                "mode": np.asarray(cols[2], dtype=np.uint8), "length": np.asarray(cols[3], dtype=np.float32),
                "a": np.asarray(cols[4], dtype=np.float32), "b": np.asarray(cols[5], dtype=np.float32),
                "group": np.asarray(cols[6], dtype=np.int32)}


def join_hydrogen_tables(*tables) -> Dict[str, np.ndarray]:
    """several hydrogen tables over the same atom numbering as one: the rows in order, the rotor ids of each moved behind the last"""
    out = {k: [] for k in _TABLE_KEYS}
    n_groups = 0
    for t in tables:
        group = np.asarray(t["group"], dtype=np.int32).reshape(-1).copy()
        group[group >= 0] += n_groups
        n_groups = max(n_groups, int(group.max()) + 1) if len(group) else n_groups
        for k in _TABLE_KEYS:
            out[k].append(group if k == "group" else np.asarray(t[k]))
    cat = lambda k, dt, tail: np.concatenate([np.asarray(a, dtype=dt).reshape((-1,) + tail) for a in out[k]]) if out[k] else np.zeros((0,) + tail, dt)
    return {"parent": cat("parent", np.int32, ()), "ref": cat("ref", np.int32, (3,)), "mode": cat("mode", np.uint8, ()),
            "length": cat("length", np.float32, ()), "a": cat("a", np.float32, ()), "b": cat("b", np.float32, ()),
            "group": cat("group", np.int32, ())}


def ligand_hydrogens_from_bonds(elements, bonds: Iterable[Tuple[int, int]], bond_orders: Optional[Sequence[float]] = None,
                                n_hydrogens=None, formal_charges=None, lengths=None) -> Dict[str, np.ndarray]:
    """The hydrogen table of a ligand from its bond graph, in indices into `elements`.  The hydrogen count per atom is the one
    `scoring.ligand_types_from_bonds` uses (`n_hydrogens` when given, else the default valences), less the hydrogens that are atoms
    already; C, N, O and S carry them.  The mode comes from the heavy neighbours and the hybridisation - a bond order of 1.5 or 2 on
    the parent gives sp2, 3 gives sp; an N with single bonds only that is bonded to an sp2 atom (amide, amidine, guanidine, aniline)
    is planar:
      three heavy neighbours   TRI
      two                      BISECT: one H in the plane (sp2; an sp3 parent with one H gets a = +54.7356 deg), two H at +-54.7356 deg
      one, n1                  sp: LINEAR; else NERF with n2 = the lowest other heavy neighbour of n1 - planar parents a = 120 deg, b =
                               0, 180 deg (one H: 180 deg); OH / SH a = 109.5 deg, b = 180 deg, a rotor; other sp3 parents a = 109.4712
                               deg, b = 60, 180, 300 deg (two H: 60, 300; one: 180) - three H on an N are a rotor
    A molecule too small to supply n1 or n2 gets ref = -1 there: the row stands, the hydrogen is not placed, and it joins no rotor."""
    z = _atomic_numbers(elements)
    n = len(z)
    bonds, orders = _bond_list(n, bonds, bond_orders, "ligand_hydrogens_from_bonds")
    charge = np.zeros(n, dtype=np.int64) if formal_charges is None else _host(formal_charges, np.int64).reshape(-1)
    if charge.shape[0] != n or (n_hydrogens is not None and len(n_hydrogens) != n):
        raise ValueError(f"ligand_hydrogens_from_bonds: {n} elements, but formal_charges / n_hydrogens of another length")
    n_h, h_nb, _, _ = _hydrogen_counts(z, bonds, orders, n_hydrogens, charge)
    length_of = _lengths(lengths)
    heavy: List[List[int]] = [[] for _ in range(n)]
    top = [1.0] * n
    for (i, j), o in zip(bonds, orders):
        top[i], top[j] = max(top[i], o), max(top[j], o)
        if z[j] != 1:
            heavy[i].append(j)
        if z[i] != 1:
            heavy[j].append(i)
    heavy = [sorted(set(h)) for h in heavy]
    sp2 = [t in (1.5, 2.0) for t in top]
    planar = [sp2[a] or (z[a] == 7 and top[a] == 1.0 and any(sp2[q] for q in heavy[a])) for a in range(n)]
    rows = _Rows()
    for p in range(n):
        n_place = int(n_h[p]) - int(h_nb[p])
        if int(z[p]) not in length_of or n_place <= 0 or len(heavy[p]) > 3:
            continue
        hv, length = heavy[p], length_of[int(z[p])]
        if len(hv) == 3:
            rows.add(p, hv, TRI, length)
        elif len(hv) == 2:
            for a in ((HALF_TETRAHEDRAL, -HALF_TETRAHEDRAL) if n_place >= 2 else (0.0 if planar[p] else HALF_TETRAHEDRAL,)):
                rows.add(p, hv, BISECT, length, a)
        else:
            n1 = hv[0] if hv else -1
            n2 = next((q for q in heavy[n1] if q != p), -1) if n1 >= 0 else -1
            if n1 >= 0 and top[p] >= 3.0:
                rows.add(p, (n1,), LINEAR, length)
            elif planar[p]:
                rows.nerf(p, n1, n2, length, _TRIGONAL, (0.0, math.pi) if n_place >= 2 else (math.pi,))
            elif z[p] in (8, 16) and n_place == 1:
                rows.nerf(p, n1, n2, length, _HYDROXYL, (math.pi,), rotor=True)
            else:
                bs = {1: (math.pi,), 2: (_STAGGERED[0], _STAGGERED[2])}.get(n_place, _STAGGERED[:n_place])
                rows.nerf(p, n1, n2, length, TETRAHEDRAL, bs, rotor=z[p] == 7 and n_place == 3)
    return rows.table()


def receptor_hydrogens_from_names(res_names: Sequence[str], atom_names: Sequence[str], residue_of, mask=None, chain_of=None,
                                  residue_number=None, lengths=None) -> Dict[str, np.ndarray]:
    """The hydrogen table of a receptor by residue and atom names, in indices into the arguments: a table of the 20 standard residues
    in the charge states `receptor_charges_from_names` assumes - LYS NH3+, ARG charged, ASP / GLU deprotonated, HIS neutral with the H
    on ND1.  Atoms with equal `residue_of` form a residue; `mask` [n] (default: all): 0 = the atom does not exist.  The backbone amide
    H is a BISECT row on N with refs CA and the C of the PREVIOUS residue: the residue with the id one lower, in the same chain when
    `chain_of` [n] is given and numbered one lower when `residue_number` [n] is.  When that C is absent (first residue, chain break,
    crop edge) the amide H is left out - there is no NH3+ terminus; PRO has none.  A hydrogen whose ref atom is missing is left out;
    an unknown residue gets none.  Hydrogens in chain: GLY 3, ALA 5, SER 5, CYS 5, VAL 9, THR 7, LEU 11, ILE 11, MET 9, PRO 7, PHE 9, TYR
    9, TRP 10, ASP 4, GLU 6, ASN 6, GLN 8, HIS 7, LYS 13, ARG 13."""
    res = _host(residue_of, np.int64).reshape(-1)
    n = res.shape[0]
    if not len(res_names) == len(atom_names) == n:
        raise ValueError(f"receptor_hydrogens_from_names: {len(res_names)} residue names, {len(atom_names)} atom names, {n} residue ids")
    ok = np.ones(n, dtype=bool) if mask is None else _host(mask, np.float64).reshape(-1) > 0
    chain = None if chain_of is None else _host(chain_of, np.int64).reshape(-1)
    number = None if residue_number is None else _host(residue_number, np.int64).reshape(-1)
    if ok.shape[0] != n or (chain is not None and chain.shape[0] != n) or (number is not None and number.shape[0] != n):
        raise ValueError(f"receptor_hydrogens_from_names: {n} atoms, but a mask, chain_of or residue_number of another length")
    length_of = _lengths(lengths)
    by_residue: Dict[int, Dict[str, int]] = {}
    kind: Dict[int, str] = {}
    for a in range(n):
        r = str(res_names[a]).strip().upper()
        if ok[a]:
            by_residue.setdefault(int(res[a]), {}).setdefault(str(atom_names[a]).strip().upper(), a)
            kind.setdefault(int(res[a]), r)
    rows = _Rows()
    for s in sorted(by_residue):
        name, atoms = kind[s], by_residue[s]
        if name not in _SIDE_CHAINS:
            continue
        entries = []
        prev = by_residue.get(s - 1, {})
        if name != "PRO" and "N" in atoms and "C" in prev:
            same_chain = chain is None or chain[prev["C"]] == chain[atoms["N"]]
            in_sequence = number is None or number[prev["C"]] + 1 == number[atoms["N"]]
            if same_chain and in_sequence:
                atoms = dict(atoms, **{"-C": prev["C"]})
                entries.append(("ar", "N", "CA", "-C"))
        entries.append(("ch2", "CA", "N", "C") if name == "GLY" else ("tri", "CA", "N", "C", "CB"))
        for what, parent, *refs in entries + _SIDE_CHAINS[name]:
            if parent not in atoms or any(r not in atoms for r in refs):
                continue
            p, r = atoms[parent], [atoms[q] for q in refs]
            length = length_of[_SYMBOL_Z[parent[0]]]
            if what == "tri":
                rows.add(p, r, TRI, length)
            elif what == "ch2":
                rows.add(p, r, BISECT, length, HALF_TETRAHEDRAL)
                rows.add(p, r, BISECT, length, -HALF_TETRAHEDRAL)
            elif what == "ar":
                rows.add(p, r, BISECT, length, 0.0)
            elif what == "me":
                rows.nerf(p, r[0], r[1], length, TETRAHEDRAL, _STAGGERED[:3])
            elif what == "oh":
                rows.nerf(p, r[0], r[1], length, _HYDROXYL, (math.pi,), rotor=True)
            elif what == "nh3":
                rows.nerf(p, r[0], r[1], length, TETRAHEDRAL, _STAGGERED[:3], rotor=True)
            else:
                rows.nerf(p, r[0], r[1], length, _TRIGONAL, (0.0, math.pi))
    return rows.table()


def _hbond_thresholds(thresholds) -> Tuple[float, float]:
    t = dict(DEFAULT_HBOND_THRESHOLDS)
    if thresholds is None:
        pass
    elif isinstance(thresholds, dict):
        bad = set(thresholds) - set(HBOND_THRESHOLD_NAMES)
        if bad:
            raise ValueError(f"Hydrogens: unknown thresholds {sorted(bad)}; they are {HBOND_THRESHOLD_NAMES}")
        t.update(thresholds)
    else:
        vals = list(thresholds)
        if len(vals) != len(HBOND_THRESHOLD_NAMES):
            raise ValueError(f"Hydrogens: thresholds are {HBOND_THRESHOLD_NAMES}, got {len(vals)} values")
        t = dict(zip(HBOND_THRESHOLD_NAMES, vals))
    d_da, angle = float(t["d_da"]), float(t["angle_min"])
    if not math.isfinite(d_da) or d_da < 0:
        raise ValueError(f"Hydrogens: d_da must be finite and not negative, got {d_da}")
    if not 0.0 <= angle <= 180.0:
        raise ValueError(f"Hydrogens: angle_min must lie in 0 .. 180 degrees, got {angle}")
    return d_da, angle


class Hydrogens(_ByteRows):
    """One system's tables for `pd_place_hydrogens` and `pd_hydrogen_bonds`: host copies (numpy: `types` uint8 [A], `ligand_idx` int32
    [L], `lig_active` uint8 [L], `rec_mask` uint8 [A], `residue_of` int32 [A]; the hydrogen table `parent` int32 [H], `ref` int32
    [H,3], `mode` uint8 [H], `length`, `a`, `b` fp32 [H], `group` int32 [H] (dense rotor ids, -1: none), `side` uint8 [H]; derived from
    them `group_h` int32 [G,3], `acc` int32 [NA_r + NA_l] (the receptor's acceptors sorted by residue, then the ligand's) with
    `racc_start` int32 [R + 1] and `lig_acc_slot` int32 [L], `polar` int32 [HP_l + HP_r] (the rows on N, O or S: the ligand's, then
    the receptor's sorted by residue) with `rh_start` int32 [R + 1] and `polar_slot` int32 [H]), `thresholds` (dict: A and degrees),
    `receptor_typing` ("given", "names" or "elements" - with the last the receptor has no hydrogens and no acceptors, so only the
    ligand's hydrogens are placed and no bond is found), `residue_labels` and, uploaded once per device, what the kernels read.
    `n_atoms` is L, `n_pose_atoms` A, `n_residues` R, `n_hydrogens` H, `n_groups` G."""
    _name = "Hydrogens"
    _kind_names = HBOND_KIND_NAMES

    def __init__(self, types, ligand_idx, lig_active, rec_mask, residue_of, n_residues, table, thresholds=None,
                 receptor_typing: str = "given", residue_labels=None, device=None):
        self.types, self.ligand_idx, self.lig_active = types, ligand_idx, lig_active
        self.rec_mask, self.residue_of, self.n_residues = rec_mask, residue_of, int(n_residues)
        A, L, R = int(types.shape[0]), int(ligand_idx.shape[0]), self.n_residues
        self.n_atoms, self.n_pose_atoms = L, A
        self.parent = np.ascontiguousarray(table["parent"], dtype=np.int32).reshape(-1)
        H = self.n_hydrogens = int(self.parent.shape[0])
        self.ref = np.ascontiguousarray(table["ref"], dtype=np.int32).reshape(-1, 3)
        self.mode = np.ascontiguousarray(table["mode"], dtype=np.uint8).reshape(-1)
        self.length, self.a, self.b = (np.ascontiguousarray(table[k], dtype=np.float32).reshape(-1) for k in ("length", "a", "b"))
        group = np.asarray(table["group"], dtype=np.int64).reshape(-1)
        if not 1 <= H <= MAX_HYDROGENS:
            raise ValueError(f"Hydrogens: {H} hydrogens; the kernels take 1 .. {MAX_HYDROGENS}")
        if any(len(v) != H for v in (self.ref, self.mode, self.length, self.a, self.b, group)):
            raise ValueError(f"Hydrogens: the hydrogen table has {H} parents, but a column of another length")
        local = np.full(A, -1, dtype=np.int64)
        local[ligand_idx] = np.arange(L)
        on_ligand = (local[np.clip(self.parent, 0, A - 1)] >= 0) & (lig_active[np.clip(local[np.clip(self.parent, 0, A - 1)], 0, L - 1)] > 0)
        if self.parent.min() < 0 or self.parent.max() >= A or not (on_ligand | (rec_mask[self.parent] > 0)).all():
            raise ValueError("Hydrogens: a hydrogen rides on an existing heavy atom of the ligand or of the receptor")
        if self.ref.min() < -1 or self.ref.max() >= A or (self.ref == self.parent[:, None]).any():
            raise ValueError(f"Hydrogens: a ref is -1 or an atom index below {A} other than the parent")
        if self.mode.max() > LINEAR:
            raise ValueError(f"Hydrogens: the modes are {dict(zip(MODE_NAMES, range(4)))}")
        if not (np.isfinite(self.length).all() and (self.length > 0).all() and np.isfinite(self.a).all() and np.isfinite(self.b).all()):
            raise ValueError("Hydrogens: lengths must be finite and positive, angles finite")
        self.side = on_ligand.astype(np.uint8)
        # rotor groups: dense ids in the order of first appearance
        ids = {}
        for g in group[group >= 0].tolist():
            ids.setdefault(g, len(ids))
        self.group = np.asarray([ids[g] if g >= 0 else -1 for g in group.tolist()], dtype=np.int32)
        G = self.n_groups = len(ids)
        self.group_h = np.full((G, 3), -1, dtype=np.int32)
        for g in range(G):
            rows = np.nonzero(self.group == g)[0]
            same = lambda v: len({tuple(np.atleast_1d(u).tolist()) for u in v}) == 1
            if len(rows) not in (1, 3):
                raise ValueError(f"Hydrogens: a rotor group has 1 or 3 hydrogens, group {g} has {len(rows)}")
            if not ((self.mode[rows] == NERF).all() and same(self.parent[rows]) and same(self.ref[rows, :2])):
                raise ValueError(f"Hydrogens: all hydrogens of a rotor group are NERF rows that share parent, n1 and n2 (group {g})")
            self.group_h[g, :len(rows)] = rows
        # acceptors: the receptor's sorted by residue, then the ligand's
        order = np.argsort(residue_of, kind="stable")
        racc = order[(rec_mask[order] > 0) & ((types[order] & ACCEPTOR) > 0)]
        lacc_local = np.nonzero((lig_active > 0) & ((types[ligand_idx] & ACCEPTOR) > 0))[0]
        self.acc = np.concatenate([racc, ligand_idx[lacc_local]]).astype(np.int32)
        self.n_receptor_acceptors, self.n_ligand_acceptors = int(len(racc)), int(len(lacc_local))
        self.racc_start = np.concatenate([[0], np.cumsum(np.bincount(residue_of[racc], minlength=R))]).astype(np.int32)
        self.lig_acc_slot = np.full(L, -1, dtype=np.int32)
        self.lig_acc_slot[lacc_local] = np.arange(len(lacc_local))
        # polar rows: the ligand's, then the receptor's sorted by the residue of the parent
        is_polar = np.isin(types[self.parent] & 15, _POLAR_CLASSES)
        lig_rows = np.nonzero(is_polar & (self.side == 1))[0]
        rec_rows = np.nonzero(is_polar & (self.side == 0))[0]
        rec_rows = rec_rows[np.argsort(residue_of[self.parent[rec_rows]], kind="stable")]
        self.polar = np.concatenate([lig_rows, rec_rows]).astype(np.int32)
        self.n_ligand_polar, self.n_receptor_polar = int(len(lig_rows)), int(len(rec_rows))
        self.rh_start = np.concatenate([[0], np.cumsum(np.bincount(residue_of[self.parent[rec_rows]], minlength=R))]).astype(np.int32)
        self.polar_slot = np.full(H, -1, dtype=np.int32)
        self.polar_slot[self.polar] = np.arange(len(self.polar))
        self.threshold_values = _hbond_thresholds(thresholds)
        self.thresholds = dict(zip(HBOND_THRESHOLD_NAMES, self.threshold_values))
        self.receptor_typing = receptor_typing
        self.residue_labels = None if residue_labels is None else [str(s) for s in residue_labels]
        if self.residue_labels is not None and len(self.residue_labels) != R:
            raise ValueError(f"Hydrogens: {len(self.residue_labels)} residue labels for {R} residues")
        # what the kernel takes: the distance as it is, the angle as a cosine, converted in double
        self._thr = (C.c_double * 2)(self.threshold_values[0], math.cos(math.radians(self.threshold_values[1])))
        self._tables = {}
        if device is not None:
            self.tables(device)

    @property
    def table(self) -> Dict[str, np.ndarray]:
        """the hydrogen table (host copies; `parent` and `ref` are pose atoms)"""
        return {k: getattr(self, k) for k in _TABLE_KEYS + ("side",)}

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_tables(types, ligand_idx, receptor_mask, residue_of, hydrogens, n_residues: Optional[int] = None, a_mask=None,
                    ligand_active=None, thresholds=None, residue_labels=None, receptor_typing: str = "given", device=None):
        """Everything is given.  types, ligand_idx, receptor_mask, residue_of, n_residues, a_mask, ligand_active, residue_labels: as
        `InteractionFingerprint.from_types` takes them (ACCEPTOR and the radius class of a type byte are looked at).  hydrogens: the
        hydrogen table, a dict of `parent` [H], `ref` [H,3], `mode` [H], `length` [H] (A), `a`, `b` [H] (radians) and `group` [H]
        (any ids, -1: no rotor) with `parent` and `ref` in pose atoms (`join_hydrogen_tables` makes one of several).  thresholds: a
        dict over `HBOND_THRESHOLD_NAMES` (a missing one keeps its default) or the two values, A and degrees."""
        base = InteractionFingerprint.from_types(types, np.zeros(len(_host(types, np.int64).reshape(-1)), dtype=np.uint8), ligand_idx,
                                                 receptor_mask, residue_of, n_residues=n_residues, a_mask=a_mask, ligand_active=ligand_active)
        missing = [k for k in _TABLE_KEYS if k not in hydrogens]
        if missing:
            raise ValueError(f"Hydrogens: the hydrogen table lacks {missing}; it holds {_TABLE_KEYS}")
        return Hydrogens(base.types, base.ligand_idx, base.lig_active, base.rec_mask, base.residue_of, base.n_residues, hydrogens, thresholds,
                         receptor_typing, residue_labels, device)

    @staticmethod
    def from_bonds(elements, bonds, ligand_idx, residue_of, bond_orders=None, receptor_types=None, receptor_hydrogens=None,
                   n_residues: Optional[int] = None, a_mask=None, n_hydrogens=None, formal_charges=None, lengths=None, thresholds=None,
                   residue_labels=None, receptor_typing: Optional[str] = None, device=None):
        """elements, bonds (pairs of LOCAL ligand indices), ligand_idx, residue_of, bond_orders, receptor_types and the other keywords:
        as `InteractionFingerprint.from_bonds` takes them - the ligand's types are made the same way, its hydrogens by
        `ligand_hydrogens_from_bonds` (`lengths=` overrides the X - H lengths).  receptor_hydrogens: the receptor's hydrogen table in
        pose atoms (e.g. `receptor_hydrogens_from_names`), default none.  Without `receptor_types` the receptor is typed by element
        alone (`receptor_typing` "elements"): no acceptors."""
        base = InteractionFingerprint.from_bonds(elements, bonds, ligand_idx, residue_of, bond_orders=bond_orders, receptor_types=receptor_types,
                                                 n_residues=n_residues, a_mask=a_mask, n_hydrogens=n_hydrogens,
                                                 formal_charges=formal_charges, receptor_typing=receptor_typing)
        z = _atomic_numbers(elements)
        lig = base.ligand_idx
        t = ligand_hydrogens_from_bonds(z[lig], bonds, bond_orders, n_hydrogens, formal_charges, lengths)
        keep = base.lig_active[t["parent"]] > 0                       # a hydrogen on an atom that does not exist is dropped
        t = {k: v[keep] for k, v in t.items()}
        exists = np.concatenate([base.lig_active > 0, [False]])       # a ref that does not exist is -1 (the last entry serves -1)
        t["ref"] = np.where(exists[t["ref"]], lig[np.clip(t["ref"], 0, None)], -1).astype(np.int32)
        t["parent"] = lig[t["parent"]]
        tables = [t] if receptor_hydrogens is None else [receptor_hydrogens, t]
        return Hydrogens.from_tables(base.types, lig, base.rec_mask, base.residue_of, join_hydrogen_tables(*tables),
                                     n_residues=base.n_residues, ligand_active=base.lig_active, thresholds=thresholds,
                                     residue_labels=residue_labels, receptor_typing=base.receptor_typing, device=device)

    @staticmethod
    def from_batch(batch, bonds, bond_orders=None, infer_meta_data=None, thresholds=None, receptor_types=None, receptor_hydrogens=None,
                   **kw):
        """from a feature dict, as `InteractionFingerprint.from_batch`: a residue is a token, the tables are uploaded to the batch's
        device.  With `infer_meta_data` (the loader's naming tables) the receptor's types, hydrogens
        (`receptor_hydrogens_from_names`, chains and residue numbers from the batch's `asym_id` / `residue_index`) and residue labels
        come from the names; without it, and without `receptor_types` / `receptor_hydrogens`, the receptor has no hydrogens and no
        acceptors - `receptor_typing` "elements" records that.  Other keywords as for `from_bonds`."""
        from .driver import ligand_atom_mask
        lig = torch.nonzero(ligand_atom_mask(batch)).flatten()
        elements = batch["ref_feat"][:, 4:132].argmax(-1) + 1
        dev = batch["ref_feat"].device
        residue_of = batch["atom_id_to_token_id"].long()
        kw.setdefault("a_mask", batch.get("a_mask"))
        kw.setdefault("device", dev if dev.type == "cuda" else None)
        kw.setdefault("n_residues", int(batch["is_ligand"].shape[0]))
        if infer_meta_data is not None:
            res, names, z, _ = names_from_meta(infer_meta_data)
            if len(res) != int(elements.shape[0]):
                raise ValueError(f"Hydrogens: infer_meta_data names {len(res)} atoms, the batch holds {int(elements.shape[0])}")
            if receptor_types is None:
                receptor_types = receptor_types_from_names(res, names, z)
                kw.setdefault("receptor_typing", "names")
            if receptor_hydrogens is None:
                mask = (z != 1) & (np.ones(len(z), dtype=bool) if kw["a_mask"] is None else _host(kw["a_mask"], np.float64).reshape(-1) > 0)
                mask &= _host(elements, np.int64) != 1                # a parent or a ref is a receptor atom of `rec_mask`
                mask[_host(lig, np.int64)] = False
                rid = _host(residue_of, np.int64)
                per_atom = lambda key: _host(batch[key], np.int64)[rid] if key in batch else None
                receptor_hydrogens = receptor_hydrogens_from_names(res, names, rid, mask, chain_of=per_atom("asym_id"),
                                                                   residue_number=per_atom("residue_index"), lengths=kw.get("lengths"))
            kw.setdefault("residue_labels", residue_labels_from_meta(infer_meta_data, _host(residue_of, np.int64), kw["n_residues"]))
        return Hydrogens.from_bonds(elements, bonds, lig, residue_of, bond_orders=bond_orders, receptor_types=receptor_types,
                                    receptor_hydrogens=receptor_hydrogens, thresholds=thresholds, **kw)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernels' tables on `device` (uploaded once)"""
        names = ("parent", "ref", "mode", "length", "a", "b", "side", "group_h", "acc", "racc_start", "lig_acc_slot", "polar", "rh_start",
                 "polar_slot", "ligand_idx")
        return ops.cached_upload(self._tables, device, lambda up: {k: up(getattr(self, k)) for k in names})

    def _poses(self, x_pred, what):
        if x_pred.dim() != 3 or x_pred.shape[1] != self.n_pose_atoms or x_pred.shape[2] != 3:
            raise ValueError(f"Hydrogens.{what}: the tables are over {self.n_pose_atoms} pose atoms, x_pred has shape {tuple(x_pred.shape)}")
        if not 1 <= x_pred.shape[0] <= MAX_POSES:
            raise ValueError(f"Hydrogens.{what}: {x_pred.shape[0]} poses; the kernels take 1 .. {MAX_POSES}")
        return x_pred.float().contiguous()

    def place(self, x_pred: torch.Tensor, orient: bool = True) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> dict of device tensors: x_h fp32 [P,H,3] (NaN for a hydrogen that is not placed), placed uint8
        [P,H], rotor_choice int32 [P,G] (the candidate k of every rotor group; all 0 with `orient=False`, which keeps the default
        angles) and x_all fp32 [P,A+H,3]: x_pred with the hydrogens appended.  Nothing is read back, nothing synchronises."""
        x = self._poses(x_pred, "place")
        L_ = ops._lib.init()
        P, A, H, G = x.shape[0], x.shape[1], self.n_hydrogens, self.n_groups
        t = self.tables(x.device)
        x_all = torch.empty((P, A + H, 3), dtype=torch.float32, device=x.device)
        x_all[:, :A] = x
        x_h = torch.empty((P, H, 3), dtype=torch.float32, device=x.device)
        placed = torch.empty((P, H), dtype=torch.uint8, device=x.device)
        choice = torch.empty((P, G), dtype=torch.int32, device=x.device)
        opt = lambda tensor, n: ops.ptr(tensor) if n else None
        NAr, NAl = self.n_receptor_acceptors, self.n_ligand_acceptors
        ops.check(L_.pd_place_hydrogens(ops.ptr(x), ops.ptr(t["parent"]), ops.ptr(t["ref"]), ops.ptr(t["mode"]), ops.ptr(t["length"]),
                                        ops.ptr(t["a"]), ops.ptr(t["b"]), ops.ptr(t["side"]), opt(t["group_h"], G), G, opt(t["acc"], NAr + NAl),
                                        NAr, NAl, self.threshold_values[0], int(bool(orient)), ops.ptr(x_h), ops.ptr(placed), opt(choice, G),
                                        P, A, H, ops.stream()), "pd_place_hydrogens")
        x_all[:, A:] = x_h
        return {"x_h": x_h, "placed": placed, "rotor_choice": choice, "x_all": x_all}

    def hbonds(self, x_pred: torch.Tensor, placed: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) and, optionally, what `place` returned for it (else `place` runs) -> dict of device tensors: bits
        uint8 [P,R] (bit 0 hbond_donor: the ligand donates to the residue, bit 1 hbond_acceptor), ligand_bits uint8 [P,L], h_bits
        uint8 [P,H] (the bit of the hydrogen's side when it bonds), counts int32 [P,2] (the (H, acceptor) pairs per kind) and the
        results of `place`.  Nothing is read back, nothing synchronises."""
        x = self._poses(x_pred, "hbonds")
        if placed is None:
            placed = self.place(x)
        P, A, H, L, R = x.shape[0], x.shape[1], self.n_hydrogens, self.n_atoms, self.n_residues
        x_h, ok = placed["x_h"], placed["placed"]
        if (tuple(x_h.shape) != (P, H, 3) or tuple(ok.shape) != (P, H) or x_h.dtype != torch.float32 or ok.dtype != torch.uint8 or
                x_h.device != x.device or ok.device != x.device):
            raise ValueError(f"Hydrogens.hbonds: `placed` is what `place` returned for these {P} poses")
        L_ = ops._lib.init()
        t = self.tables(x.device)
        HPl, HPr, NAr, NAl = self.n_ligand_polar, self.n_receptor_polar, self.n_receptor_acceptors, self.n_ligand_acceptors
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=x.device)
        nbytes = L_.pd_hydrogen_bonds_workspace(P, HPl, HPr, NAr, NAl)
        ops.check(min(nbytes, 0), "pd_hydrogen_bonds_workspace")
        ws = new((nbytes // 8,), torch.float64)
        bits, ligand_bits, h_bits, counts = new((P, R), torch.uint8), new((P, L), torch.uint8), new((P, H), torch.uint8), new((P, 2), torch.int32)
        opt = lambda tensor, n: ops.ptr(tensor) if n else None
        ops.check(L_.pd_hydrogen_bonds(ops.ptr(x), ops.ptr(x_h.contiguous()), ops.ptr(ok.contiguous()), ops.ptr(t["parent"]),
                                       opt(t["polar"], HPl + HPr), HPl, HPr, ops.ptr(t["polar_slot"]), opt(t["acc"], NAr + NAl), NAr, NAl,
                                       ops.ptr(t["racc_start"]), ops.ptr(t["rh_start"]), ops.ptr(t["ligand_idx"]), ops.ptr(t["lig_acc_slot"]),
                                       self._thr, ops.ptr(ws), nbytes, ops.ptr(bits), ops.ptr(ligand_bits), ops.ptr(h_bits), ops.ptr(counts),
                                       P, A, H, L, R, ops.stream()), "pd_hydrogen_bonds")
        return {"bits": bits, "ligand_bits": ligand_bits, "h_bits": h_bits, "counts": counts, **placed}

    #: what `compare` fingerprints reference coordinates with
    fingerprint = hbonds

    def pdb_template(self, template):
        """a `pdbio.PdbTemplate` -> one whose records are the template's heavy-atom records followed by one record per hydrogen whose
        parent has a record: the record type, residue name, chain and residue number of the parent, named H1, H2, ... within the
        residue, element H, serials that continue behind the system's atoms.  Its `format` / `blocks` take `x_all` of `place` and
        write protonated poses through `pd_pdb_format` (a pose with a hydrogen that is not placed raises there, as every coordinate
        that is not finite does)."""
        from .pdbio import PdbTemplate
        if template.n_atoms != self.n_pose_atoms:
            raise ValueError(f"Hydrogens.pdb_template: the template is over {template.n_atoms} atoms, the tables over {self.n_pose_atoms}")
        rows = template.rows.detach().cpu().numpy().reshape(-1, 81)
        record_of = {int(a): k for k, a in enumerate(template.atom.detach().cpu().tolist())}
        new_rows, atoms, seen = [], [], {}
        for h in range(self.n_hydrogens):
            k = record_of.get(int(self.parent[h]))
            if k is None:
                continue
            row = rows[k].copy()
            residue = bytes(row[17:26])
            seen[residue] = seen.get(residue, 0) + 1
            name, serial = f"H{seen[residue]}", template.n_atoms + h + 1
            if len(name) > 4 or serial > 99999:
                raise ValueError(f"Hydrogens.pdb_template: record {serial} ({name}) does not fit the fixed-width PDB columns")
            row[6:11] = np.frombuffer(f"{serial:>5}".encode("ascii"), dtype=np.uint8)
            row[12:16] = np.frombuffer(f"{name if len(name) == 4 else ' ' + name:<4}".encode("ascii"), dtype=np.uint8)
            row[76:78] = np.frombuffer(b" H", dtype=np.uint8)
            new_rows.append(row)
            atoms.append(self.n_pose_atoms + h)
        all_rows = np.concatenate([rows, np.asarray(new_rows, dtype=np.uint8).reshape(-1, 81)])
        all_atoms = np.concatenate([template.atom.detach().cpu().numpy().astype(np.int32), np.asarray(atoms, dtype=np.int32)])
        dev = template.rows.device
        return PdbTemplate.from_rows(all_rows, all_atoms, self.n_pose_atoms + self.n_hydrogens, device=dev if dev.type == "cuda" else None)

    def __repr__(self):
        return (f"Hydrogens(n_atoms={self.n_atoms}, n_pose_atoms={self.n_pose_atoms}, residues={self.n_residues}, "
                f"hydrogens={self.n_hydrogens}, rotor_groups={self.n_groups}, polar={self.n_ligand_polar}+{self.n_receptor_polar}, "
                f"acceptors={self.n_ligand_acceptors}+{self.n_receptor_acceptors}, receptor_typing={self.receptor_typing!r}, "
                f"thresholds={self.thresholds})")
