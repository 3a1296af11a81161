"""Which residues does this pose touch, and how?  A per-residue interaction fingerprint of every pose, in the manner of PLIP and
ProLIF, on the device (kernels `pd_plif_fingerprint`, `pd_plif_compare`, `pd_plif_pairwise`, csrc/plif.hip - its header comment
holds the same definition).

One system: a ligand of L atoms (`ligand_idx [L]`, `lig_active [L]`: hydrogens are inactive), the receptor atoms `rec_mask [A]` -
heavy atoms that exist and are not ligand atoms - and a residue id per atom, `residue_of [A]` in 0 .. R-1 (ids need not be
contiguous in atom order; a residue may own no receptor atom; in `from_batch` residue = token, so R = T and the ligand's tokens own
none).  A pair (active ligand atom i, receptor atom j) of a pose with the centre distance r = |x_i - x_j| shows one or more of six
kinds; bit k of a byte stands for kind k (`KIND_NAMES`):

    bit  kind            condition                                      threshold (`DEFAULT_THRESHOLDS`)
    0    contact         any pair                                       r < contact      4.0 A
    1    hydrophobic     both atoms HYDROPHOBIC                         r < hydrophobic  4.5 A
    2    hbond_donor     ligand atom DONOR, receptor atom ACCEPTOR      r < hbond        3.5 A
    3    hbond_acceptor  ligand atom ACCEPTOR, receptor atom DONOR      r < hbond        3.5 A
    4    cationic        ligand atom CATION, receptor atom ANION        r < ionic        4.5 A
    5    anionic         ligand atom ANION, receptor atom CATION        r < ionic        4.5 A

Bits 6 and 7 are always 0.  `bits [P,R]` is the OR over the pairs whose receptor atom lies in the residue, `ligand_bits [P,L]` the OR
over the receptor atoms for a ligand atom (0 for an inactive one), `min_dist [P,R]` the exact minimum of r over the residue's pairs
(+inf for a residue without receptor atom, or when no ligand atom is active), `counts [P,6]` the number of residues that show each
kind.  HYDROPHOBIC / DONOR / ACCEPTOR are the bits of the type byte of `scoring.py`; CATION = 1 and ANION = 2 live in a separate
`charge` byte.

The thresholds are the `thresholds=` argument of the constructors and reach the kernel as values.  The defaults are the usual
heavy-atom distances of fingerprint packages; they are THIS PACKAGE'S DEFAULTS AND HAVE NOT BEEN VALIDATED on real complexes.
**Two caveats.**  The model predicts no hydrogens, so there is no donor - H - acceptor angle test, and donors are inferred exactly
as in `scoring.py` (ligand: valences; receptor: residue and atom names).  Pi-stacking, pi-cation and halogen bonds need ring
centroids and normals: they are the kinds of `ring_interactions.RingInteractions`.  Metal interactions and water bridges are out of
scope.

The residue-side fingerprint is an OR over ligand atoms of equal type, so it is invariant under the ligand's automorphisms: no
`LigandSymmetry` is needed to compare it with a ground truth.

Charges.  `receptor_charges_from_names`: LYS NZ and ARG NE / NH1 / NH2 are cations, ASP OD1 / OD2 and GLU OE1 / OE2 anions; HIS and
unknown residues are neutral.  `ligand_charges_from_bonds`: with `formal_charges` the sign decides and nothing else is looked at.
Without them, on the heavy-atom graph (aromatic bonds have order 1.5):
  * anions: both oxygens of a carboxylate (a carbon with exactly two terminal oxygens - one heavy neighbour each - and, when bond
    orders are given, a C=O among them; acids count as deprotonated), and the terminal oxygens of phosphate, phosphonate, sulfate
    and sulfonate groups (a P or S with at least three oxygen neighbours);
  * cations: the nitrogens of guanidine and amidine groups (a carbon without aromatic bond, without O or S neighbour, with at least
    two nitrogen neighbours and exactly one double bond, which goes to a nitrogen - this needs bond orders), and aliphatic amine
    nitrogens: single bonds only, no aromatic bond on the nitrogen or on a neighbour, no hetero-atom neighbour, no neighbour carbon
    doubly bonded to N, O or S.  Amides, anilines and sulfonamides are therefore neutral.

`InteractionFingerprint` holds one system's tables, built once on the host (the receptor atoms sorted by residue, CSR);
`fingerprint(x_pred)` returns device tensors and never synchronises; `compare`, `pairwise` and `satisfies` work on the `bits`;
`driver.redock(..., interactions=)` reports the fingerprint of the kept poses.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .scoring import (ACCEPTOR, DONOR, HYDROPHOBIC, _atomic_numbers, _bond_list, _host, element_types, ligand_types_from_bonds,
                      names_from_meta, receptor_types_from_names)

__all__ = ["InteractionFingerprint", "KIND_NAMES", "THRESHOLD_NAMES", "DEFAULT_THRESHOLDS", "CATION", "ANION", "kind_mask",
           "receptor_charges_from_names", "ligand_charges_from_bonds", "residue_csr", "residue_labels_from_meta", "MAX_ATOMS",
           "MAX_POSE_ATOMS", "MAX_POSES"]

#: the six kinds in bit order
KIND_NAMES = ("contact", "hydrophobic", "hbond_donor", "hbond_acceptor", "cationic", "anionic")
#: the four thresholds in the order the kernel takes them, and this package's (unvalidated) defaults in A
THRESHOLD_NAMES = ("contact", "hydrophobic", "hbond", "ionic")
DEFAULT_THRESHOLDS = {"contact": 4.0, "hydrophobic": 4.5, "hbond": 3.5, "ionic": 4.5}
#: bits of a charge byte
CATION, ANION = 1, 2
#: limits of the kernels (csrc/plif.hip): ligand atoms, pose atoms, poses; and R <= A
MAX_ATOMS, MAX_POSE_ATOMS, MAX_POSES = 1024, 1 << 22, 65535

_CATIONS = {"LYS": ("NZ",), "ARG": ("NE", "NH1", "NH2")}
_ANIONS = {"ASP": ("OD1", "OD2"), "GLU": ("OE1", "OE2")}


def _mask_of(kinds: Optional[Iterable[str]], names: Sequence[str]) -> int:
    """the byte mask of a sequence of kind names out of `names` (None: all of them)"""
    if kinds is None:
        return (1 << len(names)) - 1
    if isinstance(kinds, str):
        kinds = (kinds,)
    mask = 0
    for k in kinds:
        if k not in names:
            raise ValueError(f"unknown interaction kind {k!r}; the kinds are {tuple(names)}")
        mask |= 1 << names.index(k)
    if mask == 0:
        raise ValueError("kinds must name at least one interaction kind")
    return mask


def kind_mask(kinds: Optional[Iterable[str]] = None) -> int:
    """the byte mask of a sequence of kind names (default: all six)"""
    return _mask_of(kinds, KIND_NAMES)


def receptor_charges_from_names(res_names: Sequence[str], atom_names: Sequence[str]) -> np.ndarray:
    """uint8 [n]: the charge byte of every receptor atom from its residue and atom name - LYS NZ, ARG NE / NH1 / NH2: CATION; ASP
    OD1 / OD2, GLU OE1 / OE2: ANION; HIS and everything else, unknown residues included: 0"""
    if len(res_names) != len(atom_names):
        raise ValueError(f"receptor_charges_from_names: {len(res_names)} residue names, {len(atom_names)} atom names")
    q = np.zeros(len(res_names), dtype=np.uint8)
    for k, (res, name) in enumerate(zip(res_names, atom_names)):
        res, name = str(res).strip().upper(), str(name).strip().upper()
        if name in _CATIONS.get(res, ()):
            q[k] = CATION
        elif name in _ANIONS.get(res, ()):
            q[k] = ANION
    return q


def ligand_charges_from_bonds(elements, bonds: Iterable[Tuple[int, int]], bond_orders: Optional[Sequence[float]] = None,
                              formal_charges=None) -> np.ndarray:
    """uint8 [L]: the charge byte (CATION, ANION or 0) of every ligand atom.  elements: atomic numbers (or symbols) [L]; bonds: pairs
    of indices into them; bond_orders (default: unknown - all single, aromatic 1.5).  With `formal_charges` [L] the sign decides;
    without them the rules of the module docstring: carboxylate, phosphate, phosphonate, sulfate and sulfonate oxygens are anions;
    guanidine and amidine nitrogens and aliphatic amine nitrogens are cations; amides, anilines and sulfonamides are neutral."""
    z = _atomic_numbers(elements)
    n = len(z)
    bonds, orders = _bond_list(n, bonds, bond_orders, "ligand_charges_from_bonds")
    q = np.zeros(n, dtype=np.uint8)
    if formal_charges is not None:
        fc = _host(formal_charges, np.int64).reshape(-1)
        if fc.shape[0] != n:
            raise ValueError(f"ligand_charges_from_bonds: {n} elements, {fc.shape[0]} formal charges")
        q[fc > 0] = CATION
        q[fc < 0] = ANION
        return q
    nb: List[List[Tuple[int, float]]] = [[] for _ in range(n)]
    for (i, j), o in zip(bonds, orders):
        nb[i].append((j, o))
        nb[j].append((i, o))
    heavy = [[(b, o) for b, o in nb[a] if z[b] != 1] for a in range(n)]
    aromatic = [any(o == 1.5 for _, o in nb[a]) for a in range(n)]
    terminal_o = [z[a] == 8 and len(heavy[a]) == 1 for a in range(n)]
    for a in range(n):
        if z[a] == 6:
            oxy = [(b, o) for b, o in heavy[a] if terminal_o[b]]
            n_oxy = sum(1 for b, _ in heavy[a] if z[b] == 8)
            if len(oxy) == 2 and n_oxy == 2 and len(heavy[a]) <= 3 and (bond_orders is None or any(o >= 1.5 for _, o in oxy)):
                for b, _ in oxy:                                     # carboxylate
                    q[b] = ANION
            nitro = [b for b, _ in heavy[a] if z[b] == 7]
            double = [b for b, o in heavy[a] if o == 2.0]
            if (len(nitro) >= 2 and not aromatic[a] and len(double) == 1 and z[double[0]] == 7 and
                    not any(z[b] in (8, 16) for b, _ in heavy[a])):
                for b in nitro:                                      # guanidine, amidine
                    q[b] = CATION
        elif z[a] in (15, 16):
            if sum(1 for b, _ in heavy[a] if z[b] == 8) >= 3:        # phosphate, phosphonate, sulfate, sulfonate
                for b, _ in heavy[a]:
                    if terminal_o[b]:
                        q[b] = ANION
    for a in range(n):
        if z[a] != 7 or q[a] or not heavy[a]:
            continue
        if any(o != 1.0 for _, o in nb[a]) or aromatic[a]:
            continue
        ok = True
        for b, _ in heavy[a]:
            if z[b] != 6 or aromatic[b] or any(o == 2.0 and z[c] in (7, 8, 16) for c, o in heavy[b]):
                ok = False
        if ok:
            q[a] = CATION                                            # aliphatic amine
    return q


def residue_csr(residue_of, rec_mask, n_residues: int) -> Tuple[np.ndarray, np.ndarray]:
    """(res_start int32 [R + 1], res_atom int32 [N]): the receptor atoms (rec_mask != 0) sorted by residue, atoms of one residue in
    ascending order; the atoms of residue s are res_atom[res_start[s] : res_start[s + 1]]"""
    res = np.asarray(residue_of, dtype=np.int64).reshape(-1)
    atoms = np.nonzero(np.asarray(rec_mask).reshape(-1))[0]
    R = int(n_residues)
    if len(atoms) and (res[atoms].min() < 0 or res[atoms].max() >= R):
        raise ValueError(f"InteractionFingerprint: residue_of must lie in 0 .. {R - 1}")
    order = np.argsort(res[atoms], kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(res[atoms], minlength=R))])
    return start.astype(np.int32), atoms[order].astype(np.int32)


def residue_labels_from_meta(infer_meta_data, residue_of, n_residues: int) -> List[str]:
    """a printable name per residue id from the loader's naming tables: "SER83" (residue name and, when the tables hold one, the
    residue index) for a residue of a polymer, "LIG:C7" (residue name and atom name) for a ligand token; "" for an id no atom has"""
    res, names, _, cls = names_from_meta(infer_meta_data)
    chunk_sizes = [int(c) for c in infer_meta_data["conformer_id_to_chunk_sizes"]]
    index = infer_meta_data.get("residue_index") if hasattr(infer_meta_data, "get") else None
    conf_of = np.repeat(np.arange(len(chunk_sizes)), chunk_sizes)[:len(res)]
    rid = np.asarray(residue_of, dtype=np.int64).reshape(-1)
    labels = [""] * int(n_residues)
    for a in range(min(len(res), len(rid)) - 1, -1, -1):             # descending: a residue is named by its first atom
        if str(cls[a]).lower() == "ligand":
            labels[rid[a]] = f"{res[a]}:{names[a]}"
        else:
            labels[rid[a]] = f"{res[a]}{int(index[conf_of[a]])}" if index is not None else str(res[a])
    return labels


def _thresholds(thresholds) -> Tuple[float, float, float, float]:
    t = dict(DEFAULT_THRESHOLDS)
    if thresholds is None:
        pass
    elif isinstance(thresholds, dict):
        bad = set(thresholds) - set(THRESHOLD_NAMES)
        if bad:
            raise ValueError(f"InteractionFingerprint: unknown thresholds {sorted(bad)}; they are {THRESHOLD_NAMES}")
        t.update(thresholds)
    else:
        vals = list(thresholds)
        if len(vals) != len(THRESHOLD_NAMES):
            raise ValueError(f"InteractionFingerprint: thresholds are {THRESHOLD_NAMES}, got {len(vals)} values")
        t = dict(zip(THRESHOLD_NAMES, vals))
    out = tuple(float(t[k]) for k in THRESHOLD_NAMES)
    if any(not math.isfinite(v) or v < 0 for v in out):
        raise ValueError(f"InteractionFingerprint: a threshold must be finite and not negative, got {dict(zip(THRESHOLD_NAMES, out))}")
    return out


class _ByteRows:
    """what `InteractionFingerprint` and `ring_interactions.RingInteractions` do with their `bits` [P,R] - one byte per residue, bit
    k = kind k of the class's `_kind_names`: `compare`, `pairwise`, `satisfies`, `required_row`, `describe`, all through
    `pd_plif_compare` / `pd_plif_pairwise`.  A subclass provides `_name`, `_kind_names`, `n_residues`, `n_pose_atoms`,
    `residue_labels` and `fingerprint`."""
    _name = "InteractionFingerprint"
    _kind_names = KIND_NAMES

    def _mask(self, kinds) -> int:
        return _mask_of(kinds, self._kind_names)

    def _bits(self, bits, what):
        if not isinstance(bits, torch.Tensor) or bits.dtype != torch.uint8 or bits.dim() != 2 or bits.shape[1] != self.n_residues:
            raise ValueError(f"{self._name}.{what}: bits must be a uint8 tensor [P,{self.n_residues}] as `fingerprint` returns it")
        if not 1 <= bits.shape[0] <= MAX_POSES:
            raise ValueError(f"{self._name}.{what}: {bits.shape[0]} poses; the kernel takes 1 .. {MAX_POSES}")
        return bits.contiguous()

    def compare(self, bits: torch.Tensor, reference, kinds: Optional[Iterable[str]] = None) -> Dict[str, torch.Tensor]:
        """bits [P,R] against a reference: a uint8 row [R], or coordinates [A,3] (e.g. `x_gt`), which are fingerprinted first.  Counted
        over (residue, kind) pairs of the `kinds` (names of the class's kinds, `KIND_NAMES` here; default all - `kinds=("hbond_donor",
        "hbond_acceptor", "cationic", "anionic")` leaves plain contacts out): shared int32 [P], n_pose int32 [P], n_reference int32 [], recovery [P] =
        shared / n_reference (1 where the reference shows nothing) and tanimoto [P] = shared / (n_pose + n_reference - shared) (1 where
        both show nothing).  Device tensors, no read-back."""
        mask = self._mask(kinds)
        bits = self._bits(bits, "compare")
        ref = reference if isinstance(reference, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(reference))
        ref = ref.to(bits.device)
        if ref.dtype != torch.uint8:
            if ref.dim() != 2 or tuple(ref.shape) != (self.n_pose_atoms, 3) or not ref.is_floating_point():
                raise ValueError(f"{self._name}.compare: the reference is a uint8 row [{self.n_residues}] or coordinates "
                                 f"[{self.n_pose_atoms},3], got {ref.dtype} {tuple(ref.shape)}")
            ref = self.fingerprint(ref[None])["bits"][0]
        if ref.dim() != 1 or ref.shape[0] != self.n_residues:
            raise ValueError(f"{self._name}.compare: a reference row holds {self.n_residues} bytes, got {tuple(ref.shape)}")
        ref = ref.contiguous()
        L_ = ops._lib.init()
        P, R = bits.shape
        new = lambda n, dtype: torch.empty(n, dtype=dtype, device=bits.device)
        shared, n_pose, n_ref = new(P, torch.int32), new(P, torch.int32), new(1, torch.int32)
        recovery, tanimoto = new(P, torch.float32), new(P, torch.float32)
        ops.check(L_.pd_plif_compare(ops.ptr(bits), ops.ptr(ref), mask, ops.ptr(shared), ops.ptr(n_pose), ops.ptr(n_ref), ops.ptr(recovery),
                                     ops.ptr(tanimoto), P, R, ops.stream()), "pd_plif_compare")
        return {"shared": shared, "n_pose": n_pose, "n_reference": n_ref.reshape(()), "recovery": recovery, "tanimoto": tanimoto}

    def pairwise(self, bits: torch.Tensor, kinds: Optional[Iterable[str]] = None) -> torch.Tensor:
        """tanimoto fp32 [P,P] between every two rows of bits [P,R] over the `kinds` (as in `compare`): symmetric, the diagonal exactly
        1 - a similarity to cluster poses by binding mode"""
        mask = self._mask(kinds)
        bits = self._bits(bits, "pairwise")
        L_ = ops._lib.init()
        P, R = bits.shape
        out = torch.empty((P, P), dtype=torch.float32, device=bits.device)
        ops.check(L_.pd_plif_pairwise(ops.ptr(bits), mask, ops.ptr(out), P, R, ops.stream()), "pd_plif_pairwise")
        return out

    def required_row(self, required: Iterable[Tuple[object, str]]) -> np.ndarray:
        """uint8 [R]: the byte row with the bits of `required`, pairs (residue id or residue label, kind name)"""
        row = np.zeros(self.n_residues, dtype=np.uint8)
        for residue, kind in required:
            if isinstance(residue, str):
                if self.residue_labels is None or residue not in self.residue_labels:
                    raise ValueError(f"{self._name}: no residue is labelled {residue!r}")
                residue = self.residue_labels.index(residue)
            if not 0 <= int(residue) < self.n_residues:
                raise ValueError(f"{self._name}: residue {residue} is not in 0 .. {self.n_residues - 1}")
            row[int(residue)] |= self._mask((kind,))
        return row

    def satisfies(self, bits: torch.Tensor, required: Iterable[Tuple[object, str]]) -> torch.Tensor:
        """bool [P] on the device: does the pose show every required (residue, kind)?  A `compare` against the required row with
        shared == n_reference; nothing required is satisfied by every pose."""
        out = self.compare(bits, torch.from_numpy(self.required_row(required)))
        return out["shared"] == out["n_reference"]

    def describe(self, bits_row) -> List[Tuple[object, List[str]]]:
        """host helper: one byte row [R] (a tensor is read back) -> [(residue label or id, [kind names])] of the residues that show
        anything, in residue order"""
        row = np.asarray(bits_row.detach().cpu() if isinstance(bits_row, torch.Tensor) else bits_row).reshape(-1)
        if row.shape[0] != self.n_residues:
            raise ValueError(f"{self._name}.describe: a row holds {self.n_residues} bytes, got {row.shape[0]}")
        label = (lambda s: self.residue_labels[s] or s) if self.residue_labels is not None else (lambda s: s)
        return [(label(int(s)), [k for b, k in enumerate(self._kind_names) if int(row[s]) >> b & 1]) for s in np.nonzero(row)[0]]


class InteractionFingerprint(_ByteRows):
    """One system's tables for `pd_plif_fingerprint`: host copies (numpy: `types` uint8 [A], `charges` uint8 [A], `ligand_idx` int32
    [L], `lig_active` uint8 [L], `rec_mask` uint8 [A], `residue_of` int32 [A], the CSR `res_start` int32 [R + 1] / `res_atom` int32
    [N]), `thresholds` (dict, A), `receptor_typing` (how the receptor's bytes were made: "given", "names" or "elements" - the last
    has no donors, acceptors or charges on the receptor, so the kinds hbond_donor, hbond_acceptor, cationic and anionic are empty),
    `residue_labels` (a name per residue, or None) and, uploaded once per device, what the kernel reads.  `n_atoms` is the ligand's
    atom count L, `n_pose_atoms` the A of the poses `fingerprint` takes, `n_residues` R, `n_receptor_atoms` N."""

    def __init__(self, types, charges, ligand_idx, lig_active, rec_mask, residue_of, n_residues, thresholds=None,
                 receptor_typing: str = "given", residue_labels=None, device=None):
        self.types, self.charges, self.ligand_idx, self.lig_active = types, charges, ligand_idx, lig_active
        self.rec_mask, self.residue_of, self.n_residues = rec_mask, residue_of, int(n_residues)
        self.res_start, self.res_atom = residue_csr(residue_of, rec_mask, self.n_residues)
        self.threshold_values = _thresholds(thresholds)
        self.thresholds = dict(zip(THRESHOLD_NAMES, self.threshold_values))
        self.receptor_typing = receptor_typing
        self.residue_labels = None if residue_labels is None else [str(s) for s in residue_labels]
        if self.residue_labels is not None and len(self.residue_labels) != self.n_residues:
            raise ValueError(f"InteractionFingerprint: {len(self.residue_labels)} residue labels for {self.n_residues} residues")
        self.n_atoms, self.n_pose_atoms, self.n_receptor_atoms = int(ligand_idx.shape[0]), int(types.shape[0]), int(self.res_atom.shape[0])
        self._thr = (C.c_float * len(THRESHOLD_NAMES))(*self.threshold_values)
        self._tables = {}
        if device is not None:
            self.tables(device)

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_types(types, charges, ligand_idx, receptor_mask, residue_of, n_residues: Optional[int] = None, a_mask=None,
                   ligand_active=None, thresholds=None, residue_labels=None, receptor_typing: str = "given", device=None):
        """types uint8 [A]: the type byte of every pose atom as `VinaScore` takes it (HYDROPHOBIC, DONOR, ACCEPTOR are looked at);
        charges uint8 [A]: CATION, ANION or 0; ligand_idx [L]: the ligand's atoms in a pose; receptor_mask [A] (> 0: the atom counts
        as receptor; ligand atoms never do); residue_of [A]: the residue id of every atom; n_residues (default: the largest id + 1);
        a_mask [A] (default: every atom exists); ligand_active [L] (default: all): 0 = the ligand atom takes no part (a hydrogen);
        thresholds: a dict over `THRESHOLD_NAMES` (missing ones keep their default) or four values in that order."""
        t = _host(types, np.int64).reshape(-1)
        q = _host(charges, np.int64).reshape(-1)
        lig = _host(ligand_idx, np.int64).reshape(-1)
        res = _host(residue_of, np.int64).reshape(-1)
        A, L = int(t.shape[0]), int(lig.shape[0])
        if A < 1 or A > MAX_POSE_ATOMS or not 1 <= L <= MAX_ATOMS:
            raise ValueError(f"InteractionFingerprint: {L} ligand atoms of {A}; the kernel takes 1 .. {MAX_ATOMS} of up to {MAX_POSE_ATOMS}")
        if t.min() < 0 or t.max() > 127:
            raise ValueError("InteractionFingerprint: a type byte holds bits 0 - 6 only")
        if q.shape[0] != A or q.min() < 0 or q.max() > (CATION | ANION):
            raise ValueError(f"InteractionFingerprint: charges must hold {A} bytes of CATION, ANION or 0")
        if lig.min() < 0 or lig.max() >= A or len(set(lig.tolist())) != L:
            raise ValueError(f"InteractionFingerprint: ligand_idx must hold {L} distinct atom indices below {A}")
        rec = _host(receptor_mask, np.float64).reshape(-1) > 0
        am = np.ones(A, dtype=bool) if a_mask is None else _host(a_mask, np.float64).reshape(-1) > 0
        act = np.ones(L, dtype=bool) if ligand_active is None else _host(ligand_active, np.float64).reshape(-1) > 0
        if rec.shape[0] != A or am.shape[0] != A or act.shape[0] != L or res.shape[0] != A:
            raise ValueError(f"InteractionFingerprint: types are given for {A} atoms and {L} ligand atoms; receptor_mask {rec.shape[0]}, "
                             f"a_mask {am.shape[0]}, ligand_active {act.shape[0]}, residue_of {res.shape[0]}")
        R = int(res.max()) + 1 if n_residues is None else int(n_residues)
        if res.min() < 0 or res.max() >= R or R < 1:
            raise ValueError(f"InteractionFingerprint: residue_of must lie in 0 .. {R - 1}")
        if R > A:
            raise ValueError(f"InteractionFingerprint: {R} residues of {A} atoms; the kernel takes at most one residue per atom")
        rec = rec & am
        rec[lig] = False
        return InteractionFingerprint(t.astype(np.uint8), q.astype(np.uint8), lig.astype(np.int32), (act & am[lig]).astype(np.uint8),
                                      rec.astype(np.uint8), res.astype(np.int32), R, thresholds, receptor_typing, residue_labels, device)

    @staticmethod
    def from_bonds(elements, bonds, ligand_idx, residue_of, bond_orders=None, receptor_types=None, receptor_charges=None,
                   n_residues: Optional[int] = None, a_mask=None, n_hydrogens=None, formal_charges=None, thresholds=None,
                   residue_labels=None, receptor_typing: Optional[str] = None, device=None):
        """elements: atomic numbers of all A pose atoms; bonds: pairs of LOCAL ligand indices (position in `ligand_idx`) with their
        `bond_orders`; the ligand is typed by `ligand_types_from_bonds` and `ligand_charges_from_bonds`, the receptor - every other
        existing heavy atom - by `receptor_types` / `receptor_charges` uint8 [A] when given (e.g. `receptor_types_from_names`,
        `receptor_charges_from_names`), else by its elements alone: no donors, no acceptors, no charges (`receptor_typing`
        "elements").  Hydrogens take no part on either side."""
        z = _atomic_numbers(elements)
        lig = _host(ligand_idx, np.int64).reshape(-1)
        A, L = len(z), len(lig)
        if L < 1 or lig.min() < 0 or lig.max() >= A or len(set(lig.tolist())) != L:
            raise ValueError(f"InteractionFingerprint: ligand_idx must hold distinct atom indices below {A}")
        bonds, orders = _bond_list(L, bonds, bond_orders, "InteractionFingerprint")
        if receptor_types is None:
            if receptor_charges is not None:
                raise ValueError("InteractionFingerprint: receptor_charges are given without receptor_types")
            types, typing = element_types(z), "elements"
        else:
            types, typing = _host(receptor_types, np.int64).reshape(-1).astype(np.uint8), "given"
            if types.shape[0] != A:
                raise ValueError(f"InteractionFingerprint: elements are given for {A} atoms, receptor_types for {types.shape[0]}")
        charges = np.zeros(A, dtype=np.uint8) if receptor_charges is None else _host(receptor_charges, np.int64).reshape(-1).astype(np.uint8)
        if charges.shape[0] != A:
            raise ValueError(f"InteractionFingerprint: elements are given for {A} atoms, receptor_charges for {charges.shape[0]}")
        types, charges = types.copy(), charges.copy()
        types[lig] = ligand_types_from_bonds(z[lig], bonds, orders, n_hydrogens, formal_charges)
        charges[lig] = ligand_charges_from_bonds(z[lig], bonds, None if bond_orders is None else orders, formal_charges)
        heavy = z != 1
        return InteractionFingerprint.from_types(types, charges, lig, heavy, residue_of, n_residues=n_residues, a_mask=a_mask,
                                                 ligand_active=heavy[lig], thresholds=thresholds, residue_labels=residue_labels,
                                                 receptor_typing=receptor_typing or typing, device=device)

    @staticmethod
    def from_batch(batch, bonds, bond_orders=None, infer_meta_data=None, thresholds=None, receptor_types=None, receptor_charges=None,
                   **kw):
        """from a feature dict: the ligand's atoms are those of `driver.ligand_atom_mask`, the elements come from the one-hot
        `ref_feat[:, 4:132]` (index = atomic number - 1), `a_mask` from the batch (when it has one), a residue is a token
        (`atom_id_to_token_id`; R = T, the ligand's tokens own no receptor atom); the tables are uploaded to the batch's device.  The
        receptor is typed from `receptor_types` / `receptor_charges` when given, else from `infer_meta_data` (the loader's naming
        tables: `receptor_types_from_names`, `receptor_charges_from_names`, and `residue_labels`), else by element only -
        `receptor_typing` records which.  Other keywords as for `from_bonds`."""
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
                raise ValueError(f"InteractionFingerprint: infer_meta_data names {len(res)} atoms, the batch holds {int(elements.shape[0])}")
            if receptor_types is None:
                receptor_types = receptor_types_from_names(res, names, z)
                if receptor_charges is None:
                    receptor_charges = receptor_charges_from_names(res, names)
                kw.setdefault("receptor_typing", "names")
            kw.setdefault("residue_labels", residue_labels_from_meta(infer_meta_data, _host(residue_of, np.int64), kw["n_residues"]))
        return InteractionFingerprint.from_bonds(elements, bonds, lig, residue_of, bond_orders=bond_orders, receptor_types=receptor_types,
                                                 receptor_charges=receptor_charges, thresholds=thresholds, **kw)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernel's tables on `device` (uploaded once)"""
        names = ("types", "charges", "ligand_idx", "lig_active", "res_start", "res_atom")
        return ops.cached_upload(self._tables, device, lambda up: {k: up(getattr(self, k)) for k in names})

    def fingerprint(self, x_pred: torch.Tensor) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> dict of device tensors: bits uint8 [P,R] (bit k = kind k of `KIND_NAMES` between the ligand and
        the residue), ligand_bits uint8 [P,L] (the same per ligand atom), min_dist fp32 [P,R] (the closest ligand - residue heavy-atom
        distance; +inf for a residue without receptor atom) and counts int32 [P,6] (residues per kind).  Nothing is read back, nothing
        synchronises."""
        if x_pred.dim() != 3 or x_pred.shape[1] != self.n_pose_atoms or x_pred.shape[2] != 3:
            raise ValueError(f"InteractionFingerprint.fingerprint: the tables are over {self.n_pose_atoms} pose atoms, x_pred has shape "
                             f"{tuple(x_pred.shape)}")
        if not 1 <= x_pred.shape[0] <= MAX_POSES:
            raise ValueError(f"InteractionFingerprint.fingerprint: {x_pred.shape[0]} poses; the kernel takes 1 .. {MAX_POSES}")
        L_ = ops._lib.init()
        x = x_pred.float().contiguous()
        P, A, L, R, N = x.shape[0], x.shape[1], self.n_atoms, self.n_residues, self.n_receptor_atoms
        t = self.tables(x.device)
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=x.device)
        ws_bits, ws_min = new((P, max(N, 1)), torch.uint8), new((P, max(N, 1)), torch.float32)
        bits, ligand_bits = new((P, R), torch.uint8), new((P, L), torch.uint8)
        min_dist, counts = new((P, R), torch.float32), new((P, len(KIND_NAMES)), torch.int32)
        ops.check(L_.pd_plif_fingerprint(ops.ptr(x), ops.ptr(t["ligand_idx"]), ops.ptr(t["types"]), ops.ptr(t["charges"]),
                                         ops.ptr(t["lig_active"]), ops.ptr(t["res_start"]), ops.ptr(t["res_atom"]) if N else None,
                                         self._thr, ops.ptr(ws_bits), ops.ptr(ws_min), ops.ptr(bits), ops.ptr(ligand_bits),
                                         ops.ptr(min_dist), ops.ptr(counts), P, A, L, R, N, ops.stream()), "pd_plif_fingerprint")
        return {"bits": bits, "ligand_bits": ligand_bits, "min_dist": min_dist, "counts": counts}

    def __repr__(self):
        return (f"InteractionFingerprint(n_atoms={self.n_atoms}, n_pose_atoms={self.n_pose_atoms}, residues={self.n_residues}, "
                f"receptor_atoms={self.n_receptor_atoms}, receptor_typing={self.receptor_typing!r}, thresholds={self.thresholds})")
