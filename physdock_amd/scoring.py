"""How well does the ligand fit the pocket, on a physical scale?  A Vina-style interaction score of every pose and its forces on the
ligand atoms, on the device (kernel `pd_vina_score`, csrc/vina.hip).

The functional form is the intermolecular part of the AutoDock Vina scoring function (Trott & Olson, J. Comput. Chem. 2010): over
every pair (ligand heavy atom i, receptor heavy atom j) of a pose with r = |x_i - x_j| < 8 A and the surface distance
d = r - R_i - R_j (X-Score radii `RADII`)

    gauss1       exp(-(d / 0.5)^2)                                                 weight -0.0356
    gauss2       exp(-((d - 3) / 2)^2)                                                    -0.00516
    repulsion    d^2 for d < 0                                                            +0.840
    hydrophobic  both atoms hydrophobic: 1 for d <= 0.5, 1.5 - d up to 1.5                -0.0351
    hbond        a donor and an acceptor: 1 for d <= -0.7, -d / 0.7 up to 0               -0.587

    inter = sum_t w_t terms_t,        score = inter / (1 + 0.0585 n_rot)   (kcal/mol),        forces_i = -d inter / d x_i

It needs no ground truth and no trained weights, and it is the one pose measure of the package that can compare different ligands
in one receptor.  **Two caveats.**  The weights are Vina's published ones; nothing here validates them on real complexes or fits
them to this model's poses.  The atom typing is heuristic: the model predicts heavy atoms only, so hydrogens - and with them
donors - are inferred from valences (ligand) or from residue and atom names (receptor).  Vina's intramolecular term and a minimiser
on top of the forces live in `refine.VinaRefine` (rigid-body and torsion refinement of every pose, csrc/vina_refine.hip); this score
stays the intermolecular part.

`VinaScore` holds one system's type table, built once on the host; `score(x_pred)` returns device tensors and never synchronises.
`ranking.rank_by_score` orders poses by it, `driver.redock(..., vina=)` reports it for the kept poses.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

__all__ = ["VinaScore", "TERM_NAMES", "WEIGHTS", "RADII", "DEFAULT_RADIUS", "CUTOFF", "ROT_WEIGHT", "HYDROPHOBIC", "DONOR", "ACCEPTOR",
           "radius_class", "ligand_types_from_bonds", "receptor_types_from_names", "element_types", "count_rotatable_bonds",
           "names_from_meta", "MAX_ATOMS", "MAX_POSE_ATOMS", "MAX_POSES"]

#: the five terms in the order of `terms[:, t]`, and their weights (kcal/mol)
TERM_NAMES = ("gauss1", "gauss2", "repulsion", "hydrophobic", "hbond")
WEIGHTS = (-0.0356, -0.00516, 0.840, -0.0351, -0.587)
#: X-Score radii (A) by atomic number in radius-class order (bits 0 - 3 of a type byte); any other element is class 9, DEFAULT_RADIUS
RADII = {6: 1.9, 7: 1.8, 8: 1.7, 15: 2.1, 16: 2.0, 9: 1.5, 17: 1.8, 35: 2.0, 53: 2.2}
DEFAULT_RADIUS, OTHER_CLASS = 1.2, 9
CUTOFF, ROT_WEIGHT = 8.0, 0.0585
#: flag bits of a type byte
HYDROPHOBIC, DONOR, ACCEPTOR = 16, 32, 64
#: limits of the kernel (csrc/vina.hip)
MAX_ATOMS, MAX_POSE_ATOMS, MAX_POSES = 1024, 1 << 22, 65535

_CLASS = {z: c for c, z in enumerate(RADII)}
_HALOGENS = (9, 17, 35, 53)
_VALENCE = {6: 4, 7: 3, 8: 2, 16: 2, 15: 3, 9: 1, 17: 1, 35: 1, 53: 1}
_SYMBOL_Z = {"C": 6, "N": 7, "O": 8, "P": 15, "S": 16, "F": 9, "CL": 17, "BR": 35, "I": 53, "H": 1, "D": 1}

# the 20 standard residues: side-chain carbons bonded to N or O (the backbone's CA and C always are), donors and acceptors by atom name
_STANDARD = ("ALA", "ARG", "ASN", "ASP", "CYS", "GLN", "GLU", "GLY", "HIS", "ILE", "LEU", "LYS", "MET", "PHE", "PRO", "SER", "THR", "TRP",
             "TYR", "VAL")
_POLAR_CARBONS = {"ARG": ("CD", "CZ"), "ASN": ("CG",), "ASP": ("CG",), "GLN": ("CD",), "GLU": ("CD",), "HIS": ("CG", "CD2", "CE1"),
                  "LYS": ("CE",), "PRO": ("CD",), "SER": ("CB",), "THR": ("CB",), "TRP": ("CD1", "CE2"), "TYR": ("CZ",)}
_DONORS = {"ARG": ("NE", "NH1", "NH2"), "ASN": ("ND2",), "GLN": ("NE2",), "LYS": ("NZ",), "TRP": ("NE1",), "HIS": ("ND1", "NE2"),
           "SER": ("OG",), "THR": ("OG1",), "TYR": ("OH",)}
_ACCEPTORS = {"ASP": ("OD1", "OD2"), "GLU": ("OE1", "OE2"), "ASN": ("OD1",), "GLN": ("OE1",), "HIS": ("ND1", "NE2"), "SER": ("OG",),
              "THR": ("OG1",), "TYR": ("OH",)}


def _host(t, dtype):
    return np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, dtype=dtype)


def _atomic_numbers(elements) -> np.ndarray:
    """atomic numbers from numbers or element symbols (unknown symbols: 0)"""
    seq = elements.detach().cpu().tolist() if isinstance(elements, torch.Tensor) else list(np.asarray(elements).reshape(-1).tolist())
    return np.asarray([_SYMBOL_Z.get(e.strip().upper(), 0) if isinstance(e, str) else int(e) for e in seq], dtype=np.int64)


def radius_class(elements) -> np.ndarray:
    """uint8 [n]: the radius class (bits 0 - 3 of a type byte) of each atomic number"""
    return np.asarray([_CLASS.get(int(z), OTHER_CLASS) for z in _atomic_numbers(elements)], dtype=np.uint8)


def element_types(elements, acceptors: bool = False) -> np.ndarray:
    """uint8 [n]: types from the elements alone - the radius class, carbon and the halogens hydrophobic (a carbon's neighbours are
    not known), no donor; with `acceptors` every oxygen is an acceptor"""
    z = _atomic_numbers(elements)
    t = radius_class(z)
    t[(z == 6) | np.isin(z, _HALOGENS)] |= HYDROPHOBIC
    if acceptors:
        t[z == 8] |= ACCEPTOR
    return t


def _bond_list(n, bonds, bond_orders, what):
    bonds = [(int(i), int(j)) for i, j in (bonds.tolist() if hasattr(bonds, "tolist") else bonds)]
    if any(not (0 <= i < n and 0 <= j < n) or i == j for i, j in bonds):
        raise ValueError(f"{what}: a bond leaves the {n} atoms or joins an atom to itself")
    orders = [1.0] * len(bonds) if bond_orders is None else [float(o) for o in bond_orders]
    if len(orders) != len(bonds):
        raise ValueError(f"{what}: {len(bonds)} bonds but {len(orders)} bond orders")
    return bonds, orders


def _hydrogen_counts(z, bonds, orders, n_hydrogens, charge):
    """(n_h, h_nb, heavy_nb, polar_nb) of every atom of a bond graph: the hydrogens it carries - `n_hydrogens` when given, else the
    default valence (C 4, N 3, O 2, S 2, P 3, halogen 1) - floor(sum of bond orders) + formal charge, clipped at 0, plus the explicit
    hydrogen neighbours -, its explicit hydrogen neighbours, its heavy neighbours, and whether it is bonded to N or O.  The one
    valence rule of the package: `ligand_types_from_bonds` types with it, `hydrogens.ligand_hydrogens_from_bonds` places with it."""
    n = len(z)
    order_sum, heavy_nb, h_nb, polar_nb = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for (i, j), o in zip(bonds, orders):
        for a, b in ((i, j), (j, i)):
            order_sum[a] += o
            if z[b] == 1:
                h_nb[a] += 1
            else:
                heavy_nb[a] += 1
            polar_nb[a] |= z[b] in (7, 8)
    if n_hydrogens is None:
        implicit = np.asarray([max(_VALENCE.get(int(e), 0) - int(np.floor(s + 1e-9)) + int(c), 0) if int(e) in _VALENCE else 0
                               for e, s, c in zip(z, order_sum, charge)], dtype=np.int64)
        n_h = implicit + h_nb
    else:
        n_h = _host(n_hydrogens, np.int64).reshape(-1)
    return n_h, h_nb, heavy_nb, polar_nb


def ligand_types_from_bonds(elements, bonds: Iterable[Tuple[int, int]], bond_orders: Optional[Sequence[float]] = None,
                            n_hydrogens=None, formal_charges=None) -> np.ndarray:
    """uint8 [L]: the type byte of every ligand atom from the bond graph.  elements: atomic numbers (or symbols) [L]; bonds: pairs of
    indices into them; bond_orders (default: all single; aromatic bonds count 1.5).  Hydrogens, when `n_hydrogens` [L] is not given:
    default valence (C 4, N 3, O 2, S 2, P 3, halogen 1) - floor(sum of bond orders) + formal charge, clipped at 0, plus the explicit
    hydrogen neighbours.  Donor: N or O with at least one hydrogen.  Acceptor: every O, and N without hydrogen, with at most two heavy
    neighbours and charge <= 0.  Hydrophobic: carbon not bonded to N or O, and F, Cl, Br, I."""
    z = _atomic_numbers(elements)
    n = len(z)
    bonds, orders = _bond_list(n, bonds, bond_orders, "ligand_types_from_bonds")
    charge = np.zeros(n, dtype=np.int64) if formal_charges is None else _host(formal_charges, np.int64).reshape(-1)
    if charge.shape[0] != n or (n_hydrogens is not None and len(n_hydrogens) != n):
        raise ValueError(f"ligand_types_from_bonds: {n} elements, but formal_charges / n_hydrogens of another length")
    n_h, _, heavy_nb, polar_nb = _hydrogen_counts(z, bonds, orders, n_hydrogens, charge)
    t = radius_class(z)
    t[((z == 6) & ~polar_nb) | np.isin(z, _HALOGENS)] |= HYDROPHOBIC
    t[((z == 7) | (z == 8)) & (n_h > 0)] |= DONOR
    t[(z == 8) | ((z == 7) & (n_h == 0) & (heavy_nb <= 2) & (charge <= 0))] |= ACCEPTOR
    return t


def receptor_types_from_names(res_names: Sequence[str], atom_names: Sequence[str], elements) -> np.ndarray:
    """uint8 [n]: the type byte of every receptor atom from its residue name, atom name and element, by a table of the 20 standard
    residues.  Donors: the backbone N except in PRO, ARG NE/NH1/NH2, ASN ND2, GLN NE2, LYS NZ, TRP NE1, HIS ND1/NE2, SER OG, THR OG1,
    TYR OH.  Acceptors: O/OXT, ASP OD1/OD2, GLU OE1/OE2, ASN OD1, GLN OE1, HIS ND1/NE2, SER OG, THR OG1, TYR OH.  A carbon is
    hydrophobic unless the residue's topology bonds it to N or O (CA and C always are).  An unknown residue falls back to the element
    rules (`element_types` with oxygen acceptors): no donors."""
    z = _atomic_numbers(elements)
    if not len(res_names) == len(atom_names) == len(z):
        raise ValueError(f"receptor_types_from_names: {len(res_names)} residue names, {len(atom_names)} atom names, {len(z)} elements")
    t = element_types(z, acceptors=True)
    for k, (res, name) in enumerate(zip(res_names, atom_names)):
        res, name = str(res).strip().upper(), str(name).strip().upper()
        if res not in _STANDARD:
            continue
        flags = 0
        if z[k] == 6 and name not in ("CA", "C") and name not in _POLAR_CARBONS.get(res, ()):
            flags |= HYDROPHOBIC
        if (name == "N" and res != "PRO") or name in _DONORS.get(res, ()):
            flags |= DONOR
        if name in ("O", "OXT") or name in _ACCEPTORS.get(res, ()):
            flags |= ACCEPTOR
        t[k] = (t[k] & 15) | flags
    return t


def count_rotatable_bonds(n_atoms: int, bonds: Iterable[Tuple[int, int]], bond_orders: Optional[Sequence[float]] = None) -> int:
    """Single, acyclic bonds of the heavy-atom graph whose two ends each have at least two neighbours; a bond to a triple-bonded atom
    is left out.  The amide C-N is not special-cased (Vina's own count of torsions treats it as fixed: pass `n_rot=` to override)."""
    n = int(n_atoms)
    bonds, orders = _bond_list(n, bonds, bond_orders, "count_rotatable_bonds")
    adj = [set() for _ in range(n)]
    triple = [False] * n
    for (i, j), o in zip(bonds, orders):
        adj[i].add(j); adj[j].add(i)
        if o == 3.0:
            triple[i] = triple[j] = True

    def in_ring(i, j):
        # is j reachable from i without the bond (i, j)?
        seen, stack = {i}, [i]
        while stack:
            a = stack.pop()
            for b in adj[a]:
                if (a == i and b == j) or b in seen:
                    continue
                if b == j:
                    return True
                seen.add(b); stack.append(b)
        return False

    return sum(1 for (i, j), o in zip(bonds, orders)
               if o == 1.0 and len(adj[i]) >= 2 and len(adj[j]) >= 2 and not triple[i] and not triple[j] and not in_ring(i, j))


def names_from_meta(infer_meta_data):
    """(residue names, atom names, atomic numbers, chain classes) of every atom of a system from the loader's naming tables - the object
    `pdbio.PdbTemplate` takes"""
    ccds = infer_meta_data["ccds"]
    inner = infer_meta_data["atom_id_to_conformer_atom_id"]
    chunk_sizes = [int(c) for c in infer_meta_data["conformer_id_to_chunk_sizes"]]
    conf = infer_meta_data["CONF_META_DATA"]
    res, names, z, cls = [], [], [], []
    offset, n_atoms = 0, len(inner)
    for ccd_id, (ccd, chunk) in enumerate(zip(ccds, chunk_sizes)):
        for i in inner[offset:offset + chunk]:
            if len(res) == n_atoms:
                break
            res.append(ccd.split()[0])
            names.append(str(conf[ccd]["ref_atom_name_chars"][int(i)]).strip())
            z.append(int(conf[ccd]["ref_element"][int(i)]) + 1)
            cls.append(infer_meta_data["CHAIN_CLASS"][ccd_id])
        offset += chunk
    return res, names, np.asarray(z, dtype=np.int64), cls


class VinaScore:
    """One system's tables for `pd_vina_score`: host copies (numpy: `types` uint8 [A], `ligand_idx` int32 [L], `rec_mask` uint8 [A],
    `lig_active` uint8 [L]), `n_rot`, `receptor_typing` (how the receptor's bytes were made: "given", "names" or "elements" - the last
    has no donors and no acceptors on the receptor, so its hbond term is 0) and, uploaded once per device, what the kernel reads.
    `n_atoms` is the ligand's atom count L, `n_pose_atoms` the A of the poses `score` takes."""

    def __init__(self, types, ligand_idx, rec_mask, lig_active, n_rot: float, receptor_typing: str = "given", device=None):
        self.types, self.ligand_idx, self.rec_mask, self.lig_active = types, ligand_idx, rec_mask, lig_active
        self.n_rot, self.receptor_typing = float(n_rot), receptor_typing
        self.n_atoms, self.n_pose_atoms = int(ligand_idx.shape[0]), int(types.shape[0])
        self._tables = {}
        if device is not None:
            self.tables(device)

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_types(types, ligand_idx, receptor_mask, n_rot: float, a_mask=None, ligand_active=None, receptor_typing: str = "given",
                   device=None):
        """types uint8 [A]: the type byte of every pose atom (bits 0 - 3 radius class, HYDROPHOBIC, DONOR, ACCEPTOR); ligand_idx [L]:
        the ligand's atoms in a pose; receptor_mask [A] (> 0: the atom counts as receptor; ligand atoms never do); n_rot: the
        ligand's rotatable bonds; a_mask [A] (default: every atom exists); ligand_active [L] (default: all): 0 = the ligand atom takes
        no part (a hydrogen)."""
        t = _host(types, np.int64).reshape(-1)
        lig = _host(ligand_idx, np.int64).reshape(-1)
        A, L = int(t.shape[0]), int(lig.shape[0])
        if A < 1 or A > MAX_POSE_ATOMS or not 1 <= L <= MAX_ATOMS:
            raise ValueError(f"VinaScore: {L} ligand atoms of {A}; the kernel takes 1 .. {MAX_ATOMS} of up to {MAX_POSE_ATOMS}")
        if t.min() < 0 or t.max() > 127:
            raise ValueError("VinaScore: a type byte holds bits 0 - 6 only")
        if lig.min() < 0 or lig.max() >= A or len(set(lig.tolist())) != L:
            raise ValueError(f"VinaScore: ligand_idx must hold {L} distinct atom indices below {A}")
        rec = _host(receptor_mask, np.float64).reshape(-1) > 0
        am = np.ones(A, dtype=bool) if a_mask is None else _host(a_mask, np.float64).reshape(-1) > 0
        act = np.ones(L, dtype=bool) if ligand_active is None else _host(ligand_active, np.float64).reshape(-1) > 0
        if rec.shape[0] != A or am.shape[0] != A or act.shape[0] != L:
            raise ValueError(f"VinaScore: types are given for {A} atoms and {L} ligand atoms; receptor_mask {rec.shape[0]}, a_mask "
                             f"{am.shape[0]}, ligand_active {act.shape[0]}")
        if not float(n_rot) >= 0:
            raise ValueError(f"VinaScore: n_rot must not be negative, got {n_rot}")
        rec = rec & am
        rec[lig] = False
        return VinaScore(t.astype(np.uint8), lig.astype(np.int32), rec.astype(np.uint8), (act & am[lig]).astype(np.uint8), n_rot,
                         receptor_typing, device)

    @staticmethod
    def from_bonds(elements, bonds, ligand_idx, bond_orders=None, receptor_types=None, n_rot=None, a_mask=None, n_hydrogens=None,
                   formal_charges=None, receptor_typing: Optional[str] = None, device=None):
        """elements: atomic numbers of all A pose atoms; bonds: pairs of LOCAL ligand indices (position in `ligand_idx`) with their
        `bond_orders`; the ligand is typed by `ligand_types_from_bonds`, the receptor - every other existing atom - by `receptor_types`
        uint8 [A] when given (e.g. `receptor_types_from_names`), else by its elements alone (no donors, no acceptors).  Hydrogens
        take no part on either side.  `n_rot` (default: `count_rotatable_bonds` of the ligand's heavy-atom graph)."""
        z = _atomic_numbers(elements)
        lig = _host(ligand_idx, np.int64).reshape(-1)
        A, L = len(z), len(lig)
        if L < 1 or lig.min() < 0 or lig.max() >= A or len(set(lig.tolist())) != L:
            raise ValueError(f"VinaScore: ligand_idx must hold distinct atom indices below {A}")
        bonds, orders = _bond_list(L, bonds, bond_orders, "VinaScore")
        if receptor_types is None:
            types, typing = element_types(z), "elements"
        else:
            types, typing = _host(receptor_types, np.int64).reshape(-1).astype(np.uint8), "given"
            if types.shape[0] != A:
                raise ValueError(f"VinaScore: elements are given for {A} atoms, receptor_types for {types.shape[0]}")
        types = types.copy()
        types[lig] = ligand_types_from_bonds(z[lig], bonds, orders, n_hydrogens, formal_charges)
        heavy = z != 1
        if n_rot is None:
            zl = z[lig]
            kept = [(b, o) for b, o in zip(bonds, orders) if zl[b[0]] != 1 and zl[b[1]] != 1]
            n_rot = count_rotatable_bonds(L, [b for b, _ in kept], [o for _, o in kept])
        return VinaScore.from_types(types, lig, heavy, n_rot, a_mask=a_mask, ligand_active=heavy[lig],
                                    receptor_typing=receptor_typing or typing, device=device)

    @staticmethod
    def from_batch(batch, bonds, bond_orders=None, receptor_types=None, infer_meta_data=None, **kw):
        """from a feature dict: the ligand's atoms are those of `driver.ligand_atom_mask`, the elements come from the one-hot
        `ref_feat[:, 4:132]` (index = atomic number - 1) as `PoseValidity.from_batch` reads them, `a_mask` from the batch (when it has
        one); the tables are uploaded to the batch's device.  The receptor is typed from `receptor_types` when given, else from
        `infer_meta_data` (the loader's naming tables, as `pdbio.PdbTemplate` takes them: `receptor_types_from_names`), else by element
        only, without donors and acceptors - `receptor_typing` records which.  Other keywords as for `from_bonds`."""
        from .driver import ligand_atom_mask
        lig = torch.nonzero(ligand_atom_mask(batch)).flatten()
        elements = batch["ref_feat"][:, 4:132].argmax(-1) + 1
        dev = batch["ref_feat"].device
        kw.setdefault("a_mask", batch.get("a_mask"))
        kw.setdefault("device", dev if dev.type == "cuda" else None)
        if receptor_types is None and infer_meta_data is not None:
            res, names, z, _ = names_from_meta(infer_meta_data)
            if len(res) != int(elements.shape[0]):
                raise ValueError(f"VinaScore: infer_meta_data names {len(res)} atoms, the batch holds {int(elements.shape[0])}")
            receptor_types = receptor_types_from_names(res, names, z)
            kw.setdefault("receptor_typing", "names")
        return VinaScore.from_bonds(elements, bonds, lig, bond_orders=bond_orders, receptor_types=receptor_types, **kw)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernel's tables on `device` (uploaded once)"""
        names = ("types", "ligand_idx", "rec_mask", "lig_active")
        return ops.cached_upload(self._tables, device, lambda up: {k: up(getattr(self, k)) for k in names})

    def score(self, x_pred: torch.Tensor, forces: bool = False) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> dict of device tensors: score [P] (kcal/mol, lower is better), inter [P] (before the division by
        1 + 0.0585 n_rot), terms [P,5] (unweighted, TERM_NAMES order), per_atom [P,L] (the weighted share of each ligand atom; its
        sum over the atoms is inter up to rounding) and, with `forces=True`, forces [P,L,3] = -d inter / d x of the ligand atoms.
        Nothing is read back, nothing synchronises."""
        if x_pred.dim() != 3 or x_pred.shape[1] != self.n_pose_atoms or x_pred.shape[2] != 3:
            raise ValueError(f"VinaScore.score: the tables are over {self.n_pose_atoms} pose atoms, x_pred has shape {tuple(x_pred.shape)}")
        if not 1 <= x_pred.shape[0] <= MAX_POSES:
            raise ValueError(f"VinaScore.score: {x_pred.shape[0]} poses; the kernel takes 1 .. {MAX_POSES}")
        L_ = ops._lib.init()
        x = x_pred.float().contiguous()
        P, A, L = x.shape[0], x.shape[1], self.n_atoms
        t = self.tables(x.device)
        new = lambda *shape: torch.empty(*shape, device=x.device)
        atom_terms, terms, inter, score, per_atom = new(P, L, 5), new(P, 5), new(P), new(P), new(P, L)
        f = new(P, L, 3) if forces else None
        ops.check(L_.pd_vina_score(ops.ptr(x), ops.ptr(t["ligand_idx"]), ops.ptr(t["types"]), ops.ptr(t["rec_mask"]),
                                   ops.ptr(t["lig_active"]), self.n_rot, ops.ptr(atom_terms), ops.ptr(terms), ops.ptr(inter),
                                   ops.ptr(score), ops.ptr(per_atom), ops.ptr(f), P, A, L, ops.stream()), "pd_vina_score")
        out = {"score": score, "inter": inter, "terms": terms, "per_atom": per_atom}
        if forces:
            out["forces"] = f
        return out

    def __repr__(self):
        return (f"VinaScore(n_atoms={self.n_atoms}, n_pose_atoms={self.n_pose_atoms}, receptor_atoms={int(self.rec_mask.sum())}, "
                f"n_rot={self.n_rot:g}, receptor_typing={self.receptor_typing!r})")
