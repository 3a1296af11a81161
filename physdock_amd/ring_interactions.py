"""Does the pose keep the stack with PHE 82?  Pi-stacking, pi-cation and halogen bonds of every pose per residue, on the device
(kernel `pd_plif_rings`, csrc/plif_rings.hip - its header comment holds the same definition, tests/plif_rings_ref.py restates it in
float64 numpy).  These are the kinds `interactions.InteractionFingerprint` leaves out because they need ring centroids and normals;
the conditions and the default thresholds are the published ones of PLIP.

One system: the tables of `InteractionFingerprint` - a ligand of L atoms (`ligand_idx`, `lig_active`), the receptor atoms, a residue
id per atom, one type byte (ACCEPTOR is looked at) and one charge byte (CATION is looked at) per pose atom - and, in addition, rings
and halogens.  A ring is a list of k pose atoms in cyclic order, 3 <= k <= 8 (perception gives 5- and 6-rings); for a pose, in
float64 from the fp32 coordinates,

    centroid  c = (a_0 + ... + a_{k-1}) / k
    normal    N = sum_i (a_i - c) x (a_{i+1} - c), indices mod k;  n = N / |N|

A ring whose N has zero or non-finite length, or that has a non-finite coordinate, is degenerate: it takes part in nothing and
reports n = 0.  The sign of n is never looked at, so nothing depends on where a ring's list starts or which way round it runs.
Bit k of a byte stands for kind k (`RING_KIND_NAMES`):

    bit  kind          between                                   condition (`DEFAULT_RING_THRESHOLDS`)
    0    pi_parallel   ligand ring g, receptor ring h            d = |c_g - c_h| < stack_dist 5.5 A; min(off_gh, off_hg) < stack_offset
                                                                 2.0 A; |n_g . n_h| > cos(parallel_angle 30 deg)
    1    pi_tshaped    the same                                  the same distance and offset; |n_g . n_h| < cos(t_angle 60 deg)
    2    pi_cation     ligand ring g, receptor CATION atom j     |x_j - c_g| < pication_dist 6.0 A; the offset of x_j on the plane of g
                                                                 < pication_offset 2.0 A
    3    cation_pi     ligand CATION atom i, receptor ring h     the same with the roles swapped
    4    halogen_bond  ligand halogen X (Cl, Br, I) with its     |x_X - x_j| < halogen_dist 4.0 A; the angle C - X ... j >=
                       one heavy neighbour C, receptor           halogen_angle 135 deg (= 165 - 30), tested as cos < cos(halogen_angle)
                       ACCEPTOR atom j

off_gh = sqrt(max(0, d^2 - ((c_h - c_g) . n_g)^2)) is the distance from c_g to the projection of c_h onto the plane of g.  Angles are
given in degrees; the host converts them to cosines in double and the kernel compares cosines.  Bits 5 to 7 are always 0.

`fingerprint(x_pred)` returns `bits` uint8 [P,R] (the OR over the residue's rings, cations and acceptors), `ligand_bits` uint8 [P,L]
(a ring's bits go to all of its atoms, a halogen bond to X, cation_pi to the cation; an inactive atom has 0), `ring_bits` uint8
[P,G_l] (per ligand ring), `centroid` and `normal` fp64 [P,G,3] (G = G_l + G_r, the ligand's rings first, the receptor's in ascending
order of their residue: `ring_residue`), `min_centroid_dist` fp32 [P,R] (the smallest ligand-ring to residue-ring centroid distance,
the minimum taken in fp64 and rounded once; +inf when either side has no ring that is not degenerate) and `counts` int32 [P,5].

**Caveats.**  PLIP's thresholds have not been validated on this model's poses.  There is no acceptor-side angle for halogen bonds:
the receptor's bond topology is not known.  Ligand rings are perceived from aromatic bond orders (1.5) - Kekule input has none, give
`ligand_rings=` then.  Receptor rings are those of PHE, TYR, TRP and HIS by atom names; nucleic-acid bases are not perceived.  Metal
coordination and water bridges stay out of scope: the model predicts neither waters nor reliable metal geometry.

`compare`, `pairwise`, `satisfies`, `required_row` and `describe` are those of `InteractionFingerprint`, on ring bytes (the kinds
of `RING_KIND_NAMES`); `combined` joins the two fingerprints; `driver.redock(..., ring_interactions=)` reports the kept poses'.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .interactions import (CATION, MAX_POSES, InteractionFingerprint, _ByteRows, _mask_of, residue_csr,
                           residue_labels_from_meta)
from .scoring import ACCEPTOR, _atomic_numbers, _bond_list, _host, names_from_meta

__all__ = ["RingInteractions", "RING_KIND_NAMES", "RING_THRESHOLD_NAMES", "DEFAULT_RING_THRESHOLDS", "ring_kind_mask",
           "aromatic_rings_from_bonds", "receptor_rings_from_names", "ligand_halogens_from_bonds", "MAX_LIGAND_RINGS",
           "MAX_RECEPTOR_RINGS", "MAX_HALOGENS", "MAX_RING_SIZE"]

#: the five kinds in bit order
RING_KIND_NAMES = ("pi_parallel", "pi_tshaped", "pi_cation", "cation_pi", "halogen_bond")
#: the eight thresholds in the order the kernel takes them - five distances (A), three angles (degrees) - and PLIP's defaults
RING_THRESHOLD_NAMES = ("stack_dist", "stack_offset", "pication_dist", "pication_offset", "halogen_dist", "parallel_angle", "t_angle",
                        "halogen_angle")
DEFAULT_RING_THRESHOLDS = {"stack_dist": 5.5, "stack_offset": 2.0, "pication_dist": 6.0, "pication_offset": 2.0, "halogen_dist": 4.0,
                           "parallel_angle": 30.0, "t_angle": 60.0, "halogen_angle": 135.0}
N_DISTANCES = 5
#: limits of the kernel (csrc/plif_rings.hip) beyond those of `interactions`
MAX_LIGAND_RINGS, MAX_RECEPTOR_RINGS, MAX_HALOGENS, MAX_RING_SIZE = 64, 4096, 64, 8

_RECEPTOR_RINGS = {"PHE": (("CG", "CD1", "CE1", "CZ", "CE2", "CD2"),), "TYR": (("CG", "CD1", "CE1", "CZ", "CE2", "CD2"),),
                   "TRP": (("CD2", "CE2", "CZ2", "CH2", "CZ3", "CE3"), ("CG", "CD1", "NE1", "CE2", "CD2")),
                   "HIS": (("CG", "ND1", "CE1", "NE2", "CD2"),)}
_HALOGENS = (17, 35, 53)


def ring_kind_mask(kinds: Optional[Iterable[str]] = None) -> int:
    """the byte mask of a sequence of ring kind names (default: all five)"""
    return _mask_of(kinds, RING_KIND_NAMES)


def aromatic_rings_from_bonds(n: int, bonds: Iterable[Tuple[int, int]], bond_orders: Sequence[float]) -> List[Tuple[int, ...]]:
    """The rings of 5 or 6 atoms whose bonds all have order 1.5 - the simple cycles of the aromatic subgraph, as
    `validity.planar_groups_from_bonds` perceives them - each in CYCLIC order and canonical: it starts at its smallest atom and steps
    to the smaller of that atom's two ring neighbours.  One ring per cycle of a fused system (naphthalene 2, indole 2); sorted."""
    bonds, orders = _bond_list(int(n), bonds, bond_orders, "aromatic_rings_from_bonds")
    arom = [set() for _ in range(int(n))]
    for (i, j), o in zip(bonds, orders):
        if o == 1.5:
            arom[i].add(j); arom[j].add(i)
    rings = {}

    def walk(path):
        # simple cycles through path[0], its smallest atom; each is met once per direction and kept the way that steps down first
        for nb in sorted(arom[path[-1]]):
            if nb == path[0] and len(path) in (5, 6) and path[1] < path[-1]:
                rings.setdefault(tuple(sorted(path)), tuple(path))
            elif nb > path[0] and nb not in path and len(path) < 6:
                walk(path + [nb])

    for a in range(int(n)):
        walk([a])
    return [rings[k] for k in sorted(rings)]


def receptor_rings_from_names(res_names: Sequence[str], atom_names: Sequence[str], residue_of, mask=None) -> List[Tuple[int, ...]]:
    """The aromatic rings of the receptor by residue and atom names, as tuples of atom indices in cyclic order: PHE and TYR CG CD1 CE1
    CZ CE2 CD2; TRP CD2 CE2 CZ2 CH2 CZ3 CE3 and CG CD1 NE1 CE2 CD2; HIS CG ND1 CE1 NE2 CD2.  Atoms with equal `residue_of` form a
    residue; `mask` [n] (default: all): 0 = the atom does not count.  A ring with a missing or masked atom is dropped."""
    res = _host(residue_of, np.int64).reshape(-1)
    if not len(res_names) == len(atom_names) == res.shape[0]:
        raise ValueError(f"receptor_rings_from_names: {len(res_names)} residue names, {len(atom_names)} atom names, {res.shape[0]} residue ids")
    ok = np.ones(res.shape[0], dtype=bool) if mask is None else _host(mask, np.float64).reshape(-1) > 0
    if ok.shape[0] != res.shape[0]:
        raise ValueError(f"receptor_rings_from_names: {res.shape[0]} atoms, a mask of {ok.shape[0]}")
    by_residue: Dict[int, Dict[str, int]] = {}
    kind: Dict[int, str] = {}
    for a, (r, name) in enumerate(zip(res_names, atom_names)):
        r = str(r).strip().upper()
        if r in _RECEPTOR_RINGS and ok[a]:
            by_residue.setdefault(int(res[a]), {}).setdefault(str(name).strip().upper(), a)
            kind[int(res[a])] = r
    rings = []
    for s in sorted(by_residue):
        for ring in _RECEPTOR_RINGS[kind[s]]:
            if all(name in by_residue[s] for name in ring):
                rings.append(tuple(by_residue[s][name] for name in ring))
    return rings


def ligand_halogens_from_bonds(elements, bonds: Iterable[Tuple[int, int]]) -> List[Tuple[int, int]]:
    """(X, C) pairs of indices into `elements`: every Cl, Br or I with exactly one heavy neighbour, which is a carbon"""
    z = _atomic_numbers(elements)
    bonds, _ = _bond_list(len(z), bonds, None, "ligand_halogens_from_bonds")
    heavy: List[List[int]] = [[] for _ in range(len(z))]
    for i, j in bonds:
        if z[j] != 1:
            heavy[i].append(j)
        if z[i] != 1:
            heavy[j].append(i)
    return [(a, heavy[a][0]) for a in range(len(z)) if z[a] in _HALOGENS and len(heavy[a]) == 1 and z[heavy[a][0]] == 6]


def _ring_thresholds(thresholds) -> Tuple[float, ...]:
    t = dict(DEFAULT_RING_THRESHOLDS)
    if thresholds is None:
        pass
    elif isinstance(thresholds, dict):
        bad = set(thresholds) - set(RING_THRESHOLD_NAMES)
        if bad:
            raise ValueError(f"RingInteractions: unknown thresholds {sorted(bad)}; they are {RING_THRESHOLD_NAMES}")
        t.update(thresholds)
    else:
        vals = list(thresholds)
        if len(vals) != len(RING_THRESHOLD_NAMES):
            raise ValueError(f"RingInteractions: thresholds are {RING_THRESHOLD_NAMES}, got {len(vals)} values")
        t = dict(zip(RING_THRESHOLD_NAMES, vals))
    out = tuple(float(t[k]) for k in RING_THRESHOLD_NAMES)
    if any(not math.isfinite(v) or v < 0 for v in out[:N_DISTANCES]):
        raise ValueError(f"RingInteractions: a distance threshold must be finite and not negative, got {dict(zip(RING_THRESHOLD_NAMES, out))}")
    if any(not 0.0 <= v <= 180.0 for v in out[N_DISTANCES:]):
        raise ValueError(f"RingInteractions: an angle threshold must lie in 0 .. 180 degrees, got {dict(zip(RING_THRESHOLD_NAMES, out))}")
    return out


class RingInteractions(_ByteRows):
    """One system's tables for `pd_plif_rings`: host copies (numpy: `types`, `charges` uint8 [A], `ligand_idx` int32 [L], `lig_active`
    uint8 [L], `rec_mask` uint8 [A], `residue_of` int32 [A], the CSR `res_start` / `res_atom`, the rings `ring_start` int32 [G + 1],
    `ring_atom` int32 (pose atoms), `ring_residue` int32 [G] (-1 for a ligand ring; the receptor's rings ascend in it), `halogens`
    int32 [H,2] (ligand-local X, C)), `thresholds` (dict: A and degrees), `receptor_typing` ("given", "names" or "elements" - with the
    last nothing on the receptor side can fire: no rings, no cations, no acceptors), `residue_labels` and, uploaded once per device,
    what the kernel reads.  `n_atoms` is L, `n_pose_atoms` A, `n_residues` R, `n_receptor_atoms` N, `n_ligand_rings` G_l,
    `n_receptor_rings` G_r, `n_halogens` H."""
    _name = "RingInteractions"
    _kind_names = RING_KIND_NAMES

    def __init__(self, types, charges, ligand_idx, lig_active, rec_mask, residue_of, n_residues, ligand_rings, receptor_rings, halogens,
                 thresholds=None, receptor_typing: str = "given", residue_labels=None, device=None):
        self.types, self.charges, self.ligand_idx, self.lig_active = types, charges, ligand_idx, lig_active
        self.rec_mask, self.residue_of, self.n_residues = rec_mask, residue_of, int(n_residues)
        self.res_start, self.res_atom = residue_csr(residue_of, rec_mask, self.n_residues)
        receptor_rings = sorted(receptor_rings, key=lambda r: int(residue_of[r[0]]))                  # stable: ascending in the residue
        rings = [tuple(r) for r in ligand_rings] + [tuple(r) for r in receptor_rings]
        self.n_ligand_rings, self.n_receptor_rings = len(ligand_rings), len(receptor_rings)
        self.ring_start = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
        self.ring_atom = np.asarray([a for r in rings for a in r], dtype=np.int32)
        self.ring_residue = np.asarray([-1] * len(ligand_rings) + [int(residue_of[r[0]]) for r in receptor_rings], dtype=np.int32)
        self.halogens = np.asarray(halogens, dtype=np.int32).reshape(-1, 2)
        self.n_halogens = int(self.halogens.shape[0])
        self.threshold_values = _ring_thresholds(thresholds)
        self.thresholds = dict(zip(RING_THRESHOLD_NAMES, self.threshold_values))
        self.receptor_typing = receptor_typing
        self.residue_labels = None if residue_labels is None else [str(s) for s in residue_labels]
        if self.residue_labels is not None and len(self.residue_labels) != self.n_residues:
            raise ValueError(f"RingInteractions: {len(self.residue_labels)} residue labels for {self.n_residues} residues")
        self.n_atoms, self.n_pose_atoms, self.n_receptor_atoms = int(ligand_idx.shape[0]), int(types.shape[0]), int(self.res_atom.shape[0])
        # what the kernel takes: the distances as they are, the angles as cosines, converted in double
        self._thr = (C.c_double * len(RING_THRESHOLD_NAMES))(*self.threshold_values[:N_DISTANCES],
                                                            *[math.cos(math.radians(v)) for v in self.threshold_values[N_DISTANCES:]])
        self._tables = {}
        if device is not None:
            self.tables(device)

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_tables(types, charges, ligand_idx, receptor_mask, residue_of, ligand_rings=(), receptor_rings=(), halogens=(),
                    n_residues: Optional[int] = None, a_mask=None, ligand_active=None, thresholds=None, residue_labels=None,
                    receptor_typing: str = "given", device=None):
        """Everything is given.  types, charges, ligand_idx, receptor_mask, residue_of, n_residues, a_mask, ligand_active,
        residue_labels: as `InteractionFingerprint.from_types` takes them (ACCEPTOR of a type byte and CATION of a charge byte are
        looked at).  ligand_rings: rings as sequences of LOCAL ligand indices (position in `ligand_idx`) in cyclic order;
        receptor_rings: rings as sequences of pose-atom indices in cyclic order, each inside one residue and made of receptor atoms;
        halogens: (X, C) pairs of local ligand indices.  thresholds: a dict over `RING_THRESHOLD_NAMES` (missing ones keep their
        default) or eight values in that order, distances in A and angles in degrees."""
        base = InteractionFingerprint.from_types(types, charges, ligand_idx, receptor_mask, residue_of, n_residues=n_residues, a_mask=a_mask,
                                                 ligand_active=ligand_active, residue_labels=residue_labels)
        L, A = base.n_atoms, base.n_pose_atoms

        def ring_list(rings, limit, what, n):
            out = []
            for r in rings:
                r = tuple(int(a) for a in (r.tolist() if hasattr(r, "tolist") else r))
                if not 3 <= len(r) <= MAX_RING_SIZE or len(set(r)) != len(r) or min(r) < 0 or max(r) >= n:
                    raise ValueError(f"RingInteractions: a {what} ring holds 3 .. {MAX_RING_SIZE} distinct atom indices below {n}, got {r}")
                out.append(r)
            if len(out) > limit:
                raise ValueError(f"RingInteractions: {len(out)} {what} rings; the kernel takes at most {limit}")
            return out

        lig_rings = [tuple(int(base.ligand_idx[i]) for i in r) for r in ring_list(ligand_rings, MAX_LIGAND_RINGS, "ligand", L)]
        rec_rings = ring_list(receptor_rings, MAX_RECEPTOR_RINGS, "receptor", A)
        for r in rec_rings:
            if not all(base.rec_mask[a] for a in r) or len({int(base.residue_of[a]) for a in r}) != 1:
                raise ValueError(f"RingInteractions: a receptor ring lies inside one residue and is made of receptor atoms, got {r}")
        hal = [(int(x), int(c)) for x, c in (halogens.tolist() if hasattr(halogens, "tolist") else halogens)]
        if len(hal) > MAX_HALOGENS or any(not (0 <= x < L and 0 <= c < L) or x == c for x, c in hal):
            raise ValueError(f"RingInteractions: halogens are at most {MAX_HALOGENS} pairs (X, C) of distinct ligand indices below {L}")
        return RingInteractions(base.types, base.charges, base.ligand_idx, base.lig_active, base.rec_mask, base.residue_of, base.n_residues,
                                lig_rings, rec_rings, hal, thresholds, receptor_typing, residue_labels, device)

    @staticmethod
    def from_bonds(elements, bonds, ligand_idx, residue_of, bond_orders=None, receptor_types=None, receptor_charges=None,
                   receptor_rings=(), ligand_rings=None, n_residues: Optional[int] = None, a_mask=None, n_hydrogens=None,
                   formal_charges=None, thresholds=None, residue_labels=None, receptor_typing: Optional[str] = None, device=None):
        """elements, bonds (pairs of LOCAL ligand indices), ligand_idx, residue_of, bond_orders, receptor_types, receptor_charges and
        the other keywords: as `InteractionFingerprint.from_bonds` takes them - the ligand's types and charges are made the same way.
        The ligand's rings are `aromatic_rings_from_bonds` (none without bond orders) unless `ligand_rings=` gives them (local
        indices - the way in for Kekule input), its halogens `ligand_halogens_from_bonds`; `receptor_rings` (pose-atom indices, e.g.
        `receptor_rings_from_names`) are taken as given.  Without `receptor_types` the receptor is typed by element alone
        (`receptor_typing` "elements"): no cations, no acceptors."""
        base = InteractionFingerprint.from_bonds(elements, bonds, ligand_idx, residue_of, bond_orders=bond_orders, receptor_types=receptor_types,
                                                 receptor_charges=receptor_charges, n_residues=n_residues, a_mask=a_mask, n_hydrogens=n_hydrogens,
                                                 formal_charges=formal_charges, residue_labels=residue_labels, receptor_typing=receptor_typing)
        z = _atomic_numbers(elements)
        L = base.n_atoms
        if ligand_rings is None:
            ligand_rings = aromatic_rings_from_bonds(L, bonds, bond_orders) if bond_orders is not None else []
        exists = base.lig_active > 0                                  # a ring or a halogen with an atom that does not exist is dropped
        ligand_rings = [r for r in ligand_rings if all(0 <= int(i) < L and exists[int(i)] for i in r)]
        halogens = [(x, c) for x, c in ligand_halogens_from_bonds(z[base.ligand_idx], bonds) if exists[x] and exists[c]]
        return RingInteractions.from_tables(base.types, base.charges, base.ligand_idx, base.rec_mask, base.residue_of, ligand_rings=ligand_rings,
                                            receptor_rings=receptor_rings, halogens=halogens, n_residues=base.n_residues,
                                            ligand_active=base.lig_active, thresholds=thresholds, residue_labels=residue_labels,
                                            receptor_typing=base.receptor_typing, device=device)

    @staticmethod
    def from_batch(batch, bonds, bond_orders=None, infer_meta_data=None, thresholds=None, receptor_types=None, receptor_charges=None,
                   receptor_rings=None, **kw):
        """from a feature dict, as `InteractionFingerprint.from_batch`: a residue is a token, the tables are uploaded to the batch's
        device.  With `infer_meta_data` (the loader's naming tables) the receptor's types, charges, rings (`receptor_rings_from_names`)
        and residue labels come from the names; without it, and without `receptor_types` / `receptor_charges` / `receptor_rings`, the
        receptor has no rings, cations or acceptors - `receptor_typing` "elements" records that nothing on the receptor side can
        fire.  Other keywords as for `from_bonds`."""
        from .driver import ligand_atom_mask
        from .interactions import receptor_charges_from_names
        from .scoring import receptor_types_from_names
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
                raise ValueError(f"RingInteractions: infer_meta_data names {len(res)} atoms, the batch holds {int(elements.shape[0])}")
            if receptor_types is None:
                receptor_types = receptor_types_from_names(res, names, z)
                if receptor_charges is None:
                    receptor_charges = receptor_charges_from_names(res, names)
                kw.setdefault("receptor_typing", "names")
            if receptor_rings is None:
                mask = (z != 1) & (np.ones(len(z), dtype=bool) if kw["a_mask"] is None else _host(kw["a_mask"], np.float64).reshape(-1) > 0)
                mask[_host(lig, np.int64)] = False
                receptor_rings = receptor_rings_from_names(res, names, _host(residue_of, np.int64), mask)
            kw.setdefault("residue_labels", residue_labels_from_meta(infer_meta_data, _host(residue_of, np.int64), kw["n_residues"]))
        return RingInteractions.from_bonds(elements, bonds, lig, residue_of, bond_orders=bond_orders, receptor_types=receptor_types,
                                           receptor_charges=receptor_charges, receptor_rings=receptor_rings or (), thresholds=thresholds, **kw)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernel's tables on `device` (uploaded once)"""
        names = ("types", "charges", "ligand_idx", "lig_active", "res_start", "res_atom", "ring_start", "ring_atom", "ring_residue", "halogens")
        return ops.cached_upload(self._tables, device, lambda up: {k: up(getattr(self, k)) for k in names})

    def fingerprint(self, x_pred: torch.Tensor) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> dict of device tensors: bits uint8 [P,R] (bit k = kind k of `RING_KIND_NAMES` between the ligand
        and the residue), ligand_bits uint8 [P,L], ring_bits uint8 [P,G_l], centroid and normal fp64 [P,G,3] (the ligand's rings
        first; a degenerate ring has the normal 0), min_centroid_dist fp32 [P,R] (+inf where the ligand or the residue has no ring)
        and counts int32 [P,5] (residues per kind).  Nothing is read back, nothing synchronises."""
        if x_pred.dim() != 3 or x_pred.shape[1] != self.n_pose_atoms or x_pred.shape[2] != 3:
            raise ValueError(f"RingInteractions.fingerprint: the tables are over {self.n_pose_atoms} pose atoms, x_pred has shape "
                             f"{tuple(x_pred.shape)}")
        if not 1 <= x_pred.shape[0] <= MAX_POSES:
            raise ValueError(f"RingInteractions.fingerprint: {x_pred.shape[0]} poses; the kernel takes 1 .. {MAX_POSES}")
        L_ = ops._lib.init()
        x = x_pred.float().contiguous()
        P, A, L, R, N = x.shape[0], x.shape[1], self.n_atoms, self.n_residues, self.n_receptor_atoms
        Gl, Gr, H = self.n_ligand_rings, self.n_receptor_rings, self.n_halogens
        t = self.tables(x.device)
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=x.device)
        nbytes = L_.pd_plif_rings_workspace(P, L, N, Gl, Gr, H)
        ops.check(min(nbytes, 0), "pd_plif_rings_workspace")
        ws = new((nbytes // 8,), torch.float64)
        bits, ligand_bits, ring_bits = new((P, R), torch.uint8), new((P, L), torch.uint8), new((P, Gl), torch.uint8)
        centroid, normal = new((P, Gl + Gr, 3), torch.float64), new((P, Gl + Gr, 3), torch.float64)
        min_dist, counts = new((P, R), torch.float32), new((P, len(RING_KIND_NAMES)), torch.int32)
        opt = lambda tensor, n: ops.ptr(tensor) if n else None
        ops.check(L_.pd_plif_rings(ops.ptr(x), ops.ptr(t["ligand_idx"]), ops.ptr(t["types"]), ops.ptr(t["charges"]), ops.ptr(t["lig_active"]),
                                   ops.ptr(t["res_start"]), opt(t["res_atom"], N), opt(t["ring_start"], Gl + Gr), opt(t["ring_atom"], Gl + Gr),
                                   opt(t["ring_residue"], Gl + Gr), Gl, Gr, opt(t["halogens"], H), H, self._thr, ops.ptr(ws), nbytes,
                                   ops.ptr(bits), ops.ptr(ligand_bits), opt(ring_bits, Gl), opt(centroid, Gl + Gr), opt(normal, Gl + Gr),
                                   ops.ptr(min_dist), ops.ptr(counts), P, A, L, R, N, ops.stream()), "pd_plif_rings")
        return {"bits": bits, "ligand_bits": ligand_bits, "ring_bits": ring_bits, "centroid": centroid, "normal": normal,
                "min_centroid_dist": min_dist, "counts": counts}

    @staticmethod
    def combined(bits6: torch.Tensor, ring_bits: torch.Tensor) -> torch.Tensor:
        """`torch.cat([bits6, ring_bits], 1)` uint8 [P, 2R]: the `bits` of `InteractionFingerprint.fingerprint` and of `fingerprint`
        for the same poses side by side.  Popcounts add over the columns, so `pairwise` / `compare` of either class on the combined
        rows (`InteractionFingerprint.from_types(...)` over 2R residues, or `pd_plif_pairwise` directly, with every bit in the mask:
        the six kinds use bits 0 - 5, the ring kinds 0 - 4, so masks below 64 fit) give the Tanimoto over all eleven kinds."""
        if (not isinstance(bits6, torch.Tensor) or not isinstance(ring_bits, torch.Tensor) or bits6.dtype != torch.uint8 or
                ring_bits.dtype != torch.uint8 or bits6.dim() != 2 or bits6.shape != ring_bits.shape):
            raise ValueError("RingInteractions.combined: two uint8 tensors [P,R] of one shape, the `bits` of the two fingerprints")
        return torch.cat([bits6, ring_bits], 1)

    def pairwise_combined(self, bits6: torch.Tensor, ring_bits: torch.Tensor) -> torch.Tensor:
        """tanimoto fp32 [P,P] over all eleven kinds: `pd_plif_pairwise` on `combined(bits6, ring_bits)`"""
        self._bits(bits6, "pairwise_combined"), self._bits(ring_bits, "pairwise_combined")
        rows = self.combined(bits6, ring_bits).contiguous()
        L_ = ops._lib.init()
        P, R2 = rows.shape
        out = torch.empty((P, P), dtype=torch.float32, device=rows.device)
        ops.check(L_.pd_plif_pairwise(ops.ptr(rows), 63, ops.ptr(out), P, R2, ops.stream()), "pd_plif_pairwise")
        return out

    def __repr__(self):
        return (f"RingInteractions(n_atoms={self.n_atoms}, n_pose_atoms={self.n_pose_atoms}, residues={self.n_residues}, "
                f"receptor_atoms={self.n_receptor_atoms}, ligand_rings={self.n_ligand_rings}, receptor_rings={self.n_receptor_rings}, "
                f"halogens={self.n_halogens}, receptor_typing={self.receptor_typing!r}, thresholds={self.thresholds})")
