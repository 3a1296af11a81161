"""How much of the ligand is inside the protein, and which residues form the pocket wall?  Solvent-accessible surface area (SASA,
Shrake & Rupley 1973) of every pose on the device: the ligand's area free and in the complex, the buried fraction, the polar /
apolar split of what is buried, and the area each residue loses to the ligand (kernel `pd_buried_surface`, csrc/sasa.hip - its header
comment holds the same definition).

One system, over the A atoms of a pose: `cls [A]`, one byte per atom - 0 ignored (padding, `a_mask == 0`, an inactive ligand atom,
a hydrogen), 1 receptor, 2 ligand; `radius [A]` in fp32; `probe` (1.4 A by default); `unit [n,3]`, n unit vectors
(`sphere_points(n)`, the golden spiral computed in float64 and rounded to fp32):

    t = k + 0.5,  z = 1 - 2 t / n,  phi = t pi (3 - sqrt 5),  u_k = (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z),  0 <= k < n

The default n is 96, n = 960 is the "publication" setting, any n in 1 .. 1024 is accepted.  The default radii are
`validity.VDW_RADII` / `validity.DEFAULT_RADIUS` by element (the package has one radius table); `radii={Z: r}` overrides them.

For pose p and atom i of class c != 0, with R_i = radius_i + probe:

    the point    p_ik = x_i + R_i u_k
    atom j covers it iff j != i (by index, not by distance), cls_j != 0 and |p_ik - x_j| < R_j
    same_k       any covering j has class c;      other_k    any covering j has the other class
    n_free[i]    = #{k : !same_k}                 the exposure within the atom's own molecule
    n_bound[i]   = #{k : !same_k && !other_k}     the exposure in the complex
    n_buried[i]  = n_free[i] - n_bound[i]
    an atom's area per point is 4 pi R_i^2 / n

`measure(x_pred [P,A,3])` returns device tensors, nothing is read back: `free_points int32 [P,L]` (ligand atoms in `ligand_idx`
order, 0 for an inactive one), `buried_points int32 [P,A]` (every atom; 0 for an ignored atom and for a receptor atom no ligand atom
can reach), `per_atom [P,L]` (buried area of each ligand atom), `ligand_free`, `ligand_bound`, `ligand_buried [P]` (A^2),
`buried_fraction [P]` = ligand_buried / ligand_free (0 where ligand_free is 0, never NaN), `buried_polar`, `buried_apolar [P]`
(ligand_buried split by the `polar [L]` byte: element N or O by default), `receptor_buried [P]`, `interface_area [P]` =
(ligand_buried + receptor_buried) / 2, `residue_buried [P,R]` (the area each residue loses to the ligand; a residue is a token in
`from_batch`) and `interface_residues int32 [P]` (residues with residue_buried > 0).

Counts are integers built from "any"; every float is a sum in a fixed ascending order of atoms: a pose's values are bit-identical
whatever the number of poses in the call and wherever the pose sits.

**Two caveats.**  The model predicts no hydrogens - heavy atoms only -, so absolute areas are NOT comparable with all-atom
tools (FreeSASA, PISA, NACCESS on protonated structures); compare poses of one system with each other.  The radii, the probe and
the polar default are THIS PACKAGE'S DEFAULTS AND HAVE NOT BEEN VALIDATED on real complexes.  Out of scope: solvent-excluded
(Connolly) surfaces, solvation energies, gradients of the area, ranking by burial.

`BuriedSurface` holds one system's tables, built once on the host; `driver.redock(..., surface=)` reports the measure of the kept
poses and of the ground truth.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .interactions import residue_csr, residue_labels_from_meta
from .scoring import _atomic_numbers, _host
from .validity import DEFAULT_RADIUS, VDW_RADII

__all__ = ["BuriedSurface", "sphere_points", "DEFAULT_PROBE", "DEFAULT_POINTS", "MAX_POINTS", "MAX_ATOMS", "MAX_POSE_ATOMS",
           "MAX_POSES", "TOTAL_NAMES", "IGNORED", "RECEPTOR", "LIGAND"]

#: probe radius (A) and number of points per atom unless given; the largest number of points the kernel takes
DEFAULT_PROBE, DEFAULT_POINTS, MAX_POINTS = 1.4, 96, 1024
#: limits of the kernel (csrc/sasa.hip): ligand atoms, pose atoms, poses; and R <= A
MAX_ATOMS, MAX_POSE_ATOMS, MAX_POSES = 1024, 1 << 22, 65535
#: the rows of the kernel's `totals [8,P]` in order
TOTAL_NAMES = ("ligand_free", "ligand_bound", "ligand_buried", "buried_fraction", "buried_polar", "buried_apolar", "receptor_buried",
               "interface_area")
#: values of a class byte
IGNORED, RECEPTOR, LIGAND = 0, 1, 2


def sphere_points(n: int) -> np.ndarray:
    """fp32 [n,3]: the n unit vectors of the golden spiral (module docstring), computed in float64 and rounded once"""
    n = int(n)
    if not 1 <= n <= MAX_POINTS:
        raise ValueError(f"sphere_points: {n} points; the kernel takes 1 .. {MAX_POINTS}")
    t = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * t / n
    phi = t * (math.pi * (3.0 - math.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], -1).astype(np.float32)


class BuriedSurface:
    """One system's tables for `pd_buried_surface`: host copies (numpy: `cls` uint8 [A], `radius` fp32 [A], `ligand_idx` int32 [L],
    `polar` uint8 [L], `unit` fp32 [n,3], `residue_of` int32 [A], the CSR `res_start` int32 [R + 1] / `res_atom` int32 [N] of the
    receptor atoms), `probe`, `n_points`, `residue_labels` (a name per residue, or None) and, uploaded once per device, what the
    kernel reads.  `n_atoms` is the ligand's atom count L, `n_pose_atoms` the A of the poses `measure` takes, `n_residues` R,
    `n_receptor_atoms` N."""

    def __init__(self, cls, radius, ligand_idx, polar, residue_of, n_residues, probe=DEFAULT_PROBE, n_points=DEFAULT_POINTS,
                 residue_labels=None, device=None):
        self.cls, self.radius, self.ligand_idx, self.polar = cls, radius, ligand_idx, polar
        self.residue_of, self.n_residues = residue_of, int(n_residues)
        self.probe, self.n_points = float(probe), int(n_points)
        self.unit = sphere_points(self.n_points)
        self.res_start, self.res_atom = residue_csr(residue_of, cls == RECEPTOR, self.n_residues)
        self.residue_labels = None if residue_labels is None else [str(s) for s in residue_labels]
        if self.residue_labels is not None and len(self.residue_labels) != self.n_residues:
            raise ValueError(f"BuriedSurface: {len(self.residue_labels)} residue labels for {self.n_residues} residues")
        self.n_atoms, self.n_pose_atoms, self.n_receptor_atoms = int(ligand_idx.shape[0]), int(cls.shape[0]), int(self.res_atom.shape[0])
        self._tables = {}
        if device is not None:
            self.tables(device)

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_arrays(elements, ligand_idx, receptor_mask, residue_of, n_residues: Optional[int] = None, a_mask=None, ligand_active=None,
                    polar=None, probe: float = DEFAULT_PROBE, n_points: int = DEFAULT_POINTS, radii=None, radius=None,
                    residue_labels=None, device=None):
        """elements: atomic numbers (or symbols) of all A pose atoms - they give the radii (`validity.VDW_RADII`, `radii={Z: r}`
        overrides single elements), the polar default (N or O) and leave hydrogens out on both sides; or None with `radius=` fp32 [A]
        and `polar=` given explicitly.  ligand_idx [L]: the ligand's atoms in a pose; receptor_mask [A] (> 0: the atom counts as
        receptor; ligand atoms never do); residue_of [A]: the residue id of every atom; n_residues (default: the largest id + 1);
        a_mask [A] (default: every atom exists); ligand_active [L] (default: all): 0 = the ligand atom is ignored; polar [L]: 1 =
        the ligand atom's buried area counts as polar; probe (A) and n_points (1 .. 1024)."""
        lig = _host(ligand_idx, np.int64).reshape(-1)
        res = _host(residue_of, np.int64).reshape(-1)
        rec = _host(receptor_mask, np.float64).reshape(-1) > 0
        A, L = int(rec.shape[0]), int(lig.shape[0])
        if A < 1 or A > MAX_POSE_ATOMS or not 1 <= L <= MAX_ATOMS:
            raise ValueError(f"BuriedSurface: {L} ligand atoms of {A}; the kernel takes 1 .. {MAX_ATOMS} of up to {MAX_POSE_ATOMS}")
        if lig.min() < 0 or lig.max() >= A or len(set(lig.tolist())) != L:
            raise ValueError(f"BuriedSurface: ligand_idx must hold {L} distinct atom indices below {A}")
        if not 1 <= int(n_points) <= MAX_POINTS:
            raise ValueError(f"BuriedSurface: n_points = {n_points}; the kernel takes 1 .. {MAX_POINTS}")
        if not (math.isfinite(float(probe)) and float(probe) >= 0):
            raise ValueError(f"BuriedSurface: the probe radius must be finite and not negative, got {probe}")
        z = None if elements is None else _atomic_numbers(elements)
        if z is None and radius is None:
            raise ValueError("BuriedSurface: give elements or radius=")
        if z is not None and z.shape[0] != A:
            raise ValueError(f"BuriedSurface: receptor_mask is given for {A} atoms, elements for {z.shape[0]}")
        if radius is not None:
            if radii is not None:
                raise ValueError("BuriedSurface: radii= overrides the element table; it cannot be combined with radius=")
            rad = _host(radius, np.float64).reshape(-1)
            if rad.shape[0] != A:
                raise ValueError(f"BuriedSurface: receptor_mask is given for {A} atoms, radius for {rad.shape[0]}")
        else:
            table = dict(VDW_RADII)
            table.update({int(k): float(r) for k, r in (radii or {}).items()})
            rad = np.asarray([table.get(int(e), DEFAULT_RADIUS) for e in z], dtype=np.float64)
        if not (np.isfinite(rad).all() and (rad > 0).all()):
            raise ValueError("BuriedSurface: radii must be finite and positive")
        am = np.ones(A, dtype=bool) if a_mask is None else _host(a_mask, np.float64).reshape(-1) > 0
        act = np.ones(L, dtype=bool) if ligand_active is None else _host(ligand_active, np.float64).reshape(-1) > 0
        if am.shape[0] != A or act.shape[0] != L or res.shape[0] != A:
            raise ValueError(f"BuriedSurface: receptor_mask is given for {A} atoms and ligand_idx for {L}; a_mask {am.shape[0]}, "
                             f"ligand_active {act.shape[0]}, residue_of {res.shape[0]}")
        if polar is None:
            if z is None:
                raise ValueError("BuriedSurface: without elements the polar bytes must be given (polar=)")
            pol = (z[lig] == 7) | (z[lig] == 8)
        else:
            pol = _host(polar, np.float64).reshape(-1) > 0
            if pol.shape[0] != L:
                raise ValueError(f"BuriedSurface: ligand_idx holds {L} atoms, polar {pol.shape[0]}")
        R = int(res.max()) + 1 if n_residues is None else int(n_residues)
        if res.min() < 0 or res.max() >= R or R < 1:
            raise ValueError(f"BuriedSurface: residue_of must lie in 0 .. {R - 1}")
        if R > A:
            raise ValueError(f"BuriedSurface: {R} residues of {A} atoms; the kernel takes at most one residue per atom")
        heavy = np.ones(A, dtype=bool) if z is None else z != 1
        cls = np.where(rec & am & heavy, RECEPTOR, IGNORED).astype(np.uint8)
        cls[lig] = np.where(act & am[lig] & heavy[lig], LIGAND, IGNORED)
        return BuriedSurface(cls, rad.astype(np.float32), lig.astype(np.int32), pol.astype(np.uint8), res.astype(np.int32), R, probe,
                             n_points, residue_labels, device)

    @staticmethod
    def from_batch(batch, infer_meta_data=None, **kw):
        """from a feature dict: the ligand's atoms are those of `driver.ligand_atom_mask`, every other atom is receptor, the elements
        come from the one-hot `ref_feat[:, 4:132]` (index = atomic number - 1), `a_mask` from the batch (when it has one), a residue
        is a token (`atom_id_to_token_id`; R = T, the ligand's tokens own no receptor atom); with `infer_meta_data` (the loader's
        naming tables) the residues are labelled (`interactions.residue_labels_from_meta`).  The tables are uploaded to the batch's
        device.  Other keywords as for `from_arrays`."""
        from .driver import ligand_atom_mask
        lig = torch.nonzero(ligand_atom_mask(batch)).flatten()
        elements = batch["ref_feat"][:, 4:132].argmax(-1) + 1
        dev = batch["ref_feat"].device
        residue_of = batch["atom_id_to_token_id"].long()
        kw.setdefault("a_mask", batch.get("a_mask"))
        kw.setdefault("device", dev if dev.type == "cuda" else None)
        kw.setdefault("n_residues", int(batch["is_ligand"].shape[0]))
        if infer_meta_data is not None:
            kw.setdefault("residue_labels", residue_labels_from_meta(infer_meta_data, _host(residue_of, np.int64), kw["n_residues"]))
        return BuriedSurface.from_arrays(elements, lig, np.ones(int(elements.shape[0])), residue_of, **kw)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernel's tables on `device` (uploaded once)"""
        names = ("cls", "radius", "unit", "ligand_idx", "polar", "res_start", "res_atom")
        return ops.cached_upload(self._tables, device, lambda up: {k: up(getattr(self, k)) for k in names})

    def measure(self, x_pred: torch.Tensor) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> dict of device tensors: free_points int32 [P,L], buried_points int32 [P,A], per_atom fp32 [P,L],
        ligand_free, ligand_bound, ligand_buried, buried_fraction, buried_polar, buried_apolar, receptor_buried, interface_area
        fp32 [P] (A^2; the fraction is 0 where ligand_free is 0), residue_buried fp32 [P,R] and interface_residues int32 [P] (module
        docstring).  Nothing is read back, nothing synchronises."""
        if x_pred.dim() != 3 or x_pred.shape[1] != self.n_pose_atoms or x_pred.shape[2] != 3:
            raise ValueError(f"BuriedSurface.measure: the tables are over {self.n_pose_atoms} pose atoms, x_pred has shape "
                             f"{tuple(x_pred.shape)}")
        if not 1 <= x_pred.shape[0] <= MAX_POSES:
            raise ValueError(f"BuriedSurface.measure: {x_pred.shape[0]} poses; the kernel takes 1 .. {MAX_POSES}")
        L_ = ops._lib.init()
        x = x_pred.float().contiguous()
        P, A, L, R, N = x.shape[0], x.shape[1], self.n_atoms, self.n_residues, self.n_receptor_atoms
        t = self.tables(x.device)
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=x.device)
        ws_free, free_points, buried_points = new((P, A), torch.int32), new((P, L), torch.int32), new((P, A), torch.int32)
        per_atom, totals, residue_buried = new((P, L), torch.float32), new((len(TOTAL_NAMES), P), torch.float32), new((P, R), torch.float32)
        interface_residues = new((P,), torch.int32)
        ops.check(L_.pd_buried_surface(ops.ptr(x), ops.ptr(t["cls"]), ops.ptr(t["radius"]), ops.ptr(t["unit"]), ops.ptr(t["ligand_idx"]),
                                       ops.ptr(t["polar"]), ops.ptr(t["res_start"]), ops.ptr(t["res_atom"]) if N else None, self.probe,
                                       ops.ptr(ws_free), ops.ptr(free_points), ops.ptr(buried_points), ops.ptr(per_atom), ops.ptr(totals),
                                       ops.ptr(residue_buried), ops.ptr(interface_residues), P, A, L, R, N, self.n_points, ops.stream()),
                  "pd_buried_surface")
        out = {"free_points": free_points, "buried_points": buried_points, "per_atom": per_atom}
        out.update({k: totals[i] for i, k in enumerate(TOTAL_NAMES)})
        out.update(residue_buried=residue_buried, interface_residues=interface_residues)
        return out

    def describe(self, residue_buried_row, min_area: float = 0.0) -> List[Tuple[object, float]]:
        """host helper: one row [R] of `residue_buried` (a tensor is read back) -> [(residue label or id, area)] of the residues that
        lose more than `min_area` A^2 to the ligand, the largest area first (residue order among equal areas)"""
        row = np.asarray(residue_buried_row.detach().cpu() if isinstance(residue_buried_row, torch.Tensor) else residue_buried_row,
                         dtype=np.float64).reshape(-1)
        if row.shape[0] != self.n_residues:
            raise ValueError(f"BuriedSurface.describe: a row holds {self.n_residues} areas, got {row.shape[0]}")
        label = (lambda s: self.residue_labels[s] or s) if self.residue_labels is not None else (lambda s: s)
        keep = [int(s) for s in np.nonzero(row > float(min_area))[0]]
        return [(label(s), float(row[s])) for s in sorted(keep, key=lambda s: (-row[s], s))]

    def __repr__(self):
        return (f"BuriedSurface(n_atoms={self.n_atoms}, n_pose_atoms={self.n_pose_atoms}, residues={self.n_residues}, "
                f"receptor_atoms={self.n_receptor_atoms}, active_ligand_atoms={int((self.cls == LIGAND).sum())}, probe={self.probe}, "
                f"n_points={self.n_points})")
