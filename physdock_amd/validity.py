"""Is a pose physically sensible?  PoseBusters-style geometry checks of every sampled pose on the device (kernel `pd_pose_validity`).

The reference answers the question after sampling with the `posebusters` package, on the host and through files
(PhysDock/data/relaxation.py:24-50).  Here the checks that need only geometry run for a whole batch of poses in one call:

  bit 0  bond_lengths     a bond is shorter than 0.75 or longer than 1.25 times its length in the reference conformer
  bit 1  bond_angles      the same for the distance between two atoms bonded to a common atom (a 1-3 distance pins the angle)
  bit 2  internal_clash   two ligand atoms four or more bonds apart (or of different fragments) are closer than 0.7 times the
                          sum of their van der Waals radii
  bit 3  receptor_clash   a ligand atom is closer to a receptor atom than 0.75 times the sum of their van der Waals radii
  bit 4  planarity        an atom of an aromatic ring or of a double bond's surroundings is more than 0.25 A off the group's
                          least-squares plane
  bit 5  detached         no ligand atom is within 8 A of a receptor atom

Bits 0, 1, 3 and 4 use PoseBusters' published defaults.  PoseBusters bounds the internal clash by RDKit's distance-geometry lower
bounds, which are not available here: 0.7 times the van der Waals sum is a stand-in, and the 8 A of bit 5 is this package's own.
**These two defaults have not been validated on real complexes.**  Out of scope: volume overlap, the energy ratio, anything
that needs RDKit.

`PoseValidity` holds one ligand's tables, built once on the host from the bond graph, a reference conformer and the elements -
like `ChiralityReference` and `LigandSymmetry`.  `check(x_pred)` returns device tensors and never synchronises;
`driver.redock(..., validity=, validity_filter=)` reports it for the kept poses and can reject failing poses where the chirality
test does.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import ValidityThresholds
from .mmff import _topological_distances

__all__ = ["PoseValidity", "CHECK_NAMES", "DEFAULT_THRESHOLDS", "VDW_RADII", "planar_groups_from_bonds", "MAX_ATOMS", "MAX_GROUPS",
           "GROUP_WIDTH", "REC_TILE"]

#: limits of the kernel (csrc/validity.hip); REC_TILE pose atoms share a block of its receptor pass
MAX_ATOMS, MAX_GROUPS, GROUP_WIDTH, MAX_POSE_ATOMS, REC_TILE = 1024, 256, 8, 1 << 22, 256
#: failed-check names in flag-bit order
CHECK_NAMES = ("bond_lengths", "bond_angles", "internal_clash", "receptor_clash", "planarity", "detached")
#: field order of pd_validity_thresholds
DEFAULT_THRESHOLDS = {"bond_lo": 0.75, "bond_hi": 1.25, "angle_lo": 0.75, "angle_hi": 1.25, "internal_clash": 0.7,
                      "receptor_clash": 0.75, "planarity": 0.25, "detached": 8.0}
#: van der Waals radii (A) by atomic number; any other element takes DEFAULT_RADIUS
VDW_RADII = {1: 1.2, 6: 1.7, 7: 1.6, 8: 1.55, 9: 1.5, 15: 1.95, 16: 1.8, 17: 1.8, 35: 1.9, 53: 2.1}
DEFAULT_RADIUS = 2.0


def planar_groups_from_bonds(n_atoms: int, bonds: Iterable[Tuple[int, int]], bond_orders: Sequence[float]):
    """The atom groups that must be flat, as sorted tuples in a deterministic order: every ring of 5 or 6 atoms whose bonds all
    have order 1.5, then for every order-2 bond between two atoms of degree <= 3 the two atoms plus their neighbours (groups of
    fewer than four atoms define no test and are left out)."""
    bonds = [(int(i), int(j)) for i, j in bonds]
    orders = [float(o) for o in bond_orders]
    if len(orders) != len(bonds):
        raise ValueError(f"planar_groups_from_bonds: {len(bonds)} bonds but {len(orders)} bond orders")
    adj = [set() for _ in range(n_atoms)]
    arom = [set() for _ in range(n_atoms)]
    for (i, j), o in zip(bonds, orders):
        adj[i].add(j); adj[j].add(i)
        if o == 1.5:
            arom[i].add(j); arom[j].add(i)
    rings = set()

    def walk(path):
        # simple cycles of the aromatic subgraph through path[0], its smallest atom
        for nb in sorted(arom[path[-1]]):
            if nb == path[0] and len(path) in (5, 6):
                rings.add(tuple(sorted(path)))
            elif nb > path[0] and nb not in path and len(path) < 6:
                walk(path + [nb])

    for a in range(n_atoms):
        walk([a])
    groups = sorted(rings)
    for (i, j), o in zip(bonds, orders):
        if o == 2.0 and len(adj[i]) <= 3 and len(adj[j]) <= 3:
            g = tuple(sorted({i, j} | adj[i] | adj[j]))
            if len(g) >= 4 and g not in groups:
                groups.append(g)
    return groups


class PoseValidity:
    """One ligand's tables for `pd_pose_validity`: host copies (numpy: `ligand_idx`, `radius`, `rec_mask`, `lig_active`, `pair12`,
    `d12_ref`, `pair13`, `d13_ref`, `far`, `planar`, `thresholds`) and, uploaded once per device, what the kernel reads.
    `n_atoms` is the ligand's atom count L, `n_pose_atoms` the A of the poses `check` takes."""

    def __init__(self, tables: Dict[str, np.ndarray], thresholds: Optional[dict] = None, device=None):
        self.__dict__.update(tables)
        self.n_atoms, self.n_pose_atoms = int(self.ligand_idx.shape[0]), int(self.radius.shape[0])
        self.thresholds = dict(DEFAULT_THRESHOLDS)
        unknown = set(thresholds or {}) - set(DEFAULT_THRESHOLDS)
        if unknown:
            raise ValueError(f"PoseValidity: unknown thresholds {sorted(unknown)}; known: {sorted(DEFAULT_THRESHOLDS)}")
        self.thresholds.update({k: float(v) for k, v in (thresholds or {}).items()})
        self._thr = ValidityThresholds(*[self.thresholds[k] for k in DEFAULT_THRESHOLDS])
        self._tables = {}
        if device is not None:
            self.tables(device)

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_bonds(n_lig_atoms: int, bonds, x_ref_lig, elements, ligand_idx, a_mask=None, bond_orders=None, planar_groups=None,
                   heavy_only: bool = True, radii: Optional[dict] = None, thresholds: Optional[dict] = None, device=None):
        """bonds: pairs of LOCAL ligand indices (position in `ligand_idx`); x_ref_lig [L,3] a reference conformer in that order;
        elements: atomic numbers of all A pose atoms; ligand_idx [L]: the ligand's atoms in a pose; a_mask [A] (default: every atom
        exists).  `heavy_only`: hydrogens take no part in the receptor and non-bonded checks (they still do in bonds and angles).
        `planar_groups`: explicit groups of local indices (4 to 8 atoms each); None derives them from `bond_orders`
        (`planar_groups_from_bonds`), and without bond orders there are none.  `radii={Z: r}` overrides van der Waals radii."""
        def host(t, dtype):
            return np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, dtype=dtype)
        L = int(n_lig_atoms)
        lig = host(ligand_idx, np.int64).reshape(-1)
        xr = host(x_ref_lig, np.float64)
        el = host(elements, np.int64).reshape(-1)
        A = int(el.shape[0])
        if lig.shape[0] != L:
            raise ValueError(f"PoseValidity: the tables are over {L} ligand atoms, ligand_idx holds {lig.shape[0]}")
        if xr.shape != (L, 3):
            raise ValueError(f"PoseValidity: the tables are over {L} ligand atoms, x_ref_lig has shape {tuple(xr.shape)}")
        if not 1 <= L <= MAX_ATOMS or A > MAX_POSE_ATOMS:
            raise ValueError(f"PoseValidity: {L} ligand atoms of {A}; the kernel takes 1 .. {MAX_ATOMS} of up to {MAX_POSE_ATOMS}")
        if lig.size and (lig.min() < 0 or lig.max() >= A) or len(set(lig.tolist())) != L:
            raise ValueError(f"PoseValidity: ligand_idx must hold {L} distinct atom indices below {A}")
        am = np.ones(A, dtype=bool) if a_mask is None else host(a_mask, np.float64).reshape(-1) > 0
        if am.shape[0] != A:
            raise ValueError(f"PoseValidity: elements are given for {A} atoms, a_mask for {am.shape[0]}")
        bonds = [(int(i), int(j)) for i, j in (bonds.tolist() if hasattr(bonds, "tolist") else bonds)]
        if any(not (0 <= i < L and 0 <= j < L) or i == j for i, j in bonds):
            raise ValueError(f"PoseValidity: a bond leaves the ligand's {L} atoms or joins an atom to itself")
        if bond_orders is not None and len(bond_orders) != len(bonds):
            raise ValueError(f"PoseValidity: {len(bonds)} bonds but {len(bond_orders)} bond orders")
        topo, _ = _topological_distances(L, bonds)
        iu, ju = np.triu_indices(L, 1)
        def pairs(k):
            m = topo[iu, ju] == k
            p = np.stack([iu[m], ju[m]], -1).astype(np.int32).reshape(-1, 2)
            return p, np.linalg.norm(xr[p[:, 0]] - xr[p[:, 1]], axis=-1).astype(np.float32)
        pair12, d12 = pairs(1)
        pair13, d13 = pairs(2)
        if (d12 <= 0).any() or (d13 <= 0).any():
            raise ValueError("PoseValidity: two bonded or 1-3 atoms of the reference conformer coincide")
        far = (topo >= 4).astype(np.uint8)
        np.fill_diagonal(far, 0)
        table = dict(VDW_RADII)
        table.update({int(z): float(r) for z, r in (radii or {}).items()})
        if any(not r > 0 for r in table.values()):
            raise ValueError("PoseValidity: van der Waals radii must be positive")
        radius = np.asarray([table.get(int(z), DEFAULT_RADIUS) for z in el], dtype=np.float32)
        is_lig = np.zeros(A, dtype=bool)
        is_lig[lig] = True
        heavy = el != 1 if heavy_only else np.ones(A, dtype=bool)
        if planar_groups is None:
            planar_groups = planar_groups_from_bonds(L, bonds, bond_orders) if bond_orders is not None else []
        planar = -np.ones((len(planar_groups), GROUP_WIDTH), dtype=np.int32)
        for g, atoms in enumerate(planar_groups):
            atoms = [int(a) for a in atoms]
            if not 4 <= len(atoms) <= GROUP_WIDTH or len(set(atoms)) != len(atoms) or min(atoms) < 0 or max(atoms) >= L:
                raise ValueError(f"PoseValidity: planar group {g} must hold 4 .. {GROUP_WIDTH} distinct ligand atoms, got {atoms}")
            planar[g, :len(atoms)] = atoms
        if planar.shape[0] > MAX_GROUPS:
            raise ValueError(f"PoseValidity: {planar.shape[0]} planar groups; the kernel takes up to {MAX_GROUPS}")
        return PoseValidity(dict(ligand_idx=lig.astype(np.int32), radius=radius, rec_mask=(am & ~is_lig & heavy).astype(np.uint8),
                                 lig_active=heavy[lig].astype(np.uint8), pair12=pair12, d12_ref=d12, pair13=pair13, d13_ref=d13,
                                 far=far, planar=planar), thresholds, device)

    @staticmethod
    def from_batch(batch, bonds, **kw):
        """from a feature dict: the ligand's atoms are those of `driver.ligand_atom_mask`, the elements come from the one-hot
        `ref_feat[:, 4:132]` (index = atomic number - 1), the reference conformer from `ref_pos`, `a_mask` from the batch (when it
        has one); the tables are uploaded to the batch's device.  Other keywords as for `from_bonds`."""
        from .driver import ligand_atom_mask
        lig = torch.nonzero(ligand_atom_mask(batch)).flatten()
        elements = batch["ref_feat"][:, 4:132].argmax(-1) + 1
        dev = batch["ref_pos"].device
        kw.setdefault("a_mask", batch.get("a_mask"))
        kw.setdefault("device", dev if dev.type == "cuda" else None)
        return PoseValidity.from_bonds(int(lig.numel()), bonds, batch["ref_pos"][lig], elements, lig, **kw)

    @staticmethod
    def from_mmff_terms(terms, x_ref_lig, elements, ligand_idx, **kw):
        """the bond graph of an `mmff.MMFFTerms` table (its bond rows); the other arguments as for `from_bonds`"""
        from .mmff import BOND
        return PoseValidity.from_bonds(terms.n_atoms, terms.idx[BOND], x_ref_lig, elements, ligand_idx, **kw)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernel's tables on `device` (uploaded once)"""
        names = ("ligand_idx", "radius", "rec_mask", "lig_active", "pair12", "d12_ref", "pair13", "d13_ref", "far", "planar")
        return ops.cached_upload(self._tables, device, lambda up: {k: up(getattr(self, k)) for k in names})

    def check(self, x_pred: torch.Tensor) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> dict of device tensors: valid [P] bool, flags [P] int32 (bit mask in CHECK_NAMES order),
        bond_ratio, angle_ratio [P,2] (min, max of distance / reference distance), internal_clash, receptor_clash [P] (smallest
        distance / van der Waals sum), receptor_distance [P] (smallest ligand - receptor distance, A), planarity [P] (largest
        distance to a group's plane, A), worst_pair [P,2] int32 ((ligand atom as position in ligand_idx, pose atom) of
        receptor_clash; -1 without a receptor).  Empty sets give 1, +inf, 0.  Nothing is read back, nothing synchronises."""
        if x_pred.dim() != 3 or x_pred.shape[1] != self.n_pose_atoms or x_pred.shape[2] != 3:
            raise ValueError(f"PoseValidity.check: the tables are over {self.n_pose_atoms} pose atoms, x_pred has shape {tuple(x_pred.shape)}")
        L_ = ops._lib.init()
        x = x_pred.float().contiguous()
        P, A = x.shape[0], x.shape[1]
        t = self.tables(x.device)
        n_ws = L_.pd_pose_validity_workspace_numel(P, A)
        ops.check(min(n_ws, 0), "pd_pose_validity_workspace_numel")
        ws = torch.empty(n_ws, dtype=torch.int64, device=x.device)
        val = torch.empty(P, 8, device=x.device)
        worst = torch.empty(P, 2, dtype=torch.int32, device=x.device)
        flags = torch.empty(P, dtype=torch.int32, device=x.device)
        n12, n13, G = self.pair12.shape[0], self.pair13.shape[0], self.planar.shape[0]
        ptr = lambda k, n=1: ops.ptr(t[k]) if n else None
        ops.check(L_.pd_pose_validity(ops.ptr(x), ptr("ligand_idx"), ptr("radius"), ptr("rec_mask"), ptr("lig_active"),
                                      ptr("pair12", n12), ptr("d12_ref", n12), ptr("pair13", n13), ptr("d13_ref", n13), ptr("far"),
                                      ptr("planar", G), self._thr, ops.ptr(ws), ops.ptr(val), ops.ptr(worst), ops.ptr(flags),
                                      P, A, self.n_atoms, n12, n13, G, ops.stream()), "pd_pose_validity")
        return {"valid": flags == 0, "flags": flags, "bond_ratio": val[:, 0:2], "angle_ratio": val[:, 2:4], "internal_clash": val[:, 4],
                "receptor_clash": val[:, 5], "receptor_distance": val[:, 6], "planarity": val[:, 7], "worst_pair": worst}

    @staticmethod
    def check_names(flags_row) -> list:
        """names of the failed checks of one pose's flags value"""
        f = int(flags_row)
        return [n for b, n in enumerate(CHECK_NAMES) if f >> b & 1]

    def __repr__(self):
        return (f"PoseValidity(n_atoms={self.n_atoms}, n_pose_atoms={self.n_pose_atoms}, bonds={self.pair12.shape[0]}, "
                f"angles={self.pair13.shape[0]}, planar_groups={self.planar.shape[0]})")
