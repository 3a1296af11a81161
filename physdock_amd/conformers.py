"""Where does the template pool come from?  Conformers of one ligand by distance geometry, on the device (kernels
`pd_embed_conformers` and `pd_dg_error_grad`, csrc/conformers.hip).  The reference generates the pool `ref_mol_poses [C,L,3]` of the
physics-guided template projection with RDKit ETKDG on the host (redocking.py:231-243, screening.py:251-267, model.py:188-203);
RDKit is not a dependency of this package, so this is **the package's own definition, not a port of ETKDG**: no metric-matrix
eigen-solve, no torsion-knowledge terms, no force-field clean-up.  tests/conformers_ref.py is the written definition in float64.

    bounds lo, up [L,L]     1-2 pairs d_ref +- 0.01; 1-3 pairs d_ref +- 0.04; pairs inside one planar group d_ref +- 0.05; the remaining
                            1-4 pairs [d_cis - 0.05, d_trans + 0.05] in closed form from the reference's two angles and three lengths
                            (several paths: the widest interval); every other pair [0.7 (r_i + r_j), 1000] with `validity.VDW_RADII`;
                            then triangle smoothing, the upper bounds by Floyd-Warshall, the lower by lo_ij >= lo_ik - up_kj
    stereocentres           (c, n1, n2, n3) of `chirality.centres_from_bonds`: V = (n1 - c) . ((n2 - c) x (n3 - c)) stays within
                            [0.6, 1.4] V_ref
    E(x), x [L,4]           sum_{i<j} [d2 > up2] (d2 / up2 - 1)^2 + [d2 < lo2] (2 lo2 / (lo2 + d2) - 1)^2 + w_chi sum viol(V)^2
                            + w_4d sum_a w_a^2      (d over four coordinates, V over the first three)
    embed                   C independent float64 minimisations from random points of [-box, box]^4 (Philox keyed by the seed): stage 1
                            with (w_chi, w_4d) = (1, 0.1), stage 2 with (0.2, 1.0), the BFGS of the MMFF relaxation; then the fourth
                            coordinate is dropped and the conformer centred.  It is accepted when the largest bound violation is <= 0.1
                            A, every centre has the handedness of the reference and max|w| <= 0.1.

**Caveats.**  The pool spans what the bounds allow: torsions are sampled without any preference, so eclipsed and staggered
arrangements are equally likely, and the geometry inside the tolerances is not relaxed.  The volume term sees three of a
stereocentre's four neighbours: a start can end with the fourth on the wrong side of them, 0.4 A short of its 1-3 bounds, and is then
rejected, not repaired (about a quarter of the starts on the test ligands).  Out of scope: ETKDG's torsion preferences,
an MMFF clean-up, macrocycle handling, hydrogens, parity with RDKit.  Limits: L <= 128, at most 64 centres, C <= 4096.

`ConformerEnsemble` holds one ligand's tables, built once on the host; `embed` and `error` return device tensors.  `embed(...,
prune_rms=)` drops near-duplicates by their best-fit RMSD and `coverage(poses, x_ref)` measures whether the pool contains a reference
conformer (`bestfit.BestFitRmsd`).
`driver.redock(..., physics_correction=True, conformers=)` takes the pool from `embed` when no `ref_mol_poses` is given.
`ideal_bounds(ligand)` builds the same kind of table without a reference conformer, from ideal bond lengths and angles: the bounds
behind `ligand.Ligand.embed_reference`.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import ops
from .scoring import _bond_list, _host
from .validity import DEFAULT_RADIUS, VDW_RADII

__all__ = ["ConformerEnsemble", "bounds_from_bonds", "ideal_bounds", "smooth_bounds", "MAX_ATOMS", "MAX_CENTRES", "MAX_CONFORMERS", "STATUS", "STAGES"]

#: limits of the kernel (csrc/conformers.hip)
MAX_ATOMS, MAX_CENTRES, MAX_CONFORMERS = 128, 64, 4096
#: `status` of a stage, as `refine.STATUS`
STATUS = ("converged", "max_iters", "line_search")
#: (w_chi, w_4d) of the two stages
STAGES = ((1.0, 0.1), (0.2, 1.0))
TOL_12, TOL_13, TOL_PLANAR, TOL_14, VDW_SCALE, UP_FAR = 0.01, 0.04, 0.05, 0.05, 0.7, 1000.0
VOL_RANGE, VOL_MIN = (0.6, 1.4), 0.1


def bounds_from_bonds(n_atoms: int, bonds, x_ref, elements, planar_groups=()):
    """The unsmoothed table of the module docstring -> (lo, up) float64 [L,L], symmetric, zero diagonal"""
    L = int(n_atoms)
    x = _host(x_ref, np.float64).reshape(L, 3)
    radius = np.asarray([VDW_RADII.get(int(z), DEFAULT_RADIUS) for z in _host(elements, np.int64).reshape(-1)], dtype=np.float64)
    if radius.shape[0] != L:
        raise ValueError(f"ConformerEnsemble: {radius.shape[0]} elements for {L} atoms")
    adj = [set() for _ in range(L)]
    for i, j in bonds:
        adj[i].add(j); adj[j].add(i)
    d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    lo = VDW_SCALE * (radius[:, None] + radius[None])
    up = np.full((L, L), UP_FAR)
    rank = np.zeros((L, L), dtype=np.int8)               # 0 other, 1 a 1-4 pair, 2 planar, 3 a 1-3 pair, 4 bonded: the higher wins

    def put(i, j, r, a, b):
        if r < rank[i, j]:
            return
        if r == 1 and rank[i, j] == 1:                   # a second path between the ends: the widest interval
            a, b = min(a, lo[i, j]), max(b, up[i, j])
        rank[i, j] = rank[j, i] = r
        lo[i, j] = lo[j, i] = a
        up[i, j] = up[j, i] = b

    def cos_at(i, j, k):
        u, v = x[i] - x[j], x[k] - x[j]
        return float(np.clip(u @ v / np.sqrt((u @ u) * (v @ v)), -1.0, 1.0))

    for i in range(L):
        for j in adj[i]:
            put(i, j, 4, d[i, j] - TOL_12, d[i, j] + TOL_12)
            for k in adj[j] - {i}:
                put(i, k, 3, d[i, k] - TOL_13, d[i, k] + TOL_13)
                for l in adj[k] - {i, j}:
                    a, b, c = d[i, j], d[j, k], d[k, l]
                    c1, c2 = cos_at(i, j, k), cos_at(j, k, l)
                    s1, s2 = np.sqrt(1.0 - c1 * c1), np.sqrt(1.0 - c2 * c2)
                    along = b - a * c1 - c * c2
                    put(i, l, 1, float(np.hypot(along, a * s1 - c * s2)) - TOL_14, float(np.hypot(along, a * s1 + c * s2)) + TOL_14)
    for group in planar_groups:
        g = [int(a) for a in group if int(a) >= 0]
        if any(a >= L for a in g):
            raise ValueError(f"ConformerEnsemble: the planar group {tuple(g)} leaves the {L} atoms")
        for i in g:
            for j in g:
                if i != j:
                    put(i, j, 2, d[i, j] - TOL_PLANAR, d[i, j] + TOL_PLANAR)
    np.fill_diagonal(lo, 0.0)
    np.fill_diagonal(up, 0.0)
    return lo, up


def smooth_bounds(lo, up):
    """Triangle smoothing: the upper bounds by Floyd-Warshall, then the lower bounds by lo_ij >= lo_ik - up_kj -> new (lo, up).
    ValueError when a lower bound ends above its upper bound."""
    lo, up = np.array(lo, dtype=np.float64), np.array(up, dtype=np.float64)
    for k in range(lo.shape[0]):
        np.minimum(up, up[:, k, None] + up[None, k, :], out=up)
    for k in range(lo.shape[0]):
        np.maximum(lo, lo[:, k, None] - up[None, k, :], out=lo)
        np.maximum(lo, lo[None, k, :] - up[:, k, None], out=lo)
    np.fill_diagonal(lo, 0.0)
    if (lo > up).any():
        i, j = (int(v) for v in np.argwhere(lo > up)[0])
        raise ValueError(f"ConformerEnsemble: the bounds contradict each other, smoothing leaves lo > up for the pair ({i}, {j})")
    return lo, up


#: single-bond covalent radii (Cordero et al. 2008), A; any other element: COVALENT_FALLBACK x its `VDW_RADII` entry
COVALENT_RADII = {1: 0.31, 5: 0.84, 6: 0.76, 7: 0.71, 8: 0.66, 9: 0.57, 14: 1.11, 15: 1.07, 16: 1.05, 17: 1.02, 34: 1.20, 35: 1.20, 53: 1.39}
COVALENT_FALLBACK = 0.45
#: what a bond is shorter by than the sum of the radii: single, conjugated single, aromatic, double, triple
SHRINK_SINGLE, SHRINK_CONJUGATED, SHRINK_AROMATIC, SHRINK_DOUBLE, SHRINK_TRIPLE = 0.0, 0.06, 0.13, 0.19, 0.32
#: the angle at a centre by its hybridisation index (1 SP, 2 SP2, 3 and above), and inside a ring of 3, 4, 5 atoms
IDEAL_ANGLES, RING_ANGLES = {1: 180.0, 2: 120.0}, {3: 60.0, 4: 90.0, 5: 108.0}
TETRAHEDRAL_ANGLE = 109.4712
#: the signed volume of three unit vectors to the corners of a regular tetrahedron
TETRAHEDRAL_VOLUME = 4.0 / (3.0 * np.sqrt(3.0))


def ideal_bounds(ligand, smooth: bool = True) -> Dict[str, object]:
    """Bounds without a reference conformer, from a `ligand.Ligand` (host, float64; **the package's own table, unvalidated beyond the
    bond lengths of one crystal ligand**, NOTES.md) -> dict: `lo`, `up` [L,L] smoothed (`smooth_bounds`), `lengths` [n_bonds], `centres`
    int32 [n,4] with `vol_lo`, `vol_hi` [n], `unspecified_centres` (atoms `chirality.centres_from_bonds` finds that carry no `@`).

    1-2  r_i + r_j - shrink +- TOL_12 (`COVALENT_RADII`; shrink 0 single, 0.06 conjugated single, 0.13 aromatic, 0.19 double, 0.32 triple)
    1-3  the cosine law +- TOL_13 with the centre's angle: 180 / 120 / 109.4712 degrees for hybridisation index 1 / 2 / >= 3
         (`Ligand.perceive`), the regular polygon's 60 / 90 / 108 when both neighbours share a ring of 3 / 4 / 5 atoms with the centre
    1-4  [cis - TOL_14, trans + TOL_14] in closed form from those lengths and angles (several paths: the widest interval); cis +-
         TOL_PLANAR when all four atoms lie in one ring and the central bond is aromatic
         a double bond with a row (a, b, c, d, kind, a2, d2) in `ligand.bond_stereo`: the pairs (a, d) and (a2, d2) get cis +-
         TOL_PLANAR when kind is 1 and trans +- TOL_PLANAR when it is 2, the mixed pairs (a, d2) and (a2, d) the other one - the
         isomer is pinned and the bond planar.  A double bond without a row keeps the wide interval.  `stereo_bonds` returns the rows.
    else [VDW_SCALE (r_i + r_j), UP_FAR] with `validity.VDW_RADII`
    `smooth=False` returns `lo`, `up` before the triangle smoothing.
    A centre written `@` / `@@` with four substituents, at most one of them a hydrogen: (c, n1, n2, n3) are the heavy neighbours of
    `chiral_order` without the first (with a hydrogen: without it), V = (n1 - c) . ((n2 - c) x (n3 - c)) lies within VOL_RANGE x
    (sign x TETRAHEDRAL_VOLUME x the three ideal lengths); the sign is + for `@@` and - for `@`, reversed when the hydrogen stands at
    an odd place of the order.  Anchor: `N[C@@H](C)C(=O)O` is L-alanine, (CB - CA) . ((N - CA) x (C - CA)) > 0."""
    from .chirality import centres_from_bonds
    L = ligand.n_atoms
    z, orders = ligand.elements, ligand.bond_orders
    bonds = [(int(i), int(j)) for i, j in ligand.bonds.tolist()]
    p = ligand.perceive()
    hyb, rings = p["hybridization"], [frozenset(r) for r in p["rings"]]
    vdw = np.asarray([VDW_RADII.get(int(e), DEFAULT_RADIUS) for e in z], dtype=np.float64)
    cov = np.asarray([COVALENT_RADII.get(int(e), COVALENT_FALLBACK * VDW_RADII.get(int(e), DEFAULT_RADIUS)) for e in z], dtype=np.float64)
    length, aromatic_bond = {}, {}
    for b, (i, j) in enumerate(bonds):
        o = float(orders[b])
        shrink = (SHRINK_AROMATIC if o == 1.5 else SHRINK_DOUBLE if o == 2.0 else SHRINK_TRIPLE if o == 3.0 else
                  SHRINK_CONJUGATED if (o == 1.0 and p["conjugated"][b]) else SHRINK_SINGLE)
        length[i, j] = length[j, i] = cov[i] + cov[j] - shrink
        aromatic_bond[i, j] = aromatic_bond[j, i] = o == 1.5
    adj = [set() for _ in range(L)]
    for i, j in bonds:
        adj[i].add(j); adj[j].add(i)

    def angle(i, j, k):                                      # at j, radians
        small = [len(r) for r in rings if len(r) <= 5 and i in r and j in r and k in r]
        deg = RING_ANGLES[min(small)] if small else IDEAL_ANGLES.get(int(hyb[j]), TETRAHEDRAL_ANGLE)
        return np.deg2rad(deg)

    lo = VDW_SCALE * (vdw[:, None] + vdw[None])
    up = np.full((L, L), UP_FAR)
    rank = np.zeros((L, L), dtype=np.int8)                   # as `bounds_from_bonds`: 1 a 1-4 pair, 2 planar, 3 a 1-3 pair, 4 bonded

    def put(i, j, r, a, b):
        if r < rank[i, j]:
            return
        if r == rank[i, j] and r in (1, 2):                  # a second path between the ends: the widest interval
            a, b = min(a, lo[i, j]), max(b, up[i, j])
        rank[i, j] = rank[j, i] = r
        lo[i, j] = lo[j, i] = a
        up[i, j] = up[j, i] = b

    for i in range(L):
        for j in adj[i]:
            put(i, j, 4, length[i, j] - TOL_12, length[i, j] + TOL_12)
            for k in adj[j] - {i}:
                a, b, t1 = length[i, j], length[j, k], angle(i, j, k)
                d13 = float(np.sqrt(a * a + b * b - 2.0 * a * b * np.cos(t1)))
                put(i, k, 3, d13 - TOL_13, d13 + TOL_13)
                for l in adj[k] - {i, j}:
                    c, t2 = length[k, l], angle(j, k, l)
                    along = b - a * np.cos(t1) - c * np.cos(t2)
                    cis = float(np.hypot(along, a * np.sin(t1) - c * np.sin(t2)))
                    trans = float(np.hypot(along, a * np.sin(t1) + c * np.sin(t2)))
                    if aromatic_bond[j, k] and any(i in r and j in r and k in r and l in r for r in rings):
                        put(i, l, 2, cis - TOL_PLANAR, cis + TOL_PLANAR)
                    else:
                        put(i, l, 1, cis - TOL_14, trans + TOL_14)
    for a, b, c, d, kind, a2, d2 in ligand.bond_stereo.tolist():
        for i, l, same in ((a, d, True), (a2, d2, True), (a, d2, False), (a2, d, False)):
            if i < 0 or l < 0:
                continue
            la, lb, lc, t1, t2 = length[i, b], length[b, c], length[c, l], angle(i, b, c), angle(b, c, l)
            along = lb - la * np.cos(t1) - lc * np.cos(t2)
            cis = float(np.hypot(along, la * np.sin(t1) - lc * np.sin(t2)))
            trans = float(np.hypot(along, la * np.sin(t1) + lc * np.sin(t2)))
            mid = cis if (kind == 1) == same else trans
            if rank[i, l] == 2:                              # the stated arrangement replaces a planar interval, it does not widen it
                rank[i, l] = rank[l, i] = 1
            put(i, l, 2, mid - TOL_PLANAR, mid + TOL_PLANAR)
    np.fill_diagonal(lo, 0.0)
    np.fill_diagonal(up, 0.0)
    if smooth:
        lo, up = smooth_bounds(lo, up)

    centres, vol = [], []
    for c in range(L):
        order = ligand.chiral_order.get(c)
        if not ligand.chiral[c] or order is None or len(order) != 4 or sum(1 for v in order if v < 0) > 1:
            continue
        sign = 1.0 if int(ligand.chiral[c]) == 2 else -1.0
        if -1 in order:
            if order.index(-1) % 2:
                sign = -sign
            three = [v for v in order if v >= 0]
        else:
            three = list(order[1:])
        centres.append((c, *three))
        vol.append(sign * TETRAHEDRAL_VOLUME * float(np.prod([length[c, v] for v in three])))
    vol = np.asarray(vol, dtype=np.float64)
    written = {c[0] for c in centres}
    found = centres_from_bonds(L, bonds, elements=[int(e) for e in z], bond_orders=[float(o) for o in orders],
                               implicit_h=[int(h) for h in ligand.h_count])
    return {"lo": lo, "up": up, "lengths": np.asarray([length[i, j] for i, j in bonds], dtype=np.float64),
            "centres": np.asarray(centres, dtype=np.int32).reshape(-1, 4),
            "vol_lo": np.minimum(VOL_RANGE[0] * vol, VOL_RANGE[1] * vol), "vol_hi": np.maximum(VOL_RANGE[0] * vol, VOL_RANGE[1] * vol),
            "unspecified_centres": sorted({int(q[0]) for q in found} - written), "stereo_bonds": ligand.bond_stereo}


class ConformerEnsemble:
    """One ligand's tables for `pd_embed_conformers`, as host copies: `lo`, `up` float64 [L,L] (smoothed), `centres` int32 [n,4],
    `vol_lo`, `vol_hi` float64 [n]; `box` is the half-width of the start cube, half the largest upper bound.  `bond_stereo`: None, or
    the `bond_stereo.BondStereo` of the ligand's stated double bonds that `embed` reports `stereo_ok` by."""

    def __init__(self, lo, up, centres, vol_lo, vol_hi, device=None, bond_stereo=None):
        self.lo, self.up, self.centres, self.vol_lo, self.vol_hi = lo, up, centres, vol_lo, vol_hi
        self.bond_stereo = bond_stereo
        self.n_atoms, self.n_centres = int(lo.shape[0]), int(centres.shape[0])
        self.box = 0.5 * float(up.max()) if self.n_atoms > 1 else 1.0
        self._tables = {}
        if device is not None:
            self.tables(device)

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_tables(lo, up, centres=None, vol_lo=None, vol_hi=None, device=None, bond_stereo=None):
        """lo, up [L,L] (used as they are: symmetric, zero diagonal, 0 < lo <= up off it), centres [n,4] with vol_lo <= vol_hi [n]
        of one sign each; bond_stereo: the rows (a, b, c, d, kind, a2, d2) of `ideal_bounds(...)["stereo_bonds"]` or a
        `bond_stereo.BondStereo` over the L atoms - `embed` then reports `stereo_ok`; it rejects nothing"""
        lo, up = np.ascontiguousarray(_host(lo, np.float64)), np.ascontiguousarray(_host(up, np.float64))
        if lo.ndim != 2 or lo.shape[0] != lo.shape[1] or up.shape != lo.shape:
            raise ValueError(f"ConformerEnsemble: lo {lo.shape} and up {up.shape} must be square and alike")
        L = lo.shape[0]
        if not 1 <= L <= MAX_ATOMS:
            raise ValueError(f"ConformerEnsemble: {L} atoms; the kernel takes 1 .. {MAX_ATOMS}")
        off = ~np.eye(L, dtype=bool)
        if not (np.isfinite(lo).all() and np.isfinite(up).all()) or (lo != lo.T).any() or (up != up.T).any():
            raise ValueError("ConformerEnsemble: the bounds must be finite and symmetric")
        if (lo[off] <= 0.0).any() or (lo > up).any() or np.diagonal(lo).any() or np.diagonal(up).any():
            raise ValueError("ConformerEnsemble: the bounds need 0 < lo <= up off the diagonal and zeros on it")
        c = np.ascontiguousarray(_host([] if centres is None else centres, np.int32).reshape(-1, 4))
        vlo = np.ascontiguousarray(_host([] if vol_lo is None else vol_lo, np.float64).reshape(-1))
        vhi = np.ascontiguousarray(_host([] if vol_hi is None else vol_hi, np.float64).reshape(-1))
        if c.shape[0] > MAX_CENTRES:
            raise ValueError(f"ConformerEnsemble: {c.shape[0]} centres; the kernel takes up to {MAX_CENTRES}")
        if vlo.shape[0] != c.shape[0] or vhi.shape[0] != c.shape[0]:
            raise ValueError(f"ConformerEnsemble: {c.shape[0]} centres but {vlo.shape[0]} / {vhi.shape[0]} volume bounds")
        if c.size and (c.min() < 0 or c.max() >= L or any(len(set(q)) != 4 for q in c.tolist())):
            raise ValueError(f"ConformerEnsemble: a centre leaves the {L} atoms or names an atom twice")
        if not np.isfinite(vlo).all() or not np.isfinite(vhi).all() or (vlo > vhi).any() or (vlo * vhi <= 0.0).any():
            raise ValueError("ConformerEnsemble: every centre needs vol_lo <= vol_hi of one sign")
        if bond_stereo is not None and not hasattr(bond_stereo, "accept"):
            from .bond_stereo import BondStereo
            rows = _host(bond_stereo, np.int64).reshape(-1, 7)
            bond_stereo = BondStereo(rows[:, [0, 1, 2, 3, 5, 6]], rows[:, 4], L)
        if bond_stereo is not None and bond_stereo.max_index >= L:
            raise ValueError(f"ConformerEnsemble: bond_stereo reaches atom {bond_stereo.max_index}, the ligand holds {L}")
        return ConformerEnsemble(lo, up, c, vlo, vhi, device, bond_stereo)

    @staticmethod
    def from_bonds(n_atoms: int, bonds, x_ref, elements, bond_orders=None, planar_groups=None, centres=None, device=None):
        """bonds: pairs of atom indices 0 .. n_atoms-1; x_ref [L,3]: the reference conformer (bond lengths, angles, planar groups and
        handedness are taken from it); elements: atomic numbers; planar_groups (default: `validity.planar_groups_from_bonds` when
        bond_orders is given, else none); centres (c, n1, n2, n3) (default: `chirality.centres_from_bonds(..., elements=)`)."""
        from .chirality import centres_from_bonds
        from .validity import planar_groups_from_bonds
        L = int(n_atoms)
        if not 1 <= L <= MAX_ATOMS:
            raise ValueError(f"ConformerEnsemble: {L} atoms; the kernel takes 1 .. {MAX_ATOMS}")
        x = _host(x_ref, np.float64)
        if x.shape != (L, 3) or not np.isfinite(x).all():
            raise ValueError(f"ConformerEnsemble: x_ref must be finite [{L},3], got {x.shape}")
        bonds, orders = _bond_list(L, bonds, bond_orders, "ConformerEnsemble")
        el = [int(z) for z in _host(elements, np.int64).reshape(-1)]
        if len(el) != L:
            raise ValueError(f"ConformerEnsemble: {len(el)} elements for {L} atoms")
        if planar_groups is None:
            planar_groups = planar_groups_from_bonds(L, bonds, orders) if bond_orders is not None else []
        if centres is None:
            centres = centres_from_bonds(L, bonds, elements=el, bond_orders=orders)
        c = np.asarray(list(centres), dtype=np.int64).reshape(-1, 4)
        if c.shape[0] > MAX_CENTRES:
            raise ValueError(f"ConformerEnsemble: {c.shape[0]} centres; the kernel takes up to {MAX_CENTRES}")
        if c.size and (c.min() < 0 or c.max() >= L):
            raise ValueError(f"ConformerEnsemble: a centre leaves the {L} atoms")
        e1, e2, e3 = (x[c[:, k]] - x[c[:, 0]] for k in (1, 2, 3))
        v = np.sum(e1 * np.cross(e2, e3), axis=1)
        if (np.abs(v) < VOL_MIN).any():
            flat = int(c[int(np.argmin(np.abs(v))), 0])
            raise ValueError(f"ConformerEnsemble: the centre {flat} is flat in x_ref (|V_ref| < {VOL_MIN} A^3): no handedness to keep")
        lo, up = smooth_bounds(*bounds_from_bonds(L, bonds, x, el, planar_groups))
        return ConformerEnsemble.from_tables(lo, up, c, np.minimum(VOL_RANGE[0] * v, VOL_RANGE[1] * v),
                                             np.maximum(VOL_RANGE[0] * v, VOL_RANGE[1] * v), device)

    @staticmethod
    def from_batch(batch, bonds, **kw):
        """from a feature dict: the ligand's atoms are those of `driver.ligand_atom_mask`, the elements come from the one-hot
        `ref_feat[:, 4:132]`, the reference conformer from `ref_pos`; bonds are pairs of LOCAL ligand indices.  Other keywords as for
        `from_bonds`; the tables go to the batch's device."""
        from .driver import ligand_atom_mask
        lig = torch.nonzero(ligand_atom_mask(batch)).flatten()
        elements = (batch["ref_feat"][:, 4:132].argmax(-1) + 1)[lig]
        dev = batch["ref_pos"].device
        kw.setdefault("device", dev if dev.type == "cuda" else None)
        return ConformerEnsemble.from_bonds(int(lig.numel()), bonds, batch["ref_pos"][lig], elements, **kw)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernel's tables on `device` (uploaded once)"""
        names = ("lo", "up", "centres", "vol_lo", "vol_hi")
        return ops.cached_upload(self._tables, device, lambda up: {k: up(getattr(self, k)) for k in names})

    def _head(self, device):
        t = self.tables(device)
        n = self.n_centres
        return (ops.ptr(t["lo"]), ops.ptr(t["up"]), ops.ptr(t["centres"]) if n else None, ops.ptr(t["vol_lo"]) if n else None,
                ops.ptr(t["vol_hi"]) if n else None)

    def error(self, pos4: torch.Tensor, w_chi: float, w_4d: float, gradients: bool = False) -> Dict[str, torch.Tensor]:
        """pos4 [C,L,4] (device) -> float64 device tensors err [C] = E and, with `gradients=True`, grad [C,L,4].  Nothing is read back."""
        if pos4.dim() != 3 or pos4.shape[1] != self.n_atoms or pos4.shape[2] != 4 or not 1 <= pos4.shape[0] <= MAX_CONFORMERS:
            raise ValueError(f"ConformerEnsemble.error: pos4 must be [1 .. {MAX_CONFORMERS}, {self.n_atoms}, 4], got {tuple(pos4.shape)}")
        x = pos4.double().contiguous()
        L_ = ops._lib.init()
        out = {"err": torch.empty(x.shape[0], device=x.device, dtype=torch.float64)}
        if gradients:
            out["grad"] = torch.empty_like(x)
        ops.check(L_.pd_dg_error_grad(*self._head(x.device), ops.ptr(x), float(w_chi), float(w_4d), ops.ptr(out["err"]),
                                      ops.ptr(out.get("grad")), x.shape[0], self.n_atoms, self.n_centres, ops.stream()),
                  "pd_dg_error_grad")
        return out

    def embed(self, C: int, seed: int, max_iters: int = 400, grad_tol: float = 1e-4, keep: Optional[str] = "ok", device=None,
              start: Optional[torch.Tensor] = None, box: Optional[float] = None, prune_rms: Optional[float] = None,
              symmetry=None) -> Dict[str, torch.Tensor]:
        """C conformers -> dict of device tensors: x [C,L,3] (fp32, centred; a rejected row is zeros), ok [C] (uint8), err [C] (float64,
        E at the end of stage 2), max_violation [C] (float64, A, in 3-D), iterations and status [C,2] (int32 per stage; `STATUS`), x4 and
        grad4 [C,L,4] (float64: the point stage 2 ended at, before the projection, whether accepted or not, and dE/dx there).
        Conformer c depends on (seed, c) only, not on C.  `start` [C,L,4] replaces the random start, `box` the half-width of its cube.
        Nothing is read back unless `keep="ok"`, which adds `poses`, the accepted rows compacted in order (one read of their number);
        `keep=None` leaves it out.
        `prune_rms` (A; what ETKDG users know as pruneRmsThresh): near-duplicates leave the pool.  The best-fit RMSD of every pair
        (`bestfit.BestFitRmsd(symmetry=symmetry).pairwise(x)`) goes through the greedy leader walk of
        `PoseClusters(cutoff=prune_rms).cluster(D, valid=ok)` in conformer order: `kept` [C] (uint8: accepted and a leader) and
        `duplicate_of` [C] (int32: the leader a dropped duplicate lies within prune_rms of, -1 for leaders and rejected rows) are added
        and `poses` holds the kept rows only.  Without the keyword nothing changes.
        An ensemble that was given `bond_stereo` adds `stereo_ok` [C] (uint8: every stated double bond of the conformer is the stated
        isomer, `BondStereo.accept`); nothing is rejected by it."""
        if keep not in ("ok", None):
            raise ValueError(f"ConformerEnsemble.embed: keep={keep!r}; \"ok\" or None")
        if prune_rms is not None:
            prune_rms = float(prune_rms)
            if not 0.0 <= prune_rms < float("inf"):
                raise ValueError(f"ConformerEnsemble.embed: prune_rms={prune_rms}; expected a finite value >= 0")
            if symmetry is not None and getattr(symmetry, "n_atoms", None) != self.n_atoms:
                raise ValueError(f"ConformerEnsemble.embed: symmetry= is over {getattr(symmetry, 'n_atoms', None)} atoms, the ligand "
                                 f"has {self.n_atoms}")
        elif symmetry is not None:
            raise ValueError("ConformerEnsemble.embed: symmetry= is the table of prune_rms=; give both")
        C = int(C)
        if not 1 <= C <= MAX_CONFORMERS:
            raise ValueError(f"ConformerEnsemble.embed: {C} conformers; the kernel takes 1 .. {MAX_CONFORMERS}")
        box = self.box if box is None else float(box)
        if int(max_iters) < 0 or not float(grad_tol) >= 0 or not box > 0 or not 0 <= int(seed) < 1 << 64:
            raise ValueError(f"ConformerEnsemble.embed: max_iters={max_iters}, grad_tol={grad_tol}, box={box}, seed={seed}")
        if start is not None:
            if tuple(start.shape) != (C, self.n_atoms, 4):
                raise ValueError(f"ConformerEnsemble.embed: start must be [{C}, {self.n_atoms}, 4], got {tuple(start.shape)}")
            start = start.double().contiguous()
            device = start.device
        if device is None:
            device = next(iter(self._tables), None) or torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        L_ = ops._lib.init()
        L = self.n_atoms
        new = lambda shape, dtype: torch.empty(*shape, device=device, dtype=dtype)
        numel = L_.pd_embed_conformers_workspace_numel(C, L)
        ops.check(min(numel, 0), "pd_embed_conformers_workspace_numel")
        ws = new((numel,), torch.float64)
        out = {"x": new((C, L, 3), torch.float32), "ok": new((C,), torch.uint8), "err": new((C,), torch.float64),
               "max_violation": new((C,), torch.float64), "iterations": new((C, 2), torch.int32), "status": new((C, 2), torch.int32)}
        with torch.cuda.device(device):
            ops.check(L_.pd_embed_conformers(*self._head(device), int(seed), int(max_iters), float(grad_tol), box, ops.ptr(ws), numel,
                                             ops.ptr(out["x"]), ops.ptr(out["ok"]), ops.ptr(out["err"]), ops.ptr(out["max_violation"]),
                                             ops.ptr(out["iterations"]), ops.ptr(out["status"]), ops.ptr(start), C, L, self.n_centres,
                                             ops.stream()), "pd_embed_conformers")
        tail = ws.view(C, -1)[:, 16 * L * L:]             # the workspace's tail: the final 4-D point and its gradient
        out["x4"] = tail[:, :4 * L].reshape(C, L, 4).clone()
        out["grad4"] = tail[:, 4 * L:8 * L].reshape(C, L, 4).clone()
        if self.bond_stereo is not None:
            out["stereo_ok"] = self.bond_stereo.accept(out["x"]).to(torch.uint8)
        if prune_rms is not None:
            from .bestfit import BestFitRmsd
            from .clustering import PoseClusters
            got = PoseClusters(cutoff=prune_rms).cluster(BestFitRmsd(symmetry=symmetry).pairwise(out["x"]), valid=out["ok"])
            ids = torch.arange(C, dtype=torch.int32, device=device)
            mine = got["leader"][got["labels"].clamp(min=0).long()]          # each labelled conformer's leader
            lead = (got["labels"] >= 0) & (mine == ids)
            out["kept"] = lead.to(torch.uint8)
            out["duplicate_of"] = torch.where((got["labels"] >= 0) & ~lead, mine, torch.full_like(mine, -1))
        if keep == "ok":
            out["poses"] = out["x"][(out["kept"] if prune_rms is not None else out["ok"]).bool()]
        return out

    def coverage(self, poses: torch.Tensor, x_ref: torch.Tensor, symmetry=None) -> Dict[str, torch.Tensor]:
        """Does the pool contain the reference conformer?  poses [C,L,3] (device; `embed(...)["poses"]`), x_ref [L,3] -> `rmsd` fp32 [C]
        (the best-fit RMSD of every conformer to x_ref, `bestfit.BestFitRmsd.to_reference`), `best` fp32 [1] (the coverage: their
        minimum, NaN without a finite one) and `best_index` int64 [1] (-1 then).  Nothing is read back."""
        from .bestfit import BestFitRmsd
        if not isinstance(poses, torch.Tensor) or poses.dim() != 3 or tuple(poses.shape[1:]) != (self.n_atoms, 3) or poses.shape[0] < 1:
            raise ValueError(f"ConformerEnsemble.coverage: poses must be [C >= 1, {self.n_atoms}, 3], got "
                             f"{tuple(getattr(poses, 'shape', ()))}")
        if not isinstance(x_ref, torch.Tensor) or tuple(x_ref.shape) != (self.n_atoms, 3):
            raise ValueError(f"ConformerEnsemble.coverage: x_ref must be [{self.n_atoms}, 3], got {tuple(getattr(x_ref, 'shape', ()))}")
        r = BestFitRmsd(symmetry=symmetry).cross(poses, x_ref[None])["D"][:, 0]
        key = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
        first = (key == key.min()).to(torch.int8).argmax(0, keepdim=True)                   # the first of equal minima
        best = r[first]
        return {"rmsd": r, "best": best, "best_index": torch.where(torch.isnan(best), torch.full_like(first, -1), first)}

    def __repr__(self):
        return f"ConformerEnsemble(n_atoms={self.n_atoms}, n_centres={self.n_centres}, box={self.box:.2f})"
