"""How large is the pocket the model drew around the ligand, how much of it does the ligand fill, which ligand atoms stick out into the
solvent, and which residues form the site - without a ground truth?  The grid method of LIGSITE (Hendlich, Rippmann & Barnickel 1997)
and POVME on a lattice around the ligand of every pose, on the device (kernel `pd_pocket_grid`, csrc/pocket.hip - its header comment
holds the same definition, tests/pocket_ref.py is the written one).  The model co-folds: every pose carries its own receptor, so the
lattice is recomputed per pose.

One system, over the A atoms of a pose: `cls [A]`, one byte per atom - 0 ignored (padding, `a_mask == 0`, an inactive ligand atom, a
hydrogen), 1 receptor, 2 ligand (the byte of `BuriedSurface`); `radius [A]` in fp32 (`validity.VDW_RADII` / `DEFAULT_RADIUS` by element;
`radii={Z: r}` and `radius=` override as in `BuriedSurface`).

    lattice    n points per axis (8 .. 48), spacing h (fp32).  The centre of a pose is the float64 mean of its active ligand atoms,
               summed in `ligand_idx` order and rounded once to fp32 (`centre="ligand"`), or a given one; with `snap` each coordinate c
               becomes fl32(h rint(c / h)), so that poses a fraction of a spacing apart share a lattice.  o = centre - h (n - 1) / 2;
               point (i, j, k) is g = o + (i, j, k) h with linear index (i n + j) n + k.  Everything here is evaluated in float64.
    solid(g)   some receptor atom j has d(g, x_j) < radius_j + probe
    inside(g)  some active ligand atom i has d(g, x_i) < radius_i
    near(g,j)  d(g, x_j) < radius_j + lining, for a receptor atom j
    buried(g)  of the seven directions (1,0,0) (0,1,0) (0,0,1) (1,1,1) (1,1,-1) (1,-1,1) (-1,1,1) the number in which a solid point lies
               within floor(reach / (h |d|)) lattice steps of g in the + sense and also in the - sense; leaving the lattice is no hit
    pocket     not solid and buried >= min_enclosed.  Pocket points form 6-connected components; a pocket point with inside is occupied;
               the site is the union of the components that hold an occupied point.

`measure(x_pred [P,A,3])` returns device tensors, nothing is read back: `classes uint8 [P,n^3]` (0 solid, 1 free but not pocket, 2 pocket
outside the site, 3 site and empty, 4 site and occupied), `buried uint8 [P,n^3]` (0 for a solid point), `counts int32 [P,8]`
(`COUNT_NAMES`: n_solid, n_free = every non-solid point, n_pocket, n_site, n_occupied, n_ligand = non-solid points with inside,
n_components, n_site_components), `truncated uint8 [P]` (a site point lies on a face of the lattice: the grid is too small), fp32 `[P]`:
`site_volume` = n_site h^3, `unfilled_volume` = (n_site - n_occupied) h^3 (room to grow), `pocket_volume` = n_pocket h^3,
`filled_fraction` = n_occupied / n_site and `ligand_in_site` = n_occupied / n_ligand (0 where the divisor is 0, never NaN),
`ligand_enclosure` = the mean of atom_buried / 7 over the ligand atoms that have a point; per ligand atom in `ligand_idx` order
`atom_class`, `atom_buried uint8 [P,L]` (class and enclosure of the lattice point nearest the atom, rint((x - o) / h); 255 for an inactive
atom and for one outside the lattice: a low `atom_buried` is an atom that sticks out); per residue `lining_points int32 [P,R]` (the site
points g with near(g, j) for a receptor atom j of the residue) and `lining_residues int32 [P]` (residues with a count above 0); `centre
fp32 [P,3]` (the centre used) and `ok uint8 [P]`: a pose with a non-finite coordinate in an atom of class != 0 or a non-finite centre has
ok = 0, every count 0, every float NaN, every byte map 255 and truncated 0.

Every count comes from "any" tests and integer sums, every float is one product or one quotient of exact integers: a pose's values are
bit-identical whatever the number of poses in the call and wherever the pose sits.

**Caveats.**  The defaults - h = 1.0, n = 32, probe = 1.4, lining = 2.4, reach = 12.0, min_enclosed = 5 - are THIS PACKAGE'S OWN AND HAVE
NOT BEEN VALIDATED on real complexes.  Heavy atoms only (the model predicts no hydrogens).  Volumes are counts of lattice points: they
move by a few points with the lattice position, compare poses of one system (that is what `snap` is for).  A point on a face of the
lattice has at most two enclosed directions (the five with a component along the face's normal leave the lattice), so `truncated` can
only fire with min_enclosed <= 2; with the default a site cut off by a small lattice shows as a small site, not as a flag - choose n h
well above the ligand's extent plus 2 reach.  Out of scope: pocket detection without a ligand and druggability, solvent-excluded
surfaces, hydrogens, gradients, feeding the map into the sampler or `VinaSearch`.

`PocketGrid` holds one system's tables, built once on the host; `driver.redock(..., pocket=)` reports the measure of the kept poses and
of the ground truth; `lining(result)` is the residue subset `ReceptorGeometry.chi_recovery(residues=)` takes.
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

__all__ = ["PocketGrid", "step_table", "DIRECTIONS", "COUNT_NAMES", "VALUE_NAMES", "DEFAULT_SPACING", "DEFAULT_N", "DEFAULT_PROBE",
           "DEFAULT_LINING", "DEFAULT_REACH", "DEFAULT_MIN_ENCLOSED", "MIN_N", "MAX_N", "MAX_ATOMS", "MAX_RESIDUES", "MAX_POSE_ATOMS",
           "MAX_POSES", "MAX_EDGE", "IGNORED", "RECEPTOR", "LIGAND"]

#: the defaults (this package's own, not validated): spacing (A), points per axis, probe (A), lining distance (A), reach (A), directions
DEFAULT_SPACING, DEFAULT_N, DEFAULT_PROBE, DEFAULT_LINING, DEFAULT_REACH, DEFAULT_MIN_ENCLOSED = 1.0, 32, 1.4, 2.4, 12.0, 5
#: limits of the kernel (csrc/pocket.hip): points per axis, ligand atoms, residues, pose atoms, poses, lattice edge h (n - 1) in A
MIN_N, MAX_N, MAX_ATOMS, MAX_RESIDUES, MAX_POSE_ATOMS, MAX_POSES, MAX_EDGE = 8, 48, 1024, 4096, 1 << 22, 65535, 4096.0
#: the seven directions of the enclosure test
DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1))
#: the columns of `counts [P,8]` and the rows of the kernel's `values [6,P]`
COUNT_NAMES = ("n_solid", "n_free", "n_pocket", "n_site", "n_occupied", "n_ligand", "n_components", "n_site_components")
VALUE_NAMES = ("site_volume", "unfilled_volume", "pocket_volume", "filled_fraction", "ligand_in_site", "ligand_enclosure")
#: values of a class byte
IGNORED, RECEPTOR, LIGAND = 0, 1, 2


def step_table(reach: float, h: float) -> List[int]:
    """the lattice steps a walk may take per direction: floor(reach / (h |d|)), in float64"""
    return [int(math.floor(float(reach) / (float(h) * math.sqrt(float(sum(v * v for v in d)))))) for d in DIRECTIONS]


class PocketGrid:
    """One system's tables for `pd_pocket_grid`: host copies (numpy: `cls` uint8 [A], `radius` fp32 [A], `ligand_idx` int32 [L],
    `residue_of` int32 [A], the CSR `res_start` int32 [R + 1] / `res_atom` int32 [N] of the receptor atoms), the parameters `h`, `n`,
    `probe`, `lining_distance` (fp32 values), `reach`, `min_enclosed`, `snap`, `steps` (`step_table`), `residue_labels` (a name per residue, or
    None) and, uploaded once per device, what the kernel reads.  `n_atoms` is the ligand's atom count L, `n_pose_atoms` the A of the poses
    `measure` takes, `n_residues` R, `n_receptor_atoms` N."""

    def __init__(self, cls, radius, ligand_idx, residue_of, n_residues, h=DEFAULT_SPACING, n=DEFAULT_N, probe=DEFAULT_PROBE,
                 lining=DEFAULT_LINING, reach=DEFAULT_REACH, min_enclosed=DEFAULT_MIN_ENCLOSED, snap=True, residue_labels=None, device=None):
        self.cls, self.radius, self.ligand_idx = cls, radius, ligand_idx
        self.residue_of, self.n_residues = residue_of, int(n_residues)
        f32 = lambda v: float(np.float32(v))
        self.h, self.n, self.probe, self.lining_distance = f32(h), int(n), f32(probe), f32(lining)
        self.reach, self.min_enclosed, self.snap = float(reach), int(min_enclosed), bool(snap)
        self.steps = [min(s, self.n) for s in step_table(self.reach, self.h)]
        self.res_start, self.res_atom = residue_csr(residue_of, cls == RECEPTOR, self.n_residues)
        self.residue_labels = None if residue_labels is None else [str(s) for s in residue_labels]
        if self.residue_labels is not None and len(self.residue_labels) != self.n_residues:
            raise ValueError(f"PocketGrid: {len(self.residue_labels)} residue labels for {self.n_residues} residues")
        self.n_atoms, self.n_pose_atoms, self.n_receptor_atoms = int(ligand_idx.shape[0]), int(cls.shape[0]), int(self.res_atom.shape[0])
        self._tables = {}
        if device is not None:
            self.tables(device)

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_arrays(elements, ligand_idx, receptor_mask, residue_of, n_residues: Optional[int] = None, a_mask=None, ligand_active=None,
                    h: float = DEFAULT_SPACING, n: int = DEFAULT_N, probe: float = DEFAULT_PROBE, lining: float = DEFAULT_LINING,
                    reach: float = DEFAULT_REACH, min_enclosed: int = DEFAULT_MIN_ENCLOSED, snap: bool = True, radii=None, radius=None,
                    residue_labels=None, device=None):
        """elements: atomic numbers (or symbols) of all A pose atoms - they give the radii (`validity.VDW_RADII`, `radii={Z: r}`
        overrides single elements) and leave hydrogens out on both sides; or None with `radius=` fp32 [A].  ligand_idx [L]: the ligand's
        atoms in a pose; receptor_mask [A] (> 0: the atom counts as receptor; ligand atoms never do); residue_of [A]: the residue id of
        every atom; n_residues (default: the largest id + 1); a_mask [A] (default: every atom exists); ligand_active [L] (default: all):
        0 = the ligand atom is ignored; h (A), n (8 .. 48), probe, lining, reach (A), min_enclosed (0 .. 7), snap: the lattice and the
        thresholds of the module docstring - the defaults are this package's own and have not been validated on real complexes."""
        lig = _host(ligand_idx, np.int64).reshape(-1)
        res = _host(residue_of, np.int64).reshape(-1)
        rec = _host(receptor_mask, np.float64).reshape(-1) > 0
        A, L = int(rec.shape[0]), int(lig.shape[0])
        if A < 1 or A > MAX_POSE_ATOMS or not 1 <= L <= MAX_ATOMS:
            raise ValueError(f"PocketGrid: {L} ligand atoms of {A}; the kernel takes 1 .. {MAX_ATOMS} of up to {MAX_POSE_ATOMS}")
        if lig.min() < 0 or lig.max() >= A or len(set(lig.tolist())) != L:
            raise ValueError(f"PocketGrid: ligand_idx must hold {L} distinct atom indices below {A}")
        if not MIN_N <= int(n) <= MAX_N:
            raise ValueError(f"PocketGrid: n = {n} points per axis; the kernel takes {MIN_N} .. {MAX_N}")
        if not (math.isfinite(float(h)) and float(h) > 0 and float(h) * (int(n) - 1) <= MAX_EDGE):
            raise ValueError(f"PocketGrid: the spacing must be positive and finite with h (n - 1) <= {MAX_EDGE} A, got h = {h}")
        for name, v in (("probe", probe), ("lining", lining), ("reach", reach)):
            if not (math.isfinite(float(v)) and float(v) >= 0):
                raise ValueError(f"PocketGrid: {name} must be finite and not negative, got {v}")
        if not 0 <= int(min_enclosed) <= len(DIRECTIONS):
            raise ValueError(f"PocketGrid: min_enclosed = {min_enclosed}; there are {len(DIRECTIONS)} directions")
        z = None if elements is None else _atomic_numbers(elements)
        if z is None and radius is None:
            raise ValueError("PocketGrid: give elements or radius=")
        if z is not None and z.shape[0] != A:
            raise ValueError(f"PocketGrid: receptor_mask is given for {A} atoms, elements for {z.shape[0]}")
        if radius is not None:
            if radii is not None:
                raise ValueError("PocketGrid: radii= overrides the element table; it cannot be combined with radius=")
            rad = _host(radius, np.float64).reshape(-1)
            if rad.shape[0] != A:
                raise ValueError(f"PocketGrid: receptor_mask is given for {A} atoms, radius for {rad.shape[0]}")
        else:
            table = dict(VDW_RADII)
            table.update({int(k): float(r) for k, r in (radii or {}).items()})
            rad = np.asarray([table.get(int(e), DEFAULT_RADIUS) for e in z], dtype=np.float64)
        if not (np.isfinite(rad).all() and (rad > 0).all()):
            raise ValueError("PocketGrid: radii must be finite and positive")
        am = np.ones(A, dtype=bool) if a_mask is None else _host(a_mask, np.float64).reshape(-1) > 0
        act = np.ones(L, dtype=bool) if ligand_active is None else _host(ligand_active, np.float64).reshape(-1) > 0
        if am.shape[0] != A or act.shape[0] != L or res.shape[0] != A:
            raise ValueError(f"PocketGrid: receptor_mask is given for {A} atoms and ligand_idx for {L}; a_mask {am.shape[0]}, "
                             f"ligand_active {act.shape[0]}, residue_of {res.shape[0]}")
        R = int(res.max()) + 1 if n_residues is None else int(n_residues)
        if res.min() < 0 or res.max() >= R or R < 1:
            raise ValueError(f"PocketGrid: residue_of must lie in 0 .. {R - 1}")
        if R > MAX_RESIDUES:
            raise ValueError(f"PocketGrid: {R} residues; the kernel takes at most {MAX_RESIDUES}")
        heavy = np.ones(A, dtype=bool) if z is None else z != 1
        cls = np.where(rec & am & heavy, RECEPTOR, IGNORED).astype(np.uint8)
        cls[lig] = np.where(act & am[lig] & heavy[lig], LIGAND, IGNORED)
        return PocketGrid(cls, rad.astype(np.float32), lig.astype(np.int32), res.astype(np.int32), R, h, n, probe, lining, reach,
                          min_enclosed, snap, residue_labels, device)

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
        return PocketGrid.from_arrays(elements, lig, np.ones(int(elements.shape[0])), residue_of, **kw)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernel's tables on `device` (uploaded once)"""
        names = ("cls", "radius", "ligand_idx", "res_start", "res_atom")
        return ops.cached_upload(self._tables, device, lambda up: {k: up(getattr(self, k)) for k in names})

    def measure(self, x_pred: torch.Tensor, centre="ligand", maps: bool = True) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> dict of device tensors (module docstring): classes, buried uint8 [P,n^3] (left out with
        maps=False), counts int32 [P,8], truncated uint8 [P], site_volume, unfilled_volume, pocket_volume, filled_fraction,
        ligand_in_site, ligand_enclosure fp32 [P], atom_class, atom_buried uint8 [P,L], lining_points int32 [P,R], lining_residues
        int32 [P], centre fp32 [P,3] and ok uint8 [P].  centre: "ligand" (each pose's ligand mean) or coordinates [3] / [P,3].
        Nothing is read back, nothing synchronises."""
        if x_pred.dim() != 3 or x_pred.shape[1] != self.n_pose_atoms or x_pred.shape[2] != 3:
            raise ValueError(f"PocketGrid.measure: the tables are over {self.n_pose_atoms} pose atoms, x_pred has shape "
                             f"{tuple(x_pred.shape)}")
        if not 1 <= x_pred.shape[0] <= MAX_POSES:
            raise ValueError(f"PocketGrid.measure: {x_pred.shape[0]} poses; the kernel takes 1 .. {MAX_POSES}")
        P, A, L, R, N, n3 = x_pred.shape[0], x_pred.shape[1], self.n_atoms, self.n_residues, self.n_receptor_atoms, self.n ** 3
        given = None
        if not (isinstance(centre, str) and centre == "ligand"):
            if isinstance(centre, str):
                raise ValueError(f"PocketGrid.measure: centre is \"ligand\" or coordinates [3] / [P,3], got {centre!r}")
            given = torch.as_tensor(centre, dtype=torch.float32)
            if tuple(given.shape) not in ((3,), (P, 3)):
                raise ValueError(f"PocketGrid.measure: centre has shape {tuple(given.shape)}; expected (3,) or ({P}, 3)")
        ops._lib.init()
        x = x_pred.float().contiguous()
        if given is not None:
            given = given.to(x.device).contiguous()
        t = self.tables(x.device)
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=x.device)
        out = dict(centre=new((P, 3), torch.float32), ok=new((P,), torch.uint8), classes=new((P, n3), torch.uint8),
                   buried=new((P, n3), torch.uint8), counts=new((P, len(COUNT_NAMES)), torch.int32), truncated=new((P,), torch.uint8),
                   values=new((len(VALUE_NAMES), P), torch.float32), atom_class=new((P, L), torch.uint8), atom_buried=new((P, L), torch.uint8),
                   lining_points=new((P, R), torch.int32), lining_residues=new((P,), torch.int32))
        ws = new((ops.pocket_grid_workspace_numel(P, self.n, A),), torch.int32)
        ops.pocket_grid(x, t, given, self.snap, self.h, self.n, self.probe, self.lining_distance, self.steps, self.min_enclosed, ws, out, L, R, N)
        values = out.pop("values")
        out.update({k: values[i] for i, k in enumerate(VALUE_NAMES)})
        if not maps:
            del out["classes"], out["buried"]
        return out

    def lining(self, result, min_points: int = 1) -> torch.Tensor:
        """bool [P,R] on the device: the residues with at least `min_points` site points near them - the pocket of every pose, e.g. for
        `ReceptorGeometry.chi_recovery(residues=)`"""
        return result["lining_points"] >= int(min_points)

    def describe(self, result, row: int, min_points: int = 1) -> List[Tuple[object, int]]:
        """host helper (one read-back): [(residue label or id, lining points)] of pose `row`, the largest count first (residue order
        among equal counts)"""
        counts = np.asarray(result["lining_points"][row].detach().cpu() if isinstance(result["lining_points"], torch.Tensor)
                            else np.asarray(result["lining_points"])[row], dtype=np.int64).reshape(-1)
        if counts.shape[0] != self.n_residues:
            raise ValueError(f"PocketGrid.describe: a row holds {self.n_residues} counts, got {counts.shape[0]}")
        label = (lambda s: self.residue_labels[s] or s) if self.residue_labels is not None else (lambda s: s)
        keep = [int(s) for s in np.nonzero(counts >= int(min_points))[0]]
        return [(label(s), int(counts[s])) for s in sorted(keep, key=lambda s: (-counts[s], s))]

    def to_dx(self, result, pose: int, what: str = "classes") -> str:
        """host helper (one read-back): the map `what` ("classes" or "buried") of pose `pose` as OpenDX text (PyMOL, VMD): the lattice
        of the pose with the first index along x and the last running fastest, as the linear index does"""
        if what not in ("classes", "buried"):
            raise ValueError(f"PocketGrid.to_dx: what is \"classes\" or \"buried\", got {what!r}")
        if what not in result:
            raise ValueError(f"PocketGrid.to_dx: the result holds no {what} map (measure(..., maps=True))")
        n, h = self.n, self.h
        host = torch.cat([result["centre"][pose].detach().double().cpu().reshape(-1), result[what][pose].detach().double().cpu().reshape(-1)]).numpy()
        centre, data = host[:3], host[3:].astype(np.int64)
        if data.shape[0] != n ** 3:
            raise ValueError(f"PocketGrid.to_dx: a map holds {n ** 3} points, got {data.shape[0]}")
        o = centre - h * (n - 1) / 2
        lines = [f"# physdock_amd PocketGrid {what} of pose {int(pose)}: n = {n}, h = {h:g} A",
                 f"object 1 class gridpositions counts {n} {n} {n}", f"origin {o[0]:.6f} {o[1]:.6f} {o[2]:.6f}",
                 f"delta {h:.6f} 0 0", f"delta 0 {h:.6f} 0", f"delta 0 0 {h:.6f}",
                 f"object 2 class gridconnections counts {n} {n} {n}",
                 f"object 3 class array type double rank 0 items {n ** 3} data follows"]
        lines += [" ".join(str(int(v)) for v in data[q:q + 3]) for q in range(0, n ** 3, 3)]
        lines += ['attribute "dep" string "positions"', f'object "{what}" class field', 'component "positions" value 1',
                  'component "connections" value 2', 'component "data" value 3']
        return "\n".join(lines) + "\n"

    def __repr__(self):
        return (f"PocketGrid(n_atoms={self.n_atoms}, n_pose_atoms={self.n_pose_atoms}, residues={self.n_residues}, "
                f"receptor_atoms={self.n_receptor_atoms}, active_ligand_atoms={int((self.cls == LIGAND).sum())}, h={self.h:g}, n={self.n}, "
                f"probe={self.probe:g}, lining={self.lining_distance:g}, reach={self.reach:g}, min_enclosed={self.min_enclosed}, snap={self.snap})")
