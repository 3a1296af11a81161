"""Does this pose fill the same volume, and put its donors, acceptors, charges and rings in the same places, as that one - even when
the two are different molecules?  Gaussian shape overlap after Grant, Gallardo & Pickup 1996 at first order, as ROCS uses it: a shape
Tanimoto, a "colour" Tanimoto over pharmacophore features and their sum (TanimotoCombo), on the device (csrc/shape_overlap.hip; its
header comment and tests/shape_overlap_ref.py give the definition).  It needs no atom correspondence, no ground truth and no weights:
poses of different ligands in one receptor frame are scored in place, or `overlay` first superposes them rigidly.

Atom i carries p exp(-a_i |r - x_i|^2) with p = 2 sqrt 2, a_i = KAPPA / R_i^2, KAPPA = pi (3 p / (4 pi))^(2/3) (one Gaussian's volume is
its sphere's).  O(A,B) = sum_ij p^2 exp(-a_i a_j d_ij^2 / (a_i + a_j)) (pi / (a_i + a_j))^(3/2); shape_tanimoto = O_AB / (O_AA + O_BB -
O_AB).  Features (`FEATURE_NAMES`) sit at the mean of their member atoms, are Gaussians of radius 1 A and overlap only with their own
kind: color_tanimoto likewise, 0 where neither side has a matching feature.  combo = shape + colour, in [0, 2].  Float64 arithmetic
from the fp32 coordinates in a fixed order; fp32 scores.  A structure with a non-finite named coordinate gives NaN in its row / column.

Caveats.  First-order overlap overestimates volumes (no higher-order intersection terms).  The feature perception is heuristic and
hydrogen-free (the donor / acceptor / hydrophobic bits of `scoring.ligand_types_from_bonds`, the charged groups of
`interactions.ligand_charges_from_bonds`, the aromatic rings of `ring_interactions.aromatic_rings_from_bonds`).  The default radius of
1.7 A for every atom (ROCS's default; `radii="vdw"` takes `validity.VDW_RADII`) is unvalidated here.  `overlay` finds a local optimum
from five starts and optimises shape only.  Limits: 1024 atoms and 1024 features per molecule, 65535 structures per side; `overlay`
256 atoms.  Not here: higher-order terms, colour-optimised overlay, multi-conformer database search, SuCOS's feature-map score.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

FEATURE_NAMES = ("donor", "acceptor", "cation", "anion", "hydrophobe", "ring")
P = 2.0 * math.sqrt(2.0)
KAPPA = math.pi * (3.0 * P / (4.0 * math.pi)) ** (2.0 / 3.0)
DEFAULT_RADIUS, FEATURE_RADIUS = 1.7, 1.0
COLOR_ALPHA = KAPPA / FEATURE_RADIUS ** 2
MAX_ATOMS, MAX_FEATURES, MAX_STRUCTURES, MAX_POSE_ATOMS, MAX_OVERLAY_ATOMS = 1024, 1024, 65535, 1 << 22, 256


def features_from_bonds(elements, bonds, bond_orders=None, formal_charges=None):
    """the default feature table of a molecule: a list of (kind, member atoms), kind an index into FEATURE_NAMES - one per donor atom,
    per acceptor atom, per cation, per anion, per hydrophobic atom outside every aromatic ring, and one `ring` per aromatic ring"""
    from .interactions import ANION, CATION, ligand_charges_from_bonds
    from .ring_interactions import aromatic_rings_from_bonds
    from .scoring import ACCEPTOR, DONOR, HYDROPHOBIC, ligand_types_from_bonds
    bonds = [(int(i), int(j)) for i, j in bonds]
    orders = [1.0] * len(bonds) if bond_orders is None else [float(o) for o in bond_orders]
    types = np.asarray(ligand_types_from_bonds(elements, bonds, orders, formal_charges=formal_charges))
    charges = np.asarray(ligand_charges_from_bonds(elements, bonds, orders, formal_charges=formal_charges))
    n = len(types)
    rings = aromatic_rings_from_bonds(n, bonds, orders)
    in_ring = {a for r in rings for a in r}
    feats = [(0, (i,)) for i in range(n) if types[i] & DONOR]
    feats += [(1, (i,)) for i in range(n) if types[i] & ACCEPTOR]
    feats += [(2, (i,)) for i in range(n) if charges[i] & CATION]
    feats += [(3, (i,)) for i in range(n) if charges[i] & ANION]
    feats += [(4, (i,)) for i in range(n) if (types[i] & HYDROPHOBIC) and i not in in_ring]
    feats += [(5, tuple(int(a) for a in r)) for r in rings]
    return feats


class ShapeSpec:
    """One molecule, immutable: `ligand_idx` (int64 [L], the molecule's atoms among a structure's; None: a structure IS the
    molecule), `radii` float64 [L], and the feature table in CSR form (`feat_kind` [F], `feat_start` [F+1], `feat_atom`: local atom
    indices 0 .. L-1).  Every index is checked here, on the host; the kernels follow them as they are."""

    __slots__ = ("ligand_idx", "radii", "feat_kind", "feat_start", "feat_atom", "_dev")

    def __init__(self, radii, feat_kind, feat_start, feat_atom, ligand_idx=None):
        radii = np.ascontiguousarray(np.asarray(radii, dtype=np.float64).reshape(-1))
        L = radii.shape[0]
        if not 1 <= L <= MAX_ATOMS:
            raise ValueError(f"ShapeSpec: {L} atoms; the kernels take 1 .. {MAX_ATOMS}")
        if not (np.isfinite(radii).all() and (radii > 0).all()):
            raise ValueError("ShapeSpec: radii must be finite and positive")
        kind = np.ascontiguousarray(np.asarray(feat_kind, dtype=np.int32).reshape(-1))
        start = np.ascontiguousarray(np.asarray(feat_start, dtype=np.int32).reshape(-1))
        atom = np.ascontiguousarray(np.asarray(feat_atom, dtype=np.int32).reshape(-1))
        F = kind.shape[0]
        if F > MAX_FEATURES:
            raise ValueError(f"ShapeSpec: {F} features; the kernels take at most {MAX_FEATURES}")
        if start.shape[0] != F + 1 or start[0] != 0 or start[-1] != atom.shape[0] or (np.diff(start) < 1).any():
            raise ValueError("ShapeSpec: feat_start must be [F+1], start at 0, end at len(feat_atom) and give every feature a member")
        if F and (kind.min() < 0 or kind.max() >= len(FEATURE_NAMES)):
            raise ValueError(f"ShapeSpec: feature kinds must be 0 .. {len(FEATURE_NAMES) - 1}")
        if atom.shape[0] and (atom.min() < 0 or atom.max() >= L):
            raise ValueError(f"ShapeSpec: a feature names an atom outside 0 .. {L - 1}")
        if ligand_idx is not None:
            ligand_idx = np.ascontiguousarray(np.asarray(ligand_idx.detach().cpu() if isinstance(ligand_idx, torch.Tensor) else ligand_idx,
                                                         dtype=np.int64).reshape(-1))
            if ligand_idx.shape[0] != L:
                raise ValueError(f"ShapeSpec: ligand_idx names {ligand_idx.shape[0]} atoms, radii {L}")
            if ligand_idx.min() < 0 or ligand_idx.max() >= MAX_POSE_ATOMS:
                raise ValueError(f"ShapeSpec: ligand_idx must lie in 0 .. {MAX_POSE_ATOMS - 1}")
        for k, v in (("radii", radii), ("feat_kind", kind), ("feat_start", start), ("feat_atom", atom), ("ligand_idx", ligand_idx)):
            if v is not None:
                v.setflags(write=False)
            object.__setattr__(self, k, v)
        object.__setattr__(self, "_dev", {})

    def __setattr__(self, name, value):
        raise AttributeError("ShapeSpec is immutable")

    n_atoms = property(lambda self: int(self.radii.shape[0]))
    n_features = property(lambda self: int(self.feat_kind.shape[0]))

    @property
    def features(self):
        """the table as a list of (kind name, member atoms)"""
        return [(FEATURE_NAMES[k], tuple(int(a) for a in self.feat_atom[s:e]))
                for k, s, e in zip(self.feat_kind, self.feat_start[:-1], self.feat_start[1:])]

    def __repr__(self):
        return f"ShapeSpec({self.n_atoms} atoms, {self.n_features} features)"

    @staticmethod
    def _radii(radii, elements, L):
        if radii is None:
            return np.full(L, DEFAULT_RADIUS)
        if isinstance(radii, str):
            if radii != "vdw":
                raise ValueError(f"ShapeSpec: radii={radii!r}; expected None, 'vdw' or an array")
            from .scoring import _atomic_numbers as atomic_numbers
            from .validity import DEFAULT_RADIUS as OTHER, VDW_RADII
            return np.asarray([VDW_RADII.get(int(z), OTHER) for z in atomic_numbers(elements)], dtype=np.float64)
        radii = np.asarray(radii, dtype=np.float64).reshape(-1)
        if radii.shape[0] != L:
            raise ValueError(f"ShapeSpec: {radii.shape[0]} radii for {L} atoms")
        return radii

    @staticmethod
    def from_tables(n_atoms, features=(), radii=None, ligand_idx=None, elements=None):
        """features: a sequence of (kind, members), kind a name of FEATURE_NAMES or its index"""
        kinds, start, atoms = [], [0], []
        for kind, members in features:
            if isinstance(kind, str):
                if kind not in FEATURE_NAMES:
                    raise ValueError(f"ShapeSpec: feature kind {kind!r}; expected one of {FEATURE_NAMES}")
                kind = FEATURE_NAMES.index(kind)
            members = [int(m) for m in members]
            kinds.append(int(kind)); atoms += members; start.append(len(atoms))
        return ShapeSpec(ShapeSpec._radii(radii, elements, int(n_atoms)), kinds, start, atoms, ligand_idx)

    @staticmethod
    def from_bonds(elements, bonds, bond_orders=None, ligand_idx=None, radii=None, features=None, formal_charges=None):
        """the default feature table of `features_from_bonds` (or `features`, as for `from_tables`); elements: atomic numbers or symbols"""
        n = len(elements)
        feats = features_from_bonds(elements, bonds, bond_orders, formal_charges) if features is None else features
        return ShapeSpec.from_tables(n, feats, radii, ligand_idx, elements)

    @staticmethod
    def from_batch(batch, bonds=(), bond_orders=None, **kw):
        """from a feature dict, as the other `from_batch` constructors: the molecule is the atoms of ligand tokens, the elements come
        from `ref_feat`; bonds are pairs of LOCAL ligand indices (without them the molecule has shape but no features)"""
        from .driver import ligand_atom_mask
        lig = torch.nonzero(ligand_atom_mask(batch)).flatten()
        elements = (batch["ref_feat"][:, 4:132].argmax(-1) + 1)[lig].cpu().tolist()
        return ShapeSpec.from_bonds(elements, bonds, bond_orders, ligand_idx=lig, **kw)

    @staticmethod
    def from_sdf(record, **kw):
        """from one record of `sdfio.parse_sdf`; a structure is then the record's atoms in file order (`record["coords"]`)"""
        return ShapeSpec.from_bonds(list(record["elements"]), record["bonds"], record["bond_orders"],
                                    formal_charges=record.get("charges"), **kw)

    def tables(self, device):
        """the device tables (cached per device): alpha float64 [L], kind, start, atom int32, lig int32 or None"""
        key = str(device)
        if key not in self._dev:
            up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to(device)
            self._dev[key] = dict(alpha=up(KAPPA / self.radii ** 2, np.float64), kind=up(self.feat_kind, np.int32),
                                  start=up(self.feat_start, np.int32), atom=up(self.feat_atom, np.int32),
                                  lig=None if self.ligand_idx is None else up(self.ligand_idx, np.int32))
        return self._dev[key]


def tversky(result: Dict[str, torch.Tensor], alpha: float) -> torch.Tensor:
    """O_AB / (alpha O_AA + (1 - alpha) O_BB) of a `cross` / `pairwise` / `to_reference` result: alpha = 1 asks how much of A lies in
    B, alpha = 0 how much of B in A.  [P,C] for `cross` and `pairwise`, [P] for `to_reference` (whose O_BB holds the one reference)"""
    if result["O_AB"].dim() == 1:
        return result["O_AB"] / (alpha * result["O_AA"] + (1.0 - alpha) * result["O_BB"])
    return result["O_AB"] / (alpha * result["O_AA"][:, None] + (1.0 - alpha) * result["O_BB"][None, :])


def quat_to_matrix(quat: torch.Tensor) -> torch.Tensor:
    w, x, y, z = quat.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(quat.shape[:-1] + (3, 3))


def apply(x: torch.Tensor, quat: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """x' = R(quat) x + t in float64, for x [..., A, 3] and quat [..., 4] (w, x, y, z), t [..., 3]"""
    R = quat_to_matrix(quat.double())
    return x.double() @ R.transpose(-1, -2) + t.double()[..., None, :]


class ShapeOverlap:
    """The scorer of one molecule (`spec`) against itself or another.  Every method takes device tensors, returns device tensors and
    never reads back."""

    def __init__(self, spec: ShapeSpec):
        if not isinstance(spec, ShapeSpec):
            raise ValueError(f"ShapeOverlap takes a ShapeSpec, got {type(spec).__name__}")
        self.spec = spec

    n_atoms = property(lambda self: self.spec.n_atoms)
    ligand_idx = property(lambda self: self.spec.ligand_idx)

    # ------------------------------------------------------------------ one side
    @staticmethod
    def _prepare(spec: ShapeSpec, x: torch.Tensor, what: str):
        if not isinstance(spec, ShapeSpec):
            raise ValueError(f"ShapeOverlap.{what}: expected a ShapeSpec, got {type(spec).__name__}")
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[2] != 3 or not x.is_cuda:
            raise ValueError(f"ShapeOverlap.{what}: structures must be a device tensor [n,A,3], got {tuple(getattr(x, 'shape', ()))}")
        n, A = int(x.shape[0]), int(x.shape[1])
        if not 1 <= n <= MAX_STRUCTURES or not 1 <= A <= MAX_POSE_ATOMS:
            raise ValueError(f"ShapeOverlap.{what}: {n} structures of {A} atoms; the kernels take 1 .. {MAX_STRUCTURES} of 1 .. {MAX_POSE_ATOMS}")
        L, F = spec.n_atoms, spec.n_features
        if spec.ligand_idx is None:
            if A != L:
                raise ValueError(f"ShapeOverlap.{what}: the spec holds {L} atoms, the structures {A}")
        elif int(spec.ligand_idx.max()) >= A:
            raise ValueError(f"ShapeOverlap.{what}: the spec names atom {int(spec.ligand_idx.max())}, the structures hold {A}")
        t = spec.tables(x.device)
        lig = t["lig"] if t["lig"] is not None else torch.arange(L, dtype=torch.int32, device=x.device)
        x = x.float().contiguous()
        L_ = ops._lib.init()
        numel = L_.pd_shape_workspace_numel(n, L, F)
        ops.check(min(numel, 0), "pd_shape_workspace_numel")
        ws = torch.empty(numel, dtype=torch.float64, device=x.device)
        ops.check(L_.pd_shape_prepare(ops.ptr(x), ops.ptr(lig), ops.ptr(t["alpha"]), ops.ptr(t["start"]) if F else None,
                                      ops.ptr(t["atom"]) if F else None, ops.ptr(t["kind"]) if F else None, COLOR_ALPHA, ops.ptr(ws),
                                      numel, n, A, L, F, ops.stream()), "pd_shape_prepare")
        return dict(ws=ws, numel=numel, alpha=t["alpha"], kind=t["kind"] if F else None, n=n, L=L, F=F)

    @staticmethod
    def _side(s):
        return [ops.ptr(s["ws"]), s["numel"], ops.ptr(s["alpha"]), ops.ptr(s["kind"]), s["n"], s["L"], s["F"]]

    @staticmethod
    def _self(s):
        v = s["ws"].view(s["n"], -1)[:, -2:]
        return v[:, 0], v[:, 1]

    def _overlap(self, a, b, pairwise, per_atom=False):
        dev = a["ws"].device
        n, C = a["n"], b["n"]
        new = lambda dt: torch.empty((n, C), dtype=dt, device=dev)
        out = {"O_AB": new(torch.float64), "C_AB": new(torch.float64), "shape_tanimoto": new(torch.float32),
               "color_tanimoto": new(torch.float32), "combo": new(torch.float32)}
        share = torch.empty((n, a["L"]), dtype=torch.float64, device=dev) if per_atom else None
        ops.check(ops._lib.init().pd_shape_overlap(*self._side(a), *self._side(b), COLOR_ALPHA, 1 if pairwise else 0,
                                                   *(ops.ptr(out[k]) for k in ("O_AB", "C_AB", "shape_tanimoto", "color_tanimoto", "combo")),
                                                   ops.ptr(share), ops.stream()), "pd_shape_overlap")
        out["O_AA"], out["C_AA"] = self._self(a)
        out["O_BB"], out["C_BB"] = self._self(b)
        if per_atom:
            out["atom_share"] = share
        return out

    # ------------------------------------------------------------------ the scores
    def cross(self, x: torch.Tensor, other_spec: ShapeSpec, y: torch.Tensor) -> Dict[str, torch.Tensor]:
        """x [P,A,3] of this molecule against y [C,A',3] of `other_spec`, in place -> O_AB, C_AB float64 [P,C], shape_tanimoto,
        color_tanimoto, combo fp32 [P,C], and the self-overlaps O_AA, C_AA [P], O_BB, C_BB [C] (float64)"""
        return self._overlap(self._prepare(self.spec, x, "cross"), self._prepare(other_spec, y, "cross"), False)

    def pairwise(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """x [P,A,3] against itself: the matrices of `cross`, symmetric by construction, shape diagonal exactly 1"""
        a = self._prepare(self.spec, x, "pairwise")
        return self._overlap(a, a, True)

    def to_reference(self, x: torch.Tensor, other_spec: ShapeSpec, y_ref: torch.Tensor, per_atom: bool = False) -> Dict[str, torch.Tensor]:
        """x [P,A,3] against ONE structure y_ref [A',3] of `other_spec` -> the results of `cross` as vectors [P] and, with `per_atom`,
        atom_share float64 [P,L]: each atom's part of O_AB"""
        if not isinstance(y_ref, torch.Tensor) or y_ref.dim() != 2:
            raise ValueError(f"ShapeOverlap.to_reference: y_ref must be one structure [A',3], got {tuple(getattr(y_ref, 'shape', ()))}")
        out = self._overlap(self._prepare(self.spec, x, "to_reference"), self._prepare(other_spec, y_ref[None], "to_reference"), False, per_atom)
        return {k: (v[:, 0] if v.dim() == 2 and k != "atom_share" else v) for k, v in out.items()}

    def overlay(self, x: torch.Tensor, other_spec: ShapeSpec, y: torch.Tensor, max_iters: int = 50, grad_tol: float = 1e-4,
                max_step: float = 1.0) -> Dict[str, torch.Tensor]:
        """the rigid motion of every x [P,A,3] that maximises its shape overlap with every y [C,A',3] (module docstring) -> quat float64
        [P,C,4] (w, x, y, z; w >= 0) and t float64 [P,C,3] with x' = R x + t (`apply`), x_fit float64 [P,C,L,3] (the molecule's atoms as fitted), shape_tanimoto, color_tanimoto, combo fp32 [P,C]
        at the optimum, overlap and overlap_start (in place) float64, best_start, iterations, evaluations, status int32"""
        if int(max_iters) < 0 or not grad_tol >= 0.0 or not max_step > 0.0:
            raise ValueError("ShapeOverlap.overlay: max_iters >= 0, grad_tol >= 0 and max_step > 0 are required")
        for s in (self.spec, other_spec):
            if isinstance(s, ShapeSpec) and s.n_atoms > MAX_OVERLAY_ATOMS:
                raise ValueError(f"ShapeOverlap.overlay: {s.n_atoms} atoms; the overlay takes at most {MAX_OVERLAY_ATOMS}")
        a, b = self._prepare(self.spec, x, "overlay"), self._prepare(other_spec, y, "overlay")
        dev, n, C = x.device, a["n"], b["n"]
        L_ = ops._lib.init()
        numel = L_.pd_shape_overlay_workspace_numel(n, C, a["L"])
        ops.check(min(numel, 0), "pd_shape_overlay_workspace_numel")
        ws = torch.empty(numel, dtype=torch.float64, device=dev)
        new = lambda dt, *tail: torch.empty((n, C) + tail, dtype=dt, device=dev)
        tr, sc, fit = new(torch.float64, 7), new(torch.float32, 3), new(torch.float64, a["L"], 3)
        out = {"overlap": new(torch.float64), "overlap_start": new(torch.float64), "best_start": new(torch.int32),
               "iterations": new(torch.int32), "evaluations": new(torch.int32), "status": new(torch.int32)}
        ops.check(L_.pd_shape_overlay(*self._side(a), *self._side(b), COLOR_ALPHA, int(max_iters), float(grad_tol), float(max_step),
                                      ops.ptr(ws), numel, ops.ptr(tr), ops.ptr(fit), ops.ptr(sc), *(ops.ptr(v) for v in out.values()), ops.stream()),
                  "pd_shape_overlay")
        out.update(quat=tr[..., :4], t=tr[..., 4:], x_fit=fit, shape_tanimoto=sc[..., 0], color_tanimoto=sc[..., 1], combo=sc[..., 2])
        return out


# ------------------------------------------------------------------ the driver's keyword
def _unpack(shape):
    return (shape[0], shape[1]) if isinstance(shape, (tuple, list)) else (shape, None)


def check_redock_shape(shape, batch) -> None:
    """redock(shape=): raise ValueError unless it is a ShapeOverlap of the batch's ligand, optionally with (other_spec, y_ref)"""
    if shape is None:
        return
    if isinstance(shape, (tuple, list)) and len(shape) != 2:
        raise ValueError("shape= takes a ShapeOverlap or (ShapeOverlap, (other_spec, y_ref))")
    so, ref = _unpack(shape)
    if not isinstance(so, ShapeOverlap):
        raise ValueError(f"shape= takes a shape.ShapeOverlap, got {type(so).__name__}")
    if ref is not None and not (isinstance(ref, (tuple, list)) and len(ref) == 2 and isinstance(ref[0], ShapeSpec)
                                and isinstance(ref[1], torch.Tensor) and tuple(ref[1].shape[1:]) == (3,)):
        raise ValueError("shape=: the reference is (other_spec, y_ref [A',3])")
    from .driver import ligand_atom_mask
    n = int(ligand_atom_mask(batch).sum())
    if so.n_atoms != n:
        raise ValueError(f"shape= was built over {so.n_atoms} atoms, the batch's ligand holds {n}")


def score_shape(shape, aligned, batch, ligand_idx, out) -> dict:
    """redock(shape=): {"shape": shape_tanimoto, color_tanimoto, combo [n] of the kept poses to the reference (default: the ligand of
    `x_gt`, same spec), pairwise (the dict of `ShapeOverlap.pairwise`)}, "order_shape": the pose ids by descending combo
    (`rank_by_score` of its negative; valid poses first with `validity=`)}"""
    from .ranking import rank_by_score
    so, ref = _unpack(shape)
    x = aligned if so.ligand_idx is not None else aligned[:, ligand_idx.long()]
    if ref is None:
        gt = batch["x_gt"].float()
        ref = (so.spec, gt if so.ligand_idx is not None else gt[ligand_idx.long()])
    got = so.to_reference(x, ref[0], ref[1].to(aligned.device).float())
    res = {k: got[k] for k in ("shape_tanimoto", "color_tanimoto", "combo")}
    res["pairwise"] = so.pairwise(x)
    valid = out["validity"]["valid"] if "validity" in out else None
    return {"shape": res, "order_shape": rank_by_score(-res["combo"], valid=valid)}
