"""Does the ligand have the right CONFORMATION, wherever it sits?  The best-fit ligand RMSD on the device (kernel `pd_bestfit_rmsd`,
csrc/bestfit_rmsd.hip; tests/bestfit_rmsd_ref.py is the written definition): the ligand-only RMSD minimised over rigid superpositions
and over the ligand's automorphisms - what RDKit calls `GetBestRMS`, and what PoseBusters, PLINDER and the conformer-generator
benchmarks report.  Every other ligand RMSD of the package (`ranking.pairwise_ligand_rmsd`, `pd_sym_rmsd`) is taken in a fixed frame,
after the pocket-weighted Kabsch of the receptor: it says how far the ligand is from where it should be.  A pose 4 A off with the
bioactive conformer is a placement error; a pose in the pocket with a wrong ring pucker or a flipped amide is a conformer error - this
module measures the second.

    a, b [L,3]      two ligands, each centred on its unweighted centroid in float64; G = sum of squared norms
    msd(a, b, m)  = min over proper rotations R of (1/L) sum_k |R a[k] - b[perm[m][k]]|^2
                  = (G_a + G_b - 2 lambda_max(N(a, b o perm_m))) / L                  (Horn 1987; lambda_max by cyclic Jacobi in float64)
    bestfit(a, b) = sqrt(max(0, min_m msd)), the smallest m wins a tie, rounded once to fp32

`BestFitRmsd(ligand_idx, symmetry)` is an immutable spec; `cross`, `to_reference` and `pairwise` return device tensors and read nothing
back.  `pairwise` is symmetric with a zero diagonal and goes to `PoseClusters.cluster` as it is.

**Caveats.**  Heavy atoms only (the atoms the spec names).  A table cut at `max_perms` (`symmetry.complete` False) makes every value an
upper bound.  Proper rotations only: an enantiomer does not match, as it should not.  Where lambda_max is degenerate (collinear atoms,
L <= 2) the rotation returned is one of the optimal ones.  Out of scope: weighted fits, fitting on a substructure, torsion-fingerprint
deviation.  Limits: L <= 1024, 65535 table rows, 65535 structures on either side.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _ligand_sides as sides
from . import ops
from ._ligand_sides import MAX_STRUCTURES

__all__ = ["BestFitRmsd", "MAX_ATOMS", "MAX_STRUCTURES", "quat_apply"]

#: limits of the kernel (csrc/bestfit_rmsd.hip)
MAX_ATOMS = 1024
_WHO = dict(name="BestFitRmsd", takes="the kernel takes", max_atoms=MAX_ATOMS)      # for the messages and checks of _ligand_sides


def quat_apply(quat: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """rotate v [..., L, 3] by the unit quaternions quat [..., 4] = (w, x, y, z), in the dtype of quat (torch arithmetic)"""
    w, x, y, z = (quat[..., k, None, None] for k in range(4))
    v = v.to(quat.dtype)
    vx, vy, vz = v[..., 0:1], v[..., 1:2], v[..., 2:3]
    rx = (1 - 2 * (y * y + z * z)) * vx + 2 * (x * y - w * z) * vy + 2 * (x * z + w * y) * vz
    ry = 2 * (x * y + w * z) * vx + (1 - 2 * (x * x + z * z)) * vy + 2 * (y * z - w * x) * vz
    rz = 2 * (x * z - w * y) * vx + 2 * (y * z + w * x) * vy + (1 - 2 * (x * x + y * y)) * vz
    return torch.cat([rx, ry, rz], -1)


class BestFitRmsd:
    """An immutable spec: `ligand_idx` (the L ligand atoms of a pose [A,3], in the order of the symmetry table; None: a pose holds the
    ligand alone) and `symmetry` (a `symmetry.LigandSymmetry`; None: the identity).  The indices are checked here, on the host, once:
    the kernel never sees one it could follow outside a structure."""

    __slots__ = ("ligand_idx", "symmetry", "n_atoms", "_idx")

    def __init__(self, ligand_idx=None, symmetry=None):
        idx = sides.host_idx(ligand_idx, "ligand_idx", "BestFitRmsd")
        if symmetry is not None and not (hasattr(symmetry, "table") and hasattr(symmetry, "n_atoms")):
            raise ValueError(f"BestFitRmsd: symmetry= takes a symmetry.LigandSymmetry, got {type(symmetry).__name__}")
        n = None if idx is None else int(idx.shape[0])
        if symmetry is not None:
            if n is not None and symmetry.n_atoms != n:
                raise ValueError(f"BestFitRmsd: the symmetry table is over {symmetry.n_atoms} atoms, ligand_idx names {n}")
            n = int(symmetry.n_atoms)
        if n is not None and n > MAX_ATOMS:
            raise ValueError(f"BestFitRmsd: {n} ligand atoms; the kernel takes up to {MAX_ATOMS}")
        object.__setattr__(self, "ligand_idx", None if idx is None else tuple(int(v) for v in idx))
        object.__setattr__(self, "symmetry", symmetry)
        object.__setattr__(self, "n_atoms", n)
        object.__setattr__(self, "_idx", {})

    def __setattr__(self, name, value):
        raise AttributeError("BestFitRmsd is immutable")

    def __repr__(self):
        return f"BestFitRmsd(n_atoms={self.n_atoms}, symmetry={self.symmetry!r})"

    @property
    def symmetry_complete(self) -> bool:
        """False: the table was cut, every value is an upper bound"""
        return sides.symmetry_complete(self.symmetry)

    # ------------------------------------------------------------------ plumbing
    def _device_idx(self, idx, device):
        if idx is None:
            return None
        key = (idx.tobytes(), str(device))
        t = self._idx.get(key)
        if t is None:
            t = torch.from_numpy(idx.astype(np.int32)).to(device)
            self._idx[key] = t
        return t

    def _launch(self, xa, ia, xb, ib, L, symmetric, detail):
        dev = xa.device
        na, Aa = xa.shape[0], xa.shape[1]
        nb, Ab = (na, Aa) if symmetric else (xb.shape[0], xb.shape[1])
        L_ = ops._lib.init()
        numel = L_.pd_bestfit_rmsd_workspace_numel(na, nb, L)
        ops.check(min(numel, 0), "pd_bestfit_rmsd_workspace_numel")
        ws = torch.empty(numel, dtype=torch.float64, device=dev)
        D = torch.empty(na, nb, dtype=torch.float32, device=dev)
        bp = torch.empty(na, nb, dtype=torch.int32, device=dev) if detail else None
        q = torch.empty(na, nb, 4, dtype=torch.float64, device=dev) if detail else None
        table, M = (None, 1) if self.symmetry is None else (self.symmetry.table(dev), self.symmetry.n_perms)
        with torch.cuda.device(dev):
            ops.check(L_.pd_bestfit_rmsd(ops.ptr(xa), ops.ptr(self._device_idx(ia, dev)), ops.ptr(xb), ops.ptr(self._device_idx(ib, dev)),
                                         ops.ptr(table), ops.ptr(ws), numel, ops.ptr(D), ops.ptr(bp), ops.ptr(q), na, nb, Aa, Ab, L, M,
                                         1 if symmetric else 0, ops.stream()), "pd_bestfit_rmsd")
        return D, bp, q

    def _cross(self, x, targets, target_idx, detail):
        xa, ia, xb, ib, L = sides.sides(self, x, targets, target_idx, **_WHO)
        D, bp, q = self._launch(xa, ia, xb, ib, L, False, detail)
        return D, bp, q, ia, ib, L

    # ------------------------------------------------------------------ the three calls
    def cross(self, x: torch.Tensor, targets: torch.Tensor, target_idx=None, detail: bool = False) -> Dict[str, torch.Tensor]:
        """x [n,A,3] (gathered through `ligand_idx`) against targets [C,A',3] gathered through `target_idx` - or through `ligand_idx`
        when they are whole poses - or [C,L,3] taken as they are -> `D` fp32 [n,C], `nearest` int64 [n] (the argmin over C: a NaN never
        wins, an all-NaN row gives -1, the smallest index wins a tie) and `nearest_rmsd` fp32 [n] (NaN for such a row); with
        `detail=True` also `best_perm` int32 [n,C] and `quat` float64 [n,C,4] (R(quat) pose ~ target o perm).  The rows are fixed, the
        targets permuted.  Nothing is read back."""
        D, bp, q, _, _, _ = self._cross(x, targets, target_idx, detail)
        near, near_r = sides.nearest(D)
        out = {"D": D, "nearest": near, "nearest_rmsd": near_r}
        if detail:
            out.update(best_perm=bp, quat=q)
        return out

    def to_reference(self, x: torch.Tensor, x_ref: torch.Tensor) -> Dict[str, torch.Tensor]:
        """`cross` with the one target x_ref [A,3] / [L,3] -> `rmsd` fp32 [n], `best_perm` int32 [n], `quat` float64 [n,4] and `x_fit`
        fp32 [n,L,3]: each pose's ligand rotated and translated onto the reference's (torch arithmetic from `quat` in float64, rounded
        once: plumbing, not a kernel; atom k of `x_fit` lies on atom perms[best_perm][k] of the reference)."""
        if not isinstance(x_ref, torch.Tensor) or x_ref.dim() != 2 or x_ref.shape[1] != 3:
            raise ValueError(f"BestFitRmsd.to_reference: x_ref must be [A,3], got {tuple(getattr(x_ref, 'shape', ()))}")
        D, bp, q, ia, ib, L = self._cross(x, x_ref[None], None, True)
        dev = D.device
        lig = x.to(dev).double() if ia is None else x.to(dev).double()[:, self._device_idx(ia, dev).long()]
        ref = x_ref.to(dev).double() if ib is None else x_ref.to(dev).double()[self._device_idx(ib, dev).long()]
        fit = quat_apply(q[:, 0], lig - lig.mean(1, keepdim=True)) + ref.mean(0)
        return {"rmsd": D[:, 0], "best_perm": bp[:, 0], "quat": q[:, 0], "x_fit": fit.float()}

    def pairwise(self, x: torch.Tensor) -> torch.Tensor:
        """x [n,A,3] -> D fp32 [n,n], symmetric with an exact zero diagonal (pose i fixed, pose j permuted for i < j, mirrored);
        `PoseClusters.cluster` takes it as it is"""
        ia = sides.own_idx(self)
        xa, L = sides.structures(x, "x", ia, self.n_atoms, **_WHO)
        return self._launch(xa, ia, None, None, L, True, False)[0]

