"""What `bestfit.BestFitRmsd` and `torsions.TorsionFingerprint` share on the host: the checks of an index list and of a stack of
structures before a kernel sees them, the "whole poses as targets" rule of their `cross` calls, and the argmin over the targets.
`name` is the calling class's name, for the messages."""
from __future__ import annotations

import numpy as np
import torch

#: structures on either side of a launch (csrc/bestfit_rmsd.hip, csrc/torsion.hip)
MAX_STRUCTURES = 65535


def host_idx(idx, what, name):
    """an index list as a host int64 array [L], or None"""
    if idx is None:
        return None
    if isinstance(idx, torch.Tensor):
        if idx.dtype.is_floating_point or idx.dtype == torch.bool:
            raise ValueError(f"{name}: {what} must hold integer atom indices, got {idx.dtype}")
        idx = idx.detach().cpu().numpy()
    a = np.asarray(idx)
    if a.dtype.kind not in "iu" or a.ndim != 1 or a.shape[0] < 1:
        raise ValueError(f"{name}: {what} must be a non-empty 1-D list of integer atom indices")
    if int(a.min()) < 0:
        raise ValueError(f"{name}: {what} holds a negative index")
    return a.astype(np.int64)


def own_idx(spec):
    """the spec's `ligand_idx` (a tuple or None) as a host int64 array, or None"""
    return None if spec.ligand_idx is None else np.asarray(spec.ligand_idx, dtype=np.int64)


def symmetry_complete(symmetry) -> bool:
    """False: the table was cut, every value is an upper bound"""
    return True if symmetry is None else bool(symmetry.complete)


def structures(x, what, idx, L, name, takes, device=None, max_atoms=None):
    """x [n,A,3] -> (fp32 contiguous device tensor, the number of ligand atoms it names) after the host checks: idx (host int64 or None:
    the structure is the ligand itself) stays inside the A atoms and names L of them (L None: whatever it names), `max_atoms` at the
    most when the caller's kernel has such a limit.  `takes`: "the kernel takes" / "the kernels take", for the messages."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[2] != 3 or not x.dtype.is_floating_point:
        raise ValueError(f"{name}: {what} must be a floating-point tensor [n,A,3], got {tuple(getattr(x, 'shape', ()))}")
    n, A = int(x.shape[0]), int(x.shape[1])
    if not 1 <= n <= MAX_STRUCTURES:
        raise ValueError(f"{name}: {n} structures in {what}; {takes} 1 .. {MAX_STRUCTURES}")
    have = A if idx is None else int(idx.shape[0])
    if L is not None and have != L:
        raise ValueError(f"{name}: {what} names {have} ligand atoms, expected {L}")
    if idx is not None and int(idx.max()) >= A:
        raise ValueError(f"{name}: an index of {what} ({int(idx.max())}) leaves its {A} atoms")
    if max_atoms is not None and not 1 <= have <= max_atoms:
        raise ValueError(f"{name}: {have} ligand atoms; {takes} 1 .. {max_atoms}")
    if device is not None and x.device.type == "cpu":
        x = x.to(device)                                      # targets may come from the host, as redock's template pool may
    if not x.is_cuda or (device is not None and x.device != device):
        raise ValueError(f"{name}: {what} must be on the GPU{'' if device is None else ' of the poses'}, got a tensor on {x.device}")
    return x.float().contiguous(), have


def sides(spec, x, targets, target_idx, name, takes, max_atoms=None):
    """the two sides of a `cross` call, checked: (xa, ia, xb, ib, L) - x through the spec's own index list ia, the targets through
    `target_idx` when given, through ia when they are whole poses, as they are when they are [C,L,3]"""
    ia = own_idx(spec)
    xa, L = structures(x, "x", ia, spec.n_atoms, name, takes, max_atoms=max_atoms)
    ib = host_idx(target_idx, "target_idx", name)
    if ib is None and ia is not None and isinstance(targets, torch.Tensor) and targets.dim() == 3 and targets.shape[1] != L:
        ib = ia                                               # whole poses as targets: the ligand sits where it sits in x
    xb, _ = structures(targets, "targets", ib, L, name, takes, device=xa.device, max_atoms=max_atoms)
    return xa, ia, xb, ib, L


def nearest(D):
    """D [n,C] -> (int64 [n], fp32 [n]): the argmin over C and its value - a NaN never wins, an all-NaN row gives -1 and NaN, the
    smallest index wins a tie"""
    key = torch.where(torch.isnan(D), torch.full_like(D, float("inf")), D)
    near = torch.argmin(key, dim=1)
    first = (key == key.gather(1, near[:, None])).to(torch.int8).argmax(1)      # the first of equal minima, whatever argmin picked
    value = D.gather(1, first[:, None])[:, 0]
    return torch.where(torch.isnan(value), torch.full_like(first, -1), first), value
