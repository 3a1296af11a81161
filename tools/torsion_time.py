"""Time TorsionFingerprint.pairwise and .cross (csrc/torsion.hip) with device events at the three shapes NOTES.md quotes - 64 poses pairwise
at L = 32 ligand atoms with M = 1 and with M = 64 table rows, and 64 poses against 128 templates - next to BestFitRmsd (pd_bestfit_rmsd)
at the same shapes on the same run, for scale: the other conformation metric of the package.  The ligand is a chain of 32 atoms with a
six-ring at one end (26 entries: 25 rotatable bonds and the ring; 32 base quadruples); the 64-row table is random (the identity first), as in tools/bestfit_rmsd_time.py,
so that the closure holds many more quadruples than a real group would give.  Each timed window is `--calls` back-to-back calls between
two events, after a warm-up; a line reports the median and the spread of `--windows` windows per call.

    python tools/torsion_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from physdock_amd.bestfit import BestFitRmsd  # noqa: E402
from physdock_amd.symmetry import LigandSymmetry  # noqa: E402
from physdock_amd.torsions import TorsionFingerprint  # noqa: E402
from validity_time import per_call_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    n, Lg, A, C = 64, 32, 300, 128
    rng = np.random.default_rng(61)
    idx = np.sort(rng.permutation(A)[:Lg]).astype(np.int32)
    bonds = [(k, k + 1) for k in range(Lg - 1)] + [(Lg - 1, Lg - 6)]
    poses = torch.from_numpy((rng.standard_normal((n, A, 3)) * 4 + 70).astype(np.float32)).cuda()
    pool = torch.from_numpy((rng.standard_normal((C, Lg, 3)) * 4).astype(np.float32)).cuda()
    lines = []
    for M in (1, 64):
        sym = LigandSymmetry.from_permutations(np.stack([np.arange(Lg)] + [rng.permutation(Lg) for _ in range(M - 1)]), device="cuda")
        spec, fit = TorsionFingerprint.from_bonds(Lg, bonds, ligand_idx=idx, symmetry=sym), BestFitRmsd(idx, sym)
        shape = f"T={spec.n_entries} Q={spec.quads.shape[0]}"
        tf = per_call_us(lambda: spec.pairwise(poses), args.calls, args.windows)
        bf = per_call_us(lambda: fit.pairwise(poses), args.calls, args.windows)
        lines.append(f"n={n} L={Lg} M={M} {shape}: TorsionFingerprint.pairwise {tf[0]:.1f} us per call (min {tf[1]:.1f}, max {tf[2]:.1f} over "
                     f"{args.windows} windows of {args.calls} calls; two kernels plus two allocations); BestFitRmsd.pairwise at the same "
                     f"shape {bf[0]:.1f} us (min {bf[1]:.1f}, max {bf[2]:.1f})")
        if M == 1:
            tc_ = per_call_us(lambda: spec.cross(poses, pool), args.calls, args.windows)
            bc = per_call_us(lambda: fit.cross(poses, pool), args.calls, args.windows)
            lines.append(f"n={n} x C={C} templates L={Lg} M=1 {shape}: TorsionFingerprint.cross {tc_[0]:.1f} us per call (min {tc_[1]:.1f}, max "
                         f"{tc_[2]:.1f}; three kernels plus the argmin in torch); BestFitRmsd.cross {bc[0]:.1f} us (min {bc[1]:.1f}, max "
                         f"{bc[2]:.1f})")
    for line in lines:
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
