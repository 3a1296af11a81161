"""Time BestFitRmsd.pairwise and .cross (csrc/bestfit_rmsd.hip) with device events at the three shapes NOTES.md quotes - 64 poses pairwise
at L = 32 ligand atoms with M = 1 and with M = 64 table rows, and 64 poses against 128 templates - next to
ranking.pairwise_ligand_rmsd (pd_sym_rmsd) at the same n, L, M, for scale only: that kernel superposes nothing.  Each timed window is
`--calls` back-to-back calls between two events, after a warm-up; a line reports the median and the spread of `--windows` windows per call.

    python tools/bestfit_rmsd_time.py [--out file]
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
from physdock_amd.ranking import pairwise_ligand_rmsd  # noqa: E402
from physdock_amd.symmetry import LigandSymmetry  # noqa: E402
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
    poses = torch.from_numpy((rng.standard_normal((n, A, 3)) * 4 + 70).astype(np.float32)).cuda()
    pool = torch.from_numpy((rng.standard_normal((C, Lg, 3)) * 4).astype(np.float32)).cuda()
    lig = torch.from_numpy(idx).cuda()
    lines = []
    for M in (1, 64):
        sym = LigandSymmetry.from_permutations(np.stack([np.arange(Lg)] + [rng.permutation(Lg) for _ in range(M - 1)]), device="cuda")
        spec = BestFitRmsd(idx, sym)
        fit = per_call_us(lambda: spec.pairwise(poses), args.calls, args.windows)
        fixed = per_call_us(lambda: pairwise_ligand_rmsd(poses, lig, symmetry=sym), args.calls, args.windows)
        lines.append(f"n={n} L={Lg} M={M}: BestFitRmsd.pairwise {fit[0]:.1f} us per call (min {fit[1]:.1f}, max {fit[2]:.1f} over "
                     f"{args.windows} windows of {args.calls} calls; two kernels plus two allocations); pd_sym_rmsd at the same shape "
                     f"{fixed[0]:.1f} us (min {fixed[1]:.1f}, max {fixed[2]:.1f})")
        if M == 1:
            cr = per_call_us(lambda: spec.cross(poses, pool), args.calls, args.windows)
            lines.append(f"n={n} x C={C} templates L={Lg} M=1: BestFitRmsd.cross {cr[0]:.1f} us per call (min {cr[1]:.1f}, max {cr[2]:.1f}; "
                         f"two kernels plus the argmin in torch)")
    for line in lines:
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
