"""Time ShapeOverlap.pairwise, .cross and .overlay (csrc/shape_overlap.hip) with device events at the three shapes NOTES.md quotes: 64 poses
of 32 atoms pairwise, 64 poses against 128 structures, and the overlay of 64 poses on 8 structures (five starts each, max_iters 50).
Each timed window is `--calls` back-to-back calls between two events (2000 by default: a third of a second at these shapes; the
overlay takes a twentieth of them), after a warm-up; a line reports the median and the spread of
`--windows` windows per call.  The molecules are the seeded chains of tests/shape_overlap_ref.py with its default feature tables.

    python tools/shape_overlap_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shape_overlap_cases as cases  # noqa: E402
import shape_overlap_ref as ref  # noqa: E402
from physdock_amd.shape import ShapeOverlap, ShapeSpec  # noqa: E402
from validity_time import per_call_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    n, Lg, C = 64, 32, 128
    y, radii, feats = ref.molecule(Lg, 1)
    z, radii2, feats2 = ref.molecule(Lg, 2)
    x = torch.from_numpy(np.stack([cases.rigid(y, p)[0] for p in range(n)])).cuda()
    pool = torch.from_numpy(np.stack([cases.rigid(z, 100 + p)[0] for p in range(C)])).cuda()
    so = ShapeOverlap(ShapeSpec.from_tables(Lg, feats, radii))
    other = ShapeSpec.from_tables(Lg, feats2, radii2)
    lines = []
    pw = per_call_us(lambda: so.pairwise(x), args.calls, args.windows)
    lines.append(f"n={n} L={Lg} F={len(feats)}: ShapeOverlap.pairwise {pw[0]:.1f} us per call (min {pw[1]:.1f}, max {pw[2]:.1f} over "
                 f"{args.windows} windows of {args.calls} calls; two kernels plus the allocations)")
    cr = per_call_us(lambda: so.cross(x, other, pool), args.calls, args.windows)
    lines.append(f"n={n} x C={C} L={Lg}: ShapeOverlap.cross {cr[0]:.1f} us per call (min {cr[1]:.1f}, max {cr[2]:.1f}; three kernels plus the allocations)")
    got = so.overlay(x, other, pool[:8])
    ov = per_call_us(lambda: so.overlay(x, other, pool[:8]), max(args.calls // 20, 1), args.windows)
    lines.append(f"n={n} x C=8 L={Lg}: ShapeOverlap.overlay {ov[0]:.1f} us per call (min {ov[1]:.1f}, max {ov[2]:.1f}; four kernels plus the allocations, {max(args.calls // 20, 1)} calls per window, "
                 f"{int(got['evaluations'].sum())} evaluations in the winning starts, mean iterations {float(got['iterations'].float().mean()):.1f})")
    for line in lines:
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
