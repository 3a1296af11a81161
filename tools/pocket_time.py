"""Time PocketGrid.measure (csrc/pocket.hip) with device events at P = 64 poses of A = 2048 atoms (L = 50 ligand atoms, R = 256
residues of eight atoms) on a 32^3 and on a 48^3 lattice of 1 A, next to BuriedSurface.measure (pd_buried_surface, n = 96 points) on the
same poses in the same run, for scale: the other measure of the package that tests every pose's ligand surroundings against its whole
receptor.  Each timed window is `--calls` back-to-back calls between two events, after a warm-up; a line reports the median and the
spread of `--windows` windows per call.  The receptor is the jittered 3.8 A lattice of tools/sasa_time.py with a cavity of 6 A around the
ligand's atoms, so that the poses have a site.

    python tools/pocket_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from physdock_amd.pocket import PocketGrid  # noqa: E402
from physdock_amd.surface import BuriedSurface  # noqa: E402
from sasa_time import per_call_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    n_pose, Lg, A = 64, 50, 2048
    rng = np.random.default_rng(50)
    side = 14
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    sites = (grid - (side - 1) / 2.0) * 3.8
    sites = sites[np.sqrt((sites ** 2).sum(-1)) >= 6.0]                                 # the cavity
    sites = sites[np.argsort((sites ** 2).sum(-1), kind="stable")][:A - Lg]
    lig_idx = np.sort(rng.permutation(A)[:Lg])
    rec = np.setdiff1d(np.arange(A), lig_idx)
    x = np.empty((n_pose, A, 3))
    x[:, lig_idx] = rng.normal(size=(n_pose, Lg, 3)) * 1.6
    x[:, rec] = sites + rng.uniform(-0.6, 0.6, (n_pose, A - Lg, 3))
    elements = rng.choice([6, 6, 6, 7, 8, 16], A)
    residue_of = np.arange(A) // 8
    x = torch.from_numpy(x.astype(np.float32)).cuda()
    surface = BuriedSurface.from_arrays(elements, lig_idx, np.ones(A), residue_of, device="cuda")
    lines = []
    for n in (32, 48):
        g = PocketGrid.from_arrays(elements, lig_idx, np.ones(A), residue_of, n=n, device="cuda")
        out = g.measure(x)
        assert bool((out["ok"] == 1).all())
        pk = per_call_us(lambda: g.measure(x), args.calls, args.windows)
        lean = per_call_us(lambda: g.measure(x, maps=False), args.calls, args.windows)
        bs = per_call_us(lambda: surface.measure(x), args.calls, args.windows)
        c = out["counts"].float().mean(0).tolist()
        lines.append(f"P={n_pose} L={Lg} A={A} R={g.n_residues} n={n} h={g.h:g}: PocketGrid.measure {pk[0]:.1f} us per call (min {pk[1]:.1f}, max "
                     f"{pk[2]:.1f} over {args.windows} windows of {args.calls} calls; four kernels plus twelve allocations; untuned), "
                     f"{pk[0] / n_pose:.2f} us per pose; maps=False {lean[0]:.1f} us; BuriedSurface.measure (n_points=96) on the same poses "
                     f"{bs[0]:.1f} us (min {bs[1]:.1f}, max {bs[2]:.1f}); mean per pose: n_solid {c[0]:.0f}, n_pocket {c[2]:.0f}, n_site {c[3]:.0f}, "
                     f"n_occupied {c[4]:.0f}, components {c[6]:.1f}, lining residues {float(out['lining_residues'].float().mean()):.1f}, "
                     f"truncated {int(out['truncated'].sum())} of {n_pose}")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
