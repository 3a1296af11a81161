"""Time BuriedSurface.measure (csrc/sasa.hip) with device events at P = 64 poses, L = 50 ligand atoms, A = 2048 pose atoms, R = 256
residues of eight atoms, at n = 96 and n = 960 points per atom, next to the same definition written as torch operations on the same
GPU (points of a slab of atoms, cdist against every atom, compare, any over the same and over the other class).  The torch
expression tests every point against every atom - 2.6e10 tests at n = 96 and 64 poses - so it is timed on `--torch-poses` poses and
reported per pose beside the kernels' time per pose; it is the yardstick printed beside the kernels, not a target.  Each timed
window is `--calls` back-to-back calls between two events, after a warm-up; the line reports the median and the spread of
`--windows` windows per call.  The receptor is a jittered 3.8 A lattice with the ligand's atoms on sites near its centre.

    python tools/sasa_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physdock_amd.surface import BuriedSurface  # noqa: E402


def per_call_us(fn, calls, windows, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / calls)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def torch_form(x, t, rows=1536):
    """(n_free, n_buried) int64 [P,A] of the definition as torch operations: every point against every atom"""
    cls, R, unit = t["cls"], t["R"], t["unit"]
    n, A = unit.shape[0], x.shape[1]
    live = cls != 0
    idx = torch.arange(A, device=x.device)
    slab = max(rows // n, 1)                                                            # rows of cdist per slab: slab x n
    free, buried = [], []
    for xp in x:
        fr, bu = [], []
        for a0 in range(0, A, slab):
            sl = slice(a0, min(a0 + slab, A))
            pts = xp[sl, None, :] + R[sl, None, None] * unit[None]                     # [s,n,3]
            d = torch.cdist(pts.reshape(-1, 3), xp, compute_mode="donot_use_mm_for_euclid_dist").reshape(-1, n, A)
            cover = (d < R[None, None, :]) & live[None, None, :] & (idx[sl, None, None] != idx[None, None, :])
            mine = cls[sl, None, None] == cls[None, None, :]
            same, other = (cover & mine).any(-1), (cover & ~mine).any(-1)
            fr.append((~same).sum(-1) * live[sl])
            bu.append((~same & other).sum(-1) * live[sl])
        free.append(torch.cat(fr))
        buried.append(torch.cat(bu))
    return torch.stack(free), torch.stack(buried)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--torch-poses", type=int, default=2)
    args = ap.parse_args()
    n_pose, Lg, A = 64, 50, 2048
    rng = np.random.default_rng(50)
    side = 13
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    order = np.argsort(((grid - (side - 1) / 2.0) ** 2).sum(-1), kind="stable")[:A]
    sites = (grid[order] - (side - 1) / 2.0) * 3.8
    lig_idx = np.sort(rng.permutation(A)[:Lg])
    rec = np.setdiff1d(np.arange(A), lig_idx)
    x = np.empty((n_pose, A, 3))
    x[:, lig_idx] = sites[:Lg] + rng.uniform(-0.9, 0.9, (n_pose, Lg, 3))
    x[:, rec] = sites[Lg:] + rng.uniform(-0.6, 0.6, (n_pose, A - Lg, 3))
    elements = rng.choice([6, 6, 6, 7, 8, 16], A)
    residue_of = np.arange(A) // 8
    x = torch.from_numpy(x.astype(np.float32)).cuda()
    lines = []
    for n in (96, 960):
        s = BuriedSurface.from_arrays(elements, lig_idx, np.ones(A), residue_of, n_points=n, device="cuda")
        tab = s.tables("cuda")
        t = dict(cls=tab["cls"].long(), R=tab["radius"] + np.float32(s.probe), unit=tab["unit"])
        t64 = dict(cls=t["cls"], R=tab["radius"].double() + s.probe, unit=tab["unit"].double())
        out = s.measure(x)
        tp = args.torch_poses
        free, buried = torch_form(x[:tp].double(), t64)
        lig = tab["ligand_idx"].long()
        differ = int((out["buried_points"][:tp] != buried).sum()) + int((out["free_points"][:tp] != free[:, lig]).sum())
        reached = float((out["buried_points"][:, tab["cls"] == 1] > 0).float().mean())
        hip = per_call_us(lambda: s.measure(x), args.calls, args.windows)
        tor = per_call_us(lambda: torch_form(x[:tp], t), 1, 3, warm=1)
        lines.append(f"P={n_pose} L={Lg} A={A} R={s.n_residues} n={n}: BuriedSurface.measure {hip[0]:.1f} us per call (min {hip[1]:.1f}, max "
                     f"{hip[2]:.1f} over {args.windows} windows of {args.calls} calls; two kernels plus seven allocations), {hip[0] / n_pose:.2f} "
                     f"us per pose; torch cdist expression on {tp} poses {tor[0] / tp:.1f} us per pose (min {tor[1] / tp:.1f}, max "
                     f"{tor[2] / tp:.1f}; {tor[0] / tp / (hip[0] / n_pose):.0f} x); counts that differ from the float64 expression on those poses {differ} of "
                     f"{tp * (A + Lg)} (a point within rounding of a sphere may); buried fraction {float(out['buried_fraction'].mean()):.3f} mean, receptor atoms with "
                     f"buried points {100 * reached:.1f} %")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
