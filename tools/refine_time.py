"""Time VinaRefine.refine (csrc/vina_refine.hip) with device events at P = 64 poses of a 32-atom ligand (two rings, T = 8 torsions)
in a receptor of A = 2048 pose atoms - the benchmark's crop size -, next to the float64 NumPy restatement tests/vina_refine_ref.py on
the host for the first `--ref-poses` of the same poses (wall clock, one thread of the interpreter; reported per pose).  The receptor
is a jittered 3.8 A lattice; the atoms that would overlap the ligand's base conformation are masked out, and the 64 poses are that
conformation moved by up to 0.7 A, 0.3 rad as a body and 0.5 rad per torsion, so most of them start with clashes.  Each timed window
is `--calls` back-to-back calls between two events, after a warm-up; the line reports the median and the spread of `--windows` windows.

    python tools/refine_time.py [--out file]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vina_refine_ref as ref  # noqa: E402
from physdock_amd.refine import VinaRefine  # noqa: E402
from physdock_amd.scoring import VinaScore  # noqa: E402

BONDS = ([(i, (i + 1) % 6) for i in range(6)] + [(0, 6), (6, 7), (7, 8)] + [(8 + i, 8 + (i + 1) % 6) for i in range(6)] +
         [(11, 14), (14, 15), (15, 16), (15, 17), (3, 18), (18, 19), (19, 20), (20, 21), (6, 22), (7, 23), (14, 24), (18, 25), (19, 26),
          (20, 27), (21, 28), (21, 29), (16, 30), (17, 31)])


def ligand(rng, n=32):
    """a self-avoiding walk over the bond list: 1.5 A bonds, no two atoms closer than 1.3 A"""
    y = np.zeros((n, 3))
    placed = {0}
    for i, j in BONDS:
        if j in placed:
            continue
        for _ in range(1000):
            v = rng.normal(size=3)
            cand = y[i] + 1.5 * v / np.linalg.norm(v) + 0.8 * y[i] / max(np.linalg.norm(y[i]), 1.0) * 0.5
            if all(np.linalg.norm(cand - y[k]) > 1.3 for k in placed):
                break
        y[j] = cand
        placed.add(j)
    return y - y.mean(0)


def per_call_us(fn, calls, windows, warm=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--ref-poses", type=int, default=8)
    ap.add_argument("--max-iters", type=int, default=50)
    args = ap.parse_args()
    n_pose, Lg, A = 64, 32, 2048
    rng = np.random.default_rng(64)
    side = 13
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    order = np.argsort(((grid - (side - 1) / 2.0) ** 2).sum(-1), kind="stable")[:A]
    sites = (grid[order] - (side - 1) / 2.0) * 3.8
    lig_idx = np.sort(rng.permutation(A)[:Lg])
    rec = np.setdiff1d(np.arange(A), lig_idx)
    elements = rng.choice([6, 6, 6, 7, 8, 16], A)
    elements[lig_idx] = rng.choice([6, 6, 6, 7, 8], Lg)
    vina = VinaScore.from_bonds(elements, BONDS, lig_idx, device="cuda")
    y0 = ligand(rng)
    xr = sites[Lg:] + rng.uniform(-0.6, 0.6, (A - Lg, 3))
    rad = ref.RADII[vina.types & 15]
    d = np.sqrt(((xr[:, None] - y0[None]) ** 2).sum(-1)) - rad[rec][:, None] - rad[lig_idx][None]
    vina.rec_mask[rec[d.min(1) < 0.3]] = 0                                             # the pocket
    vina._tables = {}
    r = VinaRefine.from_vina(vina, BONDS, device="cuda")
    c = dict(lig_idx=vina.ligand_idx, types=vina.types, rec_mask=vina.rec_mask, lig_active=vina.lig_active, rot=r.rot, sets=r.moving,
             mask=r.rot_mask, intra=r.intra)
    x = np.empty((n_pose, A, 3))
    x[:, rec] = xr
    for p in range(n_pose):
        s = np.concatenate([rng.uniform(-0.7, 0.7, 3), rng.uniform(-0.3, 0.3, 3) / np.sqrt(3.0), rng.uniform(-0.5, 0.5, r.n_torsions)])
        x[p, lig_idx] = ref.move(c, y0, s)
    x32 = x.astype(np.float32)
    xd = torch.from_numpy(x32).cuda()
    out = r.refine(xd, max_iters=args.max_iters)
    torch.cuda.synchronize()
    it, ev, st = out["iterations"].cpu().numpy(), out["evaluations"].cpu().numpy(), out["status"].cpu().numpy()
    kern = per_call_us(lambda: r.refine(xd, max_iters=args.max_iters), args.calls, args.windows)
    t0 = time.perf_counter()
    host = [ref.refine(c, x32[p].astype(np.float64), max_iters=args.max_iters) for p in range(args.ref_poses)]
    host_s = (time.perf_counter() - t0) / max(args.ref_poses, 1)
    agree = sum(int(h["iterations"] == it[p] and h["evaluations"] == ev[p] and h["status"] == st[p]) for p, h in enumerate(host))
    lig = torch.from_numpy(lig_idx).cuda()
    diff = max([float(np.abs(out["x_refined"][p, lig].cpu().double().numpy() - h["y"]).max()) for p, h in enumerate(host)] + [0.0])
    line = (f"P={n_pose} L={Lg} T={r.n_torsions} A={A} receptor atoms {int(vina.rec_mask.sum())} intra pairs {len(r.intra)} max_iters={args.max_iters}: "
            f"VinaRefine.refine {kern[0] / 1e3:.2f} ms per call (min {kern[1] / 1e3:.2f}, max {kern[2] / 1e3:.2f} over {args.windows} windows of "
            f"{args.calls} calls; one refinement launch, two score launches, the allocations), {kern[0] / n_pose:.1f} us per pose; iterations "
            f"{it.mean():.1f} mean ({it.min()} - {it.max()}), evaluations {ev.mean():.1f} mean ({ev.min()} - {ev.max()}), status counts "
            f"{np.bincount(st, minlength=3).tolist()}; E {float(out['energy_start'].mean()):.3f} -> {float(out['energy'].mean()):.3f} kcal/mol mean, moved "
            f"{float(out['moved'].mean()):.2f} A mean; NumPy restatement on the host {host_s * 1e3:.0f} ms per pose over {args.ref_poses} poses "
            f"({host_s * n_pose:.1f} s for {n_pose}; {host_s * n_pose / (kern[0] * 1e-6):.0f} x), same counts on {agree} of {args.ref_poses}, largest "
            f"coordinate difference {diff:.2e} A (fp32 output)")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
