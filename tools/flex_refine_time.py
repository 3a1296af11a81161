"""Time FlexRefine.refine (csrc/vina_flex.hip) with device events on the poses of tools/refine_time.py - P = 64 poses of a 32-atom
ligand in a receptor of A = 2048 pose atoms - with 0, 4 and 10 flexible residues, next to VinaRefine.refine on the same poses.
A flexible "residue" here is a chain of five receptor lattice atoms CA - CB - G - D - E next to the pocket (three chis, F = 5 rows
each; 3.8 A "bonds": the geometry is not protein-like, the work per evaluation is what is measured).  Per evaluation the kernel does
about (L + F) x A pair tests instead of L x A, so the expected cost ratio is near (L + F) / L times the ratio of the evaluation
counts.  Each timed window is `--calls` back-to-back calls between two events, after a warm-up; a line reports the median and the
spread of `--windows` windows.

    python tools/flex_refine_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import vina_refine_ref as ref  # noqa: E402
from refine_time import BONDS, ligand, per_call_us  # noqa: E402
from physdock_amd.flex import FlexRefine  # noqa: E402
from physdock_amd.refine import VinaRefine  # noqa: E402
from physdock_amd.scoring import VinaScore  # noqa: E402


def system(n_pose=64, Lg=32, A=2048):
    """the timed system: (VinaScore, VinaRefine, poses [n_pose,A,3] on the device, ten chains of five receptor atoms lining the pocket)"""
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
    xd = torch.from_numpy(x.astype(np.float32)).cuda()
    # chains of five receptor atoms that line the pocket, nearest first
    lining = rec[(vina.rec_mask[rec] > 0)]
    lining = lining[np.argsort(np.sqrt(((x[0, lining][:, None] - y0[None]) ** 2).sum(-1)).min(1), kind="stable")]
    chains = [lining[5 * k:5 * k + 5].tolist() for k in range(10)]
    return vina, r, xd, chains


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--max-iters", type=int, default=50)
    args = ap.parse_args()
    n_pose, Lg, A = 64, 32, 2048
    vina, r, xd, chains = system(n_pose, Lg, A)
    lines = []
    base = per_call_us(lambda: r.refine(xd, max_iters=args.max_iters), args.calls, args.windows)
    out = r.refine(xd, max_iters=args.max_iters)
    ev0 = float(out["evaluations"].double().mean())
    lines.append(f"VinaRefine.refine P={n_pose} L={Lg} T={r.n_torsions} A={A} max_iters={args.max_iters}: {base[0] / 1e3:.2f} ms per call (min "
                 f"{base[1] / 1e3:.2f}, max {base[2] / 1e3:.2f} over {args.windows} windows of {args.calls} calls), evaluations {ev0:.1f} mean, E "
                 f"{float(out['energy_start'].mean()):.3f} -> {float(out['energy'].mean()):.3f} kcal/mol mean")
    for n_res in (0, 4, 10):
        use = chains[:n_res]
        rec_bonds = [b for ch in use for b in zip(ch[:-1], ch[1:])]
        tors = [[(ch[k], ch[k + 1]) for k in range(3)] for ch in use]
        f = FlexRefine.from_tables(vina.types, vina.ligand_idx, vina.rec_mask, vina.lig_active, vina.n_rot, r.rot, r.moving, r.intra, rec_bonds, tors,
                                   device="cuda")
        t = per_call_us(lambda: f.refine(xd, max_iters=args.max_iters), args.calls, args.windows)
        o = f.refine(xd, max_iters=args.max_iters)
        ev = float(o["evaluations"].double().mean())
        M = f.n_atoms + f.n_flex_atoms
        lines.append(f"FlexRefine.refine residues={n_res} F={f.n_flex_atoms} S={f.n_flex_torsions} M={M}: {t[0] / 1e3:.2f} ms per call (min {t[1] / 1e3:.2f}, "
                     f"max {t[2] / 1e3:.2f}), ratio to VinaRefine.refine {t[0] / base[0]:.2f} (expected near (L+F)/L x evaluations ratio = "
                     f"{M / Lg:.2f} x {(ev + 1) / ev0:.2f} = {M / Lg * (ev + 1) / ev0:.2f}), evaluations {ev:.1f} mean (+1 uncounted at the end), iterations "
                     f"{float(o['iterations'].double().mean()):.1f} mean, E {float(o['energy_start'].mean()):.3f} -> {float(o['energy'].mean()):.3f} kcal/mol mean, "
                     f"moved {float(o['moved'].mean()):.2f} A, moved_flex {float(o['moved_flex'].mean()):.2f} A mean")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
