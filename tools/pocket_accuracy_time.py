"""Time PocketAccuracy.score (csrc/pocket_accuracy.hip) with device events at P = 64 poses of A = 2048 atoms (249 residues of eight
heavy atoms named as aspartates, so that every pocket residue can be swapped, around a ligand of 56 atoms), next to LddtPli.score and
ReceptorGeometry.check on the same poses in the same run, for scale: the two other measures of the package that walk every pose's
receptor.  Each timed window is `--calls` back-to-back calls between two events, after a warm-up; a line reports the median and the
spread of `--windows` windows per call.  The receptor is a jittered lattice of 2.7 A (0.05 heavy atoms per A^3, a protein's density) with a
cavity around the ligand; a residue is a cube of eight lattice sites.  There is no time gate: nobody has measured this before.

    python tools/pocket_accuracy_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from physdock_amd.lddt_pli import LddtPli  # noqa: E402
from physdock_amd.pocket_accuracy import PocketAccuracy  # noqa: E402
from physdock_amd.receptor_geometry import ReceptorGeometry  # noqa: E402
from sasa_time import per_call_us  # noqa: E402

ASP = ("N", "CA", "C", "O", "CB", "CG", "OD1", "OD2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    n_pose, Lg, A, h = 64, 56, 2048, 2.7
    n_res = (A - Lg) // 8
    rng = np.random.default_rng(60)
    cubes = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64) - 3.5      # 8^3 cubes of 2 x 2 x 2 sites
    corner = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64) - 0.5
    centres = cubes * 2.0 * h
    centres = centres[np.sqrt((centres ** 2).sum(-1)) >= 6.0]                           # the cavity
    centres = centres[np.argsort((centres ** 2).sum(-1), kind="stable")][:n_res]
    rec = (centres[:, None, :] + corner[None] * h).reshape(-1, 3)
    x_ref = np.concatenate([rec + rng.uniform(-0.4, 0.4, rec.shape), rng.normal(size=(Lg, 3)) * 1.6])
    x_ref = x_ref.astype(np.float32).astype(np.float64)
    res_names = ["ASP"] * (8 * n_res) + ["LIG"] * Lg
    atom_names = list(ASP) * n_res + [f"C{k + 1}" for k in range(Lg)]
    residue_of = np.concatenate([np.arange(8 * n_res) // 8, n_res + np.arange(Lg)])
    lig_idx = np.arange(8 * n_res, A)
    is_rec = np.arange(A) < 8 * n_res
    x = x_ref[None] + rng.normal(size=(n_pose, A, 3)) * np.linspace(0.1, 2.0, n_pose)[:, None, None]
    x = torch.from_numpy(x.astype(np.float32)).cuda()
    pa = PocketAccuracy.from_names(res_names, atom_names, residue_of, x_ref, lig_idx, device="cuda")
    pli = LddtPli.from_arrays(x_ref, lig_idx, is_rec, device="cuda")
    geo = ReceptorGeometry.from_names(res_names, atom_names, residue_of, x_ref, mask=is_rec, n_residues=n_res + Lg, device="cuda")
    out = pa.score(x)
    assert bool(out["ok"].all()) and bool(out["fit_ok"].all())
    t_pa = per_call_us(lambda: pa.score(x), args.calls, args.windows)
    t_pli = per_call_us(lambda: pli.score(x), args.calls, args.windows)
    t_geo = per_call_us(lambda: geo.check(x), args.calls, args.windows)
    rows = np.diff(pa.pair_start)
    line = (f"P={n_pose} A={A} L={Lg}: PocketAccuracy.score {t_pa[0]:.1f} us per call (min {t_pa[1]:.1f}, max {t_pa[2]:.1f} over {args.windows} "
            f"windows of {args.calls} calls; three kernels plus eleven allocations; untuned), {t_pa[0] / n_pose:.2f} us per pose; pocket residues "
            f"{pa.n_pocket_residues} (all swappable), pocket atoms {pa.n_pocket_atoms}, pairs {pa.n_pairs} (rows of {int(rows.min())} .. "
            f"{int(rows.max())}), CA atoms {pa.n_ca}; mean lddt_lp {float(out['lddt_lp'].mean()):.3f}, mean ca_rmsd {float(out['ca_rmsd'].mean()):.2f} A, "
            f"swapped {float(out['swapped'].float().sum(1).mean()):.1f} residues per pose; on the same poses LddtPli.score "
            f"({pli.n_contacts} contacts) {t_pli[0]:.1f} us (min {t_pli[1]:.1f}, max {t_pli[2]:.1f}) and ReceptorGeometry.check "
            f"({geo.n_terms} terms) {t_geo[0]:.1f} us (min {t_geo[1]:.1f}, max {t_geo[2]:.1f})")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
