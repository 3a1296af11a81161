"""Time ReceptorGeometry.check and .dihedrals (csrc/receptor_geometry.hip) with device events at P = 64 poses of A = 2048 receptor atoms
(a 256-residue peptide of LEU, PHE, LYS, ... built from nominal internal coordinates, cropped to 2048 atoms), next to
PoseValidity.check on poses of the same size (L = 50 ligand atoms, as tools/validity_time.py).  Each timed window is `--calls`
back-to-back calls between two events, after a warm-up; the line reports the median and the spread of `--windows` windows per call.

    python tools/receptor_geometry_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import receptor_geometry_ref as ref  # noqa: E402  (the peptide builder)
from physdock_amd.receptor_geometry import ReceptorGeometry  # noqa: E402
from physdock_amd.validity import PoseValidity  # noqa: E402
from validity_time import per_call_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    n, A = 64, 2048
    rng = np.random.default_rng(60)
    seq = [ref.ALL_TYPES[k % 20] for k in range(300)]
    res, atoms, rid, x = ref.build_peptide(seq)
    last = int(rid[A - 1])                                              # whole residues only
    keep = rid < last
    res, atoms, rid, x = [r for r, k in zip(res, keep) if k], [a for a, k in zip(atoms, keep) if k], rid[keep], x[keep]
    pad = A - len(rid)                                                  # ... topped up with atoms that take no part
    mask = np.concatenate([np.ones(len(rid), bool), np.zeros(pad, bool)])
    res, atoms = res + ["XXX"] * pad, atoms + ["X"] * pad
    rid = np.concatenate([rid, np.full(pad, last)])
    x = np.concatenate([x, np.zeros((pad, 3))])
    g = ReceptorGeometry.from_names(res, atoms, rid, x, mask=mask, device="cuda")
    poses = torch.from_numpy((x[None] + rng.standard_normal((n, A, 3)) * 0.2).astype(np.float32)).cuda()
    Lg = 50
    lig_idx = np.sort(rng.permutation(A)[:Lg])
    v = PoseValidity.from_bonds(Lg, [(i, i + 1) for i in range(Lg - 1)], np.cumsum(rng.standard_normal((Lg, 3)) * 0.9, 0), np.full(A, 6), lig_idx,
                                device="cuda")
    out = g.check(poses)
    chk = per_call_us(lambda: g.check(poses), args.calls, args.windows)
    dih = per_call_us(lambda: g.dihedrals(poses), args.calls, args.windows)
    val = per_call_us(lambda: v.check(poses), args.calls, args.windows)
    line = (f"P={n} A={A} R={g.n_residues} terms={g.n_terms} excluded={len(g.excl_atom)}: ReceptorGeometry.check {chk[0]:.1f} us per call "
            f"(min {chk[1]:.1f}, max {chk[2]:.1f} over {args.windows} windows of {args.calls} calls; three kernels plus nine output "
            f"allocations); .dihedrals {dih[0]:.1f} us (min {dih[1]:.1f}, max {dih[2]:.1f}); PoseValidity.check at L={Lg} {val[0]:.1f} us "
            f"(min {val[1]:.1f}, max {val[2]:.1f}); failing poses {int((~out['valid']).sum())} of {n}")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
