"""Time RingInteractions.fingerprint (csrc/plif_rings.hip) next to InteractionFingerprint.fingerprint (csrc/plif.hip) on the same poses
with device events: P = 64 poses, A = 2048 pose atoms, R = 256 residues of eight atoms (the benchmark crop's T = 256 / A = 2048),
L = 50 ligand atoms - the system of tools/plif_time.py.  Every sixth residue lends six of its atoms as a receptor ring (43 rings), the
ligand has three rings of six atoms and two halogens; lattice sites are no aromatic rings, but the kernels do the same work on them.
Each timed window is `--calls` back-to-back calls between two events, after a warm-up; the line reports the median and the spread of
`--windows` windows per call.

    python tools/plif_rings_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plif_time import per_call_us  # noqa: E402
from physdock_amd import interactions, scoring  # noqa: E402
from physdock_amd.interactions import InteractionFingerprint  # noqa: E402
from physdock_amd.ring_interactions import RingInteractions  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    n, Lg, A = 64, 50, 2048
    rng = np.random.default_rng(50)
    side = 13
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    order = np.argsort(((grid - (side - 1) / 2.0) ** 2).sum(-1), kind="stable")[:A]
    sites = (grid[order] - (side - 1) / 2.0) * 3.8
    lig_idx = np.sort(rng.permutation(A)[:Lg])
    rec = np.setdiff1d(np.arange(A), lig_idx)
    x = np.empty((n, A, 3))
    x[:, lig_idx] = sites[:Lg] + rng.uniform(-0.9, 0.9, (n, Lg, 3))
    x[:, rec] = sites[Lg:] + rng.uniform(-0.6, 0.6, (n, A - Lg, 3))
    elements = rng.choice([6, 6, 6, 7, 8, 16], A)
    types = scoring.element_types(elements, acceptors=True)
    types[elements == 7] |= scoring.DONOR
    charges = np.where(elements == 7, rng.integers(0, 2, A) * interactions.CATION, np.where(elements == 8, rng.integers(0, 2, A) * interactions.ANION, 0))
    residue_of = np.arange(A) // 8
    is_lig = np.zeros(A, dtype=bool)
    is_lig[lig_idx] = True
    rec_rings = []
    for s in range(0, A // 8, 6):
        atoms = [a for a in range(8 * s, 8 * s + 8) if not is_lig[a]][:6]
        if len(atoms) == 6:
            rec_rings.append(atoms)
    lig_rings = [list(range(0, 6)), list(range(6, 12)), list(range(12, 18))]
    six = InteractionFingerprint.from_types(types, charges, lig_idx, np.ones(A), residue_of, device="cuda")
    ring = RingInteractions.from_tables(types, charges, lig_idx, np.ones(A), residue_of, ligand_rings=lig_rings, receptor_rings=rec_rings,
                                        halogens=[(20, 19), (30, 29)], device="cuda")
    x = torch.from_numpy(x.astype(np.float32)).cuda()
    out = ring.fingerprint(x)
    shown = out["counts"].sum(0).tolist()
    t_ring = per_call_us(lambda: ring.fingerprint(x), args.calls, args.windows)
    t_six = per_call_us(lambda: six.fingerprint(x), args.calls, args.windows)
    line = (f"P={n} L={Lg} A={A} R={ring.n_residues} G_l={ring.n_ligand_rings} G_r={ring.n_receptor_rings} H={ring.n_halogens}: "
            f"RingInteractions.fingerprint {t_ring[0]:.1f} us per call (min {t_ring[1]:.1f}, max {t_ring[2]:.1f} over {args.windows} windows of "
            f"{args.calls} calls; four kernels plus eight allocations); InteractionFingerprint.fingerprint on the same poses {t_six[0]:.1f} us "
            f"(min {t_six[1]:.1f}, max {t_six[2]:.1f}); residues per kind over the 64 poses {shown}")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
