"""Time Hydrogens.hbonds and Hydrogens.place (csrc/hydrogens.hip) next to InteractionFingerprint.fingerprint (csrc/plif.hip) on the same
poses with device events: P = 64 poses, A = 2048 pose atoms, R = 256 residues of eight atoms (the benchmark crop's T = 256 / A = 2048),
L = 50 ligand atoms - the system of tools/plif_time.py.  Every atom carries one row of the hydrogen table (a protein has about one
hydrogen per heavy atom), its refs the next atoms of its residue (or of the ligand), the modes cycling TRI, BISECT in the plane, BISECT
out of it, methyl slot, hydroxyl rotor, LINEAR; every oxygen is an acceptor, every N, O and S a donor parent.  Lattice sites are no
molecule, but the kernels do the same work on them.  Each timed window is `--calls` back-to-back calls between two events, after a
warm-up; the line reports the median and the spread of `--windows` windows per call.

    python tools/hydrogens_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plif_time import per_call_us  # noqa: E402
from physdock_amd import hydrogens as HY, interactions, scoring  # noqa: E402
from physdock_amd.hydrogens import Hydrogens  # noqa: E402
from physdock_amd.interactions import InteractionFingerprint  # noqa: E402


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
    rows = HY._Rows()
    for a in range(A):
        mates = lig_idx if is_lig[a] else np.asarray([b for b in range(8 * (a // 8), 8 * (a // 8) + 8) if not is_lig[b]])
        mates = np.roll(mates, -int(np.nonzero(mates == a)[0][0]))[1:]
        if len(mates) < 3:
            continue
        length = HY.DEFAULT_LENGTHS[int(elements[a])]
        kind = a % 6
        if kind == 0:
            rows.add(a, mates[:3], HY.TRI, length)
        elif kind in (1, 2):
            rows.add(a, mates[:2], HY.BISECT, length, 0.0 if kind == 1 else HY.HALF_TETRAHEDRAL)
        elif kind == 3:
            rows.nerf(a, mates[0], mates[1], length, HY.TETRAHEDRAL, (np.pi,))
        elif kind == 4:
            rows.nerf(a, mates[0], mates[1], length, HY.TETRAHEDRAL, (np.pi,), rotor=True)
        else:
            rows.add(a, mates[:1], HY.LINEAR, length)
    six = InteractionFingerprint.from_types(types, charges, lig_idx, np.ones(A), residue_of, device="cuda")
    hy = Hydrogens.from_tables(types, lig_idx, np.ones(A), residue_of, rows.table(), device="cuda")
    x = torch.from_numpy(x.astype(np.float32)).cuda()
    out = hy.hbonds(x)
    shown = out["counts"].sum(0).tolist()
    placed = int(out["placed"].sum()) // n
    t_bonds = per_call_us(lambda: hy.hbonds(x), args.calls, args.windows)
    t_place = per_call_us(lambda: hy.place(x), args.calls, args.windows)
    t_six = per_call_us(lambda: six.fingerprint(x), args.calls, args.windows)
    line = (f"P={n} L={Lg} A={A} R={hy.n_residues} H={hy.n_hydrogens} (placed {placed} per pose) G={hy.n_groups} polar={hy.n_ligand_polar}+"
            f"{hy.n_receptor_polar} acceptors={hy.n_ligand_acceptors}+{hy.n_receptor_acceptors}: Hydrogens.hbonds {t_bonds[0]:.1f} us per call (min "
            f"{t_bonds[1]:.1f}, max {t_bonds[2]:.1f} over {args.windows} windows of {args.calls} calls; four kernels, two copies into x_all and "
            f"nine allocations), of which Hydrogens.place {t_place[0]:.1f} us (min {t_place[1]:.1f}, max {t_place[2]:.1f}); "
            f"InteractionFingerprint.fingerprint on the same poses {t_six[0]:.1f} us (min {t_six[1]:.1f}, max {t_six[2]:.1f}); (H, acceptor) "
            f"pairs per kind over the 64 poses {shown}")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
