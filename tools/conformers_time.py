"""Time ConformerEnsemble.embed (csrc/conformers.hip) with device events: C = 128 conformers of the 14-atom test ligand (phenyl, chain,
one stereocentre) and of extended carbon chains of 32 and 64 atoms (tests/conformers_ref.py builds them), and the numpy reference's
wall time per conformer on the host for the same ligands.  Each timed window is `--calls` back-to-back calls between two events after a
warm-up; a line reports the median and the spread of `--windows` windows per call.

    python tools/conformers_time.py [--out file]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plif_time import per_call_us  # noqa: E402
import conformers_ref as cr  # noqa: E402
from physdock_amd.conformers import ConformerEnsemble  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-conformers", type=int, default=4)
    args = ap.parse_args()
    C, lines = 128, []
    for name in ("phenyl14", "chain32", "chain64"):
        c = cr.make_case(name)
        ens = ConformerEnsemble.from_bonds(c["n_atoms"], c["bonds"], c["x_ref"], c["elements"], bond_orders=c["bond_orders"],
                                           planar_groups=c["planar_groups"], centres=c["centres"], device="cuda")
        out = ens.embed(C, 1)
        its = out["iterations"].double().mean(0).tolist()
        t = per_call_us(lambda: ens.embed(C, 1, keep=None), args.calls, args.windows, warm=2)
        tabs = cr.case_tables(name)
        t0 = time.perf_counter()
        ref = cr.embed(tabs, args.host_conformers, 1)
        host = (time.perf_counter() - t0) / args.host_conformers
        lines.append(f"L={c['n_atoms']} ({name}) C={C}: embed {t[0]:.0f} us per call (min {t[1]:.0f}, max {t[2]:.0f} over {args.windows} windows "
                     f"of {args.calls} calls), {t[0] / C:.1f} us per conformer; accepted {int(out['ok'].sum())} of {C}, mean accepted steps "
                     f"{its[0]:.0f} + {its[1]:.0f}; numpy reference {host * 1e3:.0f} ms per conformer on the host "
                     f"({sum(r['ok'] for r in ref)} of {args.host_conformers} accepted)")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
