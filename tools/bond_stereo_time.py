"""Time BondStereo.check (csrc/bond_stereo.hip) with device events: ONE launch for 64 poses of 2048 atoms with 1, 8 and 64 entries (every
entry with both second substituents, so four dihedrals each), next to the numpy restatement of the definition on the host
(tests/bond_stereo_ref.py, wall clock for the same poses).  Each timed window is `--calls` back-to-back calls between two events, after
a warm-up; a line reports the median and the spread of `--windows` windows per call.  The kernel is latency-bound (one wave per pose):
untuned, and there is no time gate - nobody has measured this before.

    python tools/bond_stereo_time.py [--out file]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bond_stereo_ref as ref  # noqa: E402
from physdock_amd.bond_stereo import BondStereo  # noqa: E402
from sasa_time import per_call_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--poses", type=int, default=64)
    ap.add_argument("--atoms", type=int, default=2048)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    x = rng.uniform(-20.0, 20.0, (args.poses, args.atoms, 3)).astype(np.float32)
    parts = []
    for n in (1, 8, 64):
        quads = np.stack([rng.choice(args.atoms, 6, replace=False) for _ in range(n)]).astype(np.int32)
        spec = BondStereo.from_tables(quads, rng.integers(1, 3, n))
        xd = torch.from_numpy(x).cuda()
        got = spec.check(xd)
        t0 = time.perf_counter()
        want = ref.check(x, quads, spec.expect, spec.max_twist)
        host = time.perf_counter() - t0
        assert np.array_equal(got["state"].cpu().numpy(), want["state"]) and np.array_equal(got["n_wrong"].cpu().numpy(), want["n_wrong"])
        t = per_call_us(lambda: spec.check(xd), args.calls, args.windows)
        parts.append(f"{n} entries {t[0]:.1f} us ({t[1]:.1f}, {t[2]:.1f}), the restatement on the host {host * 1e3:.1f} ms")
    line = (f"P={args.poses} poses of A={args.atoms} atoms; per call of BondStereo.check, median (min, max) over {args.windows} windows of "
            f"{args.calls} calls, one kernel plus seven allocations, untuned: " + "; ".join(parts))
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
