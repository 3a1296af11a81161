"""Time SdfTemplate.format and .text (csrc/sdf.hip) against the reference writer tests/sdf_ref.py on the same poses: 64 poses of a
40-atom ligand (a chain with ring closures, 43 bonds, 3 charges) in a 440-atom system with 6 data items.  `format` (three launches and
the read of the overflow counter) is timed with device events, `--calls` back-to-back calls per window after a warm-up; `text` (format,
one copy back, the split into str) and the reference writer are wall time on the host.  A line reports the median and the spread of
`--windows` windows per call.  No threshold is set.

    python tools/sdf_time.py [--out file]
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
import sdf_ref  # noqa: E402
from physdock_amd.sdfio import SdfTemplate  # noqa: E402


def wall_us(fn, calls, windows):
    fn()
    ts = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        ts.append((time.perf_counter() - t0) * 1e6 / calls)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    P, L, A = 64, 40, 440
    rng = np.random.default_rng(0)
    symbols = [["C", "C", "C", "N", "O", "S", "Cl"][i] for i in rng.integers(0, 7, L)]
    bonds = [(i, i + 1) for i in range(L - 1)] + [(0, 5), (10, 15), (20, 25), (30, 35)]
    orders = [1.5 if i < 6 else 1.0 for i in range(len(bonds))]
    charges = np.zeros(L, dtype=np.int64)
    charges[[3, 17, 29]] = [1, -1, 1]
    lig = np.arange(A - L, A)
    elements = ["C"] * (A - L) + symbols
    t = SdfTemplate.from_bonds(elements, bonds, lig, orders, charges, title="ligand", device="cuda")
    x = rng.normal(0.0, 15.0, (P, A, 3)).astype(np.float32)
    cols = [("pose", np.arange(P), None), ("ranking_confidence", rng.uniform(0, 1, P).astype(np.float32), 4),
            ("vina_score", rng.normal(-7, 2, P).astype(np.float32), 4), ("valid", rng.integers(0, 2, P).astype(bool), None),
            ("ligand_rmsd", rng.uniform(0, 12, P).astype(np.float32), 4), ("lddt_pli", rng.uniform(0, 1, P).astype(np.float32), 4)]
    dx = torch.from_numpy(x).cuda()
    props = {n: torch.from_numpy(v).cuda() if d is None else (torch.from_numpy(v).cuda(), d) for n, v, d in cols}
    host = lambda: "".join(sdf_ref.records(symbols, x[:, lig], bonds, orders, charges, cols, title="ligand"))
    want = host()
    assert t.text(dx, props) == want, "the device's file is not the reference writer's"
    f = per_call_us(lambda: t.format(dx, props), args.calls, args.windows, warm=5)
    w = wall_us(lambda: t.text(dx, props), args.calls, args.windows)
    h = wall_us(host, 2, args.windows)
    line = (f"P={P} poses, L={L} atoms, {len(bonds)} bonds, {len(cols)} items, {len(want)} bytes ({len(want) // P} per record): format "
            f"{f[0]:.0f} us per call (min {f[1]:.0f}, max {f[2]:.0f} over {args.windows} windows of {args.calls} calls, device events, with the "
            f"read of the overflow counter); format + text {w[0]:.0f} us wall (min {w[1]:.0f}, max {w[2]:.0f}); reference writer on the host "
            f"{h[0]:.0f} us wall (min {h[1]:.0f}, max {h[2]:.0f}); identical text")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
