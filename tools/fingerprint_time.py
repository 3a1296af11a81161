"""Time MorganFingerprint (csrc/fingerprint.hip) with device events on a library of 1024 ligands - the five demo SMILES of
tests/golden/smiles_demo.txt, cycled: ONE launch of LigandLibrary.fingerprints (radius 2, 2048 bits), `pairwise` (1024 x 1024),
`neighbours(8)` and `maxmin(64)` (1 + 2 * 63 launches), next to the Python restatement of the definition on the host
(tests/fingerprint_ref.py, wall clock: the fingerprints of the five distinct ligands scaled to 1024, the numpy Tanimoto matrix of the
whole library, top-8 and MaxMin on its first `--host-rows` rows).  The library holds five distinct rows, so `neighbours` and `maxmin`
run on ties throughout: that is their slowest ordering path, not a typical similarity distribution.  Each timed window is `--calls`
back-to-back calls between two events, after a warm-up; a line reports the median and the spread of `--windows` windows per call.
There is no time gate: nobody has measured this before.

    python tools/fingerprint_time.py [--out file]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fingerprint_ref as ref  # noqa: E402
from physdock_amd.ligand import Ligand, LigandLibrary  # noqa: E402
from sasa_time import per_call_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--ligands", type=int, default=1024)
    ap.add_argument("--host-rows", type=int, default=128)
    args = ap.parse_args()
    with open(os.path.join(REPO, "tests", "golden", "smiles_demo.txt")) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    distinct = [Ligand.from_smiles(s) for s in lines]
    lib = LigandLibrary([distinct[k % len(distinct)] for k in range(args.ligands)])
    fp = lib.fingerprints(device="cuda")
    t0 = time.perf_counter()
    want = [ref.fingerprint(lig) for lig in distinct]
    t_fp = (time.perf_counter() - t0) / len(distinct)
    bits = fp.bits.cpu().numpy().view(np.uint32)
    assert all(np.array_equal(bits[k], want[k % len(distinct)]["bits"]) for k in range(args.ligands))
    runs = (("fingerprints (radius 2, 2048 bits)", lambda: lib.fingerprints(device="cuda")),
            ("fingerprints(aromatize=True)", lambda: lib.fingerprints(aromatize=True, device="cuda")),
            ("fingerprints (radius 4, 4096 bits)", lambda: lib.fingerprints(4, 4096, device="cuda")),
            ("pairwise", fp.pairwise), ("neighbours(8)", lambda: fp.neighbours(8)), ("maxmin(64)", lambda: fp.maxmin(64)))
    t_gpu = {name: per_call_us(fn, args.calls, args.windows) for name, fn in runs}
    t0 = time.perf_counter()
    sim, _ = ref.tanimoto(bits, bits)
    t_sim = time.perf_counter() - t0
    assert np.array_equal(fp.pairwise().cpu().numpy().view(np.uint32), sim.view(np.uint32))
    h = args.host_rows
    t0 = time.perf_counter()
    ref.nearest(bits[:h], bits[:h], 8, exclude_self=True)
    t_near = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref.maxmin(bits[:h], min(64, h))
    t_pick = time.perf_counter() - t0
    line = (f"G={args.ligands} ligands of {min(l.n_atoms for l in distinct)} .. {max(l.n_atoms for l in distinct)} atoms ({lib.n_atoms} atoms, "
            f"{lib.n_bonds} bonds, {int(fp.n_features.min())} .. {int(fp.n_features.max())} kept features, {int(fp.popcount.min())} .. "
            f"{int(fp.popcount.max())} bits set of 2048); per call, median (min, max) over {args.windows} windows of {args.calls} calls, "
            "allocations included, untuned: " + "; ".join(f"{name} {t[0]:.1f} us ({t[1]:.1f}, {t[2]:.1f})" for name, t in t_gpu.items())
            + f"; the Python restatement on the host: fingerprints {t_fp * 1e3:.2f} ms per ligand, {t_fp * args.ligands:.2f} s for the "
            f"library; the numpy Tanimoto matrix {t_sim:.2f} s; top-8 of {h} x {h} rows {t_near:.2f} s; MaxMin {min(64, h)} of {h} rows "
            f"{t_pick:.2f} s")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
