"""Time LigandLibrary.features (csrc/ligand_features.hip) with device events: ONE launch for a library of 1024 ligands - the five
demo SMILES of tests/golden/smiles_demo.txt, cycled - next to the numpy restatement of the same tables on the host
(tests/ligand_features_ref.py, wall clock over the five distinct ligands, scaled to 1024) and to Ligand.embed_reference per ligand
(wall clock with a synchronisation: it reads the errors back).  Each timed window is `--calls` back-to-back calls between two events,
after a warm-up; a line reports the median and the spread of `--windows` windows per call.  There is no time gate: nobody has measured
this before.

    python tools/ligand_features_time.py [--out file]
"""
import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ligand_features_ref as ref  # noqa: E402
from physdock_amd.ligand import Ligand, LigandLibrary  # noqa: E402
from physdock_amd.smiles import parse_smiles  # noqa: E402
from sasa_time import per_call_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--ligands", type=int, default=1024)
    args = ap.parse_args()
    with open(os.path.join(REPO, "tests", "golden", "smiles_demo.txt")) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    t0 = time.perf_counter()
    distinct = [Ligand.from_smiles(s) for s in lines]
    t_parse = (time.perf_counter() - t0) / len(lines)
    lib = LigandLibrary([distinct[k % len(distinct)] for k in range(args.ligands)])
    lib.features("cuda")
    t_gpu = per_call_us(lambda: lib.features("cuda"), args.calls, args.windows)
    t0 = time.perf_counter()
    for s in lines:
        ref.features(parse_smiles(s))
    t_host = (time.perf_counter() - t0) / len(lines)
    embed = []
    for lig in distinct:
        lig.embed_reference(seed=0, device="cuda")                                   # warm-up: tables, the first launch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = lig.embed_reference(seed=1, device="cuda")
        torch.cuda.synchronize()
        embed.append((time.perf_counter() - t0, out["n_accepted"], out["max_violation"]))
    out_bytes = lib.n_atoms * (16 + 167 * 4) + lib.n_pairs * (8 + 42 * 4)
    line = (f"G={args.ligands} ligands of {min(l.n_atoms for l in distinct)} .. {max(l.n_atoms for l in distinct)} atoms ({lib.n_atoms} atoms, "
            f"{lib.n_pairs} pairs, {out_bytes / 1e6:.1f} MB written): LigandLibrary.features {t_gpu[0]:.1f} us per launch (min {t_gpu[1]:.1f}, max "
            f"{t_gpu[2]:.1f} over {args.windows} windows of {args.calls} calls; one kernel plus four allocations; untuned), "
            f"{t_gpu[0] / args.ligands:.3f} us per ligand; the numpy restatement on the host {t_host * 1e3:.1f} ms per ligand, "
            f"{t_host * args.ligands:.1f} s for the library; parse_smiles + Ligand {t_parse * 1e3:.2f} ms per ligand; embed_reference (C=32) "
            + ", ".join(f"{t * 1e3:.1f} ms ({n} of 32 accepted, violation {v:.3f} A)" for t, n, v in embed) + " for the five ligands")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
