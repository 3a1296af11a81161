"""Time LigandLibrary.aromaticity (csrc/aromaticity.hip) with device events: ONE launch for a library of 1024 ligands - the five demo
SMILES of tests/golden/smiles_demo.txt, cycled - in the modes kekulise (0), perceive (1) and normalise (2), next to
LigandLibrary.features (pd_ligand_features) and features(aromatize=True) in the same run, and next to the Python restatement of the
definition on the host (tests/aromaticity_ref.py, wall clock over the five distinct ligands, scaled to 1024).  Kekulise with a budget
of 0 steps stops before the first try (status 2), so the difference to the full kekulise launch is what the serial matching - one lane
per ligand - costs a library launch.  Each timed window is `--calls` back-to-back calls between two events, after a warm-up; a line
reports the median and the spread of `--windows` windows per call.  There is no time gate: nobody has measured this before.

    python tools/aromaticity_time.py [--out file]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aromaticity_ref as ref  # noqa: E402
from physdock_amd.ligand import Ligand, LigandLibrary  # noqa: E402
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
    distinct = [Ligand.from_smiles(s) for s in lines]
    lib = LigandLibrary([distinct[k % len(distinct)] for k in range(args.ligands)])
    kek = lib.kekulized("cuda")                                                      # the Kekule library: what perceive is for
    status = lib.aromaticity("normalise", device="cuda")
    assert not status["status"].any() and int(status["counts"][:, 3].sum()) > 0
    steps = status["counts"][:, 3].cpu().numpy()
    runs = (("kekulise", lambda: lib.aromaticity("kekulise", device="cuda")),
            ("kekulise with a budget of 0 steps", lambda: lib.aromaticity("kekulise", 0, "cuda")),
            ("perceive (Kekule input)", lambda: kek.aromaticity("perceive", device="cuda")),
            ("normalise", lambda: lib.aromaticity("normalise", device="cuda")),
            ("features", lambda: lib.features("cuda")),
            ("features(aromatize=True)", lambda: lib.features("cuda", aromatize=True)))
    t_gpu = {name: per_call_us(fn, args.calls, args.windows) for name, fn in runs}
    t_host = {}
    graphs = [ref.graph(lig) for lig in distinct]
    for mode in ("kekulise", "normalise"):
        t0 = time.perf_counter()
        for g in graphs:
            ref.run(g, mode)
        t_host[mode] = (time.perf_counter() - t0) / len(graphs)
    line = (f"G={args.ligands} ligands of {min(l.n_atoms for l in distinct)} .. {max(l.n_atoms for l in distinct)} atoms ({lib.n_atoms} atoms, "
            f"{lib.n_bonds} bonds, {int(steps.min())} .. {int(steps.max())} matching steps per ligand); per launch, median (min, max) over "
            f"{args.windows} windows of {args.calls} calls, one kernel plus four allocations, untuned: "
            + "; ".join(f"{name} {t[0]:.1f} us ({t[1]:.1f}, {t[2]:.1f})" for name, t in t_gpu.items())
            + f"; normalise {t_gpu['normalise'][0] / args.ligands:.3f} us per ligand; the Python restatement on the host: kekulise "
            f"{t_host['kekulise'] * 1e3:.2f} ms per ligand, normalise {t_host['normalise'] * 1e3:.2f} ms per ligand, "
            f"{t_host['normalise'] * args.ligands:.2f} s for the library")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
