"""Time CanonicalForm (csrc/canonical.hip) with device events on a library of 1024 ligands - the five demo SMILES of
tests/golden/smiles_demo.txt, cycled: ONE launch of LigandLibrary.canonical, the same with `aromatize=True` (two launches) and the
launch behind `first_of` (pd_canonical_first: with five distinct molecules every ligand past the fifth finds its first among the first
five keys it reads, but every thread still reads the keys of all ligands before it), next to the Python restatement of the definition
on the host (tests/canonical_ref.py, wall clock: the five distinct ligands scaled to 1024) and the host SMILES writer.  The demo
ligands need 2 .. 3 refinement steps each; a symmetric ligand costs in proportion to its steps (hexaphenylbenzene 1531), which the
second block of the line shows on a library of 64 of them.  Each timed window is `--calls` back-to-back calls between two events,
after a warm-up; a line reports the median and the spread of `--windows` windows per call.  There is no time gate: nobody has measured
this before.

    python tools/canonical_time.py [--out file]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import canonical_ref as ref  # noqa: E402
from physdock_amd import ops  # noqa: E402
from physdock_amd.canonical import write_smiles  # noqa: E402
from physdock_amd.ligand import Ligand, LigandLibrary  # noqa: E402
from sasa_time import per_call_us  # noqa: E402

HEXAPHENYLBENZENE = "c1ccccc1-c1c(-c2ccccc2)c(-c2ccccc2)c(-c2ccccc2)c(-c2ccccc2)c1-c1ccccc1"


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--ligands", type=int, default=1024)
    args = ap.parse_args()
    with open(os.path.join(REPO, "tests", "golden", "smiles_demo.txt")) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    distinct = [Ligand.from_smiles(s) for s in lines]
    lib = LigandLibrary([distinct[k % len(distinct)] for k in range(args.ligands)])
    form = lib.canonical(device="cuda")
    t0 = time.perf_counter()
    want = [ref.canonical(lig) for lig in distinct]
    t_ref = (time.perf_counter() - t0) / len(distinct)
    cert = form.cert.cpu().tolist()
    for k in range(args.ligands):
        assert cert[int(form.cert_start[k]):int(form.cert_start[k + 1])] == want[k % len(distinct)]["cert"]
    assert form.first_of.cpu().tolist() == [k % len(distinct) for k in range(args.ligands)]
    t0 = time.perf_counter()
    for lig, w in zip(distinct, want):
        write_smiles(lig, w["labels"])
    t_write = (time.perf_counter() - t0) / len(distinct)

    def first_of():
        first = torch.empty(form.n_ligands, device=form.cert.device, dtype=torch.int32)
        ops.check(ops._lib.init().pd_canonical_first(ops.ptr(form.key), ops.ptr(form.status), ops.ptr(form._cert_start_dev), ops.ptr(form.cert),
                                                     ops.ptr(first), form.n_ligands, int(form.cert.shape[0]), ops.stream()), "pd_canonical_first")
        return first

    heavy = LigandLibrary([Ligand.from_smiles(HEXAPHENYLBENZENE)] * 64)
    steps = int(heavy.canonical(device="cuda").steps[0])
    runs = (("canonical", lambda: lib.canonical(device="cuda")), ("canonical(aromatize=True)", lambda: lib.canonical(aromatize=True, device="cuda")),
            ("first_of", first_of), ("canonical of 64 x hexaphenylbenzene", lambda: heavy.canonical(device="cuda")))
    t_gpu = {name: per_call_us(fn, args.calls, args.windows) for name, fn in runs}
    line = (f"G={args.ligands} ligands of {min(l.n_atoms for l in distinct)} .. {max(l.n_atoms for l in distinct)} atoms ({lib.n_atoms} atoms, "
            f"{lib.n_bonds} bonds, {int(form.steps.min())} .. {int(form.steps.max())} steps, {int(form.cert.shape[0])} certificate words); per "
            f"call, median (min, max) over {args.windows} windows of {args.calls} calls, allocations included, untuned: "
            + "; ".join(f"{name} {t[0]:.1f} us ({t[1]:.1f}, {t[2]:.1f})" for name, t in t_gpu.items())
            + f" ({steps} steps each); the Python restatement on the host: {t_ref * 1e3:.2f} ms per ligand, {t_ref * args.ligands:.2f} s for the "
            f"library; write_smiles {t_write * 1e3:.2f} ms per ligand")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
