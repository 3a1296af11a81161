"""Time SubstructureSearch (csrc/substructure.hip) with device events on a library of 1024 ligands - the five demo SMILES of
tests/golden/smiles_demo.txt, cycled - against 32 functional-group queries: ONE launch of LigandLibrary.substructure (two more with
a `$()` in the set and `aromatize=True`), `matches(q, 16)` for one query and `pharmacophore_invariants`, next to the Python
restatement of the definition on the host (tests/substructure_ref.py, wall clock: the five distinct ligands x 32 queries scaled to
1024; for scale only).  The results are checked against the restatement first.  Each timed window is `--calls` back-to-back calls
between two events, after a warm-up; a line reports the median and the spread of `--windows` windows per call.  There is no time gate:
nobody has measured this before.

    python tools/substructure_time.py [--out file]
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
import substructure_ref as ref  # noqa: E402
from physdock_amd.ligand import Ligand, LigandLibrary  # noqa: E402
from physdock_amd.substructure import SubstructureQueries, pharmacophore_invariants  # noqa: E402
from sasa_time import per_call_us  # noqa: E402

#: 32 queries without a `$()`: one launch
QUERIES = ("c1ccccc1", "C#N", "C=O", "C(=O)N", "NC(=S)N", "[N-]", "Br", "C(F)(F)F", "c1ccoc1", "C1CCCCC1", "[#7;H1]", "[#8,#16;X1]", "c-c",
           "c:c:c", "[R0;D3]", "[CH3]", "cS", "cN", "a", "A", "*~*", "*~*~*", "[D1]", "[X4]", "C!@C", "*@*", "[#6]~[#7]~[#6]",
           "c1ccccc1C#N", "O=CNc", "[F,Cl,Br,I]", "[O-]", "S")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--ligands", type=int, default=1024)
    args = ap.parse_args()
    with open(os.path.join(REPO, "tests", "golden", "smiles_demo.txt")) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    distinct = [Ligand.from_smiles(s) for s in lines]
    n = len(distinct)
    lib = LigandLibrary([distinct[k % n] for k in range(args.ligands)])
    queries = SubstructureQueries(QUERIES)
    recursive = SubstructureQueries(list(QUERIES[:31]) + ["[N;!$(N-C=O)]"])
    assert queries.n_queries == 32 and queries.inner is None and recursive.inner is not None
    found = lib.substructure(queries, device="cuda")
    t0 = time.perf_counter()
    want = ref.library_search(distinct, queries.patterns)
    t_ref = (time.perf_counter() - t0) / n
    for key in ("n_embeddings", "n_unique", "status"):
        got = getattr(found, key).cpu().numpy()
        assert all(np.array_equal(got[k], want[key][k % n]) for k in range(args.ligands)), key
    assert not want["status"].any()
    q = QUERIES.index("c1ccccc1")
    rows = found.matches(q, 16)
    t0 = time.perf_counter()
    want_rows = [ref.matches(queries.patterns[q], ref.Graph(*ref.tables(lig)), 16) for lig in distinct]
    t_rows = (time.perf_counter() - t0) / n
    got_rows = rows["atoms"].cpu().numpy()
    assert all(np.array_equal(got_rows[k], want_rows[k % n][0]) for k in range(args.ligands))
    runs = (("substructure (32 queries)", lambda: lib.substructure(queries, device="cuda")),
            ("substructure (31 queries and one with a $(): two launches)", lambda: lib.substructure(recursive, device="cuda")),
            ("substructure(aromatize=True)", lambda: lib.substructure(queries, aromatize=True, device="cuda")),
            ("matches(c1ccccc1, 16)", lambda: found.matches(q, 16)),
            ("matches(c1ccccc1, 16, unique=False)", lambda: found.matches(q, 16, unique=False)),
            ("pharmacophore_invariants", lambda: pharmacophore_invariants(lib, device="cuda")))
    t_gpu = {name: per_call_us(fn, args.calls, args.windows) for name, fn in runs}
    ne = found.n_embeddings.sum(dim=1)
    line = (f"G={args.ligands} ligands of {min(l.n_atoms for l in distinct)} .. {max(l.n_atoms for l in distinct)} atoms ({lib.n_atoms} atoms, "
            f"{lib.n_bonds} bonds) x Q=32 queries of 1 .. {max(p.n_atoms for p in queries.patterns)} atoms ({int(ne.min())} .. {int(ne.max())} "
            f"embeddings per ligand over the 32, {int(found.has.sum())} of {args.ligands * 32} pairs match, max_steps 65536, every status 0); "
            f"per call, median (min, max) over {args.windows} windows of {args.calls} calls, allocations included, untuned: "
            + "; ".join(f"{name} {t[0]:.1f} us ({t[1]:.1f}, {t[2]:.1f})" for name, t in t_gpu.items())
            + f"; the Python restatement on the host, for scale only: the search {t_ref * 1e3:.1f} ms per ligand, {t_ref * args.ligands:.1f} s "
            f"for the library; matches(16) of one query {t_rows * 1e3:.2f} ms per ligand, {t_rows * args.ligands:.2f} s for the library")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
