"""The relaxation cases tests/test_mmff_kernels_gpu.py runs through pd_mmff_relax, their float32 starts and their float64 reference
results (tests/mmff_ref.py) - CPU only, computed once per process and never modified.  tests/test_mmff_ref_cpu.py asserts on the
reference alone what the GPU comparison relies on: every decision of every case is taken with a margin, the cases together reach the
branches listed there, and the reference itself moves by a tenth of the GPU tolerance at most when the summation order changes.

One case is one launch of B = 4 samples of one molecule, `synthetic_terms(L, seed)`, centred at the origin.  The four starts:
    "noise"  equilibrium + noise * N(0, 1) per coordinate
    "shift"  the same with another draw, translated by 5 A * N(0, 1) (coordinates above 1 A enter the optimiser's relative tests)
    "far"    equilibrium + 3 * noise * N(0, 1): gradients above 100 kcal/mol/A, so the gradient-halving loop runs
    "min"    the reference's own minimum (relaxed until FORCE_TOL from the equilibrium, then rounded to float32): this sample leaves
             the iteration loop at once while its neighbours in the launch run on.  Finding the minimum costs hundreds of
             iterations, so only the cases with L <= 43 carry it; the larger ones take a second "noise" draw instead.

Sizes (dim = 3 L):                threads/atom   matvec_sym                          atom passes
     4   dim  12                  8              split, 21 parts of 1, 9 of them empty  1     (runs to convergence: FORCE_TOL)
     6   dim  18                  8              split, 14 parts of 2, 5 of them empty  1     (its converged start leaves through TOLX)
    12   dim  36                  8              split, 7 parts of 6, last clamped   1
    28   dim  84                  8              split, 3 parts of 28 columns        1
    29   dim  87                  8              split, 2 parts of 44, last clamped  1
    42   dim 126                  4              split, 2 parts of 63                1
    43   dim 129                  4              plain                               1
    85   dim 255                  2              plain (every thread but one busy)   1
    86   dim 258                  2              plain, second round of outputs      1
   128   dim 384                  2              plain                               1
   129   dim 387                  1              plain                               1
   300   dim 900                  1              plain                               2, the last one ragged
"""
import collections
import functools

import numpy as np

import mmff_ref as mr

Case = collections.namedtuple("Case", "L seed noise iters starts")

_SMALL = ("noise", "min", "far", "shift")
_LARGE = ("noise", "noise", "far", "shift")

CASES = (
    Case(4, 7, 0.10, 40, _SMALL),
    Case(6, 20, 0.10, 10, _SMALL),
    Case(12, 1, 0.10, 40, _SMALL),
    Case(28, 1, 0.12, 5, _SMALL),
    Case(28, 1, 0.12, 0, _SMALL),
    Case(29, 1, 0.12, 30, _SMALL),
    Case(42, 5, 0.12, 3, _SMALL),
    Case(43, 1, 0.12, 5, _SMALL),
    Case(85, 1, 0.10, 3, _LARGE),
    Case(86, 1, 0.10, 5, _LARGE),
    Case(128, 1, 0.10, 3, _LARGE),
    Case(129, 1, 0.10, 5, _LARGE),
    Case(300, 1, 0.10, 2, _LARGE),
)

TOL_A = 2e-5                    # kernel against reference, max-abs, Angstrom (the bound of tests/test_mmff_gpu.py)
SPREAD_A = 2e-6                 # reference against itself under another summation order


def case_id(c):
    return f"L{c.L}-seed{c.seed}-it{c.iters}"


@functools.lru_cache(maxsize=None)
def molecule(L, seed):
    """(MMFFTerms, prepared reference tables, equilibrium coordinates centred at the origin)"""
    from physdock_amd import mmff
    terms, coords = mmff.synthetic_terms(L, seed)
    return terms, mr.prepare(terms.as_numpy()), coords - coords.mean(0)


@functools.lru_cache(maxsize=None)
def minimum(L, seed):
    """the reference's converged minimum next to the equilibrium, as the float32 values a launch receives"""
    _, t, coords = molecule(L, seed)
    out, trace = mr.minimize(coords, t, max_iters=1500)
    assert trace["exit"] == "force_tol", trace["exit"]
    out = out - out.mean(0)
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def starts(case):
    """[4, L, 3] float32 (read-only)"""
    _, _, coords = molecule(case.L, case.seed)
    rng = np.random.default_rng(1000 + case.seed)
    out = []
    for kind in case.starts:
        if kind == "min":
            p = minimum(case.L, case.seed)
        else:
            p = coords + case.noise * (3.0 if kind == "far" else 1.0) * rng.normal(size=coords.shape)
            if kind == "shift":
                p = p + 5.0 * rng.normal(size=(1, 3))
        out.append(p.astype(np.float32))
    out = np.stack(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """([4, L, 3] float64 relaxed positions (read-only), [4] traces) of mmff_ref.minimize on the float32 starts"""
    _, t, _ = molecule(case.L, case.seed)
    res = [mr.minimize(s.astype(np.float64), t, max_iters=case.iters) for s in starts(case)]
    out = np.stack([r[0] for r in res])
    out.setflags(write=False)
    return out, [r[1] for r in res]
