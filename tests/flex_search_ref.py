"""Float64 NumPy definition of FlexSearch (FlexRefine.search, kernel pd_vina_flex_search in csrc/vina_flex.hip): the Monte-Carlo search of
VinaSearch with flexible receptor side chains - perturb the ligand or ONE chi angle, minimise the ligand and the side chains together,
Metropolis test, keep the best.  This is the package's own definition.  It is built from the two written definitions it joins:
`evaluate`, `move` and the BFGS of `refine` come from tests/flex_refine_ref.py unchanged, `draw` (Philox4x32-10) from
tests/vina_search_ref.py.  Nothing here imports the package.

With M = L + F movable rows, n = 6 + T + S, pose id q = pose0 + p and chain c:

    start       y = the movable rows of x[p] as float64;  (y_cur, E_cur) = descend(y): the BFGS of flex_refine_ref.refine from H = I with
                max_iters, grad_tol, max_step, the fixed rows read from x[p].  best = cur, best_step = 0: every chain of a pose begins at
                exactly FlexRefine.refine's result for that pose.
    step m      (m = 1 .. steps)  the draws of vina_search_ref.draw with the same counters (q, c, m, 0) and (q, c, m, 1); the one change
                is the entity, e = (w0 (2 + T + S)) >> 32.  s = 0 in R^n, then
                    e == 0                          s[0:3] = translate_amp (2 u_{1..3} - 1)
                    e == 1                          s[3:6] = rotate_amp (2 u_{1..3} - 1)        a rotation vector, radians
                    e == 2 + k, k < T               s[6 + k] = pi (2 u_1 - 1)                   a ligand torsion
                    e == 2 + k, T <= k < T + S      s[6 + k] = chi_amp (2 u_1 - 1)              a side-chain torsion; default chi_amp = pi
                y_prop = move(y_cur, s) (flex_refine_ref.move: the rigid part acts on the ligand rows alone);
                (y_new, E_new) = descend(y_prop) from a fresh H = I, in all n coordinates
                accept on E = (inter + intra) + receptor exactly as VinaSearch does: E_new finite and (E_new < E_cur or u_4 <
                exp((E_cur - E_new) / temperature)).  On accept cur = new.
                whatever the Metropolis test said: if E_new is finite and E_new < E_best (strict), best = new, best_step = m.
    per pose    best_chain = the chain with the lowest E_best, the lowest index on a tie.

With S = 0 this is vina_search_ref.search.  The uniform choice among the 2 + T + S entities is Vina's: a site with many chis spends most
of its steps on side chains (no weight parameter).  `order=-1` reverses every summation of the energy, as in the other references: the
twin run of the conditioning guard in tests/test_flex_search_cpu.py.

`GPU_CASES` are the (case, seed, settings) tuples of tests/test_flex_search_gpu.py, the cases those of flex_refine_ref.CASES.  Their
seeds were chosen on the CPU alone (tests/test_flex_search_cpu.py asserts the conditions, with vina_search_ref's U_MARGIN and E_MARGIN):
the run and its twin take the same decisions and end within 1e-8 A of each other, every Metropolis test has |u_4 - p| >= 1e-6, every
strict comparison of two energies a gap of at least 1e-9 kcal/mol or compares identical bits.  `BEHAVIOUR` is the (case, seed, settings)
of the behavioural test: a chain whose best comes from a side-chain proposal and ends below the local refinement."""
import numpy as np

import flex_refine_ref as ref
import vina_search_ref as vs

draw_words = vs.draw
U_MARGIN, E_MARGIN = vs.U_MARGIN, vs.E_MARGIN

DEFAULTS = dict(chains=8, steps=20, temperature=1.2, translate_amp=2.0, chi_amp=np.pi, max_iters=20, grad_tol=1e-4, max_step=1.0)

#: name -> (seed, settings): K = 3, steps <= 6, max_iters <= 10
GPU_CASES = {
    "small": (3, dict(chains=3, steps=6, max_iters=5, temperature=1.2, translate_amp=2.0, rotate_amp=0.7, chi_amp=np.pi)),
    "rigid_ligand": (2, dict(chains=3, steps=6, max_iters=10, temperature=1.2, translate_amp=2.0, rotate_amp=1.0, chi_amp=np.pi)),
    "no_flex": (37, dict(chains=3, steps=6, max_iters=10, temperature=1.2, translate_amp=2.0, rotate_amp=1.0, chi_amp=np.pi)),
    "over_block": (1, dict(chains=3, steps=2, max_iters=3, temperature=1.2, translate_amp=2.0, rotate_amp=0.7, chi_amp=1.0)),
    "full_chart": (0, dict(chains=3, steps=2, max_iters=3, temperature=1.2, translate_amp=2.0, rotate_amp=0.7, chi_amp=np.pi)),
}
#: (case, seed, settings) of the behavioural test
BEHAVIOUR = ("across", 3, dict(chains=3, steps=6, max_iters=5, temperature=1.2, translate_amp=2.0, rotate_amp=0.7, chi_amp=np.pi))


def draw(seed, q, chain, m, T, S=0):
    """(entity, u[0:5], w[0:5]) of step m of chain `chain` of pose id q: vina_search_ref.draw's words, the entity among 2 + T + S"""
    _, u, w = draw_words(seed, q, chain, m, T)
    return (w[0] * (2 + T + S)) >> 32, u, w


def proposal(e, u, T, S, translate_amp, rotate_amp, chi_amp=np.pi):
    s = np.zeros(6 + T + S)
    if e == 0:
        s[0:3] = [translate_amp * (2.0 * u[j] - 1.0) for j in (1, 2, 3)]
    elif e == 1:
        s[3:6] = [rotate_amp * (2.0 * u[j] - 1.0) for j in (1, 2, 3)]
    else:
        s[6 + e - 2] = (np.pi if e - 2 < T else chi_amp) * (2.0 * u[1] - 1.0)
    return s


def descend(c, xpose, y, max_iters, grad_tol, max_step, order=1):
    """the BFGS of flex_refine_ref.refine from the conformation y among the fixed atoms of xpose"""
    xp = np.array(xpose, dtype=np.float64)
    xp[np.asarray(c["mov_idx"], dtype=np.int64)] = y
    return ref.refine(c, xp, max_iters=max_iters, grad_tol=grad_tol, max_step=max_step, order=order)


def chain(c, xpose, q, k, steps, seed=0, temperature=1.2, translate_amp=2.0, rotate_amp=1.0, chi_amp=np.pi, max_iters=20, grad_tol=1e-4,
          max_step=1.0, order=1):
    """one chain -> the dict of vina_search_ref.chain over the movable rows (y_best [M,3], ...), with moved / moved_flex: the RMSD of the
    ligand rows / the flexible rows from the pose to y_best"""
    xpose = np.asarray(xpose, dtype=np.float64)
    T, S, L = c["T"], c["S"], c["L"]
    y0 = xpose[np.asarray(c["mov_idx"], dtype=np.int64)]
    d = descend(c, xpose, y0, max_iters, grad_tol, max_step, order)
    y_cur, e_cur = d["y"], d["energy"]
    y_best, e_best, best_step = y_cur, e_cur, 0
    out = dict(y_start=y_cur, energy_start=e_cur, start_iterations=d["iterations"], start_status=d["status"], entity=[], accept=[], new_best=[],
               iterations=[], status=[], u4=[], p=[], proposals=[], trace_energy=[e_cur], gaps=[], exact=[])
    accepted, evaluations = 0, d["evaluations"]
    for m in range(1, steps + 1):
        e, u, _ = draw(seed, q, k, m, T, S)
        y_prop = ref.move(c, y_cur, proposal(e, u, T, S, translate_amp, rotate_amp, chi_amp))
        d = descend(c, xpose, y_prop, max_iters, grad_tol, max_step, order)
        y_new, e_new = d["y"], d["energy"]
        evaluations += d["evaluations"]
        with np.errstate(over="ignore", invalid="ignore"):
            p = float(np.exp((e_cur - e_new) / temperature))
        fin = bool(np.isfinite(e_new))
        acc = fin and (e_new < e_cur or u[4] < p)
        nb = fin and e_new < e_best
        out["gaps"] += [abs(e_new - e_cur), abs(e_new - e_best)]
        out["exact"] += [np.array_equal(y_new, y_cur, equal_nan=True), np.array_equal(y_new, y_best, equal_nan=True)]
        if acc:
            y_cur, e_cur, accepted = y_new, e_new, accepted + 1
        if nb:
            y_best, e_best, best_step = y_new, e_new, m
        for key, v in (("entity", int(e)), ("accept", int(acc)), ("new_best", int(nb)), ("iterations", d["iterations"]), ("status", d["status"]),
                       ("u4", u[4]), ("p", p), ("proposals", y_prop), ("trace_energy", e_new)):
            out[key].append(v)
    with np.errstate(invalid="ignore"):
        d2 = ((y_best - y0) ** 2).sum(-1)
        moved = float(np.sqrt(d2[:L].mean()))
        moved_flex = float(np.sqrt(d2[L:].mean())) if len(y0) > L else 0.0
    out.update(y_best=y_best, energy=e_best, best_step=best_step, accepted=accepted, evaluations=evaluations, y_cur=y_cur, energy_cur=e_cur,
               moved=moved, moved_flex=moved_flex)
    return out


def search(c, x=None, chains=8, steps=20, pose0=0, order=1, **kw):
    """every pose of x [P,A,3] (default: the case's own) -> dict(chains: [P][K] of `chain`, best_chain [P], energy [P], y [P,M,3])"""
    x = c["x"] if x is None else x
    runs = [[chain(c, x[p], pose0 + p, k, steps, order=order, **kw) for k in range(chains)] for p in range(len(x))]
    best = [int(np.argmin([r["energy"] for r in row])) for row in runs]                # argmin: the first of equal minima
    return dict(chains=runs, best_chain=best, energy=[row[b]["energy"] for row, b in zip(runs, best)],
                y=np.stack([row[b]["y_best"] for row, b in zip(runs, best)]))
