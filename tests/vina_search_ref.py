"""Float64 NumPy definition of VinaSearch (VinaRefine.search, kernel pd_vina_search in csrc/vina_refine.hip): a Monte-Carlo global search
of every pose - perturb, minimise locally, Metropolis test, keep the best.  This is the package's own definition, not a port of Vina's
`monte_carlo`.  It is built from the written definition of VinaRefine: `evaluate`, `move` and the BFGS of `refine` come from
tests/vina_refine_ref.py unchanged, the Philox4x32-10 from tests/conformers_ref.py.  Nothing here imports the package.

For pose id q = pose0 + p and chain c, with n = 6 + T:

    start       y = the ligand rows of x[p] as float64;  (y_cur, E_cur) = descend(y): the BFGS of `refine` from H = I with max_iters,
                grad_tol, max_step, the receptor rows read from x[p].  best = cur, best_step = 0: every chain of a pose begins at
                exactly VinaRefine.refine's result for that pose.
    step m      (m = 1 .. steps)  Philox4x32-10 with the key (seed lo, seed hi): counter (q, c, m, 0) gives the words w0 .. w3,
                counter (q, c, m, 1) gives w4 as its first word;  u_j = (w_j + 0.5) 2^-32 in float64.
                entity e = (w0 (2 + T)) >> 32, in integers.  s = 0 in R^n, then
                    e == 0      s[0:3] = translate_amp (2 u_{1..3} - 1)
                    e == 1      s[3:6] = rotate_amp (2 u_{1..3} - 1)            a rotation vector, radians
                    e == 2 + k  s[6 + k] = pi (2 u_1 - 1)
                (a cube, not Vina's ball: every step uses a fixed number of words and no rejection loop)
                y_prop = move(y_cur, s);  (y_new, E_new) = descend(y_prop) from a fresh H = I
                accept iff E_new is finite and (E_new < E_cur or u_4 < exp((E_cur - E_new) / temperature)); temperature in kcal/mol,
                > 0, may be inf (then every finite E_new is accepted).  On accept cur = new.
                whatever the Metropolis test said: if E_new is finite and E_new < E_best (strict), best = new, best_step = m.
    per pose    best_chain = the chain with the lowest E_best, the lowest index on a tie.

`descend(y)` is `vina_refine_ref.refine` on the pose with its ligand rows replaced by y (the receptor rows are all it reads beside them),
so the BFGS exists once.  `order=-1` reverses every summation of the energy, as in vina_refine_ref: the twin run of the conditioning
guard in tests/test_vina_search_cpu.py.

`GPU_CASES` are the (case, seed, settings) tuples of tests/test_vina_search_gpu.py.  Their seeds were chosen on the CPU alone
(tests/test_vina_search_cpu.py asserts the conditions): the run and its twin take the same decisions and end within 1e-8 A of each
other, every Metropolis test has |u_4 - p| >= 1e-6, every strict comparison of two energies a gap of at least 1e-9 kcal/mol."""
import numpy as np

import conformers_ref
import vina_refine_ref as ref

philox4x32 = conformers_ref.philox4x32

DEFAULTS = dict(chains=8, steps=20, temperature=1.2, translate_amp=2.0, max_iters=20, grad_tol=1e-4, max_step=1.0)

#: name -> (seed, settings): K = 3, steps <= 6, max_iters <= 10
GPU_CASES = {
    "P2_A257_L6_T2": (37, dict(chains=3, steps=6, max_iters=10, temperature=1.2, translate_amp=2.0, rotate_amp=1.0)),
    "P3_A300_L12_T3": (1, dict(chains=3, steps=6, max_iters=3, temperature=1.2, translate_amp=2.0, rotate_amp=0.7)),
    "P2_A65_L1_T0": (4, dict(chains=3, steps=6, max_iters=10, temperature=1.2, translate_amp=2.0, rotate_amp=2.0)),
}
U_MARGIN, E_MARGIN = 1e-6, 1e-9


def radius_of_gyration(c, x0):
    """of the active ligand atoms of one pose x0 [A,3]"""
    y = np.asarray(x0, dtype=np.float64)[np.asarray(c["lig_idx"], dtype=np.int64)][np.asarray(c["lig_active"]) > 0]
    return float(np.sqrt(((y - y.mean(0)) ** 2).sum(-1).mean())) if len(y) else 0.0


def default_rotate_amp(c, x0, translate_amp=2.0):
    """the host's default: translate_amp / max(1, r_gyr) of the first pose (Vina's scaling)"""
    return translate_amp / max(1.0, radius_of_gyration(c, x0))


def draw(seed, q, chain, m, T):
    """(entity, u[0:5], w[0:5]) of step m of chain `chain` of pose id q"""
    key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    w = philox4x32(key, (q, chain, m, 0)) + philox4x32(key, (q, chain, m, 1))[:1]
    u = [(float(v) + 0.5) * 2.0 ** -32 for v in w]
    return (w[0] * (2 + T)) >> 32, u, w


def proposal(e, u, T, translate_amp, rotate_amp):
    s = np.zeros(6 + T)
    if e == 0:
        s[0:3] = [translate_amp * (2.0 * u[j] - 1.0) for j in (1, 2, 3)]
    elif e == 1:
        s[3:6] = [rotate_amp * (2.0 * u[j] - 1.0) for j in (1, 2, 3)]
    else:
        s[6 + e - 2] = np.pi * (2.0 * u[1] - 1.0)
    return s


def descend(c, xpose, y, max_iters, grad_tol, max_step, order=1):
    """the BFGS of vina_refine_ref.refine from the conformation y in the receptor of xpose"""
    xp = np.array(xpose, dtype=np.float64)
    xp[np.asarray(c["lig_idx"], dtype=np.int64)] = y
    return ref.refine(c, xp, max_iters=max_iters, grad_tol=grad_tol, max_step=max_step, order=order)


def chain(c, xpose, q, k, steps, seed=0, temperature=1.2, translate_amp=2.0, rotate_amp=1.0, max_iters=20, grad_tol=1e-4, max_step=1.0,
          order=1):
    """one chain -> dict(y_best [L,3], y_start, energy, energy_start, best_step, accepted, evaluations, and per step: entity, accept,
    new_best, iterations, status, u4, p (the Metropolis probability, > 1 downhill), proposals (y_prop), trace_energy [steps + 1],
    gaps: |difference| of every pair of energies a strict comparison looked at, exact: whether the two conformations of that
    comparison are the same bits - a proposal that moved nothing, such as the rotation of a single atom, from a converged point: the
    only way to an exact tie)"""
    xpose = np.asarray(xpose, dtype=np.float64)
    T = len(c["rot"])
    y0 = xpose[np.asarray(c["lig_idx"], dtype=np.int64)]
    d = descend(c, xpose, y0, max_iters, grad_tol, max_step, order)
    y_cur, e_cur = d["y"], d["energy"]
    y_best, e_best, best_step = y_cur, e_cur, 0
    out = dict(y_start=y_cur, energy_start=e_cur, start_iterations=d["iterations"], start_status=d["status"], entity=[], accept=[], new_best=[],
               iterations=[], status=[], u4=[], p=[], proposals=[], trace_energy=[e_cur], gaps=[], exact=[])
    accepted, evaluations = 0, d["evaluations"]
    for m in range(1, steps + 1):
        e, u, _ = draw(seed, q, k, m, T)
        y_prop = ref.move(c, y_cur, proposal(e, u, T, translate_amp, rotate_amp))
        d = descend(c, xpose, y_prop, max_iters, grad_tol, max_step, order)
        y_new, e_new = d["y"], d["energy"]
        evaluations += d["evaluations"]
        with np.errstate(over="ignore", invalid="ignore"):
            p = float(np.exp((e_cur - e_new) / temperature))
        fin = bool(np.isfinite(e_new))
        acc = fin and (e_new < e_cur or u[4] < p)
        nb = fin and e_new < e_best
        out["gaps"] += [abs(e_new - e_cur), abs(e_new - e_best)]
        out["exact"] += [np.array_equal(y_new, y_cur), np.array_equal(y_new, y_best)]
        if acc:
            y_cur, e_cur, accepted = y_new, e_new, accepted + 1
        if nb:
            y_best, e_best, best_step = y_new, e_new, m
        for key, v in (("entity", int(e)), ("accept", int(acc)), ("new_best", int(nb)), ("iterations", d["iterations"]), ("status", d["status"]),
                       ("u4", u[4]), ("p", p), ("proposals", y_prop), ("trace_energy", e_new)):
            out[key].append(v)
    out.update(y_best=y_best, energy=e_best, best_step=best_step, accepted=accepted, evaluations=evaluations, y_cur=y_cur, energy_cur=e_cur)
    return out


def search(c, x=None, chains=8, steps=20, pose0=0, order=1, **kw):
    """every pose of x [P,A,3] (default: the case's own) -> dict(chains: [P][K] of `chain`, best_chain [P], energy [P], y [P,L,3])"""
    x = c["x"] if x is None else x
    runs = [[chain(c, x[p], pose0 + p, k, steps, order=order, **kw) for k in range(chains)] for p in range(len(x))]
    best = [int(np.argmin([r["energy"] for r in row])) for row in runs]                # argmin: the first of equal minima
    return dict(chains=runs, best_chain=best, energy=[row[b]["energy"] for row, b in zip(runs, best)],
                y=np.stack([row[b]["y_best"] for row, b in zip(runs, best)]))
