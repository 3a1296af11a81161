"""The seeded cases the ShapeOverlap tests share (tests/shape_overlap_ref.py builds the molecules)."""
import numpy as np

import shape_overlap_ref as ref

#: overlay cases: name -> (atoms of A, atoms of B, seed, max_iters).  Chosen on the CPU alone so that every decision of the reference
#: keeps the margins test_shape_overlap_cpu.py asserts; the short max_iters cases end on status 1
OVERLAY_CASES = {"L6_M9_a": (6, 9, 0, 50), "L6_M9_b": (6, 9, 1, 50), "L6_M9_c": (6, 9, 2, 50), "L12_M12": (12, 12, 1, 50),
                 "L40_M17_short": (40, 17, 0, 6), "L25_M40_short": (25, 40, 2, 6)}
#: the smallest margins a usable overlay case keeps (see `margin` in shape_overlap_ref.overlay): the line search and the start
#: selection in units of the energies' error bounds - the device's energies are inside those bounds, so a margin of one bound cannot
#: flip; four leaves room for the roundoff the earlier steps of a descent pass on
MARGINS = dict(axes=1e-3, line_search=4.0, grad=1e-3, start=4.0)


def overlay_case(name):
    L, M, seed, mi = OVERLAY_CASES[name]
    ya, ra, fa = ref.molecule(L, seed)
    yb, rb, fb = ref.molecule(M, seed + 50)
    return dict(A=ref.prepare(ya, ra, fa), B=ref.prepare(yb, rb, fb), xa=ya, xb=yb, ra=ra, rb=rb, fa=fa, fb=fb, max_iters=mi)


def rigid(y, seed):
    """a seeded rigid motion of y: (moved fp32, R, t)"""
    rng = np.random.default_rng(900 + seed)
    w = rng.normal(size=3)
    w *= rng.uniform(0.3, 1.2) / np.sqrt((w * w).sum())
    th = np.sqrt((w * w).sum())
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    t = rng.uniform(-1.5, 1.5, 3)
    return (np.asarray(y, dtype=np.float64) @ R.T + t).astype(np.float32), R, t
