"""Float64 NumPy definition of ShapeOverlap (physdock_amd/shape.py, csrc/shape_overlap.hip): first-order Gaussian shape and feature
("colour") overlap after Grant, Gallardo & Pickup 1996, its error bound, its gradient, the principal-axes starts and the rigid-body
overlay.  Nothing here imports the package; `move` and `generalised` are the ones of tests/vina_refine_ref.py at zero torsions.  It is
the package's own definition, not ROCS's bytes.

Atom i carries p exp(-a_i |r - x_i|^2), p = 2 sqrt 2, a_i = KAPPA / R_i^2, KAPPA = pi (3 p / (4 pi))^(2/3): one Gaussian's volume
p (pi / a)^(3/2) is its sphere's 4 pi R^3 / 3.  O(A,B) = sum_i sum_j p^2 exp(-a_i a_j d_ij^2 / (a_i + a_j)) (pi / (a_i + a_j))^(3/2), no
higher orders, O(A,A) with i = j.  A feature is (kind, members): its point is the float64 mean of the members, its radius 1 A; only
equal kinds overlap: C(A,B).  tanimoto = X_AB / (X_AA + X_BB - X_AB), colour 0 where the denominator is 0; combo = shape + colour.  A
structure with a non-finite named coordinate scores NaN.

The bound is derived, not fitted, with u = 2^-53.  One pair: the coordinate difference u, the three squares and two additions 4u:
d^2 within 5u relative (feature points add their mean's error, (m + 1) u max|x| per coordinate, to the difference); k = a_i a_j / s
3u; so the exponent e = k d^2 moves by (8 + c) u e and the exponential by that relative amount plus the device exp's documented 1 ulp
= 2u; the prefactor (pi / s)^(3/2) by 1 + 1 + 1 + 2 + 1 = 6u (sum, quotient, root, product), the two products 2u:  |t_dev - t| <=
(8 e + 10 + c e) u t.  A sum of n non-negative numbers in any order is within (n - 1) u of itself relatively; n <= L M.  The Tanimoto
x / (a + b - x) moves by (dx (a + b) + x (da + db)) / den^2 and four roundings, fp32 outputs by half an fp32 ulp more (the tests allow
one).

Overlay: maximise O(move(A, s), B) over s in R^6 (rotation vector about A's unweighted centroid, then translation) with the minimiser
of tests/vina_refine_ref.py (dfpmin / lnsrch, its constants, the chart re-centred after every accepted step, the direction cut to
max_step), E = -O.  Starts 0 .. 3: A's centroid on B's, A's principal axes on B's, turned by 180 degrees about (none, axis 1, 2, 3);
start 4: the pose as it stands.  The principal axes: eigenvalues of the second-moment matrix (central, / n) by ten sweeps of the
cyclic Jacobi of csrc/geom3.h, descending; the vector of the largest and of the middle eigenvalue as the largest cross product of two
rows of C - lambda I, normalised, the second made orthogonal to the first; each signed so that its largest-magnitude component is
positive; the third their cross product.  When an axis is not determined the four turned starts only superpose the centroids.  The
start with the largest overlap wins, the lowest index on a tie; colour is scored at that optimum.  `margin` reports how far the
discrete decisions were from flipping: `axes` (the relative eigenvalue gaps and the sign rule), `line_search` (the smallest distance of
an acceptance test from its threshold, in units of the two energies' error bounds), `grad` (the stopping test, relative to grad_tol)
and `start` (the lead of the winning start over the next, in units of the overlap's bound)."""
import numpy as np

import vina_refine_ref as vrr

U = 2.0 ** -53
P = 2.0 * np.sqrt(2.0)
P2 = 8.0
KAPPA = float(np.pi * (3.0 * P / (4.0 * np.pi)) ** (2.0 / 3.0))
DEFAULT_RADIUS, FEATURE_RADIUS = 1.7, 1.0
COLOR_ALPHA = KAPPA / FEATURE_RADIUS ** 2
FEATURE_NAMES = ("donor", "acceptor", "cation", "anion", "hydrophobe", "ring")
FUNCTOL, MOVETOL, EPS = vrr.FUNCTOL, vrr.MOVETOL, vrr.EPS
RIGID = dict(rot=[], sets=[])


def alphas(radii):
    return KAPPA / np.asarray(radii, dtype=np.float64) ** 2


def feature_points(y, feats):
    """feats: list of (kind, members) -> (points float64 [F,3], kinds int [F], members per feature)"""
    y = np.asarray(y, dtype=np.float64)
    pts = np.zeros((len(feats), 3))
    for f, (_, m) in enumerate(feats):
        pts[f] = y[np.asarray(m, dtype=np.int64)].sum(0) / len(m)
    return pts, np.asarray([k for k, _ in feats], dtype=np.int64), np.asarray([len(m) for _, m in feats], dtype=np.float64)


def pair_terms(xa, aa, xb, ab):
    """t [L,M] and the exponent e [L,M]"""
    d = xa[:, None, :] - xb[None]
    d2 = (d * d).sum(-1)
    s = aa[:, None] + ab[None]
    k = aa[:, None] * ab[None] / s
    q = np.pi / s
    e = k * d2
    return P2 * np.exp(-e) * (q * np.sqrt(q)), e, k, d


def overlap(xa, aa, xb, ab, ka=None, kb=None, ma=None, mb=None, per_atom=False):
    """(O, bound[, per-atom shares and their bounds]); ka / kb: kinds (only equal kinds count); ma / mb: members per point (the
    points are means, which widens the bound)"""
    xa, xb = np.asarray(xa, dtype=np.float64).reshape(-1, 3), np.asarray(xb, dtype=np.float64).reshape(-1, 3)
    if len(xa) == 0 or len(xb) == 0:
        return (0.0, 0.0) + ((np.zeros(len(xa)), np.zeros(len(xa))) if per_atom else ())
    with np.errstate(invalid="ignore", over="ignore"):
        t, e, k, d = pair_terms(xa, aa, xb, ab)
        if ka is not None:
            t = np.where(ka[:, None] == kb[None], t, 0.0)
        rel = 8.0 * e + 10.0
        if ma is not None:
            cmax = max(np.abs(xa).max(), np.abs(xb).max())
            dd = (ma[:, None] + mb[None] + 2.0) * U * cmax * np.sqrt(3.0)
            rel = rel + 2.0 * k * np.sqrt((d * d).sum(-1)) * dd / U
        n = xa.shape[0] * xb.shape[0]
        rows = t.sum(1)
        brow = (t * rel).sum(1) * U + xb.shape[0] * U * rows
        o = float(rows.sum())
        b = float(brow.sum() + n * U * o)
    return (o, b, rows, brow) if per_atom else (o, b)


def _tanimoto(x, a, b, dx, da, db):
    den = a + b - x
    if not den > 0.0:
        return 0.0, 0.0
    t = x / den
    return t, (dx * (a + b) + x * (da + db)) / den ** 2 + 4.0 * U * t


def prepare(y, radii, feats):
    """one structure: dict(y, alpha, fp, kind, members, O, bO, C, bC, finite)"""
    y = np.asarray(y, dtype=np.float64)
    a = alphas(radii)
    fp, kind, mem = feature_points(y, feats)
    ca = np.full(len(fp), COLOR_ALPHA)
    o, bo = overlap(y, a, y, a)
    c, bc = overlap(fp, ca, fp, ca, kind, kind, mem, mem)
    return dict(y=y, alpha=a, feats=feats, fp=fp, kind=kind, members=mem, calpha=ca, O=o, bO=bo, C=c, bC=bc, finite=bool(np.isfinite(y).all()))


def score(A, B, per_atom=False):
    """two prepared structures -> dict(O_AB, C_AB, shape_tanimoto, color_tanimoto, combo, bound{...}[, atom_share])"""
    keys = ("O_AB", "C_AB", "shape_tanimoto", "color_tanimoto", "combo")
    if not (A["finite"] and B["finite"]):
        out = {k: np.nan for k in keys}
        out["bound"] = {k: 0.0 for k in keys}
        if per_atom:
            out["atom_share"] = np.full(len(A["y"]), np.nan)
            out["bound"]["atom_share"] = np.zeros(len(A["y"]))
        return out
    got = overlap(A["y"], A["alpha"], B["y"], B["alpha"], per_atom=per_atom)
    o, bo = got[0], got[1]
    c, bc = overlap(A["fp"], A["calpha"], B["fp"], B["calpha"], A["kind"], B["kind"], A["members"], B["members"])
    st, bst = _tanimoto(o, A["O"], B["O"], bo, A["bO"], B["bO"])
    ct, bct = _tanimoto(c, A["C"], B["C"], bc, A["bC"], B["bC"])
    out = dict(O_AB=o, C_AB=c, shape_tanimoto=st, color_tanimoto=ct, combo=st + ct,
               bound=dict(O_AB=bo, C_AB=bc, shape_tanimoto=bst, color_tanimoto=bct, combo=bst + bct + U * (st + ct)))
    if per_atom:
        out["atom_share"], out["bound"]["atom_share"] = got[2], got[3]
    return out


def tversky(o_ab, o_aa, o_bb, alpha):
    return o_ab / (alpha * o_aa + (1.0 - alpha) * o_bb)


# ------------------------------------------------------------------ gradient and rigid motion
def energy(y, aa, xb, ab):
    """E = -O(y, B), dE/dy [L,3], and the bound of E"""
    t, e, k, d = pair_terms(np.asarray(y, dtype=np.float64), aa, xb, ab)
    o = float(t.sum(1).sum())
    bound = float((t * (8.0 * e + 10.0)).sum() * U + t.size * U * o)
    return -o, ((2.0 * k * t)[..., None] * d).sum(1), bound


def quat_to_matrix(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def apply(x, quat, t):
    return np.asarray(x, dtype=np.float64) @ quat_to_matrix(np.asarray(quat, dtype=np.float64)).T + np.asarray(t, dtype=np.float64)


def _jacobi(app, aqq, apq, arp, arq):
    if apq == 0.0:
        return app, aqq, apq, arp, arq
    with np.errstate(over="ignore"):                                                  # a huge theta gives t = 0, as on the device
        theta = (aqq - app) / (2.0 * apq)
        t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    return app - t * apq, aqq + t * apq, 0.0, c * arp - s * arq, s * arp + c * arq


def _null_vector(m, lam):
    rows = np.array([[m[0] - lam, m[3], m[4]], [m[3], m[1] - lam, m[5]], [m[4], m[5], m[2] - lam]])
    best, nn = None, 0.0
    for a, b in ((0, 1), (0, 2), (1, 2)):
        v = np.cross(rows[a], rows[b])
        if best is None or v @ v > nn:
            best, nn = v, float(v @ v)
    return best / np.sqrt(nn) if nn > 0.0 else None


def _fix_sign(v):
    big = v[0]
    for c in (1, 2):
        if abs(v[c]) > abs(big):
            big = v[c]
    mags = np.sort(np.abs(v))
    return (-v if big < 0.0 else v), float(min(mags[2] - mags[1], abs(big)))


def principal_axes(y):
    """(centroid, V [3,3] rows = axes or None, margin)"""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    cen = y.sum(0) / n
    r = y - cen
    m = np.array([(r[:, a] * r[:, b]).sum() / n for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))])
    a00, a11, a22, a01, a02, a12 = m
    for _ in range(10):
        a00, a11, a01, a02, a12 = _jacobi(a00, a11, a01, a02, a12)
        a00, a22, a02, a01, a12 = _jacobi(a00, a22, a02, a01, a12)
        a11, a22, a12, a01, a02 = _jacobi(a11, a22, a12, a01, a02)
    hi, lo = max(a00, a11, a22), min(a00, a11, a22)
    mid = a00 + a11 + a22 - lo - hi
    v1, v2 = _null_vector(m, hi), _null_vector(m, mid)
    if v1 is None or v2 is None:
        return cen, None, 0.0
    v2 = v2 - (v2 @ v1) * v1
    n2 = float(v2 @ v2)
    if not n2 > 0.0:
        return cen, None, 0.0
    v2 = v2 / np.sqrt(n2)
    (v1, s1), (v2, s2) = _fix_sign(v1), _fix_sign(v2)
    V = np.stack([v1, v2, np.cross(v1, v2)])
    if not np.isfinite(V).all():
        return cen, None, 0.0
    gap = min(hi - mid, mid - lo) / hi if hi > 0.0 else 0.0
    return cen, V, float(min(gap, s1, s2))


TURNS = ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))


def starts(ya, yb):
    """the five start conformations of A and the margin of the axes"""
    ya, yb = np.asarray(ya, dtype=np.float64), np.asarray(yb, dtype=np.float64)
    ca, VA, ma = principal_axes(ya)
    cb, VB, mb = principal_axes(yb)
    out = []
    for d in TURNS:
        R = np.eye(3) if VA is None or VB is None else VB.T @ np.diag(d) @ VA
        out.append(cb + (ya - ca) @ R.T)
    out.append(ya.copy())
    return out, (min(ma, mb) if VA is not None and VB is not None else np.inf)


def descend(y0, aa, xb, ab, max_iters=50, grad_tol=1e-4, max_step=1.0):
    """the minimiser of vina_refine_ref.refine on E = -O in the six rigid coordinates -> dict(y, energy_start, energy, iterations,
    evaluations, status, margin)"""
    y = np.array(y0, dtype=np.float64)
    fp, gc, b0 = energy(y, aa, xb, ab)
    g = vrr.generalised(RIGID, y, gc)
    e_start, evaluations, iterations, status, margin, gmargin = fp, 1, 0, 1, np.inf, abs(np.abs(g).max() - grad_tol) / grad_tol
    H = np.eye(6)
    xi = -g
    if np.abs(g).max() < grad_tol:
        status = 0
    while status == 1 and iterations < max_iters:
        s = np.sqrt((xi * xi).sum())
        if s > max_step:
            xi = xi * (max_step / s)
        slope = float((xi * g).sum())
        if not slope < 0.0:
            status = 2
            break
        lam_min = MOVETOL / np.abs(xi).max()
        lam, lam2, val2, moved = 1.0, 0.0, 0.0, False
        for it in range(1000):
            if lam < lam_min:
                break
            yn = vrr.move(RIGID, y, lam * xi)
            fnew, gn, bn = energy(yn, aa, xb, ab)
            evaluations += 1
            margin = min(margin, abs(fnew - fp - FUNCTOL * lam * slope) / max(bn + b0, 1e-300))
            if fnew - fp <= FUNCTOL * lam * slope:
                moved = True
                break
            if it == 0:
                tmp = -slope / (2.0 * (fnew - fp - slope))
            else:
                rhs1, rhs2 = fnew - fp - lam * slope, val2 - fp - lam2 * slope
                a = (rhs1 / (lam * lam) - rhs2 / (lam2 * lam2)) / (lam - lam2)
                b = (-lam2 * rhs1 / (lam * lam) + lam * rhs2 / (lam2 * lam2)) / (lam - lam2)
                if a == 0.0:
                    tmp = -slope / (2.0 * b)
                else:
                    disc = b * b - 3.0 * a * slope
                    if disc < 0.0:
                        tmp = 0.5 * lam
                    elif b <= 0.0:
                        tmp = (-b + np.sqrt(disc)) / (3.0 * a)
                    else:
                        tmp = -slope / (b + np.sqrt(disc))
                if tmp > 0.5 * lam:
                    tmp = 0.5 * lam
            lam2, val2 = lam, fnew
            lam = max(tmp, 0.1 * lam)
        if not moved:
            status = 2
            break
        step = lam * xi
        y, fp, b0, g_old, g = yn, fnew, bn, g, vrr.generalised(RIGID, yn, gn)
        iterations += 1
        gmargin = min(gmargin, abs(np.abs(g).max() - grad_tol) / grad_tol)
        if np.abs(g).max() < grad_tol:
            status = 0
            break
        dg = g - g_old
        hdg = H @ dg
        fac, fae, sdg, sxi = float(dg @ step), float(dg @ hdg), float(dg @ dg), float(step @ step)
        if fac > np.sqrt(EPS * sdg * sxi):
            fac, fad = 1.0 / fac, 1.0 / fae
            v = fac * step - fad * hdg
            H = H + fac * np.outer(step, step) - fad * np.outer(hdg, hdg) + fae * np.outer(v, v)
        xi = -(H @ g)
    return dict(y=y, energy_start=e_start, energy=fp, iterations=iterations, evaluations=evaluations, status=status, margin=margin, grad_margin=gmargin,
                bound=b0)


def overlay(A, B, max_iters=50, grad_tol=1e-4, max_step=1.0):
    """two prepared structures -> dict(y (A's fitted atoms), fp (its fitted feature points), overlap, overlap_start, best_start,
    iterations, evaluations, status, shape_tanimoto, color_tanimoto, combo, bound (of the overlap), margin)"""
    ys, axes = starts(A["y"], B["y"])
    runs = [descend(y0, A["alpha"], B["y"], B["alpha"], max_iters, grad_tol, max_step) for y0 in ys]
    o = np.array([-r["energy"] for r in runs])
    best = int(np.argmax(o))                                                          # the first of equals
    rest = np.delete(o, best)
    margin = dict(axes=axes, line_search=min(r["margin"] for r in runs), grad=min(r["grad_margin"] for r in runs),
                  start=float((o[best] - rest.max()) / max(r["bound"] for r in runs)))
    r = runs[best]
    fitted = dict(A, y=r["y"], fp=feature_points(r["y"], A["feats"])[0]) if "feats" in A else None
    _, _, bound = energy(r["y"], A["alpha"], B["y"], B["alpha"])
    out = dict(y=r["y"], overlap=o[best], overlap_start=-runs[4]["energy_start"], best_start=best, iterations=r["iterations"],
               evaluations=r["evaluations"], status=r["status"], bound=bound, margin=margin, runs=runs)
    if fitted is not None:
        s = score(fitted, B)
        out.update(shape_tanimoto=s["shape_tanimoto"], color_tanimoto=s["color_tanimoto"], combo=s["combo"])
    return out


# ------------------------------------------------------------------ seeded molecules
def molecule(L, seed, n_feats=None, kinds=(0, 1, 2, 3, 4, 5), spread=None, ring=True):
    """a random self-avoiding chain of L atoms (1.5 A steps, elongated so that the principal axes are distinct), radii from a small
    set, and a feature table: single-member features of the given kinds and, with `ring`, one six-member ring feature"""
    rng = np.random.default_rng(5100 + seed)
    y = [np.zeros(3)]
    drift = np.array([1.0, 0.45, 0.15])
    while len(y) < L:
        v = rng.normal(size=3) + 1.2 * drift
        p = y[-1] + 1.5 * v / np.sqrt((v * v).sum())
        if all(((p - q) ** 2).sum() > 1.2 ** 2 for q in y):
            y.append(p)
    y = np.asarray(y) + rng.uniform(-2.0, 2.0, 3)
    if spread is not None:
        y = y * spread
    radii = rng.choice([1.7, 1.55, 1.6, 1.8], L)
    feats = []
    nf = min(L, 8) if n_feats is None else n_feats
    if len(kinds):
        for f in range(nf):
            feats.append((int(kinds[f % len(kinds)]), (int(rng.integers(L)),)))
        if ring and L >= 6 and 5 in kinds:
            feats.append((5, tuple(int(i) for i in rng.permutation(L)[:6])))
    return y.astype(np.float32), radii, feats
