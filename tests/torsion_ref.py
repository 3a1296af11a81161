"""Float64 definition of the torsion fingerprint and the torsion-fingerprint deviation TFD (physdock_amd/torsions.py, kernels
pd_torsion_prepare / pd_torsion_tfd / pd_torsion_deviation, csrc/torsion.hip) in plain numpy - the yardstick of
tests/test_torsion_cpu.py and tests/test_torsion_gpu.py.  Nothing of physdock_amd is imported.  After Schulz-Gasch, Schaerfer, Guba &
Rarey 2012; the package's own definition, not RDKit's bytes.

Entries, over the heavy-atom bond graph:
    one per rotatable bond (b, c) - single, in no ring, both ends with at least two neighbours, neither end on a triple bond -
        with ALL quadruples (a, b, c, d), a a neighbour of b other than c, d a neighbour of c other than b (at most 9); max_dev 180
    one per ring of 4 .. 8 atoms - every chordless simple cycle, in canonical cyclic order (from its smallest atom towards the
        smaller of that atom's two ring neighbours) - with the n consecutive quadruples; max_dev = 180 exp(-0.025 (n - 14)^2)
    rotatable bonds first, in the order of the bond list, then the rings in ascending order of their atom tuples
Angle of a quadruple: the IUPAC dihedral in degrees, float64 from the fp32 coordinates, atan2(|b2| b1.(b2 x b3), (b1 x b2).(b2 x b3));
    NaN when a coordinate is not finite or |b1 x b2|^2 <= 1e-12 |b1|^2 |b2|^2 (or the same for b2, b3)
dev_t(x, y) = min(1, mean over the entry's quadruples of |wrap(theta_x - theta_y)| / max_dev_t)
w_t = exp(-beta d_t^2), beta = ln 10 / (max(1, max_t d_t) / 2)^2, d_t the smallest topological distance from an atom of the bond / ring
    to C, the atoms with the smallest sum of topological distances to all atoms (a pair in different components counts n_atoms)
TFD(x, y) = sum_t w_t dev_t / sum_t w_t; 0 when there is no entry; NaN when a quadruple it names has no angle in x or in y
with a permutation table: min_m TFD(x, y o perm_m), x read at (a, b, c, d), y at (perm_m[a], .., perm_m[d]); a NaN never wins, the
    smallest m wins a tie, NaN and row -1 when every m is NaN

Tolerance.  Every angle is evaluated in two algebraically different float64 forms: `dihedral` (atan2) and `dihedral_acos` (the acos of
the normalised normals' dot product with the sign of the triple product).  For one (x, y, m) the disagreement propagated through the
definition is  E_m = sum_t w_t mean_q (e_x[q] + e_y[q']) / max_dev_t / sum_t w_t  (e the circular distance of the two forms of one
angle; the circular distance, the mean and the cut at 1 are all 1-Lipschitz), E = max_m E_m, and

    B = 4 E + (Nq + T + 64) 2^-52 max_t (180 / max_dev_t)          |D - TFD_ref| <= B + 1 ulp32(TFD_ref)

The second term: a value is a weighted mean of T terms (each <= 1) of means of Nq circular distances in all, every one of which carries
the few roundings of one angle (differences of fp32 coordinates are exact in float64; with bond angles of 90 .. 150 degrees the cross
products are well conditioned) scaled by 180 / max_dev_t <= 12.2; 64 covers those roundings, the atan2 and the division."""
import numpy as np

EPS52 = 2.0 ** -52
ROT, RING = "bond", "ring"


# ------------------------------------------------------------------ perception
def adjacency(n, bonds):
    adj = [set() for _ in range(n)]
    for i, j in bonds:
        adj[int(i)].add(int(j)); adj[int(j)].add(int(i))
    return adj


def _reach(adj, start, banned):
    """the atoms reachable from `start` without crossing the bond start-banned"""
    seen, stack = {start}, [start]
    while stack:
        a = stack.pop()
        for b in adj[a]:
            if (a == start and b == banned) or b in seen:
                continue
            seen.add(b); stack.append(b)
    return seen


def rotatable_bonds(n, bonds, orders=None):
    bonds = [(int(i), int(j)) for i, j in bonds]
    orders = [1.0] * len(bonds) if orders is None else [float(o) for o in orders]
    adj = adjacency(n, bonds)
    triple = {a for b, o in zip(bonds, orders) if o == 3.0 for a in b}
    return [(i, j) for (i, j), o in zip(bonds, orders)
            if o == 1.0 and len(adj[i]) >= 2 and len(adj[j]) >= 2 and i not in triple and j not in triple and j not in _reach(adj, i, j)]


def rings(n, bonds, lo=4, hi=8):
    """every chordless simple cycle of lo .. hi atoms as a tuple in canonical cyclic order, ascending"""
    adj = adjacency(n, bonds)
    out = []

    def grow(path):
        s = path[0]
        for u in sorted(adj[path[-1]]):
            if u <= s or u in path or any(u in adj[p] for p in path[1:-1]):
                continue
            if len(path) >= 2 and u in adj[s]:
                if len(path) + 1 >= lo and path[1] < u:
                    out.append(tuple(path + [u]))
                continue
            if len(path) + 1 < hi:
                grow(path + [u])

    for s in range(n):
        grow([s])
    return sorted(out)


def ring_max_dev(n):
    return 180.0 * float(np.exp(-0.025 * (n - 14) ** 2))


def entries(n, bonds, orders=None):
    """the fingerprint: a list of dict(kind, atoms, quads [(a, b, c, d)], max_dev)"""
    adj = adjacency(n, bonds)
    out = []
    for b, c in rotatable_bonds(n, bonds, orders):
        quads = [(a, b, c, d) for a in sorted(adj[b] - {c}) for d in sorted(adj[c] - {b})]
        out.append(dict(kind=ROT, atoms=(b, c), quads=quads, max_dev=180.0))
    for r in rings(n, bonds):
        k = len(r)
        out.append(dict(kind=RING, atoms=r, quads=[tuple(r[(i + s) % k] for s in range(4)) for i in range(k)], max_dev=ring_max_dev(k)))
    return out


def topological_distances(n, bonds):
    adj = adjacency(n, bonds)
    D = np.full((n, n), n, dtype=np.int64)
    for s in range(n):
        D[s, s] = 0
        front, d = [s], 0
        while front:
            d += 1
            nxt = []
            for a in front:
                for b in adj[a]:
                    if D[s, b] == n and b != s:
                        D[s, b] = d; nxt.append(b)
            front = nxt
    return D


def entry_distances(n, bonds, ents):
    D = topological_distances(n, bonds)
    tot = D.sum(1)
    C = np.nonzero(tot == tot.min())[0]
    return np.array([min(int(D[a, c]) for a in e["atoms"] for c in C) for e in ents], dtype=np.int64), C


def weights(n, bonds, ents):
    if not ents:
        return np.zeros(0)
    d, _ = entry_distances(n, bonds, ents)
    beta = np.log(10.0) / (max(1.0, float(d.max())) / 2.0) ** 2
    return np.exp(-beta * d.astype(np.float64) ** 2)


# ------------------------------------------------------------------ angles
def _vectors(p):
    p = np.asarray(p, dtype=np.float64)
    b1, b2, b3 = p[1] - p[0], p[2] - p[1], p[3] - p[2]
    return b1, b2, b3, np.cross(b1, b2), np.cross(b2, b3)


def _exists(p, b1, b2, b3, n1, n2):
    return bool(np.isfinite(p).all() and n1 @ n1 > 1e-12 * (b1 @ b1) * (b2 @ b2) and n2 @ n2 > 1e-12 * (b2 @ b2) * (b3 @ b3))


def dihedral(p):
    """p [4,3] -> degrees in (-180, 180], or NaN"""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        b1, b2, b3, n1, n2 = _vectors(p)
        if not _exists(p, b1, b2, b3, n1, n2):
            return np.nan
        return float(np.degrees(np.arctan2(np.sqrt(b2 @ b2) * (b1 @ n2), n1 @ n2)))


def dihedral_acos(p):
    """the same angle by the other route: acos of the unit normals' dot product, the sign of the triple product b1.(b2 x b3)"""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        b1, b2, b3, n1, n2 = _vectors(p)
        if not _exists(p, b1, b2, b3, n1, n2):
            return np.nan
        c = (n1 / np.sqrt(n1 @ n1)) @ (n2 / np.sqrt(n2 @ n2))
        a = float(np.degrees(np.arccos(min(1.0, max(-1.0, c)))))
        return -a if b1 @ n2 < 0 else a


def circ(a, b):
    d = abs(a - b)
    return 360.0 - d if d > 180.0 else d


def angles(x, quads, fn=dihedral):
    """x [L,3], quads [(a,b,c,d)] -> float64 [len(quads)] degrees"""
    x = np.asarray(x)
    return np.array([fn(x[list(q)]) for q in quads], dtype=np.float64).reshape(len(quads))


# ------------------------------------------------------------------ TFD
def ulp32(v):
    s = np.float32(abs(v))
    return float(np.nextafter(s, np.float32(np.inf)) - s)


def value_bound(B, v):
    return B + ulp32(v)


def amplification(ents):
    return max([180.0 / e["max_dev"] for e in ents] + [1.0])


def tfd(x, y, ents, w, perms=None):
    """x, y [L,3] (the ligand alone, fp32 or float64 holding fp32 values), ents as `entries` gives them, w [T] -> dict(tfd, row, per_m [M],
    dev [M,T] (normalised per-entry deviations; NaN where an angle is missing), E, B)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    T = len(ents)
    perms = np.arange(x.shape[0])[None] if perms is None else np.asarray(perms, dtype=np.int64)
    M = perms.shape[0]
    if T == 0:
        return dict(tfd=0.0, row=0, per_m=np.zeros(M), dev=np.zeros((M, 0)), E=0.0, B=64 * EPS52)
    w = np.asarray(w, dtype=np.float64)
    nq = sum(len(e["quads"]) for e in ents)
    per_m, dev, Em = np.full(M, np.nan), np.full((M, T), np.nan), np.zeros(M)
    ax = [angles(x, e["quads"]) for e in ents]
    ex = [np.array([circ(a, b) for a, b in zip(ax[t], angles(x, e["quads"], dihedral_acos))]) for t, e in enumerate(ents)]
    for m in range(M):
        p = perms[m]
        num = err = 0.0
        for t, e in enumerate(ents):
            img = [tuple(int(p[a]) for a in q) for q in e["quads"]]
            ay, ay2 = angles(y, img), angles(y, img, dihedral_acos)
            d = np.array([circ(a, b) for a, b in zip(ax[t], ay)])
            dev[m, t] = min(1.0, d.mean() / e["max_dev"]) if np.isfinite(d).all() else np.nan
            num += w[t] * dev[m, t]
            err += w[t] * (ex[t] + np.array([circ(a, b) for a, b in zip(ay, ay2)])).mean() / e["max_dev"]
        per_m[m] = num / w.sum()
        Em[m] = err / w.sum()
    ok = np.isfinite(per_m)
    if not ok.any():
        return dict(tfd=np.nan, row=-1, per_m=per_m, dev=dev, E=np.nan, B=np.nan)
    row = int(np.argmin(np.where(ok, per_m, np.inf)))
    E = float(Em[ok].max())
    return dict(tfd=float(per_m[row]), row=row, per_m=per_m, dev=dev, E=E, B=4.0 * E + (nq + T + 64) * EPS52 * amplification(ents))


def gather(x, idx, L):
    x = np.asarray(x)
    return x[:, np.arange(L) if idx is None else np.asarray(idx, dtype=np.int64)].astype(np.float64)


def cross(xa, idx_a, xb, idx_b, ents, w, perms, L):
    """xa [na,Aa,3], xb [nb,Ab,3] -> [na][nb] `tfd` dicts: rows fixed, columns permuted"""
    a, b = gather(xa, idx_a, L), gather(xb, idx_b, L)
    return [[tfd(p, q, ents, w, perms) for q in b] for p in a]


def field(res, key):
    return np.array([[r[key] for r in row] for row in res])


def pairwise(x, idx, ents, w, perms, L):
    """the symmetric form: i < j computed (pose i fixed, pose j permuted) and mirrored; the diagonal 0, or NaN for a structure one of
    whose own angles is missing -> D [n,n], B [n,n]"""
    res = cross(x, idx, x, idx, ents, w, perms, L)
    n = len(res)
    D, B = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        D[i, i] = 0.0 if np.isfinite(res[i][i]["per_m"][0]) else np.nan
        for j in range(i + 1, n):
            D[i, j] = D[j, i] = res[i][j]["tfd"]
            B[i, j] = B[j, i] = res[i][j]["B"]
    return D, B
