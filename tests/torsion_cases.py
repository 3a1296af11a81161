"""Inputs of tests/test_torsion_cpu.py and tests/test_torsion_gpu.py: small molecules built from internal coordinates (every bond angle
between 90 and 150 degrees, so that tests/torsion_ref.py alone is well conditioned), and synthetic kernel cases with the tables the C
ABI takes, built here in numpy without physdock_amd.  Ligands sit 60 - 100 A from the origin."""
import numpy as np

import torsion_ref as ref


# ------------------------------------------------------------------ geometry
def place(p1, p2, p3, r, theta, phi):
    """the point at distance r from p1 with the angle theta (degrees) at p1 towards p2 and the dihedral phi (p3, p2, p1, new)"""
    p1, p2, p3 = (np.asarray(p, dtype=np.float64) for p in (p1, p2, p3))
    t, f = np.radians(theta), np.radians(phi)
    bc = (p1 - p2) / np.linalg.norm(p1 - p2)
    n = np.cross(p2 - p3, bc)
    n /= np.linalg.norm(n)
    m = np.cross(n, bc)
    return p1 + r * (-np.cos(t) * bc + np.sin(t) * np.cos(f) * m + np.sin(t) * np.sin(f) * n)


def zmatrix(rows):
    """rows: (ref1, ref2, ref3, r, theta, phi) per atom after the first three, which are (), (0, r) and (1, 0, r, theta) -> [n,3]"""
    x = []
    for row in rows:
        if len(row) == 0:
            x.append(np.zeros(3))
        elif len(row) == 2:
            x.append(np.array([row[1], 0.0, 0.0]))
        elif len(row) == 4:
            a, b, r, th = row
            d = (x[b] - x[a]) / np.linalg.norm(x[b] - x[a])
            perp = np.array([-d[1], d[0], 0.0]) if abs(d[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
            perp -= perp @ d * d
            perp /= np.linalg.norm(perp)
            x.append(x[a] + r * (np.cos(np.radians(th)) * d + np.sin(np.radians(th)) * perp))
        else:
            a, b, c, r, th, ph = row
            x.append(place(x[a], x[b], x[c], r, th, ph))
    return np.array(x)


def moved(x, seed=0):
    """x [L,3] float64 -> fp32, rotated at random and carried 60 - 100 A from the origin"""
    rng = np.random.default_rng(4200 + seed)
    q = rng.standard_normal(4)
    w, a, b, c = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b)],
                  [2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a)],
                  [2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)]])
    d = rng.standard_normal(3)
    return (x @ R.T + d / np.linalg.norm(d) * rng.uniform(60, 100)).astype(np.float32)


# ------------------------------------------------------------------ molecules: dict(n, bonds, orders, elements) and coordinates
def butane(phi):
    mol = dict(n=4, bonds=[(0, 1), (1, 2), (2, 3)], orders=[1.0] * 3, elements=[6] * 4)
    return mol, zmatrix([(), (0, 1.53), (1, 0, 1.53, 112.0), (2, 1, 0, 1.53, 112.0, phi)])


def biphenyl(psi):
    """para-disubstituted biphenyl: ring A 0 .. 5, ring B 6 .. 11, the bond 0 - 6, Cl on 3, F on 9; ring B turned by psi about the axis"""
    bonds = [(k, (k + 1) % 6) for k in range(6)] + [(6 + k, 6 + (k + 1) % 6) for k in range(6)] + [(0, 6), (3, 12), (9, 13)]
    mol = dict(n=14, bonds=bonds, orders=[1.5] * 12 + [1.0] * 3, elements=[6] * 12 + [17, 9])
    r, cb = 1.39, 1.39 + 1.48 + 1.39
    ang = np.radians(60.0 * np.arange(6))
    A = np.stack([r * np.cos(ang), r * np.sin(ang), np.zeros(6)], 1)
    p = np.radians(psi)
    B = np.stack([cb - r * np.cos(ang), r * np.sin(ang) * np.cos(p), r * np.sin(ang) * np.sin(p)], 1)
    return mol, np.concatenate([A, B, [[-r - 1.74, 0, 0]], [[cb + r + 1.35, 0, 0]]])


def tbutyl(phi):
    """(CH3)3C-CH2-CH3: the quaternary carbon 0, methyls 1, 2, 3, then 4 and 5; the t-butyl group turned by phi about 0 - 4"""
    mol = dict(n=6, bonds=[(0, 1), (0, 2), (0, 3), (0, 4), (4, 5)], orders=[1.0] * 5, elements=[6] * 6)
    x = zmatrix([(), (0, 1.53), (0, 1, 1.53, 109.47)])          # 0, 4 (second row), 5 placed below
    q, a = x[0], x[1]
    b = place(a, q, q + np.array([0.3, 0.8, 0.5]), 1.53, 112.0, 0.0)
    me = [place(q, a, b, 1.53, 109.47, phi + k * 120.0) for k in range(3)]
    return mol, np.array([q] + me + [a, b])


def cyclohexane(sign=1.0):
    mol = dict(n=6, bonds=[(k, (k + 1) % 6) for k in range(6)], orders=[1.0] * 6, elements=[6] * 6)
    ang = np.radians(60.0 * np.arange(6))
    return mol, np.stack([1.45 * np.cos(ang), 1.45 * np.sin(ang), sign * 0.25 * (-1.0) ** np.arange(6)], 1)


def amide_ligand(omega, seed=3):
    """a 25-atom chain with an amide in the middle: .. 10 (C alpha) - 11 (C, =O 24) - 12 (N) - 13 ..; atoms 0 .. 23 the chain, with a
    methyl branch nowhere: every chain atom is placed by its own dihedral, so that omega (10, 11, 12, 13) moves nothing else"""
    rng = np.random.default_rng(seed)
    n = 25
    bonds = [(k, k + 1) for k in range(23)] + [(11, 24)]
    orders = [1.0] * 23 + [2.0]
    elements = [6] * 24 + [8]
    elements[12] = 7
    rows = [(), (0, 1.52), (1, 0, 1.52, 112.0)]
    for k in range(3, 24):
        phi = omega if k == 13 else float(rng.choice([60.0, -60.0, 180.0]) + rng.uniform(-15, 15))
        rows.append((k - 1, k - 2, k - 3, 1.50, float(rng.uniform(108, 122)), phi))
    x = zmatrix(rows)
    o = place(x[11], x[10], x[9], 1.23, 121.0, 30.0)
    return dict(n=n, bonds=bonds, orders=orders, elements=elements), np.concatenate([x, o[None]])


def chain(n):
    return dict(n=n, bonds=[(k, k + 1) for k in range(n - 1)], orders=[1.0] * (n - 1), elements=[6] * n)


# ------------------------------------------------------------------ tables for the C ABI, in numpy
def canonical(q):
    q = tuple(int(v) for v in q)
    return min(q, q[::-1])


def tables(ents, w, perms):
    """entries, weights, perms [M,L] -> dict(quads int32 [Q,4], image uint16 [Nq,M], qstart int32 [T+1], w, inv float64 [T]) as
    include/physdock_hip.h describes them"""
    base = [q for e in ents for q in e["quads"]]
    perms = np.asarray(perms, dtype=np.int64)
    images = [[canonical(p[list(q)]) for p in perms] for q in base]
    quads = sorted({q for row in images for q in row})
    ids = {q: k for k, q in enumerate(quads)}
    return dict(quads=np.asarray(quads, dtype=np.int32).reshape(-1, 4),
                image=np.asarray([[ids[q] for q in row] for row in images], dtype=np.uint16).reshape(len(base), perms.shape[0]),
                qstart=np.concatenate([[0], np.cumsum([len(e["quads"]) for e in ents])]).astype(np.int32),
                w=np.asarray(w, dtype=np.float64), inv=np.array([1.0 / e["max_dev"] for e in ents], dtype=np.float64))


# ------------------------------------------------------------------ synthetic kernel cases
def block_chains(rng, n, nblocks):
    """n structures of nblocks four-atom chains (atoms 4 k .. 4 k + 3): bond angles 95 .. 145 degrees, dihedrals uniform but at least
    2 degrees away from 0 and 180 (where the acos form of the reference loses digits) -> float64 [n, 4 nblocks, 3]"""
    out = np.zeros((n, 4 * nblocks, 3))
    for s in range(n):
        for k in range(nblocks):
            phi = rng.uniform(2.0, 178.0) * rng.choice([-1.0, 1.0])
            x = zmatrix([(), (0, rng.uniform(1.3, 1.6)), (1, 0, rng.uniform(1.3, 1.6), rng.uniform(95, 145)),
                         (2, 1, 0, rng.uniform(1.3, 1.6), rng.uniform(95, 145), phi)])
            out[s, 4 * k:4 * k + 4] = x + rng.standard_normal(3) * 3.0
    return out


def block_table(rng, M, nblocks):
    """M permutations of the 4 nblocks atoms that carry blocks onto blocks, some reversed; the identity first; not a group"""
    rows = [np.arange(4 * nblocks)]
    for _ in range(M - 1):
        sigma = rng.permutation(nblocks)
        rev = rng.random(nblocks) < 0.5
        rows.append(np.concatenate([4 * sigma[k] + (np.arange(4)[::-1] if rev[k] else np.arange(4)) for k in range(nblocks)]))
    return np.stack(rows).astype(np.int64)


def scatter(rng, x, scattered):
    """x float64 [n,L,3] -> (fp32 [n,A,3] 60 - 100 A from the origin, idx int32 [L] or None)"""
    n, L = x.shape[:2]
    d = rng.standard_normal((n, 1, 3))
    x = x + d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(60, 100, (n, 1, 1))
    if not scattered:
        return x.astype(np.float32), None
    A = L + 13
    idx = rng.permutation(A)[:L].astype(np.int32)
    full = rng.standard_normal((n, A, 3)) * 3 + 70
    full[:, idx] = x
    return full.astype(np.float32), idx


def block_case(na, nb, nblocks, T, M, scattered, seed=0):
    """a kernel case on disjoint four-atom chains: Q = the blocks the table reaches from the T * 2 base quadruples (two per entry; one
    when nblocks == 1), random weights and max_dev"""
    rng = np.random.default_rng(52000 + seed + 977 * na + 131 * nb + 10 * nblocks + 7 * T + M + scattered)
    per = 1 if nblocks == 1 else 2
    blocks = rng.permutation(nblocks)[:T * per] if T * per <= nblocks else rng.integers(0, nblocks, T * per)
    ents = [dict(kind=ref.ROT, atoms=(0, 1), max_dev=float(rng.choice([180.0, ref.ring_max_dev(6), 90.0])),
                 quads=[tuple(int(4 * b + k) for k in range(4)) for b in blocks[per * t:per * t + per]]) for t in range(T)]
    w = rng.uniform(0.1, 1.0, T)
    xa, ia = scatter(rng, block_chains(rng, na, nblocks), scattered)
    xb, ib = scatter(rng, block_chains(rng, nb, nblocks), scattered)
    return dict(xa=xa, xb=xb, idx_a=ia, idx_b=ib, Lg=4 * nblocks, ents=ents, w=w, perms=block_table(rng, M, nblocks))


def _finish(rng, xs, na, quads, Lg, T_max=1024):
    """entries that own ceil(Q / T_max) quadruples each (one per entry would exceed T <= 1024), random weights; M = 1"""
    per = -(-len(quads) // T_max)
    ents = [dict(kind=ref.ROT, atoms=(0, 1), max_dev=180.0, quads=quads[k:k + per]) for k in range(0, len(quads), per)]
    xa, ia = scatter(rng, xs[:na], False)
    xb, ib = scatter(rng, xs[na:], False)
    return dict(xa=xa, xb=xb, idx_a=ia, idx_b=ib, Lg=Lg, ents=ents, w=rng.uniform(0.1, 1.0, len(ents)), perms=np.arange(Lg)[None])


def cone_case(na, nb, Q, units=46, k=10, seed=0):
    """Q of the k * k * units quadruples (a_i, b, c, d_j) of `units` bonds b - c that carry k atoms on either end, each on a cone of 95 ..
    145 degrees about the bond at a random azimuth: many overlapping quadruples on few atoms (units (2 k + 2) <= 1024), every bond
    angle in range in every structure"""
    rng = np.random.default_rng(53000 + seed + 977 * na + 131 * nb + Q)
    Lg = units * (2 * k + 2)
    xs = np.zeros((na + nb, Lg, 3))
    for x in xs:
        for u in range(units):
            o = u * (2 * k + 2)
            b = rng.standard_normal(3) * 4.0
            axis = rng.standard_normal(3)
            axis /= np.linalg.norm(axis)
            c = b + 1.5 * axis
            far = b + rng.standard_normal(3) + 5.0 * np.cross(axis, [0.3, 0.5, 0.8])
            x[o], x[o + 1] = b, c
            for i in range(k):
                x[o + 2 + i] = place(b, c, far, rng.uniform(1.2, 1.6), rng.uniform(95, 145), rng.uniform(-180, 180))
                x[o + 2 + k + i] = place(c, b, far, rng.uniform(1.2, 1.6), rng.uniform(95, 145), rng.uniform(-180, 180))
    every = [(u * (2 * k + 2) + 2 + i, u * (2 * k + 2), u * (2 * k + 2) + 1, u * (2 * k + 2) + 2 + k + j)
             for u in range(units) for i in range(k) for j in range(k)]
    pick = np.sort(rng.permutation(len(every))[:Q])
    return _finish(rng, xs, na, sorted(canonical(every[p]) for p in pick), Lg)


def chain_case(na, nb, Lg, Q, seed=0):
    """Q <= Lg - 3 consecutive quadruples (k, k+1, k+2, k+3) of zig-zag chains of Lg atoms with bond angles of 95 .. 145 degrees and
    dihedrals at least 2 degrees from 0 and 180"""
    rng = np.random.default_rng(54000 + seed + 977 * na + 131 * nb + Lg + Q)
    xs = []
    for _ in range(na + nb):
        rows = [(), (0, 1.5), (1, 0, 1.5, rng.uniform(95, 145))]
        rows += [(k - 1, k - 2, k - 3, 1.5, rng.uniform(95, 145), rng.uniform(2.0, 178.0) * rng.choice([-1.0, 1.0])) for k in range(3, Lg)]
        xs.append(zmatrix(rows))
    starts = np.sort(rng.permutation(Lg - 3)[:Q])
    return _finish(rng, np.array(xs), na, [canonical((k, k + 1, k + 2, k + 3)) for k in starts], Lg)


#: the kernel cases of tests/test_torsion_gpu.py (tests/test_torsion_cpu.py asserts that the reference is well conditioned on each):
#: (builder, keywords, the column tile TJ the kernel picks, whether the row's angles sit in LDS)
KERNEL_CASES = [
    ("block", dict(na=1, nb=1, nblocks=1, T=1, M=1, scattered=False), 64, True),          # Q = 1, T = 1, one structure
    ("block", dict(na=5, nb=63, nblocks=12, T=5, M=3, scattered=True), 64, True),         # TJ = 64: nb = TJ - 1, a random table
    ("block", dict(na=2, nb=65, nblocks=12, T=5, M=1, scattered=False), 64, True),        #          nb = TJ + 1
    ("block", dict(na=2, nb=15, nblocks=20, T=6, M=9, scattered=True), 16, True),         # TJ = 16 by M
    ("block", dict(na=2, nb=17, nblocks=200, T=80, M=3, scattered=False), 16, True),      # TJ = 16 by the LDS budget (Q 126 .. 479)
    ("block", dict(na=2, nb=3, nblocks=16, T=4, M=40, scattered=True), 4, True),          # TJ = 4 by M
    ("chain", dict(na=1, nb=5, Lg=700, Q=600), 4, True),                                  # TJ = 4 by the LDS budget (Q 480 .. 1631)
    ("block", dict(na=5, nb=2, nblocks=10, T=3, M=257, scattered=False), 1, True),        # TJ = 1: M just above one block's threads
    ("block", dict(na=1, nb=1, nblocks=10, T=3, M=300, scattered=True), 1, True),
    ("cone", dict(na=1, nb=2, Q=4079), 1, True),                                          # the largest Q whose row still sits in LDS
    ("cone", dict(na=1, nb=2, Q=4096), 1, False),                                         # Q at the limit: the row stays in global memory
]
_BUILDERS = dict(block=block_case, chain=chain_case, cone=cone_case)
_CACHE = {}


def kernel_case(k):
    """case k of KERNEL_CASES with its tables and its reference (`ref.cross`), built once"""
    if k not in _CACHE:
        kind, kw, tj, in_lds = KERNEL_CASES[k]
        c = _BUILDERS[kind](**kw)
        c["tables"] = tables(c["ents"], c["w"], c["perms"])
        c["ref"] = ref.cross(c["xa"], c["idx_a"], c["xb"], c["idx_b"], c["ents"], c["w"], c["perms"], c["Lg"])
        c["tag"] = f"{kind} " + " ".join(f"{a}={b}" for a, b in kw.items() if a != "scattered") + (" scattered" if kw.get("scattered") else "")
        c["tile"], c["row_in_lds"] = tj, in_lds
        _CACHE[k] = c
    return _CACHE[k]


def expected_tile(Q, M):
    """the column tile of include/physdock_hip.h and whether the row sits in LDS"""
    tj = 64 if M <= 4 else 16 if M <= 16 else 4 if M <= 64 else 1
    while tj > 1 and (tj + 1) * (Q | 1) * 8 > 65280:
        tj //= 4
    return tj, 2 * (Q | 1) * 8 <= 65280
