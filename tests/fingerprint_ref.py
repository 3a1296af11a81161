"""The written definition of `MorganFingerprint` (physdock_amd/fingerprints.py, csrc/fingerprint.hip) in Python integers: circular
fingerprints after Rogers & Hahn 2010 (ECFP) - the package's own definition, NOT RDKit's bytes - and the Tanimoto, top-k and MaxMin
definitions that go with them.  Every kernel result must equal these bit for bit.

All hash arithmetic is mod 2^32 on unsigned values:

    fmix(h):    h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
    push(h, v): fmix(h * 0x01000193 + v + 0x9E3779B9)            (v mod 2^32: a charge of -1 is 0xFFFFFFFF)

Inputs are the rows of `LigandLibrary`: atoms (Z, charge, h_count, flags) and bonds (i, j, o2, -) with o2 twice the order; a bond
that leaves its ligand or joins an atom to itself is skipped, as in the sibling kernels.
    id_0(a)   push chained from 0 over Z, heavy degree, h_count, charge, in-ring (the atom has a bond that is no bridge), aromatic
              (bit 0 of the flags); or `atom_invariants[a]` as given
    id_r(a)   push chained from 0 over r, id_{r-1}(a) and, for the neighbours b of a as pairs (o2(a,b) mod 2^32, id_{r-1}(b)) in
              ascending order, o2 then id
    env_0(a)  the empty set of bonds;  env_r(a) = env_{r-1}(a) | union over neighbours b of (env_{r-1}(b) | {bond a-b})
    kept      every (a, 0); (a, r), r >= 1, exactly when no feature (a', r'), r' >= 1, with the same bond set has a smaller
              (r', id_{r'}(a'), a').  An atom goes on iterating whether or not its feature was kept (RDKit's dead atoms stop).  An
              atom without a bond has the empty set at every radius, so its radius-1 feature is kept and the later ones are not.
    bits      a kept feature sets bit id & (n_bits - 1); bit k is bit k % 32 of word k // 32

Tanimoto: c = popcount(a & b), u = pa + pb - c, the value np.float32(c) / np.float32(u); an EMPTY UNION GIVES 1.0, the convention of
`pd_plif_pairwise` (csrc/plif.hip `plif_ratio`: two rows without a bit are equal).  Orders (top-k, MaxMin) compare the exact fractions
by cross-multiplication, an empty union as 1 / 1."""
import numpy as np

M = 0xFFFFFFFF
N_BITS = (512, 1024, 2048, 4096)
MAX_RADIUS = 4


def fmix(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M
    return h ^ (h >> 16)


def push(h, v):
    return fmix((h * 0x01000193 + (int(v) & M) + 0x9E3779B9) & M)


def chain(values):
    h = 0
    for v in values:
        h = push(h, v)
    return h


def tables(lig):
    """(atoms [L][4], bonds [nb][4]) of a `physdock_amd.ligand.Ligand`, the rows `LigandLibrary` makes of it"""
    atoms = [[int(z), int(q), int(h), int(bool(ar)) | (int(c) << 1)]
             for z, q, h, ar, c in zip(lig.elements, lig.charges, lig.h_count, lig.aromatic, lig.chiral)]
    bonds = [[int(i), int(j), int(round(2.0 * float(o))), 0] for (i, j), o in zip(lig.bonds.tolist(), lig.bond_orders)]
    return atoms, bonds


def _bridges(L, edges):
    """edges: (bond index, i, j) -> the set of bond indices that are bridges (j cannot be reached from i without the bond)"""
    nbr = [[] for _ in range(L)]
    for b, i, j in edges:
        nbr[i].append((j, b)); nbr[j].append((i, b))
    out = set()
    for b, i, j in edges:
        seen, todo = {i}, [i]
        while todo:
            for y, b2 in nbr[todo.pop()]:
                if b2 != b and y not in seen:
                    seen.add(y); todo.append(y)
        if j not in seen:
            out.add(b)
    return out


def morgan(atoms, bonds, radius=2, n_bits=2048, atom_invariants=None):
    """-> dict: `ids` uint32 [L, radius+1], `kept` uint8 [L, radius+1], `env` (list per radius of the bond sets as Python ints),
    `bits` uint32 [n_bits/32], `n_features`, `popcount`"""
    assert 0 <= radius <= MAX_RADIUS and n_bits in N_BITS
    atoms = [[int(v) for v in row] for row in np.asarray(atoms).reshape(-1, 4).tolist()]
    bonds = [[int(v) for v in row] for row in np.asarray(bonds).reshape(-1, 4).tolist()]
    L = len(atoms)
    edges = [(b, i, j) for b, (i, j, _, _) in enumerate(bonds) if 0 <= i < L and 0 <= j < L and i != j]
    nbr = [[] for _ in range(L)]                                   # (neighbour, bond index, o2 mod 2^32)
    for b, i, j in edges:
        nbr[i].append((j, b, bonds[b][2] & M)); nbr[j].append((i, b, bonds[b][2] & M))
    bridge = _bridges(L, edges)
    if atom_invariants is None:
        ident = [chain((atoms[a][0], len(nbr[a]), atoms[a][2], atoms[a][1], int(any(b not in bridge for _, b, _ in nbr[a])),
                        atoms[a][3] & 1)) for a in range(L)]
    else:
        assert len(atom_invariants) == L
        ident = [int(v) & M for v in atom_invariants]
    ids, envs = [ident], [[0] * L]
    for r in range(1, radius + 1):
        prev, penv = ids[-1], envs[-1]
        cur, cenv = [], []
        for a in range(L):
            values = [r, prev[a]]
            for o2, i in sorted((o2, prev[b]) for b, _, o2 in nbr[a]):
                values += [o2, i]
            cur.append(chain(values))
            e = penv[a]
            for b, k, _ in nbr[a]:
                e |= penv[b] | (1 << k)
            cenv.append(e)
        ids.append(cur); envs.append(cenv)
    kept = [[1] * L]
    first = {}
    for key in sorted((r, ids[r][a], a) for r in range(1, radius + 1) for a in range(L)):
        first.setdefault(envs[key[0]][key[2]], key)
    for r in range(1, radius + 1):
        kept.append([int(first[envs[r][a]] == (r, ids[r][a], a)) for a in range(L)])
    bits = np.zeros(n_bits // 32, dtype=np.uint32)
    for r in range(radius + 1):
        for a in range(L):
            if kept[r][a]:
                k = ids[r][a] & (n_bits - 1)
                bits[k >> 5] |= np.uint32(1 << (k & 31))
    return {"ids": np.asarray(ids, dtype=np.uint32).T.copy(), "kept": np.asarray(kept, dtype=np.uint8).T.copy(), "env": envs,
            "bits": bits, "n_features": int(np.sum(kept)), "popcount": popcount_rows(bits[None])[0]}


def fingerprint(lig, radius=2, n_bits=2048, atom_invariants=None):
    return morgan(*tables(lig), radius, n_bits, atom_invariants)


def renumbered(lig, rng):
    """the same molecule with its atoms and its bond list in a random order (and random bond directions), as tables"""
    atoms, bonds = tables(lig)
    L = len(atoms)
    perm = rng.permutation(L)                                       # old atom a becomes perm[a]
    new_atoms = [None] * L
    for a in range(L):
        new_atoms[perm[a]] = atoms[a]
    new_bonds = []
    for b in rng.permutation(len(bonds)):
        i, j, o2, f = bonds[b]
        i, j = int(perm[i]), int(perm[j])
        new_bonds.append([j, i, o2, f] if rng.integers(2) else [i, j, o2, f])
    return new_atoms, new_bonds, perm


def fold(bits, n_bits):
    """the OR-fold of rows of words to n_bits"""
    bits = np.asarray(bits, dtype=np.uint32)
    w = n_bits // 32
    out = np.zeros(bits.shape[:-1] + (w,), dtype=np.uint32)
    for k in range(0, bits.shape[-1], w):
        out |= bits[..., k:k + w]
    return out


def popcount_rows(bits):
    bits = np.ascontiguousarray(np.asarray(bits, dtype=np.uint32))
    return [int(np.unpackbits(row.view(np.uint8)).sum()) for row in bits.reshape(-1, bits.shape[-1])]


def counts(a, b):
    """(common [n,m], union [n,m]) as int64"""
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    pa, pb = np.asarray(popcount_rows(a)), np.asarray(popcount_rows(b))
    common = np.zeros((len(a), len(b)), dtype=np.int64)
    for i in range(len(a)):
        both = np.ascontiguousarray(a[i][None, :] & b)
        common[i] = np.unpackbits(both.view(np.uint8), axis=1).sum(axis=1)
    return common, pa[:, None] + pb[None, :] - common


def quotient(c, u):
    """the fp32 value of the similarity c / u; 1.0 for an empty union"""
    c, u = np.asarray(c), np.asarray(u)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = c.astype(np.float32) / u.astype(np.float32)
    return np.where(u == 0, np.float32(1.0), q).astype(np.float32)


def tanimoto(a, b):
    c, u = counts(a, b)
    return quotient(c, u), c.astype(np.int32)


def _frac(c, u):
    return (1, 1) if u == 0 else (int(c), int(u))


def _cmp(x, y):
    """the sign of x - y for x, y = (c, u), compared as exact fractions by cross-multiplication"""
    (c1, u1), (c2, u2) = _frac(*x), _frac(*y)
    d = c1 * u2 - c2 * u1
    return (d > 0) - (d < 0)


def nearest(a, b, k, exclude_self=False):
    """the k most similar rows of b for each row of a: the larger exact fraction first, the smaller column on a tie
    -> index int32 [n,k], similarity fp32 [n,k], common int32 [n,k]"""
    import functools
    c, u = counts(a, b)
    order = functools.cmp_to_key(lambda x, y: -_cmp(x[:2], y[:2]) or x[2] - y[2])
    index = np.zeros((len(c), k), dtype=np.int32)
    com = np.zeros((len(c), k), dtype=np.int32)
    for i in range(len(c)):
        cand = sorted(((int(c[i, j]), int(u[i, j]), j) for j in range(c.shape[1]) if not (exclude_self and j == i)), key=order)[:k]
        index[i] = [t[2] for t in cand]
        com[i] = [t[0] for t in cand]
    un = np.take_along_axis(u, index.astype(np.int64), axis=1)
    return index, quotient(com, un), com


def maxmin(bits, n_pick, first=0):
    """MaxMin (Ashton et al. 2002): picks[0] = first; then the unpicked row with the largest min over the picked of (1 - T), that is
    the smallest largest similarity to the picked, as exact fractions, the smallest index on a tie.
    -> picks int32 [n_pick], max_similarity fp32 [n_pick] (NaN for the first)"""
    c, u = counts(bits, bits)
    n = len(c)
    picks, sims = [int(first)], [np.float32(np.nan)]
    run = [None] * n                                                # the largest similarity to the picked so far, (c, u)
    while len(picks) < n_pick:
        p = picks[-1]
        for i in range(n):
            new = (int(c[i, p]), int(u[i, p]))
            if run[i] is None or _cmp(new, run[i]) > 0:
                run[i] = new
        best = None
        for i in range(n):
            if i not in picks and (best is None or _cmp(run[i], run[best]) < 0):
                best = i
        picks.append(best)
        sims.append(quotient(*run[best]))
    return np.asarray(picks, dtype=np.int32), np.asarray(sims, dtype=np.float32)


def colliding_fractions(limit=4096):
    """two distinct fractions c1 / u1 > c2 / u2 in [0, 1] with denominators up to `limit` whose fp32 quotients are equal, or None.
    Two distinct fractions differ by at least 1 / (limit (limit - 1)); for limit = 4096 that is 5.9619e-8 > 2^-24 = 5.9605e-8, the
    largest spacing of fp32 below 1, and two reals further apart than one spacing never round to one value: None exists up to 4096
    bits.  (At 8192 they do: 8190 / 8191 and 8191 / 8192.)  The search looks where the spacing is largest, next to 1."""
    for u1 in range(limit, max(limit - 48, 1), -1):
        for u2 in range(u1 - 1, max(limit - 49, 0), -1):
            for c1 in range(u1 - 1, max(u1 - 6, 0), -1):
                for c2 in range(u2 - 1, max(u2 - 6, 0), -1):
                    if c1 * u2 != c2 * u1 and np.float32(c1) / np.float32(u1) == np.float32(c2) / np.float32(u2):
                        return ((c1, u1), (c2, u2)) if c1 * u2 > c2 * u1 else ((c2, u2), (c1, u1))
    return None
