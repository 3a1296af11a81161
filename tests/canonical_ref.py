"""The written definition of `CanonicalForm` (physdock_amd/canonical.py, csrc/canonical.hip) in Python integers: a canonical numbering of
the heavy atoms of one ligand, an exact certificate of the annotated graph and a 64-bit key of it - the package's own definition, NOT
RDKit's canonical SMILES and NOT InChI.  Every kernel result must equal these word for word.

One ligand of n <= 128 atoms and m <= 512 bonds, as the rows of `LigandLibrary` (atoms (Z, charge, h_count, flags), bonds (i, j, o2, -)
with o2 twice the order) plus `isotopes`, `chiral_order` (per atom up to four entries, -1 a hydrogen, padded with -2; an order of fewer
than 3 or more than 4 entries is an empty row) and the `bond_stereo` rows (a, b, c, d, kind, a2, d2).  `push` and `fmix` are the hash
functions of tests/fingerprint_ref.py, mod 2^32.

    inv(a)        (Z, charge, h_count, isotope, written-aromatic flag); tuples compare lexicographically
    colouring     every atom gets the number of atoms with a strictly smaller key: a cell's colour is the position at which the cell
                  starts, and a discrete colouring is a permutation - the colour is the label
    root          the colouring by inv
    round         t(a) = the sum mod 2^32 over the bonds (a, b) of push(push(0, o2), col[b]); colour again by (col[a], t(a)).  The sum
                  commutes: no neighbour order enters, any degree is handled.  A hash collision only makes the result coarser
    refine        rounds until the number of distinct colours stops growing (none when the colouring is discrete already)
    individualise(col, v)  colour again by (col[a], 0 if a == v else 1), then refine

The search is depth-first from refine(root).  At a node that is not discrete the target cell is the cell of the smallest colour with
more than one atom, and its members are tried in ascending atom index: the child is individualise(col, v).  A member of heavy degree 1
is skipped when an earlier member of the cell has heavy degree 1, the same neighbour and the same o2 to it (terminal twins: the F of a
CF3, the methyls of a t-butyl, the O of a sulfonyl).  Every call of refine is one step, the root's included; a step that is due when
`max_steps` are spent stops the search with status 2 and the best leaf so far, which is not canonical (`canonical` = 0).  Without any
leaf the labels are the input order.

The certificate of a leaf, lab the leaf's colours, as uint32 words:
    n, m
    for label k = 0 .. n-1, the atom a with lab[a] == k:   Z | (charge + 128) << 8 | h_count << 16 | aromatic << 24,   isotope | parity << 16
    the bonds as lo << 16 | hi << 8 | o2, lo < hi in labels, ascending
    s, the number of bond_stereo rows
    the rows as b << 23 | c << 16 | a << 9 | d << 2 | kind in labels, ascending: b < c, a and d the lowest-LABEL substituents of b and
    c, kind flipped once for every end whose lowest-label substituent is not the one the input row names
parity(a) is 0 for an unmarked atom and for a mark that cannot mean anything - h_count >= 2, a chiral_order row that is empty, two
terminal heavy neighbours with equal inv and equal o2 - and else the written code (1 `@`, 2 `@@`), exchanged when the chiral_order row
mapped to labels (a hydrogen stays -1) has an odd number of inversions.  Certificates compare word by word; the smallest leaf wins,
the first one found on a tie.  key = (k0, k1): push chained over the words from the seeds 0 and 1.

Why it is exact.  (1) The tree of colourings is built from inv, o2 and the colours alone, never from an atom index except as the order
in which members are tried; so two numberings of one annotated molecule have trees that are images of each other, the same multiset of
leaf certificates and the same minimum.  (2) A certificate spells the annotated graph out - every atom's invariant and parity, every
bond, every stereo row - so equal certificates mean the same molecule; the key is a convenience and `first_of` compares certificates.
(3) A pruned subtree is the image of a kept one under the exchange of two terminal twins, which is an automorphism of the graph that
fixes every annotation: the twins have equal inv (one cell), a terminal atom has parity 0 (at most two entries in its order or two
hydrogens), their common neighbour has parity 0 by the third rule above, and `stereo_bonds_from_bonds` lists no double bond with two
substituents of one symmetry class on an end, so no stereo row tells the twins apart.  Images carry equal certificates, and the kept
subtree comes first, so neither the minimum nor the leaf that wins a tie changes.  (4) A hash collision in t(a) merges cells that a
collision-free round would split; the search then individualises where refinement would have decided, which costs steps and never
exactness, because the leaf certificate decides."""
import numpy as np

from fingerprint_ref import M, push, tables as atom_bond_tables

MAX_STEPS = 65536
MAX_STEREO = 64


def tables(lig):
    """the rows one ligand has in the launch: atoms, bonds (fingerprint_ref.tables), isotopes [n], chiral_order [n][4], stereo [s][7]"""
    atoms, bonds = atom_bond_tables(lig)
    n = len(atoms)
    order = [[-2] * 4 for _ in range(n)]
    for a, row in lig.chiral_order.items():
        if 3 <= len(row) <= 4:
            order[a][:len(row)] = [int(v) for v in row]
    return {"atoms": atoms, "bonds": bonds, "isotopes": [int(v) for v in lig.isotopes], "chiral_order": order,
            "stereo": [[int(v) for v in r] for r in lig.bond_stereo.tolist()]}


def colour(keys):
    first = {}
    for k, key in enumerate(sorted(keys)):
        first.setdefault(key, k)
    return [first[key] for key in keys]


class _Graph:
    def __init__(self, t):
        self.t = t
        self.atoms, self.bonds = t["atoms"], t["bonds"]
        self.n, self.m = len(self.atoms), len(self.bonds)
        self.inv = [(a[0], a[1], a[2], iso, a[3] & 1) for a, iso in zip(self.atoms, t["isotopes"])]
        self.nbr = [[] for _ in range(self.n)]                       # (neighbour, o2, push(0, o2))
        for i, j, o2, _ in self.bonds:
            h = push(0, o2)
            self.nbr[i].append((j, o2, h)); self.nbr[j].append((i, o2, h))
        self.deg = [len(v) for v in self.nbr]
        self.meaningful = [self._meaningful(a) for a in range(self.n)]

    def _meaningful(self, a):
        code = (self.atoms[a][3] >> 1) & 3
        row = [v for v in self.t["chiral_order"][a] if v != -2]
        if code not in (1, 2) or self.atoms[a][2] >= 2 or not 3 <= len(row) <= 4:
            return False
        terminal = [(self.inv[b], o2) for b, o2, _ in self.nbr[a] if self.deg[b] == 1]
        return len(set(terminal)) == len(terminal)

    def round(self, col):
        return colour([(col[a], sum(push(h, col[b]) for b, _, h in self.nbr[a]) & M) for a in range(self.n)])

    def refine(self, col):
        k = len(set(col))
        while k < self.n:
            new = self.round(col)
            k2 = len(set(new))
            if k2 == k:
                break
            col, k = new, k2
        return col

    def parity(self, a, lab):
        if not self.meaningful[a]:
            return 0
        code = (self.atoms[a][3] >> 1) & 3
        row = [(-1 if v == -1 else lab[v]) for v in self.t["chiral_order"][a] if v != -2]
        inversions = sum(1 for i in range(len(row)) for j in range(i + 1, len(row)) if row[i] > row[j])
        return 3 - code if inversions & 1 else code

    def certificate(self, lab):
        order = [0] * self.n
        for a, k in enumerate(lab):
            order[k] = a
        words = [self.n, self.m]
        for a in order:
            z, q, h, f = self.atoms[a]
            words += [z | (q + 128) << 8 | h << 16 | (f & 1) << 24, self.t["isotopes"][a] | self.parity(a, lab) << 16]
        words += sorted(min(lab[i], lab[j]) << 16 | max(lab[i], lab[j]) << 8 | o2 for i, j, o2, _ in self.bonds)
        rows = []
        for a, b, c, d, kind, a2, d2 in self.t["stereo"]:
            if a2 >= 0 and lab[a2] < lab[a]:
                a, kind = a2, 3 - kind
            if d2 >= 0 and lab[d2] < lab[d]:
                d, kind = d2, 3 - kind
            if lab[b] > lab[c]:
                a, b, c, d = d, c, b, a
            rows.append(lab[b] << 23 | lab[c] << 16 | lab[a] << 9 | lab[d] << 2 | kind)
        return [w & M for w in words + [len(rows)] + sorted(rows)]


class _Spent(Exception):
    pass


def canonical_tables(t, max_steps=MAX_STEPS, twins=True):
    """-> dict: labels, order, classes (lists [n]), cert (list of words), key (k0, k1), status, steps, leaves, canonical"""
    g = _Graph(t)
    n = g.n
    st = {"steps": 0, "leaves": 0, "best": None, "lab": None}

    def step(col):
        if st["steps"] >= max_steps:
            raise _Spent()
        st["steps"] += 1
        return g.refine(col)

    def node(col):
        sizes = {}
        for c in col:
            sizes[c] = sizes.get(c, 0) + 1
        if len(sizes) == n:
            cert = g.certificate(col)
            st["leaves"] += 1
            if st["best"] is None or cert < st["best"]:
                st["best"], st["lab"] = cert, list(col)
            return
        cell = min(c for c, k in sizes.items() if k > 1)
        members = [v for v in range(n) if col[v] == cell]
        for v in members:
            if twins and g.deg[v] == 1 and any(u < v and g.deg[u] == 1 and g.nbr[u][0][:2] == g.nbr[v][0][:2] for u in members):
                continue
            node(step(colour([(col[a], 0 if a == v else 1) for a in range(n)])))

    assert max_steps >= 1                                           # the root's step is always taken: `classes` is always refined
    status, classes = 0, step(colour(g.inv))
    try:
        node(classes)
    except _Spent:
        status = 2
    lab = st["lab"] if st["lab"] is not None else list(range(n))
    cert = st["best"] if st["best"] is not None else g.certificate(lab)
    order = [0] * n
    for a, k in enumerate(lab):
        order[k] = a
    k0, k1 = 0, 1
    for w in cert:
        k0, k1 = push(k0, w), push(k1, w)
    return {"labels": lab, "order": order, "classes": classes, "cert": cert, "key": (k0, k1), "status": status, "steps": st["steps"],
            "leaves": st["leaves"], "canonical": int(status == 0)}


def canonical(lig, max_steps=MAX_STEPS, twins=True):
    return canonical_tables(tables(lig), max_steps, twins)


def first_of(results):
    """per ligand the smallest earlier index with status 0 and the same certificate, else its own; a status other than 0 matches
    nothing"""
    out = []
    for g, r in enumerate(results):
        out.append(next((j for j in range(g) if r["status"] == 0 and results[j]["status"] == 0 and results[j]["cert"] == r["cert"]), g))
    return out


def renumbered(lig, rng):
    """the same molecule as a new `Ligand` with its atoms and its bond rows in a random order (and random bond directions);
    `chiral_order` and `bond_stereo` are carried along"""
    from physdock_amd.ligand import Ligand
    n = lig.n_atoms
    perm = [int(v) for v in rng.permutation(n)]                      # old atom a becomes perm[a]
    inverse = np.argsort(perm)
    bonds, orders = [], []
    for b in rng.permutation(lig.n_bonds):
        i, j = (perm[int(v)] for v in lig.bonds[b])
        bonds.append((j, i) if rng.integers(2) else (i, j))
        orders.append(float(lig.bond_orders[b]))
    take = lambda v: np.asarray(v)[inverse]
    order = {perm[a]: [(-1 if v < 0 else perm[v]) for v in row] for a, row in lig.chiral_order.items()}
    stereo = [(perm[a], perm[b], perm[c], perm[d], kind) for a, b, c, d, kind, _, _ in lig.bond_stereo.tolist()]
    return Ligand(take(lig.elements), np.asarray(bonds, dtype=np.int64).reshape(-1, 2), orders, take(lig.charges), take(lig.h_count),
                  take(lig.aromatic), take(lig.chiral), order, take(lig.isotopes), source=lig.source, bond_stereo=stereo)
