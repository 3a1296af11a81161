"""Where does a ligand come from?  A SMILES reader on the host, without a dependency (`parse_smiles`).  The reference's screening
driver reads one SMILES per line and hands it to RDKit (`get_features_from_smi`, PhysDock/data/tools/rdkit.py); RDKit is not a dependency
of this package, so this is **the package's own reader, not RDKit's**: it reads what is written and perceives nothing.

Grammar: the organic subset `B C N O P S F Cl Br I` and the aromatic `b c n o p s`; bracket atoms `[isotope symbol @|@@ Hn charge :class]`
with any element symbol of `pdbio.ELEMENTS` (and the aromatic `se`, `as`), the charge as `+`, `-`, `++`, `--`, `+2`, `-2` ..., the class
read and dropped; the bonds `- = # :` and the directional `/` and `\\`, which are single bonds whose direction is kept (below);
branches; ring closures `0`-`9` and `%nn` with an optional bond symbol on either end (two different symbols raise).

The result has the shape of a `sdfio.parse_sdf` record, over the heavy atoms in their order of appearance: `elements` (atomic numbers),
`bonds` int64 [n,2], `bond_orders` float64 (1, 2, 3, or 1.5 for `:` and for two aromatic atoms joined without a symbol), `charges`,
`aromatic` (as written), `h_count`, `isotopes`, `chiral` (0 none, 1 `@`, 2 `@@`) and `chiral_order`: for every atom written with `@` or
`@@` its neighbours in OpenSMILES order - the preceding atom, an implicit hydrogen as -1, the ring-closure partners in the order their
digits stand on the atom, then the branches and the chain.

Double-bond stereo.  Between an atom u in front and an atom v behind (a branch atom included) `/` says "v is up from u, u is down
from v" and `\\` the opposite; a symbol in front of a ring-closure digit is read from the atom in front of it to the ring partner, so
the two ends of one ring closure agree when they carry opposite characters (equal ones raise).  A double bond b=c with a marked
substituent a of b and a marked substituent d of c is cis when a seen from b and d seen from c are both up or both down, else trans:
`F/C=C/F` is trans, `F/C=C\\F` cis, `C(\\F)=C/F` is `F/C=C/F`.  The key `bond_stereo` holds int32 [n,7] rows (a, b, c, d, kind, a2, d2)
over the heavy atoms, sorted by (b, c) with b < c: a and d are the LOWEST heavy substituents of b and c, a2 and d2 the other one or -1,
kind is 1 cis / 2 trans of a against d (flipped once for every end whose lowest substituent is not the marked one).  A mark on a bond
to a folded `[H]` is passed on, inverted, to that atom's other substituent.  Two marks on one end that say the same raise.  Marks
on one end only, marks next to no double bond and marks on a bond that `ligand.stereo_bonds_from_bonds` does not list (a ring of at
most 7 atoms, two substituents no walk of the graph tells apart) give no row.  cis / trans, not CIP E / Z.

Hydrogens.  An explicit `[H]` bonded to one heavy atom is folded into that atom's `h_count` (the reference's `RemoveAllHs`) and stands
as -1 in a `chiral_order`; hydrogens bonded to each other raise.  A bracket atom has exactly the hydrogens written.  An atom of the
organic subset gets the smallest normal valence (B 3, C 4, N 3 / 5, O 2, P 3 / 5, S 2 / 4 / 6, halogens 1) that is not below its
bond-order sum, in which an aromatic atom's aromatic bonds count as (their number + 1) - except that an aromatic atom whose bonds,
counted one each, already fill a normal valence gets none (the N of `Cn1cccc1`, the S of `c1ccsc1`: the "+ 1" is the atom's own
pi electron pair there, not a missing hydrogen).

**Caveats.**  Nothing is perceived: Kekule input stays Kekule and aromatic input is not kekulised.  The one repair: an unmarked bond
between two aromatic atoms that closes no ring (the middle bond of `c1ccccc1c1ccccc1`) is single, as every SMILES reader has it.
Refused with a `ValueError` that names the character position (0-based): `.`, `*`, an unknown symbol, an unclosed ring or branch, a ring
bond of an atom to itself, a second bond between two atoms, an empty string, more than `MAX_ATOMS` heavy atoms."""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from .pdbio import ELEMENTS

__all__ = ["parse_smiles", "implicit_hydrogens", "MAX_ATOMS", "NORMAL_VALENCES"]

#: heavy atoms of one ligand (the limit of csrc/ligand_features.hip and csrc/conformers.hip)
MAX_ATOMS = 128
#: the normal valences of the organic subset, by atomic number
NORMAL_VALENCES = {5: (3,), 6: (4,), 7: (3, 5), 8: (2,), 15: (3, 5), 16: (2, 4, 6), 9: (1,), 17: (1,), 35: (1,), 53: (1,)}
_Z = {s: k + 1 for k, s in enumerate(ELEMENTS)}
_ORGANIC = ("Cl", "Br", "B", "C", "N", "O", "P", "S", "F", "I")
_AROMATIC = {"b": 5, "c": 6, "n": 7, "o": 8, "p": 15, "s": 16}
_AROMATIC_BRACKET = dict(_AROMATIC, se=34, **{"as": 33})
_BOND = {"-": 1.0, "=": 2.0, "#": 3.0, ":": 1.5, "/": 1.0, "\\": 1.0}
#: the atom behind a directional bond seen from the atom in front of it: +1 up, -1 down
_DIRECTION = {"/": 1, "\\": -1}


def implicit_hydrogens(z: int, order_sum: float, aromatic_bonds: int = 0, n_bonds: int = 0) -> int:
    """The valence rule of the module docstring for one atom of the organic subset: `order_sum` over its non-aromatic bonds,
    `aromatic_bonds` their number beside, `n_bonds` all its bonds.  Elements outside `NORMAL_VALENCES` get 0."""
    valences = NORMAL_VALENCES.get(int(z))
    if valences is None:
        return 0
    if aromatic_bonds and n_bonds in valences:
        return 0
    total = order_sum + (aromatic_bonds + 1 if aromatic_bonds else 0)
    for v in valences:
        if v >= total:
            return int(v - total)                       # (a sum with a half in it cannot occur: aromatic bonds are counted whole)
    return 0


def parse_smiles(text: str) -> Dict[str, object]:
    """One molecule -> the record of the module docstring.  Leading and trailing white space is dropped."""
    if not isinstance(text, str):
        raise ValueError(f"parse_smiles: a str expected, got {type(text).__name__}")
    lead = len(text) - len(text.lstrip())
    s = text.strip()

    def fail(k, why):
        raise ValueError(f"parse_smiles: position {k + lead}: {why}")

    if not s:
        raise ValueError("parse_smiles: position 0: an empty string")
    # every atom written (explicit hydrogens too): [z, charge, aromatic, h written or None, isotope, chiral, position]
    atoms: List[list] = []
    nbrs: List[list] = []                                # per atom, in OpenSMILES order: atom ids, -1, or ("ring", key) until closed
    bonds: List[list] = []                               # [i, j, order or None (unmarked), position]
    marks: List[tuple] = []                              # per bond: (j seen from i: +1 up, -1 down, 0 unmarked; position of the symbol)
    rings: Dict[int, tuple] = {}                         # open digits: number -> (atom, symbol or None, position, slot in nbrs)
    stack: List[tuple] = []
    prev, pending, pending_at = -1, None, -1
    k, n = 0, len(s)

    def add_atom(z, charge, aromatic, h, isotope, chiral, at):
        nonlocal prev, pending
        atoms.append([z, charge, aromatic, h, isotope, chiral, at])
        nbrs.append([])
        a = len(atoms) - 1
        if prev >= 0:
            bonds.append([prev, a, pending, at])
            marks.append((_DIRECTION.get(pending, 0), pending_at))
            nbrs[prev].append(a)
            nbrs[a].append(prev)
        elif pending is not None:
            fail(pending_at, "a bond symbol with no atom in front of it")
        if chiral and h:
            nbrs[a].append(-1)
        prev, pending = a, None

    while k < n:
        ch = s[k]
        if ch == "[":
            end = s.find("]", k)
            if end < 0:
                fail(k, "a bracket atom that is not closed")
            q = k + 1
            d = q
            while d < end and s[d].isdigit():
                d += 1
            isotope = int(s[q:d]) if d > q else 0
            q = d
            if s[q] == "*":
                fail(q, "the wildcard atom * is not read")
            aromatic = False
            if s[q:q + 2] in _AROMATIC_BRACKET:
                z, aromatic, q = _AROMATIC_BRACKET[s[q:q + 2]], True, q + 2
            elif s[q] in _AROMATIC_BRACKET:
                z, aromatic, q = _AROMATIC_BRACKET[s[q]], True, q + 1
            elif s[q:q + 2] in _Z and s[q + 1:q + 2].islower():
                z, q = _Z[s[q:q + 2]], q + 2
            elif s[q] in _Z:
                z, q = _Z[s[q]], q + 1
            else:
                fail(q, f"an unknown element symbol in {s[k:end + 1]!r}")
            chiral = 0
            if s[q] == "@":
                chiral, q = (2, q + 2) if s[q + 1] == "@" else (1, q + 1)
            h = 0
            if s[q] == "H":
                q += 1
                d = q
                while d < end and s[d].isdigit():
                    d += 1
                h, q = (int(s[q:d]) if d > q else 1), d
            charge = 0
            if s[q] in "+-":
                sign = 1 if s[q] == "+" else -1
                d = q + 1
                while d < end and s[d].isdigit():
                    d += 1
                if d > q + 1:
                    charge, q = sign * int(s[q + 1:d]), d
                else:
                    d = q
                    while d < end and s[d] == s[q]:
                        d += 1
                    charge, q = sign * (d - q), d
            if s[q] == ":":
                d = q + 1
                while d < end and s[d].isdigit():
                    d += 1
                if d == q + 1:
                    fail(q, "an atom class without a number")
                q = d
            if q != end:
                fail(q, f"{s[q]!r} is not read inside a bracket atom")
            add_atom(z, charge, aromatic, h, isotope, chiral, k)
            k = end + 1
        elif ch in _BOND:
            if pending is not None:
                fail(k, "two bond symbols in a row")
            if prev < 0:
                fail(k, "a bond symbol with no atom in front of it")
            pending, pending_at = ch, k
            k += 1
        elif ch == "(":
            if prev < 0:
                fail(k, "a branch with no atom in front of it")
            if pending is not None:
                fail(k, "a bond symbol in front of a branch")
            stack.append((prev, k))
            k += 1
        elif ch == ")":
            if not stack:
                fail(k, "a branch closes that was never opened")
            if pending is not None:
                fail(pending_at, "a bond symbol with no atom behind it")
            prev = stack.pop()[0]
            k += 1
        elif ch.isdigit() or ch == "%":
            at = k
            if ch == "%":
                if not (s[k + 1:k + 3].isdigit() and len(s[k + 1:k + 3]) == 2):
                    fail(k, "% needs two digits")
                num, k = int(s[k + 1:k + 3]), k + 3
            else:
                num, k = int(ch), k + 1
            if prev < 0:
                fail(at, "a ring-closure digit with no atom in front of it")
            if num in rings:
                a, sym, opened, slot = rings.pop(num)
                if a == prev:
                    fail(at, f"ring closure {num} bonds an atom to itself")
                if sym is not None and pending is not None and _BOND[sym] != _BOND[pending]:
                    fail(at, f"ring closure {num} is written with {sym!r} on one end and {pending!r} on the other")
                # the opening end reads a -> prev, the closing end prev -> a: the same direction in opposite characters
                way, back = _DIRECTION.get(sym, 0), -_DIRECTION.get(pending, 0)
                if way and back and way != back:
                    fail(at, f"ring closure {num} is written with {sym!r} on both ends: the two ends of one ring bond say the same "
                             "with opposite characters")
                marks.append((way, opened - 1) if way else (back, pending_at))
                sym = pending if sym is None else sym
                bonds.append([a, prev, sym, at])
                nbrs[a][slot] = prev
                nbrs[prev].append(a)
            else:
                rings[num] = (prev, pending, at, len(nbrs[prev]))
                nbrs[prev].append(("ring", num))
            pending = None
        elif ch == ".":
            fail(k, "a dot: more than one molecule")
        elif ch == "*":
            fail(k, "the wildcard atom * is not read")
        else:
            sym = next((o for o in _ORGANIC if s.startswith(o, k)), None)
            if sym is not None:
                add_atom(_Z[sym], 0, False, None, 0, 0, k)
                k += len(sym)
            elif ch in _AROMATIC:
                add_atom(_AROMATIC[ch], 0, True, None, 0, 0, k)
                k += 1
            else:
                fail(k, f"the symbol {ch!r} is not read")
    if pending is not None:
        fail(pending_at, "a bond symbol with no atom behind it")
    if stack:
        fail(stack[-1][1], "a branch that is not closed")
    if rings:
        num = min(rings, key=lambda r: rings[r][2])
        fail(rings[num][2], f"ring closure {num} is not closed")

    seen = {}
    for i, j, _, at in bonds:
        if (min(i, j), max(i, j)) in seen:
            fail(at, f"a second bond between the atoms written at {atoms[i][6] + lead} and {atoms[j][6] + lead}")
        seen[(min(i, j), max(i, j))] = at
    # bond orders: a written symbol, else 1.5 between two aromatic atoms, else 1; an unmarked aromatic bond outside every ring is single
    orders = []
    for i, j, sym, _ in bonds:
        orders.append(_BOND[sym] if sym is not None else (1.5 if atoms[i][2] and atoms[j][2] else 1.0))
    adj = [set() for _ in atoms]
    for i, j, _, _ in bonds:
        adj[i].add(j); adj[j].add(i)
    for b, (i, j, sym, _) in enumerate(bonds):
        if sym is None and orders[b] == 1.5:
            reach, todo = {i}, [i]
            while todo:
                a = todo.pop()
                for c in adj[a]:
                    if c not in reach and not (a == i and c == j):
                        reach.add(c); todo.append(c)
            if j not in reach:
                orders[b] = 1.0
    # explicit hydrogens on a heavy atom are folded
    n_all = len(atoms)
    folded = [False] * n_all
    extra = [0] * n_all
    for a in range(n_all):
        if atoms[a][0] == 1 and len(adj[a]) == 1:
            (host,) = adj[a]
            if atoms[host][0] == 1:
                fail(atoms[a][6], "hydrogens bonded to each other: no heavy atom to carry them")
            folded[a] = True
            extra[host] += 1
    new_id = np.cumsum([not f for f in folded]) - 1
    keep = [a for a in range(n_all) if not folded[a]]
    if len(keep) > MAX_ATOMS:
        fail(atoms[keep[MAX_ATOMS]][6], f"{len(keep)} heavy atoms; up to {MAX_ATOMS} are read")
    h_count = []
    for a in keep:
        z, _, _, h, _, _, _ = atoms[a]
        if h is None:
            own = [orders[b] for b, (i, j, _, _) in enumerate(bonds) if a in (i, j)]
            n_arom = sum(1 for o in own if o == 1.5)
            h = implicit_hydrogens(z, sum(o for o in own if o != 1.5), n_arom, len(own))
        h_count.append(h + extra[a])
    kept_bonds = [(b, i, j) for b, (i, j, _, _) in enumerate(bonds) if not folded[i] and not folded[j]]
    chiral_order = {}
    for a in keep:
        if atoms[a][5]:
            chiral_order[int(new_id[a])] = [-1 if (c == -1 or folded[c]) else int(new_id[c]) for c in nbrs[a]]
    record = {
        "elements": np.asarray([atoms[a][0] for a in keep], dtype=np.int64),
        "bonds": np.asarray([(new_id[i], new_id[j]) for _, i, j in kept_bonds], dtype=np.int64).reshape(-1, 2),
        "bond_orders": np.asarray([orders[b] for b, _, _ in kept_bonds], dtype=np.float64),
        "charges": np.asarray([atoms[a][1] for a in keep], dtype=np.int64),
        "aromatic": np.asarray([atoms[a][2] for a in keep], dtype=bool),
        "h_count": np.asarray(h_count, dtype=np.int64),
        "isotopes": np.asarray([atoms[a][4] for a in keep], dtype=np.int64),
        "chiral": np.asarray([atoms[a][5] for a in keep], dtype=np.int64),
        "chiral_order": chiral_order,
    }
    # double-bond stereo: what every end of a double bond says of its substituents, then the rows of the stereogenic bonds
    seen_from = {}                                       # (u, v) -> (v seen from u, position)
    for (i, j, _, _), (way, at) in zip(bonds, marks):
        if way:
            seen_from[i, j], seen_from[j, i] = (way, at), (-way, at)
    marked = []                                          # (a, b, c, d, kind) over the heavy atoms, a and d the marked substituents
    for b, (i, j, _, _) in enumerate(bonds):
        if orders[b] != 2.0 or folded[i] or folded[j]:
            continue
        ends = []
        for u, v in ((i, j), (j, i)):
            heavy = sorted(w for w in adj[u] if w != v and not folded[w])
            said = {w: seen_from[u, w] for w in heavy if (u, w) in seen_from}
            for h in sorted(w for w in adj[u] if w != v and folded[w] and (u, w) in seen_from):
                way, at = seen_from[u, h]
                if len(heavy) == 1:                      # the hydrogen's mark, inverted, on the one other substituent
                    if heavy[0] in said and said[heavy[0]][0] != -way:
                        fail(max(at, said[heavy[0]][1]), f"the two marks at the atom written at {atoms[u][6] + lead} contradict each other")
                    said.setdefault(heavy[0], (-way, at))
            if len(heavy) == 2 and len(said) == 2 and said[heavy[0]][0] == said[heavy[1]][0]:
                fail(max(said[heavy[0]][1], said[heavy[1]][1]),
                     f"the two marks at the atom written at {atoms[u][6] + lead} contradict each other: both substituents "
                     f"{'up' if said[heavy[0]][0] > 0 else 'down'}")
            ends.append(min(said.items()) if said else None)
        if ends[0] is not None and ends[1] is not None:
            (a, (up_a, _)), (d, (up_d, _)) = ends
            marked.append((int(new_id[a]), int(new_id[i]), int(new_id[j]), int(new_id[d]), 1 if up_a == up_d else 2))
    from .ligand import normalise_bond_stereo, stereo_bonds_from_bonds
    if marked:
        stereogenic = set(stereo_bonds_from_bonds(len(keep), record["bonds"], record["bond_orders"], record["elements"], record["h_count"]))
        marked = [r for r in marked if (min(r[1], r[2]), max(r[1], r[2])) in stereogenic]
    record["bond_stereo"] = normalise_bond_stereo(len(keep), record["bonds"], marked)
    return record
