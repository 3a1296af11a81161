"""Are these two records the same molecule, and what is its one spelling?  `CanonicalForm` holds, for every ligand of a
`LigandLibrary` and from ONE launch (kernel `pd_canonical_form`, csrc/canonical.hip), a canonical numbering of the heavy atoms, an exact
certificate of the annotated graph with a 64-bit key of it and - from a second launch, lazily - the earliest ligand of the library
that is the same molecule; `write_smiles` turns the numbering into a canonical SMILES on the host.  The reference's screening driver
keys each ligand by the MD5 of its SMILES text (screening.py:100-103), so a molecule written two ways is docked twice, and
`MorganFingerprint` says of itself that Tanimoto 1 is necessary, not sufficient.

**The definition** is the package's own, **not InChI and not RDKit's canonical SMILES**: tests/canonical_ref.py in Python integers,
individualisation and refinement in the manner of McKay's nauty with the certificate as the leaf invariant.  `push` is the hash of
`fingerprints.py`, mod 2^32.

    inv(a)      (Z, charge, h_count, isotope, written-aromatic flag), compared lexicographically
    colouring   every atom gets the number of atoms with a strictly smaller key, so a cell's colour is where the cell starts and a
                discrete colouring is a permutation: the colour is the label
    refine      one round colours by (colour, sum mod 2^32 over the bonds (a, b) of push(push(0, twice the order), colour[b])) -
                a commuting sum, any degree; rounds repeat until the number of colours stops growing.  The root is refine(colouring
                by inv): `classes`, the topological symmetry classes
    search      depth-first: at a colouring that is not discrete, the members of the cell of the smallest colour with more than one
                atom are tried in ascending atom index, each by colouring with (colour, a != v) and refining.  A terminal atom is
                skipped when an earlier member of the cell is terminal on the same neighbour with the same bond order (the F of a
                CF3, the methyls of a t-butyl, the O of a sulfonyl): exchanging the two is an automorphism that fixes every annotation
    budget      every refine is one step, the root's included; `max_steps` per ligand.  When a step is due and the budget is spent
                the search stops: `status` 2, the best leaf so far, `canonical` 0.  Without any leaf the labels are the input order
    certificate of a leaf, as uint32 words: n, m; per label Z | (charge + 128) << 8 | h_count << 16 | aromatic << 24 and isotope |
                parity << 16; the bonds lo << 16 | hi << 8 | twice the order in labels, ascending; s; the `bond_stereo` rows b << 23 |
                c << 16 | a << 9 | d << 2 | kind in labels with b < c and a, d the lowest-label substituents, ascending
    parity      0 without a mark and for a mark that cannot mean anything (h_count >= 2, fewer than 3 or more than 4 entries in
                `chiral_order`, two terminal neighbours of equal inv and bond order); else the written code (1 `@`, 2 `@@`),
                exchanged when `chiral_order` in labels (a hydrogen as -1) has an odd number of inversions
    the leaf    with the smallest certificate, word by word; the first found on a tie
    key         (k0, k1): push chained over the certificate from the seeds 0 and 1.  A convenience: the certificate is the identity,
                and `first_of` compares certificates word for word

The set of leaves depends on the constitution only, so every numbering of one annotated molecule has the same minimum; a certificate
spells the annotated graph out, so equal certificates mean the same molecule; a hash collision in a round only makes the refinement
coarser and costs steps.

**Caveats.**  A mark on a non-stereocentre whose equal substituents are not terminal is kept: `CC[C@H](CC)O` equals `CC[C@@H](CC)O`
but not `CCC(CC)O`.  Without `aromatize=True` the Kekule and the aromatic spelling of one molecule differ, as for the fingerprints.
No orbit pruning beyond terminal twins: every independently flippable ring doubles the tree (hexaphenylbenzene 1531 steps,
p-decaphenyl 4095, a poly-p-phenylene of 21 rings runs out of 65536), and status 2 is the honest answer.  No tautomer or charge
normalisation.  Limits: 128 atoms, 512 bonds and 64 stereo rows per ligand, isotopes up to 65535, 65535 ligands per launch;
`first_of` reads O(G^2) keys.  Out of scope: the automorphism group, CIP labels, disconnected records, `redock`.

Device tensors hold the uint32 words as int32 (the same bits)."""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from . import ops
from .pdbio import ELEMENTS
from .smiles import NORMAL_VALENCES, implicit_hydrogens

__all__ = ["CanonicalForm", "canonical_form", "write_smiles", "MAX_STEREO", "CANONICAL_STATUS"]

MAX_STEREO = 64
CANONICAL_STATUS = {0: "done", 2: "the search ran out of steps"}
_ORGANIC = {5: "B", 6: "C", 7: "N", 8: "O", 15: "P", 16: "S", 9: "F", 17: "Cl", 35: "Br", 53: "I"}
_AROMATIC = {5: "b", 6: "c", 7: "n", 8: "o", 15: "p", 16: "s"}
_AROMATIC_BRACKET = {**_AROMATIC, 34: "se", 33: "as"}
_BOND_SYMBOL = {1.0: "-", 2.0: "=", 3.0: "#", 1.5: ":"}


def _check_steps(max_steps, what):
    if isinstance(max_steps, bool) or not isinstance(max_steps, (int, np.integer)) or not 1 <= int(max_steps) < 2 ** 31:
        raise ValueError(f"{what}: max_steps {max_steps!r}; an integer in 1 .. 2^31 - 1")
    return int(max_steps)


def library_tables(library):
    """the three small tables `pd_canonical_form` reads beside the library's own, and the certificate offsets, as numpy arrays:
    `isotopes` int32 [N], `chiral_order` int32 [N,4] (padded with -2; an order of fewer than 3 or more than 4 entries is an empty row),
    `stereo_start` int32 [G+1], `stereo` int32 [S,8] and `cert_start` int32 [G+1] (3 + 2 n + m + s words per ligand).  ValueError for
    an isotope outside 0 .. 65535, an order that names an atom outside the ligand and more than `MAX_STEREO` stereo rows."""
    what = "LigandLibrary.canonical"
    iso = np.concatenate([l.isotopes for l in library.ligands]).astype(np.int64)
    if iso.min() < 0 or iso.max() > 65535:
        raise ValueError(f"{what}: an isotope outside 0 .. 65535")
    order = np.full((library.n_atoms, 4), -2, dtype=np.int32)
    stereo, counts = [], []
    for g, lig in enumerate(library.ligands):
        a0 = int(library.atom_start[g])
        for a, row in lig.chiral_order.items():
            if not 0 <= a < lig.n_atoms or any(not -1 <= v < lig.n_atoms for v in row):
                raise ValueError(f"{what}: ligand {g}: chiral_order of atom {a} leaves the {lig.n_atoms} atoms")
            if 3 <= len(row) <= 4:
                order[a0 + a, :len(row)] = row
        s = int(lig.bond_stereo.shape[0])
        if s > MAX_STEREO:
            raise ValueError(f"{what}: ligand {g}: {s} bond_stereo rows; up to {MAX_STEREO} are taken")
        counts.append(s)
        stereo.append(np.concatenate([lig.bond_stereo.astype(np.int32), np.zeros((s, 1), dtype=np.int32)], axis=1))
    stereo_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    words = 3 + 2 * np.diff(library.atom_start).astype(np.int64) + np.diff(library.bond_start) + np.asarray(counts, dtype=np.int64)
    cert_start = np.concatenate([[0], np.cumsum(words)])
    if cert_start[-1] >= 2 ** 31:
        raise ValueError(f"{what}: {int(cert_start[-1])} certificate words; fewer than 2^31 are taken")
    return {"isotopes": iso.astype(np.int32), "chiral_order": order, "stereo_start": stereo_start,
            "stereo": np.concatenate(stereo).reshape(-1, 8).astype(np.int32), "cert_start": cert_start.astype(np.int32)}


def canonical_form(library, aromatize=False, max_steps=65536, device=None) -> "CanonicalForm":
    """`LigandLibrary.canonical`: ONE launch of `pd_canonical_form` for the whole library (two with `aromatize=True`, which runs
    `pd_aromaticity` in the mode "normalise" first and takes its tables); nothing is read back.  Every check is made on the host
    before the first launch."""
    from .ligand import _device
    what = "LigandLibrary.canonical"
    max_steps = _check_steps(max_steps, what)
    cache = library.__dict__.setdefault("_canonical_tables", {})
    host = cache.get("host")
    if host is None:
        host = cache["host"] = library_tables(library)
    device = _device(device)
    t = library.tables(device)
    c = ops.cached_upload(cache.setdefault("device", {}), device, lambda up: {k: up(v) for k, v in host.items()})
    status = None
    if aromatize:
        perceived = library.aromaticity("normalise", device=device)
        t = dict(t, atoms=perceived["atoms"], bonds=perceived["bonds"])
        status = perceived["status"]
    G, N, B, S, W = library.n_ligands, library.n_atoms, library.n_bonds, int(host["stereo_start"][-1]), int(host["cert_start"][-1])
    new = lambda *shape: torch.empty(shape, device=device, dtype=torch.int32)
    out = {"labels": new(N), "order": new(N), "classes": new(N), "cert": new(W), "key": new(G, 2), "status": new(G), "steps": new(G),
           "leaves": new(G), "canonical": new(G)}
    L_ = ops._lib.init()
    with torch.cuda.device(device):
        ops.check(L_.pd_canonical_form(ops.ptr(t["atom_start"]), ops.ptr(t["bond_start"]), ops.ptr(t["atoms"]),
                                       ops.ptr(t["bonds"]) if B else None, ops.ptr(c["isotopes"]), ops.ptr(c["chiral_order"]),
                                       ops.ptr(c["stereo_start"]), ops.ptr(c["stereo"]) if S else None, ops.ptr(c["cert_start"]),
                                       ops.ptr(out["labels"]), ops.ptr(out["order"]), ops.ptr(out["classes"]), ops.ptr(out["cert"]),
                                       ops.ptr(out["key"]), ops.ptr(out["status"]), ops.ptr(out["steps"]), ops.ptr(out["leaves"]),
                                       ops.ptr(out["canonical"]), G, N, B, S, W, max_steps, ops.stream()), "pd_canonical_form")
    return CanonicalForm(library, out, c["cert_start"], host["cert_start"], bool(aromatize), status, max_steps)


class CanonicalForm:
    """Immutable, on the device, nothing read back: `labels` int32 [N] (the canonical number of every atom within its ligand), `order`
    [N] (its inverse: the atom that has each number), `classes` [N] (the refined root colouring: topological symmetry classes), `cert`
    int32 [W] (the uint32 words; ligand g owns `cert_start[g] .. cert_start[g+1]`, host offsets), `key` int32 [G,2], `status` [G]
    (`CANONICAL_STATUS`), `steps`, `leaves`, `canonical` [G] (1 exactly when the search finished) and `aromaticity_status` [G] with
    `aromatize=True`, else None.  `first_of` / `is_first` come lazily from one launch of `pd_canonical_first`."""

    __slots__ = ("library", "labels", "order", "classes", "cert", "key", "status", "steps", "leaves", "canonical", "cert_start",
                 "aromatize", "aromaticity_status", "max_steps", "n_ligands", "_cert_start_dev", "_lazy")

    def __init__(self, library, out, cert_start_dev, cert_start, aromatize, aromaticity_status, max_steps):
        set_ = lambda k, v: object.__setattr__(self, k, v)
        set_("library", library)
        for k, v in out.items():
            set_(k, v)
        set_("cert_start", cert_start); set_("_cert_start_dev", cert_start_dev); set_("aromatize", aromatize)
        set_("aromaticity_status", aromaticity_status); set_("max_steps", max_steps); set_("n_ligands", library.n_ligands)
        set_("_lazy", {})

    def __setattr__(self, name, value):
        raise AttributeError("CanonicalForm is immutable")

    def __len__(self):
        return self.n_ligands

    def __repr__(self):
        return f"CanonicalForm(n_ligands={self.n_ligands}, aromatize={self.aromatize}, max_steps={self.max_steps})"

    # ------------------------------------------------------------------ the second launch
    @property
    def first_of(self) -> torch.Tensor:
        """int32 [G]: the earliest ligand of the library with the same certificate (itself when there is none); a ligand whose search
        ran out of steps matches nothing.  One launch of `pd_canonical_first` on first use; no read-back."""
        if "first_of" not in self._lazy:
            first = torch.empty(self.n_ligands, device=self.cert.device, dtype=torch.int32)
            L_ = ops._lib.init()
            with torch.cuda.device(self.cert.device):
                ops.check(L_.pd_canonical_first(ops.ptr(self.key), ops.ptr(self.status), ops.ptr(self._cert_start_dev), ops.ptr(self.cert),
                                                ops.ptr(first), self.n_ligands, int(self.cert.shape[0]), ops.stream()), "pd_canonical_first")
            self._lazy["first_of"] = first
        return self._lazy["first_of"]

    @property
    def is_first(self) -> torch.Tensor:
        """bool [G]: the ligand is the first spelling of its molecule in the library"""
        return self.first_of == torch.arange(self.n_ligands, device=self.cert.device, dtype=torch.int32)

    def unique(self) -> torch.Tensor:
        """the indices of the firsts, ascending, int64 on the device: one entry per molecule (and one per unfinished ligand)"""
        return torch.nonzero(self.is_first).flatten()

    def same(self, i: int, j: int) -> bool:
        """are the ligands i and j the same molecule?  False when either search ran out of steps.  The one scalar read-back."""
        G = self.n_ligands
        if not (0 <= int(i) < G and 0 <= int(j) < G):
            raise ValueError(f"CanonicalForm.same: ligands {i} and {j} of {G}")
        i, j = int(i), int(j)
        first, ok = self.first_of, self.status == 0
        return bool((ok[i] & ok[j] & (first[i] == first[j])).item())

    # ------------------------------------------------------------------ the host side
    def _ligands(self):
        """the ligands the labels number: the library's own, or with `aromatize=True` their perceived form (one more launch and
        read-back, `LigandLibrary.aromatized(errors="keep")`)"""
        if "ligands" not in self._lazy:
            lib = self.library
            if self.aromatize:
                lib = lib._rewritten("normalise", self.cert.device, "keep", 65536, "canonical")
            self._lazy["ligands"] = lib.ligands
        return self._lazy["ligands"]

    def _host_labels(self) -> List[np.ndarray]:
        if "labels" not in self._lazy:
            lab, start = self.labels.cpu().numpy(), self.library.atom_start
            self._lazy["labels"] = [lab[int(start[g]):int(start[g + 1])] for g in range(self.n_ligands)]
        return self._lazy["labels"]

    def smiles(self) -> List[str]:
        """G strings: `write_smiles` of every ligand under its labels, after one read-back of `labels`.  The text of a ligand whose
        `canonical` is 0 is a valid SMILES of it, not a canonical one."""
        return [write_smiles(lig, lab) for lig, lab in zip(self._ligands(), self._host_labels())]

    def renumbered(self):
        """A new `LigandLibrary` with every ligand in canonical order - atom k is the atom labelled k, the bonds sorted - and `chiral`,
        `chiral_order` and `bond_stereo` rewritten consistently; its own `canonical()` has identity labels."""
        from .ligand import LigandLibrary
        return LigandLibrary([renumber(lig, lab) for lig, lab in zip(self._ligands(), self._host_labels())])


def renumber(lig, labels):
    """`lig` with atom a as atom labels[a]: the bonds sorted by their new ends, `chiral_order` and `bond_stereo` mapped (the marks
    stay: a mark and its order are mapped together)"""
    from .ligand import Ligand
    lab = _check_labels(lig, labels, "renumber")
    inverse = np.argsort(lab)
    pairs = sorted((min(lab[i], lab[j]), max(lab[i], lab[j]), float(o)) for (i, j), o in zip(lig.bonds.tolist(), lig.bond_orders))
    order = {lab[a]: [(-1 if v < 0 else lab[v]) for v in row] for a, row in lig.chiral_order.items()}
    stereo = [(lab[a], lab[b], lab[c], lab[d], kind) for a, b, c, d, kind, _, _ in lig.bond_stereo.tolist()]
    take = lambda v: np.asarray(v)[inverse]
    return Ligand(take(lig.elements), np.asarray([p[:2] for p in pairs], dtype=np.int64).reshape(-1, 2), [p[2] for p in pairs],
                  take(lig.charges), take(lig.h_count), take(lig.aromatic), take(lig.chiral), order, take(lig.isotopes),
                  source=lig.source, bond_stereo=stereo)


def _check_labels(lig, labels, what):
    lab = [int(v) for v in np.asarray(labels).reshape(-1)]
    if sorted(lab) != list(range(lig.n_atoms)):
        raise ValueError(f"{what}: labels must be a permutation of 0 .. {lig.n_atoms - 1}")
    return lab


def _parity(lig, a, lab, inv, nbr):
    """the parity word of the certificate for atom a (module docstring)"""
    code, row = int(lig.chiral[a]), lig.chiral_order.get(a, ())
    if code not in (1, 2) or lig.h_count[a] >= 2 or not 3 <= len(row) <= 4:
        return 0
    terminal = [(inv[b], o) for b, o in nbr[a] if len(nbr[b]) == 1]
    if len(set(terminal)) != len(terminal):
        return 0
    seq = [(-1 if v < 0 else lab[v]) for v in row]
    inversions = sum(1 for i in range(len(seq)) for j in range(i + 1, len(seq)) if seq[i] > seq[j])
    return 3 - code if inversions & 1 else code


def write_smiles(ligand, labels) -> str:
    """A SMILES string of `ligand` that depends on the numbering `labels` only (a permutation of its atoms; `CanonicalForm.labels`
    makes it canonical): depth-first from label 0, the unvisited neighbours in ascending label - the last as the chain, the others as
    branches; ring closures take the lowest free number when their first atom is written (`%nn` from 10), the closing digits of an
    atom before its opening ones, each in ascending label of the partner.  A bare organic-subset symbol stands exactly where
    `parse_smiles` would infer the same `h_count` and there is no charge, isotope or kept mark, else a bracket atom; aromatic atoms in
    lower case; a bond symbol exactly where the reader's default is another order (between two aromatic atoms 1.5 in a ring and 1
    outside one).  `@` / `@@` from the certificate's parity against the written neighbour order; `/` and `\\` on every single bond
    beside a stated double bond, by propagation over the stereo rows from the first such bond written, which is `/`.  ValueError for a
    bond order outside 1, 1.5, 2, 3, an aromatic atom that has no lower-case symbol, more than 99 open rings, and stereo rows that admit
    no consistent marking (or whose marks would state a double bond that has no row).  Host only, no dependency."""
    lig = ligand
    n = lig.n_atoms
    lab = _check_labels(lig, labels, "write_smiles")
    orders = {}
    nbr = [[] for _ in range(n)]
    for (i, j), o in zip(lig.bonds.tolist(), lig.bond_orders.tolist()):
        if o not in _BOND_SYMBOL:
            raise ValueError(f"write_smiles: the bond ({i}, {j}) has the order {o}; 1, 1.5, 2 and 3 are written")
        orders[i, j] = orders[j, i] = o
        nbr[i].append((j, int(round(2 * o)))); nbr[j].append((i, int(round(2 * o))))
    inv = [(int(lig.elements[a]), int(lig.charges[a]), int(lig.h_count[a]), int(lig.isotopes[a]), bool(lig.aromatic[a])) for a in range(n)]
    by_label = [sorted((b for b, _ in nbr[a]), key=lambda b: lab[b]) for a in range(n)]
    # ---- pass 1: the spanning tree, the ring closures, the order of writing
    root = lab.index(0)
    parent, children = [-1] * n, [[] for _ in range(n)]
    opens, closes = [[] for _ in range(n)], [[] for _ in range(n)]
    pos, closure = {}, set()
    todo = [(root, iter(by_label[root]))]
    pos[root] = 0
    while todo:
        u, it = todo[-1]
        w = next(it, None)
        if w is None:
            todo.pop()
        elif w == parent[u] or (min(u, w), max(u, w)) in closure:
            continue
        elif w in pos:                                              # an ancestor: it opens the ring, u closes it
            closure.add((min(u, w), max(u, w)))
            opens[w].append(u); closes[u].append(w)
        else:
            parent[w] = u; children[u].append(w); pos[w] = len(pos)
            todo.append((w, iter(by_label[w])))
    for a in range(n):
        opens[a].sort(key=lambda b: lab[b]); closes[a].sort(key=lambda b: lab[b])
    # ---- the default order the reader gives an unmarked bond: 1.5 between two aromatic atoms unless the bond is a bridge
    def default(i, j):
        if not (lig.aromatic[i] and lig.aromatic[j]):
            return 1.0
        reach, walk = {i}, [i]
        while walk:
            a = walk.pop()
            for c, _ in nbr[a]:
                if c not in reach and not (a == i and c == j):
                    reach.add(c); walk.append(c)
        return 1.5 if j in reach else 1.0
    # ---- double-bond stereo: one sign per single bond beside a stated double bond, +1 = `/` read from the earlier-written atom
    sign = _directions(lig, pos, nbr, orders)

    def bond_symbol(u, w):                                          # u is written first
        if (u, w) in sign:
            return "/" if sign[u, w] > 0 else "\\"
        return "" if orders[u, w] == default(u, w) else _BOND_SYMBOL[orders[u, w]]
    # ---- pass 2: the text
    free = list(range(1, 100))
    digit = {}

    def ring(number):
        return str(number) if number < 10 else f"%{number}"

    def atom_text(u):
        z, q, h, iso, arom = inv[u]
        written = ([parent[u]] if parent[u] >= 0 else []) + ([-1] if h == 1 else []) + closes[u] + opens[u] + children[u]
        p = _parity(lig, u, lab, inv, nbr)
        mark = ""
        if p:
            seq = [(-1 if v < 0 else lab[v]) for v in written]
            inversions = sum(1 for i in range(len(seq)) for j in range(i + 1, len(seq)) if seq[i] > seq[j])
            mark = "@" if (3 - p if inversions & 1 else p) == 1 else "@@"
        if arom and z not in _AROMATIC_BRACKET:
            raise ValueError(f"write_smiles: atom {u} ({ELEMENTS[z - 1]}) is aromatic; no lower-case symbol is read for it")
        own = [orders[u, b] for b, _ in nbr[u]]
        n_arom = sum(1 for o in own if o == 1.5)
        bare = (z in _ORGANIC and (not arom or z in _AROMATIC) and q == 0 and iso == 0 and not mark
                and h == implicit_hydrogens(z, sum(o for o in own if o != 1.5), n_arom, len(own)))
        if bare:
            return _AROMATIC[z] if arom else _ORGANIC[z]
        symbol = _AROMATIC_BRACKET[z] if arom else ELEMENTS[z - 1].capitalize()
        charge = "" if q == 0 else (("+" if q > 0 else "-") + (str(abs(q)) if abs(q) > 1 else ""))
        return f"[{iso if iso else ''}{symbol}{mark}{'H' + (str(h) if h > 1 else '') if h else ''}{charge}]"

    def emit(u):
        text = atom_text(u)
        for w in closes[u]:
            text += ring(digit[w, u])
        for w in opens[u]:
            if not free:
                raise ValueError("write_smiles: more than 99 rings are open at once")
            digit[u, w] = free.pop(0)
            text += bond_symbol(u, w) + ring(digit[u, w])
        for w in closes[u]:
            free.append(digit[w, u]); free.sort()
        for k, c in enumerate(children[u]):
            branch = bond_symbol(u, c) + emit(c)
            text += branch if k == len(children[u]) - 1 else f"({branch})"
        return text

    return emit(root)


def _directions(lig, pos, nbr, orders):
    """(u, w), u written before w -> +1 (`/`) or -1 (`\\`) for every single bond beside a double bond that has a stereo row.  x[u, w],
    "w seen from u is up", is the sign when u is written first and its opposite otherwise; a row (a, b, c, d, kind) asks x[b, a] ==
    x[c, d] for cis and the opposite for trans, and the two substituents of one end are opposite.  The components of these relations
    are walked from their first-written bond, which is `/`."""
    rows = lig.bond_stereo.tolist()
    if not rows:
        return {}
    key = lambda u, w: (u, w) if pos[u] < pos[w] else (w, u)
    var = lambda u, w: (key(u, w), 1 if pos[u] < pos[w] else -1)     # x[u, w] = factor * sign[key]
    edges = {}

    def relate(p, q, product):                                      # x_p * x_q = product
        (kp, fp), (kq, fq) = p, q
        edges.setdefault(kp, []).append((kq, product * fp * fq)); edges.setdefault(kq, []).append((kp, product * fp * fq))

    stated = set()
    for a, b, c, d, kind, a2, d2 in rows:
        stated.add((min(b, c), max(b, c)))
        for u, s, s2 in ((b, a, a2), (c, d, d2)):
            for w in (s, s2):
                if w >= 0 and orders[u, w] != 1.0:
                    raise ValueError(f"write_smiles: the bond ({u}, {w}) beside the stated double bond ({b}, {c}) is not single")
            if s2 >= 0:
                relate(var(u, s), var(u, s2), -1)
        relate(var(b, a), var(c, d), 1 if kind == 1 else -1)
    sign = {}
    for start in sorted(edges, key=lambda k: (pos[k[0]], pos[k[1]])):
        if start in sign:
            continue
        sign[start] = 1
        walk = [start]
        while walk:
            k = walk.pop()
            for other, product in edges[k]:
                if other not in sign:
                    sign[other] = sign[k] * product
                    walk.append(other)
                elif sign[other] != sign[k] * product:
                    raise ValueError("write_smiles: the bond_stereo rows admit no consistent marking with / and \\")
    marked = {u: set() for k in sign for u in k}
    for u, w in sign:
        marked[u].add(w); marked[w].add(u)
    for (i, j), o in zip(lig.bonds.tolist(), lig.bond_orders.tolist()):   # a double bond without a row must not be stated by the marks
        if o == 2.0 and (min(i, j), max(i, j)) not in stated and marked.get(i, set()) - {j} and marked.get(j, set()) - {i}:
            if (min(i, j), max(i, j)) in set(lig.stereo_bonds()):
                raise ValueError(f"write_smiles: the marks of its neighbours would state the double bond ({i}, {j}), which has no row")
    return sign
