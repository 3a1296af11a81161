"""How does a molecule become model input?  `Ligand` holds one ligand's graph - from a SMILES string (`smiles.parse_smiles`), a
`sdfio.parse_sdf` record or plain arrays - and `LigandLibrary` turns a whole screening library into the reference's ligand feature
blocks in ONE launch (kernel `pd_ligand_features`, csrc/ligand_features.hip): the int8 tables of `get_features_from_ref_mol`
(PhysDock/data/tools/rdkit.py) and the two packed blocks `ref_feat [L,167]` and `rel_tok_feat [L,L,42]` in the column order of
`FeatureLoader._update_smi` (feature_loader.py:327-352).  The reference computes them with RDKit on the host, a `GetShortestPath` call
per atom pair; RDKit is not a dependency of this package, so this is **the package's own definition, not RDKit's bytes**:
tests/ligand_features_ref.py is the written definition, in integers.

    d_token [L,L]            graph distance, min(30, d), 0 on the diagonal
    token_bonds, bond_type   0 single, 1 double, 2 triple, 3 aromatic (order 1.5), 4 other; a pair without a bond is 0 as in the
                             reference's zero-initialised matrices
    bond_as_double           the order as the reference's int8 table holds it: truncated, 1 for an aromatic bond
    bond_is_aromatic         order 1.5
    bond_in_ring             the bond is no bridge
    ref_in_ring_of_n         n = 3 .. 8: the atom lies on a chordless cycle of exactly n atoms
    ref_degree               min(8, heavy neighbours);  ref_implicit_valence  min(8, h_count);  ref_element  Z - 1;  ref_charge
    ref_is_aromatic          written aromatic, or any bond of order 1.5
    ref_chirality            `@@` 0, `@` 1, none 2
    bond_is_conjugated       pi atoms have a bond of order >= 1.5; donor atoms are N, O, S without one and with charge <= 0.  A single
                             bond is conjugated between two pi atoms or a pi atom and a donor; a non-aromatic multiple bond when a
                             conjugated single bond touches either end; an aromatic bond always
    ref_hybridization        v = h_count + sum of orders (an atom's aromatic bonds count as their number + 1); lone pairs =
                             max(0, group valence electrons - charge - v) // 2; n = degree + h_count + lone pairs; n <= 1 -> 0 (S),
                             2 -> 1 (SP), 3 -> 2, 4 -> 3, 5 -> 4, 6 -> 5, more -> 6; a donor atom with n = 4 on a conjugated single bond
                             is 2 (SP2): the amide N, the phenol O

`Ligand.embed_reference` makes the 3-D reference conformer `ref_pos` by distance geometry from ideal bounds
(`conformers.ideal_bounds`, `ConformerEnsemble`), `conf_meta` returns the reference's `CONF_META_DATA["XXX"]` entry and label features,
`into_batch` writes a ligand into a model feature dict on the device, and `graph()` feeds every `from_bonds` constructor of the package.

**Aromaticity.**  The constructors perceive nothing: a Kekule ring (an SD file from the PDB, `C1=CC=CC=C1`) stays Kekule in every
table unless it is asked for.  `Ligand.aromatized()` / `LigandLibrary.aromatized()` return the ligands with their aromatic rings
perceived, `kekulized()` with every aromatic bond written single or double, `LigandLibrary.aromaticity(mode)` the same as device
tables without a read-back and `LigandLibrary.features(aromatize=True)` feeds them to `pd_ligand_features` (kernel `pd_aromaticity`,
csrc/aromaticity.hip).  Again the package's own definition, tests/aromaticity_ref.py in integers: rings are the chordless cycles of
5 .. 7 atoms, each judged on its own (4n + 2 electrons from a short list of contributions); the Kekule form is the lexicographically
first perfect matching of the atoms that need a double bond, so it depends on the atom numbering.  Azulene is not perceived and
indolizine only in its five-ring (RDKit perceives both through the fused envelope); no tautomers; a double bond that lies in some
other, non-aromatic ring still counts as cyclic.

**Double-bond stereo.**  `bond_stereo` holds the cis / trans arrangement of the double bonds a SMILES string marks with `/` and `\\`
(`from_graph(bond_stereo=)`, `from_sdf(stereo="coords")` give it too); `conformers.ideal_bounds` pins those bonds, so `embed_reference`
returns the stated isomer, and `bond_stereo.BondStereo` reads the arrangement off every pose (kernel `pd_bond_stereo`).  The feature
tables hold no bond stereo, as the reference's do not.  cis / trans relative to the lowest-index substituents, not CIP E / Z.

**Caveats.**  No aromaticity perception and no kekulisation by default (above).  A stereogenic double bond without marks
(`unspecified_stereo_bonds`) comes out as either isomer and at any twist.  Ring sizes are those of chordless cycles, not of RDKit's
ring set (they agree on ordinary ring systems, not on cages).
Hybridisation and conjugation are the rules above, not RDKit's.  The conformer has no torsion preferences and no force-field clean-up.
Limits: 1 .. 128 atoms and up to 512 bonds per ligand, up to 65535 ligands per launch.  Out of scope: the CCD lookup, MSA features,
`FeatureLoader.load`."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .pdbio import ELEMENTS
from .smiles import MAX_ATOMS, NORMAL_VALENCES, implicit_hydrogens, parse_smiles

__all__ = ["Ligand", "LigandLibrary", "ATOM_COLUMNS", "PAIR_COLUMNS", "MAX_ATOMS", "MAX_BONDS", "MAX_LIGANDS", "GROUP_ELECTRONS",
           "chordless_rings", "AROMATICITY_MODES", "AROMATICITY_STATUS", "stereo_bonds_from_bonds", "normalise_bond_stereo"]

MAX_BONDS, MAX_LIGANDS = 512, 65535
#: columns of the kernel's int8 tables (rows of 16 per atom and of 8 per atom pair; the rest is zero)
ATOM_COLUMNS = ("ref_charge", "ref_element", "ref_is_aromatic", "ref_degree", "ref_hybridization", "ref_implicit_valence",
                "ref_chirality", "ref_in_ring_of_3", "ref_in_ring_of_4", "ref_in_ring_of_5", "ref_in_ring_of_6", "ref_in_ring_of_7",
                "ref_in_ring_of_8")
PAIR_COLUMNS = ("d_token", "token_bonds", "bond_type", "bond_as_double", "bond_in_ring", "bond_is_conjugated", "bond_is_aromatic")
ATOM_ROW, PAIR_ROW, REF_FEAT, REL_TOK_FEAT = 16, 8, 167, 42
#: the `mode` argument of `pd_aromaticity` and what its `status` says
AROMATICITY_MODES = {"kekulise": 0, "perceive": 1, "normalise": 2}
AROMATICITY_STATUS = {0: "done", 1: "no Kekule structure exists", 2: "the matching ran out of steps"}


def _group_electrons():
    """valence electrons by atomic number (index 0 unused): the group of a main-group element, the group number of a transition metal,
    3 for the lanthanides and actinides"""
    out = [0] * 129
    rows = ((1, 2), (3, 10), (11, 18), (19, 36), (37, 54), (55, 86), (87, 118))
    for first, last in rows:
        n = last - first + 1
        for z in range(first, last + 1):
            k = z - first + 1                                       # position in the period
            if n == 2:
                e = k
            elif n == 8:
                e = k
            elif n == 18:
                e = k if k <= 12 else k - 10
            else:                                                   # 32: s2, fourteen f elements and the first d, nine d, six p
                e = k if k <= 2 else (3 if k <= 17 else (k - 14 if k <= 26 else k - 24))
            out[z] = e
    for z in range(119, 129):
        out[z] = 0
    return tuple(out)


#: the table `lone pairs` reads (the kernel holds the same numbers)
GROUP_ELECTRONS = _group_electrons()


def chordless_rings(n_atoms: int, bonds, max_size: int = 8) -> List[tuple]:
    """every chordless cycle of 3 .. max_size atoms as a tuple of atoms in ring order, starting at its smallest atom towards the
    smaller of that atom's two ring neighbours; sorted"""
    adj = [set() for _ in range(n_atoms)]
    for i, j in bonds:
        adj[int(i)].add(int(j)); adj[int(j)].add(int(i))
    found = set()

    def walk(path, blocked):
        last = path[-1]
        for w in sorted(adj[last]):
            if w in path or w in blocked or w < path[0]:
                continue
            if len(path) >= 2 and path[0] in adj[w]:
                if path[1] < w:
                    found.add(tuple(path) + (w,))
                continue
            if len(path) + 1 < max_size:
                walk(path + [w], blocked | (adj[last] if len(path) >= 2 else set()))

    for s in range(n_atoms):
        walk([s], set())
    return sorted(found)


def stereo_bonds_from_bonds(n_atoms: int, bonds, bond_orders, elements, h_count) -> List[tuple]:
    """The stereogenic double bonds of a graph over heavy atoms as sorted pairs (b, c), b < c: the order is 2.0; both ends are C or N;
    each end has 1 or 2 heavy substituents besides the partner, at most one hydrogen, no more than two substituents in all and no
    second bond of an order above 1; at an end with two heavy substituents the two lie in different classes of
    `chirality.symmetry_classes`; and the bond lies in no chordless ring of at most 7 atoms (`chordless_rings`)."""
    from .chirality import symmetry_classes
    n = int(n_atoms)
    pairs = [(int(i), int(j)) for i, j in np.asarray(bonds, dtype=np.int64).reshape(-1, 2).tolist()]
    orders = [float(o) for o in np.asarray(bond_orders, dtype=np.float64).reshape(-1)]
    z = [int(e) for e in np.asarray(elements).reshape(-1)]
    h = [int(v) for v in np.asarray(h_count).reshape(-1)]
    if not any(o == 2.0 for o in orders):
        return []
    nbr = [{} for _ in range(n)]
    for (i, j), o in zip(pairs, orders):
        nbr[i][j] = o; nbr[j][i] = o
    cls = symmetry_classes(n, pairs, z, orders)
    in_ring = set()
    for ring in chordless_rings(n, pairs, max_size=7):
        for k in range(len(ring)):
            i, j = ring[k], ring[(k + 1) % len(ring)]
            in_ring.add((min(i, j), max(i, j)))
    out = []
    for (i, j), o in zip(pairs, orders):
        b, c = min(i, j), max(i, j)
        if o != 2.0 or (b, c) in in_ring:
            continue
        for u, v in ((b, c), (c, b)):
            subs = [w for w in nbr[u] if w != v]
            if z[u] not in (6, 7) or not 1 <= len(subs) <= 2 or h[u] > 1 or len(subs) + h[u] > 2:
                break
            if any(nbr[u][w] > 1.0 for w in subs) or (len(subs) == 2 and cls[subs[0]] == cls[subs[1]]):
                break
        else:
            out.append((b, c))
    return sorted(out)


def normalise_bond_stereo(n_atoms: int, bonds, rows) -> np.ndarray:
    """rows (a, b, c, d, kind[, a2, d2]) - a any heavy substituent of b, d any of c, kind 1 cis / 2 trans of a against d - as the int32
    [n,7] table (a, b, c, d, kind, a2, d2) of `smiles.parse_smiles`: b < c, a and d the lowest substituents of b and c (kind flipped
    once for every end whose lowest substituent is not the one named), a2 and d2 the other substituent or -1, sorted by (b, c).  Only
    the first five columns are read.  ValueError for atoms that are not bonded as stated, a kind other than 1 or 2, an end with no or
    more than two substituents, and a bond named twice."""
    n = int(n_atoms)
    rows = np.asarray([] if rows is None else rows, dtype=np.int64)
    if rows.size == 0:
        return _frozen(np.zeros((0, 7)), np.int32)
    if rows.ndim != 2 or rows.shape[1] not in (5, 7):
        raise ValueError(f"bond_stereo: rows of (a, b, c, d, kind), got an array of shape {rows.shape}")
    nbr = [set() for _ in range(n)]
    for i, j in np.asarray(bonds, dtype=np.int64).reshape(-1, 2).tolist():
        nbr[i].add(j); nbr[j].add(i)
    out = {}
    for a, b, c, d, kind in rows[:, :5].tolist():
        if min(a, b, c, d) < 0 or max(a, b, c, d) >= n:
            raise ValueError(f"bond_stereo: the row {(a, b, c, d, kind)} leaves the {n} atoms")
        if b > c:
            a, b, c, d = d, c, b, a
        if c not in nbr[b] or a not in nbr[b] or d not in nbr[c] or a == c or d == b:
            raise ValueError(f"bond_stereo: the atoms of the row {(a, b, c, d, kind)} are not bonded a-b=c-d")
        if kind not in (1, 2):
            raise ValueError(f"bond_stereo: kind {kind} of the bond ({b}, {c}); 1 is cis, 2 is trans")
        if (b, c) in out:
            raise ValueError(f"bond_stereo: two rows for the bond ({b}, {c})")
        ends = []
        for u, v, named in ((b, c, a), (c, b, d)):
            subs = sorted(nbr[u] - {v})
            if not 1 <= len(subs) <= 2:
                raise ValueError(f"bond_stereo: atom {u} of the bond ({b}, {c}) has {len(subs)} substituents; 1 or 2 are taken")
            if subs[0] != named:
                kind = 3 - kind
            ends.append((subs[0], subs[1] if len(subs) == 2 else -1))
        out[b, c] = (ends[0][0], b, c, ends[1][0], kind, ends[0][1], ends[1][1])
    return _frozen([out[k] for k in sorted(out)], np.int32).reshape(-1, 7)


def _valence_rule(elements, bonds, bond_orders, charges):
    """`smiles.implicit_hydrogens` per atom of a graph without written hydrogen counts.  A charge moves the valence it is measured
    against: a cation of group 15 / 16 has one more, an anion one fewer, any other charged atom one fewer."""
    h = np.zeros(len(elements), dtype=np.int64)
    pairs = np.asarray(bonds).reshape(-1, 2).tolist()
    for a in range(len(elements)):
        z, q = int(elements[a]), int(charges[a])
        if z not in NORMAL_VALENCES:
            continue
        own = [float(o) for (i, j), o in zip(pairs, bond_orders) if a in (i, j)]
        shift = -q if z in (7, 8, 15, 16) else abs(q)
        n_arom = sum(1 for o in own if o == 1.5)
        h[a] = implicit_hydrogens(z, sum(o for o in own if o != 1.5) + shift, n_arom, len(own) + shift)
    return h


def _device(device) -> torch.device:
    """`device` as a cache key; None is the current CUDA device, as in `ConformerEnsemble.embed`"""
    return ops.resolve_device(torch.device("cuda", torch.cuda.current_device()) if device is None else device)


def _frozen(a, dtype):
    a = np.array(a, dtype=dtype)
    a.setflags(write=False)
    return a


class Ligand:
    """One ligand's graph over its heavy atoms, immutable: `elements` (atomic numbers), `bonds` int64 [n,2], `bond_orders` float64,
    `charges`, `h_count`, `aromatic` (bool), `chiral` (0 none, 1 `@`, 2 `@@`), `chiral_order` (atom -> its neighbours in OpenSMILES
    order, -1 a hydrogen; only what a SMILES string gives), `isotopes` and `bond_stereo`: int32 [n,7] rows (a, b, c, d, kind, a2, d2)
    of the double bonds whose cis / trans arrangement is stated (`smiles.parse_smiles`; given as (a, b, c, d, kind) they are
    normalised by `normalise_bond_stereo`), empty by default.  A row on a bond that `stereo_bonds_from_bonds` does not list raises;
    `unspecified_stereo_bonds` are the listed bonds without a row."""

    def __init__(self, elements, bonds, bond_orders, charges, h_count, aromatic, chiral, chiral_order=None, isotopes=None, source="",
                 bond_stereo=None):
        self.elements = _frozen(elements, np.int64).reshape(-1)
        L = self.n_atoms = int(self.elements.shape[0])
        if not 1 <= L <= MAX_ATOMS:
            raise ValueError(f"Ligand: {L} heavy atoms; 1 .. {MAX_ATOMS} are taken")
        if self.elements.min() < 1 or self.elements.max() > len(ELEMENTS):
            raise ValueError(f"Ligand: an atomic number outside 1 .. {len(ELEMENTS)}")
        self.bonds = _frozen(bonds, np.int64).reshape(-1, 2)
        self.bond_orders = _frozen(bond_orders, np.float64).reshape(-1)
        nb = self.n_bonds = int(self.bonds.shape[0])
        if self.bond_orders.shape[0] != nb:
            raise ValueError(f"Ligand: {nb} bonds but {self.bond_orders.shape[0]} bond orders")
        if nb > MAX_BONDS:
            raise ValueError(f"Ligand: {nb} bonds; up to {MAX_BONDS} are taken")
        if nb and (self.bonds.min() < 0 or self.bonds.max() >= L or (self.bonds[:, 0] == self.bonds[:, 1]).any()):
            raise ValueError(f"Ligand: a bond leaves the {L} atoms or joins an atom to itself")
        if len({(min(i, j), max(i, j)) for i, j in self.bonds.tolist()}) != nb:
            raise ValueError("Ligand: two bonds between the same atoms")
        o2 = 2.0 * self.bond_orders
        if nb and ((o2 != np.round(o2)).any() or o2.min() < 1 or o2.max() > 8):
            raise ValueError("Ligand: bond orders are multiples of 0.5 in 0.5 .. 4")
        self.charges = _frozen(np.zeros(L) if charges is None else charges, np.int64).reshape(-1)
        self.aromatic = _frozen(np.zeros(L) if aromatic is None else aromatic, bool).reshape(-1)
        self.chiral = _frozen(np.zeros(L) if chiral is None else chiral, np.int64).reshape(-1)
        self.isotopes = _frozen(np.zeros(L) if isotopes is None else isotopes, np.int64).reshape(-1)
        if h_count is None:
            h_count = _valence_rule(self.elements, self.bonds, self.bond_orders, self.charges)
        self.h_count = _frozen(h_count, np.int64).reshape(-1)
        for name in ("charges", "aromatic", "chiral", "isotopes", "h_count"):
            if getattr(self, name).shape[0] != L:
                raise ValueError(f"Ligand: {getattr(self, name).shape[0]} entries of {name} for {L} atoms")
        if np.abs(self.charges).max() > 127 or self.h_count.min() < 0 or self.h_count.max() > 127 or not np.isin(self.chiral, (0, 1, 2)).all():
            raise ValueError("Ligand: a charge beyond +-127, an h_count outside 0 .. 127 or a chiral code other than 0, 1, 2")
        self.chiral_order = {int(a): tuple(int(v) for v in order) for a, order in (chiral_order or {}).items()}
        self.source = str(source)
        adj = self.neighbours()
        reach, todo = {0}, [0]
        while todo:
            for c in adj[todo.pop()]:
                if c not in reach:
                    reach.add(c); todo.append(c)
        if len(reach) != L:
            raise ValueError(f"Ligand: the graph is not connected: atom {min(set(range(L)) - reach)} cannot be reached from atom 0")
        self.bond_stereo = normalise_bond_stereo(L, self.bonds, bond_stereo)
        self._stereo_bonds = None
        for row in self.bond_stereo.tolist():
            if (row[1], row[2]) not in self.stereo_bonds():
                raise ValueError(f"Ligand: bond_stereo names the bond ({row[1]}, {row[2]}), which is not stereogenic "
                                 "(`stereo_bonds_from_bonds`)")
        self._features = {}

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_smiles(text: str) -> "Ligand":
        r = parse_smiles(text)
        return Ligand(r["elements"], r["bonds"], r["bond_orders"], r["charges"], r["h_count"], r["aromatic"], r["chiral"],
                      r["chiral_order"], r["isotopes"], source=text.strip(), bond_stereo=r["bond_stereo"])

    @staticmethod
    def from_graph(elements, bonds, bond_orders, charges=None, h_count=None, aromatic=None, chiral=None, bond_stereo=None) -> "Ligand":
        """elements: atomic numbers or symbols; `h_count=None` uses the valence rule of `smiles.parse_smiles`; `bond_stereo`: rows
        (a, b, c, d, kind), kind 1 cis / 2 trans of the substituent a of b against the substituent d of c"""
        z = [(_SYMBOL_Z.get(e.strip().upper(), 0) if isinstance(e, str) else int(e)) for e in (elements.tolist() if hasattr(elements, "tolist") else elements)]
        bonds = np.asarray(bonds.tolist() if hasattr(bonds, "tolist") else list(bonds), dtype=np.int64).reshape(-1, 2)
        orders = np.ones(len(bonds)) if bond_orders is None else np.asarray(bond_orders, dtype=np.float64)
        return Ligand(z, bonds, orders, charges, h_count, aromatic, chiral, bond_stereo=bond_stereo)

    @staticmethod
    def from_sdf(record: dict, stereo: Optional[str] = None, device=None) -> "Ligand":
        """a `sdfio.parse_sdf` record; its hydrogens on heavy atoms are folded into `h_count`, the heavy atoms keep their order.
        `stereo="coords"`: every stereogenic double bond (`stereo_bonds_from_bonds`) is labelled cis / trans from the record's 3-D
        coordinates (`bond_stereo.BondStereo.label`, one launch and one read of the labels); a bond whose dihedral is undefined or
        exactly perpendicular stays unspecified.  The default reads no stereo."""
        if stereo not in (None, "coords"):
            raise ValueError(f"Ligand.from_sdf: stereo={stereo!r}; None or \"coords\"")
        z = np.asarray([_SYMBOL_Z.get(str(e).strip().upper(), 0) for e in record["elements"]], dtype=np.int64)
        bonds = np.asarray(record["bonds"], dtype=np.int64).reshape(-1, 2)
        orders = np.asarray(record["bond_orders"], dtype=np.float64).reshape(-1)
        charges = np.asarray(record["charges"], dtype=np.int64).reshape(-1)
        n = len(z)
        nbr = [[] for _ in range(n)]
        for i, j in bonds.tolist():
            nbr[i].append(j); nbr[j].append(i)
        folded = np.asarray([z[a] == 1 and len(nbr[a]) == 1 and z[nbr[a][0]] != 1 for a in range(n)], dtype=bool)
        if n > 1 and ((z == 1) & ~folded).any():
            raise ValueError(f"Ligand.from_sdf: the hydrogen {int(np.nonzero((z == 1) & ~folded)[0][0])} is not bonded to one heavy atom")
        extra = np.zeros(n, dtype=np.int64)
        for a in np.nonzero(folded)[0]:
            extra[nbr[a][0]] += 1
        new_id = np.cumsum(~folded) - 1
        keep_b = ~folded[bonds[:, 0]] & ~folded[bonds[:, 1]] if len(bonds) else np.zeros(0, dtype=bool)
        h = _valence_rule(z, bonds, orders, charges)[~folded] + extra[~folded]      # the bonds to the folded hydrogens count as bonds
        lig = Ligand(z[~folded], new_id[bonds[keep_b]].reshape(-1, 2), orders[keep_b], charges[~folded], h, None, None,
                     source=str(record.get("title", "")))
        if stereo is None or not lig.stereo_bonds():
            return lig
        from .bond_stereo import BondStereo
        nbr = lig.neighbours()
        rows = [(min(w for w in nbr[b] if w != c), b, c, min(w for w in nbr[c] if w != b), 1) for b, c in lig.stereo_bonds()]
        x = torch.as_tensor(np.asarray(record["coords"], dtype=np.float32)[~folded], device=_device(device))
        state = BondStereo.from_tables(np.asarray(normalise_bond_stereo(lig.n_atoms, lig.bonds, rows))[:, [0, 1, 2, 3, 5, 6]],
                                       None).label(x[None])[0].tolist()           # the one read-back
        rows = [r[:4] + (s,) for r, s in zip(rows, state) if s in (1, 2)]
        return Ligand(lig.elements, lig.bonds, lig.bond_orders, lig.charges, lig.h_count, None, None, source=lig.source, bond_stereo=rows)

    # ------------------------------------------------------------------ the graph
    def neighbours(self) -> List[List[int]]:
        adj = [[] for _ in range(self.n_atoms)]
        for i, j in self.bonds.tolist():
            adj[i].append(j); adj[j].append(i)
        return adj

    def graph(self):
        """(elements, bonds, bond_orders, charges) for the `from_bonds` constructors of the package"""
        return self.elements.copy(), self.bonds.copy(), self.bond_orders.copy(), self.charges.copy()

    def symbols(self) -> List[str]:
        return [ELEMENTS[int(z) - 1] for z in self.elements]

    def stereo_bonds(self) -> List[tuple]:
        """`stereo_bonds_from_bonds` of this graph: the double bonds (b, c) that can be cis or trans (computed once)"""
        if self._stereo_bonds is None:
            self._stereo_bonds = tuple(stereo_bonds_from_bonds(self.n_atoms, self.bonds, self.bond_orders, self.elements, self.h_count))
        return list(self._stereo_bonds)

    @property
    def unspecified_stereo_bonds(self) -> List[tuple]:
        """the stereogenic double bonds (b, c) that `bond_stereo` has no row for"""
        stated = {(r[1], r[2]) for r in self.bond_stereo.tolist()}
        return [bc for bc in self.stereo_bonds() if bc not in stated]

    def perceive(self) -> Dict[str, np.ndarray]:
        """what `conformers.ideal_bounds` needs, by the rules of the module docstring on the host: `hybridization` [L], `conjugated`
        [n_bonds] (bool) and `rings` (`chordless_rings`)"""
        L, o = self.n_atoms, self.bond_orders
        bi, bj = self.bonds[:, 0], self.bonds[:, 1]
        arom, single, multi = o == 1.5, o == 1.0, (o >= 2.0)
        count = lambda mask, w=None: (np.bincount(bi[mask], (w[mask] if w is not None else None), L)
                                      + np.bincount(bj[mask], (w[mask] if w is not None else None), L))
        pi = count(o >= 1.5) > 0
        donor = np.isin(self.elements, (7, 8, 16)) & ~pi & (self.charges <= 0)
        conj_single = single & ((pi[bi] & pi[bj]) | (pi[bi] & donor[bj]) | (donor[bi] & pi[bj]))
        on_conj = count(conj_single) > 0
        conjugated = arom | conj_single | (multi & (on_conj[bi] | on_conj[bj]))
        n_arom = count(arom).astype(np.int64)
        v = self.h_count + np.floor(count(~arom, o)).astype(np.int64) + np.where(n_arom > 0, n_arom + 1, 0)
        lone = np.maximum(0, np.asarray(GROUP_ELECTRONS)[self.elements] - self.charges - v) // 2
        n = count(np.ones(len(o), dtype=bool)).astype(np.int64) + self.h_count + lone
        hyb = np.select([n <= 1, n == 2, n == 3, n == 4, n == 5, n == 6], [0, 1, 2, 3, 4, 5], 6)
        hyb = np.where(donor & (n == 4) & on_conj, 2, hyb)
        return {"hybridization": hyb.astype(np.int64), "conjugated": conjugated, "rings": chordless_rings(L, self.bonds.tolist())}

    # ------------------------------------------------------------------ device side
    def features(self, device=None) -> Dict[str, torch.Tensor]:
        """this ligand's tables and blocks on the device (`LigandLibrary.features` of a library of one, computed once per device):
        every name of `ATOM_COLUMNS` int8 [L], of `PAIR_COLUMNS` int8 [L,L], `ref_feat` fp32 [L,167] (columns 0 .. 2, `ref_pos`, are
        zero) and `rel_tok_feat` fp32 [L,L,42].  `device=None` is the current CUDA device.  The kernel's result is kept; every call
        returns fresh copies, so a caller may write into them."""
        device = _device(device)
        if device not in self._features:
            lib = LigandLibrary([self])
            self._features[device] = lib.split(lib.features(device), 0)
        return {k: v.clone() for k, v in self._features[device].items()}

    def aromatized(self, device=None) -> "Ligand":
        """this ligand with its aromatic rings perceived (`LigandLibrary.aromatized` of a library of one): aromatic input is kekulised
        first, so partly aromatic input is handled.  ValueError when no Kekule structure exists."""
        return LigandLibrary([self]).aromatized(device).ligands[0]

    def kekulized(self, device=None) -> "Ligand":
        """this ligand with every aromatic bond written single or double (`LigandLibrary.kekulized` of a library of one)"""
        return LigandLibrary([self]).kekulized(device).ligands[0]

    def fingerprint(self, radius: int = 2, n_bits: int = 2048, atom_invariants=None, aromatize: bool = False, device=None):
        """this ligand's circular fingerprint (`LigandLibrary.fingerprints` of a library of one): a `MorganFingerprint` of one row"""
        return LigandLibrary([self]).fingerprints(radius, n_bits, atom_invariants, aromatize, device)

    def substructure(self, queries, aromatize: bool = False, max_steps: int = 65536, device=None):
        """the queries on this ligand (`LigandLibrary.substructure` of a library of one): a `SubstructureMatches` with G = 1"""
        return LigandLibrary([self]).substructure(queries, aromatize, max_steps, device)

    def canonical(self, aromatize: bool = False, max_steps: int = 65536, device=None):
        """this ligand's canonical form (`LigandLibrary.canonical` of a library of one): a `CanonicalForm` with G = 1"""
        return LigandLibrary([self]).canonical(aromatize, max_steps, device)

    def canonical_smiles(self, aromatize: bool = False, max_steps: int = 65536, device=None) -> str:
        """the one spelling of this molecule (`canonical().smiles()[0]`); ValueError when the search ran out of `max_steps`"""
        form = self.canonical(aromatize, max_steps, device)
        if not int(form.canonical[0]):                                                  # (a read-back)
            raise ValueError(f"Ligand.canonical_smiles: the search ran out of {int(max_steps)} steps: no canonical numbering")
        return form.smiles()[0]

    def identity_key(self, aromatize: bool = False, max_steps: int = 65536, device=None) -> int:
        """the 64-bit key of this molecule's certificate, k0 << 32 | k1 (a read-back); ValueError when the search ran out of steps"""
        form = self.canonical(aromatize, max_steps, device)
        if not int(form.canonical[0]):
            raise ValueError(f"Ligand.identity_key: the search ran out of {int(max_steps)} steps: no canonical numbering")
        k0, k1 = (int(v) & 0xFFFFFFFF for v in form.key[0].tolist())
        return k0 << 32 | k1

    def embed_reference(self, seed: int = 0, C: int = 32, device=None) -> Dict[str, torch.Tensor]:
        """The reference conformer: C distance-geometry conformers from `conformers.ideal_bounds(self)`
        (`ConformerEnsemble.from_tables(...).embed`), of which the accepted one with the smallest `err` - the lowest index on a tie - is
        `ref_pos` fp32 [L,3]; `ref_feat` is `features()["ref_feat"]` with it in columns 0 .. 2.  Also `index`, `err`, `max_violation`
        (host numbers), `n_accepted` and `unspecified_centres`.  One read of the C errors.  RuntimeError when no conformer is accepted."""
        from .conformers import ConformerEnsemble, ideal_bounds
        device = _device(device)
        t = ideal_bounds(self)
        feats = self.features(device)
        if self.n_atoms == 1:
            pos = torch.zeros(1, 3, device=device)
            index, err, viol, n_ok = 0, 0.0, 0.0, 1
        else:
            ens = ConformerEnsemble.from_tables(t["lo"], t["up"], t["centres"], t["vol_lo"], t["vol_hi"])       # (the bounds pin bond_stereo)
            out = ens.embed(int(C), int(seed), keep=None, device=device)
            ok, errs = out["ok"].cpu().numpy().astype(bool), out["err"].cpu().numpy()
            if not ok.any():
                raise RuntimeError(f"Ligand.embed_reference: none of {int(C)} conformers of {self.source or 'the ligand'} was accepted "
                                   f"(seed {int(seed)})")
            index = int(np.argmin(np.where(ok, errs, np.inf)))
            pos, err, viol, n_ok = out["x"][index], float(errs[index]), float(out["max_violation"][index]), int(ok.sum())
        ref_feat = feats["ref_feat"]
        ref_feat[:, :3] = pos
        return {"ref_pos": pos, "ref_feat": ref_feat, "index": index, "err": err, "max_violation": viol, "n_accepted": n_ok,
                "unspecified_centres": t["unspecified_centres"]}

    def conf_meta(self, ref_pos=None, device=None, seed: int = 0):
        """(CONF_META_DATA["XXX"], label_feature) of the reference's `_update_smi` and `get_features_from_ref_mol` as numpy arrays:
        `ref_feat`, `rel_tok_feat`, `ref_atom_name_chars`, `ref_element`, `token_bonds`; `x_gt` is `ref_pos` (given, or embedded)."""
        f = self.features(device)
        if ref_pos is None:
            ref_pos = self.embed_reference(seed=seed, device=device)["ref_pos"]
        pos = np.asarray(ref_pos.detach().cpu() if isinstance(ref_pos, torch.Tensor) else ref_pos, dtype=np.float32).reshape(self.n_atoms, 3)
        ref_feat = f["ref_feat"].cpu().numpy().copy()
        ref_feat[:, :3] = pos
        L = self.n_atoms
        meta = {"ref_feat": ref_feat, "rel_tok_feat": f["rel_tok_feat"].cpu().numpy().copy(),
                "ref_atom_name_chars": [f"{s + str(k):<4}" for k, s in enumerate(self.symbols())],
                "ref_element": f["ref_element"].cpu().numpy().copy(), "token_bonds": f["token_bonds"].cpu().numpy().copy()}
        label = {"x_gt": pos.copy(), "x_exists": np.ones(L, dtype=np.int64), "a_mask": np.ones(L, dtype=np.int64),
                 "restype": np.array([20], dtype=np.int64), "residue_index": np.arange(1, dtype=np.int64),
                 "atom_id_to_conformer_atom_id": np.arange(L, dtype=np.int64), "conformer_id_to_chunk_sizes": np.array([L], dtype=np.int64)}
        return meta, label

    def into_batch(self, batch: Dict[str, torch.Tensor], ref_pos=None, seed: int = 0) -> Dict[str, torch.Tensor]:
        """Overwrites, in place and on the batch's device, the ligand atoms' rows of `ref_feat` and `ref_pos` (the atoms of
        `driver.ligand_atom_mask`) and the ligand x ligand block of `rel_tok_feat` and `token_bonds_feature` (the tokens of `is_ligand`,
        one per atom).  `ref_pos` [L,3]: the conformer to write (default: `embed_reference(seed)`).  A batch whose ligand has another
        atom or token count raises before anything is written."""
        from .driver import ligand_atom_mask
        atoms = torch.nonzero(ligand_atom_mask(batch)).flatten()
        tokens = torch.nonzero(batch["is_ligand"].bool()).flatten()
        L = self.n_atoms
        if int(atoms.numel()) != L or int(tokens.numel()) != L:
            raise ValueError(f"Ligand.into_batch: the batch's ligand has {int(atoms.numel())} atoms in {int(tokens.numel())} tokens, "
                             f"this ligand {L} atoms")
        device = batch["ref_feat"].device
        if tuple(batch["ref_feat"].shape[1:]) != (REF_FEAT,) or tuple(batch["rel_tok_feat"].shape[2:]) != (REL_TOK_FEAT,):
            raise ValueError("Ligand.into_batch: ref_feat must be [A,167] and rel_tok_feat [T,T,42]")
        if ref_pos is None:
            ref_pos = self.embed_reference(seed=seed, device=device)["ref_pos"]
        pos = torch.as_tensor(ref_pos, device=device).float()
        if tuple(pos.shape) != (L, 3):
            raise ValueError(f"Ligand.into_batch: ref_pos must be [{L},3], got {tuple(pos.shape)}")
        f = self.features(device)
        rows = f["ref_feat"]
        rows[:, :3] = pos
        batch["ref_feat"][atoms] = rows.to(batch["ref_feat"].dtype)
        batch["ref_pos"][atoms] = pos.to(batch["ref_pos"].dtype)
        ti, tj = tokens[:, None], tokens[None, :]
        batch["rel_tok_feat"][ti, tj] = f["rel_tok_feat"].to(batch["rel_tok_feat"].dtype)
        batch["token_bonds_feature"][ti, tj] = f["token_bonds"].to(batch["token_bonds_feature"].dtype)
        return batch

    def __repr__(self):
        return f"Ligand(n_atoms={self.n_atoms}, n_bonds={self.n_bonds}{', ' + repr(self.source) if self.source else ''})"


_SYMBOL_Z = {s.upper(): k + 1 for k, s in enumerate(ELEMENTS)}
_SYMBOL_Z["D"] = 1


class LigandLibrary:
    """G ligands as CSR tables for one launch of `pd_ligand_features`: `atom_start`, `bond_start` int32 [G+1], `pair_start` int64
    [G+1] (prefix sums of L^2), `atoms` int32 [N,4] (Z, charge, h_count, flags: bit 0 written aromatic, bits 1 - 2 the chiral code)
    and `bonds` int32 [B,4] (i, j local to the ligand, twice the order, 0).  `status` is None, or int32 [G] on a library that
    `aromatized` / `kekulized` returned: what `pd_aromaticity` said of each ligand (`AROMATICITY_STATUS`)."""

    def __init__(self, ligands: Sequence[Ligand]):
        self.ligands = list(ligands)
        G = self.n_ligands = len(self.ligands)
        if not 1 <= G <= MAX_LIGANDS:
            raise ValueError(f"LigandLibrary: {G} ligands; one launch takes 1 .. {MAX_LIGANDS}")
        if any(not isinstance(l, Ligand) for l in self.ligands):
            raise ValueError("LigandLibrary: every entry must be a Ligand")
        n = np.asarray([l.n_atoms for l in self.ligands], dtype=np.int64)
        self.atom_start = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        self.bond_start = np.concatenate([[0], np.cumsum([l.n_bonds for l in self.ligands])]).astype(np.int32)
        self.pair_start = np.concatenate([[0], np.cumsum(n * n)]).astype(np.int64)
        self.atoms = np.concatenate([np.stack([l.elements, l.charges, l.h_count, l.aromatic.astype(np.int64) | (l.chiral << 1)], axis=1)
                                     for l in self.ligands]).astype(np.int32)
        self.bonds = np.concatenate([np.concatenate([l.bonds, np.round(2.0 * l.bond_orders).astype(np.int64)[:, None],
                                                     np.zeros((l.n_bonds, 1), dtype=np.int64)], axis=1)
                                     for l in self.ligands]).astype(np.int32).reshape(-1, 4)
        self.n_atoms, self.n_bonds, self.n_pairs = int(self.atom_start[-1]), int(self.bond_start[-1]), int(self.pair_start[-1])
        self._tables = {}
        self.status = None

    @staticmethod
    def from_smiles(lines: Sequence[str]) -> "LigandLibrary":
        return LigandLibrary([Ligand.from_smiles(s) for s in lines])

    def tables(self, device) -> Dict[str, torch.Tensor]:
        names = ("atom_start", "bond_start", "pair_start", "atoms", "bonds")
        return ops.cached_upload(self._tables, device, lambda up: {k: up(getattr(self, k)) for k in names})

    def aromaticity(self, mode: str = "normalise", max_steps: int = 65536, device=None) -> Dict[str, torch.Tensor]:
        """ONE launch of `pd_aromaticity` for the whole library -> device tensors `atoms` int32 [N,4] and `bonds` int32 [B,4] in the
        layout of the library's own tables (bit 0 of the atom flags and twice the bond order rewritten; bond column 3: bit 0 in a
        perceived aromatic ring, bit 1 chosen double by the matching), `status` int32 [G] (`AROMATICITY_STATUS`; a ligand with a
        status other than 0 is copied through unchanged) and `counts` int32 [G,4] (aromatic rings found, aromatic atoms, aromatic
        bonds, matching steps).  mode: "kekulise", "perceive" (Kekule input) or "normalise" (kekulise, then perceive).  `max_steps`
        bounds the tries of the matching per ligand.  Nothing is read back."""
        if mode not in AROMATICITY_MODES:
            raise ValueError(f"LigandLibrary.aromaticity: mode {mode!r}; one of {sorted(AROMATICITY_MODES)}")
        if isinstance(max_steps, bool) or int(max_steps) != max_steps or not 0 <= int(max_steps) < 2 ** 31:
            raise ValueError(f"LigandLibrary.aromaticity: max_steps {max_steps!r}; an integer in 0 .. 2^31 - 1")
        device = _device(device)
        t = self.tables(device)
        G, N, B = self.n_ligands, self.n_atoms, self.n_bonds
        out = {"atoms": torch.empty(N, 4, device=device, dtype=torch.int32), "bonds": torch.empty(B, 4, device=device, dtype=torch.int32),
               "status": torch.empty(G, device=device, dtype=torch.int32), "counts": torch.empty(G, 4, device=device, dtype=torch.int32)}
        L_ = ops._lib.init()
        with torch.cuda.device(device):
            ops.check(L_.pd_aromaticity(ops.ptr(t["atom_start"]), ops.ptr(t["bond_start"]), ops.ptr(t["atoms"]),
                                        ops.ptr(t["bonds"]) if B else None, ops.ptr(out["atoms"]), ops.ptr(out["bonds"]) if B else None,
                                        ops.ptr(out["status"]), ops.ptr(out["counts"]), G, N, B, AROMATICITY_MODES[mode], int(max_steps),
                                        ops.stream()), "pd_aromaticity")
        return out

    def _rewritten(self, mode: str, device, errors: str, max_steps: int, what: str) -> "LigandLibrary":
        if errors not in ("raise", "keep"):
            raise ValueError(f"LigandLibrary.{what}: errors {errors!r}; 'raise' or 'keep'")
        out = self.aromaticity(mode, max_steps, device)
        atoms, bonds, status = (out[k].cpu().numpy() for k in ("atoms", "bonds", "status"))      # the one read-back
        ligands = []
        for g, lig in enumerate(self.ligands):
            if status[g]:
                if errors == "raise":
                    raise ValueError(f"LigandLibrary.{what}: ligand {g} ({lig.source or 'no source'}): status {int(status[g])}, "
                                     f"{AROMATICITY_STATUS.get(int(status[g]), 'unknown')}")
                ligands.append(lig)
                continue
            a0, a1, b0, b1 = (int(v) for v in (*self.atom_start[g:g + 2], *self.bond_start[g:g + 2]))
            orders = 0.5 * bonds[b0:b1, 2]
            double = {(min(i, j), max(i, j)) for (i, j), o in zip(lig.bonds.tolist(), orders.tolist()) if o == 2.0}
            stereo = [r for r in lig.bond_stereo.tolist() if (r[1], r[2]) in double]      # a row whose bond is no longer double is dropped
            if stereo:                                                                    # ... or no longer stereogenic in the new orders
                still = set(stereo_bonds_from_bonds(lig.n_atoms, lig.bonds, orders, lig.elements, lig.h_count))
                stereo = [r for r in stereo if (r[1], r[2]) in still]
            ligands.append(Ligand(lig.elements, lig.bonds, orders, lig.charges, lig.h_count, atoms[a0:a1, 3] & 1, lig.chiral,
                                  lig.chiral_order, lig.isotopes, source=lig.source, bond_stereo=stereo))
        lib = LigandLibrary(ligands)
        lib.status = _frozen(status, np.int32)
        return lib

    def aromatized(self, device=None, errors: str = "raise", max_steps: int = 65536) -> "LigandLibrary":
        """A new library of new ligands with their aromatic rings perceived (`aromaticity("normalise")`, one read-back): aromatic
        bonds of order 1.5 and the `aromatic` flags rewritten; `h_count`, `charges`, `chiral`, `chiral_order`, `isotopes` and `source`
        are kept.  errors="raise": a ligand without a Kekule structure (or whose matching ran out of `max_steps`) raises ValueError
        with its index, source and status; errors="keep": it is left unchanged and reported in `.status` of the result."""
        return self._rewritten("normalise", device, errors, max_steps, "aromatized")

    def kekulized(self, device=None, errors: str = "raise", max_steps: int = 65536) -> "LigandLibrary":
        """The same with every aromatic bond written single or double and every `aromatic` flag cleared (`aromaticity("kekulise")`)"""
        return self._rewritten("kekulise", device, errors, max_steps, "kekulized")

    def features(self, device=None, aromatize: bool = False) -> Dict[str, torch.Tensor]:
        """ONE launch for the whole library -> device tensors `atom_table` int8 [N,16] (`ATOM_COLUMNS`), `pair_table` int8 [P,8]
        (`PAIR_COLUMNS`), `ref_feat` fp32 [N,167], `rel_tok_feat` fp32 [P,42]; ligand g owns the atom rows atom_start[g] ..
        atom_start[g+1] and the pair rows pair_start[g] .. pair_start[g+1] (`split`).  `device=None` is the current CUDA device.  Nothing is read back.
        `aromatize=True`: `aromaticity("normalise")` first and the features of its tables - two launches, still no read-back - with
        `aromaticity_status` int32 [G] beside; a ligand whose status is not 0 has the features of its unchanged graph."""
        device = _device(device)
        t = self.tables(device)
        if aromatize:
            perceived = self.aromaticity("normalise", device=device)
            t = dict(t, atoms=perceived["atoms"], bonds=perceived["bonds"])
        N, P = self.n_atoms, self.n_pairs
        out = {"atom_table": torch.empty(N, ATOM_ROW, device=device, dtype=torch.int8),
               "pair_table": torch.empty(P, PAIR_ROW, device=device, dtype=torch.int8),
               "ref_feat": torch.empty(N, REF_FEAT, device=device, dtype=torch.float32),
               "rel_tok_feat": torch.empty(P, REL_TOK_FEAT, device=device, dtype=torch.float32)}
        L_ = ops._lib.init()
        with torch.cuda.device(device):
            ops.check(L_.pd_ligand_features(ops.ptr(t["atom_start"]), ops.ptr(t["bond_start"]), ops.ptr(t["pair_start"]), ops.ptr(t["atoms"]),
                                            ops.ptr(t["bonds"]) if self.n_bonds else None, ops.ptr(out["atom_table"]),
                                            ops.ptr(out["pair_table"]), ops.ptr(out["ref_feat"]), ops.ptr(out["rel_tok_feat"]),
                                            self.n_ligands, N, self.n_bonds, P, ops.stream()), "pd_ligand_features")
        if aromatize:
            out["aromaticity_status"] = perceived["status"]
        return out

    def fingerprints(self, radius: int = 2, n_bits: int = 2048, atom_invariants=None, aromatize: bool = False, device=None):
        """ONE launch of `pd_morgan_fingerprint` for the whole library -> an immutable `fingerprints.MorganFingerprint` (circular
        fingerprints after Rogers & Hahn 2010, the package's own definition; see that module): `bits` [G, n_bits/32], `ids` and `kept`
        [N, radius+1], `n_features` and `popcount` [G] on the device.  `radius` 0 .. 4, `n_bits` 512, 1024, 2048 or 4096;
        `atom_invariants` (one unsigned 32-bit value per atom of the library) replaces the radius-0 identifiers.  `aromatize=True`:
        `aromaticity("normalise")` first and the fingerprints of its tables - two launches, still no read-back - with
        `aromaticity_status` beside; without it a Kekule and an aromatic spelling of one molecule differ.  ValueError on the host,
        before any launch, for a bad `radius` or `n_bits` and for `atom_invariants` of another length."""
        from .fingerprints import morgan_fingerprint
        return morgan_fingerprint(self, radius, n_bits, atom_invariants, aromatize, device)

    def substructure(self, queries, aromatize: bool = False, max_steps: int = 65536, device=None):
        """Which ligands contain the queries, how often and on which atoms?  ONE launch of `pd_substructure_search` for the whole
        library x all queries -> an immutable `substructure.SubstructureMatches` on the device (see that module for the definition,
        the package's own): `n_embeddings`, `n_unique`, `status` [G, Q] and the bit rows `atom_hits`, `anchor_hits` [N, ceil(Q/32)].
        `queries`: a `substructure.SubstructureQueries`, or SMARTS strings (the subset of `smarts.parse_smarts`).  `max_steps` bounds
        the candidates tried per (query, ligand, anchor); status 2 where it ran out.  `aromatize=True`: `aromaticity("normalise")`
        first and the search of its tables; a `$()` in a query adds one launch for the inner patterns.  Nothing is read back.
        ValueError on the host, before any launch, for a query that is not read, too many queries and a bad `max_steps`."""
        from .substructure import substructure_search
        return substructure_search(self, queries, aromatize, max_steps, device)

    def canonical(self, aromatize: bool = False, max_steps: int = 65536, device=None):
        """Which ligands are the same molecule, and what is each one's one spelling?  ONE launch of `pd_canonical_form` for the whole
        library -> an immutable `canonical.CanonicalForm` on the device (see that module for the definition, the package's own):
        `labels`, `order`, `classes` [N], the certificate words `cert`, `key` [G, 2], `status`, `steps`, `leaves`, `canonical` [G];
        `first_of`, `unique()`, `same(i, j)`, `smiles()` and `renumbered()` from there.  `max_steps` bounds the refinements per ligand;
        status 2 where it ran out.  `aromatize=True`: `aromaticity("normalise")` first and the form of its tables.  Nothing is read
        back.  ValueError on the host, before any launch, for a bad `max_steps`."""
        from .canonical import canonical_form
        return canonical_form(self, aromatize, max_steps, device)

    def split(self, out: Dict[str, torch.Tensor], g: int) -> Dict[str, torch.Tensor]:
        """ligand g's part of a `features` result, as views under the reference's names (see `Ligand.features`)"""
        a0, a1, p0, p1 = (int(v) for v in (*self.atom_start[g:g + 2], *self.pair_start[g:g + 2]))
        L = a1 - a0
        r = {name: out["atom_table"][a0:a1, k] for k, name in enumerate(ATOM_COLUMNS)}
        r.update({name: out["pair_table"][p0:p1, k].view(L, L) for k, name in enumerate(PAIR_COLUMNS)})
        r["ref_feat"] = out["ref_feat"][a0:a1]
        r["rel_tok_feat"] = out["rel_tok_feat"][p0:p1].view(L, L, REL_TOK_FEAT)
        return r

    def __len__(self):
        return self.n_ligands

    def __repr__(self):
        return f"LigandLibrary(n_ligands={self.n_ligands}, n_atoms={self.n_atoms}, n_pairs={self.n_pairs})"
