"""Which ligands of a library contain a given group, and on which atoms?  `LigandLibrary.substructure(queries)` answers it for G
ligands x Q queries in one launch (csrc/substructure.hip): reactive-group and PAINS-style filters before docking, a series picked by
its scaffold, the warhead atoms to restrain.  It is the exact half of 2-D screening next to the similarity search of
`fingerprints.MorganFingerprint`.  Nothing in the reference does this, and RDKit is not a dependency: **the definition is the
package's own, not RDKit's** - tests/substructure_ref.py in Python integers; `smarts.parse_smarts` reads the queries from a stated
subset of SMARTS (that module lists it).

**The definition.**  An embedding maps the query atoms injectively to the atoms of one ligand so that every atom expression is true
and every query bond lies on a ligand bond of an allowed state (order class x ring); more ligand bonds may join the image (a
subgraph monomorphism).  The search is depth-first in the written order of the query atoms: atom 0 on every atom that passes its
expression, ascending (an *anchor*); atom k on the free neighbours of the image of its parent that pass expression k, ascending.
One candidate is one *step*, every (query, ligand, anchor) has `max_steps` of them; an anchor that has spent them when a candidate
is due stops with what it found and the pair gets status 2.  The order is fixed, so the kernel's result equals the restatement bit
for bit, exhausted budgets included, and is the same from launch to launch and anywhere in a library.

    n_embeddings   the embeddings found, saturating at 2^31 - 1
    n_unique       those that are the lexicographically smallest embedding onto their own atom set (RDKit's `uniquify` goes by atom
                   set too): `C~C~C` on cyclopropane has 6 embeddings and 1 unique one.  Decided by the same search restricted to the
                   embedding's own atoms, without a budget.  With status 2 it counts among the embeddings found.
    status         0 done, 2 a budget ran out (1 is reserved: not written)
    atom_hits      bit rows [N, ceil(Q / 32)]: the atom lies in some embedding found;  anchor_hits: it is the image of query atom 0

`$(...)` environments are searched first, in one launch of their own for all distinct inner patterns of the set (at most 32, by
text); its `anchor_hits` are the main launch's `atom_classes` on the device.  `inner_status` holds that launch's status [G, Qi]: an
inner search that ran out of steps (status 2) leaves its class bit clear on the anchors it did not finish.

`pharmacophore_invariants` marks donor, acceptor, aromatic, halogen, basic and acidic atoms by a short table of SMARTS
(`PHARMACOPHORE_SMARTS`) and feeds `LigandLibrary.fingerprints(atom_invariants=...)` without a read-back: an FCFP-like variant.

**Caveats.**  The package's own subset and semantics: no stereo in queries, no ring-size or ring-count primitives, one level of
recursion, connected queries only.  "Ring" means "no bridge" and "aromatic" is what is written (or perceived with `aromatize=True`).
Limits: 32 atoms, 64 bonds and 32 ops per atom in a query, 1024 queries and 65535 ligands per launch, 128 atoms per ligand, 256
matches per ligand.  The uniqueness test has no budget: on ordinary molecular graphs it visits a few tuples per embedding."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .smarts import MAX_INNER, OPS, SmartsPattern, parse_smarts

__all__ = ["SmartsPattern", "parse_smarts", "SubstructureQueries", "SubstructureMatches", "substructure_search",
           "pharmacophore_invariants", "PHARMACOPHORE_SMARTS", "MAX_QUERIES", "MAX_MATCHES", "STATUS"]

MAX_QUERIES, MAX_MATCHES = 1024, 256
STATUS = {0: "done", 1: "not written", 2: "a search ran out of steps"}
#: bit c of `pharmacophore_invariants` is pattern c.  The package's own table: a donor is an N or O with a hydrogen; an acceptor an
#: O, or an N without a positive charge that is no amide / sulfonamide / aniline N and no three-connected aromatic n; basic is a
#: positive N or a three-connected aliphatic amine N (no amide, aniline or sulfonamide); acidic is the OH or O- of a C, P or S oxo acid
PHARMACOPHORE_SMARTS = (
    ("donor", "[#7,#8;!H0]"),
    ("acceptor", "[#8,#7;!+;!$([#7;X3]-[#6,#16]=[#8,#16]);!$([N;X3]-a);!$([n;X3])]"),
    ("aromatic", "a"),
    ("halogen", "[F,Cl,Br,I]"),
    ("basic", "[#7;+,N&X3&!$(N-[#6,#16]=[#8,#16])&!$(N-a)]"),
    ("acidic", "[O;H1,-;$(O-[#6,#15,#16]=O)]"),
)


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


class SubstructureQueries:
    """Q queries (SMARTS strings or `SmartsPattern`s) packed for `pd_substructure_search`, immutable; the tables are uploaded once
    per device.  `patterns`, `n_queries`, `inner` (the `SubstructureQueries` of the distinct `$()` patterns of the set, or None)."""

    __slots__ = ("patterns", "n_queries", "inner", "_packed", "_tables")

    def __init__(self, patterns: Sequence):
        if isinstance(patterns, (str, SmartsPattern)):
            patterns = [patterns]
        try:
            patterns = list(patterns)
        except TypeError:
            raise ValueError(f"SubstructureQueries: a sequence of SMARTS strings expected, got {type(patterns).__name__}") from None
        if not 1 <= len(patterns) <= MAX_QUERIES:
            raise ValueError(f"SubstructureQueries: {len(patterns)} queries; one launch takes 1 .. {MAX_QUERIES}")
        parsed = []
        for k, p in enumerate(patterns):
            if isinstance(p, str):
                try:
                    p = parse_smarts(p)
                except ValueError as e:
                    raise ValueError(f"SubstructureQueries: query {k}: {e}") from None
            if not isinstance(p, SmartsPattern):
                raise ValueError(f"SubstructureQueries: query {k} is a {type(p).__name__}; a SMARTS string or a SmartsPattern")
            parsed.append(p)
        texts: List[str] = []
        inner: List[SmartsPattern] = []
        for p in parsed:
            for text, pat in zip(p.inner, p.inner_patterns):
                if text not in texts:
                    texts.append(text); inner.append(pat)
        if len(texts) > MAX_INNER:
            raise ValueError(f"SubstructureQueries: {len(texts)} distinct $() patterns in the set; up to {MAX_INNER} are taken")
        q_atom_start, q_op_start, q_ops, q_bond_start, q_bonds = [0], [0], [], [0], []
        for p in parsed:
            for program in p.programs:
                for code, arg in program:
                    if code == OPS["class"]:
                        arg = texts.index(p.inner[arg])
                    q_ops.append(code | arg << 8)
                q_op_start.append(len(q_ops))
            q_atom_start.append(q_atom_start[-1] + p.n_atoms)
            q_bonds += [(lo, hi, mask, 0) for lo, hi, mask in sorted(p.bonds, key=lambda b: b[1])]      # (stable: by the later atom)
            q_bond_start.append(len(q_bonds))
        packed = {"q_atom_start": np.asarray(q_atom_start, dtype=np.int32), "q_op_start": np.asarray(q_op_start, dtype=np.int32),
                  "q_ops": np.asarray(q_ops, dtype=np.int32), "q_bond_start": np.asarray(q_bond_start, dtype=np.int32),
                  "q_bonds": np.asarray(q_bonds, dtype=np.int32).reshape(-1, 4)}
        set_ = lambda k, v: object.__setattr__(self, k, v)
        set_("patterns", tuple(parsed)); set_("n_queries", len(parsed)); set_("_packed", packed); set_("_tables", {})
        set_("inner", SubstructureQueries(inner) if inner else None)

    def __setattr__(self, name, value):
        raise AttributeError("SubstructureQueries is immutable")

    def __len__(self):
        return self.n_queries

    def __repr__(self):
        return f"SubstructureQueries(n_queries={self.n_queries}, n_inner={len(self.inner) if self.inner else 0})"

    def tables(self, device) -> Dict[str, torch.Tensor]:
        return ops.cached_upload(self._tables, device, lambda up: {k: up(v) for k, v in self._packed.items()})

    def _args(self, device):
        """the five table pointers and the four sizes, in the order of the C interface"""
        t, p = self.tables(device), self._packed
        ptrs = [ops.ptr(t["q_atom_start"]), ops.ptr(t["q_op_start"]), ops.ptr(t["q_ops"]), ops.ptr(t["q_bond_start"]),
                ops.ptr(t["q_bonds"]) if len(p["q_bonds"]) else None]
        return ptrs, [self.n_queries, int(p["q_atom_start"][-1]), len(p["q_ops"]), len(p["q_bonds"])]


def _queries(queries, what) -> SubstructureQueries:
    if isinstance(queries, SubstructureQueries):
        return queries
    try:
        return SubstructureQueries(queries)
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from None


def _launch_search(t, library, queries: SubstructureQueries, atom_classes, max_steps, device):
    G, N, B, Q = library.n_ligands, library.n_atoms, library.n_bonds, queries.n_queries
    QW = (Q + 31) // 32
    new = lambda *shape: torch.empty(shape, device=device, dtype=torch.int32)
    out = {"n_embeddings": new(G, Q), "n_unique": new(G, Q), "status": new(G, Q), "atom_hits": new(N, QW), "anchor_hits": new(N, QW)}
    ptrs, sizes = queries._args(device)
    L_ = ops._lib.init()
    with torch.cuda.device(device):
        ops.check(L_.pd_substructure_search(ops.ptr(t["atom_start"]), ops.ptr(t["bond_start"]), ops.ptr(t["atoms"]),
                                            ops.ptr(t["bonds"]) if B else None, *ptrs, ops.ptr(atom_classes),
                                            ops.ptr(out["n_embeddings"]), ops.ptr(out["n_unique"]), ops.ptr(out["status"]),
                                            ops.ptr(out["atom_hits"]), ops.ptr(out["anchor_hits"]), G, N, B, *sizes, max_steps,
                                            ops.stream()), "pd_substructure_search")
    return out


def substructure_search(library, queries, aromatize=False, max_steps=65536, device=None) -> "SubstructureMatches":
    """`LigandLibrary.substructure`: ONE launch of `pd_substructure_search` for the whole library and all queries; one more in front
    with `aromatize=True` (`pd_aromaticity`, mode "normalise", whose tables are searched, as `fingerprints(aromatize=True)` does) and
    one more when a query holds a `$()` (the inner patterns; their `anchor_hits` become `atom_classes` on the device).  Nothing is
    read back.  Every check is made on the host before the first launch."""
    from .ligand import _device
    what = "LigandLibrary.substructure"
    queries = _queries(queries, what)
    if not _is_int(max_steps) or not 0 <= int(max_steps) < 2 ** 31:
        raise ValueError(f"{what}: max_steps {max_steps!r}; an integer in 0 .. 2^31 - 1")
    if not isinstance(aromatize, (bool, np.bool_)):
        raise ValueError(f"{what}: aromatize {aromatize!r}; True or False")
    max_steps = int(max_steps)
    device = _device(device)
    t = library.tables(device)
    aromaticity_status = None
    if aromatize:
        perceived = library.aromaticity("normalise", device=device)
        t = dict(t, atoms=perceived["atoms"], bonds=perceived["bonds"])
        aromaticity_status = perceived["status"]
    atom_classes, inner_status = None, None
    if queries.inner is not None:
        found = _launch_search(t, library, queries.inner, None, max_steps, device)
        atom_classes, inner_status = found["anchor_hits"].view(-1), found["status"]      # (at most 32 inner patterns: one word)
    out = _launch_search(t, library, queries, atom_classes, max_steps, device)
    return SubstructureMatches(library, queries, t, atom_classes, max_steps, device, out, aromaticity_status, inner_status)


class SubstructureMatches:
    """Immutable result of `LigandLibrary.substructure`, all on the device: `n_embeddings`, `n_unique`, `status` int32 [G, Q],
    `atom_hits`, `anchor_hits` int32 [N, ceil(Q / 32)] (the uint32 words; bit q % 32 of word q // 32), `has` = `n_embeddings > 0`,
    `aromaticity_status` int32 [G] with `aromatize=True` and `inner_status` int32 [G, Qi] with a `$()`, else None.  Every method
    returns device tensors and reads nothing back, except `select`."""

    __slots__ = ("library", "queries", "n_embeddings", "n_unique", "status", "atom_hits", "anchor_hits", "aromaticity_status",
                 "inner_status", "max_steps", "_t", "_classes", "_device")

    def __init__(self, library, queries, t, atom_classes, max_steps, device, out, aromaticity_status, inner_status):
        set_ = lambda k, v: object.__setattr__(self, k, v)
        set_("library", library); set_("queries", queries); set_("_t", t); set_("_classes", atom_classes); set_("max_steps", max_steps)
        set_("_device", device); set_("aromaticity_status", aromaticity_status); set_("inner_status", inner_status)
        for k, v in out.items():
            set_(k, v)

    def __setattr__(self, name, value):
        raise AttributeError("SubstructureMatches is immutable")

    def __repr__(self):
        return f"SubstructureMatches(n_ligands={self.library.n_ligands}, n_queries={self.queries.n_queries})"

    @property
    def has(self) -> torch.Tensor:
        """bool [G, Q]: the ligand contains the query"""
        return self.n_embeddings > 0

    def _query(self, q, what) -> int:
        if not _is_int(q) or not 0 <= int(q) < self.queries.n_queries:
            raise ValueError(f"SubstructureMatches.{what}: query {q!r}; an integer in 0 .. {self.queries.n_queries - 1}")
        return int(q)

    def atoms(self, q: int) -> torch.Tensor:
        """bool [N]: the atoms of the library that lie in some embedding of query q (`library.atom_start` splits them by ligand)"""
        q = self._query(q, "atoms")
        return ((self.atom_hits[:, q >> 5] >> (q & 31)) & 1).bool()

    def anchors(self, q: int) -> torch.Tensor:
        """bool [N]: the atoms that are the image of the first atom of query q"""
        q = self._query(q, "anchors")
        return ((self.anchor_hits[:, q >> 5] >> (q & 31)) & 1).bool()

    def matches(self, q: int, max_matches: int = 16, unique: bool = True) -> Dict[str, torch.Tensor]:
        """the first `max_matches` (1 .. 256) embeddings of query q in every ligand, in the order of the search - with `unique`
        only those that are the smallest onto their atom set -> `atoms` int32 [G, max_matches, nq] (atom indices local to the
        ligand, in the written order of the query atoms, -1 beyond the last row) and `n_written` int32 [G].  One launch of
        `pd_substructure_matches` on the tables and the budget of the search."""
        q = self._query(q, "matches")
        if not _is_int(max_matches) or not 1 <= int(max_matches) <= MAX_MATCHES:
            raise ValueError(f"SubstructureMatches.matches: max_matches {max_matches!r}; an integer in 1 .. {MAX_MATCHES}")
        if not isinstance(unique, (bool, np.bool_)):
            raise ValueError(f"SubstructureMatches.matches: unique {unique!r}; True or False")
        lib, dev, M, nq = self.library, self._device, int(max_matches), self.queries.patterns[q].n_atoms
        out = {"atoms": torch.empty(lib.n_ligands, M, nq, device=dev, dtype=torch.int32),
               "n_written": torch.empty(lib.n_ligands, device=dev, dtype=torch.int32)}
        ptrs, sizes = self.queries._args(dev)
        t = self._t
        L_ = ops._lib.init()
        with torch.cuda.device(dev):
            ops.check(L_.pd_substructure_matches(ops.ptr(t["atom_start"]), ops.ptr(t["bond_start"]), ops.ptr(t["atoms"]),
                                                 ops.ptr(t["bonds"]) if lib.n_bonds else None, *ptrs, ops.ptr(self._classes),
                                                 ops.ptr(out["atoms"]), ops.ptr(out["n_written"]), lib.n_ligands, lib.n_atoms,
                                                 lib.n_bonds, *sizes, q, nq, M, int(bool(unique)), self.max_steps, ops.stream()),
                      "pd_substructure_matches")
        return out

    def select(self, q: int) -> List[int]:
        """the indices of the ligands that contain query q, ascending: THE ONE READ-BACK of this class"""
        q = self._query(q, "select")
        return torch.nonzero(self.n_embeddings[:, q] > 0).flatten().tolist()


def pharmacophore_invariants(library, aromatize: bool = False, device=None) -> torch.Tensor:
    """int32 [N] on the device: bit c of an atom's value is set when pattern c of `PHARMACOPHORE_SMARTS` anchors there -

        0 donor     [#7,#8;!H0]
        1 acceptor  [#8,#7;!+;!$([#7;X3]-[#6,#16]=[#8,#16]);!$([N;X3]-a);!$([n;X3])]
        2 aromatic  a
        3 halogen   [F,Cl,Br,I]
        4 basic     [#7;+,N&X3&!$(N-[#6,#16]=[#8,#16])&!$(N-a)]
        5 acidic    [O;H1,-;$(O-[#6,#15,#16]=O)]

    the package's own table, not RDKit's feature definitions.  Two launches (the `$()` patterns, then the six classes; one more
    with `aromatize=True`), nothing read back: `library.fingerprints(atom_invariants=pharmacophore_invariants(library))` is an
    FCFP-like fingerprint made on the device from end to end."""
    found = substructure_search(library, _PHARMACOPHORE(), aromatize, 65536, device)
    return found.anchor_hits.view(-1)


_PHARMACOPHORE_QUERIES: List[Optional[SubstructureQueries]] = [None]


def _PHARMACOPHORE() -> SubstructureQueries:
    if _PHARMACOPHORE_QUERIES[0] is None:
        _PHARMACOPHORE_QUERIES[0] = SubstructureQueries([s for _, s in PHARMACOPHORE_SMARTS])
    return _PHARMACOPHORE_QUERIES[0]
