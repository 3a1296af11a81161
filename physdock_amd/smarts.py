"""What is asked of a ligand library?  A reader for a stated subset of SMARTS on the host, without a dependency (`parse_smarts`): the
query language of `substructure.SubstructureQueries` and `LigandLibrary.substructure` (csrc/substructure.hip).  Like the SMILES
reader it is **the package's own reader, not RDKit's**; what a query means on a ligand is written down in tests/substructure_ref.py.

Atoms.  Outside brackets the organic subset `B C N O P S F Cl Br I` (the element, not aromatic), the aromatic `b c n o p s` and `*`,
`a`, `A`.  Inside brackets any element symbol of `pdbio.ELEMENTS` (upper case: that element and not aromatic; `b c n o p s se as`:
that element and aromatic; a two-letter symbol is read before a one-letter primitive, so `[Co]` is cobalt), `#n` (the element,
aromatic or not), `*`, `a`, `A`, `D<n>` (heavy degree), `H<n>` (`h_count`), `X<n>` (degree + `h_count`), `R` / `R0` (the atom has /
has not a bond that is no bridge), the charge as `+`, `-`, `+n`, `-n`, and `$(...)`.  `D`, `H` and `X` without a number mean 1.  An
atom is aromatic when it is written aromatic or has a bond of order 1.5 (`ref_is_aromatic` of `ligand.py`).  Hydrogens are implicit
in the ligands, so `[H]`, `[H+]` and `[#1]` are refused.  Logic: `!`, implicit `&`, `&`, `,`, `;` with the SMARTS precedence
(`[C,N;H1]` is (C or N) and H1, `[C,N&H1]` is C or (N and H1)).  Every query atom becomes a postfix program of at most `MAX_OPS` ops.

Bonds.  `-`, `=`, `#`, `:`, `~`, `@` (the bond is no bridge) with `!`, `&` (or nothing), `,`, `;`.  A ligand bond is in one of ten
states, `2 * order class + ring` with the order classes single, double, triple, aromatic (1.5), other of `bond_type`; an expression
is folded to the 10-bit mask of the states it allows.  No symbol: single or aromatic.

Structure.  Branches, ring closures `0` - `9` and `%nn` (a bond expression on both ends must be the same set).  1 .. `MAX_QUERY_ATOMS`
atoms, at most `MAX_QUERY_BONDS` bonds, one connected component.  The match order is the written order; every atom after the first
has an earlier neighbour and its `parent` is the lowest one.

`$(...)`, one level deep: true on an atom when the inner pattern has an embedding whose first atom is this atom.  The inner patterns
of a pattern are kept by text, in order of appearance and without repeats (`inner`).

Refused with a `ValueError` that names the character position (0-based): `.`, `/`, `\\`, `@` / `@@` on atoms, isotopes, atom classes
`:n`, `r<n>`, `R<n>` with n > 0, `x<n>`, `v<n>`, `h<n>`, `++` / `--`, a `$(` inside a `$(`, a component group `(...)` in front of the
first atom, two different bond sets on one ring closure, everything the limits exclude."""
from __future__ import annotations

from typing import List, Tuple

from .pdbio import ELEMENTS

__all__ = ["SmartsPattern", "parse_smarts", "MAX_QUERY_ATOMS", "MAX_QUERY_BONDS", "MAX_OPS", "MAX_INNER", "OPS", "BOND_ALL",
           "BOND_RING", "BOND_DEFAULT", "bond_state"]

MAX_QUERY_ATOMS, MAX_QUERY_BONDS, MAX_OPS, MAX_INNER = 32, 64, 32, 32
#: opcodes of the atom programs (PD_SUBSTRUCT_OP_* of include/physdock_hip.h); an op is `code | arg << 8`
OPS = {"true": 0, "z": 1, "aromatic": 2, "aliphatic": 3, "degree": 4, "h_count": 5, "connectivity": 6, "ring": 7, "charge": 8,
       "class": 9, "not": 10, "and": 11, "or": 12, "element_aliphatic": 13, "element_aromatic": 14}
#: bond states: 2 * (0 single, 1 double, 2 triple, 3 aromatic, 4 other) + (1 when the bond is no bridge)
BOND_ALL, BOND_RING = 0x3FF, 0x2AA
_BOND_PRIMITIVE = {"-": 0x003, "=": 0x00C, "#": 0x030, ":": 0x0C0, "~": BOND_ALL, "@": BOND_RING}
BOND_DEFAULT = _BOND_PRIMITIVE["-"] | _BOND_PRIMITIVE[":"]
_BOND_CHARS = set("-=#:~@!&,;")
_Z = {s: k + 1 for k, s in enumerate(ELEMENTS)}
_ORGANIC = ("Cl", "Br", "B", "C", "N", "O", "P", "S", "F", "I")
_AROMATIC = {"b": 5, "c": 6, "n": 7, "o": 8, "p": 15, "s": 16}
_AROMATIC_TWO = {"se": 34, "as": 33}


def bond_state(o2: int, in_ring: bool) -> int:
    """the state of a ligand bond of twice the order `o2`"""
    return 2 * {2: 0, 4: 1, 6: 2, 3: 3}.get(int(o2), 4) + int(bool(in_ring))


class SmartsPattern:
    """One parsed query, immutable: `text`, `n_atoms`, `programs` (per query atom a tuple of (opcode, argument); the argument of a
    "class" op is an index into `inner`), `bonds` ((lo, hi, mask) with lo < hi, in written order), `parents` (-1 for atom 0),
    `inner` (the texts of its `$()` patterns) and `inner_patterns` (those parsed)."""

    __slots__ = ("text", "n_atoms", "programs", "bonds", "parents", "inner", "inner_patterns")

    def __init__(self, text, programs, bonds, inner, inner_patterns):
        set_ = lambda k, v: object.__setattr__(self, k, v)
        set_("text", text); set_("n_atoms", len(programs)); set_("programs", tuple(tuple(p) for p in programs))
        set_("bonds", tuple(bonds)); set_("inner", tuple(inner)); set_("inner_patterns", tuple(inner_patterns))
        parents = [-1] * len(programs)
        for k in range(1, len(programs)):
            parents[k] = min(lo for lo, hi, _ in bonds if hi == k)
        set_("parents", tuple(parents))

    def __setattr__(self, name, value):
        raise AttributeError("SmartsPattern is immutable")

    def __repr__(self):
        return f"SmartsPattern({self.text!r}, n_atoms={self.n_atoms}, n_bonds={len(self.bonds)})"


class _Reader:
    def __init__(self, s: str, offset: int, inner: bool, whole: str):
        self.s, self.offset, self.is_inner, self.whole = s, offset, inner, whole
        self.inner: List[str] = []
        self.inner_patterns: List[SmartsPattern] = []

    def fail(self, k, why):
        raise ValueError(f"parse_smarts: position {k + self.offset}: {why}")

    # ---------------------------------------------------------------- numbers
    def number(self, k) -> Tuple[int, int]:
        """(value or None, the position behind the digits)"""
        d = k
        while d < len(self.s) and self.s[d].isdigit():
            d += 1
        if d == k:
            return None, k
        if d - k > 3 or int(self.s[k:d]) > 255:
            self.fail(k, f"the number {self.s[k:d]} is beyond 255")
        return int(self.s[k:d]), d

    # ---------------------------------------------------------------- atom expressions
    def atom_primitive(self, k, first):
        """one primitive inside a bracket -> (ops, next position); `first`: nothing but `[` stands in front of it"""
        s = self.s
        ch, two = s[k], s[k:k + 2]
        if len(two) == 2 and two[0].isupper() and two[1].islower() and two in _Z:
            return [(OPS["element_aliphatic"], _Z[two])], k + 2
        if two in _AROMATIC_TWO:
            return [(OPS["element_aromatic"], _AROMATIC_TWO[two])], k + 2
        if ch == "*":
            return [(OPS["true"], 0)], k + 1
        if ch == "a":
            return [(OPS["aromatic"], 0)], k + 1
        if ch == "A":
            return [(OPS["aliphatic"], 0)], k + 1
        if ch == "#":
            n, q = self.number(k + 1)
            if n is None or n < 1 or n > len(ELEMENTS):
                self.fail(k, f"# needs an atomic number in 1 .. {len(ELEMENTS)}")
            if n == 1:
                self.fail(k, "an explicit hydrogen: the hydrogens of a ligand are implicit (use H<n>)")
            return [(OPS["z"], n)], q
        if ch in "DHX":
            if ch == "H" and first and s[k + 1:k + 2] in ("]", "+", "-"):
                self.fail(k, "an explicit hydrogen: the hydrogens of a ligand are implicit (use H<n>)")
            n, q = self.number(k + 1)
            return [(OPS[{"D": "degree", "H": "h_count", "X": "connectivity"}[ch]], 1 if n is None else n)], q
        if ch == "R":
            n, q = self.number(k + 1)
            if n is None:
                return [(OPS["ring"], 0)], q
            if n > 0:
                self.fail(k, "R<n> with n > 0 (a ring count) is not read; R and R0 are")
            return [(OPS["ring"], 0), (OPS["not"], 0)], q
        if ch in "+-":
            if s[k + 1:k + 2] == ch:
                self.fail(k + 1, f"{ch}{ch}: write the charge as {ch}2")
            n, q = self.number(k + 1)
            n = 1 if n is None else n
            if n > 127:
                self.fail(k, "a charge beyond +-127")
            return [(OPS["charge"], (n if ch == "+" else -n) + 128)], q
        if ch == "$":
            return self.recursion(k)
        if ch in _AROMATIC:
            return [(OPS["element_aromatic"], _AROMATIC[ch])], k + 1
        if ch in _Z:
            return [(OPS["element_aliphatic"], _Z[ch])], k + 1
        if ch == "@":
            self.fail(k, "@ on an atom: stereo is not read in queries")
        if ch.isdigit():
            self.fail(k, "an isotope is not read")
        if ch == ":":
            self.fail(k, "an atom class :n is not read")
        if ch in "rxvh":
            self.fail(k, f"{ch}<n> is not read")
        self.fail(k, f"{ch!r} is not read inside a bracket atom")

    def recursion(self, k):
        s = self.s
        if s[k + 1:k + 2] != "(":
            self.fail(k, "$ needs a pattern in parentheses")
        if self.is_inner:
            self.fail(k, "a $( inside a $(: one level of recursion is read")
        depth, q = 0, k + 1
        while q < len(s):
            if s[q] == "(":
                depth += 1
            elif s[q] == ")":
                depth -= 1
                if depth == 0:
                    break
            q += 1
        if q >= len(s):
            self.fail(k, "a $( that is not closed")
        text = s[k + 2:q]
        if text not in self.inner:
            pattern = _parse(text, self.offset + k + 2, True, text)      # (raises with positions in the outer text)
            if len(self.inner) == MAX_INNER:
                self.fail(k, f"more than {MAX_INNER} distinct $() patterns")
            self.inner.append(text)
            self.inner_patterns.append(pattern)
        return [(OPS["class"], self.inner.index(text))], q + 1

    def atom_not(self, k, start):
        if k < len(self.s) and self.s[k] == "!":
            ops, q = self.atom_not(k + 1, start)
            return ops + [(OPS["not"], 0)], q
        if k >= len(self.s):
            self.fail(start, "a bracket atom that is not closed")
        if self.s[k] in "],;&":
            self.fail(k, "an atom primitive is missing")
        return self.atom_primitive(k, k == start + 1)

    def atom_and(self, k, start):
        ops, k = self.atom_not(k, start)
        while k < len(self.s) and self.s[k] not in ",;]":
            if self.s[k] == "&":
                k += 1
            more, k = self.atom_not(k, start)
            ops += more + [(OPS["and"], 0)]
        return ops, k

    def atom_or(self, k, start):
        ops, k = self.atom_and(k, start)
        while k < len(self.s) and self.s[k] == ",":
            more, k = self.atom_and(k + 1, start)
            ops += more + [(OPS["or"], 0)]
        return ops, k

    def bracket(self, start):
        """the bracket atom at `start` -> (ops, the position behind `]`)"""
        ops, k = self.atom_or(start + 1, start)
        while k < len(self.s) and self.s[k] == ";":
            more, k = self.atom_or(k + 1, start)
            ops += more + [(OPS["and"], 0)]
        if k >= len(self.s) or self.s[k] != "]":
            self.fail(start, "a bracket atom that is not closed")
        if len(ops) > MAX_OPS:
            self.fail(start, f"an atom expression of {len(ops)} ops; up to {MAX_OPS} are taken")
        return ops, k + 1

    # ---------------------------------------------------------------- bond expressions
    def bond_not(self, k):
        if k < len(self.s) and self.s[k] == "!":
            m, q = self.bond_not(k + 1)
            return BOND_ALL & ~m, q
        if k >= len(self.s) or self.s[k] not in _BOND_PRIMITIVE:
            self.fail(min(k, len(self.s) - 1), "a bond primitive is missing")
        return _BOND_PRIMITIVE[self.s[k]], k + 1

    def bond_and(self, k):
        m, k = self.bond_not(k)
        while k < len(self.s) and (self.s[k] in _BOND_PRIMITIVE or self.s[k] in "!&"):
            if self.s[k] == "&":
                k += 1
            more, k = self.bond_not(k)
            m &= more
        return m, k

    def bond_or(self, k):
        m, k = self.bond_and(k)
        while k < len(self.s) and self.s[k] == ",":
            more, k = self.bond_and(k + 1)
            m |= more
        return m, k

    def bond(self, k):
        m, k = self.bond_or(k)
        while k < len(self.s) and self.s[k] == ";":
            more, k = self.bond_or(k + 1)
            m &= more
        return m, k


def _parse(s: str, offset: int, inner: bool, whole: str) -> SmartsPattern:
    r = _Reader(s, offset, inner, whole)
    fail = r.fail
    if not s:
        fail(0, "an empty pattern")
    programs: List[list] = []
    bonds: List[tuple] = []
    rings = {}                                           # open digits: number -> (atom, mask or None, position)
    stack: List[tuple] = []
    prev, pending, pending_at = -1, None, -1
    k, n = 0, len(s)

    def add_bond(i, j, mask, at):
        if i == j:
            fail(at, "a ring closure bonds an atom to itself")
        lo, hi = min(i, j), max(i, j)
        if any((lo, hi) == b[:2] for b in bonds):
            fail(at, f"a second bond between the query atoms {lo} and {hi}")
        if len(bonds) == MAX_QUERY_BONDS:
            fail(at, f"more than {MAX_QUERY_BONDS} bonds")
        bonds.append((lo, hi, BOND_DEFAULT if mask is None else mask))

    def add_atom(ops, at):
        nonlocal prev, pending
        if len(programs) == MAX_QUERY_ATOMS:
            fail(at, f"more than {MAX_QUERY_ATOMS} atoms")
        programs.append(ops)
        a = len(programs) - 1
        if prev >= 0:
            add_bond(prev, a, pending, at)
        prev, pending = a, None

    while k < n:
        ch = s[k]
        if ch == "[":
            ops, q = r.bracket(k)
            add_atom(ops, k)
            k = q
        elif ch in "/\\":
            fail(k, "a directional bond: stereo is not read in queries")
        elif ch in _BOND_CHARS:
            if pending is not None:
                fail(k, "two bond expressions in a row")
            if prev < 0:
                fail(k, "a bond expression with no atom in front of it")
            pending_at = k
            pending, k = r.bond(k)
        elif ch == "(":
            if prev < 0:
                fail(k, "a component group (...) in front of the first atom is not read")
            if pending is not None:
                fail(k, "a bond expression in front of a branch")
            stack.append((prev, k))
            k += 1
        elif ch == ")":
            if not stack:
                fail(k, "a branch closes that was never opened")
            if pending is not None:
                fail(pending_at, "a bond expression with no atom behind it")
            if prev == stack[-1][0]:
                fail(stack[-1][1], "an empty branch")
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
                a, mask, _ = rings.pop(num)
                if mask is not None and pending is not None and mask != pending:
                    fail(at, f"ring closure {num} is written with two different bond expressions")
                add_bond(a, prev, pending if mask is None else mask, at)
            else:
                rings[num] = (prev, pending, at)
            pending = None
        elif ch == ".":
            fail(k, "a dot: a query is one connected pattern")
        else:
            sym = next((o for o in _ORGANIC if s.startswith(o, k)), None)
            if sym is not None:
                add_atom([(OPS["element_aliphatic"], _Z[sym])], k)
                k += len(sym)
            elif ch in _AROMATIC:
                add_atom([(OPS["element_aromatic"], _AROMATIC[ch])], k)
                k += 1
            elif ch in "*aA":
                add_atom([(OPS[{"*": "true", "a": "aromatic", "A": "aliphatic"}[ch]], 0)], k)
                k += 1
            else:
                fail(k, f"the symbol {ch!r} is not read")
    if pending is not None:
        fail(pending_at, "a bond expression with no atom behind it")
    if stack:
        fail(stack[-1][1], "a branch that is not closed")
    if rings:
        num = min(rings, key=lambda x: rings[x][2])
        fail(rings[num][2], f"ring closure {num} is not closed")
    return SmartsPattern(whole, programs, bonds, r.inner, r.inner_patterns)


def parse_smarts(text: str) -> SmartsPattern:
    """One query -> a `SmartsPattern`.  Leading and trailing white space is dropped."""
    if not isinstance(text, str):
        raise ValueError(f"parse_smarts: a str expected, got {type(text).__name__}")
    lead = len(text) - len(text.lstrip())
    s = text.strip()
    if not s:
        raise ValueError("parse_smarts: position 0: an empty pattern")
    return _parse(s, lead, False, s)
