"""SD file records of ligand poses, formatted on the device - the second kind of file the reference's driver delivers
(`ligand_rank_k.sdf`: `Chem.MolToMolBlock(ref_mol_copy, includeStereo=True)` after `SetAtomPosition`, redocking.py:345-354 and :425-444;
`pdbio.PdbTemplate` writes the first kind).  `SdfTemplate` builds everything that does not depend on the pose ONCE per ligand on the host
- the molblock with blank coordinates, a per-byte map that says "copy" or "digit p of component c of atom a", the data-item headers -
and `pd_sdf_format` (csrc/sdf.hip) writes the records of all poses into one contiguous buffer that is a valid SD file as it stands:
bond table in -> poses -> SD file out, without RDKit.  `parse_sdf` is the reader of the same format.

The format is the CTfile V2000 specification and THIS PACKAGE'S definition (tests/sdf_ref.py writes it down); parity with RDKit's
`MolToMolBlock` is NOT pinned: RDKit's program / time-stamp line and its wedge flags differ by design, the coordinate columns are the
same `%10.4f`.  One record:

    {title}                                              line 1, <= 80 characters, no control characters
      {program:<8.8}{'':10}3D                            line 2, program = "physdock"; no time stamp, so the text is reproducible
    {comment}                                            line 3, empty by default
    {na:3d}{nb:3d}  0  0  0  0  0  0  0  0999 V2000
    {x:10.4f}{y:10.4f}{z:10.4f} {symbol:<3} 0  0  0  0  0  0  0  0  0  0  0  0      one per atom, 69 columns
    {i+1:3d}{j+1:3d}{type:3d}  0                                                   one per bond: type 1, 2, 3, and 4 for order 1.5
    M  CHG{n:3d}{atom:4d}{charge:4d}...                                            non-zero formal charges, 8 per line, atoms ascending
    M  END
    >  <{name}>                                          the data items of the pose in the order given
    {value}
    (empty line)
    $$$$

A float32 value with d decimals (0 <= d <= 8, per item) is f"{float(v):.{d}f}" - "-0.0000", "nan", "inf" and "-inf" included -, an int32
value is str(v); nothing is padded, so records differ in length and `offsets` says where each starts.  Names match
`[A-Za-z_][A-Za-z0-9_.]*` and hold at most 64 characters.  Numbers are exact (|v| 10^d is exact in float64, rint of it is the
round-half-even of the correctly rounded decimal conversion).  A coordinate that is not finite or does not fit its 10 columns (after
rounding above 99999.9999 or below -9999.9999) and a value with |v| 10^d >= 1e15 make `format` raise.

**Caveats.**  Not RDKit's bytes.  Order 1.5 is written as bond type 4 (aromatic), which RDKit and Open Babel read; input that is
already Kekule passes through.  No stereo flags: the 3-D coordinates carry the stereo.  Charges only when given.  Limits: 1 .. 999
atoms, at most 999 bonds, 32 data items, 65535 records per call; every violation raises on the host before anything is launched.
Out of scope: V3000, MOL2, Kekulisation, `from_rdkit`, receptor output.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .pdbio import ELEMENTS

__all__ = ["SdfTemplate", "parse_sdf", "BOND_TYPES", "MAX_ATOMS", "MAX_BONDS", "MAX_ITEMS", "MAX_RECORDS", "MAX_NAME", "MAX_DECIMALS",
           "DEFAULT_DECIMALS"]

#: bond order -> V2000 bond type
BOND_TYPES = {1.0: 1, 2.0: 2, 3.0: 3, 1.5: 4}
MAX_ATOMS, MAX_BONDS, MAX_ITEMS, MAX_RECORDS, MAX_NAME, MAX_DECIMALS, DEFAULT_DECIMALS = 999, 999, 32, 65535, 64, 8, 4
#: the longest text of a value: sign, 16 digits and the point for a float32 (|v| 10^d < 1e15 rounds to at most 16 digits); -2147483648
FLOAT_TEXT_MAX, INT_TEXT_MAX = 18, 11
ATOM_LINE = 70                                                            # 69 columns and the newline
_NAME = re.compile(r"[A-Za-z_][A-Za-z0-9_.]*\Z")
_COUNTS_TAIL = "  0  0  0  0  0  0  0  0999 V2000"
_ATOM_TAIL = " 0" + "  0" * 11
_SYMBOLS = {s.upper(): s for s in ELEMENTS}
_OLD_CHARGES = {0: 0, 1: 3, 2: 2, 3: 1, 4: 0, 5: -1, 6: -2, 7: -3}        # the ccc field of an atom line (4: doublet radical)


def _symbols(elements) -> List[str]:
    """element symbols from atomic numbers or symbols"""
    seq = elements.detach().cpu().tolist() if isinstance(elements, torch.Tensor) else list(np.asarray(elements).reshape(-1).tolist())
    out = []
    for e in seq:
        if isinstance(e, str):
            s = _SYMBOLS.get(e.strip().upper())
        else:
            s = ELEMENTS[int(e) - 1] if 1 <= int(e) <= len(ELEMENTS) else None
        if s is None:
            raise ValueError(f"SdfTemplate: {e!r} is neither an atomic number 1 .. {len(ELEMENTS)} nor an element symbol")
        out.append(s)
    return out


def _line(text, what, limit=80) -> str:
    text = str(text)
    if len(text) > limit or any(not 32 <= ord(c) < 127 for c in text):
        raise ValueError(f"SdfTemplate: the {what} holds at most {limit} printable ASCII characters, got {text!r}")
    return text


def _ints(a) -> np.ndarray:
    return np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.int64).reshape(-1)


class SdfTemplate:
    """The pose-independent part of a ligand's SD file records.  Host tables: `symbols` (list of str, na), `atom` int32 [na] (the index
    into a pose of every atom of the record), `n_pose_atoms` (the atoms of the poses `format` takes), `bonds` int32 [nb,2] (indices into
    the record's atoms), `bond_orders` float64 [nb], `bond_types` int32 [nb], `charges` int32 [na], `title`, `comment`, `program`;
    built from them `molblock` (str, coordinates blank), `tmpl` uint8 [M], `map` int32 [M] (-1: copy the byte, else 30 s + col: column
    col of atom s) and `atoms_at` (the offset of the first atom line).  `hydrogens`: the `Hydrogens` object `with_hydrogens` took."""

    def __init__(self, symbols, atom, n_pose_atoms, bonds=(), bond_orders=None, charges=None, title="", comment="", program="physdock",
                 device=None):
        self.symbols = _symbols(symbols)
        na = len(self.symbols)
        self.atom = _ints(atom).astype(np.int32)
        self.n_pose_atoms = int(n_pose_atoms)
        if not 1 <= na <= MAX_ATOMS:
            raise ValueError(f"SdfTemplate: {na} atoms; a V2000 record takes 1 .. {MAX_ATOMS}")
        if self.atom.shape[0] != na or self.atom.min() < 0 or self.atom.max() >= self.n_pose_atoms:
            raise ValueError(f"SdfTemplate: {na} atoms, {self.atom.shape[0]} pose indices below {self.n_pose_atoms}")
        pairs = np.asarray(bonds.detach().cpu() if isinstance(bonds, torch.Tensor) else bonds, dtype=np.int64).reshape(-1, 2)
        nb = pairs.shape[0]
        if nb > MAX_BONDS:
            raise ValueError(f"SdfTemplate: {nb} bonds; a V2000 record takes at most {MAX_BONDS}")
        if nb and (pairs.min() < 0 or pairs.max() >= na or (pairs[:, 0] == pairs[:, 1]).any()):
            raise ValueError(f"SdfTemplate: a bond leaves the {na} atoms or joins an atom to itself")
        orders = np.ones(nb) if bond_orders is None else np.asarray(
            bond_orders.detach().cpu() if isinstance(bond_orders, torch.Tensor) else bond_orders, dtype=np.float64).reshape(-1)
        if orders.shape[0] != nb:
            raise ValueError(f"SdfTemplate: {nb} bonds but {orders.shape[0]} bond orders")
        bad = sorted({float(o) for o in orders.tolist() if float(o) not in BOND_TYPES})
        if bad:
            raise ValueError(f"SdfTemplate: bond orders are 1, 1.5, 2 or 3, got {bad}")
        self.bonds, self.bond_orders = pairs.astype(np.int32), orders
        self.bond_types = np.asarray([BOND_TYPES[float(o)] for o in orders.tolist()], dtype=np.int32)
        self.charges = np.zeros(na, dtype=np.int32) if charges is None else _ints(charges).astype(np.int32)
        if self.charges.shape[0] != na or (np.abs(self.charges) > 15).any():
            raise ValueError(f"SdfTemplate: {na} atoms, {self.charges.shape[0]} formal charges in -15 .. 15")
        self.title, self.comment, self.program = _line(title, "title"), _line(comment, "comment"), _line(program, "program name")
        self.hydrogens = None
        head = "\n".join([self.title, f"  {self.program:<8.8}{'':10}3D", self.comment, f"{na:3d}{nb:3d}" + _COUNTS_TAIL]) + "\n"
        lines = [f"{'':30} {s:<3}" + _ATOM_TAIL for s in self.symbols]
        lines += [f"{i + 1:3d}{j + 1:3d}{t:3d}  0" for (i, j), t in zip(self.bonds.tolist(), self.bond_types.tolist())]
        charged = [(a + 1, int(c)) for a, c in enumerate(self.charges.tolist()) if c]
        for k in range(0, len(charged), 8):
            lines.append(f"M  CHG{len(charged[k:k + 8]):3d}" + "".join(f"{a:4d}{c:4d}" for a, c in charged[k:k + 8]))
        self.molblock = head + "\n".join(lines + ["M  END"]) + "\n"
        self.atoms_at = len(head)
        self.tmpl = np.frombuffer(self.molblock.encode("ascii"), dtype=np.uint8).copy()
        self.map = np.full(self.tmpl.shape[0], -1, dtype=np.int32)
        for s in range(na):
            at = self.atoms_at + s * ATOM_LINE
            self.map[at:at + 30] = 30 * s + np.arange(30)
        self._tables: Dict[torch.device, Dict[str, torch.Tensor]] = {}
        if device is not None:
            self.tables(device)

    n_atoms = property(lambda self: len(self.symbols), doc="the atoms of a record")
    n_bonds = property(lambda self: int(self.bonds.shape[0]), doc="the bonds of a record")
    molblock_bytes = property(lambda self: int(self.tmpl.shape[0]), doc="M: the bytes of the molblock")

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_bonds(elements, bonds, ligand_idx, bond_orders=None, charges=None, title="", comment="", program="physdock", device=None):
        """elements: atomic numbers or symbols of EVERY atom of a pose [A]; ligand_idx [L]: the ligand's atoms in a pose, the atoms of the
        record in that order; bonds: pairs of LOCAL ligand indices; bond_orders [nb] (default: all single; 1.5 is written as type 4);
        charges [L]: formal charges (default: none).  What `parse_sdf` returns feeds this with `ligand_idx = range(na)`."""
        lig = _ints(ligand_idx)
        sym = _symbols(elements)
        if lig.shape[0] and (lig.min() < 0 or lig.max() >= len(sym)):
            raise ValueError(f"SdfTemplate: ligand_idx leaves the {len(sym)} atoms of a pose")
        return SdfTemplate([sym[i] for i in lig.tolist()], lig, len(sym), bonds, bond_orders, charges, title, comment, program, device)

    @staticmethod
    def from_batch(batch, bonds, bond_orders=None, charges=None, **kw):
        """from a feature dict, as the other `from_batch` constructors: the ligand's rows are the atoms of ligand tokens, the elements
        come from `ref_feat`, the tables are uploaded to the batch's device"""
        from .driver import ligand_atom_mask
        lig = torch.nonzero(ligand_atom_mask(batch)).flatten()
        elements = batch["ref_feat"][:, 4:132].argmax(-1) + 1
        dev = batch["ref_feat"].device
        kw.setdefault("device", dev if dev.type == "cuda" else None)
        return SdfTemplate.from_bonds(elements, bonds, lig, bond_orders=bond_orders, charges=charges, **kw)

    def with_hydrogens(self, hydrogens):
        """a `hydrogens.Hydrogens` of the same system -> a new template whose records are protonated: every hydrogen of the table that
        rides on an atom of the record is appended as an atom `H` with a single bond to its parent.  `format` then takes `x_all
        [P,A+H,3]` of `Hydrogens.place`; a hydrogen that was not placed is NaN there and makes `format` raise.  Receptor hydrogens are
        not written."""
        if hydrogens.n_pose_atoms != self.n_pose_atoms:
            raise ValueError(f"SdfTemplate.with_hydrogens: the template is over {self.n_pose_atoms} pose atoms, the hydrogens over "
                             f"{hydrogens.n_pose_atoms}")
        slot = {int(a): s for s, a in enumerate(self.atom.tolist())}
        rows = [h for h in range(hydrogens.n_hydrogens) if int(hydrogens.parent[h]) in slot]
        na = self.n_atoms
        new = SdfTemplate(self.symbols + ["H"] * len(rows), np.concatenate([self.atom, self.n_pose_atoms + np.asarray(rows, dtype=np.int32)]),
                          self.n_pose_atoms + hydrogens.n_hydrogens,
                          np.concatenate([self.bonds.reshape(-1, 2), np.asarray([(slot[int(hydrogens.parent[h])], na + k) for k, h in
                                                                                 enumerate(rows)], dtype=np.int32).reshape(-1, 2)]),
                          np.concatenate([self.bond_orders, np.ones(len(rows))]), np.concatenate([self.charges, np.zeros(len(rows), dtype=np.int32)]),
                          self.title, self.comment, self.program, next(iter(self._tables), None))
        new.hydrogens = hydrogens
        return new

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernel's tables on `device` (uploaded once)"""
        return ops.cached_upload(self._tables, device, lambda up: {k: up(getattr(self, k)) for k in ("tmpl", "map", "atom")})

    @staticmethod
    def items(properties, n_poses: int, device=None):
        """properties (an ordered mapping name -> tensor [P], or name -> (tensor, decimals)) -> a list of (name, int32 tensor [P] holding
        the 32 bits of every value, decimals or -1): float tensors become float32 with `DEFAULT_DECIMALS` decimals unless told, integer
        and bool tensors int32 (decimals -1).  Every violation of the limits raises ValueError."""
        out = []
        props = dict(properties or {})
        if len(props) > MAX_ITEMS:
            raise ValueError(f"SdfTemplate: {len(props)} data items; a call takes at most {MAX_ITEMS}")
        for name, v in props.items():
            if not isinstance(name, str) or len(name) > MAX_NAME or not _NAME.match(name):
                raise ValueError(f"SdfTemplate: a data item's name matches [A-Za-z_][A-Za-z0-9_.]* and holds at most {MAX_NAME} characters, "
                                 f"got {name!r}")
            decimals = None
            if isinstance(v, tuple):
                if len(v) != 2:
                    raise ValueError(f"SdfTemplate: data item {name!r} is a tensor or (tensor, decimals)")
                v, decimals = v
            t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
            if device is not None:
                t = t.to(device)
            t = t.reshape(-1)
            if t.shape[0] != n_poses:
                raise ValueError(f"SdfTemplate: data item {name!r} holds {t.shape[0]} values, there are {n_poses} poses")
            if t.is_floating_point():
                decimals = DEFAULT_DECIMALS if decimals is None else decimals
                if isinstance(decimals, bool) or int(decimals) != decimals or not 0 <= int(decimals) <= MAX_DECIMALS:
                    raise ValueError(f"SdfTemplate: data item {name!r}: decimals are an integer 0 .. {MAX_DECIMALS}, got {decimals!r}")
                out.append((name, t.to(torch.float32).contiguous().view(torch.int32), int(decimals)))
            elif t.is_complex():
                raise ValueError(f"SdfTemplate: data item {name!r} is complex")
            else:
                if decimals is not None:
                    raise ValueError(f"SdfTemplate: data item {name!r} is an integer item and takes no decimals")
                if not t.is_cuda and t.dtype != torch.bool and t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) >= 2 ** 31):
                    raise ValueError(f"SdfTemplate: data item {name!r} does not fit an int32")
                out.append((name, t.to(torch.int32).contiguous(), -1))
        return out

    def record_bytes(self, items=()):
        """(fixed, longest): the bytes of a record that are not a value's text, and the longest possible record, for items as `items`
        returns them (or any sequence of (name, anything, decimals or -1))"""
        fixed = self.molblock_bytes + sum(len(name) + 6 + 2 for name, _, _ in items) + 5
        return fixed, fixed + sum(FLOAT_TEXT_MAX if d >= 0 else INT_TEXT_MAX for _, _, d in items)

    def format(self, x: torch.Tensor, properties=None, order=None) -> Dict[str, torch.Tensor]:
        """x [P,A,3] (or [A,3]) on the device, A = `n_pose_atoms`; properties: an ordered mapping name -> tensor [P] or name -> (tensor,
        decimals), the values indexed by pose; order int [n]: the pose of every record (default: every pose in turn), so ranked output
        needs no gather of coordinates.  Returns {"bytes": uint8 [capacity], "offsets": int64 [n + 1], "n_records": n} on the device:
        record r is bytes[offsets[r]:offsets[r + 1]], bytes[:offsets[n]] is a valid SD file as it stands, `capacity` is the host-side
        upper bound.  Only the overflow counter is read back; it raises ValueError when a coordinate or a value does not fit."""
        if x.dim() == 2:
            x = x[None]
        if not x.is_cuda:
            raise RuntimeError("SdfTemplate.format runs on an MI355X (HIP) device only; there is no CPU path")
        if x.dim() != 3 or x.shape[1] != self.n_pose_atoms or x.shape[2] != 3:
            raise ValueError(f"SdfTemplate.format: the template is over {self.n_pose_atoms} pose atoms, x has shape {tuple(x.shape)}")
        P = int(x.shape[0])
        items = self.items(properties, P, x.device)
        if order is None:
            n, order_t = P, None
        else:
            if not (isinstance(order, torch.Tensor) and order.is_cuda):
                host = _ints(order)
                if host.shape[0] and (host.min() < 0 or host.max() >= P):
                    raise ValueError(f"SdfTemplate.format: order names a pose outside 0 .. {P - 1}")
                order = torch.from_numpy(host)
            order_t = order.reshape(-1).to(device=x.device, dtype=torch.int32).contiguous()
            n = int(order_t.shape[0])
        if not 1 <= n <= MAX_RECORDS:
            raise ValueError(f"SdfTemplate.format: {n} records; a call takes 1 .. {MAX_RECORDS}")
        x = x.float().contiguous()
        K = len(items)
        fixed, longest = self.record_bytes(items)
        capacity = n * longest
        t = self.tables(x.device)
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=x.device)
        out, offsets, overflow = new((capacity,), torch.uint8), new((n + 1,), torch.int64), torch.zeros(1, dtype=torch.int32, device=x.device)
        hdr = hdr_start = decimals = values = vlen = None
        if K:
            heads = [f">  <{name}>\n".encode("ascii") for name, _, _ in items]
            hdr = torch.frombuffer(bytearray(b"".join(heads)), dtype=torch.uint8).to(x.device)
            hdr_start = torch.tensor(np.concatenate([[0], np.cumsum([len(h) for h in heads])]), dtype=torch.int32).to(x.device)
            decimals = torch.tensor([d for _, _, d in items], dtype=torch.int32).to(x.device)
            values = torch.stack([v for _, v, _ in items]).contiguous()
            vlen = new((n, K), torch.uint8)
        ops.check(ops._lib.init().pd_sdf_format(ops.ptr(x), ops.ptr(t["tmpl"]), ops.ptr(t["map"]), ops.ptr(t["atom"]), ops.ptr(order_t),
                                                ops.ptr(hdr), ops.ptr(hdr_start), ops.ptr(decimals), ops.ptr(values), ops.ptr(vlen),
                                                ops.ptr(offsets), ops.ptr(out), ops.ptr(overflow), n, P, self.n_pose_atoms,
                                                self.molblock_bytes, K, fixed, longest, capacity, ops.stream()), "pd_sdf_format")
        bad = int(overflow.item())
        if bad:
            raise ValueError(f"{bad} numbers do not fit: a coordinate is not finite or does not fit the %10.4f SD file field, a value "
                             f"times 10^decimals reaches 1e15, or order names a pose outside 0 .. {P - 1}")
        return {"bytes": out, "offsets": offsets, "n_records": n}

    @staticmethod
    def split(result) -> List[str]:
        """a `format` result -> the records as a list of str (ONE copy back: the offsets and the bytes together)"""
        n = int(result["n_records"])
        packed = torch.cat([result["offsets"].view(torch.uint8), result["bytes"]]).cpu().numpy()
        offsets, raw = packed[:8 * (n + 1)].view(np.int64), packed[8 * (n + 1):].tobytes()
        return [raw[int(offsets[r]):int(offsets[r + 1])].decode("ascii") for r in range(n)]

    def blocks(self, x: torch.Tensor, properties=None, order=None) -> List[str]:
        """the records of `format(x, properties, order)` as a list of str, one per record (one copy back)"""
        return self.split(self.format(x, properties, order))

    def text(self, x: torch.Tensor, properties=None, order=None) -> str:
        """the whole SD file of `format(x, properties, order)` as one str"""
        return "".join(self.blocks(x, properties, order))

    def write_sdf(self, path, x: torch.Tensor, properties=None, order=None) -> int:
        """write the SD file of `format(x, properties, order)` to `path`; returns the number of records"""
        records = self.blocks(x, properties, order)
        with open(path, "w", encoding="ascii", newline="") as fh:
            fh.write("".join(records))
        return len(records)

    def __repr__(self):
        return (f"SdfTemplate(atoms={self.n_atoms}, bonds={self.n_bonds}, charged={int((self.charges != 0).sum())}, "
                f"n_pose_atoms={self.n_pose_atoms}, molblock_bytes={self.molblock_bytes}, protonated={self.hydrogens is not None})")


# ---------------------------------------------------------------------- the reader
def parse_sdf(text: str) -> List[dict]:
    """The records of a V2000 SD file (or of one molfile) -> a list of dicts: `title` (str), `elements` (symbols), `coords` float64
    [na,3], `bonds` int64 [nb,2] (0-based), `bond_orders` float64 [nb] (type 4 becomes 1.5), `charges` int64 [na] (`M  CHG` lines, else
    the charge field of the atom lines) and `properties` (name -> str, in file order).  V2000 only; anything else - a V3000 counts
    line, a truncated block, a bond type beyond 1 .. 4, a property line other than `M  CHG`, a missing `M  END` - raises ValueError with
    the line number (1-based).  `SdfTemplate.from_bonds(r["elements"], r["bonds"], range(len(r["elements"])), r["bond_orders"],
    r["charges"])` takes the result as it is."""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    lines = [ln[:-1] if ln.endswith("\r") else ln for ln in lines]
    n_lines = len(lines)

    def fail(k, why):
        raise ValueError(f"parse_sdf: line {k + 1}: {why}")

    def number(k, a, b, kind, what):
        if k >= n_lines:
            fail(n_lines - 1 if n_lines else 0, f"the file ends inside the {what}")
        try:
            return kind(lines[k][a:b])
        except ValueError:
            fail(k, f"columns {a + 1} .. {b} of the {what} hold {lines[k][a:b]!r}")

    out, k = [], 0
    while k < n_lines:
        if all(not ln.strip() for ln in lines[k:]):
            break
        start = k
        if start + 3 >= n_lines:
            fail(n_lines - 1, "the file ends inside the header block")
        counts = lines[start + 3]
        if "V3000" in counts:
            fail(start + 3, "a V3000 counts line; V2000 only")
        if not counts.rstrip().endswith("V2000"):
            fail(start + 3, f"not a V2000 counts line: {counts!r}")
        na, nb = number(start + 3, 0, 3, int, "counts line"), number(start + 3, 3, 6, int, "counts line")
        if na < 1 or nb < 0:
            fail(start + 3, f"{na} atoms and {nb} bonds")
        k = start + 4
        elements, coords, old = [], np.zeros((na, 3)), np.zeros(na, dtype=np.int64)
        for a in range(na):
            if k < n_lines and (lines[k].startswith("M  ") or lines[k].startswith("$$$$") or len(lines[k]) < 32):
                fail(k, f"the atom block is truncated: atom line {a + 1} of {na} expected")
            coords[a] = [number(k, 10 * c, 10 * c + 10, float, "atom block") for c in range(3)]
            symbol = lines[k][31:34].strip()
            if not symbol:
                fail(k, "an atom line without an element symbol")
            elements.append(symbol)
            code = number(k, 36, 39, int, "atom block") if lines[k][36:39].strip() else 0
            if code not in _OLD_CHARGES:
                fail(k, f"charge code {code}")
            old[a] = _OLD_CHARGES[code]
            k += 1
        bonds, orders = np.zeros((nb, 2), dtype=np.int64), np.zeros(nb)
        for b in range(nb):
            if k < n_lines and (lines[k].startswith("M  ") or lines[k].startswith("$$$$")):
                fail(k, f"the bond block is truncated: bond line {b + 1} of {nb} expected")
            i, j, t = (number(k, 3 * c, 3 * c + 3, int, "bond block") for c in range(3))
            if not (1 <= i <= na and 1 <= j <= na and i != j):
                fail(k, f"a bond between atoms {i} and {j} of {na}")
            if t not in (1, 2, 3, 4):
                fail(k, f"bond type {t}; 1, 2, 3 and 4 (aromatic) are read")
            bonds[b], orders[b] = (i - 1, j - 1), 1.5 if t == 4 else float(t)
            k += 1
        charges, seen_chg = np.zeros(na, dtype=np.int64), False
        while True:
            if k >= n_lines or lines[k].startswith("$$$$") or lines[k].startswith(">"):
                fail(min(k, n_lines - 1), "M  END is missing")
            ln = lines[k]
            if ln.startswith("M  END"):
                k += 1
                break
            if not ln.startswith("M  CHG"):
                fail(k, f"a property line other than M  CHG: {ln!r}")
            seen_chg = True
            for e in range(number(k, 6, 9, int, "M  CHG line")):
                a, c = number(k, 9 + 8 * e, 13 + 8 * e, int, "M  CHG line"), number(k, 13 + 8 * e, 17 + 8 * e, int, "M  CHG line")
                if not 1 <= a <= na:
                    fail(k, f"a charge on atom {a} of {na}")
                charges[a - 1] = c
            k += 1
        properties: Dict[str, str] = {}
        while k < n_lines and not lines[k].startswith("$$$$"):
            ln = lines[k]
            if not ln.strip():
                k += 1
                continue
            m = re.match(r">.*<([^>]*)>", ln)
            if not m:
                fail(k, f"a data header `>  <name>` or $$$$ expected, got {ln!r}")
            k += 1
            value = []
            while k < n_lines and lines[k].strip() and not lines[k].startswith("$$$$"):
                value.append(lines[k])
                k += 1
            properties[m.group(1)] = "\n".join(value)
        k += 1                                                            # the $$$$ line (a lone molfile ends without one)
        out.append({"title": lines[start], "elements": elements, "coords": coords, "bonds": bonds, "bond_orders": orders,
                    "charges": charges if seen_chg else old, "properties": properties})
    return out


def check_redock_sdf(sdf, batch, hydrogens) -> None:
    """redock(sdf=): raise ValueError unless `sdf` is an `SdfTemplate` over the batch's atoms - or, made by `with_hydrogens` of the
    `hydrogens=` object of the same call, over the atoms and its hydrogens"""
    if sdf is None:
        return
    if not callable(getattr(sdf, "format", None)) or not hasattr(sdf, "n_pose_atoms"):
        raise ValueError("sdf= takes an sdfio.SdfTemplate of the ligand")
    n = int(batch["x_gt"].shape[0])
    if getattr(sdf, "hydrogens", None) is not None:
        if sdf.hydrogens is not hydrogens:
            raise ValueError("sdf= was protonated by with_hydrogens: pass the same Hydrogens object as hydrogens=")
        n += hydrogens.n_hydrogens
    if sdf.n_pose_atoms != n:
        raise ValueError(f"sdf= was built over {sdf.n_pose_atoms} pose atoms, the records of this call hold {n}")


def redock_items(out) -> Dict[str, object]:
    """the data items of redock(sdf=) from what the same call computed, in this order: `pose` (the index into `poses`), with
    `confidence=` `ranking_confidence`, with `vina=` `vina_score` (`vina["score"]`), with `validity=` `valid` (`validity["valid"]`),
    with the ground truth and `ranking` `ligand_rmsd` (`ranking["rmsd_all"]`) and, with `lddt_pli=`, `lddt_pli`
    (`ranking["lddt_pli_all"]`), with `clusters=` `cluster` (`clusters["labels"]`), with `conformer_rmsd=` and the ground truth
    `conformer_rmsd` (`conformer_rmsd["to_gt"]`), with `shape=` `shape_tanimoto` and `tanimoto_combo` (`shape["shape_tanimoto"]`,
    `shape["combo"]`), with `torsions=` and the ground truth `tfd` (`torsions["to_gt"]`), with `distogram=` `distogram_nll`
    (`distogram["nll_interface"]`), with `pocket_accuracy=` `lddt_lp` and `pocket_ca_rmsd` (`pocket_accuracy["lddt_lp"]`,
    `pocket_accuracy["ca_rmsd"]`), with `bond_stereo=` `stereo_ok` (`bond_stereo["ok"]`)"""
    n = int(out["poses"].shape[0])
    items: Dict[str, object] = {"pose": torch.arange(n, dtype=torch.int32, device=out["poses"].device)}
    if "confidence" in out:
        items["ranking_confidence"] = out["confidence"]["ranking_confidence"]
    if "vina" in out:
        items["vina_score"] = out["vina"]["score"]
    if "validity" in out:
        items["valid"] = out["validity"]["valid"]
    if out.get("ranking") is not None:
        items["ligand_rmsd"] = out["ranking"]["rmsd_all"]
        if "lddt_pli_all" in out["ranking"]:
            items["lddt_pli"] = out["ranking"]["lddt_pli_all"]
    if "clusters" in out:
        items["cluster"] = out["clusters"]["labels"]
    if "to_gt" in out.get("conformer_rmsd", {}):
        items["conformer_rmsd"] = out["conformer_rmsd"]["to_gt"]
    if "shape" in out:
        items["shape_tanimoto"] = out["shape"]["shape_tanimoto"]
        items["tanimoto_combo"] = out["shape"]["combo"]
    if "to_gt" in out.get("torsions", {}):
        items["tfd"] = out["torsions"]["to_gt"]
    if "distogram" in out:
        items["distogram_nll"] = out["distogram"]["nll_interface"]
    if "pocket_accuracy" in out:
        items["lddt_lp"] = out["pocket_accuracy"]["lddt_lp"]
        items["pocket_ca_rmsd"] = out["pocket_accuracy"]["ca_rmsd"].contiguous()
    if "bond_stereo" in out:
        items["stereo_ok"] = out["bond_stereo"]["ok"]
    return items


def score_sdf(sdf, aligned, out) -> dict:
    """redock(sdf=): {"sdf": SdfTemplate.format of the kept poses in their order with the items of `redock_items`}; a template made by
    `with_hydrogens` takes the poses with the hydrogens `hydrogens=` placed"""
    x = aligned if sdf.hydrogens is None else torch.cat([aligned.float(), out["hydrogens"]["x_h"]], 1)
    return {"sdf": sdf.format(x, redock_items(out))}
