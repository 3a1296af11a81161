"""The written definition of this package's SD file records (physdock_amd/sdfio.py, csrc/sdf.hip): a plain Python / numpy writer that
imports nothing from the package.  The format is the CTfile V2000 specification, not RDKit's bytes: no program time stamp (the text is
reproducible), no wedge flags (the 3-D coordinates carry the stereo), charges only in `M  CHG` lines.

One record is the molblock

    {title}                                              line 1, <= 80 characters, no control characters
      {program:<8.8}{'':10}3D                            line 2
    {comment}                                            line 3
    {na:3d}{nb:3d}  0  0  0  0  0  0  0  0999 V2000
    {x:10.4f}{y:10.4f}{z:10.4f} {symbol:<3} 0  0  0  0  0  0  0  0  0  0  0  0      one per atom, 69 columns
    {i+1:3d}{j+1:3d}{type:3d}  0                                                   one per bond: type 1, 2, 3, and 4 for order 1.5
    M  CHG{n:3d}{atom:4d}{charge:4d}...                                            the non-zero formal charges, 8 per line, atoms ascending
    M  END

followed by the data items in the order given, each `>  <{name}>`, the value, an empty line, and the line `$$$$`.  A float value with d
decimals is f"{float(v):.{d}f}" of the float32 value, an int value is str(v); nothing is padded."""
import re

import numpy as np

BOND_TYPES = {1.0: 1, 2.0: 2, 3.0: 3, 1.5: 4}
NAME = re.compile(r"[A-Za-z_][A-Za-z0-9_.]*\Z")
COUNTS_TAIL = "  0  0  0  0  0  0  0  0999 V2000"
ATOM_TAIL = " 0" + "  0" * 11


def molblock(symbols, coords, bonds=(), bond_orders=None, charges=None, title="", comment="", program="physdock"):
    """the molblock of one pose, up to and including `M  END` and its newline.  coords [na,3]: float32 values (anything else is
    rounded to float32 first); None writes 30 blanks in their place"""
    symbols = [str(s) for s in symbols]
    na, bonds = len(symbols), [(int(i), int(j)) for i, j in bonds]
    orders = [1.0] * len(bonds) if bond_orders is None else [float(o) for o in bond_orders]
    lines = [title, f"  {program:<8.8}{'':10}3D", comment, f"{na:3d}{len(bonds):3d}" + COUNTS_TAIL]
    xyz = None if coords is None else np.asarray(coords, dtype=np.float32).reshape(na, 3)
    for a, s in enumerate(symbols):
        head = " " * 30 if xyz is None else "".join(f"{float(v):10.4f}" for v in xyz[a])
        lines.append(f"{head} {s:<3}" + ATOM_TAIL)
    for (i, j), o in zip(bonds, orders):
        lines.append(f"{i + 1:3d}{j + 1:3d}{BOND_TYPES[o]:3d}  0")
    charged = [] if charges is None else [(a + 1, int(c)) for a, c in enumerate(charges) if int(c) != 0]
    for k in range(0, len(charged), 8):
        part = charged[k:k + 8]
        lines.append(f"M  CHG{len(part):3d}" + "".join(f"{a:4d}{c:4d}" for a, c in part))
    lines.append("M  END")
    return "\n".join(lines) + "\n"


def value_text(v, decimals=None):
    """the text of one data value: decimals None - an integer; else a float32 value with that many decimals"""
    if decimals is None:
        return str(int(v))
    return f"{float(np.float32(v)):.{int(decimals)}f}"


def items_text(items):
    """items: a sequence of (name, value, decimals or None) -> the data items and the `$$$$` line"""
    return "".join(f">  <{name}>\n{value_text(v, d)}\n\n" for name, v, d in items) + "$$$$\n"


def record(symbols, coords, bonds=(), bond_orders=None, charges=None, items=(), **kw):
    """one record: the molblock, the data items, `$$$$`"""
    return molblock(symbols, coords, bonds, bond_orders, charges, **kw) + items_text(items)


def records(symbols, poses, bonds=(), bond_orders=None, charges=None, properties=(), order=None, **kw):
    """the records of poses [P,na,3] in the order `order` (pose ids, default 0 .. P-1).  properties: a sequence of (name, values [P],
    decimals or None), the values indexed by pose.  A list of str."""
    poses = np.asarray(poses, dtype=np.float32)
    ids = range(poses.shape[0]) if order is None else [int(p) for p in order]
    return [record(symbols, poses[p], bonds, bond_orders, charges, [(name, vals[p], d) for name, vals, d in properties], **kw) for p in ids]
