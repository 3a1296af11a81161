"""Seeded synthetic systems for the PocketAccuracy tests, built from residue and atom NAMES (no reference data): residues of the seven
swappable types plus GLY and ALA as clouds of named heavy atoms around a 5-atom ligand at the origin, inside a +-20 A box.  A residue
sits at a chosen distance from the ligand, which decides whether it is a pocket residue (< 8 A), environment (a pair partner only) or
neither.  All coordinates lie on a grid of 2^-10 A, so that a quarter turn and a grid translation move a structure EXACTLY in fp32.
The geometry is not physical: the measure only needs names, residues and distances.

`reference(name)` computes the float64 restatement (tests/pocket_accuracy_ref.py) of a case once and shares it read-only."""
import functools

import numpy as np

import pocket_accuracy_ref as ref

GRID = 1024.0
SIDE = {"GLY": (), "ALA": ("CB",), "ASP": ("CB", "CG", "OD1", "OD2"), "GLU": ("CB", "CG", "CD", "OE1", "OE2"),
        "ARG": ("CB", "CG", "CD", "NE", "CZ", "NH1", "NH2"), "LEU": ("CB", "CG", "CD1", "CD2"), "VAL": ("CB", "CG1", "CG2"),
        "PHE": ("CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ"), "TYR": ("CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ", "OH")}
NINE = ("ASP", "GLU", "ARG", "LEU", "VAL", "PHE", "TYR", "GLY", "ALA")


def grid(x):
    return np.round(np.asarray(x, dtype=np.float64) * GRID) / GRID


def system(seed, layout, missing=(), hydrogens=0, spread=1.2):
    """layout: (residue kind, distance of its centre from the origin) per residue; missing: (residue number, atom name) masked out;
    hydrogens: that many extra "H" atoms appended to residue 0 (existing, not heavy) -> dict of per-atom lists / arrays, ligand last"""
    rng = np.random.RandomState(seed)
    res_names, atom_names, residue_of, x, mask = [], [], [], [], []
    for r, (kind, dist) in enumerate(layout):
        u = rng.normal(size=3)
        centre = u / np.linalg.norm(u) * dist
        names = ("N", "CA", "C", "O") + SIDE[kind] + (("H",) * hydrogens if r == 0 else ())
        for a in names:
            res_names.append(kind); atom_names.append(a); residue_of.append(r)
            x.append(centre + rng.normal(size=3) * spread)
            mask.append(a != "H" and (r, a) not in missing)
    lig0 = len(x)
    for k in range(5):
        res_names.append("LIG"); atom_names.append(f"C{k + 1}"); residue_of.append(len(layout) + k)
        x.append(rng.normal(size=3))
        mask.append(True)
    x = np.clip(grid(x), -20.0, 20.0)
    return dict(res_names=res_names, atom_names=atom_names, residue_of=np.asarray(residue_of), x_ref=x, mask=np.asarray(mask),
                ligand_idx=np.arange(lig0, lig0 + 5), layout=layout)


def jitter(s, seed, sigmas):
    rng = np.random.RandomState(seed)
    return np.stack([grid(s["x_ref"] + rng.normal(size=s["x_ref"].shape) * sg) for sg in sigmas])


def atom(s, r, name):
    return next(a for a in range(len(s["atom_names"])) if s["residue_of"][a] == r and s["atom_names"][a] == name)


def exchanged(s, x, residues):
    """x [A,3] with the swap pairs of the given residues exchanged"""
    x = np.array(x)
    for r in residues:
        for a, b in ref.SWAPS[s["layout"][r][0]]:
            i, j = atom(s, r, a), atom(s, r, b)
            x[[i, j]] = x[[j, i]]
    return x


QUARTER = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])          # a quarter turn about z: exact
SHIFT = np.array([1.5, -2.25, 0.125])


def moved(x):
    return np.asarray(x) @ QUARTER.T + SHIFT


def turned(x, seed=5):
    """a general rotation and translation, rounded to the grid: the fp32 rounding of the coordinates shows in the RMSD"""
    q, _ = np.linalg.qr(np.random.RandomState(seed).normal(size=(3, 3)))
    q = q * np.sign(np.linalg.det(q))
    return grid(np.asarray(x) @ q.T + np.array([3.0, -1.0, 2.0]))


def mirrored(x):
    return np.asarray(x) * np.array([-1.0, 1.0, 1.0])


def _nine():
    s = system(16, [(k, 5.0) for k in NINE])
    xr = s["x_ref"]
    # ref; ASP swapped; PHE (two pairs together); LEU and VAL, neighbours, both swapped; moved exactly; turned; mirrored; jittered
    special = [xr, exchanged(s, xr, [0]), exchanged(s, xr, [5]), exchanged(s, xr, [3, 4]), moved(xr), turned(xr), mirrored(xr)]
    return s, np.concatenate([np.stack(special), jitter(s, 17, [0.1, 0.4, 1.0, 2.0, 3.0])]), {}


def _far():
    layout = [("ASP", 5.0), ("PHE", 5.0), ("GLY", 5.0), ("LEU", 5.0), ("ARG", 5.0), ("TYR", 5.0), ("ASP", 5.0), ("GLU", 13.0), ("VAL", 13.0),
              ("ALA", 13.0), ("ALA", 17.0), ("GLY", 17.0)]
    s = system(21, layout, missing=[(6, "OD2")], hydrogens=2)
    return s, jitter(s, 22, [0.2, 1.0, 2.5]), {}


def _one():
    s = system(31, [("ASP", 3.0), ("ALA", 14.0), ("GLY", 14.0), ("VAL", 14.0), ("LEU", 14.0), ("PHE", 14.0)])
    return s, np.concatenate([s["x_ref"][None], exchanged(s, s["x_ref"], [0])[None], jitter(s, 32, [0.5])]), {}


def _two():
    s = system(41, [("ASP", 3.0), ("LEU", 3.0), ("ALA", 14.0), ("GLY", 14.0), ("VAL", 14.0), ("TYR", 14.0)])
    return s, np.concatenate([s["x_ref"][None], jitter(s, 42, [0.3, 1.5])]), {}


def _nopairs():
    s = system(51, [("VAL", 2.0), ("ALA", 15.0), ("GLY", 15.0), ("ASP", 15.0), ("GLU", 15.0), ("LEU", 15.0)])
    return s, jitter(s, 52, [0.3]), dict(pocket_radius=6.0, inclusion_radius=3.0)


def _blob(row_length):
    """56 ALA in a dense blob; the inclusion radius is set between two neighbour distances of the first pocket atom, so that its row
    holds exactly `row_length` pairs"""
    rng = np.random.RandomState(61)
    s = system(61, [("ALA", 9.0 * rng.uniform() ** (1 / 3)) for _ in range(56)])
    x, res = s["x_ref"], s["residue_of"]
    tab = ref.build(x, res, s["mask"], s["ligand_idx"], np.zeros(len(x), bool), np.zeros(len(x), bool), pocket_radius=3.0)
    i = tab["patom"][0]
    rec = np.nonzero(s["mask"])[0]
    rec = rec[(res[rec] != res[i]) & ~np.isin(rec, s["ligand_idx"])]
    d = np.sort(np.sqrt(((x[rec] - x[i]) ** 2).sum(-1)))
    assert len(d) > row_length and d[row_length] - d[row_length - 1] > 1e-6
    return s, jitter(s, 62, [0.2, 1.0]), dict(pocket_radius=3.0, inclusion_radius=float(0.5 * (d[row_length - 1] + d[row_length])))


CASES = {"nine": _nine, "far": _far, "one": _one, "two": _two, "nopairs": _nopairs, "row1": lambda: _blob(1), "row256": lambda: _blob(256),
         "row257": lambda: _blob(257)}


def tables(s, **kw):
    names = [str(a).upper() for a in s["atom_names"]]
    rec = s["mask"].copy()
    rec[s["ligand_idx"]] = False
    swaps = ref.swap_table(s["res_names"], s["atom_names"], s["residue_of"], rec)
    return ref.build(s["x_ref"], s["residue_of"], rec, s["ligand_idx"], [n == "CA" for n in names], [n in ref.BACKBONE for n in names], swaps, **kw)


def freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(s = the system, x [P,A,3] the poses, kw = the radii, tab = the restatement's tables, out = its scores): read-only"""
    s, x, kw = CASES[name]()
    tab = tables(s, **kw)
    return dict(s=freeze(s), x=freeze(dict(x=x))["x"], kw=kw, tab=freeze(tab), out=freeze(ref.score(tab, x)))
