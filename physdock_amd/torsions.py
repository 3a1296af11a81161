"""Which rotatable bond is wrong?  The ligand's torsion angles per pose and the torsion-fingerprint deviation TFD between poses on the
device (kernels `pd_torsion_prepare`, `pd_torsion_tfd`, `pd_torsion_deviation`, csrc/torsion.hip; tests/torsion_ref.py is the written
definition).  A best-fit RMSD of 1.4 A may be one flipped amide or ten small twists, and it grows with the lever arm of a torsion
rather than with its error; TFD (Schulz-Gasch, Schaerfer, Guba & Rarey 2012) compares conformations in the coordinates a chemist
thinks in, is independent of size and lies in 0 .. 1.  **The package's own definition, not RDKit's `TorsionFingerprints` bytes.**

    entries       one per rotatable bond (b, c) of `refine.rotatable_bonds` with ALL quadruples (a, b, c, d), a a neighbour of b other
                  than c, d of c other than b (at most 9; RDKit picks one pair - taking all makes the list invariant under the ligand's
                  automorphisms), max_dev 180; one per ring of 4 .. 8 atoms (every chordless simple cycle, aromatic or not) with its n
                  consecutive quadruples, max_dev = 180 exp(-0.025 (n - 14)^2)
    angle         the IUPAC dihedral in float64 from the fp32 coordinates, atan2(|b2| b1.(b2 x b3), (b1 x b2).(b2 x b3)); NaN for a
                  non-finite coordinate or a collinear triple (|b1 x b2|^2 <= 1e-12 |b1|^2 |b2|^2)
    dev_t(x, y) = min(1, mean over the entry's quadruples of |wrap(theta_x - theta_y)| / max_dev_t)
    w_t         = exp(-beta d_t^2), beta = ln 10 / (max(1, max_t d_t) / 2)^2, d_t the topological distance of the entry to the graph's
                  centre C (the atoms with the smallest sum of topological distances); `weights="uniform"` or an array overrides
    TFD(x, y)   = sum_t w_t dev_t / sum_t w_t, rounded once to fp32; 0 without entries; NaN when a quadruple it names has no angle
    with a `LigandSymmetry` table: min_m TFD(x, y o perm_m), exact, the smallest m on a tie; a NaN never wins

`TorsionFingerprint` is an immutable spec; `angles`, `cross`, `to_reference` and `pairwise` return device tensors and read nothing back
(one exception: index lists are checked on the host, so a `target_idx` or `ligand_idx` given as a DEVICE tensor is copied to the host
once, where it is given; pass host lists to avoid that).

**Caveats.**  Heavy atoms only (the graph the spec is given).  Rings of more than 8 atoms contribute nothing, so a macrocycle's
conformation is not seen.  A planar aromatic ring is an entry whose deviation is always near 0: it dilutes the value (with its weight)
rather than leaving it alone.  The weights follow the published Gaussian of the distance to the centre and are not validated against
anything.  A table cut at `max_perms` makes every value an upper bound (`symmetry_complete`).  Limits: 1024 ligand atoms, 1024
entries, 4096 distinct quadruples after closing them under the table, 65535 table rows, 65535 structures on either side."""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, Optional

import numpy as np
import torch

from . import _ligand_sides as sides
from . import ops
from ._ligand_sides import MAX_STRUCTURES
from .refine import rotatable_bonds

__all__ = ["TorsionFingerprint", "TorsionEntry", "ring_max_dev", "chordless_rings", "MAX_ATOMS", "MAX_ENTRIES", "MAX_QUADS", "MAX_STRUCTURES"]

#: limits of the kernels (csrc/torsion.hip)
MAX_ATOMS = 1024
MAX_ENTRIES = 1024
MAX_QUADS = 4096
_WHO = dict(name="TorsionFingerprint", takes="the kernels take")      # for the messages of _ligand_sides

#: one entry of the fingerprint: kind "bond" / "ring", its atoms (the bond's two, the ring in canonical cyclic order), its quadruples,
#: weight and max_dev in degrees
TorsionEntry = namedtuple("TorsionEntry", "kind atoms quads weight max_dev")


def ring_max_dev(n: int) -> float:
    """the published ring rule: 180 exp(-0.025 (n - 14)^2) degrees"""
    return 180.0 * float(np.exp(-0.025 * (int(n) - 14) ** 2))


def _adjacency(n, bonds):
    adj = [set() for _ in range(n)]
    for i, j in bonds:
        if not (0 <= i < n and 0 <= j < n) or i == j:
            raise ValueError(f"TorsionFingerprint: bond ({i}, {j}) of a graph of {n} atoms")
        adj[i].add(j); adj[j].add(i)
    return adj


def chordless_rings(n_atoms: int, bonds, smallest: int = 4, largest: int = 8):
    """every chordless simple cycle of `smallest` .. `largest` atoms as a tuple in canonical cyclic order (from its smallest atom towards
    the smaller of that atom's two ring neighbours), in ascending order.  Depth-first over paths that start at the cycle's smallest atom
    and never touch an earlier path atom other than through the closing bond."""
    adj = _adjacency(int(n_atoms), [(int(i), int(j)) for i, j in bonds])
    found = []
    for s in range(int(n_atoms)):
        stack = [[s]]
        while stack:
            path = stack.pop()
            inner = path[1:-1]
            for u in adj[path[-1]]:
                if u <= s or u in path or any(u in adj[p] for p in inner):
                    continue
                if len(path) >= 2 and u in adj[s]:
                    if len(path) + 1 >= smallest and path[1] < u:
                        found.append(tuple(path) + (u,))
                elif len(path) + 1 < largest:
                    stack.append(path + [u])
    return sorted(found)


def _centre_distances(n, bonds, atom_sets):
    """(d_t per atom set, the centre atoms): topological distances by breadth-first search; a pair in different components counts n"""
    adj = _adjacency(n, bonds)
    D = np.full((n, n), n, dtype=np.int64)
    for s in range(n):
        D[s, s] = 0
        front, d = [s], 0
        while front:
            d += 1
            nxt = []
            for a in front:
                for b in adj[a]:
                    if b != s and D[s, b] == n:
                        D[s, b] = d
                        nxt.append(b)
            front = nxt
    tot = D.sum(1)
    C = np.nonzero(tot == tot.min())[0]
    return np.array([int(D[np.ix_(list(atoms), C)].min()) for atoms in atom_sets], dtype=np.int64), C


def _canonical(q):
    """a quadruple and its reverse are one quadruple: the smaller of the two tuples"""
    q = tuple(int(v) for v in q)
    return min(q, q[::-1])


class TorsionFingerprint:
    """An immutable spec: `n_atoms` ligand atoms, `entries` (a tuple of `TorsionEntry`), `ligand_idx` (the ligand atoms of a pose [A,3]
    in the order of the graph; None: a pose holds the ligand alone) and `symmetry` (a `symmetry.LigandSymmetry`; None: the identity).
    Everything the kernels index with is checked here, on the host, once."""

    __slots__ = ("n_atoms", "entries", "n_entries", "ligand_idx", "symmetry", "quads", "image", "qstart", "_dev", "_idx")

    def __init__(self, n_atoms, entries, ligand_idx=None, symmetry=None):
        n = int(n_atoms)
        if not 1 <= n <= MAX_ATOMS:
            raise ValueError(f"TorsionFingerprint: {n} ligand atoms; the kernels take 1 .. {MAX_ATOMS}")
        idx = sides.host_idx(ligand_idx, "ligand_idx", "TorsionFingerprint")
        if idx is not None and idx.shape[0] != n:
            raise ValueError(f"TorsionFingerprint: ligand_idx names {idx.shape[0]} atoms, the graph has {n}")
        if symmetry is not None and not (hasattr(symmetry, "perms") and hasattr(symmetry, "n_atoms")):
            raise ValueError(f"TorsionFingerprint: symmetry= takes a symmetry.LigandSymmetry, got {type(symmetry).__name__}")
        if symmetry is not None and symmetry.n_atoms != n:
            raise ValueError(f"TorsionFingerprint: the symmetry table is over {symmetry.n_atoms} atoms, the graph has {n}")
        ents = []
        for e in entries:
            e = TorsionEntry(*e)
            quads = tuple(tuple(int(v) for v in q) for q in e.quads)
            if e.kind not in ("bond", "ring") or not quads or any(len(q) != 4 for q in quads):
                raise ValueError("TorsionFingerprint: an entry needs kind 'bond' or 'ring' and at least one quadruple of four atoms")
            if any(not 0 <= v < n for q in quads for v in q):
                raise ValueError(f"TorsionFingerprint: a quadruple names an atom outside 0 .. {n - 1}")
            w, md = float(e.weight), float(e.max_dev)
            if not (np.isfinite(w) and w >= 0.0) or not (np.isfinite(md) and md > 0.0):
                raise ValueError("TorsionFingerprint: weights must be finite and >= 0, max_dev finite and > 0")
            ents.append(TorsionEntry(e.kind, tuple(int(a) for a in e.atoms), quads, w, md))
        T = len(ents)
        if T > MAX_ENTRIES:
            raise ValueError(f"TorsionFingerprint: {T} entries; the kernels take up to {MAX_ENTRIES}")
        if T and not sum(e.weight for e in ents) > 0.0:
            raise ValueError("TorsionFingerprint: the weights sum to zero")
        # the base quadruples entry after entry, their closure under the table and the image of every base quadruple in every table row
        base = np.asarray([q for e in ents for q in e.quads], dtype=np.int64).reshape(-1, 4)
        perms = np.arange(n, dtype=np.int64)[None] if symmetry is None else np.asarray(symmetry.perms, dtype=np.int64)
        M, Nq = int(perms.shape[0]), int(base.shape[0])
        step = max(1, (1 << 20) // max(1, Nq))                        # table rows per pass: about 2^20 quadruples at a time

        def keys(m0):
            """the canonical images of the base quadruples under the table rows m0 .. m0 + step - 1, each as one integer [rows, Nq]"""
            img = perms[m0:m0 + step][:, base]                        # [rows, Nq, 4]
            rev = img[..., ::-1]
            flip = np.zeros(img.shape[:2], dtype=bool)
            for k in range(4):                                        # lexicographic: is the reverse the smaller tuple?
                flip |= np.all(img[..., :k] == rev[..., :k], axis=-1) & (rev[..., k] < img[..., k]) & ~flip
            img = np.where(flip[..., None], rev, img)
            return ((img[..., 0] * n + img[..., 1]) * n + img[..., 2]) * n + img[..., 3]

        uniq = np.zeros(0, dtype=np.int64)
        for m0 in range(0, M, step):                                  # first pass: the closure, refused as soon as it is too large
            uniq = np.union1d(uniq, keys(m0))
            if uniq.shape[0] > MAX_QUADS:
                raise ValueError(f"TorsionFingerprint: more than {MAX_QUADS} distinct quadruples after closing them under the symmetry "
                                 f"table ({uniq.shape[0]} within its first {min(M, m0 + step)} rows); the kernels take up to {MAX_QUADS}")
        Q = int(uniq.shape[0])
        quads = np.stack([uniq // n ** 3, uniq // n ** 2 % n, uniq // n % n, uniq % n], -1).astype(np.int32).reshape(Q, 4)
        image = np.empty((Nq, M), dtype=np.uint16)                    # m fastest
        for m0 in range(0, M, step):                                  # second pass: where every image sits in the closure
            image[:, m0:m0 + step] = np.searchsorted(uniq, keys(m0)).T
        qstart = np.concatenate([[0], np.cumsum([len(e.quads) for e in ents])]).astype(np.int32)
        for name, val in (("n_atoms", n), ("entries", tuple(ents)), ("n_entries", T), ("symmetry", symmetry), ("quads", quads),
                          ("ligand_idx", None if idx is None else tuple(int(v) for v in idx)), ("image", image), ("qstart", qstart),
                          ("_dev", {}), ("_idx", {})):
            object.__setattr__(self, name, val)

    def __setattr__(self, name, value):
        raise AttributeError("TorsionFingerprint is immutable")

    def __repr__(self):
        return f"TorsionFingerprint(n_atoms={self.n_atoms}, n_entries={self.n_entries}, symmetry={self.symmetry!r})"

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_tables(n_atoms, entries, ligand_idx=None, symmetry=None):
        """everything explicit: `entries` an iterable of (kind, atoms, quads, weight, max_dev)"""
        return TorsionFingerprint(n_atoms, entries, ligand_idx, symmetry)

    @staticmethod
    def from_bonds(n_atoms, bonds, bond_orders=None, ligand_idx=None, symmetry=None, weights=None):
        """from the heavy-atom bond graph (pairs of LOCAL ligand indices).  `weights`: None (the Gaussian of the distance to the centre),
        "uniform", or an array with one value per entry - the rotatable bonds in the order of `bonds`, then the rings ascending."""
        n = int(n_atoms)
        if not 1 <= n <= MAX_ATOMS:
            raise ValueError(f"TorsionFingerprint: {n} ligand atoms; the kernels take 1 .. {MAX_ATOMS}")
        bonds = [(int(i), int(j)) for i, j in np.asarray(bonds, dtype=np.int64).reshape(-1, 2)]
        adj = _adjacency(n, bonds)
        found = []
        for b, c in rotatable_bonds(n, bonds, bond_orders):
            found.append(("bond", (b, c), [(a, b, c, d) for a in sorted(adj[b] - {c}) for d in sorted(adj[c] - {b})], 180.0))
        for r in chordless_rings(n, bonds):
            k = len(r)
            found.append(("ring", r, [tuple(r[(i + s) % k] for s in range(4)) for i in range(k)], ring_max_dev(k)))
        T = len(found)
        if weights is None:
            if T:
                d = _centre_distances(n, bonds, [f[1] for f in found])[0].astype(np.float64)
                w = np.exp(-np.log(10.0) / (max(1.0, float(d.max())) / 2.0) ** 2 * d * d)
            else:
                w = np.zeros(0)
        elif isinstance(weights, str):
            if weights != "uniform":
                raise ValueError(f"TorsionFingerprint: weights={weights!r}; expected None, 'uniform' or one value per entry")
            w = np.ones(T)
        else:
            w = np.asarray(weights, dtype=np.float64).reshape(-1)
            if w.shape[0] != T:
                raise ValueError(f"TorsionFingerprint: {w.shape[0]} weights for {T} entries")
        return TorsionFingerprint(n, [(k, a, q, float(w[t]), md) for t, (k, a, q, md) in enumerate(found)], ligand_idx, symmetry)

    @staticmethod
    def from_batch(batch, bonds, bond_orders=None, **kw):
        """from a feature dict, as the other `from_batch` constructors: the ligand's atoms are those of `driver.ligand_atom_mask`, which
        become `ligand_idx`; bonds are pairs of LOCAL ligand indices"""
        from .driver import ligand_atom_mask
        lig = torch.nonzero(ligand_atom_mask(batch)).flatten()
        return TorsionFingerprint.from_bonds(int(lig.numel()), bonds, bond_orders, ligand_idx=lig, **kw)

    @staticmethod
    def from_sdf(record, **kw):
        """from one record of `sdfio.parse_sdf` (or the text of an SD file, whose first record is taken); a structure is then the record's
        atoms in file order.  The record must hold heavy atoms only: hydrogens are atoms of the graph like any other."""
        if isinstance(record, str):
            from .sdfio import parse_sdf
            record = parse_sdf(record)[0]
        return TorsionFingerprint.from_bonds(len(record["elements"]), record["bonds"], record["bond_orders"], **kw)

    # ------------------------------------------------------------------ description
    @property
    def symmetry_complete(self) -> bool:
        """False: the table was cut, every value is an upper bound"""
        return sides.symmetry_complete(self.symmetry)

    @property
    def n_perms(self) -> int:
        return 1 if self.symmetry is None else int(self.symmetry.n_perms)

    def describe(self, row) -> str:
        """a printable list of one row of `to_reference(...)["deviation"]` (anything with T values; read back here), worst entry first"""
        d = np.asarray(row.detach().cpu() if isinstance(row, torch.Tensor) else row, dtype=np.float64).reshape(-1)
        if d.shape[0] != self.n_entries:
            raise ValueError(f"TorsionFingerprint.describe: {d.shape[0]} values for {self.n_entries} entries")
        order = sorted(range(self.n_entries), key=lambda t: (-(d[t] if d[t] == d[t] else np.inf), t))
        lines = [f"{'entry':>5} {'kind':<4} {'dev':>6} {'degrees':>8} {'weight':>7}  atoms"]
        for t in order:
            e = self.entries[t]
            lines.append(f"{t:>5} {e.kind:<4} {d[t]:>6.3f} {d[t] * e.max_dev:>8.1f} {e.weight:>7.3f}  {'-'.join(str(a) for a in e.atoms)}")
        return "\n".join(lines)

    # ------------------------------------------------------------------ plumbing
    def tables(self, device):
        """the device tables (uploaded once per device): quads int32 [Q,4], image int16 storage [Nq,M], qstart int32 [T+1], w and
        inv_max_dev float64 [T], first int64 [n_bond_entries] (the first base quadruple of every rotatable-bond entry)"""
        def make(up):
            first = [int(self.qstart[t]) for t, e in enumerate(self.entries) if e.kind == "bond"]
            return dict(quads=up(self.quads), image=up(self.image.view(np.int16)), qstart=up(self.qstart),
                        w=up(np.array([e.weight for e in self.entries], dtype=np.float64)),
                        inv=up(np.array([1.0 / e.max_dev for e in self.entries], dtype=np.float64)),
                        first=up(np.array(first, dtype=np.int64)))
        return ops.cached_upload(self._dev, device, make)

    def _device_idx(self, idx, device):
        """idx on the device as int32; only the spec's own `ligand_idx` is cached (once per device)"""
        if idx is None:
            return None
        own = self.ligand_idx is not None and idx.shape[0] == len(self.ligand_idx) and bool((idx == sides.own_idx(self)).all())
        if not own:                                           # a caller's target_idx: uploaded for this call, not kept
            return torch.from_numpy(idx.astype(np.int32)).to(device)
        return ops.cached_upload(self._idx, device, lambda up: up(idx.astype(np.int32)))

    def _prepare(self, x, idx, want_angles=False):
        """x fp32 [n,A,3] on the device -> (ws float64 [n,Q] or None without entries, angles fp32 [n,Nq] or None)"""
        n, A = x.shape[0], x.shape[1]
        Q, Nq = int(self.quads.shape[0]), int(self.image.shape[0])
        if self.n_entries == 0:
            return None, (torch.empty(n, 0, dtype=torch.float32, device=x.device) if want_angles else None)
        L_ = ops._lib.init()
        t = self.tables(x.device)
        numel = L_.pd_torsion_workspace_numel(n, Q)
        ops.check(min(numel, 0), "pd_torsion_workspace_numel")
        ws = torch.empty(n, Q, dtype=torch.float64, device=x.device)
        ang = torch.empty(n, Nq, dtype=torch.float32, device=x.device) if want_angles else None
        with torch.cuda.device(x.device):
            ops.check(L_.pd_torsion_prepare(ops.ptr(x), ops.ptr(self._device_idx(idx, x.device)), ops.ptr(t["quads"]), ops.ptr(t["image"]),
                                            ops.ptr(ws), numel, ops.ptr(ang), n, A, self.n_atoms, Q, Nq, self.n_perms, ops.stream()),
                      "pd_torsion_prepare")
        return ws, ang

    def _tfd(self, ws_a, ws_b, na, nb, device, symmetric, detail):
        L_ = ops._lib.init()
        T, Q, Nq = self.n_entries, int(self.quads.shape[0]), int(self.image.shape[0])
        t = self.tables(device) if T else dict(qstart=None, w=None, inv=None, image=None)
        D = torch.empty(na, nb, dtype=torch.float32, device=device)
        bp = torch.empty(na, nb, dtype=torch.int32, device=device) if detail else None
        with torch.cuda.device(device):
            ops.check(L_.pd_torsion_tfd(ops.ptr(ws_a), ops.ptr(ws_b), ops.ptr(t["qstart"]), ops.ptr(t["w"]), ops.ptr(t["inv"]),
                                        ops.ptr(t["image"]), ops.ptr(D), ops.ptr(bp), na, nb, Q, T, Nq, self.n_perms,
                                        1 if symmetric else 0, ops.stream()), "pd_torsion_tfd")
        return D, bp

    # ------------------------------------------------------------------ the calls
    def angles(self, x: torch.Tensor) -> torch.Tensor:
        """x [P,A,3] -> fp32 [P,Nq] degrees in (-180, 180]: the dihedral of every base quadruple, entry after entry (entry t owns the
        columns `qstart[t]` .. `qstart[t+1]`-1; its quadruples are `entries[t].quads`); NaN where there is no angle"""
        ia = sides.own_idx(self)
        return self._prepare(sides.structures(x, "x", ia, self.n_atoms, **_WHO)[0], ia, True)[1]

    def entry_angles(self, x: torch.Tensor) -> torch.Tensor:
        """x [P,A,3] -> fp32 [P, number of rotatable-bond entries]: one representative angle per rotatable bond, that of its first
        quadruple (the smallest neighbour on either side)"""
        ang = self.angles(x)
        if self.n_entries == 0:
            return ang
        return ang[:, self.tables(ang.device)["first"]]

    def cross(self, x: torch.Tensor, targets: torch.Tensor, target_idx=None, detail: bool = False) -> Dict[str, torch.Tensor]:
        """x [n,A,3] (gathered through `ligand_idx`) against targets [C,A',3] gathered through `target_idx` - or through `ligand_idx`
        when they are whole poses - or [C,L,3] taken as they are -> `D` fp32 [n,C], `nearest` int64 [n] (the argmin over C: a NaN never
        wins, an all-NaN row gives -1, the smallest index wins a tie) and `nearest_tfd` fp32 [n] (NaN for such a row); with
        `detail=True` also `best_perm` int32 [n,C].  The rows are fixed, the targets permuted.  No result is read back; `target_idx` is a
        host list (a device tensor is copied to the host to be checked) and is uploaded per call."""
        xa, ia, xb, ib, _ = sides.sides(self, x, targets, target_idx, **_WHO)
        D, bp = self._tfd(self._prepare(xa, ia)[0], self._prepare(xb, ib)[0], xa.shape[0], xb.shape[0], xa.device, False, detail)
        near, near_v = sides.nearest(D)
        out = {"D": D, "nearest": near, "nearest_tfd": near_v}
        if detail:
            out["best_perm"] = bp
        return out

    def to_reference(self, x: torch.Tensor, x_ref: torch.Tensor) -> Dict[str, torch.Tensor]:
        """x [n,A,3] against the one reference x_ref [A,3] / [L,3] -> `tfd` fp32 [n], `best_perm` int32 [n], `deviation` fp32 [n,T] (the
        normalised deviation of every entry at the winning table row: which bond is wrong; NaN for an entry that names a missing angle
        and in a NaN row) and `worst_entry` int64 [n] (its argmax: a NaN never wins, the smallest entry on a tie, -1 without a finite
        value)"""
        if not isinstance(x_ref, torch.Tensor) or x_ref.dim() != 2 or x_ref.shape[1] != 3:
            raise ValueError(f"TorsionFingerprint.to_reference: x_ref must be [A,3], got {tuple(getattr(x_ref, 'shape', ()))}")
        xa, ia, xb, ib, _ = sides.sides(self, x, x_ref[None], None, **_WHO)
        n, dev, T = xa.shape[0], xa.device, self.n_entries
        ws_a, ws_b = self._prepare(xa, ia)[0], self._prepare(xb, ib)[0]
        D, bp = self._tfd(ws_a, ws_b, n, 1, dev, False, True)
        deviation = torch.empty(n, T, dtype=torch.float32, device=dev)
        if T:
            t = self.tables(dev)
            with torch.cuda.device(dev):
                ops.check(ops._lib.init().pd_torsion_deviation(ops.ptr(ws_a), ops.ptr(ws_b), ops.ptr(bp), ops.ptr(t["qstart"]),
                                                               ops.ptr(t["inv"]), ops.ptr(t["image"]), ops.ptr(deviation), n,
                                                               int(self.quads.shape[0]), T, int(self.image.shape[0]), self.n_perms,
                                                               ops.stream()), "pd_torsion_deviation")
            key = torch.where(torch.isnan(deviation), torch.full_like(deviation, -1.0), deviation)
            top = key.max(1, keepdim=True)[0]
            worst = (key == top).to(torch.int8).argmax(1)
            worst = torch.where(top[:, 0] < 0, torch.full_like(worst, -1), worst)
        else:
            worst = torch.full((n,), -1, dtype=torch.int64, device=dev)
        return {"tfd": D[:, 0], "best_perm": bp[:, 0], "deviation": deviation, "worst_entry": worst}

    def pairwise(self, x: torch.Tensor) -> torch.Tensor:
        """x [n,A,3] -> D fp32 [n,n], symmetric with an exact zero diagonal (NaN for a pose one of whose own angles is missing; pose i
        fixed, pose j permuted for i < j, mirrored); `PoseClusters.cluster` takes it as it is"""
        ia = sides.own_idx(self)
        xa = sides.structures(x, "x", ia, self.n_atoms, **_WHO)[0]
        return self._tfd(self._prepare(xa, ia)[0], None, xa.shape[0], xa.shape[0], xa.device, True, False)[0]


# ------------------------------------------------------------------ redock(torsions=)
def check_redock_torsions(torsions, batch) -> None:
    """redock(torsions=): raise ValueError unless it is a `TorsionFingerprint` over the batch's ligand atoms"""
    if torsions is None:
        return
    if not isinstance(torsions, TorsionFingerprint):
        raise ValueError(f"torsions= takes a torsions.TorsionFingerprint of the ligand, got {type(torsions).__name__}")
    from .driver import ligand_atom_mask
    n = int(ligand_atom_mask(batch).sum())
    if torsions.n_atoms != n:
        raise ValueError(f"torsions= was built over {torsions.n_atoms} ligand atoms, the batch's ligand holds {n}")


def score_torsions(torsions, aligned, batch, ligand_idx, pool=None) -> dict:
    """redock(torsions=): {"torsions": pairwise [n,n] (`pairwise` of the kept poses), with the ground truth to_gt [n] and deviation [n,T]
    (`to_reference` against `x_gt`) and, with a template pool [C,L,3], nearest_template / nearest_template_tfd [n] (`cross` with the
    pool)}.  A spec without `ligand_idx` is given the ligand atoms of the poses."""
    lig = ligand_idx.long()
    whole = torsions.ligand_idx is not None
    x = aligned if whole else aligned[:, lig]
    res = {"pairwise": torsions.pairwise(x)}
    if "x_gt" in batch:
        gt = batch["x_gt"].float()
        ref = torsions.to_reference(x, gt if whole else gt[lig])
        res["to_gt"], res["deviation"] = ref["tfd"], ref["deviation"]
    if pool is not None:
        near = torsions.cross(x, pool.to(aligned.device).float())
        res["nearest_template"], res["nearest_template_tfd"] = near["nearest"], near["nearest_tfd"]
    return {"torsions": res}
