"""Which ligands of a library are near-duplicates, which are closest to a known binder, which diverse few should be docked first?
`MorganFingerprint` holds the circular (Morgan / ECFP-like) fingerprints of a `LigandLibrary` on the device and compares them by
Tanimoto similarity (csrc/fingerprint.hip): the 2-D counterpart of `ShapeOverlap`, before anything is sampled.  The reference's
screening driver keys each ligand by the MD5 of its SMILES string (screening.py:100-103), so a molecule written two ways is docked
twice and nothing can be compared.

**The definition** is the package's own, after Rogers & Hahn 2010 (ECFP), **not RDKit's bytes**: tests/fingerprint_ref.py in Python
integers.  Hash arithmetic mod 2^32: `fmix(h)`: h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16 and
`push(h, v) = fmix(h * 0x01000193 + v + 0x9E3779B9)`.  Over heavy atoms:

    id_0(a)   push chained from 0 over Z, heavy degree, h_count, charge, in-ring (a bond of the atom is no bridge: `bond_in_ring` of
              `pd_ligand_features`) and the written-aromatic flag - or `atom_invariants[a]` as given (pharmacophore classes make an
              FCFP-like variant)
    id_r(a)   r = 1 .. radius: push chained from 0 over r, id_{r-1}(a) and the neighbours' pairs (twice the bond order, id_{r-1}) in
              ascending order - equal pairs are interchangeable, so the atom numbering does not matter.  Any degree.
    env_r(a)  the bonds within r steps of a: env_0 empty, env_r(a) = env_{r-1}(a) | union over neighbours b of (env_{r-1}(b) | a-b)
    kept      every radius-0 feature; (a, r), r >= 1, exactly when it is the first of all features of radius >= 1 with the same bond
              set in the order (r, id_r(a), a).  **An atom goes on iterating whether or not its feature was kept**; RDKit stops a
              "dead" atom, so the two differ beyond the hash.  (An atom without a bond keeps its radius-1 feature.)
    bits      a kept feature sets bit `id & (n_bits - 1)`; the 512-bit row is the OR-fold of the 2048-bit row

`radius` 0 .. 4 (default 2, the ECFP4 analogue), `n_bits` 512, 1024, 2048 or 4096.  Tanimoto: c common bits in a union of u give
the IEEE fp32 quotient `float(c) / float(u)`; **an empty union gives 1.0**, as `InteractionFingerprint.pairwise` (`pd_plif_pairwise`)
does for two empty rows.  `nearest` and `maxmin` order by the exact fraction (integer cross-multiplication), never by the fp32 value.

**Caveats.**  Kekule and aromatic spellings of one molecule differ (`c1ccccc1` against `C1=CC=CC=C1`) unless `aromatize=True`
perceives aromaticity first, by the package's own rules.  No chirality in the invariants (the `@` code depends on the written
neighbour order), no count vectors (ECFC); the pharmacophore classes of an FCFP-like variant come from
`substructure.pharmacophore_invariants`, an int32 device tensor that `atom_invariants` takes without a read-back.  Similarity 1 with equal atom counts is necessary for two
ligands to be the same molecule, not sufficient: this is no canonical key.  Limits: 128 atoms and 512 bonds per ligand, 65535
ligands per launch, 1 <= k <= 16.  Out of scope: RDKit parity, `redock`; substructure search is `substructure.py`
(`LigandLibrary.substructure`).

Device tensors hold the uint32 words as int32 (the same bits; `.view(torch.uint32)` is free): torch computes on int32."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops

__all__ = ["MorganFingerprint", "N_BITS", "MAX_RADIUS", "MAX_K", "morgan_fingerprint"]

N_BITS = (512, 1024, 2048, 4096)
MAX_RADIUS, MAX_K = 4, 16
MAX_ROWS = 65535 * 16


def _check_spec(radius, n_bits, what):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"{what}: radius {radius!r}; an integer in 0 .. {MAX_RADIUS}")
    if isinstance(n_bits, bool) or not isinstance(n_bits, (int, np.integer)) or int(n_bits) not in N_BITS:
        raise ValueError(f"{what}: n_bits {n_bits!r}; one of {N_BITS}")
    return int(radius), int(n_bits)


def _invariants(atom_invariants, n_atoms, what) -> Optional[np.ndarray]:
    """`atom_invariants` as uint32 [n_atoms] held in int32 (a numpy array, or the int32 device tensor that was given), or None"""
    if atom_invariants is None:
        return None
    if isinstance(atom_invariants, torch.Tensor) and atom_invariants.is_cuda and atom_invariants.dtype == torch.int32:
        if atom_invariants.dim() != 1 or atom_invariants.shape[0] != n_atoms:
            raise ValueError(f"{what}: atom_invariants of shape {tuple(atom_invariants.shape)}; one value per atom of the library "
                             f"({n_atoms},)")
        return atom_invariants.detach().contiguous()         # the uint32 values as int32 on the device: taken without a read-back
    if isinstance(atom_invariants, torch.Tensor):
        atom_invariants = atom_invariants.detach().cpu().numpy()
    v = np.asarray(atom_invariants)
    if v.ndim != 1 or v.shape[0] != n_atoms:
        raise ValueError(f"{what}: atom_invariants of shape {tuple(v.shape)}; one value per atom of the library ({n_atoms},)")
    if v.dtype.kind not in "iu":
        raise ValueError(f"{what}: atom_invariants must be integers, got {v.dtype}")
    return (v.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def morgan_fingerprint(library, radius=2, n_bits=2048, atom_invariants=None, aromatize=False, device=None) -> "MorganFingerprint":
    """`LigandLibrary.fingerprints`: ONE launch of `pd_morgan_fingerprint` for the whole library (two with `aromatize=True`, which
    runs `pd_aromaticity` in the mode "normalise" first and fingerprints its tables, as `features(aromatize=True)` does); nothing is
    read back.  Every check is made on the host before the first launch."""
    from .ligand import _device
    what = "LigandLibrary.fingerprints"
    radius, n_bits = _check_spec(radius, n_bits, what)
    inv = _invariants(atom_invariants, library.n_atoms, what)
    device = _device(device)
    t = library.tables(device)
    status = None
    if aromatize:
        perceived = library.aromaticity("normalise", device=device)
        t = dict(t, atoms=perceived["atoms"], bonds=perceived["bonds"])
        status = perceived["status"]
    G, N, B, W = library.n_ligands, library.n_atoms, library.n_bonds, n_bits // 32
    new = lambda shape, dtype: torch.empty(shape, device=device, dtype=dtype)
    bits, ids, kept = new((G, W), torch.int32), new((N, radius + 1), torch.int32), new((N, radius + 1), torch.uint8)
    n_features, popcount = new((G,), torch.int32), new((G,), torch.int32)
    if isinstance(inv, torch.Tensor):
        if inv.device != device:
            raise ValueError(f"{what}: atom_invariants on {inv.device}, the fingerprints on {device}")
        inv_t = inv
    else:
        inv_t = torch.from_numpy(inv.copy()).to(device) if inv is not None else None
    L_ = ops._lib.init()
    with torch.cuda.device(device):
        ops.check(L_.pd_morgan_fingerprint(ops.ptr(t["atom_start"]), ops.ptr(t["bond_start"]), ops.ptr(t["atoms"]),
                                           ops.ptr(t["bonds"]) if B else None, ops.ptr(inv_t), ops.ptr(bits), ops.ptr(ids), ops.ptr(kept),
                                           ops.ptr(n_features), ops.ptr(popcount), G, N, B, radius, n_bits, ops.stream()),
                  "pd_morgan_fingerprint")
    return MorganFingerprint(bits, radius, n_bits, ids=ids, kept=kept, n_features=n_features, popcount=popcount,
                             aromaticity_status=status, atom_start=library.atom_start)


class MorganFingerprint:
    """Immutable: `bits` int32 [G, n_bits/32] (the uint32 words), `radius`, `n_bits`, `n_ligands`, and - from `LigandLibrary.
    fingerprints` - `ids` int32 [N, radius+1] (uint32 identifiers), `kept` uint8 [N, radius+1], `n_features` int32 [G] (the kept
    features), `popcount` int32 [G], `aromaticity_status` int32 [G] with `aromatize=True`, else None.  `from_bits` wraps rows from
    elsewhere; it has `bits` only.  Every method returns device tensors and reads nothing back, except `explain`."""

    __slots__ = ("bits", "radius", "n_bits", "n_ligands", "ids", "kept", "n_features", "popcount", "aromaticity_status", "_atom_start")

    def __init__(self, bits, radius, n_bits, ids=None, kept=None, n_features=None, popcount=None, aromaticity_status=None,
                 atom_start=None):
        set_ = lambda k, v: object.__setattr__(self, k, v)
        set_("bits", bits); set_("radius", radius); set_("n_bits", int(n_bits)); set_("n_ligands", int(bits.shape[0]))
        set_("ids", ids); set_("kept", kept); set_("n_features", n_features); set_("popcount", popcount)
        set_("aromaticity_status", aromaticity_status); set_("_atom_start", atom_start)

    def __setattr__(self, name, value):
        raise AttributeError("MorganFingerprint is immutable")

    def __repr__(self):
        return f"MorganFingerprint(n_ligands={self.n_ligands}, radius={self.radius}, n_bits={self.n_bits})"

    def __len__(self):
        return self.n_ligands

    @staticmethod
    def from_bits(bits, device=None) -> "MorganFingerprint":
        """rows of bits from elsewhere: an integer array or tensor [G, W] of 32-bit words, W = 16, 32, 64 or 128 (bit k of a row is bit
        k % 32 of word k // 32).  `radius` is None."""
        from .ligand import _device
        if isinstance(bits, torch.Tensor):
            if bits.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                raise ValueError(f"MorganFingerprint.from_bits: a tensor of int32 or uint32 words, got {bits.dtype}")
            t = bits.view(torch.int32) if bits.dtype != torch.int32 else bits
        else:
            v = np.asarray(bits)
            if v.dtype.kind not in "iu" or (v.size and (v.min() < -2 ** 31 or v.max() >= 2 ** 32)):
                raise ValueError(f"MorganFingerprint.from_bits: 32-bit integer words, got {v.dtype}")
            t = torch.from_numpy((v.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
        if t.dim() != 2 or t.shape[0] < 1 or 32 * t.shape[1] not in N_BITS:
            raise ValueError(f"MorganFingerprint.from_bits: rows of {tuple(t.shape)}; [G >= 1, n_bits / 32] with n_bits one of {N_BITS}")
        if t.shape[0] > MAX_ROWS:
            raise ValueError(f"MorganFingerprint.from_bits: {t.shape[0]} rows; up to {MAX_ROWS} are taken")
        if not t.is_cuda or device is not None:
            t = t.to(_device(device))
        return MorganFingerprint(t.contiguous(), None, 32 * t.shape[1])

    # ------------------------------------------------------------------ comparisons
    def _other(self, other, what) -> "MorganFingerprint":
        if not isinstance(other, MorganFingerprint):
            raise ValueError(f"MorganFingerprint.{what}: the other side must be a MorganFingerprint, got {type(other).__name__}")
        if other.n_bits != self.n_bits:
            raise ValueError(f"MorganFingerprint.{what}: {self.n_bits} bits against {other.n_bits}")
        if other.bits.device != self.bits.device:
            raise ValueError(f"MorganFingerprint.{what}: rows on {self.bits.device} against rows on {other.bits.device}")
        return other

    def cross(self, other: "MorganFingerprint", common: bool = False):
        """Tanimoto similarity of every row against every row of `other` -> fp32 [n, m]; with `common=True` (similarity, common int32
        [n, m]).  One launch of `pd_fingerprint_tanimoto`."""
        other = self._other(other, "cross")
        n, m, dev = self.n_ligands, other.n_ligands, self.bits.device
        sim = torch.empty(n, m, device=dev, dtype=torch.float32)
        com = torch.empty(n, m, device=dev, dtype=torch.int32) if common else None
        L_ = ops._lib.init()
        with torch.cuda.device(dev):
            ops.check(L_.pd_fingerprint_tanimoto(ops.ptr(self.bits), ops.ptr(other.bits), ops.ptr(sim), ops.ptr(com), n, m,
                                                 self.n_bits // 32, ops.stream()), "pd_fingerprint_tanimoto")
        return (sim, com) if common else sim

    def pairwise(self) -> torch.Tensor:
        """`cross(self)`: symmetric, with a unit diagonal (a row without a bit included).  `1 - pairwise()` is a distance matrix that
        `PoseClusters.cluster` takes as it is, for up to 8192 ligands."""
        return self.cross(self)

    def _nearest(self, other, k, exclude_self, what) -> Dict[str, torch.Tensor]:
        other = self._other(other, what)
        n, m, dev = self.n_ligands, other.n_ligands, self.bits.device
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K:
            raise ValueError(f"MorganFingerprint.{what}: k {k!r}; an integer in 1 .. {MAX_K}")
        if int(k) > m - int(exclude_self):
            raise ValueError(f"MorganFingerprint.{what}: k {int(k)} of {m - int(exclude_self)} rows to choose from")
        k = int(k)
        out = {"index": torch.empty(n, k, device=dev, dtype=torch.int32), "similarity": torch.empty(n, k, device=dev, dtype=torch.float32),
               "common": torch.empty(n, k, device=dev, dtype=torch.int32)}
        L_ = ops._lib.init()
        with torch.cuda.device(dev):
            ops.check(L_.pd_fingerprint_nearest(ops.ptr(self.bits), ops.ptr(other.bits), ops.ptr(out["index"]), ops.ptr(out["similarity"]),
                                                ops.ptr(out["common"]), n, m, self.n_bits // 32, k, int(exclude_self), ops.stream()),
                      "pd_fingerprint_nearest")
        return out

    def nearest(self, other: "MorganFingerprint", k: int = 1) -> Dict[str, torch.Tensor]:
        """for each row the `k` most similar rows of `other`, best first -> `index` int32 [n, k], `similarity` fp32 [n, k], `common`
        int32 [n, k].  Ordered by the exact fraction, the smaller index of `other` on a tie; n x m is never stored.  One launch."""
        return self._nearest(other, k, False, "nearest")

    def neighbours(self, k: int) -> Dict[str, torch.Tensor]:
        """`nearest` on itself without the row itself: the pairwise use"""
        return self._nearest(self, k, True, "neighbours")

    def maxmin(self, n_pick: int, first: int = 0) -> Dict[str, torch.Tensor]:
        """A diverse subset by MaxMin (Ashton et al. 2002, RDKit's MaxMinPicker) without the matrix: `picks[0] = first`, then each
        time the unpicked row with the largest min over the picked rows of 1 - T (exact fractions, the smallest index on a tie)
        -> `picks` int32 [n_pick], `max_similarity` fp32 [n_pick]: each pick's largest similarity to the earlier picks, NaN for the
        first.  1 + 2 (n_pick - 1) small launches - per pick one that lowers every row's running minimum against the newest pick and
        one that selects - and the next pick stays on the device."""
        n, dev = self.n_ligands, self.bits.device
        for name, v, lo, hi in (("n_pick", n_pick, 1, n), ("first", first, 0, n - 1)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"MorganFingerprint.maxmin: {name} {v!r}; an integer in {lo} .. {hi} for {n} rows")
        L_ = ops._lib.init()
        numel = L_.pd_fingerprint_maxmin_workspace_numel(n)
        ops.check(min(numel, 0), "pd_fingerprint_maxmin_workspace_numel")
        ws = torch.empty(numel, device=dev, dtype=torch.int32)
        out = {"picks": torch.empty(int(n_pick), device=dev, dtype=torch.int32),
               "max_similarity": torch.empty(int(n_pick), device=dev, dtype=torch.float32)}
        with torch.cuda.device(dev):
            ops.check(L_.pd_fingerprint_maxmin(ops.ptr(self.bits), ops.ptr(ws), numel, ops.ptr(out["picks"]), ops.ptr(out["max_similarity"]),
                                               n, self.n_bits // 32, int(n_pick), int(first), ops.stream()), "pd_fingerprint_maxmin")
        return out

    # ------------------------------------------------------------------ the one read-back
    def explain(self, g: int, bit: int) -> List[Tuple[int, int, int]]:
        """the kept features (atom, radius, id) of ligand g that set `bit`, the atom local to the ligand; reads `ids` and `kept` of
        that ligand back"""
        if self.ids is None or self._atom_start is None:
            raise ValueError("MorganFingerprint.explain: rows from `from_bits` carry no features")
        if not 0 <= int(g) < self.n_ligands or not 0 <= int(bit) < self.n_bits:
            raise ValueError(f"MorganFingerprint.explain: ligand {g}, bit {bit}; {self.n_ligands} ligands of {self.n_bits} bits")
        a0, a1 = int(self._atom_start[int(g)]), int(self._atom_start[int(g) + 1])
        ids = self.ids[a0:a1].cpu().numpy().view(np.uint32)
        kept = self.kept[a0:a1].cpu().numpy()
        return [(int(a), int(r), int(ids[a, r])) for a, r in zip(*np.nonzero(kept)) if int(ids[a, r]) & (self.n_bits - 1) == int(bit)]
