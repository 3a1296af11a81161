"""lDDT-PLI: are the ligand's contacts with its pocket reproduced?  Symmetry-aware, for every pose, on the device (kernels
`pd_lddt_pli_counts` / `pd_lddt_pli_select`, csrc/lddt_pli.hip).

The measure of the CASP15 ligand assessment, as OpenStructure computes it and PLINDER reports it.  For every ligand atom i take
the receptor atoms within `radius` (6 A) of it in the ground truth, N(i), with their distances d_gt(i,j) there.  For a pose x, a
candidate atom k and a threshold t

    c_t(i,k) = #{ j in N(i) : | |x[lig[k]] - x[j]| - d_gt(i,j) | < t },          t in (0.5, 1, 2, 4) A

and for a row m of the ligand's automorphism table C_t(m) = sum_i c_t(i, perms[m][i]).  The chosen row m* is the smallest m that
maximises sum_t C_t(m), and

    lddt_pli = sum_t C_t(m*) / (4 sum_i |N(i)|)                                    (0 when there is no contact)

It needs no superposition: the model predicts the whole complex, so a pose is scored as it is.  A ligand atom that is masked out
in the ground truth has no contacts; the receptor is every pose atom of the mask that is not a ligand atom.  This is the classic
form: the "added model contacts" penalty of newer OpenStructure releases (contacts the model has and the ground truth has not)
is NOT applied.  Out of scope as well: pose-versus-pose lDDT and ligand - ligand contacts.

`LddtPli` holds one system's tables, built once on the host in float64 numpy - `x_gt` is fixed per system, as the tables of
`PoseValidity` are.  `score(x_pred)` returns device tensors and never synchronises; `ranking.rank_poses(..., lddt_pli=)` and
`driver.redock(..., lddt_pli=)` report it beside the ligand RMSD.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import ops
from .scoring import _host
from .symmetry import MAX_ATOMS, MAX_PERMS

__all__ = ["LddtPli", "DEFAULT_RADIUS", "DEFAULT_THRESHOLDS", "MAX_ATOMS", "MAX_PERMS", "MAX_CONTACTS", "CONTACT_TILE", "LDS_CANDIDATES"]

DEFAULT_RADIUS = 6.0
DEFAULT_THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
#: limits and shapes of the kernels (PD_LDDT_PLI_* of include/physdock_hip.h): an atom's contacts are taken CONTACT_TILE at a
#: time; the selection keeps the totals of up to LDS_CANDIDATES candidates in LDS and reads them from global memory beyond
MAX_CONTACTS, CONTACT_TILE, LDS_CANDIDATES = (1 << 29) - 1, 512, 4096

_TABLES = ("ligand_idx", "contact_start", "contact_atom", "contact_dist", "cand_start", "cand_atom", "slot_t")


class LddtPli:
    """One system's tables for the lDDT-PLI kernels.  Host copies (numpy): `ligand_idx` int32 [L]; the contacts in CSR form -
    `contact_start` int32 [L+1], `contact_atom` int32 (pose atom, ascending per ligand atom), `contact_dist` fp32; the candidate
    images of every ligand atom in CSR form - `cand_start` int32 [L+1], `cand_atom` int32 (the distinct `perms[:, i]`, ascending);
    `slot_t` uint16 [L, M], atom-major as `LigandSymmetry.table`: `cand_atom[cand_start[i] + slot_t[i, m]] == perms[m, i]`; and
    `perms` int32 [M, L], `atom_contacts` int32 [L] (|N(i)|), `n_contacts`, `n_candidates`, `radius`, `thresholds`,
    `symmetry_complete` (False: the automorphism table was cut, every score is a LOWER bound).  `n_atoms` is the ligand's atom
    count L, `n_pose_atoms` the A of the poses `score` takes."""

    def __init__(self, tables: Dict[str, np.ndarray], perms: np.ndarray, n_pose_atoms: int, radius: float, thresholds, complete: bool,
                 device=None):
        self.__dict__.update(tables)
        self.perms = perms
        self.n_atoms, self.n_perms, self.n_pose_atoms = int(perms.shape[1]), int(perms.shape[0]), int(n_pose_atoms)
        self.atom_contacts = np.diff(self.contact_start).astype(np.int32)
        self.n_contacts, self.n_candidates = int(self.contact_start[-1]), int(self.cand_start[-1])
        self.radius, self.thresholds, self.symmetry_complete = float(radius), tuple(float(t) for t in thresholds), bool(complete)
        self._tables = {}
        if device is not None:
            self.tables(device)

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_arrays(x_gt, ligand_idx, receptor_mask, symmetry=None, radius: float = DEFAULT_RADIUS,
                    thresholds: Sequence[float] = DEFAULT_THRESHOLDS, device=None, ligand_mask=None):
        """x_gt [A,3]: the ground truth; ligand_idx [L]: the ligand's atoms in a pose; receptor_mask [A] (> 0: the atom exists and
        may count as receptor; ligand atoms never do, whatever the mask says); symmetry: a `symmetry.LigandSymmetry` over the L
        ligand atoms in the order of ligand_idx (None: the identity alone); ligand_mask [L] (default: all): 0 = the ligand atom is
        masked out in the ground truth and has no contacts.  `thresholds`: exactly four."""
        x = _host(x_gt, np.float64)
        lig = _host(ligand_idx, np.int64).reshape(-1)
        rec = _host(receptor_mask, np.float64).reshape(-1) > 0
        if x.ndim != 2 or x.shape[1] != 3 or x.shape[0] < 1:
            raise ValueError(f"LddtPli: x_gt must have shape [A,3], got {tuple(x.shape)}")
        A, L = int(x.shape[0]), int(lig.shape[0])
        if rec.shape[0] != A:
            raise ValueError(f"LddtPli: x_gt holds {A} atoms, receptor_mask {rec.shape[0]}")
        if not 1 <= L <= MAX_ATOMS:
            raise ValueError(f"LddtPli: {L} ligand atoms; the kernels take 1 .. {MAX_ATOMS}")
        if lig.min() < 0 or lig.max() >= A or len(set(lig.tolist())) != L:
            raise ValueError(f"LddtPli: ligand_idx must hold {L} distinct atom indices below {A}")
        thresholds = tuple(float(t) for t in thresholds)
        if len(thresholds) != 4 or any(not t > 0 for t in thresholds) or not float(radius) > 0:
            raise ValueError(f"LddtPli: exactly four positive thresholds and a positive radius, got {thresholds} and {radius}")
        if symmetry is None:
            perms, complete = np.arange(L, dtype=np.int32)[None], True
        else:
            if symmetry.n_atoms != L:
                raise ValueError(f"LddtPli: symmetry is a table over {symmetry.n_atoms} atoms, ligand_idx holds {L}")
            perms, complete = np.asarray(symmetry.perms, dtype=np.int32), bool(symmetry.complete)
        M = int(perms.shape[0])
        if M > MAX_PERMS:
            raise ValueError(f"LddtPli: {M} permutations; the kernels take up to {MAX_PERMS}")
        active = np.ones(L, dtype=bool) if ligand_mask is None else _host(ligand_mask, np.float64).reshape(-1) > 0
        if active.shape[0] != L:
            raise ValueError(f"LddtPli: ligand_idx holds {L} atoms, ligand_mask {active.shape[0]}")
        # contacts: receptor atoms within the radius of each ligand atom in the ground truth (float64), ascending
        rec = rec.copy()
        rec[lig] = False
        rec_idx = np.nonzero(rec)[0]
        atoms, dists, start = [], [], np.zeros(L + 1, dtype=np.int64)
        for i in range(L):
            d = np.sqrt(((x[rec_idx] - x[lig[i]]) ** 2).sum(-1))
            near = (d < float(radius)) & active[i]
            atoms.append(rec_idx[near]); dists.append(d[near])
            start[i + 1] = start[i] + int(near.sum())
        if start[-1] > MAX_CONTACTS:
            raise ValueError(f"LddtPli: {int(start[-1])} contacts; the kernels take up to {MAX_CONTACTS}")
        contact_atom, contact_dist = np.concatenate(atoms).astype(np.int32), np.concatenate(dists).astype(np.float32)
        # candidates: the distinct images of each ligand atom, and where each table row's image sits among them
        cand, cand_start, slot_t = [], np.zeros(L + 1, dtype=np.int64), np.empty((L, M), dtype=np.uint16)
        for i in range(L):
            images, slot = np.unique(perms[:, i], return_inverse=True)
            cand.append(images)
            cand_start[i + 1] = cand_start[i] + len(images)
            slot_t[i] = slot.reshape(-1)
        tables = dict(ligand_idx=lig.astype(np.int32), contact_start=start.astype(np.int32), contact_atom=contact_atom,
                      contact_dist=contact_dist, cand_start=cand_start.astype(np.int32), cand_atom=np.concatenate(cand).astype(np.int32),
                      slot_t=np.ascontiguousarray(slot_t))
        return LddtPli(tables, perms, A, radius, thresholds, complete, device)

    @staticmethod
    def from_batch(batch, symmetry=None, **kw):
        """from a feature dict: the ground truth is `x_gt`, the ligand's atoms are those of `driver.ligand_atom_mask`, an atom
        exists where `a_mask > 0` and, when the batch has one, `x_exists > 0`; the receptor is every existing atom that is not a
        ligand atom.  The tables are uploaded to the batch's device.  Other keywords as for `from_arrays`."""
        from .driver import ligand_atom_mask
        is_lig = ligand_atom_mask(batch)
        lig = torch.nonzero(is_lig).flatten()
        exists = torch.ones_like(is_lig)
        for k in ("a_mask", "x_exists"):
            if k in batch:
                exists = exists & (batch[k].reshape(-1) > 0)
        dev = batch["x_gt"].device
        kw.setdefault("device", dev if dev.type == "cuda" else None)
        kw.setdefault("ligand_mask", exists[lig])
        return LddtPli.from_arrays(batch["x_gt"], lig, exists & ~is_lig, symmetry, **kw)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernels' tables on `device` (uploaded once; slot_t as int16 storage of its unsigned 16-bit entries)"""
        def make(up):
            t = {k: up(getattr(self, k)) for k in _TABLES if k != "slot_t"}
            t["slot_t"] = up(self.slot_t.view(np.int16))
            t["atom_contacts"] = up(self.atom_contacts)
            return t
        return ops.cached_upload(self._tables, device, make)

    def score(self, x_pred: torch.Tensor) -> dict:
        """x_pred [P,A,3] (device) -> dict of device tensors: lddt_pli [P] fp32; conserved [P,4] int32 (the chosen permutation's
        conserved contacts per threshold); per_atom [P,L] fp32 (its conserved share of each ligand atom's contacts, 0 for an atom
        without contacts); best_perm [P] int32 (the chosen row of the automorphism table) - and n_contacts (int), atom_contacts
        [L] int32 (device), symmetry_complete (False: the scores are lower bounds).  Nothing is read back, nothing synchronises."""
        if x_pred.dim() != 3 or x_pred.shape[1] != self.n_pose_atoms or x_pred.shape[2] != 3:
            raise ValueError(f"LddtPli.score: the tables are over {self.n_pose_atoms} pose atoms, x_pred has shape {tuple(x_pred.shape)}")
        L_ = ops._lib.init()
        x = x_pred.float().contiguous()
        P, A, L, nc = x.shape[0], x.shape[1], self.n_atoms, self.n_candidates
        t = self.tables(x.device)
        counts = torch.empty(P, nc, 4, dtype=torch.int32, device=x.device)
        lddt = torch.empty(P, device=x.device)
        conserved = torch.empty(P, 4, dtype=torch.int32, device=x.device)
        per_atom = torch.empty(P, L, device=x.device)
        best = torch.empty(P, dtype=torch.int32, device=x.device)
        ptr = lambda k, n=1: ops.ptr(t[k]) if n else None
        ops.check(L_.pd_lddt_pli_counts(ops.ptr(x), ptr("ligand_idx"), ptr("contact_start"), ptr("contact_atom", self.n_contacts),
                                        ptr("contact_dist", self.n_contacts), ptr("cand_start"), ptr("cand_atom"), *self.thresholds,
                                        ops.ptr(counts), P, A, L, self.n_contacts, nc, ops.stream()), "pd_lddt_pli_counts")
        ops.check(L_.pd_lddt_pli_select(ops.ptr(counts), ptr("contact_start"), ptr("cand_start"), ptr("slot_t"), ops.ptr(lddt),
                                        ops.ptr(conserved), ops.ptr(per_atom), ops.ptr(best), P, L, self.n_perms, nc, ops.stream()),
                  "pd_lddt_pli_select")
        return {"lddt_pli": lddt, "conserved": conserved, "per_atom": per_atom, "best_perm": best, "n_contacts": self.n_contacts,
                "atom_contacts": t["atom_contacts"], "symmetry_complete": self.symmetry_complete}

    def __repr__(self):
        return (f"LddtPli(n_atoms={self.n_atoms}, n_pose_atoms={self.n_pose_atoms}, n_contacts={self.n_contacts}, "
                f"n_perms={self.n_perms}, n_candidates={self.n_candidates}, symmetry_complete={self.symmetry_complete})")
