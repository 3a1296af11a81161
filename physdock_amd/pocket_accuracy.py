"""Did the model draw the right POCKET?  The lDDT of the ligand pocket (lDDT-LP) and the pocket RMSDs of every pose against the ground
truth, on the device (kernel `pd_pocket_accuracy`, csrc/pocket_accuracy.hip).

The model co-folds: every pose carries its own receptor, and `rank_poses`, `BestFitRmsd` and `LddtPli` judge the LIGAND against the
ground truth while `ReceptorGeometry` judges the receptor for plausibility only.  Co-folding benchmarks (OpenStructure's ligand
scoring, the CASP15 assessment, PLINDER) report the accuracy of the pocket beside them.  This is the package's OWN definition of the
two measures - tests/pocket_accuracy_ref.py is its written form - and does not reproduce OpenStructure's bytes.

Per system, in float64 on the host: the receptor is every existing heavy atom that is not a ligand atom; a pocket residue has a
receptor atom closer than `pocket_radius` (8 A: this package's default, not validated) to an existing ligand atom of the reference;
every atom i of a pocket residue is paired with every receptor atom j of ANOTHER residue with d_ref(i,j) < `inclusion_radius` (15 A,
the published lDDT radius).  No pair inside a residue, none with a ligand atom (those are `LddtPli`'s).  Per pose, with float64
distances from the fp32 coordinates, a pair is conserved at t in (0.5, 1, 2, 4) A when | |p_i - p_j| - d_ref | < t, and

    lddt_lp = sum_t C_t / (4 n_pairs)                                                (0 without pairs; the same per pocket residue)

The names ASP OD1/OD2, GLU OE1/OE2, ARG NH1/NH2, LEU CD1/CD2, VAL CG1/CG2 and PHE / TYR CD1/CD2 with CE1/CE2 are interchangeable: for
every pocket residue that has them all, the conserved (pair, threshold) entries of its atoms' rows are counted as given and with the
names exchanged in the pose - every other residue as given - and the residue is swapped only when the second count is strictly
greater; then everything is counted once more with all chosen swaps applied, on both sides of every pair.  Swaps are decided for
pocket residues only, each against its neighbours as given.

The fit: the pose's pocket CA atoms are superposed on the reference's with a PROPER rotation (Horn's quaternion, the float64 cyclic
Jacobi of csrc/geom3.h; a mirrored pocket does not fit).  `ca_rmsd` is their RMSD, and under that one transform `backbone_rmsd` (N, CA,
C, O), `heavy_rmsd` (all pocket atoms, swaps applied) and `residue_rmsd` (per pocket residue: which side chain is wrong); `quat` and `t`
carry a pose into the reference's frame, x' = R(quat) x + t.  With fewer than 3 pocket CA atoms, or CA atoms on a line, `fit_ok` = 0 and
RMSDs and transform are NaN; the lDDT is not affected.  A pose with a non-finite coordinate on an atom the tables name has `ok` = 0, NaN
floats and zero integers.

Heavy atoms only.  Limits: 4096 pose atoms, 1024 pocket residues, 65535 poses.  Out of scope: nucleic acids, the "added contacts" penalty
of newer OpenStructure releases, feeding the swaps into `ReceptorGeometry.chi_recovery`, several systems per launch.

`PocketAccuracy` is an immutable spec of one system; `score(x_pred)` returns device tensors and reads nothing back, `describe` is the one
read-back.  `driver.redock(..., pocket_accuracy=)` reports it for the kept poses.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .scoring import _host

__all__ = ["PocketAccuracy", "swap_table_from_names", "SWAP_NAMES", "BACKBONE_NAMES", "DEFAULT_POCKET_RADIUS", "DEFAULT_INCLUSION_RADIUS",
           "DEFAULT_THRESHOLDS", "MAX_ATOMS", "MAX_RESIDUES", "MAX_POSES", "PAIR_TILE"]

DEFAULT_POCKET_RADIUS, DEFAULT_INCLUSION_RADIUS = 8.0, 15.0
DEFAULT_THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
#: limits and the tile of the kernels (PD_POCKET_ACCURACY_* of include/physdock_hip.h)
MAX_ATOMS, MAX_RESIDUES, MAX_POSES, PAIR_TILE = 4096, 1024, 65535, 256
MAX_PAIRS = (1 << 31) - 1
#: the interchangeable atom names of a residue; all pairs of one residue swap together
SWAP_NAMES = {"ASP": (("OD1", "OD2"),), "GLU": (("OE1", "OE2"),), "ARG": (("NH1", "NH2"),), "LEU": (("CD1", "CD2"),),
              "VAL": (("CG1", "CG2"),), "PHE": (("CD1", "CD2"), ("CE1", "CE2")), "TYR": (("CD1", "CD2"), ("CE1", "CE2"))}
BACKBONE_NAMES = ("N", "CA", "C", "O")
KIND_CA, KIND_BACKBONE = 1, 2
_CHUNK = 256                        # rows of a distance search held at a time

_DEVICE_KEYS = ("patom", "patom_partner", "patom_kind", "patom_ref", "res_atom_start", "pair_start", "pair_atom", "pair_dist",
                "atom_partner", "atom_slot", "named", "pocket_residues")


def _residue_atoms(res_names, atom_names, residue_of, mask, what):
    res = _host(residue_of, np.int64).reshape(-1)
    n = res.shape[0]
    if not len(res_names) == len(atom_names) == n:
        raise ValueError(f"{what}: {len(res_names)} residue names, {len(atom_names)} atom names, {n} residue ids")
    ok = np.ones(n, dtype=bool) if mask is None else _host(mask, np.float64).reshape(-1) > 0
    if ok.shape[0] != n:
        raise ValueError(f"{what}: {n} atoms, a mask of {ok.shape[0]}")
    atoms: Dict[int, Dict[str, int]] = {}
    kind: Dict[int, str] = {}
    for a in range(n):
        if ok[a]:
            atoms.setdefault(int(res[a]), {}).setdefault(str(atom_names[a]).strip().upper(), a)
            kind.setdefault(int(res[a]), str(res_names[a]).strip().upper())
    return res, ok, atoms, kind


def swap_table_from_names(res_names: Sequence[str], atom_names: Sequence[str], residue_of, mask=None) -> np.ndarray:
    """The atom pairs whose names are interchangeable, int32 [n,2] of indices into the arguments, ascending in the residue id: the
    `SWAP_NAMES` of every residue (atoms with equal `residue_of`; `mask` [n], default all: 0 = the atom does not exist).  PHE and TYR
    give two pairs, which swap together.  A residue with one of those atoms missing gives none."""
    _, _, atoms, kind = _residue_atoms(res_names, atom_names, residue_of, mask, "swap_table_from_names")
    out = []
    for r in sorted(atoms):
        pairs = SWAP_NAMES.get(kind[r], ())
        if pairs and all(a in atoms[r] and b in atoms[r] for a, b in pairs):
            out += [(atoms[r][a], atoms[r][b]) for a, b in pairs]
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


class PocketAccuracy:
    """One system's tables for `pd_pocket_accuracy`, immutable.  Host copies (numpy, read-only): `pocket_residues` int32 [Rp] (the
    residue ids, ascending); the Np pocket atoms by (pocket residue, atom) - `patom` int32 [Np] (pose atom), `patom_partner` int32 [Np]
    (the pose atom it exchanges its name with, itself for none), `patom_kind` uint8 [Np] (bit 0 CA, bit 1 backbone), `patom_ref`
    float64 [Np,3], `res_atom_start` int32 [Rp+1]; the pairs in CSR form over the pocket atoms - `pair_start` int32 [Np+1], `pair_atom`
    int32 (pose atom, ascending per row), `pair_dist` float64; `atom_partner` and `atom_slot` int32 [A] (per pose atom: the partner, and
    the place of its residue in `pocket_residues` or -1); `named` int32 (every pose atom a table names); `swaps` int32 [n,2] (the kept
    swap pairs), `swappable` bool [Rp], `residue_pairs` int32 [Rp]; `n_pose_atoms` A, `n_pocket_residues` Rp, `n_pocket_atoms` Np,
    `n_pairs`, `n_ca`, `pocket_radius`, `inclusion_radius`, `thresholds`, `residue_labels` (one per pocket residue)."""

    def __init__(self, tables: Dict[str, np.ndarray], n_pose_atoms: int, pocket_radius: float, inclusion_radius: float, thresholds,
                 residue_labels=None, device=None):
        s = object.__setattr__
        for k, v in tables.items():
            v = np.ascontiguousarray(v)
            v.setflags(write=False)
            s(self, k, v)
        s(self, "n_pose_atoms", int(n_pose_atoms))
        s(self, "n_pocket_residues", int(self.pocket_residues.shape[0]))
        s(self, "n_pocket_atoms", int(self.patom.shape[0]))
        s(self, "n_pairs", int(self.pair_start[-1]))
        s(self, "n_ca", int(((self.patom_kind & KIND_CA) != 0).sum()))
        s(self, "pocket_radius", float(pocket_radius))
        s(self, "inclusion_radius", float(inclusion_radius))
        s(self, "thresholds", tuple(float(t) for t in thresholds))
        labels = [f"residue {int(r)}" for r in self.pocket_residues] if residue_labels is None else [str(v) for v in residue_labels]
        if len(labels) != self.n_pocket_residues:
            raise ValueError(f"PocketAccuracy: {len(labels)} residue labels for {self.n_pocket_residues} pocket residues")
        s(self, "residue_labels", tuple(labels))
        s(self, "_tables", {})
        if device is not None:
            self.tables(device)

    def __setattr__(self, name, value):
        raise AttributeError("PocketAccuracy is immutable")

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_tables(x_ref, residue_of, receptor, ligand_idx, is_ca, is_backbone, swaps=(), pocket_radius: float = DEFAULT_POCKET_RADIUS,
                    inclusion_radius: float = DEFAULT_INCLUSION_RADIUS, thresholds: Sequence[float] = DEFAULT_THRESHOLDS,
                    residue_labels=None, device=None):
        """Everything explicit, per pose atom: x_ref [A,3] the reference structure, residue_of [A], receptor [A] (> 0: an existing
        heavy atom; ligand atoms never count), ligand_idx [L] (the existing ligand atoms), is_ca and is_backbone [A] (which receptor
        atoms are CA, and N / CA / C / O), swaps [n,2] (interchangeable atom pairs, `swap_table_from_names`: kept where both atoms are
        receptor atoms of one pocket residue, dropped for a residue of which one is not).  `residue_labels`: a name per residue id
        (a sequence indexed by the id, or a dict).  `thresholds`: exactly four."""
        x = _host(x_ref, np.float64)
        res = _host(residue_of, np.int64).reshape(-1)
        rec = (_host(receptor, np.float64).reshape(-1) > 0).copy()
        lig = _host(ligand_idx, np.int64).reshape(-1)
        ca, bb = _host(is_ca, np.float64).reshape(-1) > 0, _host(is_backbone, np.float64).reshape(-1) > 0
        if x.ndim != 2 or x.shape[1] != 3:
            raise ValueError(f"PocketAccuracy: x_ref must have shape [A,3], got {tuple(x.shape)}")
        A = int(x.shape[0])
        if not 1 <= A <= MAX_ATOMS:
            raise ValueError(f"PocketAccuracy: {A} pose atoms; the kernels take 1 .. {MAX_ATOMS}")
        if not res.shape[0] == rec.shape[0] == ca.shape[0] == bb.shape[0] == A:
            raise ValueError(f"PocketAccuracy: x_ref holds {A} atoms, residue_of {res.shape[0]}, receptor {rec.shape[0]}, is_ca "
                             f"{ca.shape[0]}, is_backbone {bb.shape[0]}")
        if len(lig) < 1 or lig.min() < 0 or lig.max() >= A or len(set(lig.tolist())) != len(lig):
            raise ValueError(f"PocketAccuracy: ligand_idx must hold at least one and only distinct atom indices below {A}")
        thresholds = tuple(float(t) for t in thresholds)
        if len(thresholds) != 4 or any(not t > 0 for t in thresholds) or not float(pocket_radius) > 0 or not float(inclusion_radius) > 0:
            raise ValueError(f"PocketAccuracy: exactly four positive thresholds and positive radii, got {thresholds}, {pocket_radius} and "
                             f"{inclusion_radius}")
        rec[lig] = False
        rec_idx = np.nonzero(rec)[0]
        if not (np.isfinite(x[rec_idx]).all() and np.isfinite(x[lig]).all()):
            raise ValueError("PocketAccuracy: the reference structure is not finite on every receptor and ligand atom")
        # pocket residues: a receptor atom closer than pocket_radius to a ligand atom (chunks of rows, never an A x A matrix)
        near = np.zeros(len(rec_idx), dtype=bool)
        for k0 in range(0, len(rec_idx), _CHUNK):
            d = np.sqrt(((x[rec_idx[k0:k0 + _CHUNK], None, :] - x[None, lig, :]) ** 2).sum(-1))
            near[k0:k0 + _CHUNK] = (d < float(pocket_radius)).any(1)
        pocket = np.unique(res[rec_idx[near]])
        if len(pocket) < 1:
            raise ValueError(f"PocketAccuracy: no receptor atom lies within {pocket_radius} A of the ligand in the reference structure")
        if len(pocket) > MAX_RESIDUES:
            raise ValueError(f"PocketAccuracy: {len(pocket)} pocket residues; the kernels take up to {MAX_RESIDUES}")
        slot_of = {int(r): k for k, r in enumerate(pocket)}
        in_pocket = rec & np.isin(res, pocket)
        patom = np.asarray(sorted(np.nonzero(in_pocket)[0], key=lambda a: (slot_of[int(res[a])], a)), dtype=np.int64)
        res_atom_start = np.zeros(len(pocket) + 1, dtype=np.int64)
        np.add.at(res_atom_start, np.asarray([slot_of[int(res[a])] for a in patom]) + 1, 1)
        res_atom_start = np.cumsum(res_atom_start)
        # pairs: receptor atoms of another residue within the inclusion radius, ascending in j
        atoms, dists, start = [], [], np.zeros(len(patom) + 1, dtype=np.int64)
        for k, i in enumerate(patom):
            d = np.sqrt(((x[rec_idx] - x[i]) ** 2).sum(-1))
            keep = (d < float(inclusion_radius)) & (res[rec_idx] != res[i])
            atoms.append(rec_idx[keep]); dists.append(d[keep])
            start[k + 1] = start[k] + int(keep.sum())
        if start[-1] > MAX_PAIRS:
            raise ValueError(f"PocketAccuracy: {int(start[-1])} pairs; the kernels take up to {MAX_PAIRS}")
        # swaps: per residue all or none
        partner = np.arange(A, dtype=np.int64)
        by_res: Dict[int, list] = {}
        for a, b in np.asarray(swaps.tolist() if hasattr(swaps, "tolist") else list(swaps), dtype=np.int64).reshape(-1, 2):
            if not (0 <= a < A and 0 <= b < A) or a == b:
                raise ValueError(f"PocketAccuracy: the swap pair ({a}, {b}) leaves the {A} atoms or names one atom twice")
            by_res.setdefault(int(res[a]), []).append((int(a), int(b)))
        kept = []
        for r in sorted(by_res):
            pairs = by_res[r]
            flat = [a for pr in pairs for a in pr]
            if len(set(flat)) != len(flat):
                raise ValueError(f"PocketAccuracy: an atom of residue {r} is in two swap pairs")
            if r in slot_of and all(rec[a] and rec[b] and res[b] == r for a, b in pairs):
                for a, b in pairs:
                    partner[a], partner[b] = b, a
                kept += pairs
        atom_slot = -np.ones(A, dtype=np.int64)
        atom_slot[patom] = [slot_of[int(res[a])] for a in patom]
        pair_atom = np.concatenate(atoms) if atoms else np.zeros(0, np.int64)
        tables = dict(pocket_residues=pocket.astype(np.int32), patom=patom.astype(np.int32), patom_partner=partner[patom].astype(np.int32),
                      patom_kind=(ca[patom] * KIND_CA + bb[patom] * KIND_BACKBONE).astype(np.uint8), patom_ref=x[patom].copy(),
                      res_atom_start=res_atom_start.astype(np.int32), pair_start=start.astype(np.int32), pair_atom=pair_atom.astype(np.int32),
                      pair_dist=np.concatenate(dists).astype(np.float64) if dists else np.zeros(0), atom_partner=partner.astype(np.int32),
                      atom_slot=atom_slot.astype(np.int32), named=np.unique(np.concatenate([patom, pair_atom])).astype(np.int32),
                      swaps=np.asarray(kept, dtype=np.int32).reshape(-1, 2),
                      swappable=np.asarray([(partner[patom[a:b]] != patom[a:b]).any() for a, b in zip(res_atom_start[:-1], res_atom_start[1:])]),
                      residue_pairs=np.diff(start[res_atom_start]).astype(np.int32))
        if residue_labels is not None:
            get = residue_labels.get if hasattr(residue_labels, "get") else (lambda r, d: residue_labels[r] if r < len(residue_labels) else d)
            residue_labels = [get(int(r), f"residue {int(r)}") or f"residue {int(r)}" for r in pocket]
        return PocketAccuracy(tables, A, pocket_radius, inclusion_radius, thresholds, residue_labels, device)

    @staticmethod
    def from_names(res_names: Sequence[str], atom_names: Sequence[str], residue_of, x_ref, ligand_idx, mask=None, **kw):
        """from residue and atom names (one per pose atom): the receptor is every atom of `mask` (default: all; which atoms exist and
        are heavy is the caller's choice) that is not in `ligand_idx` (the existing ligand atoms), CA and backbone go by atom name, the
        swaps are `swap_table_from_names` of the receptor.  Other keywords as for `from_tables`."""
        res, ok, _, _ = _residue_atoms(res_names, atom_names, residue_of, mask, "PocketAccuracy")
        lig = _host(ligand_idx, np.int64).reshape(-1)
        rec = ok.copy()
        if len(lig) and (lig.min() < 0 or lig.max() >= len(rec)):
            raise ValueError(f"PocketAccuracy: ligand_idx must hold atom indices below {len(rec)}")
        rec[lig] = False
        names = [str(a).strip().upper() for a in atom_names]
        is_ca = np.asarray([n == "CA" for n in names], dtype=bool)
        is_bb = np.asarray([n in BACKBONE_NAMES for n in names], dtype=bool)
        swaps = swap_table_from_names(res_names, atom_names, res, rec)
        return PocketAccuracy.from_tables(x_ref, res, rec, lig, is_ca, is_bb, swaps, **kw)

    @staticmethod
    def from_batch(batch, infer_meta_data, x_ref=None, pocket_radius: float = DEFAULT_POCKET_RADIUS,
                   inclusion_radius: float = DEFAULT_INCLUSION_RADIUS, thresholds: Sequence[float] = DEFAULT_THRESHOLDS, **kw):
        """from a feature dict and the loader's naming tables, named exactly as `ReceptorGeometry.from_batch` names them: a residue is
        a token, an atom exists where `a_mask > 0` (and `x_exists > 0` when the batch has it), the receptor is every existing heavy atom
        that is not of a ligand token, `x_ref` defaults to `batch["x_gt"]`; the tables are uploaded to the batch's device."""
        from .driver import ligand_atom_mask
        from .interactions import residue_labels_from_meta
        from .scoring import names_from_meta
        res, names, z, _ = names_from_meta(infer_meta_data)
        rid = _host(batch["atom_id_to_token_id"], np.int64).reshape(-1)
        if len(res) != rid.shape[0]:
            raise ValueError(f"PocketAccuracy: infer_meta_data names {len(res)} atoms, the batch holds {rid.shape[0]}")
        is_lig = _host(ligand_atom_mask(batch), bool).reshape(-1)
        exists = np.ones(rid.shape[0], dtype=bool)
        for k in ("a_mask", "x_exists"):
            if batch.get(k) is not None:
                exists &= _host(batch[k], np.float64).reshape(-1) > 0
        dev = batch["x_gt"].device
        kw.setdefault("device", dev if dev.type == "cuda" else None)
        kw.setdefault("residue_labels", residue_labels_from_meta(infer_meta_data, rid, int(batch["is_ligand"].shape[0])))
        return PocketAccuracy.from_names(res, names, rid, batch["x_gt"] if x_ref is None else x_ref, np.nonzero(is_lig & exists)[0],
                                         mask=exists & (z != 1) & ~is_lig, pocket_radius=pocket_radius, inclusion_radius=inclusion_radius,
                                         thresholds=thresholds, **kw)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernel's tables on `device` (uploaded once, from copies: the host arrays are read-only)"""
        return ops.cached_upload(self._tables, device, lambda up: {k: up(np.array(getattr(self, k))) for k in _DEVICE_KEYS})

    def score(self, x_pred: torch.Tensor) -> dict:
        """x_pred [P,A,3] (device) -> dict of device tensors: lddt_lp [P] and residue_lddt [P,Rp] fp32; conserved [P,4] and swapped
        [P,Rp] int32; ca_rmsd, backbone_rmsd, heavy_rmsd [P] (views of rmsd [P,3]) and residue_rmsd [P,Rp] fp32; quat [P,4] and t [P,3]
        float64 (x' = R(quat) x + t carries the pose into the reference's frame); ok and fit_ok [P] uint8 - and n_pairs (int),
        pocket_residues [Rp] int32 (device), residue_labels (a tuple).  Nothing is read back, nothing synchronises."""
        if x_pred.dim() != 3 or x_pred.shape[1] != self.n_pose_atoms or x_pred.shape[2] != 3:
            raise ValueError(f"PocketAccuracy.score: the tables are over {self.n_pose_atoms} pose atoms, x_pred has shape {tuple(x_pred.shape)}")
        if not 1 <= x_pred.shape[0] <= MAX_POSES:
            raise ValueError(f"PocketAccuracy.score: {x_pred.shape[0]} poses; the kernel takes 1 .. {MAX_POSES}")
        L_ = ops._lib.init()
        x = x_pred.float().contiguous()
        dev = x.device
        P, A, Np, Rp = x.shape[0], self.n_pose_atoms, self.n_pocket_atoms, self.n_pocket_residues
        t = self.tables(dev)
        n_ws = L_.pd_pocket_accuracy_workspace_numel(P, Rp)
        ops.check(min(n_ws, 0), "pd_pocket_accuracy_workspace_numel")
        ws = torch.empty(n_ws, dtype=torch.int32, device=dev)
        lddt, res_lddt = torch.empty(P, device=dev), torch.empty(P, Rp, device=dev)
        conserved, swapped = torch.empty(P, 4, dtype=torch.int32, device=dev), torch.empty(P, Rp, dtype=torch.int32, device=dev)
        rmsd, res_rmsd = torch.empty(P, 3, device=dev), torch.empty(P, Rp, device=dev)
        quat, tr = torch.empty(P, 4, dtype=torch.float64, device=dev), torch.empty(P, 3, dtype=torch.float64, device=dev)
        ok, fit_ok = torch.empty(P, dtype=torch.uint8, device=dev), torch.empty(P, dtype=torch.uint8, device=dev)
        ptr = lambda k: ops.ptr(t[k]) if t[k].numel() else None
        ops.check(L_.pd_pocket_accuracy(ops.ptr(x), ptr("patom"), ptr("patom_partner"), ptr("patom_kind"), ptr("patom_ref"),
                                        ptr("res_atom_start"), ptr("pair_start"), ptr("pair_atom"), ptr("pair_dist"), ptr("atom_partner"),
                                        ptr("atom_slot"), ptr("named"), *self.thresholds, ops.ptr(ws), n_ws, ops.ptr(lddt),
                                        ops.ptr(res_lddt), ops.ptr(conserved), ops.ptr(swapped), ops.ptr(rmsd), ops.ptr(res_rmsd),
                                        ops.ptr(quat), ops.ptr(tr), ops.ptr(ok), ops.ptr(fit_ok), P, A, Np, Rp, self.n_pairs,
                                        int(self.named.shape[0]), ops.stream()), "pd_pocket_accuracy")
        return {"lddt_lp": lddt, "residue_lddt": res_lddt, "conserved": conserved, "swapped": swapped, "rmsd": rmsd, "ca_rmsd": rmsd[:, 0],
                "backbone_rmsd": rmsd[:, 1], "heavy_rmsd": rmsd[:, 2], "residue_rmsd": res_rmsd, "quat": quat, "t": tr, "ok": ok,
                "fit_ok": fit_ok, "n_pairs": self.n_pairs, "pocket_residues": t["pocket_residues"], "residue_labels": self.residue_labels}

    # ------------------------------------------------------------------ reading a result
    def describe(self, result: dict, row: int) -> List[str]:
        """one pose of a `score` result (read back here) -> a line per pocket residue, worst first: by descending residue_rmsd when
        the pose was fitted, else by ascending residue_lddt; the label, the residue's lDDT, its RMSD and whether it was swapped"""
        lddt = _host(result["residue_lddt"][row], np.float64).reshape(-1)
        rms = _host(result["residue_rmsd"][row], np.float64).reshape(-1)
        sw = _host(result["swapped"][row], np.int64).reshape(-1)
        if lddt.shape[0] != self.n_pocket_residues:
            raise ValueError(f"PocketAccuracy.describe: a row of {lddt.shape[0]} for {self.n_pocket_residues} pocket residues")
        fitted = bool(np.isfinite(rms).all())
        order = sorted(range(len(lddt)), key=(lambda r: (-rms[r], lddt[r], r)) if fitted else (lambda r: (lddt[r], r)))
        return [f"{self.residue_labels[r]}: lddt {lddt[r]:.3f}, rmsd {rms[r]:.2f} A{', swapped' if sw[r] else ''}" for r in order]

    def __repr__(self):
        return (f"PocketAccuracy(n_pose_atoms={self.n_pose_atoms}, pocket_residues={self.n_pocket_residues}, pocket_atoms="
                f"{self.n_pocket_atoms}, n_pairs={self.n_pairs}, n_ca={self.n_ca}, swappable={int(self.swappable.sum())}, "
                f"pocket_radius={self.pocket_radius}, inclusion_radius={self.inclusion_radius})")
