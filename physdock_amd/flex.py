"""Can a clash between the ligand and a side chain be answered by the side chain?  Local refinement of every pose with flexible
receptor side chains, on the device (kernels `pd_vina_flex_refine` and `pd_vina_flex_energy`, csrc/vina_flex.hip), along the route
`vina --flex` takes.  The model co-folds, so every pose carries its own receptor and a ligand atom drawn into a LYS or LEU side chain
is the ordinary failure; `VinaRefine.refine` can answer it only by pushing the ligand out of place.  `FlexRefine.refine` minimises
the same Vina energy over three sets of coordinates at once: the ligand's rigid-body coordinates, its torsions, and the chi angles
of a chosen set of side chains.  Torsion moves keep bond lengths, angles and rings exact, so no force field for the internal
geometry is needed.  tests/flex_refine_ref.py is the written definition.

    movable rows                M = L + F: the ligand atoms of the `VinaRefine` tables, then the flexible atoms - per residue its CA (the
                                anchor of chi1; it never moves), CB and every side-chain atom beyond.  Every other receptor atom is fixed
    s in R^(6+T+S)              the ligand's 6 + T coordinates of `VinaRefine`, then one chi per side-chain torsion: the central bonds of
                                the chis of this package's chi table (chi1 CA-CB, chi2 CB-G, ...), the distal side moves.  PRO, GLY and
                                ALA have none; a residue with a needed atom missing or a torsion bond in a ring (a disulfide CYS)
                                is not eligible and is reported in `skipped`
    E = inter + intra + receptor  the pair function of `VinaScore` in float64: inter over (active ligand atom, fixed atom) and (ligand atom,
                                flexible atom), intra as `VinaRefine`, receptor over (flexible atom, fixed atom) and (flexible atom,
                                flexible atom) more than three bonds apart; not divided by 1 + 0.0585 n_rot
    minimiser                   the BFGS of `VinaRefine.refine` (the same device code) in the 6 + T + S <= 64 coordinates

With no flexible residue it is `VinaRefine.refine`.  **Caveats.**  The weights are Vina's published ones, unvalidated on real
complexes and not fitted to this model's poses; the backbone and the residues that were not selected stay rigid; there is no
rotamer library and no torsional preference, so a chi angle goes wherever the pair energy sends it; heavy atoms only.  Limits: L + F
<= 1024 movable atoms, T + S <= 58 torsions, 65535 poses.  Out of scope: backbone motion, repairing geometry, a neighbour prefilter of
the fixed atoms, several systems per launch.

`FlexRefine.search` is the Monte-Carlo loop of `VinaRefine.search` over these coordinates (kernels `pd_vina_flex_search` and
`pd_vina_flex_search_select`; tests/flex_search_ref.py is the written definition): `chains` chains per pose start at `refine`'s
result; a step draws one entity uniformly among the 2 + T + S - the ligand's translation, its rotation, one ligand torsion
(+-pi) or one chi (+-`chi_amp`) - perturbs it, minimises ligand and side chains together from a fresh H = I, and applies the
Metropolis test to E.  The draws are `VinaRefine.search`'s (same counters), so with no flexible residue it is that search.  A local
minimiser never crosses the barrier between two rotamers; a chi proposal does.  **Caveats of the search.**  The entity choice is
uniform, as Vina's: a site with many chis spends most of its steps on side chains (no weight parameter); no rotamer library; the
backbone is rigid; Vina's weights are unvalidated here.  Limits: chains <= 64; the chain state is n^2 + 9 M + 8 doubles per chain,
so the poses are cut into launches under `workspace_bytes`.

`FlexRefine` is an immutable spec of one system, built once on the host; `refine(x_pred)`, `energy(x_pred)` and `search(x_pred)`
return device tensors and never synchronise (but for `search`'s default rotation amplitude).  `driver.redock(..., flex=)` reports
the refinement of the kept poses, with `flex_search=` also the search; the returned poses are not replaced.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .receptor_geometry import _CHI, _Residues, _host, residue_bonds_from_names
from .refine import MAX_CHAINS, MAX_SEARCH_BLOCKS, MAX_TORSIONS, VinaRefine, _adjacency, _side
from .scoring import MAX_POSES, VinaScore

__all__ = ["FlexRefine", "side_chain_torsions_from_names", "MAX_MOVABLE", "SELECT_CUTOFF"]

#: the kernel's limit on L + F: 6 (L + F) doubles of LDS
MAX_MOVABLE = 1024
#: `FlexRefine.select`: a residue is flexible when a side-chain atom beyond CB lies this close (A) to an active ligand atom - this
#: package's default, not a published one
SELECT_CUTOFF = 4.0
_NO_TORSIONS = ("PRO", "GLY", "ALA")


def side_chain_torsions_from_names(res_names: Sequence[str], atom_names: Sequence[str], residue_of, residues, mask=None, chain_of=None,
                                   residue_number=None, extra_bonds=None) -> Dict:
    """The side-chain torsions of the residues `residues` (ids as in `residue_of`; atoms named as for `residue_bonds_from_names`, whose
    bond graph - `extra_bonds` included - decides the moving sets).  The torsions of a residue are the central bonds of its chis in this
    package's chi table: (CA, CB), (CB, G), ... - one per chi, `a` on the backbone side.  Returns dict(residues: the eligible ids in the
    order given; torsions {id: [(a, b), ...]} as atom indices; moving {id: [sorted index array per torsion]}: the atoms reachable from b
    without crossing the bond (the distal side, whatever its size); atoms {id: [CA, CB, ...]}: CA then chi1's moving set - the residue's
    movable atoms; skipped [(id, reason)]; bonds int32 [n,2]).  Not eligible: PRO, GLY, ALA and residues without a table ("no
    torsions"), a missing CA, CB or chi atom ("missing atom"), a torsion bond in a ring of the graph, e.g. a disulfide CYS ("ring")."""
    rs = _Residues(res_names, atom_names, residue_of, mask, chain_of, residue_number, "side_chain_torsions_from_names")
    bonds = residue_bonds_from_names(res_names, atom_names, residue_of, mask, chain_of, residue_number, extra_bonds)
    adj = _adjacency(rs.n, [tuple(b) for b in bonds.tolist()])
    out = dict(residues=[], torsions={}, moving={}, atoms={}, skipped=[], bonds=bonds)
    for s in [int(r) for r in residues]:
        kind = rs.kind.get(s)
        if kind is None or kind in _NO_TORSIONS or not _CHI.get(kind):
            out["skipped"].append((s, "no torsions"))
            continue
        names = ["CA", "CB"] + list(_CHI[kind])
        atoms = rs.atoms[s]
        if any(n not in atoms for n in names):
            out["skipped"].append((s, "missing atom"))
            continue
        tors = [(atoms[names[k]], atoms[names[k + 1]]) for k in range(len(_CHI[kind]))]
        moving = [_side(adj, b, a) for a, b in tors]
        if any(a in m for (a, _), m in zip(tors, moving)):
            out["skipped"].append((s, "ring"))
            continue
        out["residues"].append(s)
        out["torsions"][s] = tors
        out["moving"][s] = [np.asarray(sorted(m), dtype=np.int64) for m in moving]
        out["atoms"][s] = [tors[0][0]] + [int(i) for i in out["moving"][s][0]]
    return out


def _within3(adj, s):
    seen, front = {s}, {s}
    for _ in range(3):
        front = {b for a in front for b in adj[a]} - seen
        seen |= front
    return seen


class FlexRefine:
    """One system's tables for `pd_vina_flex_refine`: the `VinaScore` of the system (`vina`) and, as host copies, `mov_idx` int32 [M]
    (ligand_idx then flex_idx), `fixed_mask` uint8 [A], `active` uint8 [M], `rot` int32 [T+S,2] (local rows), `moving` (the T + S moving
    sets), `rot_mask`, `pairs` int32 [n,2] (all movable - movable pairs, i < j) with `pair_start` / `pair_atom`, `excl` (per row the
    fixed atoms within three bonds) with `excl_start` / `excl_atom`, `residue_rows` (per flexible residue its local rows).
    `n_atoms` L, `n_flex_atoms` F, `n_torsions` T + S, `n_flex_torsions` S, `flex_residues` (labels), `skipped`."""

    def __init__(self, vina: VinaScore, tables: Dict, flex_residues=(), skipped=(), device=None):
        self.vina = vina
        for k, v in tables.items():
            setattr(self, k, v)
        self.n_atoms, self.n_pose_atoms = vina.n_atoms, vina.n_pose_atoms
        self.n_flex_atoms = int(self.flex_idx.shape[0])
        self.n_movable = self.n_atoms + self.n_flex_atoms
        self.n_torsions, self.n_ligand_torsions = int(self.rot.shape[0]), int(tables["n_ligand_torsions"])
        self.n_flex_torsions = self.n_torsions - self.n_ligand_torsions
        self.flex_residues, self.skipped = tuple(flex_residues), tuple(skipped)
        self._tables = {}
        if device is not None:
            self.tables(device)

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_tables(types, ligand_idx, rec_mask, lig_active, n_rot, lig_rot, lig_moving, lig_intra, rec_bonds, residue_torsions,
                    flex_residues=None, skipped=(), device=None):
        """Everything explicit.  types uint8 [A], ligand_idx [L], rec_mask [A], lig_active [L], n_rot: as `VinaScore.from_types`;
        lig_rot [T,2], lig_moving (T index arrays), lig_intra [n,2]: the ligand's tables as `VinaRefine` holds them (local indices);
        rec_bonds [n,2]: the receptor's bond graph in pose indices; residue_torsions: per flexible residue its torsions [(a, b), ...]
        in pose indices, chi1 first, a on the backbone side.  A torsion bond in a ring, a flexible atom outside rec_mask or shared by
        two residues, more than 58 torsions or 1024 movable atoms raise ValueError."""
        vina = VinaScore.from_types(types, ligand_idx, rec_mask, n_rot, ligand_active=lig_active, device=device)
        return FlexRefine._build(vina, lig_rot, lig_moving, lig_intra, rec_bonds, residue_torsions, flex_residues, skipped, device)

    @staticmethod
    def _build(vina, lig_rot, lig_moving, lig_intra, rec_bonds, residue_torsions, flex_residues, skipped, device):
        A, L = vina.n_pose_atoms, vina.n_atoms
        lig = np.asarray(vina.ligand_idx, dtype=np.int64)
        rec_bonds = np.asarray(rec_bonds, dtype=np.int64).reshape(-1, 2)
        if len(rec_bonds) and not (0 <= rec_bonds.min() and rec_bonds.max() < A):
            raise ValueError(f"FlexRefine: a receptor bond leaves the {A} pose atoms")
        adj = _adjacency(A, [tuple(b) for b in rec_bonds.tolist()])
        flex, rows_of, moving_pose = [], [], []
        for tors in residue_torsions:
            tors = [(int(a), int(b)) for a, b in tors]
            if not tors or not all(0 <= a < A and 0 <= b < A for a, b in tors):
                raise ValueError("FlexRefine: a flexible residue needs at least one torsion, of pose atoms")
            sets = [_side(adj, b, a) for a, b in tors]
            if any(a in m for (a, _), m in zip(tors, sets)):
                raise ValueError("FlexRefine: a side-chain torsion bond lies in a ring of the receptor's bond graph")
            if any(not m <= sets[0] or a not in sets[0] | {tors[0][0]} for (a, _), m in zip(tors[1:], sets[1:])):
                raise ValueError("FlexRefine: the torsions of a residue must lie behind its first one")
            atoms = [tors[0][0]] + sorted(sets[0])
            rows_of.append(np.arange(L + len(flex), L + len(flex) + len(atoms)))
            flex += atoms
            moving_pose.append((tors, sets))
        if len(set(flex)) != len(flex) or set(flex) & set(lig.tolist()):
            raise ValueError("FlexRefine: a flexible atom belongs to two residues or to the ligand")
        flex_idx = np.asarray(flex, dtype=np.int64)
        rec = np.asarray(vina.rec_mask) > 0
        if not rec[flex_idx].all():
            raise ValueError("FlexRefine: a flexible atom is not a receptor atom of rec_mask")
        F, M = len(flex), L + len(flex)
        T = int(np.asarray(lig_rot).reshape(-1, 2).shape[0])
        local = {a: L + k for k, a in enumerate(flex)}
        rot = [tuple(r) for r in np.asarray(lig_rot, dtype=np.int64).reshape(-1, 2).tolist()]
        moving = [np.asarray(m, dtype=np.int64) for m in lig_moving]
        for tors, sets in moving_pose:
            for (a, b), m in zip(tors, sets):
                rot.append((local[a], local[b]))
                moving.append(np.asarray(sorted(local[i] for i in m), dtype=np.int64))
        if len(rot) > MAX_TORSIONS or M > MAX_MOVABLE:
            raise ValueError(f"FlexRefine: {len(rot)} torsions and {M} movable atoms; the kernel takes up to {MAX_TORSIONS} and {MAX_MOVABLE}")
        mask = np.zeros((len(rot), (M + 31) // 32), dtype=np.uint32)
        for k, m in enumerate(moving):
            np.bitwise_or.at(mask[k], m // 32, (np.uint32(1) << (m % 32).astype(np.uint32)))
        fixed = rec.copy()
        fixed[flex_idx] = False
        active = np.concatenate([(np.asarray(vina.lig_active).reshape(-1) > 0).astype(np.uint8), np.ones(F, dtype=np.uint8)])
        near = {a: _within3(adj, a) for a in flex}
        excl = [np.zeros(0, dtype=np.int64)] * L + [np.asarray(sorted(j for j in near[a] if fixed[j]), dtype=np.int64) for a in flex]
        pairs = [tuple(p) for p in np.asarray(lig_intra, dtype=np.int64).reshape(-1, 2).tolist()]
        pairs += [(i, L + k) for i in range(L) if active[i] for k in range(F)]
        pairs += [(L + k, L + m) for k in range(F) for m in range(k + 1, F) if flex[m] not in near[flex[k]]]
        pairs = np.asarray(sorted(pairs), dtype=np.int32).reshape(-1, 2)
        both = np.concatenate([pairs, pairs[:, ::-1]], 0).astype(np.int64)
        both = both[np.lexsort((both[:, 1], both[:, 0]))] if len(both) else both
        tables = dict(
            flex_idx=flex_idx.astype(np.int32), mov_idx=np.concatenate([lig, flex_idx]).astype(np.int32), fixed_mask=fixed.astype(np.uint8),
            active=active, rot=np.asarray(rot, dtype=np.int32).reshape(-1, 2), moving=moving, rot_mask=mask, pairs=pairs,
            pair_start=np.concatenate([[0], np.cumsum(np.bincount(both[:, 0], minlength=M))]).astype(np.int32),
            pair_atom=both[:, 1].astype(np.int32), excl=excl,
            excl_start=np.concatenate([[0], np.cumsum([len(e) for e in excl])]).astype(np.int32),
            excl_atom=np.concatenate(excl).astype(np.int32), residue_rows=rows_of, n_ligand_torsions=T)
        labels = list(range(len(residue_torsions))) if flex_residues is None else list(flex_residues)
        if len(labels) != len(residue_torsions):
            raise ValueError(f"FlexRefine: {len(labels)} residue labels for {len(residue_torsions)} flexible residues")
        return FlexRefine(vina, tables, labels, skipped, device)

    @staticmethod
    def from_refine(refine: VinaRefine, res_names, atom_names, residue_of, flex_residues, mask=None, chain_of=None, residue_number=None,
                    extra_bonds=None, device=None, also_skipped=()):
        """refine: the system's `VinaRefine` (its `VinaScore` and ligand tables are taken as they are); the receptor's atoms named as
        for `residue_bonds_from_names`; flex_residues: residue ids.  Residues that are not eligible land in `skipped`."""
        t = side_chain_torsions_from_names(res_names, atom_names, residue_of, flex_residues, mask, chain_of, residue_number, extra_bonds)
        return FlexRefine._build(refine.vina, refine.rot, refine.moving, refine.intra, t["bonds"], [t["torsions"][s] for s in t["residues"]],
                                 t["residues"], list(t["skipped"]) + list(also_skipped), device)

    @staticmethod
    def select(ligand_xyz, x_ref, res_names, atom_names, residue_of, cutoff: float = SELECT_CUTOFF, max_torsions: int = MAX_TORSIONS,
               residues=None, mask=None, chain_of=None, residue_number=None, extra_bonds=None) -> Dict:
        """Host helper: which residues to make flexible.  ligand_xyz [n,3]: the active ligand atoms, x_ref [A,3]: the receptor, both of
        one reference structure.  Of the eligible residues (`side_chain_torsions_from_names` over `residues`, default all) those with a
        side-chain atom beyond CB within `cutoff` A (default 4.0, this package's own choice) of a ligand atom, nearest first (ties:
        lower id); the list is cut where the next residue's torsions would exceed `max_torsions` (pass 58 - T).  Returns
        dict(residues, distance {id: A}, cut [ids left out by the limit], skipped)."""
        rid = _host(residue_of, np.int64).reshape(-1)
        pool = sorted(set(rid.tolist())) if residues is None else list(residues)
        t = side_chain_torsions_from_names(res_names, atom_names, residue_of, pool, mask, chain_of, residue_number, extra_bonds)
        lig = _host(ligand_xyz, np.float64).reshape(-1, 3)
        x = _host(x_ref, np.float64).reshape(-1, 3)
        dist = {}
        for s in t["residues"]:
            beyond = [i for i in t["atoms"][s][2:]]                                   # CA, CB, then the atoms beyond
            if beyond and len(lig):
                d = float(np.sqrt(((x[beyond][:, None] - lig[None]) ** 2).sum(-1)).min())
                if d <= cutoff:
                    dist[s] = d
        order = sorted(dist, key=lambda s: (dist[s], s))
        keep, used = [], 0
        for s in order:
            if used + len(t["torsions"][s]) > max_torsions:
                break
            keep.append(s)
            used += len(t["torsions"][s])
        return dict(residues=keep, distance=dist, cut=order[len(keep):], skipped=t["skipped"])

    @staticmethod
    def from_batch(batch, infer_meta_data, bonds, flex_residues=None, bond_orders=None, cutoff: float = SELECT_CUTOFF, **kw):
        """from a feature dict: the ligand as `VinaRefine.from_batch` (same `bonds`), the receptor's atoms named as
        `ReceptorGeometry.from_batch` names them (a residue is a token).  flex_residues: token ids, or None for `select` on
        `batch["x_gt"]`; what `select` cut is appended to `skipped` with the reason "limit"."""
        from .driver import ligand_atom_mask
        from .scoring import names_from_meta
        refine = VinaRefine.from_batch(batch, bonds, bond_orders=bond_orders, infer_meta_data=infer_meta_data, **kw)
        res, names, z, _ = names_from_meta(infer_meta_data)
        rid = _host(batch["atom_id_to_token_id"], np.int64).reshape(-1)
        if len(res) != rid.shape[0]:
            raise ValueError(f"FlexRefine: infer_meta_data names {len(res)} atoms, the batch holds {rid.shape[0]}")
        mask = (z != 1) & ~_host(ligand_atom_mask(batch), bool).reshape(-1) & (np.asarray(refine.vina.rec_mask).reshape(-1) > 0)
        per_atom = lambda key: _host(batch[key], np.int64)[rid] if key in batch else None
        named = dict(mask=mask, chain_of=per_atom("asym_id"), residue_number=per_atom("residue_index"))
        cut = []
        if flex_residues is None:
            x = _host(batch["x_gt"], np.float64).reshape(-1, 3)
            lig = np.asarray(refine.vina.ligand_idx)[np.asarray(refine.vina.lig_active) > 0]
            sel = FlexRefine.select(x[lig], x, res, names, rid, cutoff, MAX_TORSIONS - refine.n_torsions, **named)
            flex_residues, cut = sel["residues"], [(s, "limit") for s in sel["cut"]]
        dev = batch["ref_feat"].device
        return FlexRefine.from_refine(refine, res, names, rid, flex_residues, device=dev if dev.type == "cuda" else None, also_skipped=cut,
                                      **named)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernel's tables on `device` (uploaded once)"""
        return ops.cached_upload(self._tables, device, lambda up: dict(
            types=self.vina.tables(device)["types"], mov_idx=up(self.mov_idx), fixed_mask=up(self.fixed_mask), active=up(self.active),
            rot=up(self.rot), rot_mask=up(self.rot_mask.view(np.int32)), pair_start=up(self.pair_start), pair_atom=up(self.pair_atom),
            excl_start=up(self.excl_start), excl_atom=up(self.excl_atom),
            residue_of_row=up(np.concatenate([np.full(len(r), k, dtype=np.int64) for k, r in enumerate(self.residue_rows)] or
                                             [np.zeros(0, dtype=np.int64)]))))

    def _poses(self, x_pred, what):
        if x_pred.dim() != 3 or x_pred.shape[1] != self.n_pose_atoms or x_pred.shape[2] != 3:
            raise ValueError(f"FlexRefine.{what}: the tables are over {self.n_pose_atoms} pose atoms, x_pred has shape {tuple(x_pred.shape)}")
        if not 1 <= x_pred.shape[0] <= MAX_POSES:
            raise ValueError(f"FlexRefine.{what}: {x_pred.shape[0]} poses; the kernel takes 1 .. {MAX_POSES}")
        x = x_pred.float().contiguous()
        t = self.tables(x.device)
        opt = lambda k, n: ops.ptr(t[k]) if n else None
        head = (ops.ptr(x), ops.ptr(t["mov_idx"]), ops.ptr(t["types"]), ops.ptr(t["fixed_mask"]), ops.ptr(t["active"]),
                opt("rot", self.n_torsions), opt("rot_mask", self.n_torsions), ops.ptr(t["pair_start"]), opt("pair_atom", len(self.pair_atom)),
                len(self.pair_atom), ops.ptr(t["excl_start"]), opt("excl_atom", len(self.excl_atom)), len(self.excl_atom))
        return x, head

    def _sizes(self, x):
        return x.shape[0], x.shape[1], self.n_atoms, self.n_flex_atoms, self.n_ligand_torsions, self.n_flex_torsions

    def energy(self, x_pred: torch.Tensor, gradients: bool = False) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> float64 device tensors energy [P] = inter + intra + receptor [P] (kcal/mol, no n_rot factor) and,
        with `gradients=True`, grad [P,L+F,3] = dE/dy of the movable atoms and ggrad [P,6+T+S].  Nothing is read back."""
        x, head = self._poses(x_pred, "energy")
        L_ = ops._lib.init()
        P = x.shape[0]
        new = lambda *shape: torch.empty(*shape, device=x.device, dtype=torch.float64)
        out = {"energy": new(P), "inter": new(P), "intra": new(P), "receptor": new(P)}
        if gradients:
            out.update(grad=new(P, self.n_movable, 3), ggrad=new(P, 6 + self.n_torsions))
        ops.check(L_.pd_vina_flex_energy(*head, ops.ptr(out["energy"]), ops.ptr(out["inter"]), ops.ptr(out["intra"]), ops.ptr(out["receptor"]),
                                         ops.ptr(out.get("grad")), ops.ptr(out.get("ggrad")), *self._sizes(x), ops.stream()),
                  "pd_vina_flex_energy")
        return out

    def refine(self, x_pred: torch.Tensor, max_iters: int = 50, grad_tol: float = 1e-4, max_step: float = 1.0,
               trace: bool = False) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> dict of device tensors: x_refined [P,A,3] (fp32; the ligand and flexible rows replaced, every other
        row copied), energy_start, energy [P] (float64, E before and after) and inter, intra, receptor [P] (the parts of `energy`),
        iterations, evaluations, status [P] (int32; `refine.STATUS`), moved [P] (float64, ligand RMSD start to end, A), moved_flex [P]
        (RMSD of the flexible atoms), residue_moved [P,R_f] (the largest displacement of an atom of each flexible residue, from the fp32
        poses), with `trace=True` energy_trace [P,max_iters+1], and score_start / score [P]: `VinaScore.score` of the poses before and
        after, as `VinaRefine.refine` reports them.  Nothing is read back."""
        if int(max_iters) < 0 or not float(grad_tol) >= 0 or not float(max_step) > 0:
            raise ValueError(f"FlexRefine.refine: max_iters={max_iters}, grad_tol={grad_tol}, max_step={max_step}")
        x, head = self._poses(x_pred, "refine")
        L_ = ops._lib.init()
        P = x.shape[0]
        f64 = lambda *shape: torch.empty(*shape, device=x.device, dtype=torch.float64)
        i32 = lambda *shape: torch.empty(*shape, device=x.device, dtype=torch.int32)
        numel = L_.pd_vina_flex_workspace_numel(P, self.n_movable, self.n_torsions)
        ops.check(min(numel, 0), "pd_vina_flex_workspace_numel")
        ws = f64(numel)
        out = {"x_refined": torch.empty_like(x), "energy_start": f64(P), "energy": f64(P), "inter": f64(P), "intra": f64(P), "receptor": f64(P),
               "iterations": i32(P), "evaluations": i32(P), "status": i32(P), "moved": f64(P), "moved_flex": f64(P)}
        if trace:
            out["energy_trace"] = f64(P, int(max_iters) + 1)
        order = ("x_refined", "energy_start", "energy", "inter", "intra", "receptor", "iterations", "evaluations", "status", "moved", "moved_flex")
        ops.check(L_.pd_vina_flex_refine(*head, int(max_iters), float(grad_tol), float(max_step), ops.ptr(ws), numel,
                                         *[ops.ptr(out[k]) for k in order], ops.ptr(out.get("energy_trace")), *self._sizes(x), ops.stream()),
                  "pd_vina_flex_refine")
        out["residue_moved"] = self._residue_moved(out["x_refined"], x, self.tables(x.device))
        out["score_start"] = self.vina.score(x)["score"]
        out["score"] = self.vina.score(out["x_refined"])["score"]
        return out

    def _residue_moved(self, x_new, x, t):
        """[P,R_f] float64: the largest displacement of an atom of each flexible residue between the fp32 poses x and x_new"""
        P = x.shape[0]
        fl = t["mov_idx"][self.n_atoms:].long()
        disp = (x_new[:, fl].double() - x[:, fl].double()).pow(2).sum(-1).sqrt()                    # [P,F]
        rm = torch.zeros(P, len(self.residue_rows), device=x.device, dtype=torch.float64)
        if self.n_flex_atoms:
            rm.scatter_reduce_(1, t["residue_of_row"][None].expand(P, -1), disp, "amax", include_self=True)
        return rm

    def search(self, x_pred: torch.Tensor, chains: int = 8, steps: int = 20, seed: int = 0, temperature: float = 1.2,
               translate_amp: float = 2.0, rotate_amp: Optional[float] = None, chi_amp: float = math.pi, max_iters: int = 20,
               grad_tol: float = 1e-4, max_step: float = 1.0, steps_per_launch: Optional[int] = None, pose0: int = 0, trace: bool = False,
               workspace_bytes: int = 256 << 20) -> Dict[str, torch.Tensor]:
        """Monte-Carlo search of every pose with the side chains flexible (module docstring; tests/flex_search_ref.py).  x_pred [P,A,3]
        (device) -> dict of device tensors: x_search [P,A,3] (fp32; the movable rows of the pose's best chain, every other row copied),
        energy [P] = (inter + intra) + receptor [P] (float64), best_chain [P] (int32), x_chains [P,K,A,3] (every chain's best as a full
        pose), energy_chains, energy_start [P,K] (float64; the latter is `refine`'s energy), best_step, accepted, evaluations [P,K]
        (int32), moved, moved_flex [P] (float64: RMSD of the ligand / the flexible atoms from x_pred to x_search, A), residue_moved
        [P,R_f], score_start / score [P] as `refine` reports them; with `trace=True` trace_energy [P,K,steps+1] and trace_entity,
        trace_accept, trace_iterations, trace_status [P,K,steps].  The pose id of x_pred[p] is pose0 + p.  `chi_amp` (rad): the
        amplitude of a side-chain proposal.  `rotate_amp=None`: `VinaRefine.default_rotate_amp` (one number read back; nothing else
        is).  `steps_per_launch` cuts the steps into launches, `workspace_bytes` the poses (at least one pose per launch, at most
        65535 // chains): neither changes a bit."""
        chains, steps, pose0 = int(chains), int(steps), int(pose0)
        if int(max_iters) < 0 or not float(grad_tol) >= 0 or not float(max_step) > 0:
            raise ValueError(f"FlexRefine.search: max_iters={max_iters}, grad_tol={grad_tol}, max_step={max_step}")
        if not 1 <= chains <= MAX_CHAINS or steps < 0 or pose0 < 0 or not float(temperature) > 0 or not float(translate_amp) >= 0:
            raise ValueError(f"FlexRefine.search: chains={chains} (1 .. {MAX_CHAINS}), steps={steps}, pose0={pose0}, temperature={temperature}, "
                             f"translate_amp={translate_amp}")
        if (rotate_amp is not None and not float(rotate_amp) >= 0) or not float(chi_amp) >= 0:
            raise ValueError(f"FlexRefine.search: rotate_amp={rotate_amp}, chi_amp={chi_amp}")
        if steps_per_launch is not None and int(steps_per_launch) < 1:
            raise ValueError(f"FlexRefine.search: steps_per_launch={steps_per_launch}")
        if int(workspace_bytes) < 1:
            raise ValueError(f"FlexRefine.search: workspace_bytes={workspace_bytes}")
        x, head = self._poses(x_pred, "search")
        if rotate_amp is None:
            rotate_amp = VinaRefine.default_rotate_amp(self, x, translate_amp)
        L_ = ops._lib.init()
        P, A, M, N, K = x.shape[0], x.shape[1], self.n_movable, self.n_torsions, chains
        sizes = lambda n: (n, K) + self._sizes(x)[1:]
        dev = x.device
        f64 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float64)
        i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)
        raw = {"x_chains": torch.empty(P, K, M, 3, device=dev), "energy_chains": f64(P, K), "energy_start": f64(P, K), "best_step": i32(P, K),
               "accepted": i32(P, K), "evaluations": i32(P, K)}
        tr = {}
        if trace:
            tr = {"trace_energy": f64(P, K, steps + 1), "trace_entity": i32(P, K, steps), "trace_accept": i32(P, K, steps),
                  "trace_iterations": i32(P, K, steps), "trace_status": i32(P, K, steps)}
        out = {"x_search": torch.empty_like(x), "energy": f64(P), "inter": f64(P), "intra": f64(P), "receptor": f64(P), "best_chain": i32(P),
               "moved": f64(P), "moved_flex": f64(P)}
        per_chain = L_.pd_vina_flex_search_workspace_numel(1, 1, M, N)
        ops.check(min(per_chain, 0), "pd_vina_flex_search_workspace_numel")
        cap = max(min(int(workspace_bytes) // (8 * per_chain * K), MAX_SEARCH_BLOCKS // K), 1)
        per = steps if steps_per_launch is None else int(steps_per_launch)
        order = ("x_chains", "energy_chains", "energy_start", "best_step", "accepted", "evaluations")
        torder = ("trace_energy", "trace_entity", "trace_accept", "trace_iterations", "trace_status")
        sel = ("best_chain", "energy", "inter", "intra", "receptor", "x_search", "moved", "moved_flex")
        ws = f64(per_chain * K * min(cap, P))
        for a in range(0, P, cap):
            b = min(a + cap, P)
            n = b - a
            numel = per_chain * K * n
            hd = (ops.ptr(x[a:b]),) + head[1:]
            step0 = 0
            while True:
                ns = min(per, steps - step0)
                ops.check(L_.pd_vina_flex_search(*hd, int(max_iters), float(grad_tol), float(max_step), int(seed) & 0xFFFFFFFFFFFFFFFF, pose0 + a,
                                                 step0, ns, steps, float(temperature), float(translate_amp), float(rotate_amp), float(chi_amp),
                                                 ops.ptr(ws), numel, *[ops.ptr(raw[k][a:b]) for k in order],
                                                 *[ops.ptr(tr[k][a:b]) if trace else None for k in torder], *sizes(n), ops.stream()),
                          "pd_vina_flex_search")
                step0 += ns
                if step0 >= steps:
                    break
            ops.check(L_.pd_vina_flex_search_select(*hd, ops.ptr(ws), numel, *[ops.ptr(out[k][a:b]) for k in sel], *sizes(n), ops.stream()),
                      "pd_vina_flex_search_select")
        t = self.tables(dev)
        mov = t["mov_idx"].long()
        full = x[:, None].expand(P, K, A, 3).contiguous()
        full[:, :, mov] = raw["x_chains"]
        out["x_chains"] = full
        out.update({k: raw[k] for k in order[1:]})
        out["residue_moved"] = self._residue_moved(out["x_search"], x, t)
        out["score_start"] = self.vina.score(x)["score"]
        out["score"] = self.vina.score(out["x_search"])["score"]
        out.update(tr)
        return out

    def describe(self) -> List[str]:
        """one line per flexible residue (label, torsions, atoms) and per skipped one (label, reason)"""
        T = self.n_ligand_torsions
        lines = []
        for lab, rows in zip(self.flex_residues, self.residue_rows):
            n = sum(1 for r in self.rot[T:] if rows[0] <= r[0] <= rows[-1])
            lines.append(f"{lab}: {n} torsion{'s' if n != 1 else ''}, {len(rows)} atoms")
        return lines + [f"{lab}: skipped ({why})" for lab, why in self.skipped]

    def __repr__(self):
        return (f"FlexRefine(n_atoms={self.n_atoms}, n_flex_atoms={self.n_flex_atoms}, n_pose_atoms={self.n_pose_atoms}, "
                f"n_torsions={self.n_torsions}, n_flex_torsions={self.n_flex_torsions}, flex_residues={len(self.flex_residues)})")
