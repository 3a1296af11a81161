"""Can a sampled pose be improved where it stands?  Local refinement of every pose in its rigid receptor, on the device (kernels
`pd_vina_refine` and `pd_vina_refine_energy`, csrc/vina_refine.hip), along the route `vina --local_only` takes: the ligand moves
only as a rigid body and about its rotatable bonds, so bond lengths, angles and rings are preserved by construction, no force field
for the ligand's internal geometry is needed, and the 6 + T coordinates replace 3 L.

    E(y) = inter + intra        the pair function of `scoring.VinaScore` (float64 here), over (active ligand atom, receptor atom)
                                and over the ligand's own pairs of active atoms more than three bonds apart; not divided by
                                1 + 0.0585 n_rot
    move(y, s), s in R^(6+T)    for k = 0 .. T-1 rotate the moving set M_k by s[6+k] about the bond a_k -> b_k, then rotate the whole
                                ligand about its centroid by the rotation vector s[3:6], then translate by s[0:3]
    minimiser                   the float64 BFGS with line search of the MMFF relaxation (csrc/mmff.hip; Numerical Recipes dfpmin /
                                lnsrch), the chart re-centred after every accepted step, the direction cut to |xi| <= max_step (A
                                and radians) before each line search; one block per pose, one launch

It stops when the largest component of the generalised gradient falls below `grad_tol` (status 0), after `max_iters` accepted steps
(status 1), or when the line search finds no lower point (status 2).  **Two caveats.**  The weights are Vina's published ones,
unvalidated on real complexes and not fitted to this model's poses, as for `VinaScore`; and the receptor is rigid here -
`flex.FlexRefine` runs the same minimiser with chosen side chains flexible.  Out of scope: Cartesian relaxation.

Does a better pose exist within a few angstrom?  `search(x_pred)` asks the same energy with the loop every docking program that
carries Vina's scoring function runs (kernel `pd_vina_search`, one block per (pose, chain); tests/vina_search_ref.py is the written
definition - the package's own, not a port of Vina's `monte_carlo`):

    start                       every chain of a pose begins at `refine`'s result for that pose
    step m = 1 .. steps         Philox4x32-10 keyed by `seed`, counters (pose id, chain, m, 0 / 1), picks one entity - the translation,
                                the rotation or one torsion - and draws its perturbation from a cube: +- translate_amp A, a rotation
                                vector within +- rotate_amp rad, a torsion within +- pi; the perturbed conformation is minimised
                                from a fresh H = I; Metropolis: accepted when E falls, else with probability
                                exp(-(E_new - E_cur) / temperature); the lowest minimum seen is kept whatever the test said
    per pose                    the chain with the lowest energy (the lowest index on a tie)

The chains' state lives on the device between launches and the draws depend on (seed, pose id, chain, step) alone, so cutting the
steps (`steps_per_launch`) or the poses into launches changes no bit.  Not Vina's search: cube draws instead of its ball, no Hessian
carried over between steps, no final merging of modes (`PoseClusters.binding_modes` on `x_chains` gives the modes).  A lower Vina
energy is not a lower RMSD.  Out of scope: grid maps, flexible side chains inside the search (`flex.FlexRefine` refines with them),
feeding the search back into the sampler.

`VinaRefine` holds one system's tables, built once on the host; `refine(x_pred)` and `energy(x_pred)` return device tensors and never
synchronise.  `driver.redock(..., refine=)` reports the refinement of the kept poses; the returned poses are not replaced.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .scoring import MAX_POSES, VinaScore, _bond_list

__all__ = ["VinaRefine", "rotatable_bonds", "torsion_table", "intra_pairs", "MAX_TORSIONS", "STATUS"]

#: the kernel's limit: 6 + T coordinates, one per lane of a wave
MAX_TORSIONS = 58
#: `status` of a refined pose
STATUS = ("converged", "max_iters", "line_search")
#: `search`: the most chains per pose, and the most (pose, chain) blocks of one launch - more poses go in several launches
MAX_CHAINS = 64
MAX_SEARCH_BLOCKS = 65535


def _adjacency(n, bonds):
    adj = [set() for _ in range(n)]
    for i, j in bonds:
        adj[i].add(j); adj[j].add(i)
    return adj


def _side(adj, start, block):
    """the atoms reachable from `start` without crossing the bond (start, block)"""
    seen, stack = {start}, [start]
    while stack:
        a = stack.pop()
        for b in adj[a]:
            if b in seen or (a == start and b == block):
                continue
            seen.add(b); stack.append(b)
    return seen


def rotatable_bonds(n_atoms: int, bonds: Iterable[Tuple[int, int]], bond_orders: Optional[Sequence[float]] = None) -> List[Tuple[int, int]]:
    """The bonds `scoring.count_rotatable_bonds` counts, in the order of `bonds`: single, in no ring, both ends with at least two
    neighbours, neither end on a triple bond."""
    n = int(n_atoms)
    bonds, orders = _bond_list(n, bonds, bond_orders, "rotatable_bonds")
    adj = _adjacency(n, bonds)
    triple = {a for b, o in zip(bonds, orders) if o == 3.0 for a in b}
    return [(i, j) for (i, j), o in zip(bonds, orders)
            if o == 1.0 and len(adj[i]) >= 2 and len(adj[j]) >= 2 and i not in triple and j not in triple and j not in _side(adj, i, j)]


def torsion_table(n_atoms: int, bonds, rotatable) -> Tuple[np.ndarray, List[np.ndarray], np.ndarray]:
    """(rot int32 [T,2], moving sets, mask uint32 [T, ceil(n/32)]) of the rotatable bonds in the graph `bonds` (hydrogens included):
    row k is (a_k, b_k) with M_k the atoms reachable from b_k without crossing the bond - the smaller side of the two, on a tie the
    one that holds the higher atom index."""
    n = int(n_atoms)
    adj = _adjacency(n, bonds)
    rows, sets = [], []
    for i, j in rotatable:
        si, sj = _side(adj, i, j), _side(adj, j, i)
        if j in si:
            raise ValueError(f"torsion_table: the bond ({i}, {j}) lies in a ring of the full graph")
        if len(sj) < len(si) or (len(sj) == len(si) and max(sj) > max(si)):
            rows.append((i, j)); sets.append(np.asarray(sorted(sj), dtype=np.int64))
        else:
            rows.append((j, i)); sets.append(np.asarray(sorted(si), dtype=np.int64))
    mask = np.zeros((len(rows), (n + 31) // 32), dtype=np.uint32)
    for k, m in enumerate(sets):
        np.bitwise_or.at(mask[k], m // 32, (np.uint32(1) << (m % 32).astype(np.uint32)))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 2), sets, mask


def intra_pairs(n_atoms: int, bonds, active=None) -> np.ndarray:
    """int32 [n,2]: the pairs i < j of active atoms more than three bonds apart (Vina's rule) or in different components"""
    n = int(n_atoms)
    adj = _adjacency(n, bonds)
    act = np.ones(n, dtype=bool) if active is None else np.asarray(active).reshape(-1) > 0
    out = []
    for s in range(n):
        if not act[s]:
            continue
        seen, front = {s}, {s}
        for _ in range(3):
            front = {b for a in front for b in adj[a]} - seen
            seen |= front
        out += [(s, j) for j in range(s + 1, n) if act[j] and j not in seen]
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


class VinaRefine:
    """One system's tables for `pd_vina_refine`: the `VinaScore` it was made from (`vina`: types, ligand_idx, rec_mask, lig_active,
    unchanged) and, as host copies, `rot` int32 [T,2] (a_k, b_k), `moving` (the T moving sets), `rot_mask` uint32 [T, ceil(L/32)],
    `intra` int32 [n_intra,2] and its per-atom neighbour lists `intra_start` [L+1] / `intra_atom` [2 n_intra] as the kernel reads
    them.  `n_torsions` is T."""

    def __init__(self, vina: VinaScore, rot, moving, rot_mask, intra, device=None):
        self.vina, self.rot, self.moving, self.rot_mask, self.intra = vina, rot, moving, rot_mask, intra
        self.n_atoms, self.n_pose_atoms, self.n_torsions = vina.n_atoms, vina.n_pose_atoms, int(rot.shape[0])
        L = self.n_atoms
        both = np.concatenate([intra, intra[:, ::-1]], 0).astype(np.int64)
        both = both[np.lexsort((both[:, 1], both[:, 0]))] if len(both) else both
        self.intra_start = np.concatenate([[0], np.cumsum(np.bincount(both[:, 0], minlength=L))]).astype(np.int32)
        self.intra_atom = both[:, 1].astype(np.int32)
        self._tables = {}
        if device is not None:
            self.tables(device)

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_vina(vina: VinaScore, bonds, bond_orders=None, device=None):
        """vina: the system's `VinaScore`; bonds: pairs of LOCAL ligand indices (position in `ligand_idx`, hydrogens included) with
        their `bond_orders` (default: all single).  Rotatable bonds are decided on the graph of the active (heavy) atoms, as
        `VinaScore.from_bonds` counts n_rot; the moving sets and the three-bond rule use the whole graph."""
        L = vina.n_atoms
        bonds, orders = _bond_list(L, bonds, bond_orders, "VinaRefine")
        act = vina.lig_active > 0
        heavy = [(b, o) for b, o in zip(bonds, orders) if act[b[0]] and act[b[1]]]
        rotatable = rotatable_bonds(L, [b for b, _ in heavy], [o for _, o in heavy])
        if len(rotatable) > MAX_TORSIONS:
            raise ValueError(f"VinaRefine: {len(rotatable)} rotatable bonds; the kernel takes up to {MAX_TORSIONS}")
        rot, moving, mask = torsion_table(L, bonds, rotatable)
        return VinaRefine(vina, rot, moving, mask, intra_pairs(L, bonds, act), device)

    @staticmethod
    def from_bonds(elements, bonds, ligand_idx, bond_orders=None, device=None, **kw):
        """as `VinaScore.from_bonds` (same arguments), then `from_vina` with the same bonds"""
        return VinaRefine.from_vina(VinaScore.from_bonds(elements, bonds, ligand_idx, bond_orders=bond_orders, device=device, **kw),
                                    bonds, bond_orders, device)

    @staticmethod
    def from_batch(batch, bonds, bond_orders=None, **kw):
        """as `VinaScore.from_batch` (same arguments), then `from_vina` with the same bonds; the tables go to the batch's device"""
        vina = VinaScore.from_batch(batch, bonds, bond_orders=bond_orders, **kw)
        dev = batch["ref_feat"].device
        return VinaRefine.from_vina(vina, bonds, bond_orders, dev if dev.type == "cuda" else None)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernel's tables on `device` (uploaded once)"""
        return ops.cached_upload(self._tables, device, lambda up: dict(
            self.vina.tables(device), rot=up(self.rot), rot_mask=up(self.rot_mask.view(np.int32)), intra_start=up(self.intra_start),
            intra_atom=up(self.intra_atom)))

    def _poses(self, x_pred, what):
        if x_pred.dim() != 3 or x_pred.shape[1] != self.n_pose_atoms or x_pred.shape[2] != 3:
            raise ValueError(f"VinaRefine.{what}: the tables are over {self.n_pose_atoms} pose atoms, x_pred has shape {tuple(x_pred.shape)}")
        if not 1 <= x_pred.shape[0] <= MAX_POSES:
            raise ValueError(f"VinaRefine.{what}: {x_pred.shape[0]} poses; the kernel takes 1 .. {MAX_POSES}")
        x = x_pred.float().contiguous()
        t = self.tables(x.device)
        head = (ops.ptr(x), ops.ptr(t["ligand_idx"]), ops.ptr(t["types"]), ops.ptr(t["rec_mask"]), ops.ptr(t["lig_active"]),
                ops.ptr(t["rot"]) if self.n_torsions else None, ops.ptr(t["rot_mask"]) if self.n_torsions else None,
                ops.ptr(t["intra_start"]), ops.ptr(t["intra_atom"]) if len(self.intra) else None, len(self.intra))
        return x, head

    def energy(self, x_pred: torch.Tensor, gradients: bool = False) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> float64 device tensors energy [P] = inter [P] + intra [P] (kcal/mol, no n_rot factor) and, with
        `gradients=True`, grad [P,L,3] = dE/dy of the ligand atoms and ggrad [P,6+T], the gradient in the rigid-body and torsion
        coordinates.  Nothing is read back."""
        x, head = self._poses(x_pred, "energy")
        L_ = ops._lib.init()
        P, A, L, T = x.shape[0], x.shape[1], self.n_atoms, self.n_torsions
        new = lambda *shape: torch.empty(*shape, device=x.device, dtype=torch.float64)
        out = {"energy": new(P), "inter": new(P), "intra": new(P)}
        if gradients:
            out.update(grad=new(P, L, 3), ggrad=new(P, 6 + T))
        ops.check(L_.pd_vina_refine_energy(*head, ops.ptr(out["energy"]), ops.ptr(out["inter"]), ops.ptr(out["intra"]),
                                           ops.ptr(out.get("grad")), ops.ptr(out.get("ggrad")), P, A, L, T, ops.stream()),
                  "pd_vina_refine_energy")
        return out

    def refine(self, x_pred: torch.Tensor, max_iters: int = 50, grad_tol: float = 1e-4, max_step: float = 1.0,
               trace: bool = False) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> dict of device tensors: x_refined [P,A,3] (fp32; the ligand rows replaced), energy_start and
        energy [P] (float64, E before and after), iterations, evaluations, status [P] (int32; `STATUS`), moved [P] (float64, ligand RMSD
        start to end, A), with `trace=True` energy_trace [P,max_iters+1], and score_start / score [P]: `VinaScore.score` of the poses
        before and after, comparable with `redock(vina=)`.  Nothing is read back."""
        if int(max_iters) < 0 or not float(grad_tol) >= 0 or not float(max_step) > 0:
            raise ValueError(f"VinaRefine.refine: max_iters={max_iters}, grad_tol={grad_tol}, max_step={max_step}")
        x, head = self._poses(x_pred, "refine")
        L_ = ops._lib.init()
        P, A, L, T = x.shape[0], x.shape[1], self.n_atoms, self.n_torsions
        f64 = lambda *shape: torch.empty(*shape, device=x.device, dtype=torch.float64)
        i32 = lambda *shape: torch.empty(*shape, device=x.device, dtype=torch.int32)
        numel = L_.pd_vina_refine_workspace_numel(P, L, T)
        ops.check(min(numel, 0), "pd_vina_refine_workspace_numel")
        ws = f64(numel)
        out = {"x_refined": torch.empty_like(x), "energy_start": f64(P), "energy": f64(P), "iterations": i32(P), "evaluations": i32(P),
               "status": i32(P), "moved": f64(P)}
        if trace:
            out["energy_trace"] = f64(P, int(max_iters) + 1)
        ops.check(L_.pd_vina_refine(*head, int(max_iters), float(grad_tol), float(max_step), ops.ptr(ws), numel, ops.ptr(out["x_refined"]),
                                    ops.ptr(out["energy_start"]), ops.ptr(out["energy"]), ops.ptr(out["iterations"]),
                                    ops.ptr(out["evaluations"]), ops.ptr(out["status"]), ops.ptr(out["moved"]),
                                    ops.ptr(out.get("energy_trace")), P, A, L, T, ops.stream()), "pd_vina_refine")
        out["score_start"] = self.vina.score(x)["score"]
        out["score"] = self.vina.score(out["x_refined"])["score"]
        return out

    def default_rotate_amp(self, x_pred: torch.Tensor, translate_amp: float = 2.0) -> float:
        """`search`'s default rotation amplitude (rad): translate_amp / max(1, r_gyr), r_gyr the radius of gyration (A) of the active
        ligand atoms in the FIRST pose - Vina's scaling.  One small read-back."""
        lig = torch.from_numpy(np.asarray(self.vina.ligand_idx)[np.asarray(self.vina.lig_active) > 0].astype(np.int64)).to(x_pred.device)
        y = x_pred[0].double()[lig]
        r_gyr = float(((y - y.mean(0)) ** 2).sum(-1).mean().sqrt()) if len(lig) else 0.0
        return float(translate_amp) / max(1.0, r_gyr)

    def search(self, x_pred: torch.Tensor, chains: int = 8, steps: int = 20, seed: int = 0, temperature: float = 1.2,
               translate_amp: float = 2.0, rotate_amp: Optional[float] = None, max_iters: int = 20, grad_tol: float = 1e-4,
               max_step: float = 1.0, steps_per_launch: Optional[int] = None, pose0: int = 0, trace: bool = False) -> Dict[str, torch.Tensor]:
        """Monte-Carlo search of every pose (module docstring; tests/vina_search_ref.py).  x_pred [P,A,3] (device) -> dict of device
        tensors: x_search [P,A,3] (fp32; the ligand rows of the pose's best chain), energy [P] (float64), best_chain [P] (int32),
        x_chains [P,K,A,3] (every chain's best as a full pose), energy_chains, energy_start [P,K] (float64; the latter is `refine`'s
        energy), best_step, accepted, evaluations [P,K] (int32), moved [P] (float64: ligand RMSD from x_pred to x_search, A), score_start /
        score [P]: `VinaScore.score` before and after, as `refine` reports them; with `trace=True` trace_energy [P,K,steps+1] (float64: E
        after the start, then E_new of every step) and trace_entity, trace_accept, trace_iterations, trace_status [P,K,steps] (int32).
        The pose id of x_pred[p] is pose0 + p: the same pose under the same id and seed gives the same chains wherever it stands.
        `temperature` (kcal/mol) may be inf; `rotate_amp=None`: `default_rotate_amp` (that default reads one number back; apart from
        it nothing is read back).  `steps_per_launch` cuts the steps into launches and changes no bit."""
        chains, steps, pose0 = int(chains), int(steps), int(pose0)
        if int(max_iters) < 0 or not float(grad_tol) >= 0 or not float(max_step) > 0:
            raise ValueError(f"VinaRefine.search: max_iters={max_iters}, grad_tol={grad_tol}, max_step={max_step}")
        if not 1 <= chains <= MAX_CHAINS or steps < 0 or pose0 < 0 or not float(temperature) > 0 or not float(translate_amp) >= 0:
            raise ValueError(f"VinaRefine.search: chains={chains} (1 .. {MAX_CHAINS}), steps={steps}, pose0={pose0}, temperature={temperature}, "
                             f"translate_amp={translate_amp}")
        if rotate_amp is not None and not float(rotate_amp) >= 0:
            raise ValueError(f"VinaRefine.search: rotate_amp={rotate_amp}")
        if steps_per_launch is not None and int(steps_per_launch) < 1:
            raise ValueError(f"VinaRefine.search: steps_per_launch={steps_per_launch}")
        x, head = self._poses(x_pred, "search")
        if rotate_amp is None:
            rotate_amp = self.default_rotate_amp(x, translate_amp)
        L_ = ops._lib.init()
        P, A, L, T, K = x.shape[0], x.shape[1], self.n_atoms, self.n_torsions, chains
        dev = x.device
        f64 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float64)
        i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)
        raw = {"x_chains": torch.empty(P, K, L, 3, device=dev), "energy_chains": f64(P, K), "energy_start": f64(P, K), "best_step": i32(P, K),
               "accepted": i32(P, K), "evaluations": i32(P, K)}
        tr = {}
        if trace:
            tr = {"trace_energy": f64(P, K, steps + 1), "trace_entity": i32(P, K, steps), "trace_accept": i32(P, K, steps),
                  "trace_iterations": i32(P, K, steps), "trace_status": i32(P, K, steps)}
        out = {"x_search": torch.empty_like(x), "energy": f64(P), "best_chain": i32(P)}
        cap = max(MAX_SEARCH_BLOCKS // K, 1)
        per = steps if steps_per_launch is None else int(steps_per_launch)
        order = ("x_chains", "energy_chains", "energy_start", "best_step", "accepted", "evaluations")
        torder = ("trace_energy", "trace_entity", "trace_accept", "trace_iterations", "trace_status")
        for a in range(0, P, cap):
            b = min(a + cap, P)
            n = b - a
            numel = L_.pd_vina_search_workspace_numel(n, K, L, T)
            ops.check(min(numel, 0), "pd_vina_search_workspace_numel")
            ws = f64(numel)
            hd = (ops.ptr(x[a:b]),) + head[1:]
            step0 = 0
            while True:
                ns = min(per, steps - step0)
                ops.check(L_.pd_vina_search(*hd, int(max_iters), float(grad_tol), float(max_step), int(seed) & 0xFFFFFFFFFFFFFFFF, pose0 + a,
                                            step0, ns, steps, float(temperature), float(translate_amp), float(rotate_amp), ops.ptr(ws), numel,
                                            *[ops.ptr(raw[k][a:b]) for k in order], *[ops.ptr(tr[k][a:b]) if trace else None for k in torder],
                                            n, K, A, L, T, ops.stream()), "pd_vina_search")
                step0 += ns
                if step0 >= steps:
                    break
            ops.check(L_.pd_vina_search_select(hd[0], head[1], ops.ptr(raw["x_chains"][a:b]), ops.ptr(raw["energy_chains"][a:b]),
                                               ops.ptr(out["best_chain"][a:b]), ops.ptr(out["energy"][a:b]), ops.ptr(out["x_search"][a:b]),
                                               n, K, A, L, ops.stream()), "pd_vina_search_select")
        lig = self.tables(dev)["ligand_idx"].long()
        full = x[:, None].expand(P, K, A, 3).contiguous()
        full[:, :, lig] = raw["x_chains"]
        out["x_chains"] = full
        out.update({k: raw[k] for k in order[1:]})
        out["moved"] = ((out["x_search"][:, lig].double() - x[:, lig].double()) ** 2).sum(-1).mean(-1).sqrt()
        out["score_start"] = self.vina.score(x)["score"]
        out["score"] = self.vina.score(out["x_search"])["score"]
        out.update(tr)
        return out

    def __repr__(self):
        return (f"VinaRefine(n_atoms={self.n_atoms}, n_pose_atoms={self.n_pose_atoms}, n_torsions={self.n_torsions}, "
                f"intra_pairs={len(self.intra)})")
