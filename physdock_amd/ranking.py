"""Pose ranking / selection - the consumer of the sampler's output (reference redocking.py:326-423).

Device side: align every accepted pose into the ground-truth frame (pocket-weighted Kabsch, redocking.py:341-342),
ligand RMSD to the ground truth (:382), the pairwise ligand-RMSD matrix (:389-390) and the template re-selection
metric (:326-335); without a ground truth, the order by the confidence head's scores (rank_by_confidence).  Host side: the K-means(5) + medoid choice on that (n x n, n <= ~100) matrix exactly as the
reference does it with scikit-learn (:392-416); when scikit-learn is missing a deterministic Lloyd iteration with
farthest-point seeding is used instead (documented divergence: the cluster labels then differ from sklearn's).
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .model import weighted_rigid_align


def pairwise_ligand_rmsd(x_aligned: torch.Tensor, ligand_idx: torch.Tensor, x_gt: torch.Tensor | None = None, symmetry=None,
                         return_perm: bool = False):
    """x_aligned [n,A,3] (device), ligand_idx int32 [L] -> (D [n,n], rmsd_to_gt [n] or None).
    `symmetry` (a `symmetry.LigandSymmetry` over the L ligand atoms in the order of ligand_idx): every value is the minimum over
    the ligand's automorphisms (kernel pd_sym_rmsd) instead of the index-wise RMSD; `return_perm=True` then adds, as a third
    element, the table row that attains the minimum against x_gt (int32 [n], None without x_gt)."""
    L_ = ops._lib.init()
    n, A = x_aligned.shape[0], x_aligned.shape[1]
    x = x_aligned.float().contiguous()
    D = torch.empty(n, n, device=x.device)
    r = torch.empty(n, device=x.device) if x_gt is not None else None
    if symmetry is None:
        if return_perm:
            raise ValueError("return_perm needs symmetry=")
        ops.check(L_.pd_pairwise_rmsd(ops.ptr(x), ops.ptr(ligand_idx), ops.ptr(x_gt.float().contiguous()) if x_gt is not None else None,
                                      ops.ptr(D), ops.ptr(r) if r is not None else None, n, A, int(ligand_idx.numel()), ops.stream()),
                  "pd_pairwise_rmsd")
        return D, r
    if symmetry.n_atoms != int(ligand_idx.numel()):
        raise ValueError(f"symmetry is a table over {symmetry.n_atoms} atoms, ligand_idx holds {int(ligand_idx.numel())}")
    best = torch.empty(n, dtype=torch.int32, device=x.device) if (return_perm and x_gt is not None) else None
    ops.check(L_.pd_sym_rmsd(ops.ptr(x), ops.ptr(ligand_idx), ops.ptr(x_gt.float().contiguous()) if x_gt is not None else None,
                             ops.ptr(symmetry.table(x.device)), ops.ptr(D), ops.ptr(r) if r is not None else None,
                             ops.ptr(best) if best is not None else None, n, A, symmetry.n_atoms, symmetry.n_perms, ops.stream()),
              "pd_sym_rmsd")
    return (D, r, best) if return_perm else (D, r)


def get_representatives(distance_matrix: np.ndarray, num_clusters: int = 5):
    """redocking.py:392-408: K-means on the rows of the distance matrix, medoid (min mean in-cluster distance) per cluster"""
    n = len(distance_matrix)
    coords = np.asarray(distance_matrix, dtype=np.float64).reshape(n, n)
    try:
        from sklearn.cluster import KMeans
        labels = KMeans(n_clusters=num_clusters, random_state=0).fit(coords).labels_
    except ImportError:                       # deterministic fallback, see module docstring
        centers = [int(np.argmin(coords.mean(1)))]
        for _ in range(1, num_clusters):
            d = np.min([((coords - coords[c]) ** 2).sum(1) for c in centers], axis=0)
            centers.append(int(np.argmax(d)))
        cent = coords[centers].copy()
        for _ in range(50):
            labels = np.argmin(((coords[:, None] - cent[None]) ** 2).sum(-1), axis=1)
            new = np.stack([coords[labels == c].mean(0) if (labels == c).any() else cent[c] for c in range(num_clusters)])
            if np.allclose(new, cent):
                break
            cent = new
    reps = []
    for c in range(num_clusters):
        idx = np.where(labels == c)[0]
        avg = np.mean(distance_matrix[idx, :], axis=0)
        reps.append(int(idx[np.argmin(avg[idx])]))
    return reps


def rank_poses(x_pred: torch.Tensor, x_gt: torch.Tensor, align_weights: torch.Tensor, is_ligand_atom: torch.Tensor,
               num_clusters: int = 5, symmetry=None, lddt_pli=None):
    """Accepted poses [n,A,3] -> dict(order=ranked pose ids (global medoid first, redocking.py:410-418),
    rmsd=ligand RMSD to x_gt of the ranked poses, x_aligned, dist).
    With `symmetry` (symmetry.LigandSymmetry) dist, rmsd_all, rmsd and order are built from the symmetry-corrected RMSD, and
    the dict also holds rmsd_plain_all (the index-wise values the reference reports) and symmetry_complete (False: the
    automorphism table was cut, the corrected values are upper bounds).
    With `lddt_pli` (lddt_pli.LddtPli of the system) it also holds lddt_pli_all [n] (device), lddt_pli (floats of the ranked poses)
    and lddt_pli_detail (the `LddtPli.score` dict) of x_pred as given - the measure needs no alignment; nothing else changes."""
    x_al = weighted_rigid_align(x_gt[None].expand(x_pred.shape[0], -1, -1).contiguous(), x_pred, align_weights)
    lig = torch.nonzero(is_ligand_atom.to(x_pred.device) > 0).flatten().to(torch.int32)
    D, r = pairwise_ligand_rmsd(x_al, lig, x_gt, symmetry=symmetry)
    Dh, rh = D.cpu().numpy().astype(np.float64), r.cpu().numpy()
    n = len(Dh)
    if n > num_clusters:
        ids = get_representatives(Dh, num_clusters)
        first = get_representatives(Dh, 1)[0]
        if first in ids:
            ids.remove(first)
            ids = [first] + ids
        else:
            ids = [first] + ids[:num_clusters - 1]
    else:
        ids = list(range(n))
    out = {"order": ids, "rmsd": [float(rh[i]) for i in ids], "x_aligned": x_al, "dist": D, "rmsd_all": r}
    if symmetry is not None:
        out["rmsd_plain_all"] = pairwise_ligand_rmsd(x_al, lig, x_gt)[1]
        out["symmetry_complete"] = bool(symmetry.complete)
    if lddt_pli is not None:
        detail = lddt_pli.score(x_pred)
        lh = detail["lddt_pli"].cpu().numpy()
        out.update(lddt_pli_all=detail["lddt_pli"], lddt_pli=[float(lh[i]) for i in ids], lddt_pli_detail=detail)
    return out


def rank_by_confidence(scores, valid=None) -> torch.Tensor:
    """Pose ids, best first, by the ground-truth-free scores of `ConfidenceModule.score_poses` (or of `get_metrics` on stacked
    logits): descending ranking_confidence, ties by descending mean_plddt, then by ascending pose id.  LongTensor [P] on the
    scores' device: two stable sorts there, nothing is read back.
    `valid` (bool [P], e.g. `PoseValidity.check(...)["valid"]`): the valid poses come first, and the valid and the invalid ones
    each keep that order among themselves (one more stable sort on the device)."""
    rc, pl = scores["ranking_confidence"].reshape(-1), scores["mean_plddt"].reshape(-1)
    if rc.shape != pl.shape:
        raise ValueError(f"ranking_confidence {tuple(rc.shape)} and mean_plddt {tuple(pl.shape)} differ in the number of poses")
    by_plddt = torch.sort(pl, descending=True, stable=True).indices          # stable: equal pLDDT keeps ascending pose id
    order = by_plddt[torch.sort(rc[by_plddt], descending=True, stable=True).indices]
    if valid is None:
        return order
    v = valid.reshape(-1)
    if v.dtype != torch.bool or v.shape != rc.shape:
        raise ValueError(f"valid must be a bool mask over the {rc.shape[0]} poses, got {v.dtype} {tuple(valid.shape)}")
    return order[torch.sort((~v.to(order.device))[order].to(torch.uint8), stable=True).indices]


def rank_by_score(scores, valid=None) -> torch.Tensor:
    """Pose ids, best first, by the interaction score of `scoring.VinaScore.score` (its dict, or the `score` tensor itself):
    ascending score (kcal/mol, lower is better), ties by ascending pose id.  LongTensor [P] on the scores' device: one stable sort
    there, nothing is read back.
    `valid` (bool [P], e.g. `PoseValidity.check(...)["valid"]`): the valid poses come first, and the valid and the invalid ones
    each keep that order among themselves (one more stable sort on the device), as in `rank_by_confidence`."""
    sc = (scores["score"] if isinstance(scores, dict) else scores).reshape(-1)
    order = torch.sort(sc, stable=True).indices                              # stable: equal scores keep ascending pose id
    if valid is None:
        return order
    v = valid.reshape(-1)
    if v.dtype != torch.bool or v.shape != sc.shape:
        raise ValueError(f"valid must be a bool mask over the {sc.shape[0]} poses, got {v.dtype} {tuple(valid.shape)}")
    return order[torch.sort((~v.to(order.device))[order].to(torch.uint8), stable=True).indices]
