"""How many distinct binding modes did the sampler find, which pose represents each one, and how populated is each?  Greedy leader
clustering of the poses on the device (kernel `pd_pose_clusters`, csrc/cluster.hip - its header comment and tests/pose_clusters_ref.py
give the definition), the way AutoDock Vina, AutoDock, GNINA and rDock report their modes: the poses are walked best first; a pose
within `cutoff` of an earlier representative (its leader) joins that mode, any other pose opens a new one.  It needs no ground truth,
it is deterministic, the number of modes follows from the poses, and because the walk takes any order - pose ids, the confidence
head's, the Vina score's, the refined score's - "the best pose of each mode" is what `leader` holds.

The distance is the (symmetry-corrected) pairwise ligand RMSD of `ranking.pairwise_ligand_rmsd`, or 1 - the Tanimoto similarity of
`InteractionFingerprint.pairwise` (`metric="interactions"`: poses that touch the same residues in the same ways share a mode, and
`cutoff` is then a Tanimoto distance in 0 .. 1), or the best-fit ligand RMSD of `bestfit.BestFitRmsd.pairwise` (`metric="conformer"`:
poses with the same internal conformation share a mode, wherever they sit), or 1 - the shape Tanimoto of
`shape.ShapeOverlap.pairwise` (`metric="shape"`: poses that fill the same volume share a mode; `cutoff` is then that distance in 0 .. 1).

`cluster` returns device tensors and never reads back: `labels` int32 [n] (-1 for an invalid pose), `dist_to_leader` fp32 [n], and per
mode, in arrays of length n of which the first `n_clusters` entries count (behind them ids are -1, sizes 0, floats NaN): `leader`,
`size`, `radius` (the largest distance of a member to the leader), `medoid` (the member with the smallest summed distance to the
others, the smallest id on a tie), `spread` (the mean distance between two different members, 0 for a singleton) and `mean_score`
(with `scores`); `n_clusters` int32 [1].

Caveats.  The default cutoff of 2.0 A is this package's choice (the customary RMSD threshold of a "correct" pose); it has not been
validated on real complexes.  Greedy clustering depends on the order: another ranking gives other leaders and can move poses that lie
between two modes.  An invalid pose never leads and never joins - with `valid=` the best pose may not be the leader of mode 0.  Not
here: hierarchical or linkage clustering, K-means on the device (`ranking.get_representatives` stays what the reference does, on the
host), several systems in one launch; at most 8192 poses.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import ops

MAX_POSES = 8192                      # PD_POSE_CLUSTERS_MAX_POSES
ORDERS = (None, "confidence", "vina", "vina_refined", "distogram")
METRICS = ("rmsd", "interactions", "conformer", "shape", "torsion")
_PER_MODE = ("leader", "size", "radius", "medoid", "spread", "mean_score")


class PoseClusters:
    """An immutable spec: `cutoff` (A for `metric="rmsd"` and `"conformer"`, a Tanimoto distance for `"interactions"` and `"shape"`, a TFD in 0 .. 1 for `"torsion"`), `by` - the order `redock` walks
    the poses in (None: pose ids; "confidence", "vina", "vina_refined", "distogram": the result's `order_confidence`, `order_vina`,
    `order_vina_refined`, `order_distogram`) - and `metric`.  `cluster` and `binding_modes` take their order from the caller."""

    __slots__ = ("cutoff", "by", "metric")

    def __init__(self, cutoff: float = 2.0, by: Optional[str] = None, metric: str = "rmsd"):
        cutoff = float(cutoff)
        if not 0.0 <= cutoff < float("inf"):
            raise ValueError(f"PoseClusters: cutoff={cutoff}; expected a finite value >= 0")
        if by not in ORDERS:
            raise ValueError(f"PoseClusters: by={by!r}; expected one of {ORDERS}")
        if metric not in METRICS:
            raise ValueError(f"PoseClusters: metric={metric!r}; expected one of {METRICS}")
        object.__setattr__(self, "cutoff", cutoff)
        object.__setattr__(self, "by", by)
        object.__setattr__(self, "metric", metric)

    def __setattr__(self, name, value):
        raise AttributeError("PoseClusters is immutable")

    def __repr__(self):
        return f"PoseClusters(cutoff={self.cutoff}, by={self.by!r}, metric={self.metric!r})"

    # ------------------------------------------------------------------ the kernel
    def cluster(self, D: torch.Tensor, order: Optional[torch.Tensor] = None, scores=None, valid: Optional[torch.Tensor] = None
                ) -> Dict[str, torch.Tensor]:
        """D fp32 [n,n] (device; symmetric, zero diagonal) -> the dict of the module docstring.  `order` (integer [n], a permutation of
        the pose ids, best first) is walked when given; else `ranking.rank_by_score(scores)` when `scores` (the dict of
        `VinaScore.score` or a tensor [n], lower is better) is given; else the pose ids.  `scores` also gives `mean_score`; `valid`
        (bool or uint8 [n]): the poses that may lead and join.  Nothing is read back, nothing synchronises - the values of `order`
        are not looked at on the host; the kernel skips an entry outside 0 .. n-1."""
        if not isinstance(D, torch.Tensor) or D.dim() != 2 or D.shape[0] != D.shape[1] or D.dtype != torch.float32:
            raise ValueError(f"PoseClusters.cluster: D must be a square fp32 matrix, got "
                             f"{getattr(D, 'dtype', type(D))} {tuple(getattr(D, 'shape', ()))}")
        n = D.shape[0]
        if not 1 <= n <= MAX_POSES:
            raise ValueError(f"PoseClusters.cluster: {n} poses; the kernel takes 1 .. {MAX_POSES}")
        score = None
        if scores is not None:
            score = scores["score"] if isinstance(scores, dict) else scores
            if not isinstance(score, torch.Tensor) or not score.dtype.is_floating_point or score.numel() != n:
                raise ValueError(f"PoseClusters.cluster: scores must hold one floating-point value per pose ({n}), got "
                                 f"{getattr(score, 'dtype', type(score))} {tuple(getattr(score, 'shape', ()))}")
            score = score.reshape(-1)
        if order is not None:
            if not isinstance(order, torch.Tensor) or order.dtype not in (torch.int32, torch.int64) or order.shape != (n,):
                raise ValueError(f"PoseClusters.cluster: order must be an int32 / int64 permutation of the {n} pose ids, got "
                                 f"{getattr(order, 'dtype', type(order))} {tuple(getattr(order, 'shape', ()))}")
        if valid is not None:
            if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8) or valid.shape != (n,):
                raise ValueError(f"PoseClusters.cluster: valid must be a bool / uint8 mask over the {n} poses, got "
                                 f"{getattr(valid, 'dtype', type(valid))} {tuple(getattr(valid, 'shape', ()))}")
        if not D.is_cuda:                  # order, scores and valid follow D to its device; a host D would hand the kernel host pointers
            raise ValueError(f"PoseClusters.cluster: D must be on the GPU, got a tensor on {D.device}")
        dev = D.device
        D = D.contiguous()
        if order is None:
            if score is not None:
                from .ranking import rank_by_score
                order = rank_by_score(score.to(dev))
            else:
                order = torch.arange(n, dtype=torch.int32, device=dev)
        order = order.to(device=dev, dtype=torch.int32).contiguous()
        score32 = score.to(device=dev, dtype=torch.float32).contiguous() if score is not None else None
        valid8 = valid.to(device=dev, dtype=torch.uint8).contiguous() if valid is not None else None
        L_ = ops._lib.init()
        numel = L_.pd_pose_clusters_workspace_numel(n)
        ops.check(min(numel, 0), "pd_pose_clusters_workspace_numel")
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        ws = new((numel,), torch.float64)
        out = {"labels": new((n,), torch.int32), "dist_to_leader": new((n,), torch.float32), "leader": new((n,), torch.int32),
               "size": new((n,), torch.int32), "radius": new((n,), torch.float32), "medoid": new((n,), torch.int32),
               "spread": new((n,), torch.float32), "mean_score": new((n,), torch.float32), "n_clusters": new((1,), torch.int32)}
        ops.check(L_.pd_pose_clusters(ops.ptr(D), ops.ptr(order), self.cutoff, ops.ptr(valid8), ops.ptr(score32), ops.ptr(ws), numel,
                                      *(ops.ptr(out[k]) for k in ("labels", "dist_to_leader", "leader", "size", "radius", "medoid",
                                                                  "spread", "mean_score", "n_clusters")), n, ops.stream()),
                  "pd_pose_clusters")
        return out

    def binding_modes(self, x_pred: torch.Tensor, ligand_idx: torch.Tensor, align_weights: Optional[torch.Tensor] = None,
                      symmetry=None, anchor: Optional[int] = None, **cluster_kwargs) -> Dict[str, torch.Tensor]:
        """The path without a ground truth: x_pred [P,A,3] (device), ligand_idx int32 [L] -> `cluster` of the poses' pairwise ligand RMSD
        (`ranking.pairwise_ligand_rmsd`, corrected for the ligand's automorphisms with `symmetry=`), plus `dist` (that matrix) and
        `x_common` (the poses the matrix was taken of).  With `align_weights` [A] every pose is first moved into the frame of pose
        `anchor` (weighted Kabsch, `weighted_rigid_align`; the default anchor is the first pose of `order=`, pose 0 without it - an
        `order` tensor is then read once for that id); without them the poses are taken as they are, e.g. poses of one rigid receptor.
        `cluster_kwargs`: `order`, `scores`, `valid` of `cluster`."""
        if not isinstance(x_pred, torch.Tensor) or x_pred.dim() != 3 or x_pred.shape[2] != 3:
            raise ValueError(f"PoseClusters.binding_modes: x_pred must be [P,A,3], got {tuple(getattr(x_pred, 'shape', ()))}")
        if self.metric != "rmsd":
            raise ValueError("PoseClusters.binding_modes clusters on the ligand RMSD; for metric='interactions' give "
                             "cluster() the matrix 1 - InteractionFingerprint.pairwise(bits), for metric='conformer' "
                             "BestFitRmsd.pairwise(x)")
        P = x_pred.shape[0]
        if not 1 <= P <= MAX_POSES:
            raise ValueError(f"PoseClusters.binding_modes: {P} poses; the kernel takes 1 .. {MAX_POSES}")
        bad = set(cluster_kwargs) - {"order", "scores", "valid"}
        if bad:
            raise TypeError(f"PoseClusters.binding_modes: unexpected keyword arguments {sorted(bad)}")
        from .ranking import pairwise_ligand_rmsd
        x = x_pred.float().contiguous()
        if align_weights is not None:
            from .model import weighted_rigid_align
            if anchor is None:
                order = cluster_kwargs.get("order")
                anchor = int(order[0]) if order is not None else 0
            if not 0 <= int(anchor) < P:
                raise ValueError(f"PoseClusters.binding_modes: anchor={anchor} is not one of the {P} poses")
            x = weighted_rigid_align(x[int(anchor)][None].expand(P, -1, -1).contiguous(), x, align_weights.to(x.device))
        D = pairwise_ligand_rmsd(x, ligand_idx.to(device=x.device, dtype=torch.int32).contiguous(), symmetry=symmetry)[0]
        out = self.cluster(D, **cluster_kwargs)
        out.update(dist=D, x_common=x)
        return out

    # ------------------------------------------------------------------ conveniences
    @staticmethod
    def representatives(result: Dict[str, torch.Tensor], per: str = "leader") -> torch.Tensor:
        """the pose id of every mode, int32 [n] on the device, -1 behind `n_clusters`: its leader (the best-ranked member) or its medoid"""
        if per not in ("leader", "medoid"):
            raise ValueError(f"PoseClusters.representatives: per={per!r}; expected 'leader' or 'medoid'")
        return result[per]

    @staticmethod
    def summary(result: Dict[str, torch.Tensor]) -> List[dict]:
        """the one host convenience: ONE read-back -> a list of dicts, one per mode in the order of their leaders: leader, medoid, size,
        members (ascending pose ids), radius, spread, mean_score"""
        n = result["labels"].shape[0]
        packed = torch.cat([result["n_clusters"].double().reshape(1), result["labels"].double()] +
                           [result[k].double() for k in _PER_MODE]).cpu().numpy()
        K, labels = int(packed[0]), packed[1:1 + n].astype(int)
        cols = {k: packed[1 + (1 + c) * n: 1 + (2 + c) * n] for c, k in enumerate(_PER_MODE)}
        return [dict(leader=int(cols["leader"][k]), medoid=int(cols["medoid"][k]), size=int(cols["size"][k]),
                     members=[int(i) for i in (labels == k).nonzero()[0]], radius=float(cols["radius"][k]),
                     spread=float(cols["spread"][k]), mean_score=float(cols["mean_score"][k])) for k in range(K)]


def check_redock_prerequisites(clusters, *, confidence=None, vina=None, refine=None, interactions=None, conformer_rmsd=None,
                               shape=None, torsions=None, distogram=None) -> None:
    """redock(clusters=): raise ValueError for what the spec needs and the call lacks - before any sampling"""
    if clusters is None:
        return
    if not isinstance(clusters, PoseClusters):
        raise ValueError(f"clusters= takes a PoseClusters, got {type(clusters).__name__}")
    if clusters.metric == "interactions" and interactions is None:
        raise ValueError("clusters=PoseClusters(metric='interactions') needs interactions=")
    if clusters.metric == "conformer" and conformer_rmsd is None:
        raise ValueError("clusters=PoseClusters(metric='conformer') needs conformer_rmsd=")
    if clusters.metric == "shape" and shape is None:
        raise ValueError("clusters=PoseClusters(metric='shape') needs shape=")
    if clusters.metric == "torsion" and torsions is None:
        raise ValueError("clusters=PoseClusters(metric='torsion') needs torsions=")
    if clusters.by == "confidence" and confidence is None:
        raise ValueError("clusters=PoseClusters(by='confidence') needs confidence=")
    if clusters.by == "vina" and vina is None:
        raise ValueError("clusters=PoseClusters(by='vina') needs vina=")
    if clusters.by == "vina_refined" and (refine is None or vina is None):
        raise ValueError("clusters=PoseClusters(by='vina_refined') needs refine= and vina=")
    if clusters.by == "distogram" and not distogram:
        raise ValueError("clusters=PoseClusters(by='distogram') needs distogram=")


def cluster_kept_poses(clusters, aligned, ligand_idx, out, interactions=None, ligand_symmetry=None) -> dict:
    """redock(clusters=): {"clusters": the clustering of the kept, aligned poses} from what the result `out` already holds (module
    docstring of driver.redock)"""
    if clusters.metric == "rmsd":
        if out.get("ranking") is not None:
            D = out["ranking"]["dist"]                 # the same matrix: the aligned poses, the same symmetry table
        else:
            from .ranking import pairwise_ligand_rmsd
            D = pairwise_ligand_rmsd(aligned, ligand_idx, symmetry=ligand_symmetry)[0]
    elif clusters.metric == "conformer":
        D = out["conformer_rmsd"]["pairwise"]          # the modes by internal conformation instead of by placement
    elif clusters.metric == "torsion":
        D = out["torsions"]["pairwise"]                # the modes by torsion angles: the cutoff is a TFD in 0 .. 1
    elif clusters.metric == "shape":
        D = 1.0 - out["shape"]["pairwise"]["shape_tanimoto"]   # poses that fill the same volume (unit diagonal: zero distance)
    else:
        D = 1.0 - interactions.pairwise(out["interactions"]["bits"])
    scores = out["vina"]["score"] if "vina" in out else None       # mean_score of a mode, whatever order is walked
    order = None
    if clusters.by == "confidence":
        order = out["order_confidence"]
    elif clusters.by == "vina":
        order = out["order_vina"]
    elif clusters.by == "vina_refined":
        order, scores = out["order_vina_refined"], out["refined"]["score"]
    elif clusters.by == "distogram":
        order = out["order_distogram"]
    else:
        order = torch.arange(aligned.shape[0], dtype=torch.int32, device=aligned.device)
    valid = out["validity"]["valid"] if "validity" in out else None
    res = clusters.cluster(D, order=order, scores=scores, valid=valid)
    res["dist"] = D
    if out.get("ranking") is not None and out["ranking"].get("rmsd_all") is not None:
        lead = res["leader"].long()
        r = out["ranking"]["rmsd_all"]
        res["leader_rmsd"] = torch.where(lead >= 0, r[lead.clamp(min=0)], torch.full_like(r, float("nan")))
    return {"clusters": res}
