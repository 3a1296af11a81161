"""Multi-round redocking driver - the caller of the hot path (reference redocking.py:156-356), without its file and
RDKit I/O.

What the reference does per system, and what is kept here:
  * rounds (redocking.py:181-183): round 0 samples freely; further rounds only with physics correction, each with
    the re-sampled MSA of that round (`batch_msa_feat[round]`, :188) and the template-projection branch of the
    sampler switched on (`align_ref_pos = round > 0`, `use_ref_mol_poses`, :283-299);
  * accept / reject (:303-317): the reference rebuilds the ligand with RDKit and compares chiral centres.  Here:
    `chirality=` (chirality.ChiralityReference: signed volumes of the stereocentres on the device, kernel pd_chirality)
    and / or an injected callable `accept_fn(x_pose_cpu [A,3]) -> bool`; default: accept.  Rejected poses go to a
    bounded deque (maxlen = max_samples, :164);
  * the adaptive threshold of the physics branch (:318-322): x1.15 after a round with any accepted pose, otherwise
    x0.7 with floor 1;
  * template pool for the next round (:323-335, and :293): accepted predicted ligands + the reference conformers
    closest to this round's poses under the sampler's own soft distance-difference metric (device, pd_template_match);
  * top-up with rejected poses when fewer than one round's worth was accepted (:336-337), alignment of every kept
    pose into the ground-truth frame with pocket weights (:341-342) and ranking (ranking.py, :357-423).
Conformer generation (ETKDG, :231-243) is an input (`ref_mol_poses [C,L,3]`), or comes from `conformers=` (a
`conformers.ConformerEnsemble`: distance geometry on the device, this package's own definition).  `ref_mol` (an RDKit molecule, a
`physdock_amd.mmff.MMFFTerms` table, or any object with `sampler_kwargs={"relax_fn": ...}`) is handed to the sampler in
every round as the reference does (:292), which switches on the relaxation branch below the adaptive threshold; as in the
reference a molecule whose atom count differs from the crop's ligand is dropped and the ODE step scale becomes 1.5
(`ref_mol_num_error`, :195-196,292,296).
"""
from __future__ import annotations

from collections import deque
from typing import Callable, Dict, List, Optional

import torch

from . import ops
from .clustering import check_redock_prerequisites, cluster_kept_poses
from .model import weighted_rigid_align
from .pdbio import PdbTemplate
from .ranking import rank_poses
from .sdfio import check_redock_sdf, score_sdf
from .bond_stereo import check_redock_bond_stereo, score_bond_stereo
from .shape import check_redock_shape, score_shape
from .torsions import check_redock_torsions, score_torsions


def ligand_atom_mask(batch: Dict[str, torch.Tensor]) -> torch.Tensor:
    """bool [A]: atoms of ligand tokens (redocking.py:189)"""
    return batch["is_ligand"][batch["atom_id_to_token_id"].long()].bool()


def pocket_align_weights(batch: Dict[str, torch.Tensor], use_pocket: bool = True) -> torch.Tensor:
    """per-atom weights of the final alignment, align_mode "pocket_ca" (redocking.py:197-201)"""
    idx = batch["atom_id_to_token_id"].long()
    w = (batch["s_mask"] * batch["is_protein"])[idx] if "s_mask" in batch and "is_protein" in batch \
        else 1.0 - batch["is_ligand"].float()[idx]
    if use_pocket:
        w = batch["pocket_res_feat"][idx] * w
    return w.float()


def template_scores(x_pred: torch.Tensor, ligand_idx: torch.Tensor, ref_mol_poses: torch.Tensor) -> torch.Tensor:
    """eps[b, c]: mean over ligand atom pairs of 1/4 sum_k sigmoid(|D_b - D_c| - {0.5, 1, 2, 4}) between the ligand of
    pose b and reference conformer c (redocking.py:326-331; same kernel as the in-loop template match, model.py:231-238)."""
    L_ = ops._lib.init()
    x = x_pred.float().contiguous()
    poses = ref_mol_poses.float().contiguous()
    B, A = x.shape[0], x.shape[1]
    C, L = poses.shape[0], poses.shape[1]
    assert ligand_idx.numel() == L, "reference conformers and ligand atoms differ in count"
    rd = torch.empty(C, L, L, device=x.device)
    ops.check(L_.pd_pose_dist(ops.ptr(poses), ops.ptr(rd), C, L, ops.stream()), "pd_pose_dist")
    eps = torch.empty(B, C, device=x.device)
    sel = torch.empty(B, dtype=torch.int32, device=x.device)
    ops.check(L_.pd_template_match(ops.ptr(x), ops.ptr(ligand_idx), ops.ptr(rd), None, None, ops.ptr(eps), ops.ptr(sel),
                                   B, A, L, C, ops.stream()), "pd_template_match")
    return eps


def select_reference_templates(x_pred: torch.Tensor, ligand_idx: torch.Tensor, ref_mol_poses: torch.Tensor, k: int) -> torch.Tensor:
    """indices of the k reference conformers closest to this round's poses: argsort of eps averaged over the poses
    (redocking.py:331-332)"""
    if k <= 0:
        return torch.empty(0, dtype=torch.long, device=x_pred.device)
    return torch.argsort(template_scores(x_pred, ligand_idx, ref_mol_poses).mean(0))[:k]


def next_gamma_factor(factor: float, any_accepted: bool) -> float:
    """redocking.py:318-322"""
    return factor * 1.15 if any_accepted else max(factor * 0.7, 1.0)


def _mol_num_atoms(ref_mol) -> Optional[int]:
    for attr in ("GetNumAtoms", "num_atoms"):
        v = getattr(ref_mol, attr, None)
        if v is not None:
            return int(v() if callable(v) else v)
    return None


def _device_accept(x_pred, chirality, validity, bond_stereo=None):
    """the device half of accept / reject: (per-pose list of bool, or None without a test; number of poses the validity test fails,
    or None without it) - the chirality mask, the double-bond stereo mask and the validity mask reach the host in ONE [*, B] read"""
    masks = ([chirality.accept(x_pred)] if chirality is not None else []) + \
            ([bond_stereo.accept(x_pred)] if bond_stereo is not None else []) + \
            ([validity.check(x_pred)["valid"]] if validity is not None else [])
    if not masks:
        return None, None
    rows = torch.stack(masks).tolist()
    return [all(c) for c in zip(*rows)], (len(rows[-1]) - sum(rows[-1]) if validity is not None else None)


def score_validity(validity, aligned, out) -> dict:
    """redock(validity=): {"validity": PoseValidity.check of the kept poses} and, when they were scored by the confidence head too,
    "order_confidence_valid": their ids best first with the valid poses in front"""
    from .ranking import rank_by_confidence
    res = {"validity": validity.check(aligned)}
    if "confidence" in out:
        res["order_confidence_valid"] = rank_by_confidence(out["confidence"], valid=res["validity"]["valid"])
    return res


def score_vina(vina, aligned, out) -> dict:
    """redock(vina=): {"vina": VinaScore.score of the kept poses, "order_vina": their ids best first (lowest score)} and, when their
    validity was checked too, "order_vina_valid": the same order with the valid poses in front"""
    from .ranking import rank_by_score
    res = {"vina": vina.score(aligned)}
    res["order_vina"] = rank_by_score(res["vina"])
    if "validity" in out:
        res["order_vina_valid"] = rank_by_score(res["vina"], valid=out["validity"]["valid"])
    return res


def score_refined(refine, aligned, validity, vina, refine_kwargs=None) -> dict:
    """redock(refine=): {"refined": VinaRefine.refine of the kept poses} - with `validity=` also refined["validity"], its check of
    `x_refined`, and with `vina=` "order_vina_refined": the poses' ids by their refined score, best first"""
    from .ranking import rank_by_score
    res = {"refined": refine.refine(aligned, **(refine_kwargs or {}))}
    if validity is not None:
        res["refined"]["validity"] = validity.check(res["refined"]["x_refined"])
    if vina is not None:
        res["order_vina_refined"] = rank_by_score({"score": res["refined"]["score"]})
    return res


def check_search(search, refine) -> None:
    """redock(search=): raise ValueError unless `search` is None, False, True or a dict of `VinaRefine.search` keyword arguments, and
    when it asks for a search without `refine=` - before anything is sampled"""
    if search is None or search is False:
        return
    if search is not True and not isinstance(search, dict):
        raise ValueError(f"search= takes True or a dict of VinaRefine.search keyword arguments, got {type(search).__name__}")
    if refine is None:
        raise ValueError("search= needs refine= (the system's refine.VinaRefine)")


def score_searched(search, refine, aligned, validity, vina) -> dict:
    """redock(search=): {"searched": VinaRefine.search of the kept poses} - with `validity=` also searched["validity"], its check of
    `x_search`, and with `vina=` "order_vina_searched": the poses' ids by their score after the search, best first"""
    from .ranking import rank_by_score
    res = {"searched": refine.search(aligned, **(search if isinstance(search, dict) else {}))}
    if validity is not None:
        res["searched"]["validity"] = validity.check(res["searched"]["x_search"])
    if vina is not None:
        res["order_vina_searched"] = rank_by_score({"score": res["searched"]["score"]})
    return res


def check_flex(flex, batch) -> None:
    """redock(flex=): raise ValueError unless it is a `flex.FlexRefine` over the batch's atoms - before anything is sampled"""
    if flex is None:
        return
    if not callable(getattr(flex, "refine", None)) or not hasattr(flex, "n_flex_atoms") or not hasattr(flex, "n_pose_atoms"):
        raise ValueError("flex= takes a flex.FlexRefine of the system")
    n = int(batch["x_gt"].shape[0])
    if flex.n_pose_atoms != n:
        raise ValueError(f"flex= was built over {flex.n_pose_atoms} pose atoms, the batch holds {n}")


def score_flex_refined(flex, aligned, validity, vina, receptor_geometry) -> dict:
    """redock(flex=): {"flex_refined": FlexRefine.refine of the kept poses} - with `validity=` also flex_refined["validity"], its check of
    `x_refined`; with `receptor_geometry=` also flex_refined["receptor_geometry"], its check of `x_refined` (the side chains moved, so
    the receptor is checked again); with `vina=` "order_vina_flex": the poses' ids by their score after it, best first"""
    from .ranking import rank_by_score
    res = {"flex_refined": flex.refine(aligned)}
    if validity is not None:
        res["flex_refined"]["validity"] = validity.check(res["flex_refined"]["x_refined"])
    if receptor_geometry is not None:
        res["flex_refined"]["receptor_geometry"] = receptor_geometry.check(res["flex_refined"]["x_refined"])
    if vina is not None:
        res["order_vina_flex"] = rank_by_score({"score": res["flex_refined"]["score"]})
    return res


def check_flex_search(flex_search, flex) -> None:
    """redock(flex_search=): raise ValueError unless `flex_search` is None, False, True or a dict of `FlexRefine.search` keyword
    arguments, and when it asks for a search without `flex=` - before anything is sampled"""
    if flex_search is None or flex_search is False:
        return
    if flex_search is not True and not isinstance(flex_search, dict):
        raise ValueError(f"flex_search= takes True or a dict of FlexRefine.search keyword arguments, got {type(flex_search).__name__}")
    if flex is None:
        raise ValueError("flex_search= needs flex= (the system's flex.FlexRefine)")


def score_flex_searched(flex_search, flex, aligned, validity, vina, receptor_geometry) -> dict:
    """redock(flex_search=): {"flex_searched": FlexRefine.search of the kept poses} - with `validity=` also flex_searched["validity"] and
    with `receptor_geometry=` also flex_searched["receptor_geometry"], their checks of `x_search`; with `vina=`
    "order_vina_flex_searched": the poses' ids by their score after the search, best first"""
    from .ranking import rank_by_score
    res = {"flex_searched": flex.search(aligned, **(flex_search if isinstance(flex_search, dict) else {}))}
    if validity is not None:
        res["flex_searched"]["validity"] = validity.check(res["flex_searched"]["x_search"])
    if receptor_geometry is not None:
        res["flex_searched"]["receptor_geometry"] = receptor_geometry.check(res["flex_searched"]["x_search"])
    if vina is not None:
        res["order_vina_flex_searched"] = rank_by_score({"score": res["flex_searched"]["score"]})
    return res


def score_interactions(interactions, aligned, batch) -> dict:
    """redock(interactions=): {"interactions": InteractionFingerprint.fingerprint of the kept poses} and, when the batch carries the
    ground truth, "interaction_recovery": its `compare` of their bits with the fingerprint of `x_gt`"""
    res = {"interactions": interactions.fingerprint(aligned)}
    if "x_gt" in batch:
        res["interaction_recovery"] = interactions.compare(res["interactions"]["bits"], batch["x_gt"].float())
    return res


def score_ring_interactions(ring_interactions, aligned, batch) -> dict:
    """redock(ring_interactions=): {"ring_interactions": RingInteractions.fingerprint of the kept poses} and, when the batch carries the
    ground truth, "ring_interaction_recovery": its `compare` of their bits with the fingerprint of `x_gt`"""
    res = {"ring_interactions": ring_interactions.fingerprint(aligned)}
    if "x_gt" in batch:
        res["ring_interaction_recovery"] = ring_interactions.compare(res["ring_interactions"]["bits"], batch["x_gt"].float())
    return res


def check_hydrogens(hydrogens, batch) -> None:
    """redock(hydrogens=): raise ValueError unless `hydrogens` is a `hydrogens.Hydrogens` over the batch's atoms"""
    if hydrogens is None:
        return
    if not callable(getattr(hydrogens, "hbonds", None)) or not hasattr(hydrogens, "n_pose_atoms"):
        raise ValueError("hydrogens= takes a hydrogens.Hydrogens of the system")
    n = int(batch["x_gt"].shape[0])
    if hydrogens.n_pose_atoms != n:
        raise ValueError(f"hydrogens= was built over {hydrogens.n_pose_atoms} pose atoms, the batch holds {n}")


def score_hydrogens(hydrogens, aligned, batch) -> dict:
    """redock(hydrogens=): {"hydrogens": x_h, placed, bits and counts of Hydrogens.hbonds of the kept poses} and, when the batch carries
    the ground truth, "hbond_recovery": its `compare` of their bits with the hydrogen bonds of `x_gt`"""
    found = hydrogens.hbonds(aligned)
    res = {"hydrogens": {k: found[k] for k in ("x_h", "placed", "bits", "counts")}}
    if "x_gt" in batch:
        res["hbond_recovery"] = hydrogens.compare(found["bits"], batch["x_gt"].float())
    return res


def check_receptor_geometry(receptor_geometry, batch) -> None:
    """redock(receptor_geometry=): raise ValueError unless it is a `receptor_geometry.ReceptorGeometry` over the batch's atoms"""
    if receptor_geometry is None:
        return
    if not callable(getattr(receptor_geometry, "chi_recovery", None)) or not hasattr(receptor_geometry, "n_pose_atoms"):
        raise ValueError("receptor_geometry= takes a receptor_geometry.ReceptorGeometry of the system")
    n = int(batch["x_gt"].shape[0])
    if receptor_geometry.n_pose_atoms != n:
        raise ValueError(f"receptor_geometry= was built over {receptor_geometry.n_pose_atoms} pose atoms, the batch holds {n}")


def score_receptor_geometry(receptor_geometry, aligned, batch, out) -> dict:
    """redock(receptor_geometry=): {"receptor_geometry": val, flags, valid, counts and residue_flags of ReceptorGeometry.check of the
    kept poses, chi_recovery = its `chi_recovery` against `x_gt` and, with `validity=`, valid_both}"""
    found = receptor_geometry.check(aligned)
    res = {k: found[k] for k in ("val", "flags", "valid", "counts", "residue_flags")}
    res["chi_recovery"] = receptor_geometry.chi_recovery(aligned, x_ref=batch["x_gt"].float())
    if "validity" in out:
        res["valid_both"] = found["valid"] & out["validity"]["valid"]
    return {"receptor_geometry": res}


def check_pocket_accuracy(pocket_accuracy, batch) -> None:
    """redock(pocket_accuracy=): raise ValueError unless it is a `pocket_accuracy.PocketAccuracy` over the batch's atoms and the batch
    carries the ground truth"""
    if pocket_accuracy is None:
        return
    if not callable(getattr(pocket_accuracy, "score", None)) or not hasattr(pocket_accuracy, "n_pocket_residues"):
        raise ValueError("pocket_accuracy= takes a pocket_accuracy.PocketAccuracy of the system")
    if batch.get("x_gt") is None:
        raise ValueError("pocket_accuracy= needs the ground truth (x_gt) in the batch")
    n = int(batch["x_gt"].shape[0])
    if pocket_accuracy.n_pose_atoms != n:
        raise ValueError(f"pocket_accuracy= was built over {pocket_accuracy.n_pose_atoms} pose atoms, the batch holds {n}")


def check_conformer_rmsd(conformer_rmsd, batch) -> None:
    """redock(conformer_rmsd=): raise ValueError unless it is a `bestfit.BestFitRmsd` over the batch's ligand atoms"""
    if conformer_rmsd is None:
        return
    if not callable(getattr(conformer_rmsd, "to_reference", None)) or not hasattr(conformer_rmsd, "ligand_idx"):
        raise ValueError("conformer_rmsd= takes a bestfit.BestFitRmsd of the ligand")
    n = int(ligand_atom_mask(batch).sum())
    if conformer_rmsd.n_atoms is not None and conformer_rmsd.n_atoms != n:
        raise ValueError(f"conformer_rmsd= was built over {conformer_rmsd.n_atoms} ligand atoms, the batch's ligand holds {n}")


def score_conformer_rmsd(conformer_rmsd, aligned, batch, ligand_idx, pool=None) -> dict:
    """redock(conformer_rmsd=): {"conformer_rmsd": pairwise [n,n] (BestFitRmsd.pairwise of the kept poses), to_gt [n] (their best-fit
    RMSD to `x_gt`: the conformer accuracy, wherever the ligand sits) and, with a template pool [C,L,3], nearest_template /
    nearest_template_rmsd [n] (`cross` of the poses with the pool) and pool_to_gt (a scalar tensor: the pool's coverage of `x_gt`)}.
    A spec without `ligand_idx` is given the ligand atoms of the poses."""
    lig = ligand_idx.long()
    whole = conformer_rmsd.ligand_idx is not None
    x = aligned if whole else aligned[:, lig]
    res = {"pairwise": conformer_rmsd.pairwise(x)}
    gt = batch["x_gt"].float() if "x_gt" in batch else None
    if gt is not None:
        res["to_gt"] = conformer_rmsd.to_reference(x, gt if whole else gt[lig])["rmsd"]
    if pool is not None:
        pool = pool.to(aligned.device).float()
        near = conformer_rmsd.cross(x, pool)
        res["nearest_template"], res["nearest_template_rmsd"] = near["nearest"], near["nearest_rmsd"]
        if gt is not None:
            from .bestfit import BestFitRmsd
            r = BestFitRmsd(symmetry=conformer_rmsd.symmetry).cross(pool, gt[lig][None])["D"][:, 0]
            best = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).min()
            res["pool_to_gt"] = torch.where(torch.isinf(best), torch.full_like(best, float("nan")), best)
    return {"conformer_rmsd": res}


def conformer_pool(conformers, batch, seed, num_confs=128):
    """redock(conformers=): (ref_mol_poses [n,L,3], log) - the accepted conformers of `conformers.embed(num_confs, seed)` on the batch's
    device and their counts.  ValueError unless `conformers` is a `conformers.ConformerEnsemble` over the batch's ligand atoms, and
    when no conformer is accepted."""
    if not callable(getattr(conformers, "embed", None)) or not hasattr(conformers, "n_atoms"):
        raise ValueError("conformers= takes a conformers.ConformerEnsemble of the ligand")
    n = int(ligand_atom_mask(batch).sum())
    if conformers.n_atoms != n:
        raise ValueError(f"conformers= was built over {conformers.n_atoms} atoms, the batch's ligand holds {n}")
    got = conformers.embed(num_confs, 0 if seed is None else int(seed), device=batch["x_gt"].device)
    n_ok = int(got["poses"].shape[0])
    if n_ok == 0:
        raise ValueError(f"conformers=: none of the {num_confs} embedded conformers was accepted (largest bound violations from "
                         f"{float(got['max_violation'].min()):.3f} A)")
    return got["poses"], {"embedded": int(num_confs), "accepted": n_ok, "max_violation": got["max_violation"], "ok": got["ok"]}


def score_surface(surface, aligned, batch) -> dict:
    """redock(surface=): {"surface": BuriedSurface.measure of the kept poses} and, when the batch carries the ground truth,
    "surface_gt": its measure of `x_gt` (one pose)"""
    res = {"surface": surface.measure(aligned)}
    if "x_gt" in batch:
        res["surface_gt"] = surface.measure(batch["x_gt"].float()[None])
    return res


#: what redock(pocket=) keeps of PocketGrid.measure (the byte maps are left out: maps=False)
POCKET_KEYS = ("site_volume", "unfilled_volume", "pocket_volume", "filled_fraction", "ligand_in_site", "ligand_enclosure", "truncated",
               "lining_residues", "ok", "counts", "atom_buried", "lining_points")


def check_pocket(pocket, batch) -> None:
    """redock(pocket=): raise ValueError unless `pocket` is a `pocket.PocketGrid` over the batch's atoms"""
    if pocket is None:
        return
    if not callable(getattr(pocket, "measure", None)) or not hasattr(pocket, "n_pose_atoms"):
        raise ValueError("pocket= takes a pocket.PocketGrid of the system")
    n = int(batch["x_gt"].shape[0])
    if pocket.n_pose_atoms != n:
        raise ValueError(f"pocket= was built over {pocket.n_pose_atoms} pose atoms, the batch holds {n}")


def score_pocket(pocket, aligned, batch) -> dict:
    """redock(pocket=): {"pocket": the scalars, counts, atom_buried and lining_points of PocketGrid.measure of the kept poses} and, when
    the batch carries the ground truth, "pocket_gt": the same of `x_gt` (one pose)"""
    keep = lambda m: {k: m[k] for k in POCKET_KEYS}
    res = {"pocket": keep(pocket.measure(aligned, maps=False))}
    if "x_gt" in batch:
        res["pocket_gt"] = keep(pocket.measure(batch["x_gt"].float()[None], maps=False))
    return res


#: what redock(distogram=) reports of DistogramScore.score of the kept poses; `potential` comes from DistogramScore.potential
DISTOGRAM_KEYS = ("nll_interface", "nll_ligand", "token_nll", "expected_error", "contact_recovery", "contact_precision", "potential")


def check_distogram(distogram) -> None:
    """redock(distogram=): raise ValueError unless it is None, False, True or a dict of `DistogramScore.from_logits` keyword arguments"""
    if distogram is None or isinstance(distogram, bool):
        return
    if not isinstance(distogram, dict):
        raise ValueError(f"distogram= takes True or a dict of DistogramScore.from_logits keyword arguments, got {type(distogram).__name__}")
    bad = set(distogram) - {"contact_cutoff", "max_expected", "receptor", "min_bin", "max_bin", "pseudo_beta"}
    if bad:
        raise ValueError(f"distogram=: unknown DistogramScore.from_logits keyword arguments {sorted(bad)}")


def score_distogram(spec, aligned, out) -> dict:
    """redock(distogram=): {"distogram": the DISTOGRAM_KEYS of `spec.score` / `spec.potential` of the kept poses, "order_distogram":
    their ids by ascending nll_interface} and, when their validity was checked too, "order_distogram_valid" (valid poses in front)"""
    from .ranking import rank_by_score
    if spec is None:
        raise RuntimeError("distogram=: the sampler returned no conditioning to take the distogram from")
    found = dict(spec.score(aligned), **spec.potential(aligned))
    res = {"distogram": {k: found[k] for k in DISTOGRAM_KEYS}}
    res["order_distogram"] = rank_by_score(found["nll_interface"])
    if "validity" in out:
        res["order_distogram_valid"] = rank_by_score(found["nll_interface"], valid=out["validity"]["valid"])
    return res


def redock(model, batch: Dict[str, torch.Tensor], *, ref_mol=None, ref_mol_poses: Optional[torch.Tensor] = None,
           accept_fn: Optional[Callable[[torch.Tensor], bool]] = None, chirality=None, physics_correction: bool = False,
           max_samples: int = 5, max_rounds: int = 10, num_samples_per_round: int = 5, steps: int = 40,
           mmff_gamma_0_factor_start: float = 6.0, karras_noise_schedule_power: float = 1000, use_pocket: bool = True,
           align_weights: Optional[torch.Tensor] = None, ranking: bool = True, seed: Optional[int] = None,
           sampler_kwargs: Optional[dict] = None, infer_meta_data=None, reuse_conditioning: bool = True, confidence=None,
           ligand_symmetry=None, validity=None, validity_filter: bool = False, lddt_pli=None, vina=None,
           interactions=None, surface=None, refine=None, clusters=None, ring_interactions=None, hydrogens=None,
           conformers=None, sdf=None, search=None, receptor_geometry=None, conformer_rmsd=None, shape=None,
           torsions=None, pocket=None, distogram=None, flex=None, flex_search=None, pocket_accuracy=None, bond_stereo=None,
           bond_stereo_filter: bool = False) -> dict:
    """One system through the reference's round loop (defaults = redocking.py:33-59).  `batch` holds device tensors
    as for `model.sample_diffusion`; with physics correction it may hold `batch_msa_feat [rounds,S,T,34]`.
    Returns dict(poses [n,A,3] in the ground-truth frame, accepted (count before the top-up), rounds (per-round log),
    gamma_factor, ranking (ranking.rank_poses output or None)); with `infer_meta_data` (the loader's per-system naming
    tables) also `pdb_blocks` / `receptor_pdb_blocks`: the `write_pdb_block` text of every kept pose (redocking.py:342-345),
    formatted on the device for the whole batch (pdbio.py).
    `reuse_conditioning`: rounds that see the SAME features (no `batch_msa_feat` re-sampling) share one run of the conditioning
    trunk - the reference recomputes it in every `sample_diffusion` call (model.py:179) with identical inputs and hence identical
    outputs; here round 0 returns its (a, ap, s, z) and later rounds take them through `conditioning=`.  Bit-identical poses.
    `confidence` (a `ConfidenceModule` on the model's device, built for the model's c_s / c_z): the kept poses are also scored
    without the ground truth - `confidence` = `confidence.score_poses` of the returned `poses` (the aligned ones, in their order) with
    the trunk's (s, z) of the last sampler call, and `order_confidence` = `ranking.rank_by_confidence` of it, a device LongTensor
    over the kept poses.  `ranking`, its `order` and `rmsd` are what they are without it.
    `ligand_symmetry` (a `symmetry.LigandSymmetry` of the ligand's atoms in pose order): `ranking` is built from the
    symmetry-corrected ligand RMSD (`rank_poses(..., symmetry=)`); sampling, accept / reject and the confidence scores do not see it.
    `validity` (a `validity.PoseValidity` of the ligand): the result gains `validity` = its `check` of the returned `poses` (the
    aligned ones, in their order) and, together with `confidence=`, `order_confidence_valid` (`rank_by_confidence(..., valid=)`:
    valid poses first).  With `validity_filter=True` as well a pose that fails a check is rejected where and when the chirality test
    rejects (`physics_correction`, before `accept_fn`; the two masks share one read per round) and each round's log entry gains
    `invalid`, the number of poses that failed.  Nothing else changes.
    `lddt_pli` (an `lddt_pli.LddtPli` of the system): `ranking` gains the lDDT-PLI of the kept poses (`rank_poses(..., lddt_pli=)`).
    `vina` (a `scoring.VinaScore` of the system): the result gains `vina` = its `score` of the returned `poses` and `order_vina` =
    `ranking.rank_by_score` of it (lowest score first), and together with `validity=` also `order_vina_valid` (valid poses first).
    Nothing else changes.
    `interactions` (an `interactions.InteractionFingerprint` of the system): the result gains `interactions` = its `fingerprint` of
    the returned `poses` (per-residue and per-ligand-atom interaction bytes, closest distances, counts) and, as the batch carries
    `x_gt`, `interaction_recovery` = its `compare` of those bits with the ground truth's.  Nothing else changes, with or without
    `validity=`.
    `ring_interactions` (a `ring_interactions.RingInteractions` of the system): the result gains `ring_interactions` = its
    `fingerprint` of the returned `poses` (pi-stacking, pi-cation and halogen-bond bytes per residue, ligand atom and ligand ring, the
    ring frames, closest centroid distances, counts) and, as the batch carries `x_gt`, `ring_interaction_recovery` = its `compare` of
    those bits with the ground truth's.  Nothing else changes, with or without `interactions=`.
    `hydrogens` (a `hydrogens.Hydrogens` of the system): the result gains `hydrogens` = `x_h`, `placed`, `bits` and `counts` of its
    `hbonds` of the returned `poses` (the riding hydrogens, the rotatable polar ones turned to the partner, and the angle-tested
    hydrogen bonds per residue) and, as the batch carries `x_gt`, `hbond_recovery` = its `compare` of those bits with the ground
    truth's.  One built over another number of atoms raises ValueError before anything is sampled.  Nothing else changes.
    `conformers` (a `conformers.ConformerEnsemble` of the ligand): with `physics_correction=True` and no `ref_mol_poses` the template
    pool is the accepted conformers of its `embed(128, seed)` (distance geometry on the device, this package's own definition, not
    ETKDG) and the result gains `conformers` = `embedded`, `accepted`, `max_violation`, `ok`; when none is accepted, or it was built over
    another number of atoms, ValueError is raised before anything is sampled.  With `ref_mol_poses` given, or without physics
    correction, it is not used.  Nothing else changes.
    `sdf` (an `sdfio.SdfTemplate` of the ligand): the result gains `sdf` = its `format` of the returned `poses` in their order (`bytes`,
    `offsets`, `n_records` on the device: an SD file as it stands, `SdfTemplate.split` cuts it into records) with the data items of what
    the same call computed (`sdfio.redock_items`): always `pose`; with `confidence=` `ranking_confidence`; with `vina=` `vina_score`; with
    `validity=` `valid`; with the ground truth and `ranking` `ligand_rmsd`; with `lddt_pli=` `lddt_pli`; with `clusters=` `cluster`.  With
    `hydrogens=` given as well and a template made by `with_hydrogens` of that same object the records are protonated.  A template over
    another number of atoms raises ValueError before anything is sampled.  Nothing else changes.
    `surface` (a `surface.BuriedSurface` of the system): the result gains `surface` = its `measure` of the returned `poses` (the
    ligand's solvent-accessible area free and in the complex, the buried fraction and its polar / apolar split, the area each residue
    loses to the ligand) and, as the batch carries `x_gt`, `surface_gt` = its `measure` of the ground truth (one pose).  Nothing else
    changes.
    `refine` (a `refine.VinaRefine` of the system): the result gains `refined` = its `refine` of the returned `poses` (rigid-body and
    torsion minimisation in the rigid receptor: `x_refined`, energies, scores before and after, iterations, status, `moved`), with
    `validity=` also `refined["validity"]` (the check of `x_refined`) and with `vina=` also `order_vina_refined` (`rank_by_score` of
    the refined scores).  The returned `poses` are not replaced; nothing else changes.
    `search` (True for the defaults, or a dict of `VinaRefine.search` keyword arguments; needs `refine=`, a missing one raises
    ValueError before anything is sampled): the result gains `searched` = `refine.search` of the returned `poses` (the Monte-Carlo
    global search in the rigid receptor: `x_search`, `energy`, `best_chain`, every chain's best and its counts, scores before and
    after, `moved`), with `validity=` also `searched["validity"]` (the check of `x_search`) and with `vina=` also
    `order_vina_searched` (`rank_by_score` of the scores after the search).  The returned `poses` are not replaced; nothing else
    changes.
    `clusters` (a `clustering.PoseClusters` spec): the result gains `clusters` = the binding modes of the returned `poses`
    (`PoseClusters.cluster`: labels, leaders, medoids, sizes, radii, spreads, `dist`).  `metric="rmsd"` clusters their pairwise ligand RMSD
    (`ranking["dist"]` when `ranking` ran, else `pairwise_ligand_rmsd` with `ligand_symmetry=`), `metric="interactions"` clusters 1 -
    `interactions.pairwise(bits)` and needs `interactions=`.  The poses are walked in the order `by` names: `"confidence"` needs
    `confidence=`, `"vina"` needs `vina=`, `"vina_refined"` needs `refine=` and `vina=`; a missing prerequisite raises ValueError before
    anything is sampled.  With `vina=` the modes carry `mean_score`, with `validity=` only valid poses lead and join, and when `ranking`
    ran `clusters["leader_rmsd"]` is the RMSD to `x_gt` of each mode's leader (NaN behind `n_clusters`).  Nothing else changes.
    `receptor_geometry` (a `receptor_geometry.ReceptorGeometry` of the system): the result gains `receptor_geometry` = `val`, `flags`,
    `valid`, `counts` and `residue_flags` of its `check` of the returned `poses` (bond lengths and angles, chirality, peptide twist and
    cis flips, planarity and clashes of each pose's RECEPTOR), `chi_recovery` (its `chi_recovery` of them against `x_gt`) and, with
    `validity=`, `valid_both` (ligand and receptor both pass).  One built over another number of atoms raises ValueError before
    anything is sampled.  No pose is rejected for it; nothing else changes.
    `conformer_rmsd` (a `bestfit.BestFitRmsd` of the ligand): the result gains `conformer_rmsd` = `pairwise` (the best-fit ligand RMSD of
    every two returned `poses`: superposed on each other and corrected for the spec's symmetry table - their difference in CONFORMATION,
    wherever they sit), `to_gt` [n] (each pose's best-fit RMSD to `x_gt`) and, with a template pool in use (`ref_mol_poses` or
    `conformers=`), `nearest_template` / `nearest_template_rmsd` [n] (the pool conformer each pose is closest to) and `pool_to_gt` (a
    scalar tensor: the best-fit RMSD of the closest pool conformer to `x_gt`, the pool's coverage).  `clusters=PoseClusters(
    metric="conformer")` clusters `pairwise` and needs it; with `sdf=` the records gain the item `conformer_rmsd` (`to_gt`).  A spec over
    another number of ligand atoms raises ValueError before anything is sampled.  Nothing else changes.
    `shape` (a `shape.ShapeOverlap` of the ligand, or `(ShapeOverlap, (other_spec, y_ref))` to compare with another molecule's
    structure y_ref [A',3] in the ground truth's frame; the default reference is the ligand of `x_gt` with the same spec): the result
    gains `shape` = `shape_tanimoto`, `color_tanimoto`, `combo` [n] of the returned `poses` to the reference (Gaussian shape and feature
    overlap, in place) and `pairwise` (`ShapeOverlap.pairwise` of them), and `order_shape` = the pose ids by descending combo
    (`rank_by_score` of its negative; valid poses first with `validity=`).  `clusters=PoseClusters(metric="shape")` clusters 1 -
    `pairwise["shape_tanimoto"]` and needs it; with `sdf=` the records gain the items `shape_tanimoto` and `tanimoto_combo`.  A spec
    over another number of atoms raises ValueError before anything is sampled.  Nothing else changes.
    `torsions` (a `torsions.TorsionFingerprint` of the ligand): the result gains `torsions` = `pairwise` (the torsion-fingerprint deviation
    TFD of every two returned `poses`, in 0 .. 1), `to_gt` [n] and `deviation` [n,T] (each pose's TFD to `x_gt` and the normalised
    deviation of every entry of the fingerprint: which bond is wrong) and, with a template pool in use, `nearest_template` /
    `nearest_template_tfd` [n].  `clusters=PoseClusters(metric="torsion")` clusters `pairwise` and needs it; with `sdf=` the records gain
    the item `tfd` (`to_gt`).  A spec over another number of ligand atoms raises ValueError before anything is sampled.  Nothing else
    changes.
    `pocket` (a `pocket.PocketGrid` of the system): the result gains `pocket` = the scalars (`site_volume`, `unfilled_volume`,
    `pocket_volume`, `filled_fraction`, `ligand_in_site`, `ligand_enclosure`, `truncated`, `lining_residues`, `ok`), `counts`,
    `atom_buried` and `lining_points` of its `measure` of the returned `poses` (the cavity each pose's own receptor leaves around the
    ligand, how much of it the ligand fills, which atoms stick out and which residues line it) and, as the batch carries `x_gt`,
    `pocket_gt` = the same of the ground truth (one pose).  One built over another number of atoms raises ValueError before anything is
    sampled.  Nothing else changes.
    `distogram` (True for the defaults, or a dict of `distogram.DistogramScore.from_logits` keyword arguments): the kept poses are
    scored against the trunk's own distogram - the logits are `model.predict_distogram` of the (s, z) of the last sampler call, taken
    once per system exactly as `confidence=` takes them (a model whose sampler does not return its conditioning raises ValueError).
    The result gains `distogram` = `nll_interface`, `nll_ligand`, `token_nll`, `expected_error`, `contact_recovery`,
    `contact_precision` of `DistogramScore.score` and `potential` of the returned `poses`, `order_distogram` = `rank_by_score` of
    `nll_interface` (the pose the trunk's distances agree with best first) and, with `validity=`, `order_distogram_valid`;
    `clusters=PoseClusters(by="distogram")` walks `order_distogram` and needs it; with `sdf=` the records gain the item
    `distogram_nll`.  A batch without `token_id_to_pseudo_beta_atom_id` is scored on the first atom of every token.  Nothing else
    changes.
    `flex` (a `flex.FlexRefine` of the system; one built over another number of atoms raises ValueError before anything is sampled):
    the result gains `flex_refined` = its `refine` of the returned `poses` (the ligand and the chosen side chains minimised together:
    `x_refined`, energies and their parts, scores before and after, `moved`, `moved_flex`, `residue_moved`), with `validity=` also
    `flex_refined["validity"]`, with `receptor_geometry=` also `flex_refined["receptor_geometry"]` (its `check` of `x_refined`: the
    side chains moved) and with `vina=` also `order_vina_flex`.  The returned `poses` are not replaced; nothing else changes.
    `flex_search` (True for the defaults, or a dict of `FlexRefine.search` keyword arguments; needs `flex=`, a missing one or another
    type raises ValueError before anything is sampled): the result gains `flex_searched` = `flex.search` of the returned `poses` (the
    Monte-Carlo search with the side chains flexible: `x_search`, `energy` and its parts, `best_chain`, every chain's best and its
    counts, scores before and after, `moved`, `moved_flex`, `residue_moved`), with `validity=` also `flex_searched["validity"]`, with
    `receptor_geometry=` also `flex_searched["receptor_geometry"]` (their checks of `x_search`) and with `vina=` also
    `order_vina_flex_searched`.  The returned `poses` are not replaced; nothing else changes.
    `pocket_accuracy` (a `pocket_accuracy.PocketAccuracy` of the system; one built over another number of atoms, or a batch without
    `x_gt`, raises ValueError before anything is sampled): the result gains `pocket_accuracy` = its `score` of the returned `poses` (the
    lDDT of the ligand pocket with the naming swaps, per residue too, and the pocket's CA / backbone / heavy-atom RMSD after the
    superposition of its CA atoms, with the transform); with `sdf=` the records gain the items `lddt_lp` and `pocket_ca_rmsd`.  Nothing
    else changes.
    `bond_stereo` (a `bond_stereo.BondStereo` of the ligand's stated double bonds, atom indices into the pose; one built over another
    ligand atom count or reaching past the batch's atoms raises ValueError before anything is sampled): the result gains `bond_stereo`
    = `state`, `dihedral`, `twist`, `n_wrong`, `n_twisted` and `ok` of its `check` of the returned `poses` (is every stated double bond
    the cis / trans isomer it was written as, and how far is it twisted); with `sdf=` the records gain the item `stereo_ok`.  With
    `bond_stereo_filter=True` as well a pose with a wrong isomer is rejected where and when the chirality test rejects (physics
    correction); its mask joins the chirality and validity masks in the one host read.  Without the keywords nothing changes."""
    keywords = {k: v for k, v in locals().items() if k not in ("model", "batch")}
    st = _RedockState(batch, None, **keywords)
    if confidence is not None and not getattr(model, "supports_conditioning_reuse", False):
        raise ValueError("confidence= needs a model whose sampler returns its conditioning (return_conditioning=)")
    if distogram and not getattr(model, "supports_conditioning_reuse", False):
        raise ValueError("distogram= needs a model whose sampler returns its conditioning (return_conditioning=)")
    need_sz = confidence is not None or bool(distogram)      # the trunk's (s, z) of the last sampler call
    reuse = bool(reuse_conditioning and getattr(model, "supports_conditioning_reuse", False))
    for rnd in range(max_rounds):
        if not st.begin_round(rnd):
            break
        call = dict(num_sample=num_samples_per_round, steps=steps, mmff_gamma_0_factor=st.factor, align_ref_pos=rnd > 0,
                    ref_mol=st.sampler_ref_mol, ref_mol_poses=st.templates, use_ref_mol_poses=rnd != 0 and physics_correction,
                    ode_step_scale_eta=st.eta, karras_noise_schedule_power=karras_noise_schedule_power)
        if seed is not None:
            call.update(seed=seed + rnd)
        call.update(st.kw)
        if reuse and "conditioning" not in call and "return_conditioning" not in call:
            if st.cond is not None:
                call.update(conditioning=st.cond)
            elif st.later_round_shares_conditioning(rnd):
                call.update(return_conditioning=True)
        want_sz = need_sz and call.get("conditioning") is None and not call.get("return_conditioning")
        if want_sz:
            call.update(return_conditioning=True)
        with torch.no_grad():
            x_pred = model.sample_diffusion(st.batch, **call)
        got = None
        if isinstance(x_pred, tuple):
            x_pred, got = x_pred
            if need_sz:
                st.conf_sz = got[2:]
            if want_sz:
                got = None                   # asked for the confidence head / the distogram alone: not kept for later rounds
        elif need_sz and call.get("conditioning") is not None:
            st.conf_sz = call["conditioning"][2:]
        st.consume(rnd, x_pred, got)
    st.take_distogram(model)
    return st.result()


def conditioning_s_z(sz, T: int):
    """the trunk's (s [T,c_s], z [T,T,c_z]) at the system's real token count from the last two tensors of a sampler conditioning
    (s [T',c_s], z [T'*T',c_z] at the padded count T')"""
    s, z = sz
    Tp = s.shape[0]
    return s[:T], z.reshape(Tp, Tp, -1)[:T, :T]


def score_kept_poses(confidence, batch, sz, poses) -> dict:
    """redock(confidence=): {"confidence": ConfidenceModule.score_poses of the kept poses, "order_confidence": their ids best first}.
    The centre atom of a token is its first atom unless the batch names it (`token_id_to_centre_atom_id`); s_mask / a_mask default
    to ones.  (The chain index get_metrics caches is then cached in a copy of the batch: one read-back per redock call.)"""
    from .ranking import rank_by_confidence
    if sz is None:
        raise RuntimeError("confidence=: the sampler returned no conditioning to score the poses with")
    b = dict(batch)
    if "token_id_to_centre_atom_id" not in b:
        chunk = batch["token_id_to_chunk_sizes"].long()
        b["token_id_to_centre_atom_id"] = torch.cumsum(chunk, 0) - chunk
    for k, ref in (("s_mask", "is_ligand"), ("a_mask", "atom_id_to_token_id")):      # a batch without masks: every token / atom counts
        if k not in b:
            b[k] = torch.ones(batch[ref].shape[0], dtype=torch.float32, device=poses.device)
    s, z = conditioning_s_z(sz, b["token_id_to_centre_atom_id"].shape[0])
    scores = confidence.score_poses(b, s, z, poses)
    return {"confidence": scores, "order_confidence": rank_by_confidence(scores)}


def redock_many(model, systems, *, streams: Optional[int] = None, group: Optional[int] = None, **common) -> List[dict]:
    """The loop over systems of the reference's drivers (`redocking.py:128-154`: one `redocking(...)` call per input system;
    `screening.py:100-116`: one receptor x many ligands) on ONE GPU.  `systems`: an iterable of feature dicts, or of
    `(batch, per_system_kwargs)` pairs (any keyword of `redock`: what differs per system); `common`: keyword arguments of `redock`
    shared by all.  Results in input order.

    Rounds of few samples cannot fill an MI355X (20 samples per round, the drivers' setting: 70 % of the per-pose rate of a 64-sample
    call), and the systems are independent, so by default two of them are in flight on two HIP streams whenever a round has fewer
    than 32 samples (`parallel.StreamPool`: one model replica, stream and host thread each; poses are bit-identical to the
    one-at-a-time run, `tests/test_concurrent_streams_gpu.py`, `tests/test_configs_3_5_gpu.py`).  `streams=1` runs them one by one;
    rounds of 32 or more samples already fill the chip and run one by one unless `streams` says otherwise.  Across GPUs the same list
    is dealt out by `parallel.map_systems`.

    `group=G` samples up to G systems TOGETHER instead (`PhysDock.sample_diffusion_many`: one step loop, every denoiser launch over
    G x num_samples_per_round rows): the systems are dealt out in groups ordered by padded shape (`group_order`), each group's round
    loops run in lockstep - one grouped sampler call per round over its systems still active - with redock's per-system rules
    (accept / reject, adaptive threshold, template pool, conditioning reuse, top-up, ranking).  Systems whose relaxation runs on
    the host (an RDKit molecule on the host backend, `relax_fn=`) go through `redock` one by one.

    `confidence=module` (see `redock`) adds `confidence` / `order_confidence` to every result on each of these paths; `pool=` is
    the `parallel.StreamPool` to run on instead of the model's cached one."""
    items = [(s, {}) if isinstance(s, dict) else (s[0], dict(s[1])) for s in systems]
    pool = common.pop("pool", None)
    confidence = common.pop("confidence", None)      # popped before every branch (the sequential one included) and handed on by name
    on_gpu = bool(items) and items[0][0]["x_gt"].is_cuda and hasattr(model, "config")
    if group is not None and on_gpu and hasattr(model, "sample_diffusion_many"):
        out: List[Optional[dict]] = [None] * len(items)
        grouped = []
        for i, (b, kw) in enumerate(items):
            args = dict(common, **kw)
            if _needs_host_relax(model, b, args.get("ref_mol"), dict(args.get("sampler_kwargs") or {})):
                out[i] = redock(model, b, **{"confidence": confidence, **args})
            else:
                grouped.append(i)
        shapes = [tuple(model._prepare_batch(items[i][0])[k].shape[0] for k in ("ref_pos", "target_feat")) for i in grouped]
        for members in group_order(shapes, int(group)):
            idx = [grouped[m] for m in members]
            for i, r in zip(idx, _redock_group(model, [items[i] for i in idx], common, confidence)):
                out[i] = r
        return out
    n = streams if streams is not None else (2 if int(common.get("num_samples_per_round", 5)) < 32 else 1)
    if n <= 1 or len(items) <= 1 or not on_gpu:
        return [redock(model, b, **{**common, "confidence": confidence, **kw}) for b, kw in items]
    from .parallel import StreamPool
    pool = pool or StreamPool.for_model(model, n=n)      # cached on the model: replicas are built once
    if confidence is not None:
        confidence = _SerialConfidence(confidence)
    return pool.map(lambda m, it: redock(m, it[0], **{**common, "confidence": confidence, **it[1]}), items)


class _SerialConfidence:
    """one ConfidenceModule shared by the host threads / streams of a StreamPool: its engine's workspace buffers serve one call at a
    time, so a call holds a lock until its stream has drained (the only synchronisation the confidence path adds, and only here)"""

    def __init__(self, module):
        import threading
        self.module, self.lock = module, threading.Lock()

    def score_poses(self, *a, **k):
        with self.lock:
            r = self.module.score_poses(*a, **k)
            torch.cuda.current_stream().synchronize()
            return r


def group_order(shapes, group: int) -> List[List[int]]:
    """redock_many(group=G): the systems dealt out in groups of up to G, ordered by padded shape (largest first; input order
    among equal shapes) so that a group pads little.  shapes: per system a sortable padded shape, e.g. (A, T)."""
    if group < 1:
        raise ValueError(f"group={group}: expected a positive group size")
    order = sorted(range(len(shapes)), key=lambda i: (tuple(-int(v) for v in shapes[i]), i))
    return [order[k:k + group] for k in range(0, len(order), group)]


def _needs_host_relax(model, batch, ref_mol, kw) -> bool:
    """would this system's relaxation branch run on the host (an RDKit molecule on the host backend, or relax_fn=)?"""
    if ref_mol is None:
        return False
    n_mol = _mol_num_atoms(ref_mol)
    if n_mol is not None and n_mol != int(ligand_atom_mask(batch).sum()):
        return False                          # redock drops the molecule (ref_mol_num_error)
    if kw.get("relax_fn") is not None:
        return True
    from . import physics
    return physics.resolve_relaxer(ref_mol, None, kw.get("mmff_backend", "auto")).kind == "host"


class _RedockState:
    """one system's redocking run, round by round: the per-system rules of `redock` and of redock_many's lockstep round loop - their
    callers build the sampler call, sample, and hand the poses to `consume`.  `pbatch`: the system's prepared batch, padded to its
    group (`PhysDock._pad_to_group`); None for a single system, which samples from `batch`."""

    def __init__(self, batch, pbatch, *, ref_mol=None, ref_mol_poses=None, accept_fn=None, chirality=None, physics_correction=False,
                 max_samples=5, max_rounds=10, num_samples_per_round=5, mmff_gamma_0_factor_start=6.0, use_pocket=True,
                 align_weights=None, ranking=True, seed=None, sampler_kwargs=None, infer_meta_data=None, reuse_conditioning=True,
                 steps=40, karras_noise_schedule_power=1000, confidence=None, ligand_symmetry=None, validity=None,
                 validity_filter=False, lddt_pli=None, vina=None, interactions=None, surface=None, refine=None, clusters=None,
                 ring_interactions=None, hydrogens=None, conformers=None, sdf=None, search=None, receptor_geometry=None,
                 conformer_rmsd=None, shape=None, torsions=None, pocket=None, distogram=None, flex=None, flex_search=None,
                 pocket_accuracy=None, bond_stereo=None, bond_stereo_filter=False):
        # (the keywords of redock, no others: a misspelt one raises TypeError; each is kept under its own name.  steps and the schedule
        #  power go to the sampler from the caller)
        vars(self).update({k: v for k, v in locals().items() if k not in ("self", "batch", "pbatch")})
        check_redock_prerequisites(clusters, confidence=confidence, vina=vina, refine=refine, interactions=interactions,
                                   conformer_rmsd=conformer_rmsd, shape=shape, torsions=torsions, distogram=distogram)
        check_distogram(distogram)
        check_redock_shape(shape, batch)
        check_redock_torsions(torsions, batch)
        check_search(search, refine)
        check_hydrogens(hydrogens, batch)
        check_pocket(pocket, batch)
        check_receptor_geometry(receptor_geometry, batch)
        check_pocket_accuracy(pocket_accuracy, batch)
        check_flex_search(flex_search, flex)
        check_flex(flex, batch)
        check_conformer_rmsd(conformer_rmsd, batch)
        check_redock_sdf(sdf, batch, hydrogens)
        check_redock_bond_stereo(bond_stereo, bond_stereo_filter, batch)
        self.pool_log = None
        if physics_correction and ref_mol_poses is None and conformers is not None:
            ref_mol_poses, self.pool_log = conformer_pool(conformers, batch, seed)
        if physics_correction and ref_mol_poses is None:
            raise ValueError("physics correction needs reference conformers (ref_mol_poses [C,L,3]); the reference generates "
                             "them with RDKit ETKDG (redocking.py:231-243), which this build does not include")
        self.batch, self.pbatch = dict(batch), None if pbatch is None else dict(pbatch)
        # (the reference accepts host conformers: `.to(device)`, model.py:185)
        self.ref_mol_poses = ref_mol_poses.to(batch["x_gt"].device) if ref_mol_poses is not None else None
        self.is_lig = ligand_atom_mask(batch)
        self.ligand_idx = torch.nonzero(self.is_lig).flatten().to(torch.int32)
        self.accept, self.reject = [], deque([], maxlen=max_samples)
        self.ligand_templates, self.reference_templates = [], []
        self.factor = float(mmff_gamma_0_factor_start)
        self.log = []
        self.kw = dict(sampler_kwargs or {})
        n_mol = _mol_num_atoms(ref_mol) if ref_mol is not None else None
        ref_mol_num_error = ref_mol is None or (n_mol is not None and n_mol != int(self.is_lig.sum()))     # redocking.py:195-196
        self.sampler_ref_mol, self.eta = (None, 1.5) if ref_mol_num_error else (ref_mol, 1.0)      # ... :292,296
        self.cond = None                     # the conditioning that rounds with the same features share
        self.conf_sz = None                  # confidence= / distogram=: (s, z) of the most recent sampler call, set by the caller
        self.distogram_spec = None           # distogram=: the system's DistogramScore, built once behind the round loop
        self.done, self.templates = False, None

    def begin_round(self, rnd) -> bool:
        """does round `rnd` run?  If so, its MSA is in place (`batch`, and `pbatch` at the group's token count) and `templates` is
        its template stack"""
        if self.done or (rnd > 0 and not self.physics_correction):
            self.done = True
            return False
        if rnd >= 1 and "batch_msa_feat" in self.batch:
            if rnd >= self.batch["batch_msa_feat"].shape[0]:
                raise ValueError(f"batch_msa_feat holds {self.batch['batch_msa_feat'].shape[0]} re-sampled MSAs, round {rnd} needs "
                                 "its own (the reference loads num_recycles = max_rounds of them, redocking.py:83)")
            msa = self.batch["batch_msa_feat"][rnd]
            self.batch["msa_feat"] = msa
            if self.pbatch is not None:
                pt = self.pbatch["target_feat"].shape[0] - msa.shape[1]        # the group-padded token count
                self.pbatch["msa_feat"] = torch.nn.functional.pad(msa.float(), (0, 0, 0, pt)).contiguous()
            self.cond = None                 # a re-sampled MSA: this round's trunk is its own
        self.templates = torch.stack(self.ligand_templates + self.reference_templates, 0) if rnd > 0 else None
        return True

    def later_round_shares_conditioning(self, rnd) -> bool:
        """can a round after `rnd` take this round's conditioning (there is one, and it sees the same features)?"""
        return self.physics_correction and rnd + 1 < self.max_rounds and "batch_msa_feat" not in self.batch

    def consume(self, rnd, x_pred, cond):
        """this round's poses: accept / reject (redocking.py:303-317), the log entry, the adaptive factor and the template pool of the
        next round; `cond`: the conditioning the sampler returned for later rounds, or None"""
        if cond is not None and self.reuse_conditioning:
            self.cond = cond
        if rnd + 1 >= self.max_rounds:       # no later round can take it: the shared conditioning (clones of a [A,c], ap [A,A,c], s,
            self.cond = None                 # z [T,T,128] - hundreds of MB at large crops, per StreamPool replica) is released here
        # on the device when a ChiralityReference or a validity filter is given (one [*, B] mask to the host), and / or through the
        # injected per-pose callable (which needs the poses on the host)
        pc = self.physics_correction
        dev_ok, n_invalid = _device_accept(x_pred, self.chirality, self.validity if self.validity_filter else None,
                                           self.bond_stereo if self.bond_stereo_filter else None) if pc else (None, None)
        x_cpu = x_pred.cpu() if (pc and self.accept_fn is not None) else x_pred
        flags = []
        for b, (x, xc) in enumerate(zip(x_pred, x_cpu)):
            ok = True
            if dev_ok is not None:
                ok = bool(dev_ok[b])
            if ok and pc and self.accept_fn is not None:
                ok = bool(self.accept_fn(xc))
            flags.append(ok)
            if ok:
                self.ligand_templates.append(x[self.is_lig])
                self.accept.append(x)
            else:
                self.reject.append(x)
        self.log.append({"round": rnd, "gamma_factor": self.factor, "accepted": int(sum(flags)), "sampled": len(flags),
                         "templates": 0 if self.templates is None else int(self.templates.shape[0])})
        if n_invalid is not None:
            self.log[-1]["invalid"] = n_invalid
        if pc:
            self.factor = next_gamma_factor(self.factor, any(flags))
            if len(self.accept) >= self.max_samples:
                self.cond, self.done = None, True        # accept count reached: the shared conditioning is released with the loop
                return
            used = select_reference_templates(x_pred, self.ligand_idx, self.ref_mol_poses, self.max_samples - len(self.ligand_templates))
            self.reference_templates = [self.ref_mol_poses[i] for i in used.tolist()]
        else:
            self.done = True
        if rnd + 1 >= self.max_rounds:
            self.done = True

    def take_distogram(self, model) -> None:
        """distogram=: the system's logits and tables from the (s, z) of its most recent sampler call - once, behind the round loop"""
        if self.distogram and self.conf_sz is not None:
            from .distogram import DistogramScore
            kw = self.distogram if isinstance(self.distogram, dict) else {}
            self.distogram_spec = DistogramScore.from_conditioning(model, self.batch, self.conf_sz, **kw)

    def result(self) -> dict:
        """top-up with rejected poses, alignment into the ground-truth frame, ranking, the pose scorers in their order (score_vina
        reads out["validity"], cluster_kept_poses almost everything, score_sdf comes last) and the PDB text"""
        self.cond = None
        batch, ligand_idx = self.batch, self.ligand_idx
        n_accepted = len(self.accept)
        accept = self.accept + list(self.reject) if n_accepted < self.num_samples_per_round else self.accept
        poses = torch.stack(accept[:self.max_samples], 0)
        w = self.align_weights if self.align_weights is not None else pocket_align_weights(batch, self.use_pocket)
        x_gt = batch["x_gt"].float()
        aligned = weighted_rigid_align(x_gt[None].expand(poses.shape[0], -1, -1).contiguous(), poses, w)
        out = {"poses": aligned, "accepted": n_accepted, "rounds": self.log, "gamma_factor": self.factor, "ranking": None}
        if self.ranking:
            out["ranking"] = rank_poses(poses, x_gt, w, self.is_lig, symmetry=self.ligand_symmetry, lddt_pli=self.lddt_pli)
        if self.confidence is not None:
            out.update(score_kept_poses(self.confidence, batch, self.conf_sz, aligned))
        if self.validity is not None:
            out.update(score_validity(self.validity, aligned, out))
        if self.vina is not None:
            out.update(score_vina(self.vina, aligned, out))
        if self.interactions is not None:
            out.update(score_interactions(self.interactions, aligned, batch))
        if self.ring_interactions is not None:
            out.update(score_ring_interactions(self.ring_interactions, aligned, batch))
        if self.hydrogens is not None:
            out.update(score_hydrogens(self.hydrogens, aligned, batch))
        if self.receptor_geometry is not None:
            out.update(score_receptor_geometry(self.receptor_geometry, aligned, batch, out))
        if self.pocket_accuracy is not None:
            out["pocket_accuracy"] = self.pocket_accuracy.score(aligned)
        if self.bond_stereo is not None:
            out.update(score_bond_stereo(self.bond_stereo, aligned))
        if self.pool_log is not None:
            out["conformers"] = self.pool_log
        if self.surface is not None:
            out.update(score_surface(self.surface, aligned, batch))
        if self.pocket is not None:
            out.update(score_pocket(self.pocket, aligned, batch))
        if self.refine is not None:
            out.update(score_refined(self.refine, aligned, self.validity, self.vina))
        if self.search:
            out.update(score_searched(self.search, self.refine, aligned, self.validity, self.vina))
        if self.flex is not None:
            out.update(score_flex_refined(self.flex, aligned, self.validity, self.vina, self.receptor_geometry))
        if self.flex_search:
            out.update(score_flex_searched(self.flex_search, self.flex, aligned, self.validity, self.vina, self.receptor_geometry))
        if self.conformer_rmsd is not None:
            out.update(score_conformer_rmsd(self.conformer_rmsd, aligned, batch, ligand_idx, self.ref_mol_poses))
        if self.shape is not None:
            out.update(score_shape(self.shape, aligned, batch, ligand_idx, out))
        if self.torsions is not None:
            out.update(score_torsions(self.torsions, aligned, batch, ligand_idx, self.ref_mol_poses))
        if self.distogram:
            out.update(score_distogram(self.distogram_spec, aligned, out))
        if self.clusters is not None:
            out.update(cluster_kept_poses(self.clusters, aligned, ligand_idx, out, interactions=self.interactions,
                                          ligand_symmetry=self.ligand_symmetry))
        if self.sdf is not None:
            out.update(score_sdf(self.sdf, aligned, out))
        if self.infer_meta_data is not None:
            out["pdb_blocks"] = PdbTemplate(self.infer_meta_data).blocks(aligned)
            out["receptor_pdb_blocks"] = PdbTemplate(self.infer_meta_data, receptor_only=True).blocks(aligned)
        return out


_MANY_SAMPLER_KEYS = {"seed", "sample_offset", "noise", "use_graph", "mmff_backend", "mmff_iters"}


def _redock_group(model, items, common, confidence=None) -> List[dict]:
    """redock for the systems of one group, their round loops in lockstep: each round is ONE sample_diffusion_many call over the
    systems still active (same schedule and sample count for all; per-system threshold, template pool, seed, relaxation)"""
    pbs = model._pad_to_group([model._prepare_batch(b) for b, _ in items])
    states = []
    for (b, kw), pb in zip(items, pbs):
        args = dict(common, **kw)
        bad = set((args.get("sampler_kwargs") or {})) - _MANY_SAMPLER_KEYS
        if bad:
            raise ValueError(f"redock_many(group=): sampler_kwargs {sorted(bad)} are not supported by grouped sampling")
        states.append(_RedockState(b, pb, **{"confidence": confidence, **args}))
        if states[-1].distogram and not getattr(model, "supports_conditioning_reuse", False):
            raise ValueError("distogram= needs a model whose sampler returns its conditioning (return_conditioning=)")
    for k in ("steps", "karras_noise_schedule_power", "num_samples_per_round", "use_graph", "mmff_backend", "mmff_iters"):
        # one sampler call per round serves the whole group: what it shares must be the same for every system
        vals = {repr(st.kw.get(k)) if k in _MANY_SAMPLER_KEYS else repr(dict(common, **kw).get(k)) for st, (_, kw) in zip(states, items)}
        if len(vals) > 1:
            raise ValueError(f"redock_many(group=): the systems of one group differ in {k} ({sorted(vals)}); it is shared by "
                             "the grouped sampler call - give it in the common keywords or run those systems without group=")
    args0 = dict(common, **items[0][1])
    steps = int(args0.get("steps", 40))
    power = args0.get("karras_noise_schedule_power", 1000)
    nspr = int(args0.get("num_samples_per_round", 5))
    max_rounds = max(st.max_rounds for st in states)      # (each system stops at its own max_rounds: begin_round / consume)
    for rnd in range(max_rounds):
        active = [st for st in states if st.begin_round(rnd)]
        if not active:
            break
        want_cond = [st.reuse_conditioning and st.cond is None and st.later_round_shares_conditioning(rnd) for st in active]
        noises = [st.kw.get("noise") for st in active]
        call = dict(num_sample=nspr, steps=steps, align_ref_pos=rnd > 0, karras_noise_schedule_power=power,
                    mmff_gamma_0_factor=[st.factor for st in active], ode_step_scale_eta=[st.eta for st in active],
                    ref_mol=[st.sampler_ref_mol for st in active], ref_mol_poses=[st.templates for st in active],
                    seeds=[st.kw.get("seed", (st.seed + rnd) if st.seed is not None else 0) for st in active],
                    sample_offsets=[st.kw.get("sample_offset", 0) for st in active], conditionings=[st.cond for st in active],
                    return_conditioning=confidence is not None or any(want_cond) or any(bool(st.distogram) for st in active))
        if any(nz is not None for nz in noises):
            call.update(noises=noises)
        for k in ("use_graph", "mmff_backend", "mmff_iters"):
            if k in active[0].kw:
                call[k] = active[0].kw[k]
        with torch.no_grad():
            r = model.sample_diffusion_many([st.pbatch for st in active], **call)
        outs, conds = r if isinstance(r, tuple) else (r, [None] * len(active))
        for st, want, x, c in zip(active, want_cond, outs, conds):
            if (confidence is not None or st.distogram) and c is not None:
                st.conf_sz = c[2:]               # (s, z) at the group's padded token count: conditioning_s_z crops them
            st.consume(rnd, x, c if want else None)
    for st in states:
        st.take_distogram(model)
    return [st.result() for st in states]
