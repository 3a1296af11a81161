"""get_metrics: the inference-time confidence scores of the reference's PhysDock/data/tools/get_metrics.py on the device
(csrc/metrics.hip): per-atom pLDDT and its mean, the expected aligned error, pTM / ipTM, the chain clash flag and

    ranking_confidence = 0.8 ipTM + 0.2 pTM - has_clash

the ground-truth-free score poses are ranked by.

    p_pae, p_pde, p_plddt = confidence(batch, s, z, x_pred)
    m = get_metrics({"p_plddt": p_plddt, "p_pae": p_pae, "x_pred": x_pred}, batch)       # the reference's keys, leading dim 1
    m = get_metrics(..., all_poses=True)          # has_clash / ranking_confidence for every row of x_pred
    m = get_metrics({"p_plddt": [P,A,nb], "p_pae": [P,T,T,nb], "x_pred": [P,A,3]}, batch)   # P logit sets in one launch

The reference moves the logits to the host and scores pose 0 in numpy; here nothing leaves the device, the logits are read once
and no call synchronises - with ONE exception: the dense chain index of a system (np.unique of asym_id) is computed on the first
call for a batch dict, which reads the number of chains back, and cached in the dict under the private key `_metrics_chain`
together with the per-atom polymer flag (as PhysDock._prepare_batch caches its derived tensors).  A dict whose asym_id,
atom_id_to_token_id or is_ligand are replaced afterwards needs that key deleted.  After that first call a get_metrics call can be
captured in a graph.

Two quirks of the reference, decided here:
* its chain loop `for a in uniq[:-1]: for b in uniq[1:]` pairs a middle chain with itself when three or more polymer chains have
  atoms; the zero self-distances then give n_clash >= N and has_clash = 1 whatever the geometry.  That is reproduced by default
  (the fixtures come from the unmodified reference); `skip_self_pairs=True` restricts the loop to a < b.
* `~is_ligand` is a logical not only for a bool array (a bitwise not for ints, an error for floats); `is_ligand == 0` is used for
  every dtype, as ConfidenceLoss does.  is_protein / is_dna / is_rna, read but never used by the reference, are not required.
"""
from __future__ import annotations

import torch

from . import _lib as ops

__all__ = ["get_metrics", "compute_plddt", "compute_predicted_aligned_error", "predicted_tm_score", "get_has_clash", "bin_centres"]

MAX_CHAINS = 64
_CACHE_KEY = "_metrics_chain"
_centres = {}


def _dev(what, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"physdock_amd.{what} runs on an MI355X (HIP) device only; there is no CPU path "
                               "(move the outputs and features to the device)")


def _f(t):
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def _i32(t):
    return t if t.dtype == torch.int32 and t.is_contiguous() else t.to(torch.int32).contiguous()


def _centres_cpu(max_bin, no_bins):
    """the bin centres as the reference forms them, with the same torch fp32 operations (get_metrics: linspace;
    _calculate_bin_centers: breaks + step / 2, the last centre one step further)"""
    breaks = torch.linspace(0., float(max_bin), no_bins - 1)
    step = breaks[1] - breaks[0]
    c = breaks + step / 2
    return torch.cat([c, (c[-1] + step)[None]])


def bin_centres(device, max_bin=32.0, no_bins=64):
    """device table [no_bins] of the PAE bin centres; one per (device, max_bin, no_bins), built on the host once"""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(), float(max_bin), int(no_bins))
    if key not in _centres:
        if no_bins < 3:
            raise ValueError(f"no_bins must be at least 3, got {no_bins}")
        _centres[key] = _centres_cpu(max_bin, no_bins).to(device)
    return _centres[key]


def _plddt(logits):
    """logits [P,A,nb] fp32 contiguous -> atom_plddts [P,A], mean_plddt [P]"""
    P, A, nb = logits.shape
    atom = torch.empty(P, A, dtype=torch.float32, device=logits.device)
    mean = torch.empty(P, dtype=torch.float32, device=logits.device)
    ops.check(ops.init().pd_metrics_plddt(ops.ptr(logits), ops.ptr(atom), ops.ptr(mean), P, A, nb, ops.stream()), "metrics_plddt")
    return atom, mean


def _pae_tm(logits, w, asym, max_bin, want_pae=True, want_rows=False):
    """logits [P,T,T,nb] fp32 contiguous -> dict pae [P,T,T] | None, ptm, iptm [P], rows [P,2] int32, per_alignment [P,2,T] | None"""
    P, T, T2, nb = logits.shape
    if T != T2 or tuple(w.shape) != (T,) or (asym is not None and tuple(asym.shape) != (T,)):
        raise ValueError(f"p_pae must be [.., T, T, bins] with weights / asym_id [T], got {tuple(logits.shape)}, {tuple(w.shape)}")
    L, dev = ops.init(), logits.device
    n = L.pd_metrics_workspace_numel(P, T)
    ops.check(min(n, 0), "metrics_workspace_numel")
    ws = torch.empty(n, dtype=torch.float32, device=dev)
    pae = torch.empty(P, T, T, dtype=torch.float32, device=dev) if want_pae else None
    ptm, iptm = torch.empty(P, dtype=torch.float32, device=dev), torch.empty(P, dtype=torch.float32, device=dev)
    rows = torch.empty(P, 2, dtype=torch.int32, device=dev)
    pa = torch.empty(P, 2, T, dtype=torch.float32, device=dev) if want_rows else None
    ops.check(L.pd_metrics_pae_tm(ops.ptr(logits), ops.ptr(bin_centres(dev, max_bin, nb)), ops.ptr(w), ops.ptr(asym), ops.ptr(ws),
                                  ops.ptr(pae), ops.ptr(ptm), ops.ptr(iptm), ops.ptr(rows), ops.ptr(pa), P, T, nb, ops.stream()),
              "metrics_pae_tm")
    return {"pae": pae, "ptm": ptm, "iptm": iptm, "rows": rows, "per_alignment": pa}


def _clash(x, a_mask, chain, poly, n_chain, skip_self_pairs, ptm=None, iptm=None):
    """x [B,A,3] -> has_clash [B] int64 and, with ptm / iptm ([1] shared or [B]), ranking_confidence [B]"""
    B, A = x.shape[0], x.shape[1]
    if n_chain > MAX_CHAINS:
        raise ValueError(f"get_has_clash supports at most {MAX_CHAINS} chains, got {n_chain}")
    dev = x.device
    counts = torch.empty(B * n_chain * n_chain, dtype=torch.int32, device=dev)
    has = torch.empty(B, dtype=torch.int64, device=dev)
    rank = torch.empty(B, dtype=torch.float32, device=dev) if ptm is not None else None
    stride = 0 if ptm is None or ptm.shape[0] == 1 else 1
    ops.check(ops.init().pd_metrics_clash(ops.ptr(x), ops.ptr(a_mask), ops.ptr(chain), ops.ptr(poly), ops.ptr(counts), ops.ptr(ptm),
                                          ops.ptr(iptm), stride, ops.ptr(has), ops.ptr(rank), B, A, int(n_chain), int(bool(skip_self_pairs)),
                                          ops.stream()), "metrics_clash")
    return has, rank


def _dense_chain(asym_atom):
    """(dense chain index [A] int32 in ascending asym_id order, number of chains): torch.unique, which synchronises"""
    uniq, inv = torch.unique(asym_atom, sorted=True, return_inverse=True)
    return inv.to(torch.int32).contiguous(), int(uniq.shape[0])


def _chain_index(batch):
    """(dense chain index [A] int32, per-atom polymer flag [A] fp32, number of chains) of a batch dict, computed on the first call
    (one read-back, see the module docstring) and cached in the dict"""
    cached = batch.get(_CACHE_KEY)
    if cached is None:                                       # once per system: torch.unique reads the chain count back
        idx = batch["atom_id_to_token_id"].long()
        chain, n_chain = _dense_chain(batch["asym_id"][idx])
        cached = batch[_CACHE_KEY] = (chain, (batch["is_ligand"] == 0)[idx].float().contiguous(), n_chain)
    return cached


def _poses(x_pred):
    x = _f(x_pred)
    if x.dim() == 2:
        x = x[None]
    if x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError(f"x_pred must be [num_poses, num_atoms, 3], got {tuple(x_pred.shape)}")
    return x


@torch.no_grad()
def compute_plddt(logits):
    """reference compute_plddt: logits [A,nb] (or [P,A,nb]) -> per-atom pLDDT in [0, 100], 100 sum_k softmax_k (k + 0.5) / nb"""
    _dev("compute_plddt", logits)
    one = logits.dim() == 2
    atom, _ = _plddt(_f(logits[None] if one else logits))
    return atom[0] if one else atom


@torch.no_grad()
def compute_predicted_aligned_error(logits, max_bin=32.0):
    """reference compute_predicted_aligned_error without the [T,T,nb] probabilities (they never exist here): logits [T,T,nb] (or
    [P,T,T,nb]) -> {"predicted_aligned_error": [T,T], "max_predicted_aligned_error": 0-d}; breaks = linspace(0, max_bin, nb - 1)"""
    _dev("compute_predicted_aligned_error", logits)
    one = logits.dim() == 3
    lg = _f(logits[None] if one else logits)
    T = lg.shape[1]
    r = _pae_tm(lg, torch.ones(T, dtype=torch.float32, device=lg.device), None, max_bin)
    return {"predicted_aligned_error": r["pae"][0] if one else r["pae"],
            "max_predicted_aligned_error": bin_centres(lg.device, max_bin, lg.shape[-1])[-1]}


@torch.no_grad()
def predicted_tm_score(logits, residue_weights=None, asym_id=None, interface=False, max_bin=32.0, return_row=False):
    """reference predicted_tm_score: logits [T,T,nb] (or [P,T,T,nb]) -> pTM, or ipTM with interface=True (needs asym_id), as a
    0-d ([P]) tensor: per_alignment at the first maximal row of per_alignment_i w_i.  return_row=True also returns that row index
    (int32) and per_alignment [T] ([P,T]) of every row."""
    _dev("predicted_tm_score", logits)
    if interface and asym_id is None:
        raise ValueError("interface=True needs asym_id")
    one = logits.dim() == 3
    lg = _f(logits[None] if one else logits)
    T = lg.shape[1]
    w = torch.ones(T, dtype=torch.float32, device=lg.device) if residue_weights is None else _f(residue_weights)
    r = _pae_tm(lg, w, _i32(asym_id) if interface else None, max_bin, want_pae=False, want_rows=return_row)
    q = 1 if interface else 0
    val = r["iptm" if interface else "ptm"]
    if not return_row:
        return val[0] if one else val
    rows, pa = r["rows"][:, q], r["per_alignment"][:, q]
    return (val[0], rows[0], pa[0]) if one else (val, rows, pa)


@torch.no_grad()
def get_has_clash(atom_pos, atom_mask, asym_id, is_polymer_chain, skip_self_pairs=False):
    """reference get_has_clash: atom_pos [A,3] (or [B,A,3]), atom_mask, asym_id, is_polymer_chain [A] per ATOM -> 0 / 1 (int64,
    0-d or [B]): 1 if for a pair of polymer chains more than 100 atom pairs, or more than half the atoms of the smaller chain,
    are closer than 1.1.  Synchronises (the chain index of asym_id is formed here); get_metrics caches it instead."""
    _dev("get_has_clash", atom_pos, atom_mask, asym_id, is_polymer_chain)
    one = atom_pos.dim() == 2
    x = _poses(atom_pos)
    chain, n = _dense_chain(asym_id)
    has, _ = _clash(x, _f(atom_mask), chain, _f(is_polymer_chain != 0), n, skip_self_pairs)
    return has[0] if one else has


@torch.no_grad()
def get_metrics(output, batch, *, all_poses=False, skip_self_pairs=False):
    """The reference's get_metrics(output, batch) on the device.  output: p_plddt [A,nb], p_pae [T,T,nb], x_pred [B,A,3];
    batch: s_mask, asym_id, is_ligand [T], a_mask, atom_id_to_token_id [A].  Returns fp32 device tensors (has_clash int64) with
    the reference's keys and leading dim 1: atom_plddts [1,A], mean_plddt [1], pae [1,T,T], ptm [1], iptm [1], has_clash [1],
    ranking_confidence [1]; as there, only pose 0 of x_pred is scored.  Beyond the reference:
    * all_poses=True: has_clash and ranking_confidence for every row of x_pred, [B] (ptm / iptm are shared and stay [1]);
    * stacked logits p_plddt [P,A,nb], p_pae [P,T,T,nb] with x_pred [P,A,3]: P poses in one launch, every output with leading dim P.
    * skip_self_pairs=True: the chain loop of the clash rule over a < b only (the reference's loop pairs a middle chain with
      itself, which flags every system of three or more polymer chains; the default reproduces that).
    The polymer flag is `is_ligand == 0` for every dtype.  No host synchronisation except on the first call for a batch dict (the
    chain index, cached under batch["_metrics_chain"]; see the module docstring).  Raises without a GPU or a built library."""
    p_plddt, p_pae, x_pred = output["p_plddt"], output["p_pae"], output["x_pred"]
    s_mask, asym, a_mask, a2t, is_lig = (batch[k] for k in ("s_mask", "asym_id", "a_mask", "atom_id_to_token_id", "is_ligand"))
    _dev("get_metrics", p_plddt, p_pae, x_pred, s_mask, asym, a_mask, a2t, is_lig)
    stacked = p_pae.dim() == 4
    if p_plddt.dim() != (3 if stacked else 2) or p_pae.dim() not in (3, 4):
        raise ValueError(f"p_plddt / p_pae must be [A,nb] / [T,T,nb] or [P,A,nb] / [P,T,T,nb], got {tuple(p_plddt.shape)} / {tuple(p_pae.shape)}")
    lp, la = _f(p_plddt if stacked else p_plddt[None]), _f(p_pae if stacked else p_pae[None])
    x = _poses(x_pred)
    P, A, T = la.shape[0], lp.shape[1], la.shape[1]
    if lp.shape[0] != P or x.shape[1] != A or tuple(a_mask.shape) != (A,) or tuple(a2t.shape) != (A,) or tuple(is_lig.shape) != (T,):
        raise ValueError(f"inconsistent shapes: p_plddt {tuple(p_plddt.shape)}, p_pae {tuple(p_pae.shape)}, x_pred {tuple(x_pred.shape)}, "
                         f"a_mask {tuple(a_mask.shape)}, is_ligand {tuple(is_lig.shape)}")
    if stacked:
        if x.shape[0] != P:
            raise ValueError(f"stacked logits of {P} poses need x_pred with {P} rows, got {x.shape[0]}")
    elif not all_poses:
        x = x[:1]
    chain, poly, n_chain = _chain_index(batch)
    atom, mean = _plddt(lp)
    r = _pae_tm(la, _f(s_mask), _i32(asym), 32.0)
    has, rank = _clash(x, _f(a_mask), chain, poly, n_chain, skip_self_pairs, r["ptm"], r["iptm"])
    return {"atom_plddts": atom, "mean_plddt": mean, "pae": r["pae"], "ptm": r["ptm"], "iptm": r["iptm"], "has_clash": has,
            "ranking_confidence": rank}
