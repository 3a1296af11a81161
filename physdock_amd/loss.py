"""PhysDockLoss: the five-term loss of the training-time forward, on the device (reference PhysDock/models/loss.py:78-181,
245-318, 535-559, 576-625).  Forward values only - no gradients.

    outputs = model(batch)                                   # x_denoised, x_hat, t_hat, p_distogram
    cum_loss, losses = PhysDockLoss(cfg)(outputs, batch)     # or: model(batch, return_loss=True)

The kernels (csrc/loss.hip) form every atom / token pair in registers, so none of the reference's [B,A,A], [B,T,T] or
[T,T,39] tensors exists; reductions are ordered, so a call gives the same bits every time.

Sizes: `PhysDock.forward` returns its tensors cut to the REAL atom / token counts of the system, and the loss takes `feats`
in the same real sizes - pass the batch as the feature loader made it, not a padded copy.

`feats` uses the reference's key names: x_gt [A,3], x_exists [A] (falls back to a_mask), atom_id_to_token_id [A],
token_id_to_centre_atom_id [T], token_id_to_pseudo_beta_atom_id [T], token_bonds [T,T], is_dna / is_rna / is_ligand /
is_key_res [T].  As in the reference, what the functions compute is what its code does, not what its comments say:
weighted_mse_loss uses sigma_data = 16 whatever it is given and one masked mean over samples AND atoms; bond_loss and
key_res_loss multiply the sample mean of the EDM scale with the sample mean of the masked sum; a non-finite coordinate makes
a term NaN even where its mask is zero (0 * NaN), and PhysDockLoss replaces such a term by zero with a warning.
"""
from __future__ import annotations

import logging

import torch

from . import _lib as ops

__all__ = ["PhysDockLoss", "weighted_mse_loss", "smooth_lddt_loss", "bond_loss", "key_res_loss", "distogram_loss"]

LOSS_TERMS = ("weighted_mse_loss", "smooth_lddt_loss", "bond_loss", "key_res_loss", "distogram_loss")


def _dev(what, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"physdock_amd.{what} runs on an MI355X (HIP) device only; there is no CPU path "
                               "(move the outputs and features to the device)")


def _f(t):
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def _l(t):
    return t if t.dtype == torch.int64 and t.is_contiguous() else t.long().contiguous()


def _xd(x_denoised):
    x = _f(x_denoised)
    if x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError(f"x_denoised must be [num_samples, num_atoms, 3], got {tuple(x.shape)}")
    return x


def _ws(B, A, T, device):
    n = ops.init().pd_loss_workspace_numel(B, A, T)
    ops.check(min(n, 0), "loss_workspace_numel")
    return torch.empty(n, dtype=torch.float32, device=device)


def smooth_lddt_loss(x_denoised, x_gt, x_exists, max_clamp_distance=16, _ws_buf=None, _out=None, **kwargs):
    """reference loss.py:162-181"""
    _dev("smooth_lddt_loss", x_denoised, x_gt, x_exists)
    xd, xg, ex = _xd(x_denoised), _f(x_gt), _f(x_exists)
    B, A = xd.shape[0], xd.shape[1]
    ws = _ws(B, A, 1, xd.device) if _ws_buf is None else _ws_buf
    out = torch.empty(1, dtype=torch.float32, device=xd.device) if _out is None else _out
    ops.check(ops.init().pd_loss_smooth_lddt(ops.ptr(xd), ops.ptr(xg), ops.ptr(ex), float(max_clamp_distance), ops.ptr(ws), ops.ptr(out),
                                             B, A, ops.stream()), "loss_smooth_lddt")
    return out[0]


def _centre_pairs(x_denoised, x_gt, t_hat, token_bonds, is_key_res, is_ligand, token_id_to_centre_atom_id, sd_bond, sd_key, eps,
                  _ws_buf=None, _out=None):
    xd, xg, th = _xd(x_denoised), _f(x_gt), _f(t_hat)
    B, A = xd.shape[0], xd.shape[1]
    c = _l(token_id_to_centre_atom_id)
    T = c.shape[0]
    tb = _f(token_bonds) if token_bonds is not None else torch.zeros(T, T, dtype=torch.float32, device=xd.device)
    kr = _f(is_key_res) if is_key_res is not None else torch.zeros(T, dtype=torch.float32, device=xd.device)
    lg = _f(is_ligand) if is_ligand is not None else torch.zeros(T, dtype=torch.float32, device=xd.device)
    ws = _ws(B, A, T, xd.device) if _ws_buf is None else _ws_buf
    out = torch.empty(2, dtype=torch.float32, device=xd.device) if _out is None else _out
    ops.check(ops.init().pd_loss_centre_pairs(ops.ptr(xd), ops.ptr(xg), ops.ptr(c), ops.ptr(tb), ops.ptr(kr), ops.ptr(lg), ops.ptr(th),
                                              float(sd_bond), float(sd_key), float(eps), ops.ptr(ws), ops.ptr(out), B, A, T,
                                              ops.stream()), "loss_centre_pairs")
    return out


def bond_loss(x_denoised, x_gt, token_bonds, t_hat, sigma_data, token_id_to_centre_atom_id, eps=1e-9, **kwargs):
    """reference loss.py:245-318"""
    _dev("bond_loss", x_denoised, x_gt, token_bonds, t_hat, token_id_to_centre_atom_id)
    return _centre_pairs(x_denoised, x_gt, t_hat, token_bonds, None, None, token_id_to_centre_atom_id, sigma_data, sigma_data, eps)[0]


def key_res_loss(x_denoised, x_gt, t_hat, is_ligand, is_key_res, sigma_data, token_id_to_centre_atom_id, eps=1e-9, **kwargs):
    """reference loss.py:535-559"""
    _dev("key_res_loss", x_denoised, x_gt, t_hat, is_ligand, is_key_res, token_id_to_centre_atom_id)
    return _centre_pairs(x_denoised, x_gt, t_hat, None, is_key_res, is_ligand, token_id_to_centre_atom_id, sigma_data, sigma_data, eps)[1]


def distogram_boundaries_sq(min_bin, max_bin, no_bins, device):
    """the reference's own expression for the squared bin edges (loss.py:92-98), evaluated by torch on the device"""
    return (torch.linspace(min_bin, max_bin, no_bins - 1, device=device) ** 2).contiguous()


def distogram_loss(p_distogram, x_gt, x_exists, token_id_to_pseudo_beta_atom_id, min_bin=3.25, max_bin=50.75, no_bins=39, eps=1e-9,
                   _ws_buf=None, _out=None, _bounds=None, **kwargs):
    """reference loss.py:78-115 (`eps` is accepted and unused, as there)"""
    _dev("distogram_loss", p_distogram, x_gt, x_exists, token_id_to_pseudo_beta_atom_id)
    pd, xg, ex, pb = _f(p_distogram), _f(x_gt), _f(x_exists), _l(token_id_to_pseudo_beta_atom_id)
    A, T = xg.shape[0], pb.shape[0]
    if tuple(pd.shape) != (T, T, no_bins):
        raise ValueError(f"p_distogram must be [{T}, {T}, {no_bins}], got {tuple(pd.shape)}")
    b2 = distogram_boundaries_sq(min_bin, max_bin, no_bins, pd.device) if _bounds is None else _bounds
    ws = _ws(1, A, T, pd.device) if _ws_buf is None else _ws_buf
    out = torch.empty(1, dtype=torch.float32, device=pd.device) if _out is None else _out
    ops.check(ops.init().pd_loss_distogram(ops.ptr(pd), ops.ptr(xg), ops.ptr(ex), ops.ptr(pb), ops.ptr(b2), int(no_bins), ops.ptr(ws),
                                           ops.ptr(out), A, T, ops.stream()), "loss_distogram")
    return out[0]


def mse_weights(is_dna, is_rna, is_ligand, alpha_dna, alpha_rna, alpha_ligand, atom_id_to_token_id, x_exists):
    """per-atom weights of the weighted MSE (loss.py:138-139)"""
    return ((1 + _f(is_dna) * alpha_dna + _f(is_rna) * alpha_rna + _f(is_ligand) * alpha_ligand)[_l(atom_id_to_token_id)]
            * _f(x_exists)).contiguous()


def weighted_mse_loss(x_denoised, x_gt, t_hat, sigma_data, is_dna, is_rna, is_ligand, alpha_dna, alpha_rna, alpha_ligand,
                      atom_id_to_token_id, x_exists, _ws_buf=None, _out=None, _aligned=None, _weights=None, **kwargs):
    """reference loss.py:118-159 (`sigma_data` is accepted and replaced by 16, as there)"""
    _dev("weighted_mse_loss", x_denoised, x_gt, t_hat, is_dna, is_rna, is_ligand, atom_id_to_token_id, x_exists)
    xd, xg, th, ex = _xd(x_denoised), _f(x_gt), _f(t_hat), _f(x_exists)
    B, A = xd.shape[0], xd.shape[1]
    w = mse_weights(is_dna, is_rna, is_ligand, alpha_dna, alpha_rna, alpha_ligand, atom_id_to_token_id, ex) if _weights is None else _weights
    al = torch.empty_like(xd) if _aligned is None else _aligned
    ws = _ws(B, A, 1, xd.device) if _ws_buf is None else _ws_buf
    out = torch.empty(1, dtype=torch.float32, device=xd.device) if _out is None else _out
    L = ops.init()
    # weighted_rigid_align(x_denoised * x_exists, x_gt, weights): x_gt moves onto the masked prediction
    ops.check(L.pd_kabsch_align(ops.ptr(xd), ops.ptr(ex), ops.ptr(xg), 0, ops.ptr(w), ops.ptr(al), B, A, ops.stream()), "kabsch")
    ops.check(L.pd_loss_weighted_mse(ops.ptr(xd), ops.ptr(al), ops.ptr(w), ops.ptr(th), ops.ptr(ws), ops.ptr(out), B, A, ops.stream()),
              "loss_weighted_mse")
    return out[0]


class PhysDockLoss(torch.nn.Module):
    """`cum_loss, losses = PhysDockLoss(config)(outputs, feats)` (reference loss.py:576-625): the weighted sum of the five
    terms and a dict of the terms and the sum under "loss", each a 0-d fp32 device tensor.  Weights and per-term settings come
    from `config.loss`.  A NaN / Inf term is replaced by zero with a logging.warning, as in the reference; that check is the
    only host read of the call.  `outputs` are what `PhysDock.forward` returns (real sizes), `feats` the un-padded batch."""

    def __init__(self, config):
        super().__init__()
        self.config = config.loss

    @torch.no_grad()
    def terms(self, outputs, feats):
        """the five raw terms as one [5] device tensor in the order of LOSS_TERMS (no host read; capturable)"""
        c = self.config
        f = dict(feats)
        if "x_exists" not in f:
            f["x_exists"] = f["a_mask"]
        xd = outputs["x_denoised"]
        _dev("PhysDockLoss", xd, outputs["t_hat"], outputs["p_distogram"], f["x_gt"])
        B, A, T = xd.shape[0], xd.shape[1], f["token_id_to_centre_atom_id"].shape[0]
        ws = _ws(B, A, T, xd.device)
        out = torch.empty(5, dtype=torch.float32, device=xd.device)
        both = {**outputs, **f}
        weighted_mse_loss(**both, **_settings(c.weighted_mse_loss), _ws_buf=ws, _out=out[0:1])
        smooth_lddt_loss(**both, **_settings(c.smooth_lddt_loss), _ws_buf=ws, _out=out[1:2])
        _centre_pairs(xd, f["x_gt"], outputs["t_hat"], f["token_bonds"], f["is_key_res"], f["is_ligand"], f["token_id_to_centre_atom_id"],
                      c.bond_loss.sigma_data, c.key_res_loss.sigma_data, 1e-9, _ws_buf=ws, _out=out[2:4])
        distogram_loss(**both, **_settings(c.distogram_loss), _ws_buf=ws, _out=out[4:5])
        return out

    @torch.no_grad()
    def forward(self, outputs, feats):
        t = self.terms(outputs, feats)
        bad = (~torch.isfinite(t)).tolist()                    # the one host read
        for name, b in zip(LOSS_TERMS, bad):
            if b:
                logging.warning(f"{name} loss is NaN. Skipping...")
        if any(bad):
            t = torch.where(torch.isfinite(t), t, torch.zeros_like(t))
        cum = torch.zeros((), dtype=torch.float32, device=t.device)
        losses = {}
        for k, name in enumerate(LOSS_TERMS):
            cum = cum + float(self.config[name].weight) * t[k]
            losses[name] = t[k].clone()
        losses["loss"] = cum.clone()
        return cum, losses


def _settings(block):
    return {k: v for k, v in block.items() if k != "weight"}
