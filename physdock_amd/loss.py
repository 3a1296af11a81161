"""PhysDockLoss: the five-term loss of the training-time forward, on the device (reference PhysDock/models/loss.py:78-181,
245-318, 535-559, 576-625), with its gradients to the network's outputs x_denoised and p_distogram.

    outputs = model(batch)                                   # x_denoised, x_hat, t_hat, p_distogram
    cum_loss, losses = PhysDockLoss(cfg)(outputs, batch)     # or: model(batch, return_loss=True)
    cum_loss.backward()                                      # where x_denoised / p_distogram require grad
    terms, g_x, g_p = PhysDockLoss(cfg).grads(outputs, batch)   # the same gradients, no host read (capturable)

Gradients (csrc/loss_grad.hip) are what torch autograd gives for the reference's code, and flow to x_denoised and p_distogram
only: another input that requires grad (x_gt, t_hat, a feature) raises NotImplementedError.  As in the reference, only
`cum_loss` carries the graph, the per-term values in `losses` are detached, and a non-finite term adds no gradient.  With no
input requiring grad every call returns what the forward-only code returned, bit for bit.

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

The second half of the file is ConfidenceLoss: cal_lddt, plddt_loss, pde_loss and pae_loss (reference loss.py:184-207, 320-532;
csrc/confidence_loss.hip) with their gradients to the logits of ConfidenceModule.
"""
from __future__ import annotations

import logging

import torch

from . import _lib as ops

__all__ = ["PhysDockLoss", "weighted_mse_loss", "smooth_lddt_loss", "bond_loss", "key_res_loss", "distogram_loss",
           "ConfidenceLoss", "cal_lddt", "plddt_loss", "pde_loss", "pae_loss"]

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


def _gws(B, A, T, device):
    n = ops.init().pd_loss_grad_workspace_numel(B, A, T)
    ops.check(min(n, 0), "loss_grad_workspace_numel")
    return torch.empty(n, dtype=torch.float32, device=device)


def _wants_grad(t):
    return torch.is_grad_enabled() and isinstance(t, torch.Tensor) and t.requires_grad


def _no_grad_to(what, _only="x_denoised and p_distogram", **tensors):
    """gradients flow to x_denoised and p_distogram only (the confidence losses: to the logits only); refuse the others loudly
    rather than return a silent None"""
    if not torch.is_grad_enabled():
        return
    for k, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise NotImplementedError(f"physdock_amd.{what}: no gradient to `{k}` (only {_only} are "
                                      f"differentiable here); pass it detached")


def _scale_ptr(g):
    return g.detach().float().contiguous().reshape(1)


class _Grad(torch.autograd.Function):
    """cum = value (computed without a graph); backward(g) = fn(g) -> one gradient per differentiable input"""

    @staticmethod
    def forward(ctx, value, fn, *inputs):
        ctx.fn = fn
        return value.clone()

    @staticmethod
    def backward(ctx, g):
        return (None, None, *ctx.fn(g))


def _attach(value, fn, *inputs):
    """`value` with a grad_fn when an input requires grad (else `value` unchanged)"""
    if not any(_wants_grad(t) for t in inputs):
        return value
    return _Grad.apply(value, fn, *inputs)


def _smooth_lddt_grad(xd, xg, ex, clamp, scale, g, ws, accumulate):
    B, A = xd.shape[0], xd.shape[1]
    ops.check(ops.init().pd_loss_smooth_lddt_grad(ops.ptr(xd), ops.ptr(xg), ops.ptr(ex), float(clamp), ops.ptr(scale), ops.ptr(ws),
                                                  ops.ptr(g), B, A, int(accumulate), ops.stream()), "loss_smooth_lddt_grad")


def _centre_pairs_grad(xd, xg, th, c, tb, kr, lg, sd_bond, sd_key, eps, scale2, g, ws, accumulate):
    B, A, T = xd.shape[0], xd.shape[1], c.shape[0]
    ops.check(ops.init().pd_loss_centre_pairs_grad(ops.ptr(xd), ops.ptr(xg), ops.ptr(c), ops.ptr(tb), ops.ptr(kr), ops.ptr(lg), ops.ptr(th),
                                                   float(sd_bond), float(sd_key), float(eps), ops.ptr(scale2), ops.ptr(ws), ops.ptr(g),
                                                   B, A, T, int(accumulate), ops.stream()), "loss_centre_pairs_grad")


def _distogram_grad(pd, xg, ex, pb, b2, no_bins, scale, g, ws):
    A, T = xg.shape[0], pb.shape[0]
    ops.check(ops.init().pd_loss_distogram_grad(ops.ptr(pd), ops.ptr(xg), ops.ptr(ex), ops.ptr(pb), ops.ptr(b2), int(no_bins),
                                                ops.ptr(scale), ops.ptr(ws), ops.ptr(g), A, T, ops.stream()), "loss_distogram_grad")


def _weighted_mse_grad(xd, al, w, th, scale, g, ws, accumulate):
    B, A = xd.shape[0], xd.shape[1]
    ops.check(ops.init().pd_loss_weighted_mse_grad(ops.ptr(xd), ops.ptr(al), ops.ptr(w), ops.ptr(th), ops.ptr(scale), ops.ptr(ws),
                                                   ops.ptr(g), B, A, int(accumulate), ops.stream()), "loss_weighted_mse_grad")


def _as_input(g, like):
    """a gradient computed for the fp32 contiguous copy, in the dtype of the tensor that was passed in"""
    return g if g.dtype == like.dtype else g.to(like.dtype)


def smooth_lddt_loss(x_denoised, x_gt, x_exists, max_clamp_distance=16, _ws_buf=None, _out=None, **kwargs):
    """reference loss.py:162-181"""
    _dev("smooth_lddt_loss", x_denoised, x_gt, x_exists)
    if _wants_grad(x_denoised):
        _no_grad_to("smooth_lddt_loss", x_gt=x_gt, x_exists=x_exists)
        with torch.no_grad():
            v = smooth_lddt_loss(x_denoised, x_gt, x_exists, max_clamp_distance)
        xd, xg, ex = _xd(x_denoised.detach()), _f(x_gt), _f(x_exists)

        def back(g):
            gx = torch.empty_like(xd)
            _smooth_lddt_grad(xd, xg, ex, max_clamp_distance, _scale_ptr(g), gx, _gws(xd.shape[0], xd.shape[1], 1, xd.device), 0)
            return (_as_input(gx, x_denoised),)
        return _attach(v, back, x_denoised)
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


def _centre_pairs_term(which, x_denoised, x_gt, t_hat, token_bonds, is_key_res, is_ligand, centre, sigma_data, eps):
    """bond_loss (which = 0) or key_res_loss (which = 1), differentiable in x_denoised"""
    _no_grad_to(("bond_loss", "key_res_loss")[which], x_gt=x_gt, t_hat=t_hat, token_bonds=token_bonds, is_key_res=is_key_res,
                is_ligand=is_ligand)
    with torch.no_grad():
        v = _centre_pairs(x_denoised, x_gt, t_hat, token_bonds, is_key_res, is_ligand, centre, sigma_data, sigma_data, eps)[which]
    xd, xg, th, c = _xd(x_denoised.detach()), _f(x_gt), _f(t_hat), _l(centre)
    T = c.shape[0]
    z = torch.zeros(T, dtype=torch.float32, device=xd.device)
    tb = _f(token_bonds) if token_bonds is not None else torch.zeros(T, T, dtype=torch.float32, device=xd.device)
    kr = _f(is_key_res) if is_key_res is not None else z
    lg = _f(is_ligand) if is_ligand is not None else z

    def back(g):
        s2 = torch.zeros(2, dtype=torch.float32, device=xd.device)
        s2[which] = g.detach().float()
        gx = torch.empty_like(xd)
        _centre_pairs_grad(xd, xg, th, c, tb, kr, lg, sigma_data, sigma_data, eps, s2, gx,
                           _gws(xd.shape[0], xd.shape[1], T, xd.device), 0)
        return (_as_input(gx, x_denoised),)
    return _attach(v, back, x_denoised)


def bond_loss(x_denoised, x_gt, token_bonds, t_hat, sigma_data, token_id_to_centre_atom_id, eps=1e-9, **kwargs):
    """reference loss.py:245-318"""
    _dev("bond_loss", x_denoised, x_gt, token_bonds, t_hat, token_id_to_centre_atom_id)
    if _wants_grad(x_denoised):
        return _centre_pairs_term(0, x_denoised, x_gt, t_hat, token_bonds, None, None, token_id_to_centre_atom_id, sigma_data, eps)
    return _centre_pairs(x_denoised, x_gt, t_hat, token_bonds, None, None, token_id_to_centre_atom_id, sigma_data, sigma_data, eps)[0]


def key_res_loss(x_denoised, x_gt, t_hat, is_ligand, is_key_res, sigma_data, token_id_to_centre_atom_id, eps=1e-9, **kwargs):
    """reference loss.py:535-559"""
    _dev("key_res_loss", x_denoised, x_gt, t_hat, is_ligand, is_key_res, token_id_to_centre_atom_id)
    if _wants_grad(x_denoised):
        return _centre_pairs_term(1, x_denoised, x_gt, t_hat, None, is_key_res, is_ligand, token_id_to_centre_atom_id, sigma_data, eps)
    return _centre_pairs(x_denoised, x_gt, t_hat, None, is_key_res, is_ligand, token_id_to_centre_atom_id, sigma_data, sigma_data, eps)[1]


def distogram_boundaries_sq(min_bin, max_bin, no_bins, device):
    """the reference's own expression for the squared bin edges (loss.py:92-98), evaluated by torch on the device"""
    return (torch.linspace(min_bin, max_bin, no_bins - 1, device=device) ** 2).contiguous()


def distogram_loss(p_distogram, x_gt, x_exists, token_id_to_pseudo_beta_atom_id, min_bin=3.25, max_bin=50.75, no_bins=39, eps=1e-9,
                   _ws_buf=None, _out=None, _bounds=None, **kwargs):
    """reference loss.py:78-115 (`eps` is accepted and unused, as there)"""
    _dev("distogram_loss", p_distogram, x_gt, x_exists, token_id_to_pseudo_beta_atom_id)
    if _wants_grad(p_distogram):
        _no_grad_to("distogram_loss", x_gt=x_gt, x_exists=x_exists)
        with torch.no_grad():
            v = distogram_loss(p_distogram, x_gt, x_exists, token_id_to_pseudo_beta_atom_id, min_bin, max_bin, no_bins, eps)
        pd, xg, ex, pb = _f(p_distogram.detach()), _f(x_gt), _f(x_exists), _l(token_id_to_pseudo_beta_atom_id)

        def back(g):
            gp = torch.empty_like(pd)
            _distogram_grad(pd, xg, ex, pb, distogram_boundaries_sq(min_bin, max_bin, no_bins, pd.device), no_bins, _scale_ptr(g), gp,
                            _gws(1, xg.shape[0], pb.shape[0], pd.device))
            return (_as_input(gp, p_distogram),)
        return _attach(v, back, p_distogram)
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
    if _wants_grad(x_denoised):
        _no_grad_to("weighted_mse_loss", x_gt=x_gt, t_hat=t_hat, is_dna=is_dna, is_rna=is_rna, is_ligand=is_ligand, x_exists=x_exists)
        xd = _xd(x_denoised.detach())
        B, A = xd.shape[0], xd.shape[1]
        with torch.no_grad():
            w = mse_weights(is_dna, is_rna, is_ligand, alpha_dna, alpha_rna, alpha_ligand, atom_id_to_token_id, _f(x_exists))
            al = torch.empty_like(xd)
            v = weighted_mse_loss(xd, x_gt, t_hat, sigma_data, is_dna, is_rna, is_ligand, alpha_dna, alpha_rna, alpha_ligand,
                                  atom_id_to_token_id, x_exists, _aligned=al, _weights=w)
        th = _f(t_hat)

        def back(g):
            gx = torch.empty_like(xd)
            _weighted_mse_grad(xd, al, w, th, _scale_ptr(g), gx, _gws(B, A, 1, xd.device), 0)
            return (_as_input(gx, x_denoised),)
        return _attach(v, back, x_denoised)
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
    only host read of the call.  `outputs` are what `PhysDock.forward` returns (real sizes), `feats` the un-padded batch.
    Where outputs["x_denoised"] and / or outputs["p_distogram"] require grad, `cum_loss` has a grad_fn and `cum_loss.backward()`
    fills their .grad (the launches of `grads`); the values are the same bits either way."""

    def __init__(self, config):
        super().__init__()
        self.config = config.loss
        self._wdev = {}

    def _feats(self, outputs, feats):
        f = dict(feats)
        if "x_exists" not in f:
            f["x_exists"] = f["a_mask"]
        _dev("PhysDockLoss", outputs["x_denoised"], outputs["t_hat"], outputs["p_distogram"], f["x_gt"])
        return f

    @torch.no_grad()
    def terms(self, outputs, feats, _keep=None):
        """the five raw terms as one [5] device tensor in the order of LOSS_TERMS (no host read; capturable)"""
        c = self.config
        f = self._feats(outputs, feats)
        xd = outputs["x_denoised"].detach()
        B, A, T = xd.shape[0], xd.shape[1], f["token_id_to_centre_atom_id"].shape[0]
        ws = _ws(B, A, T, xd.device)
        out = torch.empty(5, dtype=torch.float32, device=xd.device)
        both = {**outputs, **f, "x_denoised": xd, "p_distogram": outputs["p_distogram"].detach()}
        keep = {}
        if _keep is not None:     # the alignment and weights of the weighted MSE, for the backward (same values as without)
            cm = c.weighted_mse_loss
            keep["w"] = mse_weights(f["is_dna"], f["is_rna"], f["is_ligand"], cm.alpha_dna, cm.alpha_rna, cm.alpha_ligand,
                                    f["atom_id_to_token_id"], _f(f["x_exists"]))
            keep["al"] = torch.empty_like(_xd(xd))
            _keep.update(keep)
        weighted_mse_loss(**both, **_settings(c.weighted_mse_loss), _ws_buf=ws, _out=out[0:1], _aligned=keep.get("al"),
                          _weights=keep.get("w"))
        smooth_lddt_loss(**both, **_settings(c.smooth_lddt_loss), _ws_buf=ws, _out=out[1:2])
        _centre_pairs(xd, f["x_gt"], outputs["t_hat"], f["token_bonds"], f["is_key_res"], f["is_ligand"], f["token_id_to_centre_atom_id"],
                      c.bond_loss.sigma_data, c.key_res_loss.sigma_data, 1e-9, _ws_buf=ws, _out=out[2:4])
        distogram_loss(**both, **_settings(c.distogram_loss), _ws_buf=ws, _out=out[4:5])
        return out

    def _weights(self, device):
        """the five term weights as a [5] fp32 device tensor (made once per device, outside any capture)"""
        key = str(device)
        if key not in self._wdev:
            self._wdev[key] = torch.tensor([float(self.config[n].weight) for n in LOSS_TERMS], dtype=torch.float32, device=device)
        return self._wdev[key]

    @torch.no_grad()
    def _backward(self, outputs, feats, t, keep, up, need_x=True, need_p=True):
        """g_x [B,A,3] and g_p [T,T,bins] of sum_t weight_t term_t x up, from the raw terms t [5] on the device: the scale of a
        term is weight x up x isfinite(term), read by the launchers from device memory (no host read).  Launch order: weighted
        MSE writes g_x, smooth lDDT and the centre pairs add to it; the distogram writes g_p."""
        c = self.config
        f = self._feats(outputs, feats)
        xd, pd = _xd(outputs["x_denoised"].detach()), _f(outputs["p_distogram"].detach())
        B, A = xd.shape[0], xd.shape[1]
        ci = _l(f["token_id_to_centre_atom_id"])
        T = ci.shape[0]
        w = self._weights(t.device)
        sc = torch.where(torch.isfinite(t), w * up if up is not None else w, torch.zeros_like(t)).contiguous()
        ws = _gws(B, A, T, xd.device)
        xg, ex = _f(f["x_gt"]), _f(f["x_exists"])
        g_x = g_p = None
        if need_x:
            g_x = torch.empty_like(xd)
            _weighted_mse_grad(xd, keep["al"], keep["w"], _f(outputs["t_hat"]), sc[0:1], g_x, ws, 0)
            _smooth_lddt_grad(xd, xg, ex, c.smooth_lddt_loss.max_clamp_distance, sc[1:2], g_x, ws, 1)
            _centre_pairs_grad(xd, xg, _f(outputs["t_hat"]), ci, _f(f["token_bonds"]), _f(f["is_key_res"]), _f(f["is_ligand"]),
                               c.bond_loss.sigma_data, c.key_res_loss.sigma_data, 1e-9, sc[2:4], g_x, ws, 1)
        if need_p:
            cd = c.distogram_loss
            g_p = torch.empty_like(pd)
            _distogram_grad(pd, xg, ex, _l(f["token_id_to_pseudo_beta_atom_id"]),
                            distogram_boundaries_sq(cd.min_bin, cd.max_bin, cd.no_bins, pd.device), cd.no_bins, sc[4:5], g_p, ws)
        return g_x, g_p

    @torch.no_grad()
    def grads(self, outputs, feats, grad_scale=None):
        """(terms [5], g_x [B,A,3], g_p [T,T,bins]): the raw terms and the gradients of the weighted total to x_denoised and
        p_distogram, scaled by `grad_scale` (a 0-d device tensor, or None for 1).  A non-finite term adds no gradient.  No host
        read: capturable in a hipGraph.  The same bits as `cum_loss.backward()`."""
        keep = {}
        t = self.terms(outputs, feats, _keep=keep)
        up = None if grad_scale is None else grad_scale.detach().float().reshape(())
        g_x, g_p = self._backward(outputs, feats, t, keep, up)
        return t, g_x, g_p

    def forward(self, outputs, feats):
        xd, pd = outputs["x_denoised"], outputs["p_distogram"]
        need_x, need_p = _wants_grad(xd), _wants_grad(pd)
        if need_x or need_p:
            f = self._feats(outputs, feats)
            _no_grad_to("PhysDockLoss", t_hat=outputs["t_hat"],
                        **{k: f[k] for k in ("x_gt", "x_exists", "token_bonds", "is_dna", "is_rna", "is_ligand", "is_key_res") if k in f})
        keep = {} if need_x or need_p else None
        with torch.no_grad():
            t = self.terms(outputs, feats, _keep=keep)
            bad = (~torch.isfinite(t)).tolist()                    # the one host read
            for name, b in zip(LOSS_TERMS, bad):
                if b:
                    logging.warning(f"{name} loss is NaN. Skipping...")
            tz = torch.where(torch.isfinite(t), t, torch.zeros_like(t)) if any(bad) else t
            cum = torch.zeros((), dtype=torch.float32, device=t.device)
            losses = {}
            for k, name in enumerate(LOSS_TERMS):
                cum = cum + float(self.config[name].weight) * tz[k]
                losses[name] = tz[k].clone()
            losses["loss"] = cum.clone()
        if need_x or need_p:
            def back(g):
                g_x, g_p = self._backward(outputs, feats, t, keep, g.detach().float().reshape(()), need_x, need_p)
                return (_as_input(g_x, xd) if need_x else None, _as_input(g_p, pd) if need_p else None)
            cum = _Grad.apply(cum, back, xd, pd)
        return cum, losses


def _settings(block):
    return {k: v for k, v in block.items() if k != "weight"}


# ---------------------------------------------------------------------------------------------------------------------------
# The confidence losses (reference loss.py:184-207, 320-532; csrc/confidence_loss.hip)
#
#     p_pae, p_pde, p_plddt = confidence_module(batch, s, z, x_pred)
#     cum_loss, losses = ConfidenceLoss(cfg)({"p_plddt": p_plddt, "p_pde": p_pde, "p_pae": p_pae, "x_pred": x_pred}, batch)
#     cum_loss.backward()                                    # where the logits require grad
#     terms, g_plddt, g_pde, g_pae = ConfidenceLoss(cfg).grads(outputs, batch)     # the same gradients, no host read
#
# Every target is a hard bin of a distance, formed on the fly; gradients flow to the logits only.  Only pose 0 of x_pred enters
# the three losses, as in the reference.
CONF_TERMS = ("plddt_loss", "pde_loss", "pae_loss")
CONF_LOGITS = ("p_plddt", "p_pde", "p_pae")
FRAME_KEYS = ("token_id_to_frame_atom_id_0", "token_id_to_frame_atom_id_1", "token_id_to_frame_atom_id_2")
_LOGITS_ONLY = "the logits"


def _cws(A, T, device):
    n = ops.init().pd_conf_loss_workspace_numel(1, A, T)
    ops.check(min(n, 0), "conf_loss_workspace_numel")
    return torch.empty(n, dtype=torch.float32, device=device)


def _poses(x_pred):
    x = _f(x_pred)
    if x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError(f"x_pred must be [num_poses, num_atoms, 3], got {tuple(x.shape)}")
    return x


def _lddt(xp, xg, dna, rna, poly, c):
    """[B,A] per-atom lDDT of the fp32 contiguous poses xp [B,A,3]"""
    B, A, T = xp.shape[0], xp.shape[1], c.shape[0]
    if tuple(xg.shape) != (A, 3):
        raise ValueError(f"x_gt must be [{A}, 3], got {tuple(xg.shape)}")
    out = torch.empty(B, A, dtype=torch.float32, device=xp.device)
    ops.check(ops.init().pd_lddt_atoms(ops.ptr(xp), ops.ptr(xg), ops.ptr(c), ops.ptr(dna), ops.ptr(rna), ops.ptr(poly), ops.ptr(out),
                                       B, A, T, ops.stream()), "lddt_atoms")
    return out


def _polymer(is_ligand):
    """the reference writes `~is_ligand`, which raises on the float32 is_ligand its own loader produces; `is_ligand == 0` is the
    same for the bool input it accepts and works for every dtype"""
    return (is_ligand == 0).float().contiguous()


@torch.no_grad()
def cal_lddt(x_pred, x_gt, is_dna, is_rna, is_polymer, token_id_to_centre_atom_id, **kwargs):
    """reference loss.py:320-372: per-atom lDDT [B,A] of the poses x_pred [B,A,3] ([A] for one pose [A,3]) against x_gt over the
    token-centre atoms: four hard thresholds 0.5 / 1 / 2 / 4 on |d_pred - d_gt|, inclusion d_gt < 30 (nucleotide tokens) or 15,
    times is_polymer.  No epsilon: an atom with an empty inclusion set is NaN, as there.  Piecewise constant: no gradient."""
    _dev("cal_lddt", x_pred, x_gt, is_dna, is_rna, is_polymer, token_id_to_centre_atom_id)
    one = x_pred.dim() == 2
    out = _lddt(_poses(x_pred[None] if one else x_pred), _f(x_gt), _f(is_dna), _f(is_rna), _f(is_polymer), _l(token_id_to_centre_atom_id))
    return out[0] if one else out


def _frames(x, ids):
    """[T,13] frames (e1 | e2 | e3 | origin | valid) of the coordinates x [A,3]: express_coordinates_in_frame, loss.py:184-207"""
    T = ids[0].shape[0]
    out = torch.empty(T, 13, dtype=torch.float32, device=x.device)
    ops.check(ops.init().pd_conf_frames(ops.ptr(x), ops.ptr(ids[0]), ops.ptr(ids[1]), ops.ptr(ids[2]), ops.ptr(out), x.shape[0], T,
                                        ops.stream()), "conf_frames")
    return out


def _plddt_launch(p, no_bins, lddt0, ex, ws=None, out=None, grad=None, scale=None):
    A = ex.shape[0]
    if tuple(p.shape) != (A, no_bins):
        raise ValueError(f"p_plddt must be [{A}, {no_bins}], got {tuple(p.shape)}")
    ws = _cws(A, 1, p.device) if ws is None else ws
    out = torch.empty(1, dtype=torch.float32, device=p.device) if out is None else out
    ops.check(ops.init().pd_conf_loss_plddt(ops.ptr(p), ops.ptr(lddt0), ops.ptr(ex), int(no_bins), ops.ptr(scale), ops.ptr(ws),
                                            ops.ptr(out), ops.ptr(grad), A, ops.stream()), "conf_loss_plddt")
    return out[0]


def _pairs_launch(mode, p, x0, xg, ex, c, fr, min_bin, max_bin, no_bins, ws=None, out=None, grad=None, scale=None):
    A, T = xg.shape[0], c.shape[0]
    if tuple(p.shape) != (T, T, no_bins):
        raise ValueError(f"{('p_pde', 'p_pae')[mode]} must be [{T}, {T}, {no_bins}], got {tuple(p.shape)}")
    ws = _cws(A, T, p.device) if ws is None else ws
    out = torch.empty(1, dtype=torch.float32, device=p.device) if out is None else out
    fp, fg = fr if fr is not None else (None, None)
    ops.check(ops.init().pd_conf_loss_pairs(mode, ops.ptr(p), ops.ptr(x0), ops.ptr(xg), ops.ptr(ex), ops.ptr(c), ops.ptr(fp), ops.ptr(fg),
                                            float(min_bin), float(max_bin - min_bin), int(no_bins), ops.ptr(scale), ops.ptr(ws),
                                            ops.ptr(out), ops.ptr(grad), A, T, ops.stream()), "conf_loss_pairs")
    return out[0]


def _logit_term(what, logits, launch, **others):
    """value of one confidence term, with a grad_fn where the logits require grad; launch(p, grad, scale) -> 0-d value"""
    _no_grad_to(what, _only=_LOGITS_ONLY, **others)
    with torch.no_grad():
        p = _f(logits.detach())
        v = launch(p, None, None)
    if not _wants_grad(logits):
        return v

    def back(g):
        gp = torch.empty_like(p)
        launch(p, gp, _scale_ptr(g))
        return (_as_input(gp, logits),)
    return _attach(v, back, logits)


def plddt_loss(p_plddt, no_bins, x_pred, x_gt, x_exists, is_dna, is_rna, is_ligand, token_id_to_centre_atom_id, **kwargs):
    """reference loss.py:375-421.  is_polymer = (is_ligand == 0) for every dtype: the reference's `~is_ligand` is the same for the
    bool input it accepts and raises on the float32 is_ligand of its own loader.  A NaN lDDT (an atom with no polymer centre in
    range) goes to bin 0."""
    _dev("plddt_loss", p_plddt, x_pred, x_gt, x_exists, is_dna, is_rna, is_ligand, token_id_to_centre_atom_id)
    with torch.no_grad():
        lddt0 = _lddt(_poses(x_pred)[0:1], _f(x_gt), _f(is_dna), _f(is_rna), _polymer(is_ligand), _l(token_id_to_centre_atom_id))[0]
        ex = _f(x_exists)
    return _logit_term("plddt_loss", p_plddt, lambda p, g, s: _plddt_launch(p, no_bins, lddt0, ex, grad=g, scale=s),
                       x_pred=x_pred, x_gt=x_gt, x_exists=x_exists, is_dna=is_dna, is_rna=is_rna, is_ligand=is_ligand)


def pde_loss(p_pde, x_pred, x_gt, x_exists, token_id_to_centre_atom_id, min_bin=0.0, max_bin=32.0, no_bins=64, **kwargs):
    """reference loss.py:472-532"""
    _dev("pde_loss", p_pde, x_pred, x_gt, x_exists, token_id_to_centre_atom_id)
    with torch.no_grad():
        x0, xg, ex, c = _poses(x_pred)[0], _f(x_gt), _f(x_exists), _l(token_id_to_centre_atom_id)
    return _logit_term("pde_loss", p_pde,
                       lambda p, g, s: _pairs_launch(0, p, x0, xg, ex, c, None, min_bin, max_bin, no_bins, grad=g, scale=s),
                       x_pred=x_pred, x_gt=x_gt, x_exists=x_exists)


def pae_loss(p_pae, x_pred, x_gt, x_exists, token_id_to_centre_atom_id, token_id_to_frame_atom_id_0, token_id_to_frame_atom_id_1,
             token_id_to_frame_atom_id_2, min_bin=0, max_bin=32, no_bins=64, **kwargs):
    """reference loss.py:424-469: the error of token j's centre expressed in token i's frame (express_coordinates_in_frame,
    loss.py:184-207), zero where the frame of i is invalid (its three atoms within 25 degrees of a line) in x_gt or in pose 0"""
    ids = (token_id_to_frame_atom_id_0, token_id_to_frame_atom_id_1, token_id_to_frame_atom_id_2)
    _dev("pae_loss", p_pae, x_pred, x_gt, x_exists, token_id_to_centre_atom_id, *ids)
    with torch.no_grad():
        x0, xg, ex, c = _poses(x_pred)[0], _f(x_gt), _f(x_exists), _l(token_id_to_centre_atom_id)
        ids = tuple(_l(i) for i in ids)
        fr = (_frames(x0, ids), _frames(xg, ids))
    return _logit_term("pae_loss", p_pae,
                       lambda p, g, s: _pairs_launch(1, p, x0, xg, ex, c, fr, min_bin, max_bin, no_bins, grad=g, scale=s),
                       x_pred=x_pred, x_gt=x_gt, x_exists=x_exists)


class ConfidenceLoss(torch.nn.Module):
    """`cum_loss, losses = ConfidenceLoss(config)(outputs, feats)`: the weighted sum of plddt_loss, pde_loss and pae_loss and a dict
    of the three terms and the sum under "loss", each a detached 0-d fp32 device tensor.  `outputs` holds the logits of
    ConfidenceModule, p_plddt [A,bins], p_pde and p_pae [T,T,bins], and the poses x_pred [B,A,3] (pose 0 is read); `feats` uses the
    reference's key names: x_gt, x_exists (falls back to a_mask), is_dna, is_rna, is_ligand, token_id_to_centre_atom_id and the
    three token_id_to_frame_atom_id_{0,1,2}.  Weights and settings come from config.loss.{plddt_loss, pde_loss, pae_loss}.
    is_polymer = (is_ligand == 0) for every dtype (see plddt_loss).  A NaN / Inf term is replaced by zero with a logging.warning as
    in PhysDockLoss; that check is the only host read.  Where a logit tensor requires grad `cum_loss` has a grad_fn.

    The reference's feature loader never makes the frame-atom ids and the default PAE weight is 0: without the three keys and with
    a zero weight the PAE term is not launched (losses["pae_loss"] = 0, g_pae = None); with a non-zero weight it is a KeyError."""

    def __init__(self, config):
        super().__init__()
        self.config = config.loss
        self._wdev = {}

    def _prepare(self, outputs, feats):
        """everything the launches read, fp32 / int64 contiguous, with the lDDT of pose 0 and the frames (no host read)"""
        c = self.config
        f = dict(feats)
        if "x_exists" not in f:
            f["x_exists"] = f["a_mask"]
        has_frames = all(k in f for k in FRAME_KEYS)
        if not has_frames and float(c.pae_loss.weight) != 0.0:
            raise KeyError(f"pae_loss has weight {c.pae_loss.weight} but feats lacks {[k for k in FRAME_KEYS if k not in f]}")
        _dev("ConfidenceLoss", outputs["p_plddt"], outputs["p_pde"], outputs["x_pred"], f["x_gt"], f["x_exists"],
             *([outputs["p_pae"]] if has_frames else []))
        _no_grad_to("ConfidenceLoss", _only=_LOGITS_ONLY, x_pred=outputs["x_pred"],
                    **{k: f[k] for k in ("x_gt", "x_exists", "is_dna", "is_rna", "is_ligand")})
        with torch.no_grad():
            k = {"x0": _poses(outputs["x_pred"])[0], "xg": _f(f["x_gt"]), "ex": _f(f["x_exists"]),
                 "c": _l(f["token_id_to_centre_atom_id"]), "fr": None}
            k["p"] = [_f(outputs[n].detach()) if (n != "p_pae" or has_frames) else None for n in CONF_LOGITS]
            k["lddt0"] = _lddt(k["x0"][None], k["xg"], _f(f["is_dna"]), _f(f["is_rna"]), _polymer(f["is_ligand"]), k["c"])[0]
            if has_frames:
                ids = tuple(_l(f[n]) for n in FRAME_KEYS)
                k["fr"] = (_frames(k["x0"], ids), _frames(k["xg"], ids))
            k["ws"] = _cws(k["xg"].shape[0], k["c"].shape[0], k["xg"].device)
        return k

    def _launch(self, k, out, grads=(None, None, None), sc=None):
        """the three terms into out [3] (PAE untouched without frames); grads[t], where given, is overwritten with sc[t] x d term_t"""
        c = self.config
        s = [None if sc is None else sc[t:t + 1] for t in range(3)]
        _plddt_launch(k["p"][0], c.plddt_loss.no_bins, k["lddt0"], k["ex"], ws=k["ws"], out=out[0:1], grad=grads[0], scale=s[0])
        for t, name in ((1, "pde_loss"), (2, "pae_loss")):
            if t == 2 and k["fr"] is None:
                continue
            st = {"min_bin": 0, "max_bin": 32, "no_bins": 64, **_settings(c[name])}
            _pairs_launch(t - 1, k["p"][t], k["x0"], k["xg"], k["ex"], k["c"], k["fr"] if t == 2 else None, st["min_bin"], st["max_bin"],
                          st["no_bins"], ws=k["ws"], out=out[t:t + 1], grad=grads[t], scale=s[t])
        return out

    @torch.no_grad()
    def terms(self, outputs, feats, _k=None):
        """the three raw terms as one [3] device tensor in the order of CONF_TERMS (no host read; capturable)"""
        k = self._prepare(outputs, feats) if _k is None else _k
        return self._launch(k, torch.zeros(3, dtype=torch.float32, device=k["xg"].device))

    def _weights(self, device):
        key = str(device)
        if key not in self._wdev:
            self._wdev[key] = torch.tensor([float(self.config[n].weight) for n in CONF_TERMS], dtype=torch.float32, device=device)
        return self._wdev[key]

    @torch.no_grad()
    def _backward(self, k, t, up, need=(True, True, True)):
        """the gradients of sum_t weight_t term_t x up to the logits, from the raw terms t [3]: the scale of a term is weight x up x
        isfinite(term), read by the launchers from device memory (no host read)"""
        w = self._weights(t.device)
        sc = torch.where(torch.isfinite(t), w * up if up is not None else w, torch.zeros_like(t)).contiguous()
        grads = [torch.empty_like(k["p"][i]) if (need[i] and k["p"][i] is not None) else None for i in range(3)]
        if any(g is not None for g in grads):
            self._launch(k, torch.empty(3, dtype=torch.float32, device=t.device), grads, sc)
        return grads

    @torch.no_grad()
    def grads(self, outputs, feats, grad_scale=None):
        """(terms [3], g_plddt, g_pde, g_pae): the raw terms and the gradients of the weighted total to the three logit tensors,
        scaled by `grad_scale` (a 0-d device tensor, or None for 1).  A non-finite term adds no gradient; g_pae is None where the
        PAE term is not launched.  No host read: capturable in a hipGraph.  The same bits as `cum_loss.backward()`."""
        k = self._prepare(outputs, feats)
        t = self.terms(outputs, feats, _k=k)
        up = None if grad_scale is None else grad_scale.detach().float().reshape(())
        return (t, *self._backward(k, t, up))

    def forward(self, outputs, feats):
        k = self._prepare(outputs, feats)
        logits = [outputs[n] if k["p"][i] is not None else None for i, n in enumerate(CONF_LOGITS)]
        need = [_wants_grad(p) for p in logits]
        with torch.no_grad():
            t = self.terms(outputs, feats, _k=k)
            bad = (~torch.isfinite(t)).tolist()                    # the one host read
            for name, b in zip(CONF_TERMS, bad):
                if b:
                    logging.warning(f"{name} loss is NaN. Skipping...")
            tz = torch.where(torch.isfinite(t), t, torch.zeros_like(t)) if any(bad) else t
            cum = torch.zeros((), dtype=torch.float32, device=t.device)
            losses = {}
            for i, name in enumerate(CONF_TERMS):
                cum = cum + float(self.config[name].weight) * tz[i]
                losses[name] = tz[i].clone()
            losses["loss"] = cum.clone()
        if any(need):
            live = [p for p, n in zip(logits, need) if n]

            def back(g):
                gs = self._backward(k, t, g.detach().float().reshape(()), need)
                return tuple(_as_input(gs[i], logits[i]) for i in range(3) if need[i])
            cum = _Grad.apply(cum, back, *live)
        return cum, losses
