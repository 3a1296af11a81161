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


def _gws(B, A, T, device):
    n = ops.init().pd_loss_grad_workspace_numel(B, A, T)
    ops.check(min(n, 0), "loss_grad_workspace_numel")
    return torch.empty(n, dtype=torch.float32, device=device)


def _wants_grad(t):
    return torch.is_grad_enabled() and isinstance(t, torch.Tensor) and t.requires_grad


def _no_grad_to(what, **tensors):
    """gradients flow to x_denoised and p_distogram only; refuse the others loudly rather than return a silent None"""
    if not torch.is_grad_enabled():
        return
    for k, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise NotImplementedError(f"physdock_amd.{what}: no gradient to `{k}` (only x_denoised and p_distogram are "
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
