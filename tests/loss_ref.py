"""Float64 definition of the five loss terms of csrc/loss.hip and of their gradients (csrc/loss_grad.hip), in the call shape of the
ten launchers, so that a kernel-level case needs no fixture and no reference tree.

Forward: the terms as tests/test_loss_cpu.py::restate_f64 states them (tests/test_loss_ref_cpu.py holds the two together at 1e-10).
The weighted MSE takes x_gt_aligned and the weights as inputs, as pd_loss_weighted_mse does: the alignment is not restated here.

Gradients: the closed forms named in loss_grad.hip's comments, with torch autograd's conventions: sign(0) = 0, a zero distance
has a zero direction, the clamp of the weighted MSE passes the gradient where the pre-clamp value is <= 1e4 and nowhere else
(a NaN value passes none).  `torch_smooth_lddt` .. `torch_weighted_mse` are the same forward in torch float64; tests/test_loss_ref_cpu.py pins the closed forms
to its autograd at one small case, and to the stored g64 rows of the g16 fixtures.

Tie bookkeeping as tools/make_golden_loss_grad.py does it: where |d_pred - d_gt| < tau two fp32 implementations may give sign()
either way, so the gradient of smooth lDDT and of the key-residue term carries a per-atom allowance, the sum of |contribution|
over such pairs; tau = 8 fp32 ulp of the largest |coordinate| (6.1e-5 at 64 A).  `clamp_margin` / `bin_margin` give the closest
relative approach of a ground-truth pair to the clamp radius / of a pseudo-beta pair to a bin edge: below those an fp32 distance
may fall on the other side than the float64 one.
"""
import numpy as np

CS = (0.5, 1.0, 2.0, 4.0)
SD_MSE = 16.0                  # weighted_mse_loss overwrites sigma_data with 16
CLAMP_MSE = 1e4


def f64(a):
    return np.asarray(a, dtype=np.float64)


def sig4(d):
    return [1.0 / (1.0 + np.exp(c - d)) for c in CS]


def eps4(d):
    return 0.25 * sum(sig4(d))


def deps4(d):
    return 0.25 * sum(s * (1.0 - s) for s in sig4(d))


def pairdist2(x, y=None):
    """[n,m] squared distances, coordinate by coordinate (no [n,m,3] temporary)"""
    y = x if y is None else y
    d2 = np.zeros((x.shape[0], y.shape[0]))
    for c in range(3):
        d = x[:, None, c] - y[None, :, c]
        d2 += d * d
    return d2


def pairdist(x, y=None):
    return np.sqrt(pairdist2(x, y))


def edm_scale(t_hat, sd):
    t = f64(t_hat)
    return float(np.mean((t ** 2 + sd ** 2) / (t * sd) ** 2))


def tau_of(*coords):
    """8 fp32 ulp of the largest finite |coordinate| (tools/make_golden_loss_grad.py)"""
    m = max(float(np.abs(c[np.isfinite(c)]).max()) for c in coords)
    return 8.0 * float(np.spacing(np.float32(m)))


# ------------------------------------------------------------------ forward
def lddt_mask(x_gt, x_exists, clamp):
    ex = f64(x_exists)
    dgt = pairdist(f64(x_gt))
    return dgt, (dgt < clamp) * np.outer(ex, ex)


def smooth_lddt(x_denoised, x_gt, x_exists, clamp):
    xd = f64(x_denoised)
    dgt, m = lddt_mask(x_gt, x_exists, clamp)
    n = 1e-9 + m.sum()
    return float(np.mean([np.sum(m * eps4(np.abs(pairdist(xd[b]) - dgt))) / n for b in range(xd.shape[0])]))


def centre_pairs(x_denoised, x_gt, centre, token_bonds, is_key_res, is_ligand, t_hat, sd_bond, sd_key, eps):
    """(bond_loss, key_res_loss)"""
    xd, xg = f64(x_denoised), f64(x_gt)
    ci = np.asarray(centre, dtype=np.int64)
    dg = pairdist(xg[ci])
    tb, km = f64(token_bonds), np.outer(f64(is_key_res), f64(is_ligand))
    sb = sk = 0.0
    for b in range(xd.shape[0]):
        diff = pairdist(xd[b][ci]) - dg
        sb += np.sum(tb * diff ** 2)
        sk += np.sum(km * eps4(np.abs(diff)) ** 2)
    B = xd.shape[0]
    return (float(edm_scale(t_hat, sd_bond) * (sb / B) / (tb.sum() + eps)),
            float(edm_scale(t_hat, sd_key) * (sk / B) / (km.sum() + eps)))


def distogram_parts(p_distogram, x_gt, x_exists, pseudo_beta, boundaries_sq, no_bins):
    """(mask [T,T], softmax of the masked logits [T,T,bins], log-softmax, one-hot of the true bin)"""
    xg, ex = f64(x_gt), f64(x_exists)
    pb = np.asarray(pseudo_beta, dtype=np.int64)
    b2 = f64(boundaries_sq)
    assert b2.shape == (no_bins - 1,)
    bins = np.sum(pairdist2(xg[pb])[..., None] > b2, -1)
    md = np.outer(ex[pb], ex[pb])
    lg = f64(p_distogram) * md[..., None]
    lg = lg - lg.max(-1, keepdims=True)
    lse = np.log(np.exp(lg).sum(-1, keepdims=True))
    onehot = np.arange(no_bins) == bins[..., None]
    return md, np.exp(lg - lse), lg - lse, onehot


def distogram(p_distogram, x_gt, x_exists, pseudo_beta, boundaries_sq, no_bins):
    md, _, logp, onehot = distogram_parts(p_distogram, x_gt, x_exists, pseudo_beta, boundaries_sq, no_bins)
    err = -np.sum(onehot * md[..., None] * logp, -1)
    return float(np.sum(md * err) / (1e-9 + md.sum()))


def weighted_mse_pre_clamp(x_denoised, x_gt_aligned, weights, t_hat):
    r, w = f64(x_denoised) - f64(x_gt_aligned), f64(weights)
    B = r.shape[0]
    mm = np.sum(w[None] * (r ** 2).sum(-1)) / (1e-9 + B * w.sum())
    return float(edm_scale(t_hat, SD_MSE) * mm / 3.0)


def weighted_mse(x_denoised, x_gt_aligned, weights, t_hat):
    v = weighted_mse_pre_clamp(x_denoised, x_gt_aligned, weights, t_hat)
    return v if np.isnan(v) else min(v, CLAMP_MSE)


# ------------------------------------------------------------------ gradients (closed forms)
def _pair_grad(C, x):
    """sum_j C_ij (x_i - x_j), by numpy's own summation: a BLAS product would make the last bits depend on the BLAS build"""
    return C.sum(1)[:, None] * x - np.stack([(C * x[None, :, c]).sum(1) for c in range(3)], 1)


def smooth_lddt_grad(x_denoised, x_gt, x_exists, clamp, tau=None, rows=None):
    """(g [B,A,3], allowance [B,A]): d smooth_lddt / d x_denoised and the tie allowance per atom; with `rows`, of those samples only"""
    xd = f64(x_denoised)
    B = xd.shape[0]
    tau = tau_of(xd, f64(x_gt)) if tau is None else tau
    dgt, m = lddt_mask(x_gt, x_exists, clamp)
    k = 1.0 / B / (1e-9 + m.sum())
    ms = m + m.T
    xd = xd if rows is None else xd[np.asarray(rows)]
    g, a = np.zeros_like(xd), np.zeros(xd.shape[:2])
    for b in range(xd.shape[0]):
        D = pairdist(xd[b])
        dl = D - dgt
        e = ms * deps4(np.abs(dl))
        with np.errstate(divide="ignore", invalid="ignore"):
            C = np.where(D > 0, e * np.sign(dl) / D, 0.0)
        g[b] = k * _pair_grad(C, xd[b])
        a[b] = k * np.where((np.abs(dl) < tau) & (D > 0), e, 0.0).sum(1)
    return g, a


def centre_pairs_grad(x_denoised, x_gt, centre, token_bonds, is_key_res, is_ligand, t_hat, sd_bond, sd_key, eps, tau=None, rows=None):
    """(g_bond, g_key [B,A,3], allowance of the key term [B,A]); with `rows`, of those samples only"""
    xd, xg = f64(x_denoised), f64(x_gt)
    B, A = xd.shape[:2]
    tau = tau_of(xd, xg) if tau is None else tau
    ci = np.asarray(centre, dtype=np.int64)
    dg = pairdist(xg[ci])
    tb, km = f64(token_bonds), np.outer(f64(is_key_res), f64(is_ligand))
    kb = edm_scale(t_hat, sd_bond) / B / (tb.sum() + eps)
    kk = edm_scale(t_hat, sd_key) / B / (km.sum() + eps)
    tbs, kms = tb + tb.T, km + km.T
    xd = xd if rows is None else xd[np.asarray(rows)]
    gb, gk, a = np.zeros_like(xd), np.zeros_like(xd), np.zeros(xd.shape[:2])
    for b in range(xd.shape[0]):
        xc = xd[b][ci]
        D = pairdist(xc)
        diff = D - dg
        ek = kms * 2 * eps4(np.abs(diff)) * deps4(np.abs(diff))
        with np.errstate(divide="ignore", invalid="ignore"):
            Cb = np.where(D > 0, tbs * 2 * diff / D, 0.0)
            Ck = np.where(D > 0, ek * np.sign(diff) / D, 0.0)
        np.add.at(gb[b], ci, kb * _pair_grad(Cb, xc))
        np.add.at(gk[b], ci, kk * _pair_grad(Ck, xc))
        np.add.at(a[b], ci, kk * np.where((np.abs(diff) < tau) & (D > 0), ek, 0.0).sum(1))
    return gb, gk, a


def distogram_grad(p_distogram, x_gt, x_exists, pseudo_beta, boundaries_sq, no_bins):
    md, sm, _, onehot = distogram_parts(p_distogram, x_gt, x_exists, pseudo_beta, boundaries_sq, no_bins)
    return (md ** 3)[..., None] * (sm - onehot) / (1e-9 + md.sum())


def weighted_mse_grad(x_denoised, x_gt_aligned, weights, t_hat):
    r, w = f64(x_denoised) - f64(x_gt_aligned), f64(weights)
    B = r.shape[0]
    v = weighted_mse_pre_clamp(x_denoised, x_gt_aligned, weights, t_hat)
    k = 2.0 * edm_scale(t_hat, SD_MSE) / (3.0 * (1e-9 + B * w.sum())) if v <= CLAMP_MSE else 0.0      # NaN <= 1e4 is False
    return k * w[None, :, None] * r if k else np.zeros_like(r)


# ------------------------------------------------------------------ margins
def clamp_margin(x_gt, clamp):
    """closest relative distance of a ground-truth pair to the clamp radius"""
    dgt = pairdist(f64(x_gt))
    return float(np.abs(dgt - clamp).min() / clamp)


def bin_margin(x_gt, pseudo_beta, boundaries_sq):
    """closest relative distance of a pseudo-beta pair's squared distance to a squared bin edge"""
    pb = np.asarray(pseudo_beta, dtype=np.int64)
    b2 = f64(boundaries_sq)
    d2 = pairdist2(f64(x_gt)[pb])
    return float((np.abs(d2[..., None] - b2) / b2).min())


# ------------------------------------------------------------------ the same forward in torch float64, for autograd
def _t(a, dtype=np.float64):
    import torch
    return torch.as_tensor(np.asarray(a, dtype=dtype))


def _tnorm(v):
    import torch
    return torch.norm(v, dim=-1)


def _te4(d):
    import torch
    return sum(torch.sigmoid(d - c) for c in CS) / 4


def _tsc(t_hat, sd):
    t = _t(t_hat)
    return ((t ** 2 + sd ** 2) / (t * sd) ** 2).mean()


def torch_smooth_lddt(xd, x_gt, x_exists, clamp):
    """xd: float64 tensor [B,A,3] (the caller's leaf); a 0-d float64 tensor"""
    xg, ex = _t(x_gt), _t(x_exists)
    dgt = _tnorm(xg[:, None] - xg[None])
    m = (dgt < clamp) * ex[:, None] * ex[None]
    d = _tnorm(xd[:, :, None] - xd[:, None, :])
    return ((m * _te4((d - dgt).abs())).sum((-1, -2)) / (1e-9 + m.sum())).mean()


def torch_centre_pairs(xd, x_gt, centre, token_bonds, is_key_res, is_ligand, t_hat, sd_bond, sd_key, eps):
    ci = _t(centre, np.int64)
    xc, gc = xd[:, ci], _t(x_gt)[ci]
    diff = _tnorm(xc[:, :, None] - xc[:, None, :]) - _tnorm(gc[:, None] - gc[None])
    tb, km = _t(token_bonds), _t(is_key_res)[:, None] * _t(is_ligand)[None]
    return (_tsc(t_hat, sd_bond) * ((tb * diff ** 2).sum((-1, -2)) / (tb.sum() + eps)).mean(),
            _tsc(t_hat, sd_key) * ((km * _te4(diff.abs()) ** 2).sum((-1, -2)) / (km.sum() + eps)).mean())


def torch_distogram(p, x_gt, x_exists, pseudo_beta, boundaries_sq, no_bins):
    import torch
    pb, ex = _t(pseudo_beta, np.int64), _t(x_exists)
    gp = _t(x_gt)[pb]
    bins = (((gp[:, None] - gp[None]) ** 2).sum(-1)[..., None] > _t(boundaries_sq)).sum(-1)
    md = ex[pb][:, None] * ex[pb][None]
    logp = torch.log_softmax(p * md[..., None], -1)
    err = -(torch.nn.functional.one_hot(bins, no_bins) * md[..., None] * logp).sum(-1)
    return (md * err).sum() / (1e-9 + md.sum())


def torch_weighted_mse(xd, x_gt_aligned, weights, t_hat):
    import torch
    w = _t(weights)
    mm = (w[None] * ((xd - _t(x_gt_aligned)) ** 2).sum(-1)).sum() / (1e-9 + xd.shape[0] * w.sum())
    return torch.clamp(_tsc(t_hat, SD_MSE) * mm / 3, max=CLAMP_MSE)
