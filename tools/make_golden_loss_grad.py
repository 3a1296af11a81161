"""Generate tests/golden/g16_loss_grad_*.npz: gradients of the UNMODIFIED reference loss (PhysDock/models/loss.py, imported
read-only) with respect to x_denoised and p_distogram, by torch autograd in fp32 on the CPU, next to an independent float64
restatement of the same gradients.

    python tools/make_golden_loss_grad.py [--ref /path/to/reference] [--only small,clamped]

Cases: the g15 inputs (small, ragged, cfg1, degenerate, nan; rebuilt through synthetic.loss_case as make_golden_loss.py does)
and three built here from the small case: clamped (t_hat small enough that the weighted MSE is above the 1e4 clamp),
shared-centre (two pairs of tokens with one centre atom each) and grad-only-p (x_denoised does not require grad).

Per case and term t (x terms: gradient to x_denoised [B,A,3]; distogram: gradient to p_distogram [T,T,bins]):
  g64_<t>      float64 restatement (below), on the stored rows    ref_<t>    the reference's fp32 autograd gradient, same rows
  allow_<t>    (smooth lDDT, key-res) per atom and sample: sum of |contribution| over the pairs with |delta| < tau, tau = 8 fp32
               ulp of the largest |coordinate|: there sign(d - d_gt) may come out either way in two fp32 implementations.
               A flip from +1 to -1 moves a pair by twice its contribution; the reference's own flips of that kind show in
               e_ref (ragged smooth lDDT: one pair, 1.2e-3 of max |g64|), which the tests' tol = max(2e-5, 4 e_ref) takes on
  absmax_<t>   max |g64| per sample (x terms) / of the array (distogram), over the FULL arrays
  e_ref_<t>    the reference's own distance to g64: max over samples of max(0, |ref - g64| - allow) / absmax
  ratio_<t>    max over samples of sum(allow) / ||g64||_1 (the generator refuses a fixture above 1 %)
  sum_g64_<t>  float64 [sum, sum of squares] of the full g64 array; allow_sum_<t>, allow_max_<t> of the full allowance
  has_<t>      False where the term is not differentiated: non-finite (nan case: skipped, no gradient) or its input does not
               require grad (grad-only-p)
Rows: every sample / token where the array is small, else `rows` (samples) and `prow` (token rows of g_p); the checksums and
maxima always cover the full arrays.  The total: e_ref_cum_x / e_ref_cum_p of the reference's gradient of PhysDockLoss's cum
(the weighted sum of the finite terms' gradients) against sum_t weight_t g64_t.  cfg1's smooth lDDT is run by the reference in
chunks of 4 samples (the loss is a sample mean: chunk gradient x 4 / B) to keep its [B,A,A] autograd tensors in memory.
"""
import argparse
import logging
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")
TERMS = ("weighted_mse_loss", "smooth_lddt_loss", "bond_loss", "key_res_loss", "distogram_loss")
X_TERMS = TERMS[:4]
G15 = ("small", "ragged", "cfg1", "degenerate", "nan")
NEW = ("clamped", "shared-centre", "grad-only-p")
MAX_RATIO = 0.01
AGREE = 1e-3          # the restatement and the reference's fp32 autograd agree to this (relative to max |g64|, after the allowance)


# ------------------------------------------------------------------ float64 restatement of the gradients
def _pd(x):
    return np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))


def _sig(d):
    return [1.0 / (1.0 + np.exp(c - d)) for c in (0.5, 1.0, 2.0, 4.0)]


def _eps(d):
    return 0.25 * sum(_sig(d))


def _deps(d):
    return 0.25 * sum(s * (1.0 - s) for s in _sig(d))


def _pair_grad(C, x):
    """sum_j C_ij (x_i - x_j)"""
    return C.sum(1)[:, None] * x - C @ x


def g64_weighted_mse(o, f, c):
    xd, xg, ex, t = (a.astype(np.float64) for a in (o["x_denoised"], f["x_gt"], f["x_exists"], o["t_hat"]))
    B = xd.shape[0]
    w = (1 + f["is_dna"] * c["alpha_dna"] + f["is_rna"] * c["alpha_rna"] + f["is_ligand"] * c["alpha_ligand"]).astype(np.float64)
    w = w[f["atom_id_to_token_id"]] * ex
    g, num = np.zeros_like(xd), 0.0
    for b in range(B):
        xp = xd[b] * ex[:, None]
        mu_p, mu_g = w @ xp / w.sum(), w @ xg / w.sum()
        H = (xg - mu_g).T @ (w[:, None] * (xp - mu_p))
        U, _, Vh = np.linalg.svd(H)
        R = U @ Vh
        if np.linalg.det(R) < 0:
            R = U @ np.diag([1.0, 1.0, -1.0]) @ Vh
        r = xd[b] - ((xg - mu_g) @ R + mu_p)
        num += (w * (r ** 2).sum(-1)).sum()
        g[b] = 2 * w[:, None] * r
    sc = ((t ** 2 + 256.0) / (t * 16.0) ** 2).mean()
    value = sc * num / (1e-9 + B * w.sum()) / 3
    k = sc / (3 * (1e-9 + B * w.sum())) if value <= 1e4 else 0.0          # torch.clamp(max=1e4) passes nothing above
    return g * k, None, value


def g64_smooth_lddt(o, f, c, tau):
    xd, xg, ex = (a.astype(np.float64) for a in (o["x_denoised"], f["x_gt"], f["x_exists"]))
    B = xd.shape[0]
    dgt = _pd(xg)
    m = (dgt < c["max_clamp_distance"]) * np.outer(ex, ex)
    k = 1.0 / B / (1e-9 + m.sum())
    ms = m + m.T
    g, a = np.zeros_like(xd), np.zeros(xd.shape[:2])
    for b in range(B):
        D = _pd(xd[b])
        dl = D - dgt
        e = ms * _deps(np.abs(dl))
        with np.errstate(divide="ignore", invalid="ignore"):
            C = np.where(D > 0, e * np.sign(dl) / D, 0.0)
        g[b] = k * _pair_grad(C, xd[b])
        a[b] = k * np.where((np.abs(dl) < tau) & (D > 0), e, 0.0).sum(1)
    return g, a


def g64_centre(o, f, c, which, tau):
    xd, xg, t = (a.astype(np.float64) for a in (o["x_denoised"], f["x_gt"], o["t_hat"]))
    B, A = xd.shape[:2]
    ci = f["token_id_to_centre_atom_id"].astype(np.int64)
    dg = _pd(xg[ci])
    if which == 0:
        M = f["token_bonds"].astype(np.float64)
    else:
        M = np.outer(f["is_key_res"], f["is_ligand"]).astype(np.float64)
    sd = c["sigma_data"]
    k = ((t ** 2 + sd ** 2) / (t * sd) ** 2).mean() / B / (M.sum() + 1e-9)
    Ms = M + M.T
    g, a = np.zeros_like(xd), np.zeros((B, A))
    for b in range(B):
        xc = xd[b][ci]
        D = _pd(xc)
        diff = D - dg
        if which == 0:
            e = Ms * 2 * diff
            s = np.ones_like(diff)
        else:
            e = Ms * 2 * _eps(np.abs(diff)) * _deps(np.abs(diff))
            s = np.sign(diff)
        with np.errstate(divide="ignore", invalid="ignore"):
            C = np.where(D > 0, e * s / D, 0.0)
        np.add.at(g[b], ci, k * _pair_grad(C, xc))
        if which == 1:
            np.add.at(a[b], ci, k * np.where((np.abs(diff) < tau) & (D > 0), np.abs(e), 0.0).sum(1))
    return g, (a if which == 1 else None)


def g64_distogram(o, f, c):
    xg, ex = f["x_gt"].astype(np.float64), f["x_exists"].astype(np.float64)
    pb = f["token_id_to_pseudo_beta_atom_id"]
    b2 = np.linspace(c["min_bin"], c["max_bin"], c["no_bins"] - 1) ** 2
    d2 = ((xg[pb][:, None] - xg[pb][None]) ** 2).sum(-1)
    bins = (d2[..., None] > b2).sum(-1)
    md = ex[pb][:, None] * ex[pb][None, :]
    lg = o["p_distogram"].astype(np.float64) * md[..., None]
    sm = np.exp(lg - lg.max(-1, keepdims=True))
    sm /= sm.sum(-1, keepdims=True)
    onehot = np.arange(c["no_bins"]) == bins[..., None]
    return (md ** 3)[..., None] * (sm - onehot) / (1e-9 + md.sum())


# ------------------------------------------------------------------ the reference's fp32 autograd
def ref_grad(RL, t, o, f, st, wrt, chunk=None):
    """gradient of the reference term t to `wrt` (x_denoised or p_distogram); None if the reference raises or the value is not
    finite (PhysDockLoss skips that term)"""
    B = o["x_denoised"].shape[0]
    if chunk and wrt == "x_denoised" and B > chunk:
        parts = []
        for b0 in range(0, B, chunk):
            oc = dict(o, x_denoised=o["x_denoised"][b0:b0 + chunk], t_hat=o["t_hat"][b0:b0 + chunk])
            g = ref_grad(RL, t, oc, f, st, wrt)
            if g is None:
                return None
            parts.append(g * np.float32(oc["x_denoised"].shape[0] / B))
        return np.concatenate(parts)
    leaf = o[wrt].clone().requires_grad_(True)
    try:
        v = getattr(RL, t)(**dict(o, **{wrt: leaf}), **f, **st)
    except RuntimeError:
        return None
    if not torch.isfinite(v):
        return None
    v.backward()
    return leaf.grad.numpy().copy()


def excess(ref, g64, allow, absmax):
    """max(0, |ref - g64| - allow) / absmax per sample (x: [B,A,3]; p: one 'sample')"""
    if g64.ndim == 3 and absmax.ndim == 1:
        d = np.abs(ref.astype(np.float64) - g64) - (allow[..., None] if allow is not None else 0.0)
        d = np.maximum(d, 0.0).reshape(g64.shape[0], -1).max(1)
        return float(max((di / m if m > 0 else (0.0 if di == 0 else np.inf)) for di, m in zip(d, absmax)))
    d = float(np.maximum(np.abs(ref.astype(np.float64) - g64), 0.0).max())
    return d / float(absmax) if absmax > 0 else (0.0 if d == 0 else np.inf)


# ------------------------------------------------------------------ cases
def build_case(name, B_cfg1):
    from physdock_amd.synthetic import loss_case
    if name in G15:
        o, f, note = loss_case(name, B_cfg1)
        return o, f, note, name, True
    o, f, _ = loss_case("small")
    if name == "clamped":
        o["t_hat"] = (o["t_hat"] * np.float32(1e-3)).contiguous()
        note = "the small case with t_hat x 1e-3: the weighted MSE before its clamp is above 1e4, so it has no gradient"
    elif name == "shared-centre":
        ci = f["token_id_to_centre_atom_id"].clone()
        key = torch.nonzero(f["is_key_res"]).flatten()
        prot = torch.nonzero((f["is_ligand"] == 0) & (f["is_key_res"] == 0)).flatten()
        lig = torch.nonzero(f["is_ligand"]).flatten()
        ci[int(prot[0])] = ci[int(key[0])]                    # a plain protein token names a key residue's centre atom
        ci[int(lig[-1])] = ci[int(lig[0])]                    # two ligand tokens name one atom
        f["token_id_to_centre_atom_id"] = ci
        note = (f"the small case with token {int(prot[0])} -> centre of key token {int(key[0])} and ligand token {int(lig[-1])} -> "
                f"centre of ligand token {int(lig[0])}")
    elif name == "grad-only-p":
        note = "the small case; x_denoised does not require grad, only p_distogram has a gradient"
    return o, f, note, "small", name != "grad-only-p"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("PHYSDOCK_REFERENCE", "/root/reference"))
    ap.add_argument("--only", default=",".join(G15 + NEW))
    ap.add_argument("--cfg1-samples", type=int, default=48)
    args = ap.parse_args()
    import tools.make_golden as mg
    mg.REF = args.ref
    mg.install_shims()
    import PhysDock.models.loss as RL
    from PhysDock.configs import PhysDockConfig as RefConfig
    from physdock_amd.synthetic import LOSS_FEAT_KEYS, LOSS_OUT_KEYS
    rcfg = RefConfig(model_name="medium")
    lcfg = {k: dict(rcfg.loss[k]) for k in TERMS}
    weights = np.array([lcfg[t]["weight"] for t in TERMS], dtype=np.float64)
    logging.disable(logging.WARNING)
    torch.set_num_threads(os.cpu_count() or 4)
    for name in args.only.split(","):
        o, f, note, base, need_x = build_case(name, args.cfg1_samples)
        on = {k: v.numpy() for k, v in o.items()}
        fn = {k: v.numpy() for k, v in f.items()}
        B, A = on["x_denoised"].shape[:2]
        T = fn["is_ligand"].shape[0]
        fin = np.isfinite(on["x_denoised"])
        tau = 8.0 * float(np.spacing(np.float32(max(np.abs(on["x_denoised"][fin]).max(), np.abs(fn["x_gt"]).max()))))
        rows = np.arange(B) if B * A <= 4096 else np.array([0, B - 1])
        prow = np.arange(T) if T <= 32 else np.array([0, T // 2, T - 1])
        arrays = {"case": np.array(name), "base": np.array(base), "note": np.array(note), "need_x": np.bool_(need_x),
                  "tau": np.float64(tau), "rows": rows, "prow": prow, "weights": weights}
        if name in NEW:
            for k in LOSS_FEAT_KEYS:
                arrays[k] = fn[k]
            for k in LOSS_OUT_KEYS:
                arrays[k] = on[k]
        print(f"g16_loss_grad_{name}: B = {B}, A = {A}, T = {T}, tau = {tau:.3e}")
        cum_ref_x, cum_64_x, cum_allow = np.zeros((B, A, 3), np.float32), np.zeros((B, A, 3)), np.zeros((B, A))
        for k, t in enumerate(TERMS):
            st = {kk: v for kk, v in lcfg[t].items() if kk != "weight"}
            wrt = "p_distogram" if t == "distogram_loss" else "x_denoised"
            if wrt == "x_denoised" and not need_x:
                arrays["has_" + t] = np.bool_(False)
                continue
            ref = ref_grad(RL, t, o, f, st, wrt, chunk=4 if (t == "smooth_lddt_loss" and name == "cfg1") else None)
            arrays["has_" + t] = np.bool_(ref is not None)
            if ref is None:
                print(f"    {t}: not finite in the reference (skipped by PhysDockLoss): no gradient")
                continue
            allow = None
            if t == "weighted_mse_loss":
                g64, _, value = g64_weighted_mse(on, fn, st)
                arrays["pre_clamp_weighted_mse"] = np.float64(value)
            elif t == "smooth_lddt_loss":
                g64, allow = g64_smooth_lddt(on, fn, st, tau)
            elif t in ("bond_loss", "key_res_loss"):
                g64, allow = g64_centre(on, fn, st, 0 if t == "bond_loss" else 1, tau)
            else:
                g64 = g64_distogram(on, fn, st)
            if wrt == "x_denoised":
                absmax = np.abs(g64).reshape(B, -1).max(1)
                l1 = np.abs(g64).reshape(B, -1).sum(1)
                ratio = 0.0
                if allow is not None:
                    for b in range(B):
                        r = allow[b].sum() / l1[b] if l1[b] > 0 else (0.0 if allow[b].sum() == 0 else np.inf)
                        ratio = max(ratio, float(r))
                    assert ratio <= MAX_RATIO, f"{name} {t}: allowance ratio {ratio:.3e} above {MAX_RATIO}: choose other inputs"
                    arrays["allow_" + t] = allow[rows]
                    arrays["allow_sum_" + t], arrays["allow_max_" + t] = np.float64(allow.sum()), np.float64(allow.max())
                    arrays["ratio_" + t] = np.float64(ratio)
                e = excess(ref, g64, allow, absmax)
                # the restatement agrees with the reference away from ties: at a tie the reference may flip a sign, which moves
                # the pair by up to twice its contribution (2 x allow)
                e_agree = excess(ref, g64, None if allow is None else 2 * allow, absmax)
                arrays["ref_" + t], arrays["g64_" + t] = ref[rows], g64[rows]
                cum_ref_x += np.float32(weights[k]) * ref
                cum_64_x += weights[k] * g64
                if allow is not None:
                    cum_allow += weights[k] * allow
            else:
                absmax = np.float64(np.abs(g64).max())
                e = excess(ref, g64, None, absmax)
                e_agree = e
                arrays["ref_" + t], arrays["g64_" + t] = ref[prow], g64[prow]
                ref_p = ref
            arrays["absmax_" + t] = np.asarray(absmax, dtype=np.float64)
            arrays["e_ref_" + t] = np.float64(e)
            arrays["sum_g64_" + t] = np.array([g64.sum(), (g64 ** 2).sum()])
            print(f"    {t:18s} max|g64| {float(np.max(absmax)):.4e}  e_ref {e:.3e}" +
                  (f"  allowance ratio {arrays['ratio_' + t]:.2e}" if allow is not None else ""))
            assert e_agree <= AGREE, f"{name} {t}: the float64 restatement and the reference's autograd disagree ({e_agree:.3e})"
            assert e <= max(2e-5, 4 * e), (name, t)           # the reference passes the tests' bar (tol = max(2e-5, 4 e_ref))
        # the total: PhysDockLoss's cum = sum_t weight_t term_t over the finite terms
        if need_x:
            absmax = np.abs(cum_64_x).reshape(B, -1).max(1)
            arrays["e_ref_cum_x"] = np.float64(excess(cum_ref_x, cum_64_x, cum_allow, absmax))
            print(f"    cum (x)            e_ref {float(arrays['e_ref_cum_x']):.3e}")
        gp64 = weights[4] * g64_distogram(on, fn, lcfg["distogram_loss"])
        arrays["e_ref_cum_p"] = np.float64(excess(np.float32(weights[4]) * ref_p, gp64, None, np.abs(gp64).max()))
        print(f"    cum (p)            e_ref {float(arrays['e_ref_cum_p']):.3e}")
        path = os.path.join(OUT, f"g16_loss_grad_{name}.npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
        print(f"    wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
