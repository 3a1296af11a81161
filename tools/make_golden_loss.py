"""Generate tests/golden/g15_loss_*.npz from the UNMODIFIED reference loss (PhysDock/models/loss.py), imported read-only.

    python tools/make_golden_loss.py [--ref /path/to/reference] [--only small,ragged]

Per fixture: the inputs (arrays only - never a pair tensor), the reference's five terms and PhysDockLoss total in fp32 on the
CPU (`ref_<term>`, `ref_loss`, `ref_cum_loss`), a float64 evaluation of the same formulas (`f64_<term>`, `f64_loss`) and the
relative distance of the reference's fp32 value to it (`ref_vs_f64_rel_<term>`, `ref_vs_f64_rel_loss`).  The generator refuses
a fixture in which a pair lies within a relative 1e-5 of a decision threshold (the smooth-lDDT clamp on the distance, a
distogram bin edge on the squared distance): two fp32 implementations may put such a pair on either side.  The closest
approach is printed and stored (`closest_clamp_rel`, `closest_bin_rel`).
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
#: outputs above this many bytes are not stored: the tests rebuild them bit for bit from the stored features and t_hat
#: (physdock_amd.synthetic.loss_case(stored=...), integer-hash noise) and check them against the stored float64 checksums
MAX_STORED = 512 << 10
MARGIN = 1e-5


# ------------------------------------------------------------------ float64 evaluation of the reference's formulas
def _eps64(d):
    return 0.25 * sum(1.0 / (1.0 + np.exp(c - d)) for c in (0.5, 1.0, 2.0, 4.0))


def _pdist64(x):
    return np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))


def f64_terms(o, f, cfg):
    """the five terms in float64 (numpy), sample by sample so that no [B,A,A] array exists"""
    xd, xg, ex = o["x_denoised"].astype(np.float64), f["x_gt"].astype(np.float64), f["x_exists"].astype(np.float64)
    t = o["t_hat"].astype(np.float64)
    B = xd.shape[0]
    res = {}
    # weighted MSE (loss.py:118-159): sigma_data = 16, one masked mean over samples and atoms
    c = cfg["weighted_mse_loss"]
    w = (1 + f["is_dna"] * c["alpha_dna"] + f["is_rna"] * c["alpha_rna"] + f["is_ligand"] * c["alpha_ligand"]).astype(np.float64)
    w = w[f["atom_id_to_token_id"]] * ex
    num = 0.0
    for b in range(B):
        xp = xd[b] * ex[:, None]
        mu_p, mu_g = (xp * w[:, None]).sum(0) / w.sum(), (xg * w[:, None]).sum(0) / w.sum()
        ph, gh = xp - mu_p, xg - mu_g
        H = np.einsum("ij,ik->jk", gh * w[:, None], ph)
        if not np.isfinite(H).all():
            num = float("nan")
            break
        U, _, Vh = np.linalg.svd(H)
        R = U @ Vh
        if np.linalg.det(R) < 0:
            R = U @ np.diag([1.0, 1.0, -1.0]) @ Vh
        al = gh @ R + mu_p                      # einsum("ij,kj->ki", R^T, gh)
        num += (w * ((xd[b] - al) ** 2).sum(-1)).sum()
    scale = (t ** 2 + 16.0 ** 2) / (t * 16.0) ** 2
    res["weighted_mse_loss"] = min(float((scale * (num / (1e-9 + B * w.sum())) / 3).mean()), 10000.0) if np.isfinite(num) else float("nan")
    # smooth lDDT (loss.py:162-181)
    dgt = _pdist64(xg)
    m = (dgt < cfg["smooth_lddt_loss"]["max_clamp_distance"]) * ex[:, None] * ex[None, :]
    per = []
    for b in range(B):
        e = _eps64(np.abs(_pdist64(xd[b]) - dgt))
        per.append((m * e).sum() / (1e-9 + m.sum()))
    res["smooth_lddt_loss"] = float(np.mean(per))
    # bond / key residue (loss.py:245-318, 535-559)
    ci = f["token_id_to_centre_atom_id"]
    dg = _pdist64(xg[ci])
    tb = f["token_bonds"].astype(np.float64)
    km = f["is_key_res"].astype(np.float64)[:, None] * f["is_ligand"].astype(np.float64)[None, :]
    sb, sk = [], []
    for b in range(B):
        diff = _pdist64(xd[b][ci]) - dg
        sb.append((tb * diff ** 2).sum() / (tb.sum() + 1e-9))
        sk.append((km * _eps64(np.abs(diff)) ** 2).sum() / (km.sum() + 1e-9))
    for name, s in (("bond_loss", sb), ("key_res_loss", sk)):
        sd = cfg[name]["sigma_data"]
        res[name] = float(((t ** 2 + sd ** 2) / (t * sd) ** 2 * np.mean(s)).mean())
    # distogram (loss.py:78-115)
    c = cfg["distogram_loss"]
    pb = f["token_id_to_pseudo_beta_atom_id"]
    b2 = np.linspace(c["min_bin"], c["max_bin"], c["no_bins"] - 1) ** 2
    d2 = ((xg[pb][:, None] - xg[pb][None]) ** 2).sum(-1)
    bins = (d2[..., None] > b2).sum(-1)
    md = ex[pb][:, None] * ex[pb][None, :]
    lg = o["p_distogram"].astype(np.float64) * md[..., None]
    mx = lg.max(-1, keepdims=True)
    lsm = lg - mx - np.log(np.exp(lg - mx).sum(-1, keepdims=True))
    err = -md * np.take_along_axis(lsm, bins[..., None], -1)[..., 0]
    res["distogram_loss"] = float((md * err).sum() / (1e-9 + md.sum()))
    return res


def closest_approach(f, cfg):
    """smallest relative distance of a pair to the smooth-lDDT clamp (on d) and to a distogram bin edge (on d^2), in float64"""
    xg = f["x_gt"].astype(np.float64)
    clamp = cfg["smooth_lddt_loss"]["max_clamp_distance"]
    r_clamp = float(np.abs(_pdist64(xg) - clamp).min() / clamp)
    c = cfg["distogram_loss"]
    pb = f["token_id_to_pseudo_beta_atom_id"]
    b2 = np.linspace(c["min_bin"], c["max_bin"], c["no_bins"] - 1) ** 2
    d2 = ((xg[pb][:, None] - xg[pb][None]) ** 2).sum(-1)
    r_bin = float((np.abs(d2[..., None] - b2) / b2).min())
    return r_clamp, r_bin


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else (0.0 if a == 0 else float("inf"))


# ------------------------------------------------------------------ fixtures
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("PHYSDOCK_REFERENCE", "/root/reference"))
    ap.add_argument("--only", default="small,ragged,cfg1,degenerate,nan")
    ap.add_argument("--cfg1-samples", type=int, default=48)
    args = ap.parse_args()
    import tools.make_golden as mg
    mg.REF = args.ref
    mg.install_shims()
    import PhysDock.models.loss as RL
    from physdock_amd.synthetic import LOSS_FEAT_KEYS, LOSS_OUT_KEYS, loss_case
    from PhysDock.configs import PhysDockConfig as RefConfig
    rcfg = RefConfig(model_name="medium")
    lcfg = {k: dict(rcfg.loss[k]) for k in TERMS}
    for name in args.only.split(","):
        o, f, note = loss_case(name, args.cfg1_samples)
        r_clamp, r_bin = closest_approach({k: v.numpy() for k, v in f.items()}, lcfg)
        print(f"g15_loss_{name}: closest approach to the clamp {r_clamp:.3e}, to a bin edge {r_bin:.3e}")
        assert r_clamp > MARGIN and r_bin > MARGIN, "a pair sits on a decision threshold: choose another seed"
        ref, raised = {}, {}
        with torch.no_grad():
            for t in TERMS:
                try:
                    ref[t] = float(getattr(RL, t)(**o, **f, **{k: v for k, v in lcfg[t].items() if k != "weight"}))
                except RuntimeError as e:       # torch.linalg.svd refuses a non-finite matrix on the CPU: the term has no value
                    ref[t], raised[t] = float("nan"), type(e).__name__
                    print(f"    {t}: the reference raises {type(e).__name__}")
            logging.disable(logging.WARNING)
            if raised:                           # the class raises with it; its total is the weighted sum of the finite terms
                cum = torch.tensor(0.)
                for t in TERMS:
                    cum = cum + lcfg[t]["weight"] * (torch.tensor(ref[t]) if np.isfinite(ref[t]) else torch.tensor(0.))
                losses = {**{t: ref[t] if np.isfinite(ref[t]) else 0.0 for t in TERMS}, "loss": cum}
            else:
                cum, losses = RL.PhysDockLoss(rcfg)(o, f)
            logging.disable(logging.NOTSET)
        for t in TERMS:      # the class returns the same terms, NaN / Inf ones replaced by zero
            assert float(losses[t]) == (ref[t] if np.isfinite(ref[t]) else 0.0), (t, float(losses[t]), ref[t])
        f64 = f64_terms({k: v.numpy() for k, v in o.items()}, {k: v.numpy() for k, v in f.items()}, lcfg)
        f64["loss"] = sum(lcfg[t]["weight"] * (f64[t] if np.isfinite(f64[t]) else 0.0) for t in TERMS)
        arrays = {"case": np.array(name), "cfg1_samples": np.int64(args.cfg1_samples)}
        for k, v in {**o, **f}.items():
            v = v.numpy()
            if v.nbytes <= MAX_STORED or k in LOSS_FEAT_KEYS or k == "t_hat":
                arrays[k] = v
            arrays["checksum_" + k] = np.array([np.nansum(v.astype(np.float64)), np.nansum(v.astype(np.float64) ** 2)])
        for t in TERMS:
            assert np.isfinite(ref[t]) == np.isfinite(f64[t]), (t, ref[t], f64[t])
            arrays["ref_" + t], arrays["f64_" + t] = np.float32(ref[t]), np.float64(f64[t])
            arrays["ref_vs_f64_rel_" + t] = np.float64(rel(ref[t], f64[t]) if np.isfinite(ref[t]) else 0.0)
            print(f"    {t:18s} ref {ref[t]:.8g}  f64 {f64[t]:.12g}  rel {float(arrays['ref_vs_f64_rel_' + t]):.2e}")
        arrays["ref_loss"], arrays["ref_cum_loss"], arrays["f64_loss"] = np.float32(float(losses["loss"])), np.float32(float(cum)), np.float64(f64["loss"])
        arrays["ref_vs_f64_rel_loss"] = np.float64(rel(float(cum), f64["loss"]))
        print(f"    {'loss':18s} ref {float(cum):.8g}  f64 {f64['loss']:.12g}  rel {float(arrays['ref_vs_f64_rel_loss']):.2e}")
        arrays["weights"] = np.array([lcfg[t]["weight"] for t in TERMS], dtype=np.float64)
        arrays["closest_clamp_rel"], arrays["closest_bin_rel"] = np.float64(r_clamp), np.float64(r_bin)
        arrays["ref_raised"] = np.array([t in raised for t in TERMS])
        arrays["note"] = np.array(note)
        path = os.path.join(OUT, f"g15_loss_{name}.npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
        print(f"    wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
