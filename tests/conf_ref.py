"""The operations of csrc/confidence_loss.hip and csrc/metrics.hip restated in numpy, per row and for any no_bins, min_bin and
max_bin.  Every function takes `dtype`: np.float64 is the definition the kernel tests compare with, np.float32 is the plain fp32
evaluation of the same formula, whose distance from the former is the `e32` of the bars (tests/test_metrics_cpu.bound).

They generalise the float64 restatements of tests/test_confidence_loss_cpu.py (lddt_sums, lddt_bin, in_frame, binned, masked_ce)
and tests/test_metrics_cpu.py (softmax, centres, has_clash), which were written from the reference's formulas and are imported
from there; tests/test_conf_ref_cpu.py checks that both sets agree on the g17 and g18 fixtures."""
import numpy as np

from test_confidence_loss_cpu import binned, lddt_bin, lddt_sums, norm
from test_metrics_cpu import centres, softmax        # noqa: F401  (centres: re-exported for the cases)

COS_VALID = 0.906308
CLASH_DIST = 1.1


def ulp32(v):
    return float(np.spacing(np.float32(np.abs(v).max())))


def bar(v32, v64):
    """(e32, 4 e32 + 8 ulp32(max |f64|)): the rule of tests/test_sampler_kernels_gpu.py and tests/test_metrics_cpu.bound"""
    v64 = np.asarray(v64, np.float64)
    e32 = float(np.abs(np.asarray(v32, np.float64) - v64).max())
    return e32, 4 * e32 + 8 * ulp32(v64)


# ------------------------------------------------------------------ confidence_loss.hip
def lddt(x_pred, x_gt, centre, is_dna, is_rna, is_polymer):
    """cal_lddt: (lddt [B,A] as the reference's fp32 gives it, NaN where no token is included; num, den [B,A] in float64).
    The decisions are taken in float64, the ratio is the one fp32 division of the two exact sums."""
    f = lambda a: np.asarray(a, np.float64)
    num, den = lddt_sums(f(x_pred), f(x_gt), f(is_dna), f(is_rna), f(is_polymer), np.asarray(centre))
    return lddt_bin(num, den, 1)[0], num, den


def plddt_bins(lddt_row, no_bins):
    """clamp(long(lddt * no_bins), 0, no_bins - 1) of fp32 lDDT values: one fp32 product, truncation, NaN -> 0"""
    with np.errstate(invalid="ignore"):
        v = np.asarray(lddt_row, np.float32) * np.float32(no_bins)
    return np.where(np.isnan(v), 0, np.clip(np.trunc(np.nan_to_num(v)), 0, no_bins - 1)).astype(np.int64)


def frames(x, ids, dtype=np.float64):
    """express_coordinates_in_frame per token: ([T,13] = e1 | e2 | e3 | origin b | valid, cos [T], |w1 + w2| and |w2 - w1| [T])"""
    x = np.asarray(x).astype(dtype)
    eps = dtype(1e-6)
    a, b, c = x[ids[0]], x[ids[1]], x[ids[2]]
    w1 = (a - b) / norm(a - b + eps)[:, None]
    w2 = (c - b) / norm(c - b + eps)[:, None]
    cos = (w1 * w2).sum(-1)
    e1 = (w1 + w2) / norm(w1 + w2 + eps)[:, None]
    e2 = (w2 - w1) / norm(w2 - w1 + eps)[:, None]
    valid = (cos < dtype(COS_VALID)).astype(dtype)
    return np.concatenate([e1, e2, np.cross(e1, e2), b, valid[:, None]], -1), cos, np.stack([norm(w1 + w2), norm(w2 - w1)])


def frames_zero_past(x, ids, first=256):
    """WRONG on purpose: the tokens >= `first` are left at zero (a kernel that ran one block only)"""
    fr = frames(x, ids)[0]
    fr[first:] = 0
    return fr


def pde_error(x_pred0, x_gt, centre, dtype=np.float64):
    xp, xg = np.asarray(x_pred0).astype(dtype)[centre], np.asarray(x_gt).astype(dtype)[centre]
    return np.abs(norm(xp[:, None] - xp[None]) - norm(xg[:, None] - xg[None]))


def pae_error(x_pred0, x_gt, centre, fr_pred, fr_gt, dtype=np.float64):
    """|R_p (x_j - b_p) - R_g (xg_j - b_g)| valid_g valid_p [T,T] with the frames [T,13] as given (the launcher's own inputs)"""
    def local(x, fr):
        fr = np.asarray(fr).astype(dtype)
        d = np.asarray(x).astype(dtype)[centre][None, :, :] - fr[:, None, 9:12]
        return np.einsum("fij,faj->fai", fr[:, :9].reshape(-1, 3, 3), d), fr[:, 12]
    up, vp = local(x_pred0, fr_pred)
    ug, vg = local(x_gt, fr_gt)
    return norm(up - ug) * vg[:, None] * vp[:, None]


def pair_bins(e, min_bin, max_bin, no_bins, use_min_bin=True):
    """use_min_bin=False is WRONG on purpose: min_bin ignored in the numerator"""
    return binned(e, min_bin, max_bin, no_bins) if use_min_bin else binned(e + min_bin, min_bin, max_bin, no_bins)


def edge_margin(e, min_bin, max_bin, no_bins):
    """distance of every error to the nearest INNER bin edge (min_bin + k step, 0 < k < no_bins; the two outer edges decide nothing:
    below the first and above the last the index is clamped).  inf for no_bins = 1."""
    if no_bins < 2:
        return np.full(np.shape(e), np.inf)
    step = (max_bin - min_bin) / no_bins
    k = np.clip(np.round((np.asarray(e, np.float64) - min_bin) / step), 1, no_bins - 1)
    return np.abs(e - (min_bin + k * step))


def ce(logits, bins, mask, scale=1.0, dtype=np.float64, lanes=None):
    """softmax_cross_entropy(p m, onehot m) under masked_mean: (loss, per-row ce [R], gradient coef m^3 (softmax - onehot) [R,nb]),
    coef = scale / (1e-9 + sum m).  logits [R,nb], bins, mask [R].
    lanes=64 is WRONG on purpose: the softmax runs over 64 lanes with zeros in place of -inf for the bins >= nb."""
    z = np.asarray(logits).astype(dtype) * np.asarray(mask).astype(dtype)[:, None]
    m = np.asarray(mask).astype(dtype)
    nb = z.shape[-1]
    if lanes:
        z = np.concatenate([z, np.zeros((z.shape[0], lanes - nb), dtype)], -1)
    z = z - z.max(-1, keepdims=True)
    ez = np.exp(z)
    s = ez.sum(-1, keepdims=True)
    logp = (z - np.log(s))[:, :nb]
    onehot = (np.arange(nb) == np.asarray(bins)[:, None]).astype(dtype)
    row = -m * (onehot * logp).sum(-1)
    den = dtype(1e-9) + m.sum(dtype=dtype)
    loss = (m * row).sum(dtype=dtype) / den
    g = (dtype(scale) / den) * (m ** 3)[:, None] * ((ez / s)[:, :nb] - onehot)
    return loss, row, g


# ------------------------------------------------------------------ metrics.hip
def plddt(logits, dtype=np.float64, lanes=None):
    """compute_plddt: (atom_plddts [P,A], mean_plddt [P]); bin centres (k + 0.5) / nb.
    lanes=64 is WRONG on purpose: zeros in place of -inf for the bins >= nb (centre 0)"""
    l = np.asarray(logits).astype(dtype)
    nb = l.shape[-1]
    c = ((np.arange(nb) + 0.5) / nb).astype(dtype)
    if lanes:
        l = np.concatenate([l, np.zeros(l.shape[:-1] + (lanes - nb,), dtype)], -1)
        c = np.concatenate([c, np.zeros(lanes - nb, dtype)])
    atom = (softmax(l) * c).sum(-1) * dtype(100)
    return atom, atom.mean(-1)


def tm_d0(w):
    return 1.24 * (max(int(np.asarray(w, np.float64).sum()), 19) - 15) ** (1.0 / 3.0) - 1.8


def pae_tm(logits, cen, w, asym, dtype=np.float64, tie="first", keep=None):
    """compute_predicted_aligned_error and predicted_tm_score for P logit sets [P,T,T,nb]: dict of pae [P,T,T], ptm, iptm [P],
    rows [P,2], per_alignment [P,2,T], gaps [P,2] (top two of per_alignment_i w_i).  asym None: one chain (ipTM 0, row 0).
    tie="last" is WRONG on purpose (the last maximal row); keep [T] bool is WRONG on purpose (the pairs j outside it are dropped
    from the numerator)."""
    w = np.asarray(w).astype(dtype)
    T = w.shape[0]
    c = np.asarray(cen).astype(dtype)
    tmk = dtype(1) / (dtype(1) + c * c / (dtype(tm_d0(w)) ** 2))
    asym = np.zeros(T, np.int64) if asym is None else np.asarray(asym)
    out = {k: [] for k in ("pae", "ptm", "iptm", "rows", "per_alignment", "gaps")}
    for lp in logits:                                               # one set at a time: the stack of eight is 270 MB in float64
        probs = softmax(np.asarray(lp).astype(dtype))
        out["pae"].append((probs * c).sum(-1))
        tm = (probs * tmk).sum(-1)
        if keep is not None:
            tm = tm * keep[None, :]
        rows, pas, gaps, vals = [], [], [], []
        for m in (np.ones((T, T), dtype), (asym[:, None] != asym[None, :]).astype(dtype)):
            pw = m * (w[None, :] * w[:, None])
            per = (tm * m * (pw / (dtype(1e-8) + pw.sum(-1, keepdims=True)))).sum(-1)
            sel = per * w
            r = int(sel.argmax()) if tie == "first" else int(T - 1 - sel[::-1].argmax())
            top = np.sort(sel)
            rows.append(r)
            pas.append(per)
            gaps.append(top[-1] - top[-2] if T > 1 else np.inf)
            vals.append(per[r])
        out["ptm"].append(vals[0])
        out["iptm"].append(vals[1])
        out["rows"].append(rows)
        out["per_alignment"].append(np.stack(pas))
        out["gaps"].append(gaps)
    return {k: np.asarray(v) for k, v in out.items()}


def clash(x, a_mask, chain, polymer, n_chain):
    """get_has_clash on dense chain ids: (counts [B,nc,nc] of ORDERED eligible pairs closer than 1.1 A, i == j included;
    has_clash [B]; has_clash [B] with the loop restricted to a < c; the distance of an eligible pair (i != j) nearest to 1.1).
    Eligible: a_mask == 1, polymer != 0, chain in [0, nc).  The reference loops a over uniq[:-1] and c over uniq[1:] of the
    chains with eligible atoms."""
    x = np.asarray(x, np.float64)
    chain = np.asarray(chain)
    el = (np.asarray(a_mask) == 1) & (np.asarray(polymer) != 0) & (chain >= 0) & (chain < n_chain)
    ce_, xe = chain[el], x[:, el]
    d = norm(xe[:, :, None] - xe[:, None])
    onehot = (ce_[:, None] == np.arange(n_chain)[None]).astype(np.float64)
    counts = np.stack([onehot.T @ (db < CLASH_DIST) @ onehot for db in d]).astype(np.int64)      # small integers: exact
    N = onehot.sum(0).astype(np.int64)
    uniq = np.nonzero(N)[0]
    has = np.zeros((2, x.shape[0]), np.int64)
    for b in range(x.shape[0]):
        for a in uniq[:-1]:
            for c in uniq[1:]:
                n = counts[b, a, c]
                if n > 100 or n / min(N[a], N[c]) > 0.5:
                    has[0, b] = 1
                    has[1, b] |= int(a < c)
    off = ~np.eye(len(ce_), dtype=bool)
    closest = float(np.abs(d[:, off] - CLASH_DIST).min()) if off.any() else np.inf
    return counts, has[0], has[1], closest


def ranking(ptm, iptm, has, dtype=np.float64):
    return dtype(0.8) * np.asarray(iptm).astype(dtype) + dtype(0.2) * np.asarray(ptm).astype(dtype) - np.asarray(has).astype(dtype)
