"""Plain float64 references of the trunk "glue" kernels (physdock_amd/csrc/pair.hip) and the rounding bounds their tests use.

torch on the CPU, no device code.  Every function transcribes the formula in the comment above its kernel (or the line of
oracle/physdock_oracle.py it stands for) as whole-tensor algebra; none of them follows a kernel's loop structure.  Shapes as the
C ABI has them: pos [A, 3], uid [A], cl / cm [A, c_ap], Wp [c_ap, 3], Wd / Wv [c_ap] (or [c_ap, 1]), ap [A, A, c_ap],
zt [T, T, c_ap], a2t [A], si / sj [T, CZ], W [CZ, 115] (the RelPos weight as the model stores it; the kernel takes its transpose),
wb [CZ], bonds [T, T], u [B, A, C], tok_start [T + 1], add [T, C], ba [B, A, C], us [B, T, C], y [R, C], x [N, C], idx [R].

Two kinds of expectation:

* exact - pair_gather_add, unpool_add, gather_rows_add, template_mask and the v == 0 entries of atom_pair_init do one IEEE fp32
  operation per element (or a product with a 0 / 1 factor).  Their references take ``dtype=torch.float32`` and then ARE that fp32
  operation, done by torch on the CPU; the device result is compared with torch.equal.
* bounded - atom_pair_init (v == 1), pair_init_z, segment_pool, axpby.  Next to each reference a ``*_bound`` function returns, per
  element, gamma_k * S with S the float64 sum of the absolute values of the terms that enter the element, k the number of fp32
  roundings on the longest chain of the formula (counted in the function's comment) and gamma_k = k u / (1 - k u), u = 2^-24
  (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1: the first-order count k u made rigorous).  Fusing a multiply
  and an add into one FMA only removes roundings from a chain, so the count covers contracted code as it stands.  Where the formula
  holds a division or a square root the bound is doubled (SAFETY_DIV) for `1.f / x` and sqrtf delivered within one ulp instead of
  half an ulp, and for a reciprocal-then-multiply in the place of a division.  Nothing here is tuned on a kernel's output.
"""
import torch

import physdock_oracle as orc

F64 = torch.float64
U32 = 2.0 ** -24                      # unit roundoff of fp32
SAFETY_DIV = 2.0                      # see the module docstring: applied to atom_pair_init and segment_pool only


def _d(t, dtype=F64):
    return None if t is None else torch.as_tensor(t).to(dtype)


def gamma(k):
    """gamma_k = k u / (1 - k u) per element; k a number or a tensor of rounding counts"""
    k = torch.as_tensor(k, dtype=F64)
    return k * U32 / (1 - k * U32)


# ------------------------------------------------------------------ the comparison every bounded test calls
def bound_ratio(dev, ref64, bound):
    """max over the elements of |dev - ref64| / bound; an element with bound 0 must be met exactly (ratio 0, else inf).
    A non-finite device value gives inf."""
    dev = torch.as_tensor(dev).detach().cpu().to(F64)
    assert dev.shape == ref64.shape == bound.shape, (dev.shape, ref64.shape, bound.shape)
    err = (dev - ref64).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    ratio = torch.where(torch.isfinite(dev), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max()) if ratio.numel() else 0.0


def assert_within_bound(kernel, case, dev, ref64, bound):
    """the one bounded comparison of tests/test_trunk_glue_kernels_gpu.py (tests/test_trunk_glue_ref_cpu.py runs the float64
    reference rounded to fp32, and deliberately wrong variants, through this same function).  Prints the worst |error| / bound."""
    dev = torch.as_tensor(dev).detach().cpu()
    assert torch.isfinite(dev).all(), (kernel, case, "non-finite (or never written) output element")
    ratio = bound_ratio(dev, ref64, bound)
    err = float((dev.to(F64) - ref64).abs().max()) if dev.numel() else 0.0
    print(f"BOUND | {kernel} | {case} | max |err| {err:.2e} | max bound {float(bound.max()):.2e} | mean |ref| "
          f"{float(ref64.abs().mean()):.2e} | worst err/bound {ratio:.3f}")
    assert ratio <= 1.0, (kernel, case, "worst |err| / bound", ratio)
    return ratio


# ------------------------------------------------------------------ atom_pair_init
def _pair_terms(pos, uid, Wp, Wd, Wv, dtype):
    pos = _d(pos, dtype)
    d = pos[:, None, :] - pos[None, :, :]
    v = (torch.as_tensor(uid)[:, None] == torch.as_tensor(uid)[None, :]).to(dtype)[..., None]
    inv = 1 / (1 + torch.linalg.norm(d, dim=-1, keepdim=True))
    return d, v, inv, _d(Wp, dtype), _d(Wd, dtype).reshape(-1), _d(Wv, dtype).reshape(-1)


def atom_pair_init64(pos, uid, cl, cm, Wp, Wd, Wv, dtype=F64):
    """ap[l, m, :] = cl[l] + cm[m] + v (Wp . d + Wd / (1 + |d|) + Wv),  d = pos_l - pos_m,  v = [uid_l == uid_m]"""
    d, v, inv, Wp, Wd, Wv = _pair_terms(pos, uid, Wp, Wd, Wv, dtype)
    return _d(cl, dtype)[:, None, :] + _d(cm, dtype)[None, :, :] + v * (d @ Wp.T + inv * Wd + Wv)


def atom_pair_same_uid(uid):
    uid = torch.as_tensor(uid)
    return uid[:, None] == uid[None, :]


def atom_pair_init_bound(pos, uid, cl, cm, Wp, Wd, Wv):
    """k = 10, doubled (SAFETY_DIV: the formula has a square root and a reciprocal).  The longest chain is the Wd / (1 + |d|) term:
    d_x = pos_l - pos_m (1 rounding) -> d_x^2 (2 * 1 + 1 = 3 relative roundings) -> the sum of three squares (+2 = 5) -> sqrt
    (halves what it receives, adds its own: 3.5) -> 1 + . (<= 4.5) -> 1 / . (5.5) -> Wd * . (6.5) -> added to the Wp . d term (7.5)
    -> + Wv (8.5) -> + (cl + cm) (9.5), rounded up to 10.  (Wp . d: 1 + 1 + 2 adds + 3 = 7; cl + cm: 2.)"""
    d, v, inv, Wp, Wd, Wv = _pair_terms(pos, uid, Wp, Wd, Wv, F64)
    S = _d(cl).abs()[:, None, :] + _d(cm).abs()[None, :, :] + v * (d.abs() @ Wp.abs().T + inv * Wd.abs() + Wv.abs())
    return SAFETY_DIV * gamma(10) * S


# ------------------------------------------------------------------ pair_gather_add
def pair_gather_add64(ap, zt, a2t, dtype=F64):
    """ap[l, m, :] + zt[a2t[l], a2t[m], :]"""
    a2t = torch.as_tensor(a2t).long()
    return _d(ap, dtype) + _d(zt, dtype)[a2t][:, a2t]


# ------------------------------------------------------------------ pair_init_z
def _rel_pos(ids, dtype=F64):
    return orc.rel_pos_features({"asym_id": torch.as_tensor(ids["asym_id"]).long(), "sym_id": torch.as_tensor(ids["sym_id"]).long(),
                                 "entity_id": torch.as_tensor(ids["entity_id"]).long(),
                                 "residue_index": torch.as_tensor(ids["residue_index"]).long(),
                                 "rel_tok_feat": _d(ids["rel_tok_feat"], dtype)})


def pair_init_z64(si, sj, W, wb, ids, bonds):
    """z[i, j, :] = si[i] + sj[j] + W . rel_pos_features(i, j) + bonds[i, j] wb;  ids: asym_id, sym_id, entity_id, residue_index [T]
    and rel_tok_feat [T, T, 42]"""
    return _d(si)[:, None, :] + _d(sj)[None, :, :] + _rel_pos(ids) @ _d(W).T + _d(bonds)[..., None] * _d(wb).reshape(-1)


def pair_init_z_bound(si, sj, W, wb, ids, bonds):
    """k = 47, no further factor (multiplies and adds only).  The longest chain is the first of the 42 feature products: its own
    rounding (1), the 42 adds that build the RelPos sum on top of the d_res column (42), + the same-entity column (1), + the
    d_chain column (1), + (si + sj) (1), + bonds * wb (1).  (si + sj: 3; bonds * wb: 2.)"""
    S = _d(si).abs()[:, None, :] + _d(sj).abs()[None, :, :] + _rel_pos(ids).abs() @ _d(W).abs().T \
        + _d(bonds).abs()[..., None] * _d(wb).abs().reshape(-1)
    return gamma(47) * S


# ------------------------------------------------------------------ segment_pool
def _token_of_atom(tok_start):
    ts = torch.as_tensor(tok_start).long()
    n = ts[1:] - ts[:-1]
    assert (n >= 0).all()
    return ts, n, torch.repeat_interleave(torch.arange(n.numel()), n)            # atoms ts[0] .. ts[-1] - 1, in order


def _segment_sums(u, tok_start):
    ts, n, tok = _token_of_atom(tok_start)
    body = u[:, int(ts[0]):int(ts[-1])]                                           # atoms outside every token are never read
    return torch.zeros(u.shape[0], n.numel(), u.shape[2], dtype=u.dtype).index_add_(1, tok, body), n


def segment_pool64(u, tok_start, add=None):
    """out[b, t, :] = sum_{atoms of t} u[b, atom, :] / (n_t + 1e-3) [+ add[t, :]],  token t = atoms tok_start[t] .. tok_start[t + 1] - 1"""
    s, n = _segment_sums(_d(u), tok_start)
    out = s / (n.to(F64)[None, :, None] + 1e-3)
    return out if add is None else out + _d(add)[None]


def segment_pool_bound(u, tok_start, add=None):
    """k = n_t + 3, doubled (SAFETY_DIV: a reciprocal and a multiply where the formula divides).  n_t - 1 adds for the sum of n_t
    terms, n_t + 1e-3 (1), the reciprocal (1), the scale (1), the optional add (1).  S = sum |u| / (n_t + 1e-3) [+ |add|]; a token
    without atoms and without add has S = 0: exactly zero is required."""
    s, n = _segment_sums(_d(u).abs(), tok_start)
    S = s / (n.to(F64)[None, :, None] + 1e-3)
    if add is not None:
        S = S + _d(add).abs()[None]
    return SAFETY_DIV * gamma(n.to(F64) + 3)[None, :, None] * S


# ------------------------------------------------------------------ unpool_add, gather_rows_add
def unpool_add64(ba, us, a2t, dtype=F64):
    """ba[b, l, :] + us[b, a2t[l], :]"""
    return _d(ba, dtype) + _d(us, dtype)[:, torch.as_tensor(a2t).long()]


def gather_rows_add64(y, x, idx, dtype=F64):
    """y[r, :] + x[idx[r], :]"""
    return _d(y, dtype) + _d(x, dtype)[torch.as_tensor(idx).long()]


# ------------------------------------------------------------------ axpby
def _axpby_terms(a, sa, b, sb_ptr, sb):
    ta = _d(a) * float(sa)
    if b is None:
        return ta, torch.zeros_like(ta)
    scale = float(sb) if sb_ptr is None else float(_d(sb_ptr).reshape(-1)[0]) * float(sb)
    return ta, _d(b) * scale


def axpby64(a, sa, b=None, sb_ptr=None, sb=1.0):
    """a sa [+ b (sb_ptr[0] sb)]  (sb_ptr None: b sb)"""
    ta, tb = _axpby_terms(a, sa, b, sb_ptr, sb)
    return ta + tb


def axpby_bound(a, sa, b=None, sb_ptr=None, sb=1.0):
    """k = 3, no further factor.  The b term: sb_ptr[0] * sb (1), b * . (1), the add (1).  (The a term: 2.)"""
    ta, tb = _axpby_terms(a, sa, b, sb_ptr, sb)
    return gamma(3) * (ta.abs() + tb.abs())


# ------------------------------------------------------------------ template_mask
def template_mask64(z_mask, templ_feat, asym, dtype=F64):
    """mask2d[i, j] = z_mask[i, j] * templ_feat[i, j, D - 1] * [asym_i == asym_j]"""
    asym = torch.as_tensor(asym)
    same = (asym[:, None] == asym[None, :]).to(dtype)
    return _d(z_mask, dtype) * _d(templ_feat, dtype)[..., -1] * same
