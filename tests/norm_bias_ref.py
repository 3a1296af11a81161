"""Plain float64 references of the row-norm kernels (physdock_amd/csrc/norm.hip: pd_rowstats, pd_rownorm, pd_norm_split,
pd_norm_split2) and of the pair-bias kernels (csrc/pairbias.hip: pd_pair_bias, pd_pair_bias_split), the rounding bounds their tests
use, the two fragment address maps and the operand splits in exact torch.

torch on the CPU, no device code.  Every function transcribes the formula in the comment above its kernel (or in
include/physdock_hip.h) as whole-tensor algebra; none of them follows a kernel's loop structure.  gamma, bound_ratio and
assert_within_bound are those of tests/trunk_glue_ref.py; the conventions are the ones stated there: a bound is gamma_k * S with S
the float64 sum of the absolute values that enter the element and k the fp32 roundings on the longest chain, counted in the
function's comment; SAFETY_DIV doubles a bound whose formula holds a division or rsqrtf.  Two things are particular to this file:

* sums over a row are bounded for ANY summation order: n terms cost n - 1 roundings (the worst, serial, chain), so the bound holds
  for the lanes-then-shuffles order of rownorm_kernel, the DPP tree of pair_bias_kernel, the serial loop of colstats_kernel and
  whatever order torch's CPU kernels choose.
* the errors of the row statistics are propagated: with dm >= |mean^ - mean| and dr >= |rstd^ - rstd| the normalised value
  (x - mean) rstd is off by at most (dm + u a) R + a dr + u a R, a = |x - mean| + dm >= |x - mean^|, R = rstd + dr >= rstd^
  (subtraction error, error of rstd, rounding of the product).  The variance sees the mean's error only in second order:
  sum (x - mean^)^2 = sum (x - mean)^2 + C (mean^ - mean)^2 exactly, since the first-order term sums to zero.  For a row far from the
  origin (|mean| / std >= 1e4) and a wide C that second-order term is no longer small against the variance: the bound then
  degrades to the trivial 0 <= rstd^ <= eps^-1/2 - the honest statement about a row that fp32 cannot centre, and the reason the
  narrow-C cases are the ones that tell a one-pass variance from the two-pass one.

Nothing here is tuned on a kernel's output.
"""
import math

import torch

from trunk_glue_ref import F64, SAFETY_DIV, U32, assert_within_bound, bound_ratio, gamma  # noqa: F401 (re-exported to the tests)

RMS, LN = 0, 1
ACT_NONE, ACT_SILU, ACT_SIGMOID, ACT_RELU = 0, 1, 2, 3
F32 = torch.float32


def _d(t, dtype=F64):
    return None if t is None else torch.as_tensor(t).to(dtype)


# ------------------------------------------------------------------ pd_rowstats
def rowstats64(x, mode, eps, dtype=F64):
    """RMS: (0, rsqrt(mean(x^2) + eps));  LN: (mean(x), rsqrt(mean((x - mean)^2) + eps)), over the last axis"""
    x = _d(x, dtype)
    if mode == RMS:
        mean = torch.zeros(x.shape[:-1], dtype=dtype)
        var = (x * x).mean(-1)
    else:
        mean = x.mean(-1)
        var = ((x - mean[..., None]) ** 2).mean(-1)
    return mean, torch.rsqrt(var + eps)


def _stat_err(x, mode, eps):
    """(mean, rstd, dm, dr): the float64 statistics and the bounds of their fp32 evaluation.

    mean: C - 1 adds and the division, k = C, doubled (SAFETY_DIV), S = mean |x|; RMS: exactly 0.
    variance: RMS  x^2 (1), C - 1 adds, the division: k = C + 1 on v = mean x^2 (all terms positive: S = v);
              LN   x - mean^ (1) -> squared (2 * 1 + 1 = 3) -> C - 1 adds -> the division: k = C + 3 on v + dm^2, plus dm^2 itself.
    t = v + eps: one more rounding of t.  rstd = rsqrtf(t): the relative error r = dt / t of t becomes (1 - r)^-1/2 - 1 (exact, not
    first order; the function is convex), times the one rounding of rsqrtf, doubled (SAFETY_DIV: rsqrtf is good to an ulp, not half).
    Where r >= 1/2 the chain says nothing any more and the bound is that of 0 <= rstd^ <= eps^-1/2 (v^ >= 0 always)."""
    x = _d(x)
    C = x.shape[-1]
    mean, rstd = rowstats64(x, mode, eps)
    if mode == RMS:
        dm = torch.zeros_like(mean)
        var = (x * x).mean(-1)
        dv = gamma(C + 1) * var
    else:
        dm = SAFETY_DIV * gamma(C) * x.abs().mean(-1)
        var = ((x - mean[..., None]) ** 2).mean(-1)
        dv = gamma(C + 3) * (var + dm * dm) + dm * dm
    t = var + eps
    dt = dv + U32 * (var + dv + eps)
    r = dt / t
    chain = SAFETY_DIV * rstd * ((1 - r.clamp(max=0.5)).rsqrt() * (1 + U32) - 1)
    trivial = torch.full_like(rstd, (1 + 4 * U32) / math.sqrt(eps)) if eps > 0 else torch.full_like(rstd, float("inf"))
    dr = torch.where(r < 0.5, torch.minimum(chain, trivial), trivial)
    return mean, rstd, dm, dr


def rowstats_bound(x, mode, eps):
    """(bound of mean, bound of rstd), see _stat_err"""
    _, _, dm, dr = _stat_err(x, mode, eps)
    return dm, dr


def _xhat_err(x, mode, eps):
    """(xhat, a, R, E): xhat = (x - mean) rstd in float64, a >= |x - mean^|, R >= rstd^ and E >= |xhat^ - xhat| (module docstring)"""
    x = _d(x)
    mean, rstd, dm, dr = (t[..., None] for t in _stat_err(x, mode, eps))
    a = (x - mean).abs() + dm
    R = rstd + dr
    return (x - mean) * rstd, a, R, (dm + U32 * a) * R + a * dr + U32 * a * R


# ------------------------------------------------------------------ pd_rownorm
def _act64(t, act):
    if act == ACT_SILU:
        return t * torch.sigmoid(t)
    if act == ACT_SIGMOID:
        return torch.sigmoid(t)
    if act == ACT_RELU:
        return torch.relu(t)
    return t


def rownorm64(x, res, w, b, mode, eps, act, dtype=F64):
    """y = [res +] act(((x - mean) rstd) [* w] [+ b])"""
    x = _d(x, dtype)
    mean, rstd = rowstats64(x, mode, eps, dtype)
    t = (x - mean[..., None]) * rstd[..., None]
    if w is not None:
        t = t * _d(w, dtype)
    if b is not None:
        t = t + _d(b, dtype)
    t = _act64(t, act)
    return t if res is None else t + _d(res, dtype)


def _mod_err(x, w, b, mode, eps):
    """(t, E) of t = xhat w + b (w, b broadcast against x; None: 1 / 0): the error of xhat times |w|, the rounding of the product
    and of the add (k = 2 on |xhat^ w|, 1 on |b|)"""
    xhat, a, R, E = _xhat_err(x, mode, eps)
    w = torch.ones(()).to(F64) if w is None else _d(w)
    b = torch.zeros(()).to(F64) if b is None else _d(b)
    return xhat * w + b, E * w.abs() + gamma(2) * a * R * w.abs() + U32 * b.abs()


def rownorm_bound(x, res, w, b, mode, eps, act):
    """The chain of _mod_err, then the activation, then the residual add (1 rounding on |act| + |res|).
    relu: 1-Lipschitz, exact.  sigmoid s = 1 / (1 + e), e = __expf(-t) = exp2(-t log2 e): the exponent carries two roundings (the
    constant, the product) of size u |t| log2 e, which is 2 |t| u relative on e, + 1 for exp2: (2 |t| + 1) u on e, passed on with
    ds/de e = s (1 - s); the add and the division: 2 more on s; 1/4-Lipschitz in t.  silu = t / (1 + e): the same count relative to
    |silu|; its derivative stays below 1.1.  The own error of both is doubled (SAFETY_DIV: a division, exp2 good to an ulp)."""
    t, E = _mod_err(x, w, b, mode, eps)
    at = t.abs() + E
    s = torch.sigmoid(t)
    own = SAFETY_DIV * U32 * ((1 - s) * (2 * at + 1) + 2)
    if act == ACT_SIGMOID:
        E = 0.25 * E + own * s
    elif act == ACT_SILU:
        E = 1.1 * E + own * at * s
    y = _act64(t, act)
    if res is not None:
        E = E + U32 * (y.abs() + E + _d(res).abs())
    return E


# ------------------------------------------------------------------ pd_norm_split / pd_norm_split2
def _group_rows(tab, M, rows_per_group):
    if tab is None:
        return None
    tab = _d(tab)
    g = torch.arange(M) // rows_per_group if rows_per_group > 0 else torch.zeros(M, dtype=torch.long)
    return tab.reshape(-1, tab.shape[-1])[g]


def norm_mod64(x, w_tab, b_tab, rows_per_group, mode, eps, dtype=F64):
    """a'[m, :] = (x[m] - mean_m) rstd_m w[g] + b[g],  g = m // rows_per_group (0: row 0 for all; None: 1 / 0);  w_tab, b_tab [G, C]"""
    x = _d(x, dtype)
    M = x.shape[0]
    mean, rstd = rowstats64(x, mode, eps, dtype)
    t = (x - mean[:, None]) * rstd[:, None]
    w, b = _group_rows(w_tab, M, rows_per_group), _group_rows(b_tab, M, rows_per_group)
    if w is not None:
        t = t * w.to(dtype)
    return t if b is None else t + b.to(dtype)


def norm_mod_bound(x, w_tab, b_tab, rows_per_group, mode, eps):
    """_mod_err with the gain and shift row of each row's group.  The three bf16 parts add up to the fp32 value exactly and the
    power-of-two operand scale is exact, so this is also the bound of the sum of the parts (split 2: + split2_bound)."""
    M = _d(x).shape[0]
    return _mod_err(x, _group_rows(w_tab, M, rows_per_group), _group_rows(b_tab, M, rows_per_group), mode, eps)[1]


# ------------------------------------------------------------------ the splits in exact torch
def split3_bf16(a):
    """h = bf16(a), m = bf16(a - h), l = bf16(a - h - m) (round to nearest even, then subtract, twice); fp32 in, three fp32 out"""
    a = torch.as_tensor(a, dtype=F32)
    h = a.to(torch.bfloat16).to(F32)
    r = a - h
    m = r.to(torch.bfloat16).to(F32)
    return h, m, (r - m).to(torch.bfloat16).to(F32)


def split2_f16(a):
    """h = fp16(a), l = fp16(a - h); fp32 in, two fp32 out"""
    a = torch.as_tensor(a, dtype=F32)
    h = a.to(torch.float16).to(F32)
    return h, (a - h).to(torch.float16).to(F32)


def split2_bound(v):
    """|h + l - a| for |a| <= v < 65504: a - h is exact in fp32 and at most half an fp16 ulp of a, 2^-11 2^e for a in [2^e, 2^(e+1));
    l rounds it with relative error 2^-11, or absolute error 2^-25 where it is subnormal in fp16 (spacing 2^-24):
    2^-25 max(1, 2^(e+3)) - the binade of a is the scale of the 2^-25."""
    v = _d(v).abs()
    e = torch.frexp(v.clamp(min=2.0 ** -30))[1] - 1
    return 2.0 ** -25 * torch.ldexp(torch.ones_like(v), (e + 3).clamp(min=0))


def pow2_scale(amax):
    """2^(14 - floor(log2 amax)) of the fp32 value amax: amax * scale in [2^14, 2^15).  The exponent floor(log2 amax) is clamped to
    [87 - 127, 200 - 127] as pd_pow2_scale clamps the biased exponent, so the scale stays within [2^-59, 2^54]."""
    a = float(torch.tensor(float(amax), dtype=F32))
    fl = math.frexp(a)[1] - 1 if a > 0 else -1000
    return 2.0 ** (14 - min(max(fl, 87 - 127), 200 - 127))


_FORMATS = {"bf16": (8, -126), "fp16": (11, -14)}          # significand bits with the hidden one, smallest normal exponent


def _ulp(y, fmt):
    p, emin = _FORMATS[fmt]
    e = (torch.frexp(y.abs().clamp(min=2.0 ** -200))[1] - 1).clamp(min=emin)
    return torch.ldexp(torch.ones_like(y), e - p + 1)


def round_to(y64, fmt):
    """the float64 tensor rounded to the nearest bf16 / fp16 number, ties to even, without a detour over fp32"""
    y64 = _d(y64)
    ulp = _ulp(y64, fmt)
    return torch.round(y64 / ulp) * ulp


def assert_high_part(kernel, case, hi, y64, E, fmt):
    """the high part of a split is the correctly rounded bf16 / fp16 value of the float64 result or a neighbour of it, and where it is
    the neighbour the float64 result lies within the fp32 evaluation bound E of the rounding boundary between the two.  Stated for
    any E: the interval of reals that round to `hi` holds a point within E of the float64 result (the kernel rounds its own fp32
    value, which is such a point); where E is below half a step that allows the nearest value and, next to a boundary, one neighbour."""
    hi, y64, E = _d(hi), _d(y64), _d(E)
    assert torch.isfinite(hi).all(), (kernel, case)
    nearest = round_to(y64, fmt)
    off = hi != nearest
    print(f"HIGH | {kernel} | {case} | {int(off.sum())} of {off.numel()} high parts differ from the nearest {fmt} value")
    if off.any():
        mag = hi.abs()
        up, down = mag + _ulp(mag, fmt) / 2, mag - _ulp(mag * (1 - 2.0 ** -20), fmt) / 2      # a power of two has the finer spacing below it
        sign = torch.where(hi < 0, -1.0, 1.0).to(F64)
        lo_edge, hi_edge = torch.minimum(sign * down, sign * up), torch.maximum(sign * down, sign * up)
        closest = torch.minimum(torch.maximum(y64, lo_edge), hi_edge)
        assert_within_bound(kernel + " (rounding boundary)", case, closest[off], y64[off], E[off])
        sharp = off & (E < _ulp(nearest, fmt) / 4)
        step = _ulp(torch.maximum(mag, nearest.abs()), fmt)
        assert bool(((hi - nearest).abs() <= step)[sharp].all()), (kernel, case, "high part is no neighbour of the rounded value")


# ------------------------------------------------------------------ pd_pair_bias
def _madd(mask, maskval, M):
    if mask is None:
        return torch.zeros(M, 1, dtype=F64)
    return torch.where(torch.as_tensor(mask).reshape(M, 1) == 0, float(maskval), 0.0).to(F64)


def _dense(rows, T1, T2, transpose):
    """[T1 * T2, H] -> [H, nq, nk]: row m = (i, j) = (m // T2, m % T2) is query i, key j; with `transpose` query j, key i"""
    d = rows.reshape(T1, T2, -1).permute(2, 0, 1)
    return d.transpose(1, 2) if transpose else d


def pair_bias64(x, Wf, c2, mask, maskval, out_scale, T1, T2, transpose, mode, eps, dtype=F64):
    """[H, nq, nk] of ((xhat . Wf_h + c2_h) + madd) out_scale, xhat = (x - mean) rstd, madd = maskval where mask == 0 (None: 0),
    out_scale 0 meaning 1"""
    x = _d(x, dtype)
    mean, rstd = rowstats64(x, mode, eps, dtype)
    p = ((x - mean[:, None]) * rstd[:, None]) @ _d(Wf, dtype).T
    if c2 is not None:
        p = p + _d(c2, dtype)
    s = float(out_scale) if out_scale != 0 else 1.0
    return _dense((p + _madd(mask, maskval, x.shape[0]).to(dtype)) * s, T1, T2, transpose)


def pair_bias_bound(x, Wf, c2, mask, maskval, out_scale, T1, T2, transpose, mode, eps):
    """The kernel contracts x - mean^ with Wf and scales by rstd^ afterwards.  Contraction over C: the subtraction (1), the product
    (1), C - 1 adds: k = C + 1 on D = sum_k a_k |Wf_hk|, plus the error of the mean on every term, dm sum_k |Wf_hk|.  Times rstd^:
    that error times R, D dr for the error of rstd, 1 rounding.  Then + c2, + madd, * out_scale: with the product by rstd^ k = 4 on
    D R + |c2| + |madd| - this is where |maskval| enters S."""
    x, Wf = _d(x), _d(Wf)
    C = x.shape[-1]
    _, a, R, _ = _xhat_err(x, mode, eps)
    _, _, dm, dr = (t[:, None] for t in _stat_err(x, mode, eps))
    D = a @ Wf.abs().T
    Ed = gamma(C + 1) * D + dm * Wf.abs().sum(-1)
    c2a = torch.zeros(Wf.shape[0], dtype=F64) if c2 is None else _d(c2).abs()
    s = abs(float(out_scale)) if out_scale != 0 else 1.0
    E = (Ed * R + D * dr + gamma(4) * (D * R + c2a + _madd(mask, maskval, x.shape[0]).abs())) * s
    return _dense(E, T1, T2, transpose)


def z2_ref64(x, eps, scale, T, transpose):
    """[batch, row, C] of x / rms(x) * scale for x [T * T, C]: batch, row = the pair indices (i, j), swapped with `transpose`"""
    xhat, _, _, _ = _xhat_err(x, RMS, eps)
    z = (xhat * scale).reshape(T, T, -1)
    return z.transpose(0, 1) if transpose else z


def z2_bound(x, eps, scale, T, transpose):
    """x * (rstd^ scale): the scale is a power of two (exact), so a dr for the error of rstd and 1 rounding of the product; then the
    two-part split of the result (split2_bound)"""
    xhat, a, R, _ = _xhat_err(x, RMS, eps)
    E = (a * _stat_err(x, RMS, eps)[3][:, None] + U32 * a * R) * scale
    E = (E + split2_bound(xhat.abs() * scale + E)).reshape(T, T, -1)
    return E.transpose(0, 1) if transpose else E


# ------------------------------------------------------------------ the two fragment address maps
def bias_frag_numel(H, nq, nk):
    return H * ((nq + 31) // 32) * ((nk + 31) // 32) * 1024


def bias_frag_index(H, nq, nk):
    """float index of bias[h, q, k] in the attention kernel's fragment layout: 32 x 32 tiles, [h][q tile][k tile] of 1024 floats;
    inside a tile, with q5 = q % 32 and k5 = k % 32 = 8 g + 4 hh + e:  g * 256 + (q5 + 32 * hh) * 4 + e"""
    h = torch.arange(H)[:, None, None]
    q = torch.arange(nq)[None, :, None]
    k = torch.arange(nk)[None, None, :]
    nqt, nkt = (nq + 31) // 32, (nk + 31) // 32
    q5, k5 = q % 32, k % 32
    g, hh, e = k5 // 8, (k5 // 4) % 2, k5 % 4
    return ((h * nqt + q // 32) * nkt + k // 32) * 1024 + g * 256 + (q5 + 32 * hh) * 4 + e


def bias_frag_scatter(dense, fill=float("nan")):
    """(fragment buffer holding `dense` [H, nq, nk] with `fill` in the pad slots, boolean mask of the real slots)"""
    H, nq, nk = dense.shape
    idx = bias_frag_index(H, nq, nk).reshape(-1)
    frag = torch.full((bias_frag_numel(H, nq, nk),), fill, dtype=dense.dtype)
    frag[idx] = dense.reshape(-1)
    real = torch.zeros(frag.numel(), dtype=torch.bool)
    real[idx] = True
    return frag, real


Z2_C = 128


def z2_numel(T):
    return T * ((T + 31) // 32) * 8 * 2 * 64 * 8


def z2_index(T):
    """half index of the HIGH part of z2[batch b, row r, channel c]: [b][32-row tile][k-step s = c // 16][part][lane'][8 halves] with
    lane' = r % 32 + 32 hh, hh = (c % 16) // 8, and c % 8 the position among the 8 halves; the low part lies 64 * 8 halves on"""
    b = torch.arange(T)[:, None, None]
    r = torch.arange(T)[None, :, None]
    c = torch.arange(Z2_C)[None, None, :]
    nt = (T + 31) // 32
    s, hh, j = c // 16, (c % 16) // 8, c % 8
    return ((((b * nt + r // 32) * 8 + s) * 2 + 0) * 64 + (r % 32 + 32 * hh)) * 8 + j


def z2_real(T):
    real = torch.zeros(z2_numel(T), dtype=torch.bool)
    idx = z2_index(T).reshape(-1)
    real[idx] = True
    real[idx + 512] = True
    return real


def z2_scatter(hi, lo, fill):
    """fp16 buffer holding the parts hi, lo [T, T, 128] (batch, row, channel), `fill` (an fp16 tensor scalar) in the other slots"""
    T = hi.shape[0]
    idx = z2_index(T).reshape(-1)
    buf = torch.full((z2_numel(T),), 0, dtype=torch.float16)
    buf[:] = fill
    buf[idx] = hi.reshape(-1).to(torch.float16)
    buf[idx + 512] = lo.reshape(-1).to(torch.float16)
    return buf


def z2_gather(buf, T):
    """(hi, lo) [T, T, 128] float64 of an fp16 buffer in the z2 layout"""
    idx = z2_index(T)
    return buf[idx].to(F64), buf[idx + 512].to(F64)
