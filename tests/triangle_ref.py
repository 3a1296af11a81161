"""Plain float64 references of the triangle kernels (physdock_amd/csrc/tri_mul.hip: pd_tri_mul; csrc/tri_tail.hip: pd_tri_tail,
modes 0 and 1; csrc/tri_attn.hip: pd_tri_attention), the derived per-element bounds their kernel-level tests use, and the cached cases of those tests.

torch on the CPU, no device code.  The references transcribe the formulas of include/physdock_hip.h as whole-tensor algebra; none of
them follows a kernel's loop structure.  Built on tests/norm_bias_ref.py (gamma, split2_bound, pow2_scale, _stat_err and the comparison
assert_within_bound) with the conventions stated there: a bound is a sum of terms, each a rounding count times the float64 sum of the
absolute values that enter the element.  Terms particular to the two-part fp16 operand format (common.h pd_split2h, pd_pow2_scale):

* operand rounding: an fp32 value v is multiplied by a power of two s (exact) and split, h = fp16(v s), l = fp16(v s - h); |h + l - v s| <=
  split2_bound(v s), so the operand the MFMAs see is off by split2_bound(s v) / s.  Where v itself carries an evaluation error dv (the
  normalised rows of pd_tri_tail) the operand is off by dv + split2_bound(s (|v| + dv)) / s.
* the dropped low x low product: the kernels form h h' + h l' + l h'.  |l| <= 2^-11 |v s| + 2^-25 (half an fp16 ulp of the high part, or half
  the subnormal spacing 2^-24), with one more fp16 rounding of its own: (1 + 2^-10) covers it.
* accumulation: K products go through K / 16 steps of v_mfma_f32_32x32x16_f16, three instructions per step.  Assumed of the instruction:
  what the CDNA programming guide states of the fp32-input MFMA (section "FP32-input MFMA", Numerics: a chain of additions, one fp32
  rounding each, no wider internal accumulation) - the worst case for an error bound; a wider internal sum only lowers the error.  Per
  step: 15 additions inside the high x high instruction and its addition to the accumulator (16), the additions of the two cross
  instructions to the accumulator (2; their internal roundings act on sums 2^-11 as large: 1 more covers them): MMA_STEP = 19 roundings
  per 16 products.  The steps run in the order of k, so a product of step s of S meets the roundings of steps s .. S - 1 only: it is
  weighted with gamma(19 (S - s)), against |a| |b| of the operands as rounded.  A step whose products are all zero (the padded j of
  pd_tri_mul's last slice) adds zeros, exactly: K counts the real products.
* rsqrtf and __expf: the two hardware figures.  Neither guide states the accuracy of v_rsq_f32 or v_exp_f32, so both were measured on an
  MI355X against float64 (2^31 arguments each; NOTES.md "Triangle kernel tests"): v_rsq_f32 and rsqrtf 1.58 u over 2^[-40, 60], v_exp_f32
  1.43 u over [-120, 15], u = 2^-24.  The constants carry a factor 2 (one run samples the function sparsely): RSQ_REL = 3.2, EXP2_REL = 2.9.

Nothing here is tuned on a kernel's output.
"""
import functools
import math

import torch

import norm_bias_ref as nb
from norm_bias_ref import F32, F64, RMS, SAFETY_DIV, U32, assert_within_bound, bound_ratio, gamma, pow2_scale, split2_bound  # noqa: F401

MMA_STEP = 19                 # fp32 roundings per 16-wide MFMA step of the three-product scheme (module docstring)
RSQ_REL = 3.2                 # relative error of rsqrtf in units of u: 2 x the measured 1.58
EXP2_REL = 2.9                # relative error of v_exp_f32 in units of u: 2 x the measured 1.43
NAN = float("nan")


def _d(t):
    return None if t is None else torch.as_tensor(t).to(F64)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f32(x):
    """the float the C ABI receives"""
    return float(torch.tensor(float(x), dtype=F32))


def _lo_bound(vs):
    """bound of |l| for the low part of a split of the scaled value |v s| <= vs (module docstring)"""
    return torch.where(vs > 0, (2.0 ** -11 * vs + 2.0 ** -25) * (1 + 2.0 ** -10), torch.zeros_like(vs))


def _split_err(vs):
    """nb.split2_bound of the scaled magnitude vs; an operand that is exactly zero splits into two zeros"""
    return torch.where(vs > 0, split2_bound(vs), torch.zeros_like(vs))


def _mma_err(A, dA, sA, B, dB, sB, K, exactA=False):
    """bound of the error of sum_k A[.., m, k] B[.., n, k] on the two-part fp16 format: A, B float64 values [.., M, K] / [.., N, K], dA, dB
    bounds of their fp32 evaluation before the split (0: the fp32 operand is exact), sA, sB their power-of-two scales (numbers or
    per-row columns).  Terms in the order of the module docstring: operand rounding (first order and the cross term), the dropped
    low x low product, the accumulation.  exactA: A IS the sum of two given fp16 parts over sA (the z2 operand of pd_tri_attention)."""
    Aa, Ba = A.abs() + dA, B.abs() + dB
    eA = dA + (torch.zeros_like(Aa) if exactA else _split_err(Aa * sA) / sA)
    eB = dB + _split_err(Ba * sB) / sB
    T_ = lambda t: t.transpose(-1, -2)
    operand = eA @ T_(B.abs()) + A.abs() @ T_(eB) + eA @ T_(eB)
    lowlow = (_lo_bound(Aa * sA) / sA) @ T_(_lo_bound(Ba * sB) / sB)
    Ar, Br, S = Aa + eA, Ba + eB, (K + 15) // 16
    accum = 0.0
    for s in range(S):                      # the steps run in the order of k: a product of step s meets the roundings of steps s .. S - 1
        sl = slice(16 * s, 16 * s + 16)
        accum = accum + gamma(MMA_STEP * (S - s)) * (Ar[..., sl] @ T_(Br[..., sl]))
    return operand + lowlow + accum


# ================================================================== pd_tri_mul
def _tri_mul_operands(q, k, Treal, transpose):
    """(A, B): the rows of A are the output rows, those of B the output columns, the last axis the reduction index j < Treal"""
    q, k = _d(q), _d(k)
    if transpose:
        return k[:, :Treal].transpose(1, 2), q[:, :Treal].transpose(1, 2)
    return q[:, :, :Treal], k[:, :, :Treal]


def tri_mul64(q, k, Treal, transpose):
    """transpose == 0:  o[c, i, I] = sum_{j < Treal} q[c, i, j] k[c, I, j];  transpose == 1:  o[c, a, b] = sum_{j < Treal} k[c, j, a] q[c, j, b];
    q, k [nch, T, T]; entries whose reduction index is >= Treal are never read"""
    A, B = _tri_mul_operands(q, k, Treal, transpose)
    return A @ B.transpose(1, 2)


def tri_mul_bound(q, k, Treal, transpose, q_amax, k_amax):
    """_mma_err over K = Treal products (the kernel runs whole 32-slices with the padded j as zeros, which add exactly) with exact fp32
    operands scaled by pow2_scale of their bounds, + 1 rounding of the result: acc * 1 / (sa sb) is exact unless it underflows"""
    A, B = _tri_mul_operands(q, k, Treal, transpose)
    sq, sk = pow2_scale(q_amax), pow2_scale(k_amax)
    sA, sB = (sk, sq) if transpose else (sq, sk)
    return _mma_err(A, 0.0, sA, B, 0.0, sB, Treal) + U32 * (A @ B.transpose(1, 2)).abs()


def _parts(v, s, low=True):
    """the operand the MFMAs see, in float64: both fp16 parts of the fp32 product v s (exact torch), or the high part alone"""
    h, l = nb.split2_f16(torch.as_tensor(v, dtype=F32) * s)
    return h.to(F64), (l.to(F64) if low else torch.zeros_like(h, dtype=F64))


def tri_mul_emulated(q, k, Treal, transpose, q_amax, k_amax, low=True, extra_j=0):
    """the kernel's arithmetic with exact accumulation: h h' + h l' + l h' of the split operands.  low = False: a kernel that drops the low
    parts; extra_j = 1: a kernel whose reduction includes index Treal"""
    A, B = _tri_mul_operands(q, k, min(Treal + extra_j, q.shape[-1]), transpose)
    sq, sk = pow2_scale(q_amax), pow2_scale(k_amax)
    sA, sB = (sk, sq) if transpose else (sq, sk)
    (ah, al), (bh, bl) = _parts(A, sA, low), _parts(B, sB, low)
    T_ = lambda t: t.transpose(1, 2)
    return (ah @ T_(bh) + ah @ T_(bl) + al @ T_(bh)) / (sA * sB)


TRI_MUL_SHAPES = [(4, 1), (4, 4), (36, 33), (36, 34), (36, 35), (64, 63), (64, 64), (100, 97), (132, 129)]      # (T, Treal)
TRI_MUL_NCH = [1, 3, 5, 32]
ZERO_PLANE, AMAX_PLANE = 1, 2          # planes of q with special content, where nch allows


@functools.lru_cache(maxsize=None)
def tri_mul_case(T, nch):
    """(q, k, max|q|, max|k|): [nch, T, T] operands randn; one operand of every plane carries the wide factor exp(1.5 randn) per element
    (q in the even planes, k in the odd ones); plane 1 of q all zero, plane 2 with |q| = max|q| everywhere.  All entries finite: a test poisons the entries its form must not read."""
    g = gen(1000 * T + nch)
    wide = [torch.exp(1.5 * torch.randn(nch, T, T, generator=g)) for _ in range(2)]
    even = (torch.arange(nch) % 2 == 0)[:, None, None]
    # the wide factor sits on q in the even planes and on k in the odd ones: on both operands of one plane the largest of the T^3 products
    # is e^10 times the typical one, and no bound of the accumulation stays below 1e-3 of the mean |o| (test_triangle_ref_cpu.py)
    q = torch.randn(nch, T, T, generator=g) * torch.where(even, wide[0], torch.ones(()))
    k = torch.randn(nch, T, T, generator=g) * torch.where(even, torch.ones(()), wide[1])
    qa, ka = float(q.abs().max()), float(k.abs().max())
    if nch > ZERO_PLANE:
        q[ZERO_PLANE] = 0
    if nch > AMAX_PLANE:
        # signs that depend on the last index alone, the same on q and on k of this plane: every product of a sum has one sign in either
        # form, so |o| = sum |q| |k| there and the plane's bound - the largest of the case, q sits at the top of its range - is gamma-small
        # against the plane's own outputs, which carry the case's mean |o| (the non-vacuity condition of test_triangle_ref_cpu.py)
        sgn = (1 - 2 * (torch.rand(T, generator=g) < 0.5).float())[None, :]
        q[AMAX_PLANE] = qa * sgn
        k[AMAX_PLANE] = k[AMAX_PLANE].abs() * sgn
    return q, k, qa, ka


def tri_mul_poisoned(x, Treal, transpose):
    """x with NaN wherever the reduction index is >= Treal: the last axis in the row form, the first in the column form"""
    x = x.clone()
    if transpose:
        x[:, Treal:, :] = NAN
    else:
        x[:, :, Treal:] = NAN
    return x


@functools.lru_cache(maxsize=None)
def tri_mul_expected(T, Treal, nch, transpose, loose):
    """(reference, bound, q_amax, k_amax): the bounds given tight (the exact maxima) or loose (x 1000)"""
    q, k, qa, ka = tri_mul_case(T, nch)
    f = 1000.0 if loose else 1.0
    qa, ka = f32(qa * f), f32(ka * f)
    return tri_mul64(q, k, Treal, transpose), tri_mul_bound(q, k, Treal, transpose, qa, ka), qa, ka


# ================================================================== pd_tri_tail
C_, CO = 128, 32
TAIL_EPS = f32(1e-8)
BM = 64                                  # rows per block tile of tri_tail_kernel
TAIL_SMALL_M = [1, 3, 63, 64, 65, 100, 129]
TAIL_GRID_M = {0: 768 * 64 + 64 + 5, 1: 512 * 64 + 64 + 5}      # one full and one partial tile past the launch's grid


def w_row_scale(W, rows_per_scale=1):
    """the per-row power of two of packing.split2_f16: max_k |W[n, k]| scale[n] in [2^14, 2^15); rows of zeros: 1"""
    amax = torch.as_tensor(W, dtype=F32).abs().amax(1)
    if rows_per_scale > 1:
        amax = amax.reshape(-1, rows_per_scale).amax(1, keepdim=True).expand(-1, rows_per_scale).reshape(-1)
    e = torch.frexp(amax)[1]
    return torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), 15 - e), torch.ones_like(amax)).to(F64)


def _norm_rows(x, w, eps):
    """(t, E): t = x / rms(x) * w in float64 and the bound of its fp32 evaluation x * rstd^ * w.  nb._mod_err (statistics of any
    summation order, the product by rstd^ and by w: 2 roundings) with the error of rstd topped up from the 2 u nb._stat_err allows
    rsqrtf to the measured RSQ_REL u."""
    t, E = nb._mod_err(x, w, None, RMS, eps)
    _, a, R, _ = nb._xhat_err(x, RMS, eps)
    return t, E + max(RSQ_REL - 2.0, 0.0) * U32 * a * R * _d(w).abs()


def tri_tail64(mode, z, o, w_in, w_out, Wg, bg, Wz, bz, eps=TAIL_EPS):
    """mode 0: z[m] + sigmoid(W_g RMSNorm(z[m]) w_in + b_g) * (W_z RMSNorm(o[:, m]) w_out + b_z), o [Co, M];
    mode 1: z[m] + (W_g RMSNorm(z[m]) w_in + b_g) * (W_z o[m] + b_z), o [M, C].  bg / bz None: 0.  Returns (result, update)."""
    z = _d(z)
    zn = z * torch.rsqrt((z * z).mean(-1, keepdim=True) + eps) * _d(w_in)
    gl = zn @ _d(Wg).T + (0 if bg is None else _d(bg))
    if mode == 0:
        ot = _d(o).T
        b = ot * torch.rsqrt((ot * ot).mean(-1, keepdim=True) + eps) * _d(w_out)
        gate = torch.sigmoid(gl)
    else:
        b, gate = _d(o), gl
    upd = gate * (b @ _d(Wz).T + (0 if bz is None else _d(bz)))
    return z + upd, upd


def tri_tail_bound(mode, z, o, w_in, w_out, Wg, bg, Wz, bz, zn_amax, on_amax, eps=TAIL_EPS):
    """gate logits: _mma_err over K = 128 of the normalised rows (error of the statistics and of the two products: _norm_rows) against
    W_g split per row, then acc * (wg_inv / z_s) (powers of two: exact) + b_g: 1 rounding.  Second contraction: the same over K = 32 with the
    normalised columns of o (mode 0), over K = 128 with the exact fp32 rows of o (mode 1); + b_z: 1 rounding.
    sigmoid s = 1 / (1 + __expf(-t)) (mode 0): 1/4-Lipschitz in t; own error as nb.rownorm_bound counts it with the measured exp2:
    the exponent -t log2 e carries two roundings of size u |t| log2 e (2 |t| u relative on e), + EXP2_REL for v_exp_f32, passed on with
    ds/de e = s (1 - s); the addition 1 and the division 2 (an IEEE division or v_rcp_f32, good to an ulp) more on s.
    z + gate * update: the errors of both factors to first order with the cross term, 1 rounding of the product, 1 of the sum."""
    z, Wg, Wz = _d(z), _d(Wg), _d(Wz)
    zs, os_ = pow2_scale(zn_amax), pow2_scale(on_amax)
    zn, dzn = _norm_rows(z, w_in, eps)
    gl = zn @ Wg.T
    Egl = _mma_err(zn, dzn, zs, Wg, 0.0, w_row_scale(Wg)[:, None], C_)
    bga = 0.0 if bg is None else _d(bg).abs()
    gl_full = gl + (0 if bg is None else _d(bg))
    Egl = Egl + U32 * (gl.abs() + Egl + bga)
    if mode == 0:
        b, db = _norm_rows(_d(o).T, w_out, eps)
        s = torch.sigmoid(gl_full)
        at = gl_full.abs() + Egl
        gate, Eg = s, 0.25 * Egl + U32 * ((1 - s) * (2 * at + EXP2_REL) + 3) * s
    else:
        b, db = _d(o), 0.0
        gate, Eg = gl_full, Egl
    up = b @ Wz.T
    Eup = _mma_err(b, db, os_, Wz, 0.0, w_row_scale(Wz)[:, None], Wz.shape[1])
    bza = 0.0 if bz is None else _d(bz).abs()
    up_full = up + (0 if bz is None else _d(bz))
    Eup = Eup + U32 * (up.abs() + Eup + bza)
    P = gate * up_full
    EP = Eg * (up_full.abs() + Eup) + gate.abs() * Eup
    EP = EP + U32 * (P.abs() + EP)
    return EP + U32 * (z.abs() + P.abs() + EP)


TAIL_KINDS = ("ordinary", "spread", "zero z row", "zero o column", "constant")


@functools.lru_cache(maxsize=None)
def tri_tail_weights(mode):
    """(w_in, w_out, Wg, bg, Wz, bz): gains 1 + 0.2 randn, projections randn / sqrt(K), biases 0.3 randn"""
    g = gen(77 + mode)
    K2 = CO if mode == 0 else C_
    w_in = 1 + 0.2 * torch.randn(C_, generator=g)
    w_out = 1 + 0.2 * torch.randn(CO, generator=g)
    Wg = torch.randn(C_, C_, generator=g) / math.sqrt(C_)
    if mode == 1:                         # a raw gate: a common component in W_g and in the rows keeps |gate| away from the cancellation
        Wg = Wg + 0.05                    # noise sum |zn| |W| u that the bound carries (the non-vacuity condition of test_triangle_ref_cpu.py)
    bg = 0.3 * torch.randn(C_, generator=g)
    Wz = torch.randn(C_, K2, generator=g) / math.sqrt(K2)
    bz = 0.3 * torch.randn(C_, generator=g)
    return w_in, w_out, Wg, bg, Wz, bz


@functools.lru_cache(maxsize=None)
def tri_tail_case(mode, M):
    """(z [M, C], o ([Co, M] or [M, C]), kind per row, zn_amax, on_amax): row r has kind (r + r // 5) % 5 of TAIL_KINDS - ordinary rows,
    rows whose norms spread over exp(randn), an all-zero z row, an all-zero column (mode 1: row) of o, constant rows.  The static
    bounds as the engine derives them: sqrt(C) max|w_in| 1.0001, sqrt(Co) max|w_out| 1.0001 (mode 0), max|o| (mode 1)."""
    g = gen(31 * M + mode)
    w_in, w_out = tri_tail_weights(mode)[:2]
    r = torch.arange(M)
    kind = (r + r // 5) % 5
    z = torch.randn(M, C_, generator=g) + (0.5 if mode == 1 else 0.0)
    spread = torch.exp(torch.randn(M, 1, generator=g))
    const = (0.7 * (1 + r % 5) * (1 - 2.0 * (r % 2)))[:, None].expand(M, C_)
    z = torch.where((kind == 1)[:, None], z * spread, z)
    z = torch.where((kind == 2)[:, None], torch.zeros(()), z)
    z = torch.where((kind == 4)[:, None], const, z).contiguous()
    K2 = CO if mode == 0 else C_
    o = 2.0 * torch.randn(M, K2, generator=g)
    o = torch.where((kind == 1)[:, None], o * torch.exp(torch.randn(M, 1, generator=g)), o) if mode == 0 else o
    o = torch.where((kind == 3)[:, None], torch.zeros(()), o)
    o = torch.where((kind == 4)[:, None], 1.5 * torch.ones(()), o)
    zn_amax = f32(math.sqrt(C_) * float(w_in.abs().max()) * 1.0001)
    on_amax = f32(math.sqrt(CO) * float(w_out.abs().max()) * 1.0001) if mode == 0 else f32(float(o.abs().max()))
    o = (o.T if mode == 0 else o).contiguous()
    return z, o, kind, zn_amax, on_amax


@functools.lru_cache(maxsize=None)
def tri_tail_expected(mode, M, biases):
    """(reference, bound, update); biases False: bg = bz = NULL"""
    z, o, _, zn_amax, on_amax = tri_tail_case(mode, M)
    w_in, w_out, Wg, bg, Wz, bz = tri_tail_weights(mode)
    if not biases:
        bg = bz = None
    ref, upd = tri_tail64(mode, z, o, w_in, w_out, Wg, bg, Wz, bz)
    return ref, tri_tail_bound(mode, z, o, w_in, w_out, Wg, bg, Wz, bz, zn_amax, on_amax), upd


def tri_tail_emulated(mode, M, biases, low=True):
    """pd_tri_tail's arithmetic with exact accumulation and exact statistics: both contractions as h h' + h l' + l h' of the operands split as
    the kernel splits them.  low = False: a kernel that drops the low parts."""
    z, o, _, zn_amax, on_amax = tri_tail_case(mode, M)
    w_in, w_out, Wg, bg, Wz, bz = tri_tail_weights(mode)
    if not biases:
        bg = bz = None
    zs, os_ = pow2_scale(zn_amax), pow2_scale(on_amax)
    zd = _d(z)
    zn = zd * torch.rsqrt((zd * zd).mean(-1, keepdim=True) + TAIL_EPS) * _d(w_in)
    if mode == 0:
        ot = _d(o).T
        b = ot * torch.rsqrt((ot * ot).mean(-1, keepdim=True) + TAIL_EPS) * _d(w_out)
    else:
        b = _d(o)

    def contract(a, sa, W):
        sw = w_row_scale(W)[:, None]
        (ah, al), (wh, wl) = _parts(a.to(F32), sa, low), _parts(torch.as_tensor(W, dtype=F32) * sw.to(F32), 1.0, low)
        return (ah @ wh.T + ah @ wl.T + al @ wh.T) / sa / sw.T
    gl = contract(zn, zs, Wg) + (0 if bg is None else _d(bg))
    up = contract(b, os_, Wz) + (0 if bz is None else _d(bz))
    return zd + (torch.sigmoid(gl) if mode == 0 else gl) * up


# ================================================================== pd_tri_attention
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
LAZY = 3.0                                # tri_attn.hip: the running maximum follows a sub-tile's maximum only when that exceeds it by more than 3 (base-2 logits)
PSH = 14.0 - LAZY
MASKVAL = -1e9
ATT_H, ATT_D = 4, 32
ZN_AMAX = f32(math.sqrt(C_) * 1.0001)


def attn_scales(qkv_amax):
    """(qs, sq, sk, sv, a_s) as the kernel and pd_attention_bias_prescale_log2 derive them in fp32: qs = fl(fl(1 / sqrt(32)) fl(log2 e)), sq =
    pow2_scale(fl(q_amax qs)), sk, sv = pow2_scale of the k, v bounds, a_s = pow2_scale(zn_amax).  The bias prescale is sq sk."""
    qs = f32(f32(1.0 / math.sqrt(32.0)) * f32(LOG2E))
    return qs, pow2_scale(f32(f32(qkv_amax[0]) * qs)), pow2_scale(qkv_amax[1]), pow2_scale(qkv_amax[2]), pow2_scale(ZN_AMAX)


def _qkv(zhat, Wf):
    B, T = zhat.shape[:2]
    return [(zhat @ W.T).reshape(B, T, ATT_H, ATT_D).permute(0, 2, 1, 3) for W in _d(Wf).chunk(3)]          # [B, H, T, 32]


def tri_attention64(zhat, Wf, bias_pre, Treal, qkv_amax, parts=False):
    """o[b, r, 32 h + d] = sum_{k < Treal} softmax_k(q[b, r, h] . k[b, k, h] / sqrt(32) + bias[h, r, k]) v[b, k, h, d] with q | k | v = zhat . Wf^T,
    from the GIVEN operand zhat [B, T, 128] (= the two fp16 parts of z2 over their scale) and the GIVEN prescaled bias [H, T, >= Treal]
    (= bias log2 e sq sk): base-2 logits q . k log2 e / sqrt(32) + bias_pre / (sq sk).  parts: also the logits, the weights and v."""
    _, sq, sk, _, _ = attn_scales(qkv_amax)
    q, k, v = _qkv(_d(zhat), Wf)
    logit = q @ k[:, :, :Treal].transpose(-1, -2) * (LOG2E / math.sqrt(32.0)) + _d(bias_pre)[None, :, :, :Treal] / (sq * sk)
    p = torch.softmax(logit * LN2, -1)
    o = (p @ v[:, :, :Treal]).permute(0, 2, 1, 3).reshape(zhat.shape[0], zhat.shape[1], C_)
    return (o, logit, p, (q, k, v)) if parts else o


def tri_attention_bound(zhat, Wf, bias_pre, live, Treal, qkv_amax):
    """Bound of o for the query rows that have a live key (live [T, Treal]: the key is not masked; a masked logit lies 1.4e9 below every live one,
    its weight is exactly 0 in float64 and below 2^-1000 of the row's in the kernel, whatever its rounding: E = 0 there).
    Projection: _mma_err over K = 128 of the exact operand zhat against Wf split with one scale per 32 rows.  q is multiplied by fl(qs / (a_s
    w_scale)), qs = fl(fl(scale) fl(log2 e)) sq: 4 roundings against the exact scale log2 e / sqrt(32), then split at scale sq; k and v by
    powers of two (exact), split at sk, sv.  Logit error E per (b, h, query, key): _mma_err over K = 32 of those operands, + the bias tile as
    the accumulator's first value: the 2 x 19 + 1 roundings of the two steps act on it as well, + its division by sq sk: exact.
    Softmax: p^ = exp2^(fl(s c_s + mneg)), mneg = fl(-m c_s + PSH) for the running maximum m the phase holds: l_k - 3 <= m <= M = the row's
    largest live logit, so the fma's rounding is at most u (M - l_k + 14) in the exponent; every rescale (at most one per sub-tile: n of
    them) carries the roundings of (m - m') c_s and of the two mneg, u (4 max|l| + 22) in the exponent, the exp2 of alpha and the product
    o alpha or l alpha: (EXP2_REL + 1) u relative; the exp2 of p^ itself EXP2_REL u.  What is common to numerator and denominator cancels, the
    rest is Etot_k; |dp_k| <= p_k (e^(Etot_k + Emax) - 1), Emax the row's largest Etot.
    P . V: the weights are split (2^-22 relative where the low part is normal, 2^-25 absolute below, against a normaliser of at least 2^8 in
    the same units: 2^-33 per key), low x low dropped (2^-22), 2 x 19 roundings per sub-tile and 1 per rescale; the normaliser: 16 adds per
    lane and sub-tile, 1 to the running sum, 1 per rescale, the cross-half add; the division (SAFETY_DIV) and the product by it."""
    qs, sq, sk, sv, a_s = attn_scales(qkv_amax)
    zhat = _d(zhat)
    o, logit, p, (q, k, v) = tri_attention64(zhat, Wf, bias_pre, Treal, qkv_amax, parts=True)
    nsub = (Treal + 31) // 32
    ws = w_row_scale(Wf, 32)
    B, T = zhat.shape[:2]
    dq, dk, dv = [_mma_err(zhat, 0.0, a_s, W, 0.0, s[:, None], C_, exactA=True).reshape(B, T, ATT_H, ATT_D).permute(0, 2, 1, 3)
                  for W, s in zip(_d(Wf).chunk(3), ws.chunk(3))]
    c = LOG2E / math.sqrt(32.0)
    E = _mma_err(q * c, (dq + 4 * U32 * q.abs()) * c, sq, k[:, :, :Treal], dk[:, :, :Treal], sk, ATT_D)
    E = E + gamma(2 * MMA_STEP + 1) * (_d(bias_pre)[None, :, :, :Treal] / (sq * sk)).abs()
    lv = live[None, None]
    E = torch.where(lv, E, torch.zeros_like(E))
    neg = torch.full_like(logit, -float("inf"))
    M = torch.where(lv, logit, neg).amax(-1, keepdim=True)
    Mabs = torch.where(lv, logit.abs() + E, torch.zeros_like(E)).amax(-1, keepdim=True)
    Etot = LN2 * (E + U32 * ((M - logit).clamp(min=0) + 14 + E) + nsub * U32 * (4 * Mabs + 22)) + U32 * (EXP2_REL + nsub * (EXP2_REL + 1))
    Etot = torch.where(lv, Etot, torch.zeros_like(Etot))
    Emax = Etot.amax(-1, keepdim=True)
    va, vr = v[:, :, :Treal].abs(), None
    dvt = dv[:, :, :Treal] + _split_err((va + dv[:, :, :Treal]) * sv) / sv
    R = gamma(2 * MMA_STEP * nsub + nsub) + gamma(18 * nsub + 2) + 2.0 ** -21 + (SAFETY_DIV + 1) * U32
    grow = torch.exp(2 * Emax)
    bound = (p * torch.expm1(Etot + Emax)) @ va + grow * (p @ dvt + R * (p @ (va + dvt)) + 2.0 ** -33 * (lv.to(F64) @ (va + dvt)))
    return bound.permute(0, 2, 1, 3).reshape(B, T, C_)


ATTN_TREAL = [1, 29, 32, 33, 64, 65, 96, 100, 128, 131, 160, 192, 199, 224, 225, 256]
ATTN_FEW = [(256, 40), (200, 64)]
ATTN_VARIANTS = {"mild": 0.0, "std10": 0.0, "ramp+0.1": 0.1, "ramp+0.05": 0.05, "ramp-0.1": -0.1}


def attn_T_values(Treal):
    """the smallest T >= Treal with T % 8 == 0 (the remapped grid) and with T % 8 == 4 (the plain grid), within 256"""
    return [t for t in ((Treal + 7) // 8 * 8, (Treal + 3) // 8 * 8 + 4) if Treal <= t <= 256]


def attn_batches(T):
    """the batch rows compared with float64: all of them up to T = 132; beyond, 24 of them (the first and last eight, eight spread between) -
    a float64 reference of all 256 costs 10 s a case.  Every batch row is launched, written and checked to be finite."""
    if T <= 132:
        return torch.arange(T)
    return torch.unique(torch.cat([torch.arange(8), torch.arange(T - 8, T), torch.linspace(8, T - 9, 8).long()]))


@functools.lru_cache(maxsize=None)
def attn_weights(variant):
    """Wf [384, 128] = q | k | v.  All weights positive (w0 |1 + 0.5 randn|) and the rows of z with a common component: the projections and
    the scores then have little cancellation, sum |a| |b| stays near |sum a b|, and the worst-case accumulation terms stay below 1e-3 of the
    mean |o| (with the randn / sqrt(C) weights of tests/test_tri_attn_gpu.py they do not: test_triangle_ref_cpu.py prints the figure).
    "std10": q and k scaled so that the float64 logits of batch row 0 have a standard deviation of 10 over the keys."""
    g = gen(404)
    base = (1 + 0.5 * torch.randn(3 * C_, C_, generator=g)).abs()
    w0 = torch.tensor([0.0124, 0.0124, 0.02]).repeat_interleave(C_)[:, None]
    Wf = base * w0
    if variant == "std10":
        zhat = attn_zhat(128, 128, True)[0][:1]
        q, k, _ = _qkv(zhat.to(F64), Wf)
        sd = float((q @ k.transpose(-1, -2) / math.sqrt(32.0)).std(-1).mean())
        Wf[:2 * C_] *= math.sqrt(10.0 / sd)
    return Wf.contiguous()


@functools.lru_cache(maxsize=None)
def attn_zhat(T, Treal, signed=False):
    """(zhat [T, T, 128] float64 = (hi + lo) / a_s, hi, lo): rows x / rms(x), x = randn + mu with mu in [0.3, 2] per row, scaled by a_s and split in
    exact torch; the rows r in [Treal, T) one-hot at the bound sqrt(128).  signed (the "std10" cases): mu takes a random sign per row, so the
    logits are spread about 0 - a standard deviation of 10 at |logit| ~ 10 and not on top of a mean of 40, which the logit error follows -
    while every projection still sums terms of one sign; a query's weight sits on the keys of its own sign, so o does not cancel either."""
    g = gen(7 * T + Treal + (500000 if signed else 0))
    mu = 0.3 + 1.7 * torch.rand(T, T, 1, generator=g)
    if signed:
        mu = mu * (1 - 2.0 * (torch.rand(T, T, 1, generator=g) < 0.5))
    x = torch.randn(T, T, C_, generator=g) + mu
    zn = (x.double() * torch.rsqrt((x.double() ** 2).mean(-1, keepdim=True))).float()
    if Treal < T:
        b, r = torch.meshgrid(torch.arange(T), torch.arange(Treal, T), indexing="ij")
        hot = torch.zeros(T, T - Treal, C_)
        hot.scatter_(2, ((b + r) % C_)[..., None], (math.sqrt(C_) * (1 - 2.0 * ((b + r) % 2)))[..., None].float())
        zn[:, Treal:] = hot
    a_s = pow2_scale(ZN_AMAX)
    hi, lo = nb.split2_f16(zn * a_s)
    return (hi.double() + lo.double()) / a_s, hi, lo


@functools.lru_cache(maxsize=None)
def attn_case(T, Treal, variant="mild", amax_f=1.0001, nk0=False):
    """dict of the launch's operands: zhat / hi / lo, Wf, qkv_amax (static: the largest row norm of each block times sqrt(128) amax_f), ps,
    bias_dense [H, T, nkl] fp32 prescaled (nkl = Treal if nk0 else T; NaN for the keys >= Treal), live [T, Treal], full (query rows with no
    live key).  Bias 0.5 randn + g k + the masks: 10 % at random; from 8 keys on, row 3 fully masked, row 5 with a single live key, row 7 with
    live keys in the last sub-tile only."""
    g = gen(13 * T + Treal + 1000 * len(variant))
    zhat, hi, lo = attn_zhat(T, Treal, variant == "std10")
    Wf = attn_weights("std10" if variant == "std10" else "mild")
    amax = tuple(f32(float(W.double().norm(dim=1).max()) * math.sqrt(C_) * amax_f) for W in Wf.chunk(3))
    _, sq, sk, _, _ = attn_scales(amax)
    live = torch.rand(T, Treal, generator=g) > 0.1
    if Treal >= 8:
        live[3] = False
        live[5] = False
        live[5, Treal // 2] = True
        live[7] = False
        live[7, 32 * ((Treal - 1) // 32):] = True
    nat = 0.5 * torch.randn(ATT_H, T, Treal, generator=g).double() + ATTN_VARIANTS[variant] * torch.arange(Treal).double()
    nat = torch.where(live[None], nat, torch.full_like(nat, MASKVAL))
    nkl = Treal if nk0 else T
    dense = torch.full((ATT_H, T, nkl), NAN)
    dense[:, :, :Treal] = (nat * (LOG2E * sq * sk)).float()
    return dict(zhat=zhat, hi=hi, lo=lo, Wf=Wf, qkv_amax=amax, ps=sq * sk, bias=dense, live=live, full=~live.any(1), nkl=nkl)


@functools.lru_cache(maxsize=None)
def attn_expected(T, Treal, variant="mild", amax_f=1.0001, nk0=False):
    """(batch rows, reference [nb, T, 128], bound, uniform [nb, 128]: the fp32 statement of a fully masked row, the mean of v over the real keys)"""
    c = attn_case(T, Treal, variant, amax_f, nk0)
    bs = attn_batches(T)
    refs, bounds, uni = [], [], []
    for ch in bs.split(16):
        z = c["zhat"][ch]
        refs.append(tri_attention64(z, c["Wf"], c["bias"], Treal, c["qkv_amax"]))
        bounds.append(tri_attention_bound(z, c["Wf"], c["bias"], c["live"], Treal, c["qkv_amax"]))
        uni.append((z[:, :Treal] @ _d(c["Wf"])[2 * C_:].T).mean(1))
    return bs, torch.cat(refs), torch.cat(bounds), torch.cat(uni)


def lazy_rises(logit, live):
    """[.., T, nsub - 1] bool: at the transition into sub-tile j the lazy running maximum of the row rises, i.e. the sub-tile's largest live
    logit exceeds the running maximum by more than LAZY (then the running maximum follows it)"""
    Treal = logit.shape[-1]
    l = torch.where(live, logit, torch.full_like(logit, -float("inf")))
    nsub = (Treal + 31) // 32
    sub = torch.stack([l[..., 32 * j:32 * j + 32].amax(-1) for j in range(nsub)], -1)
    m, out = sub[..., 0], []
    for j in range(1, nsub):
        rise = sub[..., j] > m + LAZY
        m = torch.where(rise, torch.maximum(m, sub[..., j]), m)
        out.append(rise)
    return torch.stack(out, -1) if out else torch.zeros(*logit.shape[:-1], 0, dtype=torch.bool)
