"""The conditions tests/test_triangle_kernels_gpu.py relies on, asserted without a GPU: the float64 references of tests/triangle_ref.py
agree with independent plain-torch formulations; the static bounds handed to the kernels bound the operands; no bound is vacuous
(no live element's bound above 1e-3 of the case's mean |output|, for pd_tri_tail of its mean |update|); the kernels' arithmetic with exact
accumulation stays within the bounds, and subtly wrong kernels emulated on the CPU do not."""
import itertools
import math

import pytest
import torch

import triangle_ref as tr
from triangle_ref import F64

VACUOUS = 1e-3


# ------------------------------------------------------------------ pd_tri_mul
@pytest.mark.parametrize("T,Treal", tr.TRI_MUL_SHAPES)
def test_tri_mul_reference_is_the_einsum(T, Treal):
    for nch, transpose in itertools.product((1, 5), (0, 1)):
        q, k, _, _ = tr.tri_mul_case(T, nch)
        qd, kd = q.double(), k.double()
        if transpose:
            want = torch.einsum("cja,cjb->cab", kd[:, :Treal], qd[:, :Treal])
        else:
            want = torch.einsum("cij,cIj->ciI", qd[:, :, :Treal], kd[:, :, :Treal])
        got = tr.tri_mul64(q, k, Treal, transpose)
        assert got.shape == (nch, T, T)
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12 * float(want.abs().max()))
        # the poisoned entries are never read
        assert torch.equal(got, tr.tri_mul64(tr.tri_mul_poisoned(q, Treal, transpose), tr.tri_mul_poisoned(k, Treal, transpose), Treal, transpose))


@pytest.mark.parametrize("T,Treal", tr.TRI_MUL_SHAPES)
def test_tri_mul_static_bounds_and_bounds_not_vacuous(T, Treal):
    for nch, transpose, loose in itertools.product(tr.TRI_MUL_NCH, (0, 1), (False, True)):
        q, k, _, _ = tr.tri_mul_case(T, nch)
        ref, bound, qa, ka = tr.tri_mul_expected(T, Treal, nch, transpose, loose)
        assert float(q.abs().max()) <= qa and float(k.abs().max()) <= ka
        assert torch.isfinite(bound).all() and (bound >= 0).all()
        worst = float(bound.max() / ref.abs().mean())
        print(f"tri_mul T={T} Treal={Treal} nch={nch} transpose={transpose} loose={loose}: max bound / mean|o| = {worst:.2e}")
        assert worst <= VACUOUS
        if nch > tr.ZERO_PLANE:           # an all-zero plane must come back as exact zeros
            assert float(bound[tr.ZERO_PLANE].max()) == 0.0 and float(ref[tr.ZERO_PLANE].abs().max()) == 0.0


@pytest.mark.parametrize("T,Treal", tr.TRI_MUL_SHAPES)
def test_tri_mul_bound_admits_the_kernel_arithmetic(T, Treal):
    for nch, transpose, loose in itertools.product((3, 32), (0, 1), (False, True)):
        q, k, _, _ = tr.tri_mul_case(T, nch)
        ref, bound, qa, ka = tr.tri_mul_expected(T, Treal, nch, transpose, loose)
        emu = tr.tri_mul_emulated(q, k, Treal, transpose, qa, ka).float()
        assert tr.bound_ratio(emu, ref, bound) <= 1.0


def _worst_over_cases(wrong):
    worst = 0.0
    for (T, Treal), nch, transpose, loose in itertools.product(tr.TRI_MUL_SHAPES, (3, 32), (0, 1), (False, True)):
        q, k, _, _ = tr.tri_mul_case(T, nch)
        ref, bound, qa, ka = tr.tri_mul_expected(T, Treal, nch, transpose, loose)
        out = wrong(q, k, T, Treal, transpose, qa, ka)
        if out is not None:
            worst = max(worst, tr.bound_ratio(out.float(), ref, bound))
    return worst


def test_tri_mul_bound_rejects_a_kernel_that_drops_the_low_parts():
    """(a) operands rounded to one fp16 part"""
    worst = _worst_over_cases(lambda q, k, T, Treal, tp, qa, ka: tr.tri_mul_emulated(q, k, Treal, tp, qa, ka, low=False))
    print(f"one fp16 part: worst |err| / bound {worst:.1f}")
    assert worst > 1.0


@pytest.mark.parametrize("transpose", [0, 1])
def test_tri_mul_bound_rejects_a_kernel_that_reduces_over_index_Treal(transpose):
    """(c) the reduction includes index Treal, in each form: with the finite operand entry that sits there, and with the NaN the GPU
    cases put there"""
    def wrong(poison):
        def f(q, k, T, Treal, tp, qa, ka):
            if tp != transpose or Treal == T:
                return None
            if poison:
                q, k = tr.tri_mul_poisoned(q, Treal, tp), tr.tri_mul_poisoned(k, Treal, tp)
            return tr.tri_mul_emulated(q, k, Treal, tp, qa, ka, extra_j=1)
        return f
    for poison in (False, True):
        worst = _worst_over_cases(wrong(poison))
        print(f"reduction over j <= Treal, transpose={transpose}, poisoned={poison}: worst |err| / bound {worst:.1f}")
        assert worst > 1.0


# ------------------------------------------------------------------ pd_tri_tail
TAIL_CPU_M = tr.TAIL_SMALL_M


def _tail_formula(mode, z, o, w_in, w_out, Wg, bg, Wz, bz, eps):
    """the header's formula row by row, independent of tri_tail64's whole-tensor algebra"""
    z, o, w_in, w_out, Wg, Wz = (t.double() for t in (z, o, w_in, w_out, Wg, Wz))
    out = torch.empty_like(z)
    for m in range(z.shape[0]):
        zn = z[m] / torch.sqrt((z[m] ** 2).sum() / z.shape[1] + eps) * w_in
        gl = Wg @ zn + (bg.double() if bg is not None else 0)
        if mode == 0:
            col = o[:, m]
            b = col / torch.sqrt((col ** 2).sum() / col.numel() + eps) * w_out
            gate = 1 / (1 + torch.exp(-gl))
        else:
            b, gate = o[m], gl
        out[m] = z[m] + gate * (Wz @ b + (bz.double() if bz is not None else 0))
    return out


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M", TAIL_CPU_M)
def test_tri_tail_reference_is_the_header_formula(mode, M):
    z, o, kind, _, _ = tr.tri_tail_case(mode, M)
    w_in, w_out, Wg, bg, Wz, bz = tr.tri_tail_weights(mode)
    for biases in (True, False):
        ref, _, upd = tr.tri_tail_expected(mode, M, biases)
        want = _tail_formula(mode, z, o, w_in, w_out, Wg, bg if biases else None, Wz, bz if biases else None, tr.TAIL_EPS)
        assert torch.allclose(ref, want, rtol=1e-12, atol=1e-12)
        assert torch.equal(ref - z.double(), upd) or torch.allclose(ref - z.double(), upd, rtol=0, atol=1e-12)
    if M >= 10:
        assert set(kind.tolist()) == set(range(len(tr.TAIL_KINDS)))          # every kind of row occurs


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M", TAIL_CPU_M + [None])
def test_tri_tail_static_bounds_and_bounds_not_vacuous(mode, M):
    M = tr.TAIL_GRID_M[mode] if M is None else M
    z, o, _, zn_amax, on_amax = tr.tri_tail_case(mode, M)
    w_in, w_out = tr.tri_tail_weights(mode)[:2]
    zd = z.double()
    zn = zd * torch.rsqrt((zd * zd).mean(-1, keepdim=True) + tr.TAIL_EPS) * w_in.double()
    assert float(zn.abs().max()) <= zn_amax
    if mode == 0:
        od = o.double().T
        on = od * torch.rsqrt((od * od).mean(-1, keepdim=True) + tr.TAIL_EPS) * w_out.double()
        assert float(on.abs().max()) <= on_amax
    else:
        assert float(o.abs().max()) <= on_amax
    for biases in (True, False):
        ref, bound, upd = tr.tri_tail_expected(mode, M, biases)
        assert torch.isfinite(bound).all()
        worst = float(bound.max() / upd.abs().mean())
        print(f"tri_tail mode {mode} M={M} biases={biases}: max bound / mean|update| = {worst:.2e}")
        assert worst <= VACUOUS
        assert tr.bound_ratio(ref.float(), ref, bound) <= 1.0                 # the correctly rounded result is admitted


@pytest.mark.parametrize("mode", [0, 1])
def test_tri_tail_bound_rejects_a_kernel_that_skips_the_last_partial_tile(mode):
    """(e) the rows of the last partial tile left un-updated"""
    rejected = 0
    for M in [m for m in tr.TAIL_SMALL_M + [tr.TAIL_GRID_M[mode]] if m % tr.BM]:
        z, _, _, _, _ = tr.tri_tail_case(mode, M)
        ref, bound, _ = tr.tri_tail_expected(mode, M, True)
        out = ref.float()
        first = M // tr.BM * tr.BM
        out[first:] = z[first:]
        ratio = tr.bound_ratio(out, ref, bound)
        print(f"tri_tail mode {mode} M={M}: last partial tile skipped: worst |err| / bound {ratio:.1f}")
        rejected += ratio > 1.0
    assert rejected >= 1


def test_contraction_bound_follows_the_operand_scale():
    """a bound given 1000 x too large costs the small elements their low bits: the bound grows, and only through the subnormal term"""
    T, Treal, nch = 36, 33, 5
    tight = tr.tri_mul_expected(T, Treal, nch, 0, False)[1]
    loose = tr.tri_mul_expected(T, Treal, nch, 0, True)[1]
    assert (loose >= tight * (1 - 1e-12)).all()
    assert float(loose.max()) <= 2 * float(tight.max())
    assert math.isclose(tr.pow2_scale(3.0) * 3.0, 2.0 ** 14 * 1.5)


@pytest.mark.parametrize("mode", [0, 1])
def test_tri_tail_bound_admits_the_kernel_arithmetic_and_rejects_dropped_low_parts(mode):
    """the two split contractions with exact accumulation stay within the bound; (a) with the low parts dropped they do not"""
    worst = 0.0
    for M, biases in itertools.product(tr.TAIL_SMALL_M, (True, False)):
        ref, bound, _ = tr.tri_tail_expected(mode, M, biases)
        assert tr.bound_ratio(tr.tri_tail_emulated(mode, M, biases).float(), ref, bound) <= 1.0
        worst = max(worst, tr.bound_ratio(tr.tri_tail_emulated(mode, M, biases, low=False).float(), ref, bound))
    print(f"tri_tail mode {mode}, one fp16 part: worst |err| / bound {worst:.1f}")
    assert worst > 1.0


# ------------------------------------------------------------------ pd_tri_attention
def attn_gpu_cases():
    """every (T, Treal, variant, amax_f, nk0) of tests/test_triangle_kernels_gpu.py"""
    out = [(T, Tr, "mild", 1.0001, False) for Tr in tr.ATTN_TREAL for T in tr.attn_T_values(Tr)]
    out += [(T, Tr, "mild", 1.0001, False) for T, Tr in tr.ATTN_FEW]
    out += [(T, Tr, "mild", 1.0001, True) for T, Tr in ((36, 33), (128, 100), (256, 40))]
    out += [(T, T, v, 1.0001, False) for T in (128, 256) for v in tr.ATTN_VARIANTS]
    out += [(T, Tr, "mild", 30.0, False) for T, Tr in ((36, 33), (128, 128), (200, 199))]
    return list(dict.fromkeys(out))


SMALL_ATTN = [c for c in attn_gpu_cases() if c[0] <= 64]


def test_attention_case_list_covers_the_sub_tile_counts():
    cases = attn_gpu_cases()
    for grid in (0, 4):
        seen = {((Tr + 31) // 32, Tr % 32 == 0) for T, Tr, *_ in cases if T % 8 == grid}
        assert {n for n, _ in seen} == set(range(1, 9)), (grid, seen)
        assert {full for _, full in seen} == {True, False}


@pytest.mark.parametrize("case", SMALL_ATTN, ids=str)
def test_tri_attention_reference_is_the_softmax_attention(case):
    T, Treal = case[:2]
    c = tr.attn_case(*case)
    bs, ref, _, uni = tr.attn_expected(*case)
    Wq, Wk, Wv = c["Wf"].double().chunk(3)
    nat = c["bias"].double()[:, :, :Treal] / (tr.LOG2E * c["ps"])
    for n, b in enumerate(bs.tolist()):
        z = c["zhat"][b]
        for h in range(4):
            sl = slice(32 * h, 32 * h + 32)
            s = (z @ Wq[sl].T) @ (z[:Treal] @ Wk[sl].T).T / math.sqrt(32.0) + nat[h]
            want = torch.softmax(s, -1) @ (z[:Treal] @ Wv[sl].T)
            keep = ~c["full"]
            assert torch.allclose(ref[n][keep][:, sl], want[keep], rtol=1e-9, atol=1e-12)
    assert torch.allclose(uni, (c["zhat"][bs][:, :Treal] @ Wv.T).mean(1))


def _attn_vacuity(case):
    T, Treal = case[:2]
    c = tr.attn_case(*case)
    _, ref, bound, _ = tr.attn_expected(*case)
    keep = ~c["full"]
    keep[Treal:] = False
    return float(bound[:, keep].max() / ref[:, keep].abs().mean()), bool(torch.isfinite(bound[:, keep]).all())


@pytest.mark.parametrize("case", attn_gpu_cases(), ids=str)
def test_tri_attention_static_bounds_and_bounds_not_vacuous(case):
    T, Treal = case[:2]
    c = tr.attn_case(*case)
    for blk, (W, a) in enumerate(zip(c["Wf"].double().chunk(3), c["qkv_amax"])):
        assert float((c["zhat"][:8] @ W.T).abs().max()) <= a
    assert float(c["zhat"].abs().max()) <= tr.ZN_AMAX
    worst, finite = _attn_vacuity(case)
    print(f"tri_attention {case}: max bound / mean|o| = {worst:.2e}")
    assert finite and worst <= VACUOUS


def _attn_ratio(case, out_of):
    """worst |err| / bound over the bounded rows of what `out_of(case dict, batch rows)` returns as [nb, T, 128]"""
    T, Treal = case[:2]
    c = tr.attn_case(*case)
    bs, ref, bound, _ = tr.attn_expected(*case)
    keep = ~c["full"]
    keep[Treal:] = False
    out = out_of(c, bs)
    return tr.bound_ratio(out[:, keep].float(), ref[:, keep], bound[:, keep])


def test_tri_attention_bound_admits_the_rounded_reference_and_rejects_one_fp16_part():
    """(a) z2 and the weights rounded to their high parts"""
    case = (36, 33, "mild", 1.0001, False)

    def high_only(c, bs):
        a_s = tr.pow2_scale(tr.ZN_AMAX)
        ws = tr.w_row_scale(c["Wf"], 32)[:, None]
        Wh = (c["Wf"].double() * ws).to(torch.float16).double() / ws
        return tr.tri_attention64(c["hi"][bs].double() / a_s, Wh, c["bias"], 33, c["qkv_amax"])
    assert _attn_ratio(case, lambda c, bs: tr.tri_attention64(c["zhat"][bs], c["Wf"], c["bias"], 33, c["qkv_amax"])) <= 1.0
    worst = _attn_ratio(case, high_only)
    print(f"tri_attention, one fp16 part: worst |err| / bound {worst:.1f}")
    assert worst > 1.0


def test_tri_attention_bound_rejects_a_softmax_over_key_Treal():
    """(b) key Treal included: with the NaN the cases put into its bias slot, and with a finite bias there"""
    case = (36, 33, "mild", 1.0001, False)
    for fill in (tr.NAN, 0.0):
        def wrong(c, bs):
            bias = c["bias"].clone()
            bias[:, :, 33] = fill
            o = tr.tri_attention64(c["zhat"][bs], c["Wf"], bias, 34, c["qkv_amax"])
            return torch.where(torch.isnan(o), torch.full_like(o, float("inf")), o)
        worst = _attn_ratio(case, wrong)
        print(f"tri_attention, key Treal in the softmax (bias there {fill}): worst |err| / bound {worst:.1f}")
        assert worst > 1.0


def test_tri_attention_bound_rejects_a_running_maximum_that_is_never_updated():
    """(d) the maximum of the first sub-tile kept to the end: P = 2^(l - m + PSH) leaves the fp16 range on the ascending ramp"""
    case = (128, 128, "ramp+0.1", 1.0001, False)

    def wrong(c, bs):
        o, logit, p, _ = tr.tri_attention64(c["zhat"][bs], c["Wf"], c["bias"], 128, c["qkv_amax"], parts=True)
        lv = c["live"][None, None]
        l = torch.where(lv, logit, torch.full_like(logit, -float("inf")))
        over = ((l - l[..., :32].amax(-1, keepdim=True) + tr.PSH) >= 16).any(-1)                  # [nb, H, T]: a weight beyond 65504
        bad = over.permute(0, 2, 1)[..., None].expand(-1, -1, -1, 32).reshape(o.shape)
        return torch.where(bad, torch.full_like(o, float("inf")), o)
    worst = _attn_ratio(case, wrong)
    print(f"tri_attention, running maximum never updated: worst |err| / bound {worst}")
    assert worst > 1.0


def test_tri_attention_bound_rejects_a_bias_pitch_taken_from_Treal():
    """(f) the bias laid out for nk = T read with the tile pitch of nk = Treal"""
    import norm_bias_ref as nb
    case = (256, 40, "mild", 1.0001, False)

    def wrong(c, bs):
        frag, _ = nb.bias_frag_scatter(c["bias"])
        idx = nb.bias_frag_index(4, 256, 40)
        dense = frag[idx]
        o = tr.tri_attention64(c["zhat"][bs], c["Wf"], dense, 40, c["qkv_amax"])
        return torch.where(torch.isnan(o), torch.full_like(o, float("inf")), o)
    worst = _attn_ratio(case, wrong)
    print(f"tri_attention, bias pitch from Treal: worst |err| / bound {worst}")
    assert worst > 1.0


@pytest.mark.parametrize("T", [128, 256])
def test_ramp_cases_do_what_they_claim(T):
    """transitions at which the lazy running maximum rises, over the ordinary query rows (the kernel rescales a wave when any of its rows rises)"""
    frac = {}
    for v in ("ramp+0.1", "ramp+0.05", "ramp-0.1"):
        c = tr.attn_case(T, T, v)
        bs = tr.attn_batches(T)[:4]
        _, logit, _, _ = tr.tri_attention64(c["zhat"][bs], c["Wf"], c["bias"], T, c["qkv_amax"], parts=True)
        rises = tr.lazy_rises(logit, c["live"][None, None])
        rises[:, :, :8] = False                                                   # rows 3, 5, 7 carry the special masks
        waves = rises.reshape(rises.shape[0], 4, T // 32, 32, rises.shape[-1]).any(3)      # the kernel rescales a wave when any of its 32 rows rises
        frac[v] = (float(rises[:, :, 8:].float().mean()), bool(waves.all()), bool(rises.any()))
        print(f"T={T} {v}: lazy maximum rises at {frac[v][0]:.2f} of the (row, transition) pairs; in every wave at every transition: {frac[v][1]}")
    assert frac["ramp+0.1"][1]
    assert not frac["ramp-0.1"][2]
    assert 0.0 < frac["ramp+0.05"][0] < 1.0


def test_existing_random_weights_would_be_vacuous():
    """the figure behind attn_weights' docstring: randn / sqrt(C) weights on rows without a common component"""
    g = tr.gen(5)
    T = Treal = 36
    x = torch.randn(T, T, 128, generator=g).double()
    zhat = x * torch.rsqrt((x * x).mean(-1, keepdim=True))
    Wf = torch.randn(384, 128, generator=g) * 1.5 / math.sqrt(128.0)
    amax = tuple(tr.f32(float(W.double().norm(dim=1).max()) * math.sqrt(128.0) * 1.0001) for W in Wf.chunk(3))
    bias = torch.zeros(4, T, T)
    live = torch.ones(T, Treal, dtype=torch.bool)
    ref = tr.tri_attention64(zhat[:8], Wf, bias, Treal, amax)
    bound = tr.tri_attention_bound(zhat[:8], Wf, bias, live, Treal, amax)
    print(f"randn / sqrt(C) weights, T = 36: max bound / mean|o| = {float(bound.max() / ref.abs().mean()):.2e}")
