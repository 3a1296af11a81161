"""The float64 references of tests/norm_bias_ref.py are right, the inputs of tests/test_norm_bias_kernels_gpu.py are well posed, and
every bounded check has power.  CPU only: the layout maps are bijections and tie ops.bias_to_frag down, the split helpers reconstruct,
the conditions the GPU cases rely on are asserted on the real generators, and - through the very comparison functions the GPU tests
call - the float64 reference evaluated in fp32 by torch (another summation order than any kernel's) passes on every case while each
deliberately wrong variant is rejected on a named case."""
import math

import pytest
import torch

import norm_bias_ref as nb
import test_norm_bias_kernels_gpu as gk
from norm_bias_ref import ACT_NONE, F32, F64, LN, RMS

EPS = gk.EPS


def rejected(kernel, case, dev, ref, bound):
    with pytest.raises(AssertionError):
        nb.assert_within_bound(kernel, case, dev, ref, bound)
    return True


def stats32(x, mode):
    return torch.stack(nb.rowstats64(x, mode, EPS[mode], dtype=F32), -1)


# ------------------------------------------------------------------ layout maps
BIAS_SHAPES = [(4, 1, 4), (4, 4, 1), (8, 5, 12), (16, 33, 36), (24, 68, 65), (4, 40, 72)]


@pytest.mark.parametrize("H,nq,nk", BIAS_SHAPES)
def test_bias_fragment_map_is_a_bijection_and_ops_bias_to_frag_agrees(H, nq, nk):
    from physdock_amd import ops
    idx = nb.bias_frag_index(H, nq, nk).reshape(-1)
    n = nb.bias_frag_numel(H, nq, nk)
    assert n == ops.bias_frag_numel(H, nq, nk)
    assert int(idx.min()) >= 0 and int(idx.max()) < n and idx.unique().numel() == H * nq * nk
    dense = torch.randn(H, nq, nk, generator=gk.gen(1)) + 3.0                      # no zero among the real values
    frag, real = nb.bias_frag_scatter(dense)
    assert int(real.sum()) == H * nq * nk and torch.isnan(frag[~real]).all()
    assert torch.equal(frag[nb.bias_frag_index(H, nq, nk)], dense)                 # scatter, then gather: the identity
    helper = ops.bias_to_frag(dense)                                               # pads with 0, scales by log2 e
    mine, _ = nb.bias_frag_scatter(dense * ops._lib.LOG2E, fill=0.0)
    assert torch.equal(helper, mine)
    assert torch.equal(helper != 0, real)
    # four consecutive keys of one query share a 16-byte slot; (q, k) and (k, q) do not share an address
    four = nb.bias_frag_index(H, nq, 4 * (nk // 4) or nk)[..., :4 * (nk // 4)].reshape(H, nq, -1, 4)
    assert bool((four[..., 1:] - four[..., :-1] == 1).all()) and bool((four[..., 0] % 4 == 0).all())


@pytest.mark.parametrize("T", gk.PBS_T + [32, 33])
def test_z2_map_is_a_bijection(T):
    from physdock_amd import ops
    idx = nb.z2_index(T).reshape(-1)
    n = nb.z2_numel(T)
    assert n == ops.tri_z2_numel(T)
    both = torch.cat([idx, idx + 512])
    assert int(both.min()) >= 0 and int(both.max()) < n and both.unique().numel() == 2 * T * T * 128
    real = nb.z2_real(T)
    assert int(real.sum()) == 2 * T * T * 128
    assert (int(real.sum()) == n) == (T % 32 == 0)                                 # rows beyond T of the last tile: no real slot
    hi = torch.randn(T, T, 128, generator=gk.gen(2)).half()
    lo = torch.randn(T, T, 128, generator=gk.gen(3)).half()
    buf = nb.z2_scatter(hi, lo, torch.tensor(float("nan"), dtype=torch.float16))
    assert torch.isnan(buf[~real]).all() and not torch.isnan(buf[real]).any()
    h2, l2 = nb.z2_gather(buf, T)
    assert torch.equal(h2, hi.double()) and torch.equal(l2, lo.double())
    # the eight halves of a slot are eight consecutive channels of one row; the two parts of a slot lie 512 halves apart
    i = nb.z2_index(T)
    assert bool((i[..., 1:8] - i[..., 0:7] == 1).all()) and bool((i[..., 0] % 8 == 0).all())
    assert int(i[0, 0, 8] - i[0, 0, 0]) == 32 * 8 and int(i[0, 0, 16] - i[0, 0, 0]) == 2 * 64 * 8
    if T > 1:
        assert int(i[0, 1, 0] - i[0, 0, 0]) == 8 and int(i[1, 0, 0] - i[0, 0, 0]) == ((T + 31) // 32) * 8 * 2 * 64 * 8


# ------------------------------------------------------------------ split helpers
def _wide_range(n, seed):
    g = gk.gen(seed)
    return (torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 15, (n,), generator=g).float())).float()


def test_three_way_bf16_split_reconstructs_exactly():
    a = torch.cat([_wide_range(20000, 4), torch.tensor([0.0, 1.0, -1.0, 255.5, 1e-30, 3e38 / 4])])
    h, m, l = nb.split3_bf16(a)
    assert torch.equal(h.double() + m.double() + l.double(), a.double())
    assert torch.equal((h + m) + l, a)
    for p in (h, m, l):
        assert torch.equal(p.to(torch.bfloat16).float(), p)
    assert torch.equal(h, nb.round_to(a.double(), "bf16").float())


def test_two_way_fp16_split_reconstructs_within_its_bound():
    a = torch.cat([_wide_range(20000, 5).clamp(-32767, 32767), torch.tensor([0.0, 1.0, 2.0 ** -20, 32767.0, -16384.25, 2.0 ** -3])])
    h, l = nb.split2_f16(a)
    err = (h.double() + l.double() - a.double()).abs()
    bound = nb.split2_bound(a)
    assert bool((err <= bound).all())
    assert bool((bound <= 2.0 ** -25 * torch.maximum(torch.ones(()), 8 * a.abs().double())).all())      # 2^-25 times the binade scale
    assert float((err / bound).max()) > 0.5                                       # and no looser than a factor two
    assert torch.equal(h, nb.round_to(a.double(), "fp16").float())                # subnormal fp16 values included


def test_pow2_scale():
    for amax, want in ((40.0, 2.0 ** 9), (32.0, 2.0 ** 9), (gk.AMAX_BELOW_32, 2.0 ** 10), (1e-20, 2.0 ** 54), (1e30, 2.0 ** -59),
                       (16.0, 2.0 ** 10), (math.sqrt(128.0), 2.0 ** 11), (gk.ZN_AMAX[2], 2.0 ** 11), (1.0, 2.0 ** 14), (0.75, 2.0 ** 15)):
        s = nb.pow2_scale(amax)
        assert s == want, (amax, s, want)
        if 1e-10 < amax < 1e10:
            assert 2.0 ** 14 <= float(torch.tensor(amax, dtype=F32)) * s < 2.0 ** 15
        # the bit arithmetic of pd_pow2_scale, as a second opinion
        e = (int(torch.tensor(amax, dtype=F32).view(torch.int32)) >> 23) & 0xff
        assert s == 2.0 ** (268 - min(max(e, 87), 200) - 127)


# ------------------------------------------------------------------ the conditions the GPU cases rely on
def test_rows_hold_the_four_kinds():
    for M, C in ((63, 12), (65, 128), (333, 1024), (4, 128)):
        x, k = gk.rows(M, C, "mix", 5)
        assert set(k.tolist()) == {0, 1, 2, 3}
        xd = x.double()
        const, zero, off, normal = xd[k == 2], xd[k == 3], xd[k == 1], xd[k == 0]
        assert bool((const.max(-1).values == const.min(-1).values).all()) and bool((const[:, 0] != 0).all())
        assert len(set(const[:, 0].tolist())) > 1 or M == 4
        assert bool((zero == 0).all())
        assert bool((off.mean(-1).abs() / off.std(-1, unbiased=False) >= 1e4).all())
        assert bool((normal.std(-1) > 0.1).all())
    for i, kind in enumerate(gk.KINDS):
        assert gk.row_kinds(1) == gk.KINDS and gk.rows(1, 24, kind, 5)[1].tolist() == [i]
    x, k = gk.rowstats_case(63, 12, "mix")
    assert x.dtype == F32 and k.shape == (63,)
    # a zero row with eps = 1e-8: rstd = 1e4
    mean, rstd = nb.rowstats64(torch.zeros(2, 8), RMS, 1e-8)
    assert torch.equal(mean, torch.zeros(2, dtype=F64)) and torch.allclose(rstd, torch.full((2,), 1e4, dtype=F64), rtol=1e-12)


def _lanes_per_row(C):                                      # the launcher's rule: one float4 per lane while the row fits a wave
    n, lpr = C // 4, 4
    while lpr < 64 and (lpr * 4 < n or lpr * 2 <= n):
        lpr *= 2
    return lpr


def test_norm_shapes_reach_every_instantiation():
    lpr = {C: _lanes_per_row(C) for C in gk.NORM_C}
    assert set(lpr.values()) == {4, 8, 16, 32, 64}
    assert lpr == {4: 4, 12: 4, 24: 4, 40: 8, 96: 16, 128: 32, 384: 64, 768: 64, 1024: 64}
    idle = {C for C in gk.NORM_C if (C // 4) % lpr[C] != 0}
    assert idle == {4, 12, 24, 40, 96, 384}                                       # a last chunk slot that only some lanes of the row fill
    assert (768 // 4) == 3 * lpr[768] and (1024 // 4) == 4 * lpr[1024]            # 768: the fourth slot of every lane stays empty
    assert _lanes_per_row(1028) * 4 < 1028 // 4 and max(gk.NORM_C) == 1024
    for C in gk.NORM_C:
        rpb = 256 // lpr[C]
        assert any(M % rpb for M in gk.ROWSTATS_M) and any(M % rpb for M in gk.ROWNORM_M)      # a last block with dead rows
        assert any(M > rpb for M in gk.ROWSTATS_M)                                              # and more than one block
    assert all(C % 32 == 0 for C in gk.SPLIT_C) and {_lanes_per_row(C) for C in gk.SPLIT_C} == {8, 16, 64}
    assert 1 in gk.KMAJOR_M and any(M > 256 for M in gk.KMAJOR_M) and any(M % 256 for M in gk.KMAJOR_M)
    # every activation, res / w / b each present and absent, both modes, and the in-place form
    acts = {c[0] for c in gk.ROWNORM_CFGS}
    assert acts == {0, 1, 2, 3} and {c[4] for c in gk.ROWNORM_CFGS} == {RMS, LN} and any(c[5] for c in gk.ROWNORM_CFGS)
    assert {c[1:4] for c in gk.ROWNORM_CFGS} == {(r, w, b) for r in (False, True) for w in (False, True) for b in (False, True)}


def test_norm_split_cases():
    c = gk.norm_split_case(200, 96)
    assert c["tab"].shape == (4, 192) and 200 % gk.GROUP_ROWS == 8                 # four groups, the last ragged
    assert gk.norm_split_case(65, 96)["tab"].shape[0] == 2 and gk.norm_split_case(1, 96)["tab"].shape[0] == 1
    tab = c["tab"]
    assert float((tab[1:] - tab[:-1]).abs().min()) > 0                            # no two groups share a gain or a shift
    assert float((tab[:, 96:] - 1).abs().max()) < 2 and float(tab[:, :96].abs().max()) < 1      # shift first, gain second
    assert {cfg[0] for cfg in gk.SPLIT_CFGS} == {0, 32} and {cfg[1] for cfg in gk.SPLIT_CFGS} == {0, "M", 64}
    assert {cfg[3] for cfg in gk.SPLIT_CFGS} == {"wb", "w", "b", ""}
    amax = [cfg[4] for cfg in gk.SPLIT2_CFGS]
    assert set(amax) == {40.0, 32.0, gk.AMAX_BELOW_32, 1e-20, 1e30} and gk.AMAX_BELOW_32 == 32.0 - 2.0 ** -19
    assert nb.pow2_scale(1e-20) == 2.0 ** 54 and nb.pow2_scale(1e30) == 2.0 ** -59      # both exponent clamps


@pytest.mark.parametrize("C", gk.SPLIT_C)
@pytest.mark.parametrize("M", gk.SPLIT_M)
def test_norm_split2_inputs_stay_below_amax(M, C):
    for cfg in gk.SPLIT2_CFGS:
        tab, scale, ref, bound = gk.norm_split2_expected(M, C, cfg)
        amax = float(torch.tensor(cfg[4], dtype=F32))
        assert scale == nb.pow2_scale(amax)
        assert float(ref.abs().max()) < amax and float(ref.abs().max()) * scale < 2.0 ** 15, (M, C, cfg)
        if cfg[3] == "wb":
            assert float(ref.abs().max()) * scale > 0.9 * min(amax * scale, 2.0 ** 15)      # and reach close to the limit


def test_pair_bias_cases():
    assert {(C, H) for C, H, _, _ in gk.PB_CASES} == {(128, 4), (128, 8), (128, 16), (16, 4), (16, 24)}
    for C, tile in ((128, 8), (16, 32)):
        shapes = gk.PB_SHAPES[C]
        assert all(T2 % 4 == 0 for _, T2 in shapes)
        assert any(T2 < tile and T1 * T2 > tile for T1, T2 in shapes)             # several pair rows in one wave tile, more than one tile
        assert any(T2 < tile and T1 * T2 < tile for T1, T2 in shapes)             # a single ragged tile
        assert any(T2 > tile and T2 % tile for T1, T2 in shapes)                  # tiles that cross a row end at varying offsets
        assert any(T1 > 32 and T2 > 32 for T1, T2 in shapes)                      # more than one fragment tile along both axes
    assert (7, 20) in gk.PB_SHAPES[16] and {(m * 32) % 20 for m in range(5)} == {0, 12, 4, 16, 8}
    for C, H, T1, T2 in gk.PB_GRID_STRIDE:
        assert H == 4 and -(-T1 * T2 // (8 if C == 128 else 32)) > 2048 * 4
    assert 516 * 516 == 266256 and 516 * 516 * 16 * 4 < 17.1e6
    cf = gk.PB_CFGS
    assert {c[0] for c in cf} == {False, True} and {c[1] for c in cf} == {RMS, LN}
    assert {c[2] for c in cf} == {False, True} and {c[3] for c in cf} == {False, True}
    assert {0.0, gk.LOG2E, gk.LOG2E * 128} == {c[4] for c in cf}
    assert {(c[0], c[1]) for c in cf if c[2] and c[3]} == {(t, m) for t in (False, True) for m in (RMS, LN)}
    c = gk.pair_bias_case(16, 24, 7, 20)
    assert c["x"].shape == (140, 16) and c["Wf"].shape == (24, 16) and c["c2"].shape == (24,) and float(c["c2"].abs().min()) > 0


@pytest.mark.parametrize("T1,T2", sorted({s for v in gk.PB_SHAPES.values() for s in v} | {(260, 260), (516, 516), (4, 4), (100, 100)}))
def test_pair_bias_mask(T1, T2):
    for transpose in (False, True):
        nq, nk = (T2, T1) if transpose else (T1, T2)
        m = gk.pair_bias_mask(T1, T2, transpose).reshape(T1, T2)
        grid = m.t() if transpose else m                                          # [query, key]
        assert set(m.unique().tolist()) <= {0.0, 1.0}
        assert bool((grid.sum(1) == nk).any())                                    # a fully live query
        if nq > 1:
            assert bool((grid.sum(1) == 0).any())                                 # a fully masked one
        if nq * nk >= 1000:
            assert 0.05 < float((grid[1:-1] == 0).float().mean()) < 0.15


# ------------------------------------------------------------------ fp32 torch within the bound on every case
@pytest.mark.parametrize("C", gk.NORM_C)
def test_rowstats_fp32_torch_is_within_the_bound(C):
    for M in sorted(set(gk.ROWSTATS_M) | set(gk.KMAJOR_M if C in gk.KMAJOR_C else [])):
        for kind, mode in ((k, m) for k in gk.row_kinds(M) for m in (RMS, LN)):
            x, _ = gk.rowstats_case(M, C, kind)
            ref, bound = gk.rowstats_expected(M, C, kind, mode)
            nb.assert_within_bound("rowstats (torch fp32)", f"M={M} C={C} {kind} mode={mode}", stats32(x, mode), ref, bound)
            # a serial left-to-right sum, the other extreme of the summation orders
            xs = x.clone()
            s1 = torch.zeros(M)
            for c in range(C):
                s1 = s1 + xs[:, c]
            if mode == LN and C <= 128:
                mean = s1 / C
                q = torch.zeros(M)
                for c in range(C):
                    q = q + (xs[:, c] - mean) ** 2
                serial = torch.stack([mean, torch.rsqrt(q / C + EPS[mode])], -1)
                nb.assert_within_bound("rowstats (serial fp32)", f"M={M} C={C} {kind}", serial, ref, bound)


@pytest.mark.parametrize("C", gk.NORM_C)
def test_rownorm_fp32_torch_is_within_the_bound(C):
    for M in gk.ROWNORM_M:
        for kind in gk.row_kinds(M):
            c = gk.rownorm_case(M, C, kind)
            for cfg in gk.ROWNORM_CFGS:
                ref, bound = gk.rownorm_expected(M, C, kind, cfg)
                assert torch.isfinite(bound).all()
                got = nb.rownorm64(**gk.rownorm_args(c, cfg), dtype=F32)
                nb.assert_within_bound("rownorm (torch fp32)", f"M={M} C={C} {kind} {cfg}", got, ref, bound)


@pytest.mark.parametrize("C", gk.SPLIT_C)
@pytest.mark.parametrize("M", gk.SPLIT_M)
def test_norm_split_fp32_torch_is_within_the_bound(M, C):
    c = gk.norm_split_case(M, C)
    for cfg in gk.SPLIT_CFGS:
        ref, bound = gk.norm_split_expected(M, C, cfg)
        got = nb.norm_mod64(**gk._split_args(c, cfg), dtype=F32)
        case = f"M={M} C={C} {cfg}"
        nb.assert_within_bound("norm_split (torch fp32)", case, got, ref, bound)
        h, m, l = nb.split3_bf16(got)
        assert torch.equal(h.double() + m.double() + l.double(), got.double())
        nb.assert_high_part("norm_split (torch fp32)", case, h, ref, bound, "bf16")
    for cfg in gk.SPLIT2_CFGS:
        tab, scale, ref, bound = gk.norm_split2_expected(M, C, cfg)
        got = nb.norm_mod64(**gk._split_args(c, cfg, tab), dtype=F32) * scale
        h, l = nb.split2_f16(got)
        case = f"M={M} C={C} {cfg}"
        nb.assert_within_bound("norm_split2 (torch fp32)", case, (h.double() + l.double()) / scale, ref,
                               bound + nb.split2_bound(ref.abs() * scale + bound * scale) / scale)
        nb.assert_high_part("norm_split2 (torch fp32)", case, h, ref * scale, bound * scale, "fp16")
        assert float(h.abs().max()) < 2.0 ** 15


@pytest.mark.parametrize("C,H,T1,T2", gk.PB_CASES + gk.PB_GRID_STRIDE)
def test_pair_bias_fp32_torch_is_within_the_bound(C, H, T1, T2):
    for cfg in (gk.PB_CFGS if (C, H, T1, T2) in gk.PB_CASES else gk.PB_CFGS_GRID_STRIDE):
        kw = gk.pair_bias_args(C, H, T1, T2, cfg)
        ref, bound, real = gk.pair_bias_expected(C, H, T1, T2, cfg)
        assert int(real.sum()) == H * T1 * T2 and torch.isfinite(bound).all()
        got, _ = nb.bias_frag_scatter(nb.pair_bias64(**kw, dtype=F32))
        nb.assert_within_bound("pair_bias (torch fp32)", f"C={C} H={H} T1={T1} T2={T2} {cfg}", got[real], ref[real], bound[real])


@pytest.mark.parametrize("T", gk.PBS_T)
def test_z2_fp32_torch_is_within_the_bound(T):
    x = gk.pair_bias_case(128, 4, T, T)["x"]
    _, rstd = nb.rowstats64(x, RMS, EPS[RMS], dtype=F32)
    for transpose in (False, True):
        for zn_amax in gk.ZN_AMAX:
            scale, ref, bound = gk.pair_bias_split_expected(T, transpose, zn_amax)
            assert float(ref.abs().max()) < 2.0 ** 15
            z = (x * (rstd * scale)[:, None]).reshape(T, T, 128)
            h, l = nb.split2_f16(z.transpose(0, 1) if transpose else z)
            buf = nb.z2_scatter(h, l, torch.tensor(float("nan"), dtype=torch.float16))
            hi, lo = nb.z2_gather(buf, T)
            nb.assert_within_bound("z2 (torch fp32)", f"T={T} transpose={transpose} zn_amax={zn_amax!r}", hi + lo, ref, bound)
            nb.assert_high_part("z2 (torch fp32)", f"T={T}", hi, ref, bound, "fp16")


# ------------------------------------------------------------------ every wrong variant is rejected on a named case
def test_one_pass_variance_is_rejected_on_the_offset_rows():
    """case: rowstats M = 63, C = 12, LayerNorm - the rows 1000 + 0.01 randn"""
    x, k = gk.rowstats_case(63, 12, "mix")
    ref, bound = gk.rowstats_expected(63, 12, "mix", LN)
    off = k == 1
    mean = x.mean(-1)
    one_pass = torch.stack([mean, torch.rsqrt(((x * x).mean(-1) - mean * mean).clamp(min=0) + EPS[LN])], -1)
    nb.assert_within_bound("rowstats (two-pass fp32)", "offset rows", stats32(x, LN)[off], ref[off], bound[off])
    assert rejected("rowstats (one-pass variance)", "M=63 C=12 offset rows", one_pass[off], ref[off], bound[off])
    assert bool((bound[off][:, 1] < 0.25 * ref[off][:, 1]).all())                 # the bound on these rows is the chain's, not the trivial one
    # and through the normalised value: rownorm M = 65, C = 12
    c = gk.rownorm_case(65, 12, "mix")
    cfg = (ACT_NONE, False, False, False, LN, False)
    kw = gk.rownorm_args(c, cfg)
    x = c["x"]
    mean = x.mean(-1, keepdim=True)
    y = (x - mean) * torch.rsqrt(((x * x).mean(-1, keepdim=True) - mean * mean).clamp(min=0) + EPS[LN])
    assert rejected("rownorm (one-pass variance)", "M=65 C=12", y, nb.rownorm64(**kw), nb.rownorm_bound(**kw))


def test_divisor_c_minus_one_is_rejected():
    """case: rowstats M = 333, C = 1024 (where 1 / (C - 1) is closest to 1 / C), LayerNorm"""
    for C in (4, 1024):
        x, k = gk.rowstats_case(333, C, "mix")
        ref, bound = gk.rowstats_expected(333, C, "mix", LN)
        xd = x.double()
        wrong = torch.stack([xd.mean(-1), torch.rsqrt(xd.var(-1, unbiased=True) + EPS[LN])], -1)
        assert rejected("rowstats (divisor C - 1)", f"M=333 C={C}", wrong.float(), ref, bound)
        assert rejected("rowstats (divisor C - 1)", f"M=333 C={C} ordinary rows", wrong.float()[k == 0], ref[k == 0], bound[k == 0])


def test_dropped_eps_is_rejected_on_the_constant_and_the_zero_rows():
    """case: rowstats M = 65, C = 40 - constant rows (LayerNorm) and all-zero rows (RMS)"""
    x, k = gk.rowstats_case(65, 40, "mix")
    for mode, kind in ((LN, 2), (RMS, 3), (LN, 3)):
        ref, bound = gk.rowstats_expected(65, 40, "mix", mode)
        wrong = torch.stack(nb.rowstats64(x, mode, 0.0), -1)[k == kind]
        assert not torch.isfinite(wrong.float()).all() or float((wrong - ref[k == kind]).abs().max()) > 1e3
        assert rejected("rowstats (no eps)", f"M=65 C=40 kind {kind}", wrong.float(), ref[k == kind], bound[k == kind])
        other = k < 2                                                             # ... and only there: ordinary and offset rows do not see eps
        nb.assert_within_bound("rowstats (no eps)", "M=65 C=40 ordinary rows, RMS", torch.stack(nb.rowstats64(x, RMS, 0.0), -1)[other].float(),
                               gk.rowstats_expected(65, 40, "mix", RMS)[0][other], gk.rowstats_expected(65, 40, "mix", RMS)[1][other])


def test_neighbouring_group_row_is_rejected():
    """case: norm_split M = 200, C = 96, groups of 64 rows - the gain, then the shift, of group g + 1; and groups of 65 rows"""
    c = gk.norm_split_case(200, 96)
    cfg = (0, gk.GROUP_ROWS, LN, "wb")
    ref, bound = gk.norm_split_expected(200, 96, cfg)
    kw = gk._split_args(c, cfg)
    for which in ("w_tab", "b_tab"):
        wrong = nb.norm_mod64(**{**kw, which: kw[which].roll(-1, 0)})
        assert rejected(f"norm_split ({which} of the next group)", "M=200 C=96", wrong.float(), ref, bound)
    wrong = nb.norm_mod64(**{**kw, "rows_per_group": gk.GROUP_ROWS + 1})
    assert rejected("norm_split (row / (rows_per_group + 1))", "M=200 C=96", wrong.float(), ref, bound)
    assert rejected("norm_split (row / (rows_per_group + 1))", "M=65 C=96", nb.norm_mod64(**{**gk._split_args(gk.norm_split_case(65, 96), cfg),
                    "rows_per_group": gk.GROUP_ROWS + 1}).float(), *gk.norm_split_expected(65, 96, cfg))


def test_rms_in_the_place_of_layernorm_is_rejected():
    """case: rownorm M = 65, C = 40, LayerNorm, every activation"""
    c = gk.rownorm_case(65, 40, "mix")
    for cfg in (cf for cf in gk.ROWNORM_CFGS if cf[4] == LN):
        ref, bound = gk.rownorm_expected(65, 40, "mix", cfg)
        wrong = nb.rownorm64(**{**gk.rownorm_args(c, cfg), "mode": RMS})
        assert rejected("rownorm (RMS for LN)", f"M=65 C=40 {cfg}", wrong.float(), ref, bound)


def test_activation_after_the_residual_is_rejected():
    """case: rownorm M = 65, C = 24, every activation but none, res present"""
    c = gk.rownorm_case(65, 24, "mix")
    for cfg in (cf for cf in gk.ROWNORM_CFGS if cf[0] != ACT_NONE and cf[1]):
        ref, bound = gk.rownorm_expected(65, 24, "mix", cfg)
        kw = gk.rownorm_args(c, cfg)
        wrong = nb._act64(nb.rownorm64(**{**kw, "act": ACT_NONE}), cfg[0])
        assert rejected("rownorm (act after res)", f"M=65 C=24 {cfg}", wrong.float(), ref, bound)


def test_swapped_pair_indices_are_rejected():
    """case: pair_bias C = 128, H = 4, T1 = T2 = 36 (the square shape of pd_pair_bias_split), both stores"""
    for transpose in (False, True):
        cfg = gk.pair_bias_split_cfg(transpose)
        ref, bound, real = gk.pair_bias_expected(128, 4, 36, 36, cfg)
        kw = gk.pair_bias_args(128, 4, 36, 36, cfg)
        wrong, _ = nb.bias_frag_scatter(nb.pair_bias64(**{**kw, "transpose": not transpose}))
        assert rejected("pair_bias (i <-> j)", f"T=36 transpose={transpose}", wrong.float()[real], ref[real], bound[real])
        live = ref.abs() < 1e8                                                    # also without the help of the mask
        assert rejected("pair_bias (i <-> j)", f"T=36 transpose={transpose} live", wrong.float()[real & live], ref[real & live], bound[real & live])
        # the same in z2: batch and row exchanged
        scale, zref, zbound = gk.pair_bias_split_expected(36, transpose, 16.0)
        assert rejected("z2 (batch <-> row)", "T=36", zref.transpose(0, 1).float(), zref, zbound)


def test_row_ij_without_the_short_row_branch_is_rejected():
    """case: pair_bias C = 16, (T1, T2) = (9, 4) and (7, 20): (i, j) of a tile row taken as (tq + [rr >= T2], rr - [rr >= T2] T2).
    (At C = 128 the tile has 8 rows and T2 % 4 == 0 leaves T2 = 4 as the only shorter row: two whole rows per tile, for which the
    first form is right as well - there the distinction cannot be observed.)"""
    for C, H, T1, T2, tile in ((16, 4, 9, 4, 32), (16, 4, 7, 20, 32)):
        cfg = gk.PB_CFGS[0]
        kw = gk.pair_bias_args(C, H, T1, T2, cfg)
        ref, bound, real = gk.pair_bias_expected(C, H, T1, T2, cfg)
        rows = nb.pair_bias64(**kw).permute(1, 2, 0).reshape(T1 * T2, H)
        m = torch.arange(T1 * T2)
        m0 = (m // tile) * tile
        rr = m0 % T2 + (m - m0)
        dq = (rr >= T2).long()
        i, j = m0 // T2 + dq, rr - dq * T2
        keep = (i < T1) & (j < T2) & (j >= 0)
        assert not bool(keep.all()) or not torch.equal(i * T2 + j, m)
        frag = torch.full((ref.numel(),), float("nan"), dtype=F64)
        idx = nb.bias_frag_index(H, T1, T2)
        frag[idx[:, i[keep], j[keep]].reshape(-1)] = rows[keep].t().reshape(-1)
        assert rejected("pair_bias (row_ij, first form only)", f"C={C} T1={T1} T2={T2}", frag.float()[real], ref[real], bound[real])


def test_mask_after_the_scale_is_rejected():
    """case: pair_bias C = 16, H = 24, (7, 20), LayerNorm, out_scale = 128 log2 e"""
    cfg = gk.PB_CFGS[2]
    assert cfg[1] == LN and cfg[3] and cfg[4] == gk.LOG2E * 128
    kw = gk.pair_bias_args(16, 24, 7, 20, cfg)
    ref, bound, real = gk.pair_bias_expected(16, 24, 7, 20, cfg)
    unmasked = nb.pair_bias64(**{**kw, "mask": None})
    madd = nb.pair_bias64(**{**kw, "out_scale": 1.0}) - nb.pair_bias64(**{**kw, "mask": None, "out_scale": 1.0})
    wrong, _ = nb.bias_frag_scatter(unmasked + madd)
    assert rejected("pair_bias (mask after out_scale)", "C=16 H=24 7x20", wrong.float()[real], ref[real], bound[real])


def test_omitted_c2_is_rejected():
    """case: pair_bias C = 16, H = 24, (7, 20) and C = 128, H = 16, (5, 12), LayerNorm"""
    for C, H, T1, T2 in ((16, 24, 7, 20), (128, 16, 5, 12)):
        cfg = gk.PB_CFGS[3]
        assert cfg[1] == LN
        kw = gk.pair_bias_args(C, H, T1, T2, cfg)
        ref, bound, real = gk.pair_bias_expected(C, H, T1, T2, cfg)
        wrong, _ = nb.bias_frag_scatter(nb.pair_bias64(**{**kw, "c2": None}))
        assert rejected("pair_bias (no c2)", f"C={C} H={H}", wrong.float()[real], ref[real], bound[real])


def test_truncated_high_part_is_rejected():
    """case: norm_split M = 65, C = 96 (bf16) and norm_split2 M = 65, C = 96, amax = 40 (fp16)"""
    c = gk.norm_split_case(65, 96)
    cfg = gk.SPLIT_CFGS[1]
    ref, bound = gk.norm_split_expected(65, 96, cfg)
    got = nb.norm_mod64(**gk._split_args(c, cfg), dtype=F32)
    trunc = (got.view(torch.int32) & -65536).view(F32)
    nb.assert_high_part("norm_split", "rounded", nb.split3_bf16(got)[0], ref, bound, "bf16")
    with pytest.raises(AssertionError):
        nb.assert_high_part("norm_split (high part truncated)", "M=65 C=96", trunc, ref, bound, "bf16")
    cfg2 = gk.SPLIT2_CFGS[1]
    tab, scale, ref, bound = gk.norm_split2_expected(65, 96, cfg2)
    got = nb.norm_mod64(**gk._split_args(c, cfg2, tab), dtype=F32) * scale
    trunc = (got.view(torch.int32) & -8192).view(F32)                              # 13 of the 23 fraction bits dropped (values are normal in fp16)
    with pytest.raises(AssertionError):
        nb.assert_high_part("norm_split2 (high part truncated)", "M=65 C=96", trunc, ref * scale, bound * scale, "fp16")
    # a high part two steps away is no neighbour
    with pytest.raises(AssertionError):
        far = nb.split3_bf16(gk.norm_split_case(65, 96)["x"])[0] * 0 + nb.round_to(gk.norm_split_expected(65, 96, cfg)[0], "bf16").float() * (1 + 2.0 ** -6)
        nb.assert_high_part("norm_split (two steps off)", "M=65 C=96", far, *gk.norm_split_expected(65, 96, cfg), "bf16")


def test_operand_scale_off_by_two_at_a_power_of_two_is_rejected():
    """case: norm_split2 M = 65, C = 96, amax = 32.0 and z2 T = 36, zn_amax = 16.0 - the scale of floor(log2) + 1 (right for every
    amax that is no power of two when computed as ceil)"""
    c = gk.norm_split_case(65, 96)
    cfg = next(cf for cf in gk.SPLIT2_CFGS if cf[4] == 32.0)
    tab, scale, ref, bound = gk.norm_split2_expected(65, 96, cfg)
    assert scale == 2.0 ** 9
    for wrong_scale in (scale * 2, scale / 2):
        h, l = nb.split2_f16(nb.norm_mod64(**gk._split_args(c, cfg, tab), dtype=F32) * wrong_scale)
        assert rejected("norm_split2 (scale off by two)", "M=65 C=96 amax=32", (h.double() + l.double()) / scale, ref,
                        bound + nb.split2_bound(ref.abs() * scale + bound * scale) / scale)
    scale, zref, zbound = gk.pair_bias_split_expected(36, False, 16.0)
    assert scale == 2.0 ** 10
    assert rejected("z2 (scale off by two)", "T=36 zn_amax=16", (zref / 2).float(), zref, zbound)
    # the neighbouring float of the power of two takes the next scale: the two cases differ by exactly that factor
    assert gk.pair_bias_split_expected(36, False, gk.ZN_AMAX[2])[0] == 2 * scale


def test_stale_and_stray_fragment_slots_are_rejected():
    """a real slot never written (NaN) fails the bounded comparison; the GPU tests check the pad slots with isnan / torch.equal"""
    cfg = gk.PB_CFGS[0]
    ref, bound, real = gk.pair_bias_expected(128, 4, 5, 12, cfg)
    stale = ref.clone()
    stale[int(torch.nonzero(real)[7])] = float("nan")
    assert rejected("pair_bias (slot never written)", "5x12", stale.float()[real], ref[real], bound[real])
    assert int((~real).sum()) == ref.numel() - 4 * 5 * 12 > 0
