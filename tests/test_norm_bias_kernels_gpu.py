"""Kernel-level parity of the row-norm kernels (csrc/norm.hip: pd_rowstats, pd_rownorm, pd_norm_split, pd_norm_split2) and of the
pair-bias kernels (csrc/pairbias.hip: pd_pair_bias, pd_pair_bias_split), straight on the C ABI, against the float64 references and the
derived per-element bounds of tests/norm_bias_ref.py (nb.assert_within_bound prints the worst |error| / bound of every comparison;
pytest -s).  Exact expectations (the three bf16 parts of pd_norm_split, the bias and statistics of the split variant, every slot a
kernel must leave alone) are compared with torch.equal.

Every buffer a kernel writes is a slice of a larger allocation with a NaN band in front of it and behind it, NaN before the launch;
the two fragment outputs are NaN-filled as a whole: real slots must come back finite and within the bound, every other slot unchanged.

Rows come in four kinds (row_kinds / rows): ordinary, 1000 + 0.01 randn (|mean| / std >= 1e4: a one-pass variance has no correct digit
left), constant (zero variance) and all zero (rstd = eps^-1/2).  A case of four rows or more interleaves them; a single row is run once
per kind.  eps is 1e-8 for RMS and 1e-5 for LayerNorm, as in the model.

The input generators and the ``*_expected`` functions (CPU tensors only, cached: a case and its float64 reference are computed once and
never modified) are imported by tests/test_norm_bias_ref_cpu.py, which asserts the conditions the cases rely on without a GPU.

Not covered: the 64-bit row index of pair_bias_kernel matters beyond 2^31 elements of x (T = 4096 at C = 128: a 8.6 GB operand with
a 34 GB float64 reference), out of reach of a test shape; pd_rowstats with kmajor is tested at the C <= 128 the triangle update uses.
"""
import functools
import itertools
import math

import pytest
import torch

import norm_bias_ref as nb
from norm_bias_ref import ACT_NONE, ACT_SIGMOID, ACT_SILU, LN, RMS

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN = float("nan")
BAND = 64                               # elements of NaN in front of and behind every written buffer (16-byte aligned for 2- and 4-byte types)
EPS = {RMS: float(torch.tensor(1e-8, dtype=torch.float32)), LN: float(torch.tensor(1e-5, dtype=torch.float32))}      # the floats the C ABI receives
LOG2E = 1.4426950408889634
MASKVAL = -1e9


# ------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module")
def L():
    from physdock_amd import ops
    return ops._lib.init()


def P(t):
    from physdock_amd import ops
    return ops.ptr(t)


def S():
    from physdock_amd import ops
    return ops.stream()


def ok(rc, what):
    from physdock_amd import ops
    ops.check(rc, what)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def dev(t):
    return None if t is None else t.cuda().contiguous()


def guarded(shape, init=None, dtype=torch.float32):
    """(allocation, view): a device buffer of `shape` with BAND NaNs on either side; the view holds `init` (a CPU tensor) or NaN"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * BAND,), NAN, device="cuda", dtype=dtype)
    view = buf[BAND:BAND + n].view(*shape)
    if init is not None:
        view.copy_(init)
    return buf, view


def bands_intact(buf):
    torch.cuda.synchronize()
    return bool(torch.isnan(buf[:BAND]).all() and torch.isnan(buf[-BAND:]).all())


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def padded(x, pad, lead):
    """x [M, C] as a column slice of a NaN-filled [M, C + pad] device array, `lead` NaN columns in front of it"""
    if pad == 0:
        return dev(x)
    wide = torch.full((x.shape[0], x.shape[1] + pad), NAN)
    wide[:, lead:lead + x.shape[1]] = x
    return dev(wide)[:, lead:]


# ------------------------------------------------------------------ rows of the four kinds
KINDS = ("normal", "offset", "const", "zero")


def row_kinds(M):
    return ("mix",) if M >= 4 else KINDS


def rows(M, C, kind, seed):
    """(x [M, C], kind index per row); "mix": row r has kind (r + r // 4) % 4"""
    g = gen(seed)
    r = torch.arange(M)
    normal = 2 * torch.randn(M, C, generator=g) * torch.exp(0.5 * torch.randn(M, 1, generator=g)) + 0.5
    offset = 1000 + 0.01 * torch.randn(M, C, generator=g)
    const = (0.7 * (1 + r % 5) * (1 - 2 * (r % 2)))[:, None].expand(M, C)
    k = (r + r // 4) % 4 if kind == "mix" else torch.full((M,), KINDS.index(kind))
    x = torch.where((k == 0)[:, None], normal, torch.where((k == 1)[:, None], offset, torch.where((k == 2)[:, None], const, torch.zeros(()))))
    return x.contiguous(), k


# ------------------------------------------------------------------ pd_rowstats
ROWSTATS_M = [1, 63, 65, 333]            # one row; 63 / 65 / 333: a last block with dead rows for every lanes-per-row choice
NORM_C = [4, 12, 24, 40, 96, 128, 384, 768, 1024]      # lanes per row 4, 4, 4, 8, 16, 32, 64, 64, 64; lanes without a chunk at 4, 12, 24, 40, 96, 384; 768: three of the four chunk slots
KMAJOR_M, KMAJOR_C = [1, 255, 257], [4, 32, 128]


@functools.lru_cache(maxsize=None)
def rowstats_case(M, C, kind):
    return rows(M, C, kind, 11 + 7 * M + C)


@functools.lru_cache(maxsize=None)
def rowstats_expected(M, C, kind, mode):
    """(reference, bound) as [M, 2] = (mean, rstd) pairs"""
    x, _ = rowstats_case(M, C, kind)
    return torch.stack(nb.rowstats64(x, mode, EPS[mode]), -1), torch.stack(nb.rowstats_bound(x, mode, EPS[mode]), -1)


@pytest.mark.parametrize("C", NORM_C)
@pytest.mark.parametrize("M", ROWSTATS_M)
def test_rowstats(L, M, C):
    for kind, pad, mode in itertools.product(row_kinds(M), (0, 8), (RMS, LN)):
        x, _ = rowstats_case(M, C, kind)
        ref, bound = rowstats_expected(M, C, kind, mode)
        xd = padded(x, pad, 4)
        buf, st = guarded((M, 2))
        ok(L.pd_rowstats(P(xd), P(st), M, C, C + pad, 0, mode, EPS[mode], S()), "pd_rowstats")
        assert bands_intact(buf)
        nb.assert_within_bound("rowstats", f"M={M} C={C} {kind} ldx=C+{pad} mode={mode}", st.cpu(), ref, bound)
        if mode == RMS:
            assert torch.equal(st.cpu()[:, 0], torch.zeros(M))


@pytest.mark.parametrize("C", KMAJOR_C)
@pytest.mark.parametrize("M", KMAJOR_M)
def test_rowstats_kmajor(L, M, C):
    """x [C][M] with the row index fastest (colstats_kernel), ldx = M and ldx = M + 3 with NaN behind the rows"""
    for kind, pad, mode in itertools.product(row_kinds(M), (0, 3), (RMS, LN)):
        x, _ = rowstats_case(M, C, kind)
        ref, bound = rowstats_expected(M, C, kind, mode)
        xt = torch.full((C, M + pad), NAN)
        xt[:, :M] = x.t()
        xd = dev(xt)
        buf, st = guarded((M, 2))
        ok(L.pd_rowstats(P(xd), P(st), M, C, M + pad, 1, mode, EPS[mode], S()), "pd_rowstats kmajor")
        assert bands_intact(buf)
        nb.assert_within_bound("rowstats kmajor", f"M={M} C={C} {kind} ldx=M+{pad} mode={mode}", st.cpu(), ref, bound)


def test_rowstats_zero_row_gives_the_reciprocal_root_of_eps(L):
    x = torch.zeros(5, 128, device="cuda")
    buf, st = guarded((5, 2))
    ok(L.pd_rowstats(P(x), P(st), 5, 128, 128, 0, RMS, 1e-8, S()), "pd_rowstats")
    assert bands_intact(buf)
    want = torch.tensor([0.0, 1e4], dtype=torch.float64).expand(5, 2)
    nb.assert_within_bound("rowstats", "all-zero rows, eps 1e-8", st.cpu(), want, torch.stack(nb.rowstats_bound(x.cpu(), RMS, 1e-8), -1))


def test_rowstats_refusals(L):
    x = torch.zeros(8, 1032, device="cuda")
    buf, st = guarded((8, 2))
    call = lambda xp, sp, M, C, ldx: L.pd_rowstats(xp, sp, M, C, ldx, 0, LN, 1e-5, S())
    assert call(P(x), P(st), 8, 1028, 1028) == PD_ERR_UNSUPPORTED          # more than 64 lanes x 4 float4
    assert call(P(x), P(st), 8, 1024, 1024) == 0                            # the limit itself is served
    torch.cuda.synchronize()
    assert torch.isfinite(st).all()
    st.fill_(NAN)
    assert call(P(x), P(st), 8, 6, 8) == PD_ERR_UNSUPPORTED                 # C % 4
    assert call(P(x), P(st), 8, 8, 10) == PD_ERR_UNSUPPORTED                # ldx % 4
    assert call(P(x) + 4, P(st), 8, 8, 8) == PD_ERR_UNSUPPORTED             # x not 16-byte aligned
    assert call(P(x), P(st), 0, 8, 8) == PD_ERR_ARG
    assert call(None, P(st), 8, 8, 8) == PD_ERR_ARG
    assert call(P(x), None, 8, 8, 8) == PD_ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


# ------------------------------------------------------------------ pd_rownorm
ROWNORM_M = [1, 65, 333]
#: (act, res, w, b, mode, res aliases y): every activation with everything present in both modes; every other presence pattern of
#: res / w / b; the engine's in-place form y = res
ROWNORM_CFGS = [(act, True, True, True, mode, False) for act in range(4) for mode in (RMS, LN)] \
    + [(ACT_SILU, r, w, b, (RMS, LN)[i % 2], False) for i, (r, w, b) in enumerate(itertools.product((False, True), repeat=3)) if not (r and w and b)] \
    + [(ACT_NONE, True, True, False, RMS, True), (ACT_SIGMOID, True, True, True, LN, True)]


@functools.lru_cache(maxsize=None)
def rownorm_case(M, C, kind):
    g = gen(21 + 5 * M + C)
    x, _ = rows(M, C, kind, 23 + 5 * M + C)
    return dict(x=x, res=torch.randn(M, C, generator=g), w=1 + 0.3 * torch.randn(C, generator=g), b=0.2 * torch.randn(C, generator=g))


def rownorm_args(c, cfg):
    act, r, w, b, mode, _ = cfg
    return dict(x=c["x"], res=c["res"] if r else None, w=c["w"] if w else None, b=c["b"] if b else None, mode=mode, eps=EPS[mode], act=act)


@functools.lru_cache(maxsize=None)
def rownorm_expected(M, C, kind, cfg):
    kw = rownorm_args(rownorm_case(M, C, kind), cfg)
    return nb.rownorm64(**kw), nb.rownorm_bound(**kw)


@pytest.mark.parametrize("C", NORM_C)
@pytest.mark.parametrize("M", ROWNORM_M)
def test_rownorm(L, M, C):
    for kind in row_kinds(M):
        c = rownorm_case(M, C, kind)
        x, res, w, b = dev(c["x"]), dev(c["res"]), dev(c["w"]), dev(c["b"])
        for cfg in ROWNORM_CFGS:
            act, hr, hw, hb, mode, alias = cfg
            ref, bound = rownorm_expected(M, C, kind, cfg)
            buf, y = guarded((M, C), c["res"] if alias else None)
            rp = P(y) if alias else (P(res) if hr else None)
            ok(L.pd_rownorm(P(x), P(y), rp, P(w) if hw else None, P(b) if hb else None, M, C, mode, EPS[mode], act, S()), "pd_rownorm")
            assert bands_intact(buf)
            nb.assert_within_bound("rownorm", f"M={M} C={C} {kind} act={act} res={hr} w={hw} b={hb} mode={mode} alias={alias}",
                                   y.cpu(), ref, bound)
        assert torch.equal(x.cpu(), c["x"]) and torch.equal(res.cpu(), c["res"])


def test_rownorm_refusals(L):
    x = torch.zeros(8, 1032, device="cuda")
    buf, y = guarded((8, 1032))
    call = lambda xp, yp, M, C: L.pd_rownorm(xp, yp, None, None, None, M, C, LN, 1e-5, 0, S())
    assert call(P(x), P(y), 8, 1028) == PD_ERR_UNSUPPORTED
    assert call(P(x), P(y), 8, 6) == PD_ERR_UNSUPPORTED
    assert call(P(x) + 4, P(y), 8, 8) == PD_ERR_UNSUPPORTED
    assert call(P(x), P(y), 0, 8) == PD_ERR_ARG
    assert call(None, P(y), 8, 8) == PD_ERR_ARG
    assert call(P(x), None, 8, 8) == PD_ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


# ------------------------------------------------------------------ pd_norm_split, pd_norm_split2
SPLIT_M, SPLIT_C = [1, 65, 200], [32, 96, 512, 1024]     # C 32 / 96: lanes per row 8 / 16 (96 with idle lanes); 65, 200: ragged last block
GROUP_ROWS = 64                                          # M = 200: four groups, the last of 8 rows; M = 65: two, the last of one row
#: (ldx - C, rows per group (0, "M" or 64), mode, which of the gain w and the shift b are passed)
SPLIT_CFGS = [(pad, rpg, mode, "wb") for pad in (0, 32) for rpg in (0, "M", GROUP_ROWS) for mode in (RMS, LN)] \
    + [(0, GROUP_ROWS, LN, "b"), (32, GROUP_ROWS, RMS, "w"), (0, 0, LN, "")]
#: exact power of two, the float below it, a loose bound, and both clamps of the exponent of pd_pow2_scale
AMAX_BELOW_32 = float(torch.nextafter(torch.tensor(32.0), torch.tensor(0.0)))
SPLIT2_CFGS = [cfg + (40.0,) for cfg in SPLIT_CFGS] + [(0, GROUP_ROWS, LN, "wb", a) for a in (32.0, AMAX_BELOW_32, 1e-20, 1e30)]


@functools.lru_cache(maxsize=None)
def norm_split_case(M, C):
    """x (the four kinds of rows) and the modulation table as the engine lays it out: one row of 2 C floats per group, the shift in the
    first C, the gain in the second (gstride = 2 C)"""
    g = gen(31 + 3 * M + C)
    x, _ = rows(M, C, "mix" if M >= 4 else "normal", 37 + 3 * M + C)
    G = -(-M // GROUP_ROWS)
    tab = torch.cat([0.2 * torch.randn(G, C, generator=g), 1 + 0.3 * torch.randn(G, C, generator=g)], 1)
    return dict(x=x, tab=tab)


def _split_args(c, cfg, tab=None):
    _, rpg, mode, wb = cfg[:4]
    M, C = c["x"].shape
    tab = c["tab"] if tab is None else tab
    return dict(x=c["x"], w_tab=tab[:, C:] if "w" in wb else None, b_tab=tab[:, :C] if "b" in wb else None,
                rows_per_group=M if rpg == "M" else rpg, mode=mode, eps=EPS[mode])


@functools.lru_cache(maxsize=None)
def norm_split_expected(M, C, cfg):
    kw = _split_args(norm_split_case(M, C), cfg)
    return nb.norm_mod64(**kw), nb.norm_mod_bound(**kw)


@functools.lru_cache(maxsize=None)
def norm_split2_expected(M, C, cfg):
    """(table, scale, reference, bound of the evaluation): the table is rescaled (where both gain and shift are passed) so that the
    largest |a'| sits 2 % below the smaller of amax and 2^15 / scale - the latter matters where the exponent clamp makes the scale
    smaller than amax asks for"""
    c = norm_split_case(M, C)
    amax = cfg[4]
    scale = nb.pow2_scale(amax)
    tab = c["tab"]
    if cfg[3] == "wb":
        y0 = nb.norm_mod64(**_split_args(c, cfg))
        tab = (tab.double() * (0.98 * min(float(torch.tensor(amax, dtype=torch.float32)), 2.0 ** 15 / scale) / float(y0.abs().max()))).float()
    kw = _split_args(c, cfg, tab)
    return tab, scale, nb.norm_mod64(**kw), nb.norm_mod_bound(**kw)


def _launch_split(L, which, c, cfg, tab, out, amax=None):
    pad, rpg, mode, wb = cfg[:4]
    M, C = c["x"].shape
    xd, td = padded(c["x"], pad, 16), dev(tab)
    wp = td.data_ptr() + 4 * C if "w" in wb else None
    bp = td.data_ptr() if "b" in wb else None
    rpg = M if rpg == "M" else rpg
    if which == 3:
        rc = L.pd_norm_split(P(xd), C + pad, M, C, mode, EPS[mode], wp, bp, rpg, 2 * C, P(out), S())
    else:
        rc = L.pd_norm_split2(P(xd), C + pad, M, C, mode, EPS[mode], wp, bp, rpg, 2 * C, P(amax), P(out), S())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("C", SPLIT_C)
@pytest.mark.parametrize("M", SPLIT_M)
def test_norm_split(L, M, C):
    c = norm_split_case(M, C)
    for cfg in SPLIT_CFGS:
        ref, bound = norm_split_expected(M, C, cfg)
        buf, out = guarded((3, M, C), dtype=torch.bfloat16)
        ok(_launch_split(L, 3, c, cfg, c["tab"], out), "pd_norm_split")
        assert bands_intact(buf)
        parts = out.cpu().float()                                                # planes at [p][M][C]
        case = f"M={M} C={C} ldx=C+{cfg[0]} rows_per_group={cfg[1]} mode={cfg[2]} given={cfg[3]!r}"
        total = parts.double().sum(0)                                            # exact: 3 x 8 significand bits
        nb.assert_within_bound("norm_split", case, total, ref, bound)
        nb.assert_high_part("norm_split", case, parts[0], ref, bound, "bf16")
        h, m, l = nb.split3_bf16(total.float())                                  # the parts are THE error-free split of their sum
        assert torch.equal(total.float().double(), total)
        assert torch.equal(parts[0], h) and torch.equal(parts[1], m) and torch.equal(parts[2], l)


@pytest.mark.parametrize("C", SPLIT_C)
@pytest.mark.parametrize("M", SPLIT_M)
def test_norm_split2(L, M, C):
    c = norm_split_case(M, C)
    for cfg in SPLIT2_CFGS:
        tab, scale, ref, bound = norm_split2_expected(M, C, cfg)
        amax = torch.tensor([cfg[4]], device="cuda")
        buf, out = guarded((2, M, C), dtype=torch.float16)
        ok(_launch_split(L, 2, c, cfg, tab, out, amax), "pd_norm_split2")
        assert bands_intact(buf)
        parts = out.cpu().double()
        case = f"M={M} C={C} ldx=C+{cfg[0]} rows_per_group={cfg[1]} mode={cfg[2]} given={cfg[3]!r} amax={cfg[4]!r}"
        nb.assert_within_bound("norm_split2", case, parts.sum(0) / scale, ref, bound + nb.split2_bound(ref.abs() * scale + bound * scale) / scale)
        nb.assert_high_part("norm_split2", case, parts[0], ref * scale, bound * scale, "fp16")
        assert float(parts[0].abs().max()) < 2.0 ** 15


def test_norm_split_refusals(L):
    x = torch.zeros(8, 64, device="cuda")
    w = torch.ones(72, device="cuda")
    amax = torch.tensor([40.0], device="cuda")
    buf, out = guarded((3, 8, 64), dtype=torch.bfloat16)
    s3 = lambda C, outp, wp, bp, gs: L.pd_norm_split(P(x), 64, 8, C, LN, 1e-5, wp, bp, 0, gs, outp, S())
    s2 = lambda C, outp, wp, bp, gs, ap: L.pd_norm_split2(P(x), 64, 8, C, LN, 1e-5, wp, bp, 0, gs, ap, outp, S())
    for call in (s3, lambda *a: s2(*a, P(amax))):
        assert call(48, P(out), P(w), P(w), 0) == PD_ERR_UNSUPPORTED          # C % 32
        assert call(64, P(out) + 8, P(w), P(w), 0) == PD_ERR_UNSUPPORTED      # out not 16-byte aligned
        assert call(64, P(out), P(w) + 4, P(w), 0) == PD_ERR_UNSUPPORTED      # gain row not 16-byte aligned
        assert call(64, P(out), P(w), P(w) + 4, 0) == PD_ERR_UNSUPPORTED      # shift row
        assert call(64, P(out), P(w), P(w), 6) == PD_ERR_UNSUPPORTED          # gstride % 4
        assert call(64, None, P(w), P(w), 0) == PD_ERR_ARG
    assert s2(64, P(out), P(w), P(w), 0, None) == PD_ERR_ARG                  # no a_amax
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


# ------------------------------------------------------------------ pd_pair_bias
PB_SHAPES = {128: [(1, 4), (3, 4), (5, 12), (33, 36), (40, 72)],      # T2 = 4 < the 8-row tile: two pair rows per wave tile
             16: [(1, 4), (9, 4), (7, 20), (33, 36), (65, 68)]}       # T2 = 4: eight pair rows per 32-row tile; 20: a tile crosses 1 - 2 row ends
PB_CH = [(128, 4), (128, 8), (128, 16), (16, 4), (16, 24)]
PB_CASES = [(C, H, T1, T2) for C, H in PB_CH for T1, T2 in PB_SHAPES[C]]
PB_GRID_STRIDE = [(128, 4, 260, 260), (16, 4, 516, 516)]             # more tiles than 2048 blocks x 4 waves hold
#: (transpose, mode, stats_out given, maskadd given, out_scale); out_scale 0 means 1
PB_CFGS = [(False, RMS, True, True, LOG2E), (True, RMS, True, True, LOG2E * 128), (False, LN, True, True, LOG2E * 128),
           (True, LN, True, True, LOG2E), (False, RMS, False, False, 0.0), (True, LN, True, False, 0.0), (False, LN, False, True, LOG2E)]
PB_CFGS_GRID_STRIDE = [PB_CFGS[0], PB_CFGS[3]]


@functools.lru_cache(maxsize=None)
def pair_bias_case(C, H, T1, T2):
    """x [T1 * T2, C] of the four kinds of rows; Wf = W diag(w) and c2 = W b as fp32 tensors - the kernel's operands, and the reference's"""
    g = gen(41 + C + 3 * H + 5 * T1 + T2)
    M = T1 * T2
    x, _ = rows(M, C, "mix", 43 + C + 3 * H + 5 * T1 + T2)
    w, b = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    W = torch.randn(H, C, generator=g) / C ** 0.5
    return dict(x=x, Wf=(W * w[None]).contiguous(), c2=(W @ b).contiguous())


@functools.lru_cache(maxsize=None)
def pair_bias_mask(T1, T2, transpose):
    """mask [T1 * T2] in x's row order, built on the (query, key) grid: about 10 % zeros, the last query fully masked, query 0 fully live"""
    nq, nk = (T2, T1) if transpose else (T1, T2)
    m = (torch.rand(nq, nk, generator=gen(47 + 3 * T1 + T2 + int(transpose))) > 0.1).float()
    m[nq - 1] = 0
    m[0] = 1
    return (m.t() if transpose else m).contiguous().reshape(-1)


def pair_bias_args(C, H, T1, T2, cfg):
    transpose, mode, _, with_mask, out_scale = cfg
    c = pair_bias_case(C, H, T1, T2)
    return dict(x=c["x"], Wf=c["Wf"], c2=c["c2"] if mode == LN else None, mask=pair_bias_mask(T1, T2, transpose) if with_mask else None,
                maskval=MASKVAL, out_scale=float(torch.tensor(out_scale, dtype=torch.float32)), T1=T1, T2=T2, transpose=transpose,
                mode=mode, eps=EPS[mode])


@functools.lru_cache(maxsize=None)
def pair_bias_expected(C, H, T1, T2, cfg):
    """(reference, bound, real-slot mask) in the fragment layout, scattered through the independent map"""
    kw = pair_bias_args(C, H, T1, T2, cfg)
    ref, real = nb.bias_frag_scatter(nb.pair_bias64(**kw))
    return ref, nb.bias_frag_scatter(nb.pair_bias_bound(**kw), fill=0.0)[0], real


def _launch_pair_bias(L, kw, C, H, frag, stats, z2=None, zn_amax=None):
    x, Wf, c2, mask = dev(kw["x"]), dev(kw["Wf"]), dev(kw["c2"]), dev(kw["mask"])
    if z2 is None:
        rc = L.pd_pair_bias(P(x), P(Wf), P(c2), P(stats), P(mask), kw["maskval"], kw["out_scale"], P(frag), kw["T1"], kw["T2"], C, H,
                            int(kw["transpose"]), kw["mode"], kw["eps"], S())
    else:
        rc = L.pd_pair_bias_split(P(x), P(Wf), P(c2), P(stats), P(mask), kw["maskval"], kw["out_scale"], P(frag), kw["T1"],
                                  int(kw["transpose"]), kw["eps"], P(z2), zn_amax, S())
    torch.cuda.synchronize()
    return rc


def _check_pair_bias(L, C, H, T1, T2, cfg):
    kw = pair_bias_args(C, H, T1, T2, cfg)
    ref, bound, real = pair_bias_expected(C, H, T1, T2, cfg)
    M = T1 * T2
    fbuf, frag = guarded((ref.numel(),))
    sbuf, st = guarded((M, 2)) if cfg[2] else (None, None)
    ok(_launch_pair_bias(L, kw, C, H, frag, st), "pd_pair_bias")
    assert bands_intact(fbuf)
    out = frag.cpu()
    case = f"C={C} H={H} T1={T1} T2={T2} transpose={cfg[0]} mode={cfg[1]} stats={cfg[2]} mask={cfg[3]} out_scale={cfg[4]:.4g}"
    masked = ref.abs() > 1e8                                  # told apart on the reference: their bound carries u |maskval out_scale|
    nb.assert_within_bound("pair_bias", case, out[real & ~masked], ref[real & ~masked], bound[real & ~masked])
    if bool((real & masked).any()):                           # (a single query with four keys may have none)
        nb.assert_within_bound("pair_bias masked", case, out[real & masked], ref[real & masked], bound[real & masked])
    assert torch.isnan(out[~real]).all(), "a pad slot of the fragment buffer was written"
    if cfg[2]:
        assert bands_intact(sbuf)
        sref, sbound = (torch.stack(t, -1) for t in (nb.rowstats64(kw["x"], cfg[1], kw["eps"]), nb.rowstats_bound(kw["x"], cfg[1], kw["eps"])))
        nb.assert_within_bound("pair_bias statistics", case, st.cpu(), sref, sbound)


@pytest.mark.parametrize("C,H,T1,T2", PB_CASES)
def test_pair_bias(L, C, H, T1, T2):
    for cfg in PB_CFGS:
        _check_pair_bias(L, C, H, T1, T2, cfg)


@pytest.mark.parametrize("C,H,T1,T2", PB_GRID_STRIDE)
def test_pair_bias_grid_stride(L, C, H, T1, T2):
    tile = 8 if C == 128 else 32
    assert -(-T1 * T2 // tile) > 2048 * 4
    for cfg in PB_CFGS_GRID_STRIDE:
        _check_pair_bias(L, C, H, T1, T2, cfg)


def test_pair_bias_refusals(L):
    kw = pair_bias_args(128, 4, 5, 12, PB_CFGS[0])
    x, Wf = dev(kw["x"]), dev(kw["Wf"])
    buf, frag = guarded((nb.bias_frag_numel(24, 12, 12),))
    call = lambda xp, wp, fp, T2, C, H: L.pd_pair_bias(xp, wp, None, None, None, 0.0, 1.0, fp, 5, T2, C, H, 0, RMS, 1e-8, S())
    assert call(P(x), P(Wf), P(frag), 6, 128, 4) == PD_ERR_UNSUPPORTED         # T2 % 4
    assert call(P(x), P(Wf), P(frag), 12, 64, 4) == PD_ERR_UNSUPPORTED
    assert call(P(x), P(Wf), P(frag), 12, 128, 5) == PD_ERR_UNSUPPORTED
    assert call(P(x), P(Wf), P(frag), 12, 16, 8) == PD_ERR_UNSUPPORTED         # H = 8 exists for C = 128 only
    assert call(P(x) + 4, P(Wf), P(frag), 12, 128, 4) == PD_ERR_UNSUPPORTED
    assert call(P(x), P(Wf) + 4, P(frag), 12, 128, 4) == PD_ERR_UNSUPPORTED
    assert call(P(x), P(Wf), P(frag) + 4, 12, 128, 4) == PD_ERR_UNSUPPORTED
    assert call(None, P(Wf), P(frag), 12, 128, 4) == PD_ERR_ARG
    assert call(P(x), P(Wf), None, 12, 128, 4) == PD_ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


# ------------------------------------------------------------------ pd_pair_bias_split
PBS_T = [4, 36, 100]                     # 4: eight batches per 32-row tile slot, rows 4 .. 31 never written; 36, 100: a ragged second / fourth tile
ZN_AMAX = [float(torch.tensor(math.sqrt(128.0), dtype=torch.float32)), 16.0, float(torch.nextafter(torch.tensor(16.0), torch.tensor(0.0)))]


def pair_bias_split_cfg(transpose):
    return (transpose, RMS, True, True, LOG2E * 128)


@functools.lru_cache(maxsize=None)
def pair_bias_split_expected(T, transpose, zn_amax):
    """(scale, reference, bound) [batch, row, 128] of the decoded z2"""
    x = pair_bias_case(128, 4, T, T)["x"]
    scale = nb.pow2_scale(zn_amax)
    return scale, nb.z2_ref64(x, EPS[RMS], scale, T, transpose), nb.z2_bound(x, EPS[RMS], scale, T, transpose)


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("T", PBS_T)
def test_pair_bias_split(L, T, transpose):
    cfg = pair_bias_split_cfg(transpose)
    kw = pair_bias_args(128, 4, T, T, cfg)
    ref, bound, real = pair_bias_expected(128, 4, T, T, cfg)
    fbuf0, frag0 = guarded((ref.numel(),))
    sbuf0, st0 = guarded((T * T, 2))
    ok(_launch_pair_bias(L, kw, 128, 4, frag0, st0), "pd_pair_bias")
    zreal = nb.z2_real(T)
    for zn_amax in ZN_AMAX:
        case = f"T={T} transpose={transpose} zn_amax={zn_amax!r}"
        fbuf, frag = guarded((ref.numel(),))
        sbuf, st = guarded((T * T, 2))
        zbuf, z2 = guarded((nb.z2_numel(T),), dtype=torch.float16)             # the fp16 NaN 0x7e00 in every slot
        before = bits(zbuf).clone()
        ok(_launch_pair_bias(L, kw, 128, 4, frag, st, z2, zn_amax), "pd_pair_bias_split")
        # the bias tiles and the statistics of the split variant are those of pd_pair_bias, bit for bit (pad slots and bands included)
        assert torch.equal(bits(fbuf), bits(fbuf0)) and torch.equal(bits(sbuf), bits(sbuf0))
        live = real & (ref.abs() < 1e8)
        nb.assert_within_bound("pair_bias_split bias", case, frag.cpu()[live], ref[live], bound[live])
        # z2: the real slots decode to xhat * scale, every other slot (bands included) keeps its sentinel
        scale, zref, zbound = pair_bias_split_expected(T, transpose, zn_amax)
        hi, lo = nb.z2_gather(z2.cpu(), T)
        nb.assert_within_bound("pair_bias_split z2", case, hi + lo, zref, zbound)
        nb.assert_high_part("pair_bias_split z2", case, hi, zref, zbound, "fp16")
        keep = torch.ones(zbuf.numel(), dtype=torch.bool)
        keep[BAND:BAND + zreal.numel()] = ~zreal
        assert torch.equal(bits(zbuf).cpu()[keep], before.cpu()[keep]), "a z2 slot of a row beyond T (or outside the buffer) was written"


def test_pair_bias_split_refusals(L):
    kw = pair_bias_args(128, 4, 36, 36, pair_bias_split_cfg(False))
    fbuf, frag = guarded((nb.bias_frag_numel(4, 36, 36),))
    zbuf, z2 = guarded((nb.z2_numel(36),), dtype=torch.float16)
    assert _launch_pair_bias(L, {**kw, "T1": 6, "T2": 6}, 128, 4, frag, None, z2, 16.0) == PD_ERR_UNSUPPORTED      # T % 4
    assert _launch_pair_bias(L, kw, 128, 4, frag, None, z2, 0.0) == PD_ERR_ARG
    assert _launch_pair_bias(L, kw, 128, 4, frag, None, z2, -1.0) == PD_ERR_ARG
    assert _launch_pair_bias(L, kw, 128, 4, frag, None, z2, NAN) == PD_ERR_ARG
    x, Wf = dev(kw["x"]), dev(kw["Wf"])
    assert L.pd_pair_bias_split(P(x), P(Wf), None, None, None, 0.0, 1.0, P(frag), 36, 0, 1e-8, None, 16.0, S()) == PD_ERR_ARG      # no z2
    assert L.pd_pair_bias_split(P(x), P(Wf), None, None, None, 0.0, 1.0, P(frag), 36, 0, 1e-8, P(z2) + 8, 16.0, S()) == PD_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(fbuf).all() and torch.isnan(zbuf).all()
