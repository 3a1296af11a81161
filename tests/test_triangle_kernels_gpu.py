"""Kernel-level parity of the triangle kernels (csrc/tri_mul.hip: pd_tri_mul; csrc/tri_tail.hip: pd_tri_tail, modes 0 and 1;
csrc/tri_attn.hip: pd_tri_attention), straight on the C ABI, against the float64 references and the derived per-element bounds of tests/triangle_ref.py
(assert_within_bound prints the worst |error| / bound of every comparison; pytest -s), and the refusals of the three triangle entry
points pd_tri_mul, pd_tri_tail and pd_tri_attention.

Every buffer a kernel writes is a slice of a larger allocation with a NaN band in front of it and behind it; outputs are NaN before
the launch, operand entries a kernel must not read are NaN, and every slot a kernel must leave alone has to come back NaN.  Cases and
references are the cached CPU tensors of tests/triangle_ref.py; tests/test_triangle_ref_cpu.py asserts the conditions they rely on.

Not covered here: the `static bool raised` LDS attribute of pd_tri_attention on a second device; beyond T = 132 the float64 comparison
of pd_tri_attention takes 24 of the batch rows (triangle_ref.attn_batches), the others are checked to be written and finite.
"""
import ctypes as C
import itertools
import math

import pytest
import torch

import triangle_ref as tr

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN = float("nan")
BAND = 64                               # elements of NaN in front of and behind every written buffer (a multiple of 16 bytes)


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


def scalar(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


# ------------------------------------------------------------------ pd_tri_mul
def tri_mul_args(q, k, o, T, Treal, nch, stride, transpose, qa, ka):
    from physdock_amd import _lib
    a = _lib.TriMulArgs()
    a.q, a.k, a.o = P(q), P(k), P(o)
    a.T, a.Treal, a.nch, a.ch_stride, a.transpose = T, Treal, nch, stride, transpose
    a.q_amax, a.k_amax = P(qa), P(ka)
    return a


def planes(x, T, stride):
    """x [nch, T, T] as planes `stride` floats apart in a NaN-filled device array"""
    nch = x.shape[0]
    wide = torch.full((nch, stride), NAN)
    wide[:, :T * T] = x.reshape(nch, -1)
    return dev(wide)


@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("T,Treal", tr.TRI_MUL_SHAPES)
def test_tri_mul(L, T, Treal, transpose):
    worst = 0.0
    for nch, pad, loose in itertools.product(tr.TRI_MUL_NCH, (0, 8), (False, True)):
        q, k, _, _ = tr.tri_mul_case(T, nch)
        ref, bound, qa, ka = tr.tri_mul_expected(T, Treal, nch, transpose, loose)
        stride = T * T + pad
        qd = planes(tr.tri_mul_poisoned(q, Treal, transpose), T, stride)
        kd = planes(tr.tri_mul_poisoned(k, Treal, transpose), T, stride)
        buf, o = guarded((nch, stride))
        qs, ks = scalar(qa), scalar(ka)
        a = tri_mul_args(qd, kd, o, T, Treal, nch, stride, transpose, qs, ks)
        ok(L.pd_tri_mul(C.byref(a), S()), "pd_tri_mul")
        assert bands_intact(buf)
        case = f"T={T} Treal={Treal} nch={nch} transpose={transpose} stride=T*T+{pad} bounds {'x1000' if loose else 'tight'}"
        worst = max(worst, tr.assert_within_bound("pd_tri_mul", case, o[:, :T * T].reshape(nch, T, T), ref, bound))
        assert bool(torch.isnan(o[:, T * T:]).all()), case            # the gap between the planes is left alone
    print(f"WORST | pd_tri_mul | T={T} Treal={Treal} transpose={transpose} | worst err/bound of the 16 (nch, stride, bounds) launches {worst:.3f}")


# ------------------------------------------------------------------ pd_tri_tail
def tri_tail_args(mode, z, o, M, w_in, w_out, Wg2, bg, Wz2, bz, zn, on, Cdim=128, Co=None):
    from physdock_amd import _lib
    a = _lib.TriTailArgs()
    a.z, a.o, a.M, a.C, a.Co = P(z), P(o), M, Cdim, (Co if Co is not None else (tr.CO if mode == 0 else tr.C_))
    a.w_in, a.w_out, a.eps = P(w_in), (P(w_out) if w_out is not None else None), tr.TAIL_EPS
    a.Wg, a.wg_inv, a.bg = Wg2[0].data_ptr(), Wg2[1].data_ptr(), (P(bg) if bg is not None else None)
    a.Wz, a.wz_inv, a.bz = Wz2[0].data_ptr(), Wz2[1].data_ptr(), (P(bz) if bz is not None else None)
    a.zn_amax, a.on_amax, a.mode = P(zn), P(on), mode
    return a


def tail_weights(mode):
    from physdock_amd.packing import split2_f16
    w_in, w_out, Wg, bg, Wz, bz = tr.tri_tail_weights(mode)
    return dev(w_in), dev(w_out), split2_f16(dev(Wg)), dev(bg), split2_f16(dev(Wz)), dev(bz)


def run_tri_tail(L, mode, M, biases, o_offset=0):
    """one launch, in place, on a guarded z of M + 70 rows of which the kernel is told M; o at `o_offset` floats past a 16-byte boundary"""
    z, o, _, zn_amax, on_amax = tr.tri_tail_case(mode, M)
    ref, bound, _ = tr.tri_tail_expected(mode, M, biases)
    w_in, w_out, Wg2, bg, Wz2, bz = tail_weights(mode)
    extra = 70
    buf, zv = guarded((M + extra, tr.C_))
    zv[:M].copy_(z)
    oall = torch.full((o.numel() + 4 + o_offset,), NAN, device="cuda")
    od = oall[o_offset:o_offset + o.numel()].view(*o.shape)
    od.copy_(o)
    assert od.data_ptr() % 16 == 4 * o_offset
    a = tri_tail_args(mode, zv, od, M, w_in, w_out, Wg2, bg if biases else None, Wz2, bz if biases else None, scalar(zn_amax), scalar(on_amax))
    ok(L.pd_tri_tail(C.byref(a), S()), "pd_tri_tail")
    assert bands_intact(buf)
    case = f"mode {mode} M={M} biases={'given' if biases else 'NULL'} o offset {4 * o_offset} bytes"
    tr.assert_within_bound("pd_tri_tail", case, zv[:M], ref, bound)
    assert bool(torch.isnan(zv[M:]).all()), case                      # rows >= M are left alone


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M", tr.TAIL_SMALL_M)
def test_tri_tail_small(L, mode, M):
    for biases in (True, False):
        run_tri_tail(L, mode, M, biases)
    if mode == 0:                                                     # o only 4-byte aligned: mode 1 alone requires 16 bytes of o
        run_tri_tail(L, mode, M, True, o_offset=1)


@pytest.mark.parametrize("mode", [0, 1])
def test_tri_tail_past_the_grid(L, mode):
    """the grid-stride arm: one block fetches a second, full tile and one a second, partial tile"""
    run_tri_tail(L, mode, tr.TAIL_GRID_M[mode], True)


# ------------------------------------------------------------------ pd_tri_attention
def attn_cases():
    import test_triangle_ref_cpu as cpu
    return cpu.attn_gpu_cases()


@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("case", attn_cases(), ids=str)
def test_tri_attention(L, case, transpose):
    from physdock_amd import _lib, ops
    from physdock_amd.packing import split2_f16
    import norm_bias_ref as nb
    T, Treal, variant, amax_f, nk0 = case
    c = tr.attn_case(*case)
    bs, ref, bound, uni = tr.attn_expected(*case)
    assert c["ps"] == ops.attn_bias_prescale(c["qkv_amax"][0], c["qkv_amax"][1])          # the host's arithmetic and the reference's agree
    z2 = dev(nb.z2_scatter(c["hi"], c["lo"], torch.zeros((), dtype=torch.float16)))       # slots of rows >= T: zero (the header's contract)
    frag, _ = nb.bias_frag_scatter(c["bias"])                                             # NaN in the slots of keys >= Treal and in the pad slots
    frag = dev(frag)
    W2 = split2_f16(dev(c["Wf"]), rows_per_scale=32)
    amax = torch.tensor(c["qkv_amax"], dtype=torch.float32, device="cuda")
    buf, o = guarded((T, T, tr.C_))
    a = _lib.TriAttnArgs()
    a.z2, a.W2, a.w_inv = z2.data_ptr(), W2[0].data_ptr(), W2[1].data_ptr()
    a.bias, a.bias_prescale, a.bias_nk, a.o = P(frag), c["ps"], (0 if nk0 else T), P(o)
    a.T, a.Treal, a.C, a.nheads, a.transpose = T, Treal, tr.C_, tr.ATT_H, transpose
    a.zn_amax, a.qkv_amax, a.scale = tr.ZN_AMAX, P(amax), 1.0 / math.sqrt(32.0)
    ok(L.pd_tri_attention(C.byref(a), S()), "pd_tri_attention")
    assert bands_intact(buf)
    out = (o.transpose(0, 1) if transpose else o).cpu()                                   # [batch, query, C]
    assert bool(torch.isfinite(out).all()), case                                          # every (b, r) with b, r < T is written
    keep = ~c["full"]
    keep[Treal:] = False
    name = f"{case} transpose={transpose}"
    tr.assert_within_bound("pd_tri_attention", name, out[bs][:, keep], ref[:, keep], bound[:, keep])
    full = c["full"].clone()
    full[Treal:] = False
    if full.any():            # fully masked query rows: the fp32 statement, uniform over the real keys (tests/test_tri_attn_gpu.py's threshold)
        got, want = out[bs][:, full].double(), uni[:, None, :].expand(-1, int(full.sum()), -1)
        worst = float((got - want).abs().max() / want.abs().mean())
        print(f"FULL | pd_tri_attention | {name} | fully masked rows vs the uniform mean of v: max |diff| / mean|o| = {worst:.2e}")
        assert worst < 1e-4


# ------------------------------------------------------------------ refusals
def test_tri_attn_args_size(L):
    from physdock_amd import _lib
    assert L.pd_tri_attn_args_size() == C.sizeof(_lib.TriAttnArgs)


def test_tri_mul_refusals(L):
    T, Treal, nch = 36, 33, 3
    q, k, qa, ka = tr.tri_mul_case(T, nch)
    big = torch.zeros(nch * T * T + 16)
    qd, kd = dev(big), dev(big)
    buf, o = guarded((nch * T * T + 16,))
    qs, ks = scalar(qa), scalar(ka)

    def args(**kw):
        a = tri_mul_args(qd, kd, o, T, Treal, nch, T * T, 0, qs, ks)
        for name, v in kw.items():
            setattr(a, name, v)
        return a
    cases = [(f"{n} NULL", {n: None}, PD_ERR_ARG) for n in ("q", "k", "o", "q_amax", "k_amax")]
    cases += [("T = 0", {"T": 0}, PD_ERR_UNSUPPORTED), ("T < 0", {"T": -4}, PD_ERR_UNSUPPORTED), ("Treal = 0", {"Treal": 0}, PD_ERR_UNSUPPORTED),
              ("Treal > T", {"Treal": T + 1}, PD_ERR_UNSUPPORTED), ("T % 4", {"T": 34, "Treal": 33}, PD_ERR_UNSUPPORTED),
              ("nch = 0", {"nch": 0}, PD_ERR_UNSUPPORTED), ("nch < 0", {"nch": -1}, PD_ERR_UNSUPPORTED),
              ("ch_stride % 4", {"ch_stride": T * T + 2}, PD_ERR_UNSUPPORTED)]
    for name, t in (("q", qd), ("k", kd), ("o", o)):
        for off in (1, 2):
            cases.append((f"{name} + {4 * off} bytes", {name: P(t) + 4 * off}, PD_ERR_UNSUPPORTED))
    assert L.pd_tri_mul(None, S()) == PD_ERR_ARG
    for what, kw, want in cases:
        assert L.pd_tri_mul(C.byref(args(**kw)), S()) == want, what
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    ok(L.pd_tri_mul(C.byref(args()), S()), "pd_tri_mul")             # the unmodified arguments are accepted
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", [0, 1])
def test_tri_tail_refusals(L, mode):
    M = 100
    z, o, _, zn_amax, on_amax = tr.tri_tail_case(mode, M)
    w_in, w_out, Wg2, bg, Wz2, bz = tail_weights(mode)
    buf, zv = guarded((M + 1, tr.C_))
    od = torch.zeros(o.numel() + 16, device="cuda")
    zn, on = scalar(zn_amax), scalar(on_amax)
    w_in_pad = torch.ones(tr.C_ + 16, device="cuda")

    def args(**kw):
        a = tri_tail_args(mode, zv, od, M, w_in, w_out, Wg2, bg, Wz2, bz, zn, on)
        for name, v in kw.items():
            setattr(a, name, v)
        return a
    required = ["z", "o", "w_in", "Wg", "wg_inv", "Wz", "wz_inv", "zn_amax", "on_amax"] + (["w_out"] if mode == 0 else [])
    cases = [(f"{n} NULL", {n: None}, PD_ERR_ARG) for n in required]
    cases += [("mode 2", {"mode": 2}, PD_ERR_ARG), ("mode -1", {"mode": -1}, PD_ERR_ARG),
              ("C = 64", {"C": 64}, PD_ERR_UNSUPPORTED), ("Co of the other mode", {"Co": tr.C_ if mode == 0 else tr.CO}, PD_ERR_UNSUPPORTED),
              ("Co = 64", {"Co": 64}, PD_ERR_UNSUPPORTED), ("M = 0", {"M": 0}, PD_ERR_UNSUPPORTED), ("M < 0", {"M": -5}, PD_ERR_UNSUPPORTED)]
    aligned = [("z", P(zv)), ("w_in", P(w_in_pad)), ("Wg", Wg2[0].data_ptr()), ("Wz", Wz2[0].data_ptr())] + ([("o", P(od))] if mode == 1 else [])
    for name, base in aligned:
        for off in (4, 8):
            cases.append((f"{name} + {off} bytes", {name: base + off}, PD_ERR_UNSUPPORTED))
    for what, kw, want in cases:
        assert L.pd_tri_tail(C.byref(args(**kw)), S()) == want, what
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


def test_tri_attention_refusals(L):
    from physdock_amd import _lib, ops
    from physdock_amd.packing import split2_f16
    T, Treal = 36, 33
    z2 = torch.zeros(ops.tri_z2_numel(T) + 16, dtype=torch.float16, device="cuda")
    W2 = split2_f16(torch.randn(384, 128, generator=tr.gen(5)).cuda() / math.sqrt(128.0), rows_per_scale=32)
    w_inv_pad = torch.ones(384 + 16, device="cuda")
    bias = torch.zeros(ops.bias_frag_numel(4, T, T), device="cuda")
    amax = torch.tensor([20.0, 20.0, 15.0], device="cuda")
    buf, o = guarded((T * T * 128 + 16,))
    ps = ops.attn_bias_prescale(20.0, 20.0)

    def args(**kw):
        a = _lib.TriAttnArgs()
        a.z2, a.W2, a.w_inv = z2.data_ptr(), W2[0].data_ptr(), W2[1].data_ptr()
        a.bias, a.bias_prescale, a.bias_nk, a.o = P(bias), ps, T, P(o)
        a.T, a.Treal, a.C, a.nheads, a.transpose = T, Treal, 128, 4, 0
        a.zn_amax, a.qkv_amax, a.scale = math.sqrt(128.0) * 1.0001, P(amax), 1.0 / math.sqrt(32.0)
        for name, v in kw.items():
            setattr(a, name, v)
        return a
    cases = [(f"{n} NULL", {n: None}, PD_ERR_ARG) for n in ("z2", "W2", "w_inv", "bias", "o", "qkv_amax")]
    cases += [("T = 0", {"T": 0}, PD_ERR_ARG), ("T < 0", {"T": -4}, PD_ERR_ARG), ("Treal = 0", {"Treal": 0}, PD_ERR_ARG),
              ("Treal < 0", {"Treal": -1}, PD_ERR_ARG), ("Treal > T", {"Treal": T + 1}, PD_ERR_ARG),
              ("T % 4", {"T": 34, "Treal": 33}, PD_ERR_UNSUPPORTED), ("T > 256", {"T": 260}, PD_ERR_UNSUPPORTED),
              ("C = 64", {"C": 64}, PD_ERR_UNSUPPORTED), ("nheads = 8", {"nheads": 8}, PD_ERR_UNSUPPORTED),
              ("bias_prescale = 0", {"bias_prescale": 0.0}, PD_ERR_UNSUPPORTED), ("bias_prescale < 0", {"bias_prescale": -1.0}, PD_ERR_UNSUPPORTED),
              ("bias_prescale NaN", {"bias_prescale": NAN}, PD_ERR_UNSUPPORTED), ("bias_prescale > 2^90", {"bias_prescale": 2.0 ** 91}, PD_ERR_UNSUPPORTED),
              ("zn_amax = 0", {"zn_amax": 0.0}, PD_ERR_UNSUPPORTED), ("zn_amax < 0", {"zn_amax": -1.0}, PD_ERR_UNSUPPORTED),
              ("zn_amax NaN", {"zn_amax": NAN}, PD_ERR_UNSUPPORTED)]
    for name, base in (("z2", z2.data_ptr()), ("W2", W2[0].data_ptr()), ("o", P(o)), ("w_inv", P(w_inv_pad))):
        for off in (4, 8):
            cases.append((f"{name} + {off} bytes", {name: base + off}, PD_ERR_UNSUPPORTED))
    assert L.pd_tri_attention(None, S()) == PD_ERR_ARG
    for what, kw, want in cases:
        assert L.pd_tri_attention(C.byref(args(**kw)), S()) == want, what
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
