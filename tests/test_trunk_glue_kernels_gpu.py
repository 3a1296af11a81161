"""Kernel-level parity of the trunk "glue" kernels (csrc/pair.hip) and of pd_atom_pair_ffn (csrc/pair_ffn.hip), straight on the C ABI.

Two kinds of comparison (tests/trunk_glue_ref.py):
* exact - pd_pair_gather_add, pd_unpool_add(_g), pd_gather_rows_add, pd_template_mask and the v == 0 entries of pd_atom_pair_init do
  one IEEE fp32 operation per element: the expectation is the same fp32 operation done by torch on the CPU, compared with torch.equal.
* bounded - pd_atom_pair_init (v == 1), pd_pair_init_z, pd_segment_pool(_g), pd_axpby against the float64 reference under the
  derived per-element bound gamma_k * S (tr.assert_within_bound prints the worst |error| / bound of every comparison; pytest -s).

Every output the kernel must write completely is NaN before the launch and finite after it.  Every buffer a kernel writes (outputs and
in-place operands) is a slice of a larger allocation with a NaN band in front of it and behind it; the bands are checked after the launch.

The input generators (``*_case`` / ``*_tables`` functions, CPU tensors only, cached: a case and its float64 reference are computed once
and never modified) are imported by tests/test_trunk_glue_ref_cpu.py, which asserts the conditions the cases rely on without a GPU.

Not covered: the 64-bit index instantiation of unpool_add_kernel is chosen when B * A * C / 4 approaches 2^31 quads - a 32 GiB
operand, out of reach of a test shape; the launcher is left as it is.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import trunk_glue_ref as tr

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN = float("nan")
BAND = 64                               # floats of NaN in front of and behind every written buffer (a multiple of 4: 16-byte alignment)


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


def guarded(shape, init=None):
    """(allocation, view): a device buffer of `shape` with BAND NaNs on either side; the view holds `init` (a CPU tensor) or NaN"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * BAND,), NAN, device="cuda")
    view = buf[BAND:BAND + n].view(*shape)
    if init is not None:
        view.copy_(init)
    return buf, view


def bands_intact(buf):
    torch.cuda.synchronize()
    return bool(torch.isnan(buf[:BAND]).all() and torch.isnan(buf[-BAND:]).all())


# ------------------------------------------------------------------ pd_atom_pair_init
ATOM_PAIR_A = [1, 70, 259]               # 259: two x-blocks, the second ragged
C_AP = [8, 16, 32]


@functools.lru_cache(maxsize=None)
def atom_pair_init_case(A, C):
    """uid groups of four atoms scattered over the atom order (ids not dense); atoms 0 and 1 coincide and share a uid (d = 0)"""
    g = gen(100 + 7 * A + C)
    pos = torch.randn(A, 3, generator=g) * 5
    uid = ((torch.arange(A) // 4) * 3 + 7)[torch.randperm(A, generator=g)].long()
    if A > 1:
        pos[1] = pos[0]
        uid[1] = uid[0]
    return dict(pos=pos, uid=uid, cl=torch.randn(A, C, generator=g), cm=torch.randn(A, C, generator=g),
                Wp=torch.randn(C, 3, generator=g) * 0.3, Wd=torch.randn(C, 1, generator=g), Wv=torch.randn(C, 1, generator=g))


@functools.lru_cache(maxsize=None)
def atom_pair_init_expected(A, C):
    c = atom_pair_init_case(A, C)
    return tr.atom_pair_init64(**c), tr.atom_pair_init_bound(**c), tr.atom_pair_init64(**c, dtype=torch.float32)


def _launch_atom_pair_init(L, c, A, C, ap):
    pos, uid, cl, cm = dev(c["pos"]), dev(c["uid"]), dev(c["cl"]), dev(c["cm"])
    Wp, Wd, Wv = dev(c["Wp"]), dev(c["Wd"]), dev(c["Wv"])
    rc = L.pd_atom_pair_init(P(pos), P(uid), P(cl), P(cm), P(Wp), P(Wd), P(Wv), P(ap), A, C, S())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("C", C_AP)
@pytest.mark.parametrize("A", ATOM_PAIR_A)
def test_atom_pair_init(L, A, C):
    c = atom_pair_init_case(A, C)
    ref, bound, ref32 = atom_pair_init_expected(A, C)
    buf, ap = guarded((A, A, C))
    ok(_launch_atom_pair_init(L, c, A, C, ap), "pd_atom_pair_init")
    assert bands_intact(buf)
    out = ap.cpu()
    tr.assert_within_bound("atom_pair_init", f"A={A} c_ap={C}", out, ref, bound)
    other = ~tr.atom_pair_same_uid(c["uid"])                     # v == 0: one fp32 add, cl[l] + cm[m]
    assert torch.equal(out[other], ref32[other])


def test_atom_pair_init_refuses_other_widths(L):
    c = atom_pair_init_case(70, 16)
    buf, ap = guarded((70, 70, 12))
    assert _launch_atom_pair_init(L, c, 70, 12, ap) == PD_ERR_UNSUPPORTED
    assert torch.isnan(buf).all()


# ------------------------------------------------------------------ pd_pair_gather_add
@functools.lru_cache(maxsize=None)
def pair_gather_add_case(A, T, C):
    """a2t: several atoms per token (repeats), the last five atoms padded (token 0)"""
    g = gen(200 + 7 * A + 3 * T + C)
    a2t = torch.sort(torch.randint(0, T, (A,), generator=g)).values
    a2t[-5:] = 0
    return dict(ap=torch.randn(A, A, C, generator=g), zt=torch.randn(T, T, C, generator=g), a2t=a2t.long())


@pytest.mark.parametrize("C", C_AP)
@pytest.mark.parametrize("T", [1, 24])
@pytest.mark.parametrize("A", [70, 259])
def test_pair_gather_add(L, A, T, C):
    c = pair_gather_add_case(A, T, C)
    want = tr.pair_gather_add64(**c, dtype=torch.float32)
    buf, ap = guarded((A, A, C), c["ap"])
    zt, a2t = dev(c["zt"]), dev(c["a2t"])
    ok(L.pd_pair_gather_add(P(ap), P(zt), P(a2t), A, T, C, S()), "pd_pair_gather_add")
    assert bands_intact(buf)
    assert torch.equal(ap.cpu(), want)
    assert torch.equal(zt.cpu(), c["zt"])


def test_pair_gather_add_refuses_other_widths(L):
    c = pair_gather_add_case(70, 24, 16)
    buf, ap = guarded((70, 70, 12))
    zt, a2t = dev(c["zt"]), dev(c["a2t"])
    assert L.pd_pair_gather_add(P(ap), P(zt), P(a2t), 70, 24, 12, S()) == PD_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


# ------------------------------------------------------------------ pd_pair_init_z
#: both sides of the 16-way key split (T >= 64); 65 and 97 leave empty trailing chunks, 97 also a short last one, 80 divides evenly;
#: CZ 32 / 128 / 160: blocks of 64 / 128 / 192 threads, 160 with idle lanes in the channel loop
PAIR_Z_CASES = [(T, CZ) for T in (24, 63, 64, 65, 80, 97) for CZ in (32, 128)] + [(65, 160)]
#: (asym_id, entity_id, sym_id, tokens); the first chain takes what is left of T.  Four copies of entity 10 with sym 0, 1, 2, 2, 5 give
#: every clamped sym difference -2 .. 2 between different chains (0 between the two sym-2 copies), entity 11 the other-entity class.
_CHAINS = [(3, 10, 0, None), (0, 10, 1, 3), (7, 10, 2, 3), (9, 10, 2, 3), (4, 10, 5, 3), (12, 11, 0, 4)]
_RES_HEAD = [5, 5, 6, 37, 38, 80, 4, 37]      # first chain: offsets 0, +-32, +-33, +-75 among these


def pair_ids(T, seed=0):
    g = gen(300 + T + seed)
    n0 = T - sum(n for *_, n in _CHAINS[1:])
    assert n0 >= len(_RES_HEAD)
    asym, ent, sym, res = [], [], [], []
    for a, e, s, n in _CHAINS:
        n = n0 if n is None else n
        asym += [a] * n
        ent += [e] * n
        sym += [s] * n
        res += (_RES_HEAD + torch.randint(0, 100, (n - len(_RES_HEAD),), generator=g).tolist()) if a == 3 else list(range(n))
    perm = torch.randperm(T, generator=g)                        # chains interleaved: every class lands in every key chunk
    return dict(asym_id=torch.tensor(asym, dtype=torch.int32)[perm], entity_id=torch.tensor(ent, dtype=torch.int32)[perm],
                sym_id=torch.tensor(sym, dtype=torch.int32)[perm], residue_index=torch.tensor(res, dtype=torch.int64)[perm])


@functools.lru_cache(maxsize=None)
def pair_init_z_case(T, CZ):
    g = gen(400 + 5 * T + CZ)
    ids = pair_ids(T)
    ids["rel_tok_feat"] = torch.randn(T, T, 42, generator=g) * (torch.rand(T, T, 42, generator=g) < 0.5)
    bonds = (torch.rand(T, T, generator=g) < 0.25) * (0.5 + torch.rand(T, T, generator=g))
    return dict(si=torch.randn(T, CZ, generator=g), sj=torch.randn(T, CZ, generator=g), W=torch.randn(CZ, 115, generator=g) * 0.5,
                wb=torch.randn(CZ, generator=g), ids=ids, bonds=bonds)


@functools.lru_cache(maxsize=None)
def pair_init_z_expected(T, CZ):
    c = pair_init_z_case(T, CZ)
    return tr.pair_init_z64(**c), tr.pair_init_z_bound(**c)


@pytest.mark.parametrize("T,CZ", PAIR_Z_CASES)
def test_pair_init_z(L, T, CZ):
    c = pair_init_z_case(T, CZ)
    ref, bound = pair_init_z_expected(T, CZ)
    ids = c["ids"]
    si, sj, WT, wb = dev(c["si"]), dev(c["sj"]), dev(c["W"].t()), dev(c["wb"])
    asym, sym, ent, res = dev(ids["asym_id"]), dev(ids["sym_id"]), dev(ids["entity_id"]), dev(ids["residue_index"])
    rtf, bonds = dev(ids["rel_tok_feat"]), dev(c["bonds"])
    buf, z = guarded((T, T, CZ))
    ok(L.pd_pair_init_z(P(si), P(sj), P(WT), P(wb), P(asym), P(sym), P(ent), P(res), P(rtf), P(bonds), P(z), T, CZ, S()), "pd_pair_init_z")
    assert bands_intact(buf)
    tr.assert_within_bound("pair_init_z", f"T={T} CZ={CZ}", z.cpu(), ref, bound)


# ------------------------------------------------------------------ token tables of the pool / unpool kernels
#: 0, 1, 7, 8, 9, 16, 17 atoms: the boundaries of the 8-wide unrolled load; three systems with different tables, padded to one shape
POOL_SIZES = ([0, 1, 7, 8, 9, 16, 17, 5, 0, 2], [0, 1, 7, 8, 9, 16, 17, 11], [0, 1, 7, 8, 9, 16, 17, 4, 4, 4, 1])
POOL_A, POOL_T, POOL_G = 80, 13, 3


@functools.lru_cache(maxsize=None)
def pool_tables():
    """per system (tok_start int32 [T + 1], a2t int64 [A], sizes [T]): the sizes above in a seeded order, the last real token not
    empty (it ends exactly at the last real atom), padded tokens (start == end) and padded atoms (token 0 for the unpool) behind"""
    out = []
    for gi, sizes in enumerate(POOL_SIZES):
        sizes = torch.tensor(sizes)[torch.randperm(len(sizes), generator=gen(500 + gi))]
        if sizes[-1] == 0:
            k = int(torch.nonzero(sizes)[0])
            sizes[-1], sizes[k] = sizes[k].clone(), 0
        n = torch.zeros(POOL_T, dtype=torch.long)
        n[:sizes.numel()] = sizes
        ts = torch.zeros(POOL_T + 1, dtype=torch.int32)
        ts[1:] = torch.cumsum(n, 0).to(torch.int32)
        a2t = torch.zeros(POOL_A, dtype=torch.int64)
        a2t[:int(ts[-1])] = torch.repeat_interleave(torch.arange(POOL_T), n)
        out.append((ts, a2t, n))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pool_case(C, B):
    """u [G * B, A, C] (NaN on the padded atoms of each system: never read), add [G, T, C]"""
    g = gen(600 + C + B)
    u = torch.randn(POOL_G * B, POOL_A, C, generator=g) * 3
    for gi, (ts, _, _) in enumerate(pool_tables()):
        u[gi * B:(gi + 1) * B, int(ts[-1]):] = NAN
    return dict(u=u, add=torch.randn(POOL_G, POOL_T, C, generator=g))


@functools.lru_cache(maxsize=None)
def pool_expected(C, B, with_add):
    """float64 reference and bound of every system, stacked as the grouped launch lays them out"""
    c = pool_case(C, B)
    refs, bounds = [], []
    for gi, (ts, _, _) in enumerate(pool_tables()):
        u, add = c["u"][gi * B:(gi + 1) * B], c["add"][gi] if with_add else None
        refs.append(tr.segment_pool64(u, ts, add))
        bounds.append(tr.segment_pool_bound(u, ts, add))
    return torch.cat(refs), torch.cat(bounds)


def _check_pool(name, case, out, ref, bound, add, sizes):
    tr.assert_within_bound(name, case, out, ref, bound)
    empty = sizes == 0                                           # a token without atoms: exactly add[t], or exactly 0
    want = torch.zeros_like(out[:, empty]) if add is None else add[empty][None].expand_as(out[:, empty])
    assert torch.equal(out[:, empty], want)


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [4, 256])
def test_segment_pool(L, C, B, with_add):
    c = pool_case(C, B)
    ref, bound = pool_expected(C, B, with_add)
    tabs = pool_tables()
    A, T, G = POOL_A, POOL_T, POOL_G
    u = dev(c["u"])
    add = dev(c["add"]) if with_add else None
    tok = dev(torch.stack([t[0] for t in tabs]))
    # one system per launch
    for gi, (ts, _, sizes) in enumerate(tabs):
        buf, out = guarded((B, T, C))
        u1, tok1, add1 = u[gi * B:(gi + 1) * B], tok[gi], add[gi] if with_add else None
        ok(L.pd_segment_pool(P(u1), P(tok1), P(add1), P(out), B, A, T, C, S()), "pd_segment_pool")
        assert bands_intact(buf)
        sl = slice(gi * B, (gi + 1) * B)
        _check_pool("segment_pool", f"C={C} B={B} add={with_add} system {gi}", out.cpu(), ref[sl], bound[sl],
                    c["add"][gi] if with_add else None, sizes)
    # the grouped launch: G systems, each with its own table and add rows
    buf, out = guarded((G * B, T, C))
    ok(L.pd_segment_pool_g(P(u), P(tok), P(add), P(out), G, B, A, T, C, S()), "pd_segment_pool_g")
    assert bands_intact(buf)
    res = out.cpu()
    for gi, (_, _, sizes) in enumerate(tabs):
        sl = slice(gi * B, (gi + 1) * B)
        _check_pool("segment_pool_g", f"C={C} B={B} add={with_add} system {gi}", res[sl], ref[sl], bound[sl],
                    c["add"][gi] if with_add else None, sizes)


def test_segment_pool_refuses_a_width_that_is_no_multiple_of_four(L):
    ts = dev(pool_tables()[0][0])
    u = torch.zeros(1, POOL_A, 6, device="cuda")
    buf, out = guarded((1, POOL_T, 6))
    assert L.pd_segment_pool(P(u), P(ts), None, P(out), 1, POOL_A, POOL_T, 6, S()) == PD_ERR_ARG
    assert L.pd_segment_pool_g(P(u), P(ts), None, P(out), 1, 1, POOL_A, POOL_T, 6, S()) == PD_ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


# ------------------------------------------------------------------ pd_unpool_add
@functools.lru_cache(maxsize=None)
def unpool_case(C, B):
    g = gen(700 + C + B)
    return dict(ba=torch.randn(POOL_G * B, POOL_A, C, generator=g), us=torch.randn(POOL_G * B, POOL_T, C, generator=g))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [4, 128])
def test_unpool_add(L, C, B):
    c = unpool_case(C, B)
    tabs = pool_tables()
    A, T, G = POOL_A, POOL_T, POOL_G
    want = torch.cat([tr.unpool_add64(c["ba"][gi * B:(gi + 1) * B], c["us"][gi * B:(gi + 1) * B], tabs[gi][1], dtype=torch.float32)
                      for gi in range(G)])
    us = dev(c["us"])
    a2t = dev(torch.stack([t[1] for t in tabs]))
    for gi in range(G):
        sl = slice(gi * B, (gi + 1) * B)
        buf, ba = guarded((B, A, C), c["ba"][sl])
        us1, a2t1 = us[sl], a2t[gi]
        ok(L.pd_unpool_add(P(ba), P(us1), P(a2t1), B, A, T, C, S()), "pd_unpool_add")
        assert bands_intact(buf)
        assert torch.equal(ba.cpu(), want[sl]), gi
    buf, ba = guarded((G * B, A, C), c["ba"])
    ok(L.pd_unpool_add_g(P(ba), P(us), P(a2t), G, B, A, T, C, S()), "pd_unpool_add_g")
    assert bands_intact(buf)
    assert torch.equal(ba.cpu(), want)
    assert torch.equal(us.cpu(), c["us"])


# ------------------------------------------------------------------ pd_gather_rows_add
@functools.lru_cache(maxsize=None)
def gather_rows_case(R, C):
    """fewer source rows than R: indices repeat and come in no order"""
    g = gen(800 + 3 * R + C)
    N = max(1, R // 3)
    return dict(y=torch.randn(R, C, generator=g), x=torch.randn(N, C, generator=g), idx=torch.randint(0, N, (R,), generator=g).long())


@pytest.mark.parametrize("C", [4, 128])
@pytest.mark.parametrize("R", [1, 70, 259])
def test_gather_rows_add(L, R, C):
    c = gather_rows_case(R, C)
    x, idx = dev(c["x"]), dev(c["idx"])
    buf, y = guarded((R, C), c["y"])
    ok(L.pd_gather_rows_add(P(y), P(x), P(idx), R, C, S()), "pd_gather_rows_add")
    assert bands_intact(buf)
    assert torch.equal(y.cpu(), tr.gather_rows_add64(**c, dtype=torch.float32))
    # the confidence head's use: y zeroed first, the result is a pure gather
    buf, y = guarded((R, C), torch.zeros(R, C))
    ok(L.pd_gather_rows_add(P(y), P(x), P(idx), R, C, S()), "pd_gather_rows_add")
    assert bands_intact(buf)
    assert torch.equal(y.cpu(), c["x"][c["idx"]])
    assert torch.equal(x.cpu(), c["x"])


# ------------------------------------------------------------------ pd_axpby
AXPBY_N = [1, 2, 3, 4, 5, 1023, 1024, 1025, 4099]
AXPBY_SCALES = [(1.0, 1.0), (-0.5, 0.25)]


@functools.lru_cache(maxsize=None)
def axpby_case(n):
    g = gen(900 + n)
    return dict(a=torch.randn(n, generator=g), b=torch.randn(n, generator=g), sb_ptr=torch.tensor([0.7]))


def axpby_variants():
    """(with b, with sb_ptr, sa, sb)"""
    return [(wb, wp, sa, sb) for wb in (True, False) for wp in (True, False) for sa, sb in AXPBY_SCALES]


def axpby_args(c, wb, wp, sa, sb):
    return dict(a=c["a"], sa=sa, b=c["b"] if wb else None, sb_ptr=c["sb_ptr"] if wp else None, sb=sb)


@pytest.mark.parametrize("n", AXPBY_N)
def test_axpby(L, n):
    c = axpby_case(n)
    a, b, sp = dev(c["a"]), dev(c["b"]), dev(c["sb_ptr"])
    for wb, wp, sa, sb in axpby_variants():
        kw = axpby_args(c, wb, wp, sa, sb)
        bp, spp = (P(b) if wb else None), (P(sp) if wp else None)
        buf, out = guarded((n,))
        ok(L.pd_axpby(P(out), P(a), sa, bp, spp, sb, n, S()), "pd_axpby")
        assert bands_intact(buf)                                 # nothing behind element n - 1 (the tail of an n % 4 != 0) is touched
        res = out.cpu()
        tr.assert_within_bound("axpby", f"n={n} b={wb} sb_ptr={wp} sa={sa} sb={sb}", res, tr.axpby64(**kw), tr.axpby_bound(**kw))
        # the engine's two in-place forms: out == a (z += tpo * t_mask) and out == b (a = a0 + a)
        buf, io = guarded((n,), c["a"])
        ok(L.pd_axpby(P(io), P(io), sa, bp, spp, sb, n, S()), "pd_axpby out == a")
        assert bands_intact(buf)
        assert torch.equal(io.cpu(), res), ("out == a", wb, wp, sa, sb)
        if wb:
            buf, io = guarded((n,), c["b"])
            ok(L.pd_axpby(P(io), P(a), sa, P(io), spp, sb, n, S()), "pd_axpby out == b")
            assert bands_intact(buf)
            assert torch.equal(io.cpu(), res), ("out == b", wp, sa, sb)
    assert torch.equal(a.cpu(), c["a"]) and torch.equal(b.cpu(), c["b"])


# ------------------------------------------------------------------ pd_template_mask
@functools.lru_cache(maxsize=None)
def template_mask_case(T, D):
    """z_mask and the mask column hold values other than 0 / 1 (a dropped factor shows), every other column is noise"""
    g = gen(1000 + 3 * T + D)
    z_mask = torch.rand(T, T, generator=g) * (torch.rand(T, T, generator=g) < 0.8)
    asym = torch.tensor([3, 0, 7])[torch.randint(0, 3, (T,), generator=g)].int()
    return dict(z_mask=z_mask, templ_feat=torch.rand(T, T, D, generator=g) + 0.5, asym=asym)


@pytest.mark.parametrize("D", [40, 7])
@pytest.mark.parametrize("T", [1, 24, 65])
def test_template_mask(L, T, D):
    c = template_mask_case(T, D)
    zm, tf, asym = dev(c["z_mask"]), dev(c["templ_feat"]), dev(c["asym"])
    buf, out = guarded((T, T))
    ok(L.pd_template_mask(P(zm), P(tf), P(asym), P(out), T, D, S()), "pd_template_mask")
    assert bands_intact(buf)
    assert torch.equal(out.cpu(), tr.template_mask64(**c, dtype=torch.float32))


# ------------------------------------------------------------------ pd_atom_pair_ffn
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 257])
def test_atom_pair_ffn_row_counts(L, rows):
    """ap += W2 (silu(W1 ap) * (W3 ap)) around the kernel's 32-row groups; the comparison and the tolerance of
    tests/test_round2_gpu.py::test_atom_pair_ffn_fused_kernel"""
    g = gen(3)
    ap = torch.randn(rows, 16, generator=g)
    W1, W3 = torch.randn(128, 16, generator=g) / 4, torch.randn(128, 16, generator=g) / 4
    W2 = torch.randn(16, 128, generator=g) / 11
    ref = ap + (F.silu(ap @ W1.T) * (ap @ W3.T)) @ W2.T
    w1, w3, w2 = dev(W1), dev(W3), dev(W2)
    buf, apd = guarded((rows, 16), ap)
    ok(L.pd_atom_pair_ffn(P(apd), P(w1), P(w3), P(w2), rows, 16, 128, S()), "pd_atom_pair_ffn")
    assert bands_intact(buf)                                     # the rows behind the last one of a ragged group stay untouched
    torch.testing.assert_close(apd.cpu(), ref, atol=2e-5, rtol=1e-4)
