"""The nine launchers of csrc/confidence_loss.hip and csrc/metrics.hip, called on the C ABI against the float64 definition
tests/conf_ref.py at the cases of tests/conf_cases.py (the table and the branch each case reaches are in that file's docstring;
tests/test_conf_ref_cpu.py checks the references, the cases' margins and their sensitivity without a GPU).

Exact: lDDT bits with the NaN positions, every target bin (read off the zero-logit gradient), the frame valid flag and origin,
the pTM / ipTM rows, clash counts, has_clash, +0.0 in masked gradient rows and under a zero scale, the loss of one bin.
Values, the project's own bars: a cross entropy within 2e-5 |f64| and its gradient, per element, within 2e-5 max|g64|
(tests/test_confidence_loss_gpu.py); pLDDT, PAE, pTM, ipTM, per_alignment, ranking and the nine rotation floats of a frame within
4 e32 + 8 ulp32(max|f64|), e32 = what a plain fp32 numpy evaluation of the same formula costs on the same input
(tests/test_metrics_cpu.bound, tests/test_sampler_kernels_gpu.py).  Every case prints its error, e32 and bar.
Every output and workspace sits in front of a sentinel guard that must come back untouched; a workspace holds exactly
pd_conf_loss_workspace_numel / pd_metrics_workspace_numel floats, is filled with NaN before the call, and a second call with other
garbage in it must give the same bits."""
import functools

import numpy as np
import pytest
import torch

import conf_cases as cc
import conf_ref as cr

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
GUARD = 256
SENT = {torch.float32: 1234.5, torch.int32: -77, torch.int64: -77}
TOL = cc.TOL
NAN, GARBAGE = float("nan"), -3.0e38


def _ops():
    from physdock_amd import _lib as ops
    return ops, ops.init()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(n, fill=None, dtype=torch.float32):
    """n elements of `fill` (the sentinel by default) in front of GUARD sentinels"""
    buf = torch.full((n + GUARD,), SENT[dtype], dtype=dtype, device="cuda")
    if fill is not None:
        buf[:n] = fill
    return buf


def guard_ok(buf, n):
    return bool((buf[n:] == SENT[buf.dtype]).all())


def shifted(t):
    """the same floats through a view that starts one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
    v = buf[1:]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == 4
    return v


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return all(torch.equal(bits(a[k]) if a[k].dtype == torch.float32 else a[k], bits(b[k]) if b[k].dtype == torch.float32 else b[k]) for k in a)


def check(what, got, v32, v64):
    """|got - f64| <= 4 e32 + 8 ulp32(max|f64|), everything finite"""
    got = np.asarray(got, np.float64)
    assert got.shape == np.shape(v64) and np.isfinite(got).all(), what
    e32, bar = cr.bar(v32, v64)
    err = float(np.abs(got - v64).max())
    print(f"{what}: max |hip - f64| {err:.3e}  e32 {e32:.3e}  bar {bar:.3e}")
    assert err <= bar, what


# ------------------------------------------------------------------ pd_lddt_atoms, pd_conf_frames
@pytest.mark.parametrize("name", cc.LDDT)
def test_lddt_atoms(name):
    ops, L = _ops()
    p, c, ref = ops.ptr, cc.lddt(name), cc.lddt_ref(name)
    t = [dev(a) for a in (c.x_pred, c.x_gt, c.centre, c.is_dna, c.is_rna, c.is_polymer)]
    out = guarded(c.B * c.A)
    assert L.pd_lddt_atoms(*(p(a) for a in t), p(out), c.B, c.A, c.T, ops.stream()) == 0
    torch.cuda.synchronize()
    assert guard_ok(out, c.B * c.A)
    got = out[:c.B * c.A].cpu().numpy().reshape(c.B, c.A)
    nan = np.isnan(ref)
    print(f"lddt {name}: {nan.sum()} NaN, {(got.view(np.uint32)[~nan] != ref.view(np.uint32)[~nan]).sum()} of {(~nan).sum()} values differ in bits")
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan])


@pytest.mark.parametrize("T", cc.FRAMES)
def test_conf_frames(T):
    ops, L = _ops()
    p, c = ops.ptr, cc.frames(T)
    f64, f32 = cc.frames_ref(T)
    t = [dev(c.x)] + [dev(i) for i in c.ids]
    out = guarded(T * 13)
    assert L.pd_conf_frames(*(p(a) for a in t), p(out), c.A, T, ops.stream()) == 0
    torch.cuda.synchronize()
    assert guard_ok(out, T * 13)
    got = out[:T * 13].cpu().numpy().reshape(T, 13)
    assert np.isfinite(got).all() and np.array_equal(got[:, 12], f64[:, 12]), "valid flag"
    assert np.array_equal(got[:, 9:12], c.x[c.ids[1]]), "origin"
    check(f"frames T {T} e1 | e2 | e3", got[:, :9], f32[:, :9], f64[:, :9])


# ------------------------------------------------------------------ the cross entropies
def ce_call(c, mode, logits, scale=1.0, want_grad=True, ws_fill=NAN):
    """(loss as a 0-d fp32 tensor, gradient [R, nb] or None), both on the CPU; mode None: pLDDT"""
    ops, L = _ops()
    p = ops.ptr
    R = c.A if mode is None else c.T * c.T
    nws = L.pd_conf_loss_workspace_numel(1, c.A, 1 if mode is None else c.T)
    assert nws == 4 + (max(R, c.A) + 63) // 64
    ws, out = guarded(nws, ws_fill), guarded(1)
    g = guarded(R * c.nb) if want_grad else None
    sc = None if scale is None else torch.tensor([scale], dtype=torch.float32, device="cuda")
    lg = dev(logits)
    if mode is None:
        t = [dev(c.lddt), dev(c.x_exists)]
        rc = L.pd_conf_loss_plddt(p(lg), p(t[0]), p(t[1]), c.nb, p(sc), p(ws), p(out), p(g), c.A, ops.stream())
    else:
        t = [dev(a) for a in (c.x_pred0, c.x_gt, c.x_exists, c.centre)] + [dev(c.frames_pred), dev(c.frames_gt)] * (mode == "pae")
        fr = (p(t[4]), p(t[5])) if mode == "pae" else (None, None)
        rc = L.pd_conf_loss_pairs(cc.MODES[mode], p(lg), *(p(a) for a in t[:4]), *fr, c.min_bin, c.max_bin - c.min_bin, c.nb, p(sc),
                                  p(ws), p(out), p(g), c.A, c.T, ops.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guard_ok(ws, nws) and guard_ok(out, 1) and (g is None or guard_ok(g, R * c.nb)), f"{c.name}: a guard was written"
    return out[0].cpu(), (g[:R * c.nb].cpu().reshape(R, c.nb) if want_grad else None)


def ce_checks(what, c, mode, logits, bins, mask, ref):
    (l64, _, g64), (l32, _, g32) = ref
    nb, R = c.nb, mask.shape[0]
    # two calls, NaN and other garbage in the workspace: the same bits
    loss, g = ce_call(c, mode, logits)
    loss2, g2 = ce_call(c, mode, logits, ws_fill=GARBAGE)
    assert torch.equal(bits(loss), bits(loss2)) and torch.equal(bits(g), bits(g2)), what
    err, gmax = abs(float(loss) - l64), np.abs(g64).max()
    gerr = np.abs(g.double().numpy() - g64).max()
    print(f"{what}: loss hip {float(loss)!r} f64 {l64!r} |err| {err:.3e} (fp32 numpy {abs(l32 - l64):.3e}) bar {TOL * abs(l64):.3e}; "
          f"gradient max err {gerr:.3e} (fp32 numpy {np.abs(g32 - g64).max():.3e}) bar {TOL * gmax:.3e}")
    assert torch.isfinite(g).all()
    if nb == 1:
        assert float(loss) == 0.0 and not bits(g).any(), what           # one bin: log softmax is exactly 0
    else:
        assert err <= TOL * abs(l64) and gerr <= TOL * gmax, what
    masked = torch.from_numpy(mask == 0)
    assert not bits(g[masked]).any(), f"{what}: masked rows must be +0.0"
    # the value-only call (no gradient, no scale): the same loss bits
    only, none = ce_call(c, mode, logits, scale=None, want_grad=False)
    assert none is None and torch.equal(bits(only), bits(loss)), what
    # a zero scale: an all-zero gradient, the loss unchanged
    l0, g0 = ce_call(c, mode, logits, scale=0.0)
    assert torch.equal(bits(l0), bits(loss)) and not bits(g0).any(), what
    # another scale scales the gradient
    _, gs = ce_call(c, mode, logits, scale=-2.5)
    assert np.abs(gs.double().numpy() + 2.5 * g64).max() <= 2.5 * TOL * gmax or nb == 1, what
    # the target bins, read off the gradient at zero logits: coef (1 / nb - onehot) is negative at the target only
    _, gz = ce_call(c, mode, np.zeros_like(logits))
    live = (gz != 0).any(-1)
    if nb == 1:
        assert not bits(gz).any()
    else:
        assert torch.equal(live, ~masked) and ((gz < 0).sum(-1)[live] == 1).all(), what
        assert torch.equal(gz.argmin(-1)[live], torch.from_numpy(bins)[live]), f"{what}: target bins"
        assert not bits(gz[masked]).any()


@pytest.mark.parametrize("A,nb", cc.PLDDT_LOSS)
def test_conf_loss_plddt(A, nb):
    c = cc.plddt_loss(A, nb)
    ce_checks(f"plddt loss {c.name}", c, None, c.logits, c.bins, c.x_exists, cc.plddt_loss_ref(A, nb))


@pytest.mark.parametrize("mode", cc.MODES)
@pytest.mark.parametrize("name", cc.PAIRS)
def test_conf_loss_pairs(name, mode):
    c = cc.pairs(name)
    ce_checks(f"{mode} loss {name}", c, mode, c.logits[mode], c.bins[mode].reshape(-1), c.mask.reshape(-1), cc.pairs_ref(name, mode))


# ------------------------------------------------------------------ pd_metrics_plddt
def plddt_call(lg, P, A, nb):
    ops, L = _ops()
    atom, mean = guarded(P * A), guarded(P)
    assert L.pd_metrics_plddt(ops.ptr(lg), ops.ptr(atom), ops.ptr(mean), P, A, nb, ops.stream()) == 0
    torch.cuda.synchronize()
    assert guard_ok(atom, P * A) and guard_ok(mean, P)
    return atom[:P * A].cpu().reshape(P, A), mean[:P].cpu()


@pytest.mark.parametrize("P,A,nb", cc.PLDDT)
def test_metrics_plddt(P, A, nb):
    c = cc.plddt(P, A, nb)
    (a64, m64), (a32, m32) = cc.plddt_ref(P, A, nb)
    lg = dev(c.logits)
    assert lg.data_ptr() % 16 == 0
    atom, mean = plddt_call(lg, P, A, nb)
    path = "vector" if nb % 4 == 0 else "scalar"
    check(f"plddt {c.name} atom ({path} loads)", atom.numpy(), a32, a64)
    check(f"plddt {c.name} mean ({path} loads)", mean.numpy(), m32, m64)
    if nb % 4 == 0:                                                   # the alignment fallback: scalar loads of the same floats
        atom_s, mean_s = plddt_call(shifted(lg), P, A, nb)
        check(f"plddt {c.name} atom (misaligned: scalar loads)", atom_s.numpy(), a32, a64)
        check(f"plddt {c.name} mean (misaligned: scalar loads)", mean_s.numpy(), m32, m64)
        print(f"plddt {c.name}: vector and scalar load paths bit-equal: {torch.equal(bits(atom), bits(atom_s)) and torch.equal(bits(mean), bits(mean_s))}")


# ------------------------------------------------------------------ pd_metrics_pae_tm
def pae_tm_call(c, lg, asym=True, pae=True, per=True, ws_fill=NAN):
    """dict of CPU tensors: pae [P,T,T], ptm, iptm [P], rows [P,2], per_alignment [P,2,T] (None where not asked for)"""
    ops, L = _ops()
    p, (P, T, nb) = ops.ptr, (c.P, c.T, c.nb)
    nws = L.pd_metrics_workspace_numel(P, T)
    assert nws == 64 + 2 * P * T * ((T + 15) // 16)
    n = {"pae": P * T * T, "ptm": P, "iptm": P, "rows": 2 * P, "per_alignment": 2 * P * T}
    o = {k: guarded(v, dtype=torch.int32 if k == "rows" else torch.float32) for k, v in n.items()}
    ws = guarded(nws, ws_fill)
    t = [dev(c.centres), dev(c.weights), dev(c.asym) if asym else None]
    rc = L.pd_metrics_pae_tm(p(lg), p(t[0]), p(t[1]), p(t[2]), p(ws), p(o["pae"]) if pae else None, p(o["ptm"]), p(o["iptm"]), p(o["rows"]),
                             p(o["per_alignment"]) if per else None, P, T, nb, ops.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guard_ok(ws, nws) and all(guard_ok(o[k], n[k]) for k in n), f"{c.name}: a guard was written"
    if not pae:
        assert guard_ok(o["pae"], 0)
    if not per:
        assert guard_ok(o["per_alignment"], 0)
    shape = {"pae": (P, T, T), "ptm": (P,), "iptm": (P,), "rows": (P, 2), "per_alignment": (P, 2, T)}
    return {k: o[k][:n[k]].cpu().reshape(shape[k]) for k in n if (pae or k != "pae") and (per or k != "per_alignment")}


def pae_tm_check(what, c, got, r64, r32):
    assert got["rows"].tolist() == r64["rows"].tolist(), f"{what}: rows"
    for k in ("pae", "ptm", "iptm", "per_alignment"):
        if k in got:
            check(f"{what} {k}", got[k].numpy(), r32[k], r64[k])
    P = c.P
    for q, k in enumerate(("ptm", "iptm")):                         # the value is per_alignment at the chosen row
        if "per_alignment" in got:
            assert torch.equal(got["per_alignment"][torch.arange(P), q, got["rows"][:, q].long()], got[k])


@functools.lru_cache(None)
def pae_tm_run(name):
    """the full call of a case, run twice (NaN and other garbage in the workspace: the same bits), kept for the module"""
    c = cc.pae_tm(name)
    lg = dev(c.logits)
    assert lg.data_ptr() % 16 == 0
    got = pae_tm_call(c, lg)
    assert same_bits(got, pae_tm_call(c, lg, ws_fill=GARBAGE)), name
    return got


@pytest.mark.parametrize("name", cc.PAE_TM)
def test_metrics_pae_tm(name):
    c = cc.pae_tm(name)
    r64, r32 = cc.pae_tm_ref(name)
    nsplit, chunk, iters = c.geometry
    pae_tm_check(f"pae_tm {name} (nsplit {nsplit}, chunk {chunk}, {iters} iterations, {'vector' if c.nb % 4 == 0 else 'scalar'} loads)", c,
                 pae_tm_run(name), r64, r32)


@pytest.mark.parametrize("name", ("1x257x64", "2x40x48", "1x65x50"))
def test_metrics_pae_tm_nullable_arguments_and_load_paths(name):
    c = cc.pae_tm(name)
    r64, r32 = cc.pae_tm_ref(name)
    full, lg = pae_tm_run(name), dev(c.logits)
    # pae = NULL, per_alignment = NULL: the other outputs keep their bits
    part = pae_tm_call(c, lg, pae=False, per=False)
    assert set(part) == {"ptm", "iptm", "rows"} and same_bits(part, {k: full[k] for k in part})
    # asym_id = NULL: one chain - ipTM 0 from row 0, pae and pTM unchanged
    one = pae_tm_call(c, lg, asym=False)
    assert not bits(one["iptm"]).any() and not one["rows"][:, 1].any() and not bits(one["per_alignment"][:, 1]).any()
    assert all(torch.equal(bits(one[k]), bits(full[k])) for k in ("pae", "ptm")) and torch.equal(one["rows"][:, 0], full["rows"][:, 0])
    assert torch.equal(bits(one["per_alignment"][:, 0]), bits(full["per_alignment"][:, 0]))
    if c.nb % 4 == 0:                                                 # the alignment fallback: scalar loads of the same floats
        s = pae_tm_call(c, shifted(lg))
        pae_tm_check(f"pae_tm {name} (misaligned: scalar loads)", c, s, r64, r32)
        print(f"pae_tm {name}: vector and scalar load paths bit-equal: {same_bits(s, full)}")


def test_split_invariance():
    """the logits of 1x257x64 (five blocks of 64 pairs per row) as slice 5 of 8x257x64 (one block of five iterations per row)"""
    one, stack = pae_tm_run("1x257x64"), pae_tm_run("8x257x64")
    assert cc.pae_tm("1x257x64").geometry[0] == 5 and cc.pae_tm("8x257x64").geometry[0] == 1
    for k in ("pae", "ptm", "iptm", "per_alignment"):
        assert torch.equal(bits(one[k][0]), bits(stack[k][cc.SLICE])), k
    assert torch.equal(one["rows"][0], stack["rows"][cc.SLICE])


@pytest.mark.parametrize("rows,T", (((0, 256), 257), ((200, 256), 257), ((3, 259), 260)))
def test_first_maximal_row_wins_a_tie(rows, T):
    """T 257, rows 0 and 256: the first and the second row of lane 0 of tm_final_kernel (its own strict > scan); rows 200 and 256: a
    lane with one row against the second row of lane 0 (the cross-lane rule); T 260, rows 3 and 259: the two rows of lane 3"""
    c = cc.tie(*rows, T=T)
    got = pae_tm_call(c, dev(c.logits))
    per = got["per_alignment"][0]
    assert got["rows"].tolist() == [[rows[0], rows[0]]], (rows, got["rows"].tolist())
    for q, k in enumerate(("ptm", "iptm")):
        assert torch.equal(bits(per[q, rows[0]]), bits(per[q, rows[1]])) and torch.equal(bits(got[k][0]), bits(per[q, rows[0]]))
        sel = per[q] * torch.from_numpy(c.weights)
        assert int((sel == sel.max()).sum()) == 2


# ------------------------------------------------------------------ pd_metrics_clash
@pytest.mark.parametrize("name", cc.CLASH)
def test_metrics_clash(name):
    ops, L = _ops()
    p, c = ops.ptr, cc.clash(name)
    counts, has, has_skip, _ = cc.clash_ref(name)
    B, A, nc = c.B, c.A, c.nc
    t = [dev(a) for a in (c.x_pred, c.a_mask, c.chain, c.polymer)]
    ptm, iptm = dev(c.ptm), dev(c.iptm)
    for skip, want in ((0, has), (1, has_skip)):
        for stride, rank in ((0, True), (1, True), (0, False)):
            cnt, hc, rk = guarded(B * nc * nc, dtype=torch.int32), guarded(B, dtype=torch.int64), guarded(B)
            rc = L.pd_metrics_clash(*(p(a) for a in t), p(cnt), p(ptm) if rank else None, p(iptm) if rank else None, stride, p(hc),
                                    p(rk) if rank else None, B, A, nc, skip, ops.stream())
            assert rc == 0, rc
            torch.cuda.synchronize()
            assert guard_ok(cnt, B * nc * nc) and guard_ok(hc, B) and guard_ok(rk, B if rank else 0)
            assert np.array_equal(cnt[:B * nc * nc].cpu().numpy().reshape(B, nc, nc), counts), (name, skip)
            assert hc[:B].cpu().tolist() == want.tolist(), (name, skip)
            if rank:
                sel = slice(None) if stride else slice(0, 1)
                check(f"clash {name} skip {skip} stride {stride} ranking", rk[:B].cpu().numpy(), cr.ranking(c.ptm[sel], c.iptm[sel], want, np.float32),
                      cr.ranking(c.ptm[sel], c.iptm[sel], want))
    print(f"clash {name}: counts {counts.sum((1, 2)).tolist()} has_clash {has.tolist()} / a < c only {has_skip.tolist()}: equal")


# ------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    """return codes of the confidence-loss launchers (those of metrics.hip: tests/test_metrics_gpu.py::test_launcher_guards)"""
    ops, L = _ops()
    p, s = ops.ptr, ops.stream()
    out, ws, g = guarded(0), guarded(0), guarded(0)
    sc = torch.ones(1, device="cuda")
    c = cc.lddt("mixed")
    keep = [dev(a) for a in (c.x_pred, c.x_gt, c.centre, c.is_dna, c.is_rna, c.is_polymer)]
    t = [p(a) for a in keep] + [p(out)]
    for k in range(7):
        u = list(t)
        u[k] = None
        assert L.pd_lddt_atoms(*u, c.B, c.A, c.T, s) == PD_ERR_ARG, k
    for B, A, T in ((0, c.A, c.T), (c.B, 0, c.T), (c.B, c.A, 0), (-1, c.A, c.T)):
        assert L.pd_lddt_atoms(*t, B, A, T, s) == PD_ERR_ARG
    assert L.pd_lddt_atoms(*t, 65536, c.A, c.T, s) == PD_ERR_UNSUPPORTED
    f = cc.frames(257)
    keepf = [dev(f.x)] + [dev(i) for i in f.ids]
    t = [p(a) for a in keepf] + [p(out)]
    for k in range(5):
        u = list(t)
        u[k] = None
        assert L.pd_conf_frames(*u, f.A, f.T, s) == PD_ERR_ARG, k
    assert L.pd_conf_frames(*t, 0, f.T, s) == PD_ERR_ARG and L.pd_conf_frames(*t, f.A, 0, s) == PD_ERR_ARG
    c = cc.plddt_loss(17, 64)
    keepl = [dev(c.logits), dev(c.lddt), dev(c.x_exists)]
    t = [p(a) for a in keepl]
    call = lambda a=t, nb=c.nb, sc_=p(sc), ws_=p(ws), out_=p(out), g_=p(g), A=c.A: L.pd_conf_loss_plddt(*a, nb, sc_, ws_, out_, g_, A, s)
    for k in range(3):
        u = list(t)
        u[k] = None
        assert call(a=u) == PD_ERR_ARG, k
    assert call(nb=0) == PD_ERR_ARG and call(nb=-1) == PD_ERR_ARG and call(nb=65) == PD_ERR_UNSUPPORTED and call(A=0) == PD_ERR_ARG
    assert call(ws_=None) == PD_ERR_ARG and call(out_=None) == PD_ERR_ARG
    assert call(sc_=None) == PD_ERR_ARG                                # a gradient without a scale
    c = cc.pairs("9x33")
    keepp = [dev(a) for a in (c.logits["pae"], c.x_pred0, c.x_gt, c.x_exists, c.centre, c.frames_pred, c.frames_gt)]
    t = [p(a) for a in keepp]
    def pairs(a=t, mode=1, nb=c.nb, sc_=p(sc), ws_=p(ws), out_=p(out), g_=p(g), A=c.A, T=c.T):
        return L.pd_conf_loss_pairs(mode, *a, c.min_bin, c.max_bin - c.min_bin, nb, sc_, ws_, out_, g_, A, T, s)
    for k in range(5):
        u = list(t)
        u[k] = None
        assert pairs(a=u) == PD_ERR_ARG and pairs(a=u, mode=0) == PD_ERR_ARG, k
    for k in (5, 6):                                                  # PAE without frames
        u = list(t)
        u[k] = None
        assert pairs(a=u) == PD_ERR_ARG, k
    for mode in (-1, 2, 3):
        assert pairs(mode=mode) == PD_ERR_ARG, mode
    assert pairs(nb=0) == PD_ERR_ARG and pairs(nb=65) == PD_ERR_UNSUPPORTED and pairs(nb=65, mode=0) == PD_ERR_UNSUPPORTED
    assert pairs(A=0) == PD_ERR_ARG and pairs(T=0) == PD_ERR_ARG and pairs(ws_=None) == PD_ERR_ARG and pairs(out_=None) == PD_ERR_ARG
    assert pairs(sc_=None) == PD_ERR_ARG and pairs(sc_=None, mode=0) == PD_ERR_ARG
    W = L.pd_conf_loss_workspace_numel
    assert W(0, 1, 1) == W(1, 0, 1) == W(1, 1, 0) == PD_ERR_ARG
    torch.cuda.synchronize()
    assert guard_ok(out, 0) and guard_ok(ws, 0) and guard_ok(g, 0)      # nothing was launched
