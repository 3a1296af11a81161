"""Kernel-level tests of the model's entry kernels, straight on the C ABI: csrc/features.hip (pd_target_feat, pd_msa_feat, pd_outer_mask,
pd_chain_contacts, pd_pdb_format), csrc/confidence.hip (pd_confidence_pair_init, pd_pair_symmetrize, pd_atom_dist_embed and the three
*_poses forms), pd_template_feat (csrc/pair.hip) and pd_chirality (csrc/sampler.hip).

Everything but one column is compared with torch.equal against the fp32 reference of tests/entry_kernels_ref.py (the module docstring
there says why each kernel is exact); the atan column of pd_msa_feat goes through the one rule of tests/test_sampler_kernels_gpu.py
(check_close: |dev - ref64| <= 4 E + 8 ulp32(max |ref64|); it prints E, the error, the bound and their ratio under pytest -s).

Every buffer a kernel writes is a slice of a larger allocation with a band in front of it and behind it (NaN for floats - the helpers
of tests/test_trunk_glue_kernels_gpu.py -, 0xA5 bytes and a sentinel number for unsigned char / int / long long); every output a
kernel must write completely holds the sentinel before the launch and none after it; the bands are checked after the launch.
The refusal tests pass only arguments the launcher rejects before it launches anything.

The inputs are the cached ``*_case`` functions of tests/entry_kernels_ref.py; tests/test_entry_kernels_ref_cpu.py asserts their
conditions without a GPU.

Not covered: the single-pose launchers of confidence.hip cast their block count to unsigned without the grid check of the pose forms
(bites above T * T * C / 4 = 2^40 threads, out of reach of a test shape).
"""
import math

import pytest
import torch

import entry_kernels_ref as er
import test_sampler_kernels_gpu as ts
import test_trunk_glue_kernels_gpu as gk
from test_trunk_glue_kernels_gpu import BAND, P, S, bands_intact, dev, guarded, ok

pytestmark = pytest.mark.gpu

L = gk.L                                 # the module-scoped fixture: ops._lib.init()
PD_OK, PD_ERR_ARG, PD_ERR_UNSUPPORTED = 0, -1, -3
F32 = torch.float32
SENT = {torch.uint8: 0xA5, torch.int32: -7777, torch.int64: -7777}


# ------------------------------------------------------------------ integer guard bands
def guarded_int(shape, dtype, init=None):
    """(allocation, view) of an unsigned char / int / long long buffer: BAND sentinels on either side, the view holds `init` or the sentinel"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * BAND,), SENT[dtype], dtype=dtype, device="cuda")
    view = buf[BAND:BAND + n].view(*shape)
    if init is not None:
        view.copy_(torch.as_tensor(init, dtype=dtype))
    return buf, view


def int_bands_intact(buf):
    torch.cuda.synchronize()
    return bool((buf[:BAND] == SENT[buf.dtype]).all() and (buf[-BAND:] == SENT[buf.dtype]).all())


def untouched(buf):
    torch.cuda.synchronize()
    return bool(torch.isnan(buf).all() if buf.dtype.is_floating_point else (buf == SENT[buf.dtype]).all())


def refused(L, name, args, pointers=(), counts=(), bufs=(), code=PD_ERR_ARG):
    """every required pointer NULL in turn, every count at each of its bad values in turn: `code`, and nothing written"""
    fn = getattr(L, name)
    for i in pointers:
        a = list(args)
        a[i] = None
        assert fn(*a) == code, (name, "argument", i, "NULL")
    for i, values in counts:
        for v in values:
            a = list(args)
            a[i] = v
            assert fn(*a) == code, (name, "argument", i, v)
    for buf in bufs:
        assert untouched(buf), name


# ------------------------------------------------------------------ pd_target_feat
def _target_args(c, out):
    T, NP = c["restype"].shape[0], c["profile"].shape[1]
    prof = dev(c["profile"]) if NP else torch.zeros(4, device="cuda")          # n_profile = 0: never read, but not NULL
    keep = (dev(c["restype"]), prof, dev(c["deletion_mean"]))
    return keep, [P(keep[0]), P(keep[1]), P(keep[2]), P(out), T, c["n_class"], NP, S()]


@pytest.mark.parametrize("n_profile", [0, 32])
@pytest.mark.parametrize("T", [1, 5, 300])
def test_target_feat(L, T, n_profile):
    """restype == n_class and restype == -1 match no column: today's behaviour, an all-zero one-hot, is pinned here"""
    c = er.target_case(T, n_profile)
    buf, out = guarded((T, 32 + n_profile + 1))
    keep, args = _target_args(c, out)
    ok(L.pd_target_feat(*args), "pd_target_feat")
    assert bands_intact(buf)
    res = out.cpu()
    assert torch.equal(res, er.target_feat(**c))
    for t in range(min(T, 4)):
        assert float(res[t, :32].sum()) == (1.0 if t < 2 else 0.0)


# ------------------------------------------------------------------ pd_msa_feat
MSA_CASES = [(R, T, 32) for R in (1, 3, 5) for T in (1, 7)] + [(3, 7, 3)]


@pytest.mark.parametrize("R,T,n_class", MSA_CASES)
def test_msa_feat(L, R, T, n_class):
    c = er.msa_case(R, T, n_class)
    W = n_class + 2
    msa, dele, inds = dev(c["msa"]), dev(c["deletion"]), dev(c["inds"])
    buf, out = guarded((R, T, W))
    ok(L.pd_msa_feat(P(msa), P(dele), P(inds), er.TWO_OVER_PI, P(out), R, T, n_class, S()), "pd_msa_feat")
    assert bands_intact(buf)
    res = out.cpu()
    assert torch.equal(res[..., :W - 1], er.msa_feat_exact(**c))
    ts.check_close("msa_feat atan", f"R={R} T={T} n_class={n_class}", res[..., W - 1],
                   er.msa_feat_atan(c["deletion"], c["inds"], er.TWO_OVER_PI, F32), er.msa_feat_atan(c["deletion"], c["inds"], er.TWO_OVER_PI))


# ------------------------------------------------------------------ pd_outer_mask
@pytest.mark.parametrize("N", [1, 17, 257])
def test_outer_mask(L, N):
    m = er.outer_mask_case(N)
    md = dev(m)
    buf, out = guarded((N, N))
    ok(L.pd_outer_mask(P(md), P(out), N, S()), "pd_outer_mask")
    assert bands_intact(buf)
    assert torch.equal(out.cpu(), er.outer_mask(m))


# ------------------------------------------------------------------ pd_chain_contacts
def _contacts(L, c, n_pairs=None, with_min=True, with_arg=True, zeroed=True):
    """launch on guarded buffers -> (rc, between, min, arg, allocations)"""
    T = c["T"]
    n = c["pairs"].shape[0] if n_pairs is None else n_pairs
    keep = [dev(c[k]) for k in ("x", "a_mask", "chain_start", "pairs", "a2t")]
    bb, between = guarded((T, T), torch.zeros(T, T) if zeroed else None)
    mb, mins = guarded((max(n, 1),))
    ab, args = guarded_int((max(n, 1),), torch.int64)
    rc = L.pd_chain_contacts(P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), n, P(keep[4]), c["threshold"], P(between), T,
                             P(mins) if with_min else None, P(args) if with_arg else None, S())
    torch.cuda.synchronize()
    return rc, between, mins, args, (bb, mb, ab)


def _check_contacts(c, rc, between, mins, args, bufs, want):
    assert rc == PD_OK
    assert bands_intact(bufs[0]) and bands_intact(bufs[1]) and int_bands_intact(bufs[2])
    wmin, warg, wbetween = want
    assert torch.equal(args.cpu(), warg), (args.cpu().tolist(), warg.tolist())
    assert torch.equal(mins.cpu(), wmin)
    res = between.cpu()
    assert torch.equal(res, wbetween) and torch.equal(res, res.T)


def test_chain_contacts_ties_masks_threshold_and_empty_chains(L):
    c, expect = er.chain_contacts_case()
    want = er.chain_contacts(**c)
    rc, between, mins, args, bufs = _contacts(L, c)
    _check_contacts(c, rc, between, mins, args, bufs, want)
    for (name, *_), k, got, v in zip(er.CONTACT_SCENARIOS, expect, args.cpu().tolist(), mins.cpu().tolist()):
        assert k is None or got == k, name
        assert not name.startswith("empty") or (got == -1 and v == er.INF), name
        assert name != "second chain fully masked" or v >= 1000.0, name


def test_chain_contacts_against_the_oracle_case(L):
    c, _ = er.chain_contacts_oracle_case()
    rc, between, mins, args, bufs = _contacts(L, c)
    _check_contacts(c, rc, between, mins, args, bufs, er.chain_contacts(**c))


@pytest.mark.parametrize("with_min,with_arg", [(False, True), (True, False), (False, False)])
def test_chain_contacts_optional_outputs(L, with_min, with_arg):
    c, _ = er.chain_contacts_case()
    wmin, warg, wbetween = er.chain_contacts(**c)
    rc, between, mins, args, bufs = _contacts(L, c, with_min=with_min, with_arg=with_arg)
    assert rc == PD_OK and bands_intact(bufs[0])
    assert torch.equal(between.cpu(), wbetween)
    assert torch.equal(mins.cpu(), wmin) if with_min else untouched(bufs[1])
    assert torch.equal(args.cpu(), warg) if with_arg else untouched(bufs[2])


def test_chain_contacts_without_pairs_writes_nothing(L):
    c, _ = er.chain_contacts_case()
    rc, _, _, _, bufs = _contacts(L, c, n_pairs=0, zeroed=False)
    assert rc == PD_OK and all(untouched(b) for b in bufs)


def test_chain_contacts_refusals(L):
    c, _ = er.chain_contacts_case()
    keep = [dev(c[k]) for k in ("x", "a_mask", "chain_start", "pairs", "a2t")]
    bb, between = guarded((c["T"], c["T"]))
    mb, mins = guarded((13,))
    ab, args = guarded_int((13,), torch.int64)
    a = [P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), 13, P(keep[4]), 2.5, P(between), c["T"], P(mins), P(args), S()]
    refused(L, "pd_chain_contacts", a, pointers=(0, 1, 2, 3, 5, 7), counts=((4, (-1,)), (8, (0, -1))), bufs=(bb, mb, ab))


# ------------------------------------------------------------------ pd_chirality
def _chirality(L, c, ref_sign, want_sign, want_accept, mode):
    B, nc, A = c["x"].shape[0], c["nc"], c["A"]
    x = dev(c["x"])
    cen = dev(c["centres"]) if nc else torch.zeros(4, dtype=torch.int32, device="cuda")       # n_centres = 0: never read, not NULL
    ref = dev(ref_sign) if nc else torch.zeros(1, dtype=torch.int32, device="cuda")
    ab, acc = guarded_int((B,), torch.int32)
    sb, sg = guarded_int((B * max(nc, 1),), torch.int32)          # n_centres = 0: a buffer that must stay as it is
    use_acc, use_sg = mode != "sign", mode != "accept"
    ok(L.pd_chirality(P(x), P(cen), P(ref) if use_acc else None, P(acc) if use_acc else None, P(sg) if use_sg else None, B, A, nc, S()),
       "pd_chirality")
    assert int_bands_intact(ab) and int_bands_intact(sb)
    assert torch.equal(sg.cpu().reshape(B, -1), want_sign) if use_sg and nc else untouched(sb)
    assert torch.equal(acc.cpu(), want_accept) if use_acc else untouched(ab)


@pytest.mark.parametrize("mode", ["both", "sign", "accept"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nc", er.CHIRALITY_N)
def test_chirality(L, nc, B, mode):
    """pose 0 (rotated, translated) accepted; the mirror image and the flat pose rejected; no centre: every pose accepted"""
    c = er.chirality_case(nc, B)
    ref_sign, ref_ok = er.chirality_sign(c["x_ref"][None], c["centres"])
    sign, decided = er.chirality_sign(c["x"], c["centres"])
    assert ref_ok.all() and decided.all()
    accept = er.chirality_accept(sign, ref_sign[0])
    assert accept.tolist() == ([1] * B if nc == 0 else [1, 0, 0][:B])
    _chirality(L, c, ref_sign[0], sign, accept, mode)


@pytest.mark.parametrize("mode", ["both", "accept"])
def test_chirality_one_flipped_centre(L, mode):
    """130 centres: a mismatch only at centre 0, only at 64 (lane 0, second trip), only at 129 (lane 1, third trip)"""
    c = er.chirality_flip_case()
    ref_sign, _ = er.chirality_sign(c["x_ref"][None], c["centres"])
    sign, decided = er.chirality_sign(c["x"], c["centres"])
    assert decided.all()
    accept = er.chirality_accept(sign, ref_sign[0])
    assert accept.tolist() == [1, 0, 0, 0]
    for p, k in enumerate(c["flipped"]):
        assert (sign[p] != ref_sign[0]).nonzero().flatten().tolist() == ([] if k is None else [k])
    _chirality(L, c, ref_sign[0], sign, accept, mode)


def test_chirality_refusals(L):
    c = er.chirality_case(65, 3)
    x, cen = dev(c["x"]), dev(c["centres"])
    ref = torch.ones(65, dtype=torch.int32, device="cuda")
    ab, acc = guarded_int((3,), torch.int32)
    sb, sg = guarded_int((3, 65), torch.int32)
    a = [P(x), P(cen), P(ref), P(acc), P(sg), 3, c["A"], 65, S()]
    refused(L, "pd_chirality", a, pointers=(0, 1), counts=((5, (0, -1)), (6, (0, -1)), (7, (-1,))), bufs=(ab, sb))
    assert L.pd_chirality(P(x), P(cen), P(ref), None, None, 3, c["A"], 65, S()) == PD_ERR_ARG          # neither output
    assert L.pd_chirality(P(x), P(cen), None, P(acc), P(sg), 3, c["A"], 65, S()) == PD_ERR_ARG          # accept without ref_sign
    assert untouched(ab) and untouched(sb)


# ------------------------------------------------------------------ pd_template_feat
def _template(L, c):
    T, NB = c["pb"].shape[0], c["lower"].shape[0]
    keep = [dev(c[k]) for k in ("x", "pb", "z_mask", "is_protein", "lower")]
    buf, out = guarded((T, T, NB + 1))
    ok(L.pd_template_feat(*[P(k) for k in keep], P(out), T, NB, S()), "pd_template_feat")
    assert bands_intact(buf)
    return out.cpu()


@pytest.mark.parametrize("NB", [1, 4, 39])
@pytest.mark.parametrize("T", [1, 17])
def test_template_feat_on_the_edges(L, T, NB):
    c = er.template_edges_case(T, NB)
    assert torch.equal(_template(L, c), er.template_feat(**c))


def test_template_feat_production_edges(L):
    c = er.template_random_case()
    assert torch.equal(_template(L, c), er.template_feat(**c))


def test_template_feat_refusals(L):
    c = er.template_edges_case(17, 4)
    keep = [dev(c[k]) for k in ("x", "pb", "z_mask", "is_protein", "lower")]
    buf, out = guarded((17, 17, 5))
    a = [*[P(k) for k in keep], P(out), 17, 4, S()]
    refused(L, "pd_template_feat", a, pointers=range(6), counts=((6, (0, -1)), (7, (0, -1))), bufs=(buf,))


# ------------------------------------------------------------------ confidence.hip
def _centres(T):
    return er.centre_rows() if T == 9 else (torch.tensor([2] * T),)


#: (P, padding floats between poses; None: x_stride = 0, every pose reads pose 0)
POSE_LAYOUTS = [(1, 0), (3, 0), (3, 5), (3, None)]


def _pose_case(make, *shape, P_, pad):
    c = make(*shape, P=1 if pad is None else P_, pad=pad or 0)
    stride = 0 if pad is None else c["stride"]
    return c, stride, er.pose_coordinates(c["x"], stride, c["A"], P_)


@pytest.mark.parametrize("T,C", er.CONF_SHAPES)
def test_confidence_pair_init(L, T, C):
    c = er.confidence_case(T, C)
    z, si, sj, WdT, x = (dev(c[k]) for k in ("z", "si", "sj", "WdT", "x"))
    for centre in _centres(T):
        cd = dev(centre)
        buf, out = guarded((T, T, C))
        ok(L.pd_confidence_pair_init(P(z), P(si), P(sj), P(WdT), P(x), P(cd), P(out), T, C, S()), "pd_confidence_pair_init")
        assert bands_intact(buf)
        assert torch.equal(out.cpu(), er.confidence_pair_init(c["z"], c["si"], c["sj"], c["WdT"], c["x"].reshape(-1, 3), centre))


def test_confidence_bins_at_midpoints_and_ends(L):
    """z = si = sj = 0 and WdT[k, :] = k: the output IS the bin.  Atom 0 against the axis: 0, 3.375 and 4.25 -> bin 0, every
    midpoint -> the lower bin, 24.375 and everything beyond -> bin 12; all 13 bins occur"""
    T, C = 17, 4
    A = len(er.CENTRE_AXIS)
    x = torch.zeros(A, 3)
    x[:, 0] = torch.tensor(er.CENTRE_AXIS)
    zero2, zero1 = torch.zeros(T, T, C, device="cuda"), torch.zeros(T, C, device="cuda")
    WdT, xd, cd = dev(torch.arange(13.0)[:, None].expand(13, C)), dev(x), dev(torch.arange(T))
    buf, out = guarded((T, T, C))
    ok(L.pd_confidence_pair_init(P(zero2), P(zero1), P(zero1), P(WdT), P(xd), P(cd), P(out), T, C, S()), "pd_confidence_pair_init")
    assert bands_intact(buf)
    res = out.cpu()
    assert res[0, :, 0].tolist() == [0, 0] + list(range(12)) + [12, 12, 12]
    assert torch.equal(res[..., 0].long(), er.nearest_bin(er.centre_distance(x, torch.arange(T)))) and torch.equal(res[..., 0], res[..., 3])
    assert set(res[0, :, 0].tolist()) == set(range(13))


@pytest.mark.parametrize("P_,pad", POSE_LAYOUTS)
@pytest.mark.parametrize("T,C", er.CONF_SHAPES)
def test_confidence_pair_init_poses(L, T, C, P_, pad):
    """every pose bit-equal to the single-pose kernel on that pose's coordinates, and to the reference"""
    c, stride, poses = _pose_case(er.confidence_case, T, C, P_=P_, pad=pad)
    z, si, sj, WdT, x = (dev(c[k]) for k in ("z", "si", "sj", "WdT", "x"))
    centre = _centres(T)[-1]
    cd = dev(centre)
    buf, out = guarded((P_, T, T, C))
    ok(L.pd_confidence_pair_init_poses(P(z), P(si), P(sj), P(WdT), P(x), P(cd), P(out), T, C, P_, stride, S()),
       "pd_confidence_pair_init_poses")
    assert bands_intact(buf)
    res = out.cpu()
    for p in range(P_):
        xp = x[p * stride:]
        b1, one = guarded((T, T, C))
        ok(L.pd_confidence_pair_init(P(z), P(si), P(sj), P(WdT), P(xp), P(cd), P(one), T, C, S()), "pd_confidence_pair_init")
        assert bands_intact(b1)
        assert torch.equal(res[p], one.cpu()), p
        assert torch.equal(res[p], er.confidence_pair_init(c["z"], c["si"], c["sj"], c["WdT"], poses[p], centre)), p


@pytest.mark.parametrize("P_", [1, 3])
@pytest.mark.parametrize("T,C", er.CONF_SHAPES)
def test_pair_symmetrize(L, T, C, P_):
    z = torch.randn(P_, T, T, C, generator=er.gen(5200 + T + C + P_))
    zd = dev(z)
    want = torch.stack([er.pair_symmetrize(z[p]) for p in range(P_)])
    assert torch.equal(torch.diagonal(want, dim1=1, dim2=2), 2 * torch.diagonal(z, dim1=1, dim2=2))
    buf, out = guarded((P_, T, T, C))
    ok(L.pd_pair_symmetrize_poses(P(zd), P(out), T, C, P_, S()), "pd_pair_symmetrize_poses")
    assert bands_intact(buf)
    assert torch.equal(out.cpu(), want)
    for p in range(P_):
        buf, one = guarded((T, T, C))
        ok(L.pd_pair_symmetrize(P(zd[p]), P(one), T, C, S()), "pd_pair_symmetrize")
        assert bands_intact(buf)
        assert torch.equal(one.cpu(), want[p])
    assert torch.equal(zd.cpu(), z)


@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("P_,pad", POSE_LAYOUTS)
@pytest.mark.parametrize("C", [4, 16])
@pytest.mark.parametrize("A", [1, 9, 23])
def test_atom_dist_embed(L, A, C, P_, pad, with_b):
    """the pose form against the reference, and every pose bit-equal to the single-pose kernel"""
    c, stride, poses = _pose_case(er.embed_case, A, C, P_=P_, pad=pad)
    x, w, b = dev(c["x"]), dev(c["w"]), dev(c["b"]) if with_b else None
    buf, out = guarded((P_, A, A, C))
    ok(L.pd_atom_dist_embed_poses(P(x), P(w), P(b), P(out), A, C, P_, stride, S()), "pd_atom_dist_embed_poses")
    assert bands_intact(buf)
    res = out.cpu()
    for p in range(P_):
        b1, one = guarded((A, A, C))
        ok(L.pd_atom_dist_embed(P(x[p * stride:]), P(w), P(b), P(one), A, C, S()), "pd_atom_dist_embed")
        assert bands_intact(b1)
        assert torch.equal(res[p], one.cpu()), p
        assert torch.equal(res[p], er.atom_dist_embed(poses[p], c["w"], c["b"] if with_b else None)), p
    if A > 1:
        assert torch.equal(res[:, 0, 1], (c["b"] if with_b else torch.zeros(C)).expand(P_, C))           # d = 0


def test_confidence_refusals(L):
    T, C, A, Pn = 9, 36, 20, 3
    c = er.confidence_case(T, C, P=Pn)
    z, si, sj, WdT, x = (dev(c[k]) for k in ("z", "si", "sj", "WdT", "x"))
    cd, w = dev(er.centre_rows()[0]), torch.ones(C, device="cuda")
    zp = torch.zeros(Pn, T, T, C, device="cuda")
    buf, out = guarded((Pn, T, T, C))
    ab, ap = guarded((Pn, A, A, C))
    st = c["stride"]
    init = [P(z), P(si), P(sj), P(WdT), P(x), P(cd), P(out), T, C]
    tc = ((7, (0, -1)), (8, (0, -1)))
    refused(L, "pd_confidence_pair_init", init + [S()], range(7), tc, (buf,))
    refused(L, "pd_confidence_pair_init_poses", init + [Pn, st, S()], range(7), tc + ((9, (0, -1)), (10, (-1,))), (buf,))
    refused(L, "pd_pair_symmetrize", [P(zp), P(out), T, C, S()], (0, 1), ((2, (0, -1)), (3, (0, -1))), (buf,))
    refused(L, "pd_pair_symmetrize_poses", [P(zp), P(out), T, C, Pn, S()], (0, 1), ((2, (0, -1)), (3, (0, -1)), (4, (0, -1))), (buf,))
    emb = [P(x), P(w), P(w), P(ap), A, C]
    refused(L, "pd_atom_dist_embed", emb + [S()], (0, 1, 3), ((4, (0, -1)), (5, (0, -1))), (ab,))
    refused(L, "pd_atom_dist_embed_poses", emb + [Pn, st, S()], (0, 1, 3), ((4, (0, -1)), (5, (0, -1)), (6, (0, -1)), (7, (-1,))), (ab,))
    # a channel count that is no multiple of four
    for name, args, i in (("pd_confidence_pair_init", init + [S()], 8), ("pd_confidence_pair_init_poses", init + [Pn, st, S()], 8),
                          ("pd_pair_symmetrize", [P(zp), P(out), T, C, S()], 3), ("pd_pair_symmetrize_poses", [P(zp), P(out), T, C, Pn, S()], 3),
                          ("pd_atom_dist_embed", emb + [S()], 5), ("pd_atom_dist_embed_poses", emb + [Pn, st, S()], 5)):
        refused(L, name, args, counts=((i, (6, 34)),), bufs=(buf, ab), code=PD_ERR_UNSUPPORTED)
    # in place
    assert L.pd_pair_symmetrize(P(out), P(out), T, C, S()) == PD_ERR_ARG
    assert L.pd_pair_symmetrize_poses(P(out), P(out), T, C, Pn, S()) == PD_ERR_ARG
    assert untouched(buf)


# ------------------------------------------------------------------ features.hip refusals
def test_feature_refusals(L):
    c = er.target_case(5, 32)
    buf, out = guarded((5, 65))
    keep, a = _target_args(c, out)
    refused(L, "pd_target_feat", a, range(4), ((4, (0, -1)), (5, (0, -1)), (6, (-1,))), (buf,))
    m = er.msa_case(3, 7, 32)
    msa, dele, inds = dev(m["msa"]), dev(m["deletion"]), dev(m["inds"])
    buf, out = guarded((3, 7, 34))
    a = [P(msa), P(dele), P(inds), er.TWO_OVER_PI, P(out), 3, 7, 32, S()]
    refused(L, "pd_msa_feat", a, (0, 1, 2, 4), ((5, (0, -1)), (6, (0, -1)), (7, (0, -1))), (buf,))
    md = dev(er.outer_mask_case(17))
    buf, out = guarded((17, 17))
    refused(L, "pd_outer_mask", [P(md), P(out), 17, S()], (0, 1), ((2, (0, -1)),), (buf,))


# ------------------------------------------------------------------ pd_pdb_format
def _pdb(L, c, preset=0):
    B, N, A = c["x"].shape[0], c["atom"].shape[0], c["A"]
    x, tmpl, atom = dev(c["x"]), dev(c["tmpl"]), dev(c["atom"])
    ob, out = guarded_int((B, N, 81), torch.uint8)
    cb, count = guarded_int((1,), torch.int32, [preset])
    ok(L.pd_pdb_format(P(x), P(tmpl), P(atom), P(out), P(count), B, A, N, S()), "pd_pdb_format")
    assert int_bands_intact(ob) and int_bands_intact(cb)
    return out.cpu(), int(count.cpu())


@pytest.mark.parametrize("N", [1, 7])
@pytest.mark.parametrize("B", [1, 3])
def test_pdb_format(L, B, N):
    c = er.pdb_case(B, N)
    want, bad = er.pdb_format(c["x"], c["tmpl"], c["atom"])
    out, count = _pdb(L, c)
    assert bad == 0 and count == 0
    assert torch.equal(out, want)
    keep = [col for col in range(81) if not 30 <= col < 54]
    assert torch.equal(out[:, :, keep], c["tmpl"][None, :, keep].expand(B, N, len(keep)))


@pytest.mark.parametrize("preset", [0, 5])
def test_pdb_format_bad_fields_and_limits(L, preset):
    """one bad field per record for -1000, 10000, inf and nan: eight '*' there, the two other fields of the record formatted; the
    decimal limits (as fp32 numbers: -999.9995 does not fit, the others do); *overflow counts the bad fields on top of its preset"""
    c = er.pdb_bad_case()
    want, bad = er.pdb_format(c["x"], c["tmpl"], c["atom"])
    out, count = _pdb(L, c, preset)
    assert torch.equal(out, want)
    assert bad == len(er.BAD_VALUES) + 1 and count == preset + bad
    stars = (out[:, :, 30:54] == ord("*")).reshape(3, 7, 3, 8)
    assert int(stars.sum()) == 8 * bad and set(stars.sum(-1).flatten().tolist()) == {0, 8}
    for k in range(len(er.BAD_VALUES)):
        assert stars[k % 3, k].all(-1).tolist() == [f == k % 3 for f in range(3)]
    assert stars[0, 4].all(-1).tolist() == [False, False, False] and stars[0, 5].all(-1).tolist() == [False, True, False]


def test_pdb_format_no_records_and_refusals(L):
    c = er.pdb_case(3, 7)
    x, tmpl, atom = dev(c["x"]), dev(c["tmpl"]), dev(c["atom"])
    ob, out = guarded_int((3, 7, 81), torch.uint8)
    cb, count = guarded_int((1,), torch.int32)
    a = [P(x), P(tmpl), P(atom), P(out), P(count), 3, c["A"], 7, S()]
    assert L.pd_pdb_format(*a[:7], 0, S()) == PD_OK                                                # N == 0
    assert untouched(ob) and untouched(cb)
    refused(L, "pd_pdb_format", a, range(5), ((5, (0, -1)), (6, (0, -1)), (7, (-1,))), (ob, cb))
