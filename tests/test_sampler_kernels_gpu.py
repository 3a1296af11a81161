"""Kernel-level parity of the per-step sampler kernels (csrc/sampler.hip) and of the Philox draws, straight on the C ABI.

Every floating-point comparison follows ONE rule.  For a case, ref64 is the float64 reference (tests/sampler_ref.py) and ref32 the
same operation in fp32 on the CPU (the oracle function where one exists, else the same formula in torch float32);
E = max|ref32 - ref64| is what fp32 arithmetic alone costs on that input.  The device must satisfy

    |dev - ref64| <= TOL_FACTOR * E + TOL_FLOOR_ULPS * ulp32(max|ref64|)

with E and the floor taken per sample for the block-per-sample kernels (augment, Kabsch, template eps), so that one
ill-conditioned sample does not loosen the others.  The factor is two bits of allowance for another summation order (four-wave tree
against torch's pairwise sums) and the device's logf / sincosf / expf; the floor covers inputs where ref32 happens to be exact.
Everything without arithmetic (gather, scatter, selections, untouched elements, shard invariance) is compared with torch.equal.
Every output buffer is one row longer than needed and pre-filled with a sentinel (NaN, -7 for ints).

The input generators (``*_case`` functions, CPU tensors only) are imported by tests/test_sampler_ref_cpu.py, which asserts their
conditions (Kabsch conditioning, template selection gaps, the moments of the pooled draws) without a GPU.

Not covered: the 64-bit index instantiation of precond_kernel needs more than 2^31 output quads (about 34 GB of output).
pd_euler is never called in place by the sampler loop (model.py: x_hat -> x_a, two buffers; the kernel's pointers are
__restrict__), so aliasing x_next with x_hat is not part of the contract and is not tested.
"""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import physdock_oracle as orc
import sampler_ref as sr

pytestmark = pytest.mark.gpu

#: the two constants of the tolerance rule (module docstring)
TOL_FACTOR = 4.0
TOL_FLOOR_ULPS = 8.0

PD_ERR_ARG = -1
LAM = float(np.float32(1.003))          # noise_scale_lambda as the kernel receives it
NAN = float("nan")


# ------------------------------------------------------------------ rule, sentinels, plumbing
def _ulp32(t):
    s = t.abs().float()
    return (torch.nextafter(s, torch.full_like(s, float("inf"))) - s).double()


def tolerance(ref32, ref64, per_sample):
    """(bound, E) of the rule, broadcastable against ref64"""
    d = (ref32.double() - ref64).abs()
    if per_sample:
        shape = (ref64.shape[0],) + (1,) * (ref64.dim() - 1)
        E = d.flatten(1).amax(1).reshape(shape)
        scale = ref64.abs().flatten(1).amax(1).reshape(shape)
    else:
        E, scale = d.max(), ref64.abs().max()
    return TOL_FACTOR * E + TOL_FLOOR_ULPS * _ulp32(scale), E


def check_close(kernel, case, dev, ref32, ref64, per_sample=False):
    dev = dev.detach().cpu().double()
    assert dev.shape == ref64.shape, (kernel, case, dev.shape, ref64.shape)
    assert torch.isfinite(dev).all(), (kernel, case, "non-finite output")
    bound, E = tolerance(ref32, ref64, per_sample)
    err = (dev - ref64).abs()
    ratio = float((err / bound).max())
    # one line per comparison (pytest -s shows them): the source of the table in NOTES.md
    print(f"ENVELOPE | {kernel} | {case} | {float(E.max()):.2e} | {float(err.max()):.2e} | {float(bound.max()):.2e} | {ratio:.2f} |")
    assert ratio <= 1.0, (kernel, case, "E", float(E.max()), "err", float(err.max()), "err/bound", ratio)


def sentinel(*shape, dtype=torch.float32):
    """an output buffer of `shape` plus one tail row, filled with NaN (-7 for integers)"""
    fill = NAN if dtype.is_floating_point else -7
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")


def is_sentinel(t):
    return torch.isnan(t) if t.dtype.is_floating_point else t == -7


def body(buf, written=True):
    """the output rows of a sentinel buffer, after checking the tail row (and, if written, that no sentinel survived)"""
    torch.cuda.synchronize()
    assert is_sentinel(buf[-1]).all(), "the row behind the output was written"
    if written:
        assert not is_sentinel(buf[:-1]).any(), "an output element kept its sentinel"
    return buf[:-1]


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


def random_rotation(g):
    q = torch.randn(4, generator=g, dtype=torch.float64)
    w, x, y, z = (q / q.norm()).tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


# ------------------------------------------------------------------ pd_denoise
DENOISE_C = [4, 36, 64, 128, 132, 384, 512]
DENOISE_BA = [(1, 1), (3, 7), (5, 257)]


def denoise_case(B, A, C, seed=0):
    g = gen(1000 + seed + 7 * C + A)
    return dict(ba=50.0 + torch.randn(B, A, C, generator=g), x_hat=torch.randn(B, A, 3, generator=g) * 30,
                nw=1.0 + 0.3 * torch.randn(C, generator=g), nb=0.2 * torch.randn(C, generator=g),
                Wr=torch.randn(3, C, generator=g) / math.sqrt(C) * torch.tensor([[1.0], [-2.0], [0.5]]),
                cs_b=0.1 + 0.8 * torch.rand(B, generator=g) + 0.01 * torch.arange(B), co_b=1.0 + torch.arange(B) * 0.7)


def _denoise32(c, eps, cs, co):
    r = F.linear(F.layer_norm(c["ba"], c["ba"].shape[-1:], c["nw"], c["nb"], eps), c["Wr"])
    return cs * c["x_hat"] + co * r


@pytest.mark.parametrize("B,A,C", [(b, a, c) for c in DENOISE_C for (b, a) in DENOISE_BA] + [(64, 2056, 128)])
def test_pd_denoise(L, B, A, C):
    c = denoise_case(B, A, C)
    d = {k: dev(v) for k, v in c.items()}
    assert (B * A) % 8 != 0 or (B, A) == (64, 2056)
    for eps, per_sample in itertools.product((1e-5, 1e-8), (False, True)):
        out = sentinel(B, A, 3)
        if per_sample:
            rc = L.pd_denoise(P(d["ba"]), P(d["x_hat"]), P(d["nw"]), P(d["nb"]), P(d["Wr"]), eps, 0.0, 0.0, P(d["cs_b"]),
                              P(d["co_b"]), P(out), B, A, C, S())
            cs, co = c["cs_b"], c["co_b"]
            cs32, co32 = cs[:, None, None], co[:, None, None]
        else:
            cs, co = 0.375, 2.25
            rc = L.pd_denoise(P(d["ba"]), P(d["x_hat"]), P(d["nw"]), P(d["nb"]), P(d["Wr"]), eps, cs, co, None, None, P(out),
                              B, A, C, S())
            cs32, co32 = cs, co
        ok(rc, "pd_denoise")
        ref64 = sr.denoise64(c["ba"], c["x_hat"], c["nw"], c["nb"], c["Wr"], eps, cs, co)
        check_close("pd_denoise", f"B={B} A={A} C={C} eps={eps:g} {'per-sample' if per_sample else 'scalar'}", body(out),
                    _denoise32(c, eps, cs32, co32), ref64)


@pytest.mark.parametrize("C", [516, 6])
def test_pd_denoise_rejects_unsupported_widths(L, C):
    c = {k: dev(v) for k, v in denoise_case(2, 5, 520).items()}
    out = sentinel(2, 5, 3)
    rc = L.pd_denoise(P(c["ba"]), P(c["x_hat"]), P(c["nw"]), P(c["nb"]), P(c["Wr"]), 1e-5, 0.5, 0.5, None, None, P(out), 2, 5, C, S())
    assert rc != 0
    assert is_sentinel(body(out, written=False)).all()


# ------------------------------------------------------------------ pd_precond / pd_precond_g
C_IN = 11.0 / 256.0          # exact in fp32, as every scalar handed to a kernel by value here


def precond_case(G, B, A, C, seed=0):
    g = gen(2000 + seed + C + 13 * A + G)
    return dict(x_hat=torch.randn(G * B, A, 3, generator=g) * 40, Wx=torch.randn(C, 3, generator=g), bx=torch.randn(C, generator=g),
                a=torch.randn(G, A, C, generator=g) * 3 + torch.arange(G)[:, None, None],
                c_in_b=0.01 + 0.05 * torch.rand(G * B, generator=g) + 0.003 * torch.arange(G * B))


def _precond32(x_hat, c_in, Wx, bx, a):
    return F.linear(x_hat * c_in, Wx, bx) + a[None]


@pytest.mark.parametrize("C", [4, 64, 128, 384])
@pytest.mark.parametrize("A", [1, 91, 257])
@pytest.mark.parametrize("B", [1, 5])
def test_pd_precond(L, B, A, C):
    c = precond_case(1, B, A, C)
    d = {k: dev(v) for k, v in c.items()}
    for per_sample in (False, True):
        out = sentinel(B, A, C)
        cin = c["c_in_b"] if per_sample else C_IN
        ok(L.pd_precond(P(d["x_hat"]), 0.0 if per_sample else cin, P(d["c_in_b"]) if per_sample else None, P(d["Wx"]), P(d["bx"]),
                        P(d["a"]), P(out), B, A, C, S()), "pd_precond")
        ref32 = _precond32(c["x_hat"], cin[:, None, None] if per_sample else cin, c["Wx"], c["bx"], c["a"][0])
        check_close("pd_precond", f"B={B} A={A} C={C} {'per-sample' if per_sample else 'scalar'}", body(out), ref32,
                    sr.precond64(c["x_hat"], cin, c["Wx"], c["bx"], c["a"][0]))


@pytest.mark.parametrize("C", [4, 64, 128, 384])
@pytest.mark.parametrize("A", [1, 91, 257])
@pytest.mark.parametrize("G,B", [(1, 5), (3, 1), (3, 5)])
def test_pd_precond_g(L, G, B, A, C):
    c = precond_case(G, B, A, C, seed=5)
    d = {k: dev(v) for k, v in c.items()}
    assert len(set(c["c_in_b"].tolist())) == G * B
    for per_sample in (False, True):
        out = sentinel(G * B, A, C)
        ok(L.pd_precond_g(P(d["x_hat"]), 0.0 if per_sample else C_IN, P(d["c_in_b"]) if per_sample else None, P(d["Wx"]),
                          P(d["bx"]), P(d["a"]), P(out), G, B, A, C, S()), "pd_precond_g")
        r32, r64 = [], []
        for gi in range(G):
            sl = slice(gi * B, (gi + 1) * B)
            cin = c["c_in_b"][sl] if per_sample else C_IN
            r32.append(_precond32(c["x_hat"][sl], cin[:, None, None] if per_sample else cin, c["Wx"], c["bx"], c["a"][gi]))
            r64.append(sr.precond64(c["x_hat"][sl], cin, c["Wx"], c["bx"], c["a"][gi]))
        check_close("pd_precond_g", f"G={G} B={B} A={A} C={C} {'per-sample' if per_sample else 'scalar'}", body(out),
                    torch.cat(r32), torch.cat(r64))


# ------------------------------------------------------------------ pd_kabsch_align
#: (A, B, pred_mask, per-sample target, weights, offset, target kind); every variant of each column appears at least once
KABSCH_CASES = [
    (3, 1, False, False, "uniform", 0.0, "plain"),
    (3, 4, False, True, "random", 0.0, "plain"),
    (5, 1, False, False, "random", 0.0, "mirrored"),
    (5, 4, False, True, "uniform", 1000.0, "plain"),
    (255, 1, True, False, "sparse", 0.0, "plain"),
    (255, 4, True, True, "random", 0.0, "planar"),
    (256, 1, False, False, "uniform", 1000.0, "plain"),
    (256, 4, True, True, "sparse", 0.0, "mirrored"),
    (257, 1, True, False, "random", 0.0, "planar"),
    (257, 4, False, True, "uniform", 0.0, "mirrored"),
    (2056, 1, True, False, "random", 0.0, "plain"),
    (2056, 4, False, True, "sparse", 1000.0, "plain"),
    (2056, 4, True, True, "random", 0.0, "mirrored"),
]
KABSCH_IDS = [f"A{a}-B{b}-{'mask' if m else 'nomask'}-{'pergt' if p else 'sharedgt'}-{w}-off{int(o)}-{k}"
              for a, b, m, p, w, o, k in KABSCH_CASES]


def kabsch_case(A, B, masked, per_sample_gt, weights, offset, kind):
    """x_pred [B, A, 3]: noisy copies of an anisotropic cloud; the target: a rotated, shifted copy with 1 A of noise (per sample, or
    one for all), optionally flattened to z = 0 or mirrored in x before the common offset is added"""
    g = gen(3000 + A * 31 + B * 7 + len(weights) + len(kind) + int(offset))
    cloud = torch.randn(A, 3, generator=g, dtype=torch.float64)
    if A <= 5:                             # a handful of random points is too often nearly collinear: perturb a spread-out set
        cloud = 0.1 * cloud + torch.tensor([[1.0, 0.0, 0.3], [-0.6, 1.0, -0.4], [-0.5, -1.0, 0.2], [0.2, 0.1, 1.2],
                                            [0.4, -0.3, -1.1]], dtype=torch.float64)[:A]
    cloud = cloud * torch.tensor([12.0, 8.0, 5.0], dtype=torch.float64)
    x_pred = cloud[None] + 0.5 * torch.randn(B, A, 3, generator=g, dtype=torch.float64)
    n_gt = B if per_sample_gt else 1
    gts = []
    for b in range(n_gt):
        src = x_pred[b] if per_sample_gt else cloud
        t = src @ random_rotation(g).T + torch.randn(A, 3, generator=g, dtype=torch.float64) \
            + 4.0 * torch.randn(3, generator=g, dtype=torch.float64)
        if kind == "planar":
            t[:, 2] = 0.0
        elif kind == "mirrored":
            t[:, 0] = -t[:, 0]
        gts.append(t)
    x_gt = torch.stack(gts) if per_sample_gt else gts[0]
    if weights == "uniform":
        w = torch.ones(A)
    elif weights == "random":
        w = 0.25 + 0.75 * torch.rand(A, generator=g)
        if A >= 255:
            w[torch.randperm(A, generator=g)[: A // 20]] = 0.0
    else:                                   # the ligand-only pattern of model.py: 0 / 1, about 3 % set
        w = torch.zeros(A)
        w[torch.randperm(A, generator=g)[: max(4, round(0.03 * A))]] = 1.0
    mask = None
    if masked:
        mask = torch.ones(A)
        mask[torch.randperm(A, generator=g)[: round(0.1 * A)]] = 0.0
    return dict(x_pred=(x_pred + offset).float(), x_gt=(x_gt + offset).float(), w=w, mask=mask)


def kabsch_moved_target(c, seed=0):
    """the same case with its target moved by a rigid transform (rotation about the target's own centre + 5 A shift)"""
    g = gen(3500 + seed)
    G = c["x_gt"].double()
    ctr = G.mean(-2, keepdim=True)
    moved = (G - ctr) @ random_rotation(g).T + ctr + 5.0 * torch.randn(3, generator=g, dtype=torch.float64)
    return dict(c, x_gt=moved.float())


def kabsch_floor(c, ref64):
    """the ulp floor at the coordinate scale of a case, per sample [B]"""
    scale = torch.maximum(ref64.abs().flatten(1).amax(1), c["x_gt"].double().abs().max())
    return TOL_FLOOR_ULPS * _ulp32(scale)


def _kabsch_dev(L, c):
    B, A = c["x_pred"].shape[:2]
    out = sentinel(B, A, 3)
    stride = 3 * A if c["x_gt"].dim() == 3 else 0
    d = {k: dev(c[k]) for k in ("x_pred", "mask", "x_gt", "w")}           # kept alive until the kernel has run
    ok(L.pd_kabsch_align(P(d["x_pred"]), P(d["mask"]), P(d["x_gt"]), stride, P(d["w"]), P(out), B, A, S()), "pd_kabsch_align")
    return body(out).cpu()


def _kabsch32(c):
    xp = c["x_pred"] if c["mask"] is None else c["x_pred"] * c["mask"][None, :, None]
    return orc.weighted_rigid_align(xp, c["x_gt"], c["w"])


@pytest.mark.parametrize("case", KABSCH_CASES, ids=KABSCH_IDS)
def test_pd_kabsch_align(L, case):
    A, B = case[:2]
    tag = KABSCH_IDS[KABSCH_CASES.index(case)]
    c = kabsch_case(*case)
    if c["x_gt"].dim() == 3 and B > 1:
        assert not torch.equal(c["x_gt"][0], c["x_gt"][1])
    ref64, sv = sr.kabsch64(c["x_pred"], c["mask"], c["x_gt"], c["w"])
    assert (sr.kabsch_margin64(c["x_pred"], c["mask"], c["x_gt"], c["w"]) >= 0.05).all()
    out = _kabsch_dev(L, c)
    ref32 = _kabsch32(c)
    check_close("pd_kabsch_align", tag, out, ref32, ref64, per_sample=True)
    bound, _ = tolerance(ref32, ref64, per_sample=True)

    # invariants that do not go through the reference
    o64 = out.double()
    G = c["x_gt"].double()
    G = G if G.dim() == 3 else G[None].expand(B, -1, -1)
    floor = TOL_FLOOR_ULPS * _ulp32(torch.maximum(o64.abs().flatten(1).amax(1), G.abs().flatten(1).amax(1)))
    sub = slice(None) if A <= 512 else torch.randperm(A, generator=gen(1))[:512]
    d_out, d_gt = torch.cdist(o64[:, sub], o64[:, sub]), torch.cdist(G[:, sub], G[:, sub])
    assert ((d_out - d_gt).abs() <= floor[:, None, None]).all(), float((d_out - d_gt).abs().max())
    # the weighted centroid: that of ref64 is exactly the centroid of x_pred * mask, and a centroid moves by no more than the
    # largest element error, so the element bound of the sample is the bound of its centroid
    w = c["w"].double()
    Pm = c["x_pred"].double() * (1.0 if c["mask"] is None else c["mask"].double()[None, :, None])
    cen = lambda x: (x * w[None, :, None]).sum(-2) / w.sum()
    assert ((cen(o64) - cen(Pm)).abs() <= bound.reshape(B, 1)).all()
    # a rigid move of the target beforehand: same output.  The moved target is rounded to fp32 again, which moves the exact answer
    # by no more than the ulp floor (asserted on these inputs without a GPU: test_sampler_ref_cpu.py::
    # test_kabsch_moved_target_keeps_the_answer), so two device runs may differ by their two bounds plus that floor
    m = kabsch_moved_target(c)
    out_m = _kabsch_dev(L, m)
    ref64_m, _ = sr.kabsch64(m["x_pred"], m["mask"], m["x_gt"], m["w"])
    ref32_m = _kabsch32(m)
    check_close("pd_kabsch_align", tag + " moved", out_m, ref32_m, ref64_m, per_sample=True)
    bound_m, _ = tolerance(ref32_m, ref64_m, per_sample=True)
    assert ((out_m.double() - o64).abs() <= bound + bound_m + kabsch_floor(c, ref64).reshape(B, 1, 1)).all()


# ------------------------------------------------------------------ pd_augment, parity mode
def augment_case(B, A, seed=0):
    g = gen(4000 + seed + A * 3 + B)
    mask = torch.ones(A)
    if A > 1:
        mask[torch.randperm(A, generator=g)[: max(1, A // 8)]] = 0.0
    return dict(x=torch.randn(B, A, 3, generator=g) * 9 + 300.0, mask=mask,
                rot_u=(torch.rand(4, B, generator=g) * 0.9 + 0.05), trans=torch.randn(B, 3, generator=g),
                noise=torch.randn(B, A, 3, generator=g))


def _augment32(x, x_scale, mask, u, trans, noise, lam, sdev):
    y = orc.centre_random_augmentation(x * x_scale, mask, u, trans)
    return y if sdev == 0 else y + lam * noise * sdev


@pytest.mark.parametrize("A", [1, 255, 256, 257, 2056])
@pytest.mark.parametrize("B", [1, 5])
def test_pd_augment_parity(L, B, A):
    c = augment_case(B, A)
    d = {k: dev(v) for k, v in c.items()}
    if B > 1:
        assert not torch.equal(c["rot_u"], c["rot_u"].T.reshape(4, B))          # a [B][4] reading sees other values
    lam = LAM
    for x_scale, sdev in itertools.product((1.0, 160.0), (0.0, 2.5)):
        out = sentinel(B, A, 3)
        ok(L.pd_augment(P(d["x"]), x_scale, P(d["mask"]), P(d["rot_u"]), P(d["trans"]), P(d["noise"]) if sdev else None, lam, sdev,
                        None, 0, 0, P(out), B, A, S()), "pd_augment")
        ref64 = sr.augment64(c["x"], x_scale, c["mask"], c["rot_u"], c["trans"], c["noise"] if sdev else None, lam, sdev)
        ref32 = _augment32(c["x"], x_scale, c["mask"], c["rot_u"], c["trans"], c["noise"], lam, sdev)
        check_close("pd_augment", f"parity B={B} A={A} x_scale={x_scale:g} sdev={sdev:g}", body(out), ref32, ref64, per_sample=True)


# ------------------------------------------------------------------ seeded draws: pd_augment (Philox) and pd_init_noise
SEEDS = [7, 2 ** 32 + 7, 2 ** 63 + 12345]
POOL = dict(seed=7, B=64, A=2056)           # the pooled pd_init_noise draws of the moment check


def seed_buffer(seed):
    return torch.from_numpy(np.array([seed], dtype=np.uint64).view(np.int64)).cuda()


def _init_noise_dev(L, seed, sample0, sigma0, B, A):
    out = sentinel(B, A, 3)
    sd = seed_buffer(seed)
    ok(L.pd_init_noise(P(out), P(sd), sample0, sigma0, B, A, S()), "pd_init_noise")
    return body(out)


@pytest.mark.parametrize("A", [1, 257, 2056])
@pytest.mark.parametrize("B", [1, 4])
def test_pd_init_noise(L, B, A):
    sigma0 = 160.0 * 16.0
    outs = {}
    for seed, sample0 in itertools.product(SEEDS, (0, 5)):
        out = _init_noise_dev(L, seed, sample0, sigma0, B, A)
        ref64 = torch.from_numpy(sr.init_noise_draws(seed, sample0, sigma0, B, A))
        ref32 = torch.from_numpy(sr.init_noise_draws(seed, sample0, sigma0, B, A, np.float32))
        check_close("pd_init_noise", f"B={B} A={A} seed={seed:#x} sample0={sample0}", out, ref32, ref64)
        outs[(seed, sample0)] = out.clone()
    assert not torch.equal(outs[(7, 0)], outs[(2 ** 32 + 7, 0)])            # the high key word matters
    assert not torch.equal(outs[(7, 0)], outs[(7, 5)])


def test_pd_init_noise_shard_invariance(L):
    for seed in SEEDS:
        full = _init_noise_dev(L, seed, 0, 2560.0, 4, 257)
        parts = torch.cat([_init_noise_dev(L, seed, 0, 2560.0, 2, 257), _init_noise_dev(L, seed, 2, 2560.0, 2, 257)])
        assert torch.equal(full, parts)


def test_pd_init_noise_pool_moments(L):
    B, A = POOL["B"], POOL["A"]
    x = _init_noise_dev(L, POOL["seed"], 0, 1.0, B, A)
    ref64 = torch.from_numpy(sr.init_noise_draws(POOL["seed"], 0, 1.0, B, A))
    ref32 = torch.from_numpy(sr.init_noise_draws(POOL["seed"], 0, 1.0, B, A, np.float32))
    check_close("pd_init_noise", f"pool B={B} A={A}", x, ref32, ref64)
    mean, var, kurt = sr.moments(x.cpu().numpy())
    n = x.numel()
    print(f"pool moments: mean {mean:.3e} var {var:.5f} kurtosis {kurt:.4f} (n = {n})")
    assert abs(mean) <= 5 / math.sqrt(n) and abs(var - 1) <= 0.01 and abs(kurt - 3) <= 0.05, (mean, var, kurt)
    same = (x[:, None] == x[None]).all(-1)                   # [B, B, A]: atom rows shared by two samples
    same &= ~torch.eye(B, dtype=torch.bool, device="cuda")[:, :, None]
    assert not same.any()
    assert torch.unique(x.reshape(B, -1), dim=0).shape[0] == B


def seeded_augment_case(B, A):
    g = gen(5000 + A + B)
    mask = torch.ones(A)
    if A > 1:
        mask[torch.randperm(A, generator=g)[: max(1, A // 8)]] = 0.0
    return dict(x=torch.randn(B, A, 3, generator=g) * 9, mask=mask)


def _augment_seeded_dev(L, x, mask, seed, step, sample0, lam, sdev):
    B, A = x.shape[:2]
    out = sentinel(B, A, 3)
    sd = seed_buffer(seed)
    ok(L.pd_augment(P(x), 1.0, P(mask), None, None, None, lam, sdev, P(sd), step, sample0, P(out), B, A, S()),
       "pd_augment")
    return body(out)


@pytest.mark.parametrize("A", [1, 257, 2056])
@pytest.mark.parametrize("B", [1, 4])
def test_pd_augment_seeded(L, B, A):
    c = seeded_augment_case(B, A)
    x, mask = dev(c["x"]), dev(c["mask"])
    lam, sdev = LAM, 1.75
    outs = {}
    for seed, step, sample0 in itertools.product(SEEDS, (0, 1, 199), (0, 5)):
        out = _augment_seeded_dev(L, x, mask, seed, step, sample0, lam, sdev)
        u = torch.from_numpy(sr.augment_rot_uniforms(seed, step, sample0, B))
        t64, n64 = sr.augment_trans_draws(seed, step, sample0, B), sr.augment_noise_draws(seed, step, sample0, B, A)
        t32 = sr.augment_trans_draws(seed, step, sample0, B, np.float32)
        n32 = sr.augment_noise_draws(seed, step, sample0, B, A, np.float32)
        ref64 = sr.augment64(c["x"], 1.0, c["mask"], u, t64, n64, lam, sdev)
        ref32 = _augment32(c["x"], 1.0, c["mask"], u, torch.from_numpy(t32), torch.from_numpy(n32), lam, sdev)
        check_close("pd_augment", f"seeded B={B} A={A} seed={seed:#x} step={step} sample0={sample0}", out, ref32, ref64,
                    per_sample=True)
        outs[(seed, step, sample0)] = out.clone()
    for step, sample0 in itertools.product((0, 1, 199), (0, 5)):
        assert not torch.equal(outs[(7, step, sample0)], outs[(2 ** 32 + 7, step, sample0)])
    a, b = outs[(7, 0, 0)], outs[(7, 1, 0)]                              # only the step differs: every sample moves
    assert all(not torch.equal(a[i], b[i]) for i in range(B))


def test_pd_augment_seeded_shard_invariance(L):
    c = seeded_augment_case(4, 257)
    x, mask = dev(c["x"]), dev(c["mask"])
    for seed in SEEDS:
        full = _augment_seeded_dev(L, x, mask, seed, 3, 0, LAM, 1.75)
        parts = torch.cat([_augment_seeded_dev(L, x[:2].contiguous(), mask, seed, 3, 0, LAM, 1.75),
                           _augment_seeded_dev(L, x[2:].contiguous(), mask, seed, 3, 2, LAM, 1.75)])
        assert torch.equal(full, parts)


def test_pd_augment_seeded_rotation_is_proper(L):
    """sdev = 0 on a regular tetrahedron centred on the origin (sum_i v_i v_i^T = 4 I): R = 1/4 sum_i out_i v_i^T, t = mean out"""
    V = torch.tensor([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])
    B = 4
    x, mask = dev(V[None].repeat(B, 1, 1)), dev(torch.ones(4))
    for seed, step in itertools.product(SEEDS, (0, 1, 199)):
        out = _augment_seeded_dev(L, x, mask, seed, step, 0, LAM, 0.0).cpu().double()
        R = torch.einsum("bik,ij->bkj", out, V.double()) / 4
        floor = TOL_FLOOR_ULPS * _ulp32(out.abs().flatten(1).amax(1))
        assert ((R @ R.transpose(-1, -2) - torch.eye(3, dtype=torch.float64)).abs().flatten(1).amax(1) <= floor).all()
        assert ((torch.linalg.det(R) - 1).abs() <= floor).all()
        u = torch.from_numpy(sr.augment_rot_uniforms(seed, step, 0, B))
        assert ((R - sr.rotation64(u)).abs().flatten(1).amax(1) <= TOL_FACTOR * (orc.rotation_from_uniforms(u).double()
                - sr.rotation64(u)).abs().flatten(1).amax(1) + floor).all()


# ------------------------------------------------------------------ pd_euler
def euler_case(B, A, seed=0):
    g = gen(6000 + seed + A + B)
    x_hat = torch.randn(B, A, 3, generator=g) * 20
    w01 = (torch.rand(A, generator=g) < 0.3).float()
    return dict(x_hat=x_hat, x_den=x_hat + torch.randn(B, A, 3, generator=g), x_proj=x_hat + torch.randn(B, A, 3, generator=g),
                w01=w01, wfrac=torch.rand(A, generator=g))


def _euler32(x_hat, x_den, x_proj, w, t_hat, eta, dt):
    t, dt = torch.tensor(t_hat, dtype=torch.float32), torch.tensor(dt, dtype=torch.float32)
    if x_proj is None:
        d = (x_hat - x_den) / t
    else:
        wa = w[None, :, None]
        d = (x_hat - x_den) / t * (1 - wa) + (x_hat - x_proj) / t * wa
    return x_hat + eta * dt * d


@pytest.mark.parametrize("A", [1, 257])
@pytest.mark.parametrize("B", [1, 5])
def test_pd_euler(L, B, A):
    c = euler_case(B, A)
    d = {k: dev(v) for k, v in c.items()}
    for (t_hat, dt), eta, form in itertools.product(((160.0 * 16.0, -331.0), (6.4e-3, -6.4e-3)), (1.0, 1.5), ("plain", "w01", "wfrac")):
        out = sentinel(B, A, 3)
        proj, w = (None, None) if form == "plain" else (c["x_proj"], c[form])
        ok(L.pd_euler(P(d["x_hat"]), P(d["x_den"]), None if proj is None else P(d["x_proj"]), None if w is None else P(d[form]),
                      t_hat, eta, dt, P(out), B, A, S()), "pd_euler")
        t32, dt32 = float(np.float32(t_hat)), float(np.float32(dt))           # what the kernel is handed
        check_close("pd_euler", f"B={B} A={A} t_hat={t_hat:g} eta={eta} {form}", body(out),
                    _euler32(c["x_hat"], c["x_den"], proj, w, t_hat, eta, dt),
                    sr.euler64(c["x_hat"], c["x_den"], proj, w, t32, eta, dt32))


# ------------------------------------------------------------------ pd_timestep_embed
def timestep_case(n):
    ends = [0.25 * math.log(160.0 * 16.0 / 16.0), 0.25 * math.log(6.4e-3 / 16.0)]
    fixed = [ends[0], ends[1], 0.0, 50.0, -50.0]
    tau = fixed[:n] if n <= len(fixed) else fixed + torch.linspace(ends[1], ends[0], n - len(fixed)).tolist()
    return torch.tensor(tau, dtype=torch.float32)


def _timestep32(tau):
    freq = torch.exp(-math.log(10000.0) * torch.arange(128, dtype=torch.float32) / 128)
    arg = tau[:, None] * freq[None]
    return torch.cat([torch.cos(arg), torch.sin(arg)], dim=-1)


@pytest.mark.parametrize("n", [1, 40, 257])
def test_pd_timestep_embed(L, n):
    taus = [timestep_case(n)] + ([torch.tensor([50.0]), torch.tensor([-50.0]), torch.tensor([0.0])] if n == 1 else [])
    for tau in taus:
        out = sentinel(n, 256)
        tau_d = dev(tau)
        ok(L.pd_timestep_embed(P(tau_d), P(out), n, S()), "pd_timestep_embed")
        o = body(out)
        check_close("pd_timestep_embed", f"n={n} tau0={float(tau[0]):.3g}", o, _timestep32(tau), sr.timestep_embed64(tau))
        if float(tau[0]) == 0.0:
            assert torch.equal(o[0].cpu(), torch.cat([torch.ones(128), torch.zeros(128)]))        # layout [cos | sin]


# ------------------------------------------------------------------ pd_pose_dist / pd_template_match
def template_case(Lg, Cn, B, seed=0):
    """conformers [Cn, Lg, 3] (for Cn >= 3 the last is a copy of conformer Cn // 3: a tie), samples that are rigidly moved noisy
    copies of chosen conformers - sample 0 of the duplicated one - inside a larger atom array with a scattered, unsorted lig_idx"""
    g = gen(7000 + seed + Lg * 5 + Cn * 3 + B)
    poses = torch.randn(Cn, Lg, 3, generator=g) * 3
    if Cn >= 3:
        poses[Cn - 1] = poses[Cn // 3]
    target = [(Cn // 3 if b == 0 else (3 + 7 * b)) % Cn for b in range(B)]
    A = Lg + 37
    lig_idx = torch.randperm(A, generator=g)[:Lg].to(torch.int32)
    x = torch.randn(B, A, 3, generator=g) * 20
    for b in range(B):
        lig = poses[target[b]].double() @ random_rotation(g).T + 6.0 * torch.randn(3, generator=g, dtype=torch.float64)
        x[b, lig_idx.long()] = (lig + 0.05 * torch.randn(Lg, 3, generator=g, dtype=torch.float64)).float()
    return dict(poses=poses, x=x, lig_idx=lig_idx, target=target, A=A)


def template_expected(c, ref_dist):
    """per sample: the lowest index among the conformers whose distance matrix equals that of the sample's source conformer, and
    the smallest eps64 gap from it to any conformer outside that set (inf if there is none)"""
    lig = c["x"][:, c["lig_idx"].long()]
    sel, gap = [], []
    for b, t in enumerate(c["target"]):
        e = sr.template_eps64(lig[b:b + 1], ref_dist)[0]
        tied = [k for k in range(ref_dist.shape[0]) if torch.equal(ref_dist[k], ref_dist[t])]
        rest = [k for k in range(ref_dist.shape[0]) if k not in tied]
        sel.append(min(tied))
        gap.append(float((e[rest] - e[tied].max()).min()) if rest else float("inf"))
    return torch.tensor(sel), gap


@pytest.mark.parametrize("Lg", [1, 7, 64, 200])
@pytest.mark.parametrize("Cn", [1, 3, 40])
@pytest.mark.parametrize("B", [1, 5])
def test_pd_pose_dist_and_template_match(L, B, Cn, Lg):
    c = template_case(Lg, Cn, B)
    A = c["A"]
    x, lig_idx, poses = dev(c["x"]), dev(c["lig_idx"]), dev(c["poses"])
    tag = f"B={B} Cn={Cn} L={Lg}"

    rd_buf = sentinel(Cn, Lg, Lg)
    ok(L.pd_pose_dist(P(poses), P(rd_buf), Cn, Lg, S()), "pd_pose_dist")
    rd = body(rd_buf).contiguous()
    p64 = sr.pose_dist64(c["poses"])
    p32 = torch.norm(c["poses"][:, :, None] - c["poses"][:, None], dim=-1)
    check_close("pd_pose_dist", f"Cn={Cn} L={Lg}", rd, p32, p64)
    assert torch.equal(rd, rd.transpose(1, 2)) and (torch.diagonal(rd, dim1=1, dim2=2) == 0).all()

    rd_cpu = rd.cpu()
    lig = c["x"][:, c["lig_idx"].long()]
    e64 = torch.cat([sr.template_eps64(lig[b:b + 1], rd_cpu) for b in range(B)])
    e32 = torch.cat([orc.template_epsilon(lig[b:b + 1], rd_cpu) for b in range(B)])
    want_sel, _ = template_expected(c, rd_cpu.double())
    want_ref = torch.full((B, A, 3), NAN)
    want_ref[:, c["lig_idx"].long()] = c["poses"][want_sel]

    def run(two_pass, with_sel=True, with_ref=True):
        eps = sentinel(B, Cn) if two_pass else None
        sel = sentinel(B, dtype=torch.int32) if with_sel else None
        ref = sentinel(B, A, 3) if with_ref else None
        ok(L.pd_template_match(P(x), P(lig_idx), P(rd), P(poses) if with_ref else None, P(ref) if with_ref else None,
                               P(eps) if two_pass else None, P(sel) if with_sel else None, B, A, Lg, Cn, S()), "pd_template_match")
        return (None if eps is None else body(eps).cpu(), None if sel is None else body(sel).cpu().long(),
                None if ref is None else body(ref, written=False).cpu())

    eps2, sel2, ref2 = run(True)
    _, sel1, ref1 = run(False)
    check_close("pd_template_match", tag, eps2, e32, e64, per_sample=True)
    assert torch.equal(sel1, want_sel) and torch.equal(sel2, want_sel), (sel1, sel2, want_sel)
    for ref in (ref1, ref2):                      # the chosen pose at the ligand atoms, the sentinel everywhere else
        assert torch.equal(torch.isnan(ref), torch.isnan(want_ref))
        assert torch.equal(torch.nan_to_num(ref, nan=0.0), torch.nan_to_num(want_ref, nan=0.0))
    # optional outputs left out
    for two_pass in (True, False):
        _, _, ref_ns = run(two_pass, with_sel=False)
        assert torch.equal(torch.nan_to_num(ref_ns, nan=0.0), torch.nan_to_num(want_ref, nan=0.0))
        e_only, s_only, _ = run(two_pass, with_ref=False)
        assert torch.equal(s_only, want_sel)
        if two_pass:
            assert torch.equal(e_only, eps2)
    e_alone, _, _ = run(True, with_sel=False, with_ref=False)
    assert torch.equal(e_alone, eps2)


# ------------------------------------------------------------------ pd_pairwise_rmsd
def rmsd_case(n, Lg, scattered, seed=0):
    g = gen(8000 + seed + n * 11 + Lg + scattered)
    A = Lg + 29 if scattered else Lg
    x = torch.randn(n, A, 3, generator=g) * 5 + torch.randn(n, 1, 3, generator=g) * 2
    idx = torch.randperm(A, generator=g)[:Lg].to(torch.int32) if scattered else None
    return dict(x=x, idx=idx, ref=torch.randn(A, 3, generator=g) * 5, A=A)


def _rmsd32(x, idx, ref):
    xs = x if idx is None else x[:, idx.long()]
    D = torch.sqrt(((xs[:, None] - xs[None]) ** 2).sum(-1).mean(-1))
    if ref is None:
        return D, None
    rs = ref if idx is None else ref[idx.long()]
    return D, torch.sqrt(((xs - rs[None]) ** 2).sum(-1).mean(-1))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("Lg", [1, 63, 64, 65, 300])
def test_pd_pairwise_rmsd(L, Lg, n):
    for scattered, with_ref in itertools.product((False, True), (False, True)):
        c = rmsd_case(n, Lg, scattered)
        D, r = sentinel(n, n), sentinel(n)
        d = {k: dev(c[k]) for k in ("x", "idx", "ref")}
        ok(L.pd_pairwise_rmsd(P(d["x"]), P(d["idx"]), P(d["ref"]) if with_ref else None, P(D), P(r), n, c["A"], Lg, S()),
           "pd_pairwise_rmsd")
        D64, r64 = sr.pairwise_rmsd64(c["x"], c["idx"], c["ref"] if with_ref else None)
        D32, r32 = _rmsd32(c["x"], c["idx"], c["ref"] if with_ref else None)
        tag = f"n={n} L={Lg} {'scattered' if scattered else 'all'}"
        Dd = body(D)
        check_close("pd_pairwise_rmsd", tag + " D", Dd, D32, D64)
        assert torch.equal(Dd, Dd.T) and (torch.diagonal(Dd) == 0).all()
        if with_ref:
            check_close("pd_pairwise_rmsd", tag + " ref", body(r), r32, r64)
        else:
            assert is_sentinel(body(r, written=False)).all()


# ------------------------------------------------------------------ pd_ligand_gather / pd_ligand_scatter
@pytest.mark.parametrize("B,A,Lg", [(1, 1, 1), (3, 50, 1), (3, 50, 17), (2, 300, 300), (5, 257, 100)])
def test_pd_ligand_gather_scatter(L, B, A, Lg):
    g = gen(9000 + A + Lg)
    idx = torch.randperm(A, generator=g)[:Lg]
    slot = torch.full((A,), -1, dtype=torch.int32)
    slot[idx] = torch.arange(Lg, dtype=torch.int32)
    x, src = torch.randn(B, A, 3, generator=g), torch.randn(B, A, 3, generator=g)
    relaxed = torch.randn(B, Lg, 3, generator=g)
    idx_d, slot_d, x_d, src_d, relaxed_d = dev(idx.to(torch.int32)), dev(slot), dev(x), dev(src), dev(relaxed)

    lig = sentinel(B, Lg, 3)
    ok(L.pd_ligand_gather(P(x_d), P(idx_d), P(lig), B, A, Lg, S()), "pd_ligand_gather")
    assert torch.equal(body(lig).cpu(), x[:, idx])

    dst = sentinel(B, A, 3)
    ok(L.pd_ligand_scatter(P(dst), P(src_d), P(relaxed_d), P(slot_d), B, A, Lg, S()), "pd_ligand_scatter")
    want = src.clone()
    want[:, idx] = relaxed
    got = body(dst)
    assert torch.equal(got.cpu(), want)
    rest = torch.ones(A, dtype=torch.bool)
    rest[idx] = False
    assert torch.equal(got.cpu()[:, rest], src[:, rest])

    back = sentinel(B, Lg, 3)
    got_c = got.contiguous()
    ok(L.pd_ligand_gather(P(got_c), P(idx_d), P(back), B, A, Lg, S()), "pd_ligand_gather")
    assert torch.equal(body(back).cpu(), relaxed)


# ------------------------------------------------------------------ argument checks (all return before a launch)
def test_argument_checks(L):
    f = torch.zeros(64, device="cuda")
    i = torch.zeros(16, dtype=torch.int32, device="cuda")
    sd = seed_buffer(1)
    p, q, s = P(f), P(i), S()
    bad = {
        "augment null x": L.pd_augment(None, 1.0, p, p, p, None, 1.0, 0.0, None, 0, 0, p, 1, 1, s),
        "augment null mask": L.pd_augment(p, 1.0, None, p, p, None, 1.0, 0.0, None, 0, 0, p, 1, 1, s),
        "augment null out": L.pd_augment(p, 1.0, p, p, p, None, 1.0, 0.0, None, 0, 0, None, 1, 1, s),
        "augment no draws": L.pd_augment(p, 1.0, p, None, None, None, 1.0, 0.0, None, 0, 0, p, 1, 1, s),
        "augment rot_u without trans": L.pd_augment(p, 1.0, p, p, None, None, 1.0, 0.0, None, 0, 0, p, 1, 1, s),
        "augment sdev without noise": L.pd_augment(p, 1.0, p, p, p, None, 1.0, 1.0, None, 0, 0, p, 1, 1, s),
        "augment B=0": L.pd_augment(p, 1.0, p, p, p, None, 1.0, 0.0, None, 0, 0, p, 0, 1, s),
        "init_noise null x": L.pd_init_noise(None, P(sd), 0, 1.0, 1, 1, s),
        "init_noise null seed": L.pd_init_noise(p, None, 0, 1.0, 1, 1, s),
        "init_noise B=0": L.pd_init_noise(p, P(sd), 0, 1.0, 0, 1, s),
        "init_noise A=-1": L.pd_init_noise(p, P(sd), 0, 1.0, 1, -1, s),
        "precond null Wx": L.pd_precond(p, 1.0, None, None, p, p, p, 1, 1, 4, s),
        "precond C%4": L.pd_precond(p, 1.0, None, p, p, p, p, 1, 1, 6, s),
        "precond_g G=0": L.pd_precond_g(p, 1.0, None, p, p, p, p, 0, 1, 1, 4, s),
        "precond_g B=0": L.pd_precond_g(p, 1.0, None, p, p, p, p, 1, 0, 1, 4, s),
        "denoise null Wr": L.pd_denoise(p, p, p, p, None, 1e-5, 1.0, 1.0, None, None, p, 1, 1, 4, s),
        "denoise C%4": L.pd_denoise(p, p, p, p, p, 1e-5, 1.0, 1.0, None, None, p, 1, 1, 6, s),
        "denoise C>512": L.pd_denoise(p, p, p, p, p, 1e-5, 1.0, 1.0, None, None, p, 1, 1, 516, s),
        "denoise B=0": L.pd_denoise(p, p, p, p, p, 1e-5, 1.0, 1.0, None, None, p, 0, 1, 4, s),
        "denoise A=0": L.pd_denoise(p, p, p, p, p, 1e-5, 1.0, 1.0, None, None, p, 1, 0, 4, s),
        "kabsch null w": L.pd_kabsch_align(p, None, p, 0, None, p, 1, 3, s),
        "kabsch B=0": L.pd_kabsch_align(p, None, p, 0, p, p, 0, 3, s),
        "kabsch A=0": L.pd_kabsch_align(p, None, p, 0, p, p, 1, 0, s),
        "template null lig_idx": L.pd_template_match(p, None, p, None, None, p, q, 1, 1, 1, 1, s),
        "template ref_pos without poses": L.pd_template_match(p, q, p, None, p, p, q, 1, 1, 1, 1, s),
        "template Cn=0": L.pd_template_match(p, q, p, None, None, p, q, 1, 1, 1, 0, s),
        "pose_dist null D": L.pd_pose_dist(p, None, 1, 1, s),
        "pose_dist Cn=0": L.pd_pose_dist(p, p, 0, 1, s),
        "pose_dist L=0": L.pd_pose_dist(p, p, 1, 0, s),
        "rmsd null D": L.pd_pairwise_rmsd(p, None, None, None, None, 1, 1, 1, s),
        "rmsd ref without rmsd_ref": L.pd_pairwise_rmsd(p, None, p, p, None, 1, 1, 1, s),
        "rmsd n=0": L.pd_pairwise_rmsd(p, None, None, p, None, 0, 1, 1, s),
        "euler null x_den": L.pd_euler(p, None, None, None, 1.0, 1.0, -0.1, p, 1, 1, s),
        "euler x_proj without w": L.pd_euler(p, p, p, None, 1.0, 1.0, -0.1, p, 1, 1, s),
        "euler B=0": L.pd_euler(p, p, None, None, 1.0, 1.0, -0.1, p, 0, 1, s),
        "euler A=0": L.pd_euler(p, p, None, None, 1.0, 1.0, -0.1, p, 1, 0, s),
        "timestep null emb": L.pd_timestep_embed(p, None, 1, s),
        "timestep n=0": L.pd_timestep_embed(p, p, 0, s),
        "gather L=0": L.pd_ligand_gather(p, q, p, 1, 1, 0, s),
        "scatter null slot": L.pd_ligand_scatter(p, p, p, None, 1, 1, 1, s),
    }
    wrong = {k: v for k, v in bad.items() if v != PD_ERR_ARG}
    assert not wrong, wrong
    torch.cuda.synchronize()
    assert (f == 0).all() and (i == 0).all()
    # a valid call right after still succeeds
    out = sentinel(2, 5, 3)
    xh, xd = torch.ones(2, 5, 3, device="cuda"), torch.zeros(2, 5, 3, device="cuda")
    ok(L.pd_euler(P(xh), P(xd), None, None, 2.0, 1.0, -1.0, P(out), 2, 5, S()), "pd_euler")
    assert torch.equal(body(out), torch.full((2, 5, 3), 0.5, device="cuda"))
