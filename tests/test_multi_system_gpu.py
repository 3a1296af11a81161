"""Several systems in one sampler call (PhysDock.sample_diffusion_many): grouped attention and the grouped per-system
denoiser kernels against per-group launches, one system against sample_diffusion, several against the CPU oracle, group
addressing, and driver.redock_many(group=).  GPU only."""
import ctypes as C_
import os
import sys

import pytest
import torch

from conftest import rmsd

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))


def to_dev(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


@pytest.fixture(scope="module")
def small(small_model_inputs):
    from physdock_amd import PhysDock
    cfg, P, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P, strict=True)
    return model.cuda().eval(), cfg, P


# ------------------------------------------------------------------ grouped attention
def _attn_case(H, N, reals, B, seed):
    from physdock_amd import ops
    g = torch.Generator().manual_seed(seed)
    C = H * 32
    qkv = (torch.randn(len(reals) * B, N, 3 * C, generator=g) * 0.5).cuda()
    dense = []
    for r in reals:
        d = torch.randn(H, N, N, generator=g)
        d[:, :, r:] = -1e9                           # masked keys, as the producers write them
        dense.append(d)
    frags = torch.stack([ops.bias_to_frag(d).reshape(-1) for d in dense]).cuda().contiguous()
    return qkv, frags, dense, C


def _launch(qkv, bias, nk, nbatch, H, N, C, ps, ws, amax, **gkw):
    from physdock_amd import ops
    from physdock_amd._lib import lib
    o = torch.empty(nbatch, N, C, device="cuda")
    st = (N * 3 * C, 3 * C)
    seen = []
    ops.ATTN_HOOK = lambda a, launch: (seen.append((lib().pd_attention_variant(C_.byref(a)), a.group_samples)), launch())
    try:
        ops.attention(qkv.data_ptr(), qkv.data_ptr() + 4 * C, qkv.data_ptr() + 8 * C, o, nq=N, nk=nk, nbatch=nbatch, nheads=H,
                      q_strides=st, k_strides=st, v_strides=st, o_strides=(N * C, C), bias=bias, bias_nk=N, ws=ws,
                      f16_amax=amax, bias_prescale=ps, **gkw)
    finally:
        ops.ATTN_HOOK = None
    return o, seen[-1][0]


_ATOM, _TOKEN = (4, 2048, (1803, 2048, 1920)), (16, 256, (227, 256, 240))


@pytest.mark.parametrize("mode,H,N,reals", [(m, *_ATOM) for m in ("pipe", "parts", "keysplit", "bf16", "fp32")] +
                         [(m, *_TOKEN) for m in ("pipe", "parts", "bf16", "fp32")])      # (256 keys are never key-split)
def test_grouped_attention_matches_per_group_launches(mode, H, N, reals):
    """one grouped launch (three bias sets, three real key counts) against three launches of one system each, on every kernel family"""
    from physdock_amd import ops
    B = 1 if mode in ("parts", "keysplit") else 20
    G = len(reals)
    qkv, bias, dense, C = _attn_case(H, N, reals, B, seed=H + N)
    nfr = bias.shape[1]
    amax, ps, ws = None, 0.0, None
    saved = (ops.F16_ATTN, ops.SPLIT_ATTN)
    try:
        if mode in ("pipe", "parts", "keysplit"):
            amax = tuple(float(qkv[..., k * C:(k + 1) * C].abs().max()) * 1.01 for k in range(3))
            if mode == "pipe":
                ps = ops.attn_bias_prescale(amax[0], amax[1])
                bias = bias * ps
            if mode == "keysplit":
                ws = torch.empty(ops.attn_split_ws_numel(G * B, N, N, H), device="cuda")
        elif mode == "bf16":
            ops.F16_ATTN = False
        else:
            ops.SPLIT_ATTN = False
        nkg = torch.tensor(reals, dtype=torch.int32, device="cuda")
        og, vg = _launch(qkv, bias, max(reals), G * B, H, N, C, ps, ws, amax, group_samples=B, bias_gstride=nfr, nk_group=nkg)
        lo, hi = {"pipe": (3000, 4000), "parts": (2000, 2100), "keysplit": (2100, 3000), "bf16": (1000, 2000), "fp32": (0, 1000)}[mode]
        assert lo <= vg < hi, (mode, vg)
        ws1 = ws
        if mode == "keysplit":
            # the chunk count of a key-split launch follows its block count and key range; the one-system launches are held to the
            # grouped launch's count through the size of their scratch (pd_attention lowers the count to what the scratch holds)
            ns = (vg % 1000) // 100
            assert ns >= 2, vg
            ws1 = torch.empty(ns * B * N * H * 34, device="cuda")
        for g, r in enumerate(reals):
            o1, v1 = _launch(qkv[g * B:(g + 1) * B], bias[g], r, B, H, N, C, ps, ws1, amax)
            if mode == "keysplit":
                assert v1 == vg, (g, vg, v1)
            assert torch.equal(og[g * B:(g + 1) * B], o1), (mode, g, vg, v1)
        if mode == "bf16":                            # one float64 check of the grouped result
            for g, r in enumerate(reals):
                sl = qkv[g * B:(g + 1) * B].double().cpu().reshape(B, N, 3, H, 32)
                q, k, v = (sl[:, :, j].transpose(1, 2) for j in range(3))
                sc = q @ k.transpose(-1, -2) / 32 ** 0.5 + dense[g].double()[None]
                sc[..., r:] = -float("inf")
                ref = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B, N, C)
                err = float((og[g * B:(g + 1) * B].double().cpu() - ref).abs().max())
                assert err < 1e-5 * max(1.0, float(ref.abs().max())), (g, err)
    finally:
        ops.F16_ATTN, ops.SPLIT_ATTN = saved


# ------------------------------------------------------------------ grouped per-system denoiser kernels
def test_grouped_pool_unpool_precond_match_per_group_launches():
    from physdock_amd import ops
    from physdock_amd._lib import init
    L = init()
    sp = ops.stream()
    g = torch.Generator().manual_seed(7)
    G, B, A, T, Ca, Cs = 3, 4, 192, 40, 128, 256
    # ragged token tables, padded atoms (no token) and padded tokens (no atoms); system 1 has a token of 12 atoms (other tpb)
    tabs, a2ts = [], []
    for gi, (nreal_t, maxc) in enumerate([(37, 5), (40, 12), (33, 4)]):
        sizes = torch.randint(1, maxc + 1, (nreal_t,), generator=g)
        while int(sizes.sum()) > A - 8:
            sizes = torch.clamp(sizes - 1, min=1)
        ts = torch.zeros(T + 1, dtype=torch.int32)
        ts[1:nreal_t + 1] = torch.cumsum(sizes, 0).to(torch.int32)
        ts[nreal_t + 1:] = ts[nreal_t]
        a2t = torch.zeros(A, dtype=torch.int64)
        for t in range(nreal_t):
            a2t[int(ts[t]):int(ts[t + 1])] = t
        tabs.append(ts)
        a2ts.append(a2t)
    tok = torch.stack(tabs).cuda().contiguous()
    a2t = torch.stack(a2ts).cuda().contiguous()
    u = torch.randn(G * B, A, Cs, generator=g).cuda()
    add = torch.randn(G, T, Cs, generator=g).cuda()
    out_g = torch.empty(G * B, T, Cs, device="cuda")
    ops.check(L.pd_segment_pool_g(ops.ptr(u), ops.ptr(tok), ops.ptr(add), ops.ptr(out_g), G, B, A, T, Cs, sp), "pool_g")
    for gi in range(G):
        o1 = torch.empty(B, T, Cs, device="cuda")
        ops.check(L.pd_segment_pool(ops.ptr(u[gi * B:(gi + 1) * B]), ops.ptr(tok[gi]), ops.ptr(add[gi]), ops.ptr(o1), B, A, T, Cs, sp), "pool")
        assert torch.equal(out_g[gi * B:(gi + 1) * B], o1)
    # G = 1 is the existing entry point
    o1 = torch.empty(B, T, Cs, device="cuda")
    o2 = torch.empty(B, T, Cs, device="cuda")
    ops.check(L.pd_segment_pool_g(ops.ptr(u), ops.ptr(tok), ops.ptr(add), ops.ptr(o1), 1, B, A, T, Cs, sp), "pool_g")
    ops.check(L.pd_segment_pool(ops.ptr(u), ops.ptr(tok), ops.ptr(add), ops.ptr(o2), B, A, T, Cs, sp), "pool")
    assert torch.equal(o1, o2)
    # unpool
    ba = torch.randn(G * B, A, Ca, generator=g).cuda()
    us = torch.randn(G * B, T, Ca, generator=g).cuda()
    bg = ba.clone()
    ops.check(L.pd_unpool_add_g(ops.ptr(bg), ops.ptr(us), ops.ptr(a2t), G, B, A, T, Ca, sp), "unpool_g")
    for gi in range(G):
        b1 = ba[gi * B:(gi + 1) * B].clone()
        ops.check(L.pd_unpool_add(ops.ptr(b1), ops.ptr(us[gi * B:(gi + 1) * B]), ops.ptr(a2t[gi]), B, A, T, Ca, sp), "unpool")
        assert torch.equal(bg[gi * B:(gi + 1) * B], b1)
        # and the pair of launches against something outside themselves: the same fp32 add on the CPU
        assert torch.equal(b1.cpu(), ba[gi * B:(gi + 1) * B].cpu() + us[gi * B:(gi + 1) * B].cpu()[:, a2t[gi].cpu()])
    # precond
    x = torch.randn(G * B, A, 3, generator=g).cuda()
    Wx, bx = torch.randn(Ca, 3, generator=g).cuda(), torch.randn(Ca, generator=g).cuda()
    a = torch.randn(G, A, Ca, generator=g).cuda()
    pg = torch.empty(G * B, A, Ca, device="cuda")
    ops.check(L.pd_precond_g(ops.ptr(x), 0.37, None, ops.ptr(Wx), ops.ptr(bx), ops.ptr(a), ops.ptr(pg), G, B, A, Ca, sp), "precond_g")
    for gi in range(G):
        p1 = torch.empty(B, A, Ca, device="cuda")
        ops.check(L.pd_precond(ops.ptr(x[gi * B:(gi + 1) * B]), 0.37, None, ops.ptr(Wx), ops.ptr(bx), ops.ptr(a[gi]), ops.ptr(p1),
                               B, A, Ca, sp), "precond")
        assert torch.equal(pg[gi * B:(gi + 1) * B], p1)
    # fused downscale + pool: per-group launches, and the minimum tpb over the group
    from physdock_amd.packing import split2_f16
    Wd, bd = (torch.randn(Cs, Ca, generator=g) / Ca ** 0.5).cuda(), torch.randn(Cs, generator=g).cuda()
    w2p, w2i = split2_f16(Wd)
    tpb = min(min(32, 64 // int((t[1:] - t[:-1]).max())) for t in tabs)
    fg = torch.empty(G * B, T, Cs, device="cuda")
    rc = L.pd_downscale_pool_g(ops.ptr(ba), w2p.data_ptr(), ops.ptr(w2i), ops.ptr(bd), ops.ptr(tok), ops.ptr(add), ops.ptr(fg),
                               G, B, A, T, Ca, Cs, tpb, sp)
    ops.check(rc, "downscale_pool_g")
    for gi in range(G):
        f1 = torch.empty(B, T, Cs, device="cuda")
        ops.check(L.pd_downscale_pool(ops.ptr(ba[gi * B:(gi + 1) * B]), w2p.data_ptr(), ops.ptr(w2i), ops.ptr(bd), ops.ptr(tok[gi]),
                                      ops.ptr(add[gi]), ops.ptr(f1), B, A, T, Ca, Cs, tpb, sp), "downscale_pool")
        assert torch.equal(fg[gi * B:(gi + 1) * B], f1)


# ------------------------------------------------------------------ the sampler
def _noise(B, steps, A, seed):
    import physdock_oracle as orc
    g = torch.Generator().manual_seed(seed)
    n_noisy = int((orc.karras_noise_schedule(steps, p=1000)[:-1] > 1.0).sum())
    return {"init": torch.randn(B, A, 3, generator=g), "rot_u": torch.rand(steps, 4, B, generator=g),
            "trans": torch.randn(steps, B, 3, generator=g), "diffuse": torch.randn(n_noisy, B, A, 3, generator=g)}


@pytest.mark.parametrize("mode", ["seeded", "noise", "templates", "mmff"])
def test_one_system_equals_sample_diffusion(small, mode):
    """templates / mmff: sigma = 2560, 310, 37.4, 4.50, 0.54, 0.064 against a threshold factor 6.0 gives 3 align steps and 3
    plain (templates) or device-relaxation (mmff) steps: the shared tail runs all three branches from both entry points"""
    from physdock_amd import mmff
    from physdock_amd.synthetic import reference_conformers, small_batch
    model, cfg, P = small
    raw = small_batch(0)
    b = to_dev(raw)
    A = b["ref_pos"].shape[0]
    kw = dict(num_sample=3, steps=6, karras_noise_schedule_power=1000)
    if mode in ("templates", "mmff"):
        kw.update(align_ref_pos=True, mmff_gamma_0_factor=6.0)
        pool = reference_conformers(raw, n_conf=4)
        lig = raw["is_ligand"][raw["atom_id_to_token_id"]].bool()
        mol = mmff.synthetic_terms(int(lig.sum()), 5, coords=raw["x_gt"][lig].double().numpy())[0] if mode == "mmff" else None
        ref = model.sample_diffusion(b, seed=5, sample_offset=2, ref_mol_poses=pool, ref_mol=mol, **kw)
        for _ in range(2):
            (x,) = model.sample_diffusion_many([b], seeds=[5], sample_offsets=[2], ref_mol_poses=[pool], ref_mol=[mol], **kw)
            assert torch.equal(x, ref)
    elif mode == "noise":
        nz = _noise(3, 6, A, 11)
        ref = model.sample_diffusion(b, noise=nz, **kw)
        for _ in range(2):                               # first call (eager + capture), then the replay
            (x,) = model.sample_diffusion_many([b], noises=[nz], **kw)
            assert torch.equal(x, ref)
    else:
        ref = model.sample_diffusion(b, seed=5, sample_offset=2, **kw)
        for _ in range(2):
            (x,) = model.sample_diffusion_many([b], seeds=[5], sample_offsets=[2], **kw)
            assert torch.equal(x, ref)


@pytest.mark.parametrize("templates", [False, True])
def test_three_systems_vs_oracle(small, templates):
    import physdock_oracle as orc
    from physdock_amd.synthetic import make_batch, reference_conformers
    model, cfg, P = small
    sizes = [(18, 5, 6), (14, 5, 4), (16, 5, 8)]
    bs = [make_batch(n, apr, nl, 8, seed=20 + i) for i, (n, apr, nl) in enumerate(sizes)]
    B, steps = 2, 6
    nzs = [_noise(B, steps, b["ref_pos"].shape[0], 30 + i) for i, b in enumerate(bs)]
    kw = dict(num_sample=B, steps=steps, align_ref_pos=True, karras_noise_schedule_power=1000)
    poses = [reference_conformers(b, n_conf=4, seed=40 + i) for i, b in enumerate(bs)] if templates else None
    mf = 100.0 if templates else 1.0
    xs = model.sample_diffusion_many([to_dev(b) for b in bs], noises=nzs, ref_mol_poses=poses, mmff_gamma_0_factor=mf, **kw)
    for i, b in enumerate(bs):
        ref = orc.sample_diffusion(P, b, nzs[i], ref_mol_poses=poses[i] if templates else None, mmff_gamma_0_factor=mf, **kw)
        assert xs[i].shape == ref.shape
        d = rmsd(xs[i].cpu(), ref)
        print(f"system {i}: {d:.2e} A")
        assert d < 1e-3, (i, d)


@pytest.fixture(scope="module")
def medium():
    from physdock_amd import PhysDock, PhysDockConfig, param_shapes, seeded_state_dict
    cfg = PhysDockConfig(model_name="medium")
    model = PhysDock(cfg)
    model.load_state_dict(seeded_state_dict(param_shapes(cfg), seed=0), strict=True)
    return model.cuda().eval()


def _count_calls(monkeypatch, name):
    """count the library's calls of one entry point (and their return codes)"""
    from physdock_amd import ops
    L = ops._lib.init()
    fn = getattr(L, name)
    rcs = []

    def wrapped(*a):
        rc = fn(*a)
        rcs.append(rc)
        return rc
    monkeypatch.setattr(L, name, wrapped)
    return rcs


def test_reference_fixtures_at_medium_size(medium, monkeypatch):
    """the medium-model denoiser through the grouped launches (fused downscale + pool for the group, grouped atom / token attention)
    against the reference's own trajectories: g9_medium_ragged (A = 1803 -> 1856 padded -> 2048 in the group) together with sample 0
    of g9_medium_cfg1_b16 (A = 2048); samples of a reference call are independent"""
    from conftest import golden_noise, load_golden
    from physdock_amd.synthetic import cfg1_batch, make_batch
    gr, gc = load_golden("g9_medium_ragged"), load_golden("g9_medium_cfg1_b16")
    assert gr["steps"] == gc["steps"]
    nr, nc = golden_noise(gr), golden_noise(gc)
    nc = {"init": nc["init"][:1], "rot_u": nc["rot_u"][:, :, :1], "trans": nc["trans"][:, :1], "diffuse": nc["diffuse"][:, :1]}
    pool = _count_calls(monkeypatch, "pd_downscale_pool_g")
    xs = medium.sample_diffusion_many([to_dev(make_batch(221, 8, 35, 64, 2)), to_dev(cfg1_batch(0))], num_sample=1, steps=gr["steps"],
                                      karras_noise_schedule_power=1000, align_ref_pos=False, noises=[nr, nc])
    assert pool and all(rc == 0 for rc in pool), pool          # the fused grouped pool ran (no fall-back to projection + pool)
    dr, dc = rmsd(xs[0].cpu(), gr["x_pred"]), rmsd(xs[1].cpu(), gc["x_pred"][:1])
    print(f"grouped vs reference: ragged {dr:.3e} A, cfg1 sample 0 {dc:.3e} A")
    assert xs[0].shape == gr["x_pred"].shape and xs[1].shape == gc["x_pred"][:1].shape
    assert dr < 1e-3 and dc < 1e-3, (dr, dc)


def test_group_addressing_at_the_benchmark_dispatch(medium):
    """three medium systems of different real sizes, 20 samples each, 40 steps, seeded, template projection, one of them relaxed by a
    device MMFF table: the atom and token attention run the pipelined kernel with one bias set per 20 samples; each system's poses are
    bit-identical under a permutation of the group and when a neighbour is replaced by another system of the same padded shape"""
    from physdock_amd import mmff, ops
    from physdock_amd._lib import lib
    from physdock_amd.synthetic import cfg1_batch, make_batch, reference_conformers
    raw = [cfg1_batch(0), make_batch(221, 8, 35, 64, 2), make_batch(210, 9, 30, 128, 3)]
    bs = [to_dev(b) for b in raw]
    poses = [reference_conformers(b, n_conf=8, seed=11 + i) for i, b in enumerate(raw)]
    lig = raw[1]["is_ligand"][raw[1]["atom_id_to_token_id"]].bool()
    terms, _ = mmff.synthetic_terms(int(lig.sum()), 5, coords=raw[1]["x_gt"][lig].double().numpy())
    facs, mols, seeds = [6.0, 6.0, 3.0], [None, terms, None], [1, 2, 3]
    kw = dict(num_sample=20, steps=40, karras_noise_schedule_power=1000, align_ref_pos=True)

    def run(order, systems=None, mol=None):
        systems = systems or bs
        mol = mol or mols
        return medium.sample_diffusion_many([systems[i] for i in order], seeds=[seeds[i] for i in order],
                                            ref_mol_poses=[poses[i] for i in order], ref_mol=[mol[i] for i in order],
                                            mmff_gamma_0_factor=[facs[i] for i in order], **kw)
    seen = []
    ops.ATTN_HOOK = lambda a, launch: (seen.append((lib().pd_attention_variant(C_.byref(a)), a.group_samples, a.nbatch, a.nq)), launch())
    try:
        x = run([0, 1, 2])
    finally:
        ops.ATTN_HOOK = None
    dit = [(v, gs, nq) for v, gs, nb, nq in seen if nb == 60]
    for nq in (2048, 256):                                     # atom and token attention of the denoiser
        fam = [(v, gs) for v, gs, q in dit if q == nq]
        assert fam and all(v >= 3000 and gs == 20 for v, gs in fam), (nq, sorted(set(fam)))
    x2 = run([0, 1, 2])                                        # replayed units
    for i in range(3):
        assert torch.equal(x2[i], x[i]), i
    perm = [2, 0, 1]
    xp = run(perm)
    for j, i in enumerate(perm):
        assert torch.equal(xp[j], x[i]), ("permutation", i)
    # system 2 replaced by another one that pads to the group's shape (1840 atoms, 240 tokens)
    other = make_batch(200, 9, 40, 128, 4)
    poses.append(reference_conformers(other, n_conf=8, seed=20))
    bs.append(to_dev(other))
    seeds.append(9)
    facs.append(6.0)
    mols.append(None)
    xn = run([0, 1, 3])
    assert torch.equal(xn[0], x[0]) and torch.equal(xn[1], x[1]), "neighbour"


def test_redock_many_groups_in_lockstep(small):
    from physdock_amd.driver import next_gamma_factor, redock, redock_many
    from physdock_amd.synthetic import make_batch, reference_conformers
    model, cfg, P = small
    systems = []
    for i, (n, nl) in enumerate([(18, 6), (14, 5), (16, 6), (18, 4)]):
        b = make_batch(n, 5, nl, 8, seed=70 + i)
        systems.append((to_dev(b), {"ref_mol_poses": reference_conformers(b, n_conf=6, seed=80 + i), "seed": 100 + i}))

    def accept(x):
        return float(x[0, 0]) > 0.0

    common = dict(physics_correction=True, accept_fn=accept, max_samples=4, max_rounds=3, num_samples_per_round=3, steps=6,
                  ranking=False)
    res = redock_many(model, systems, group=3, **common)
    assert len(res) == 4
    for (sb, _), r in zip(systems, res):
        log = r["rounds"]
        assert log[0]["round"] == 0 and log[0]["templates"] == 0 and log[0]["gamma_factor"] == 6.0
        for a, b in zip(log, log[1:]):
            assert b["gamma_factor"] == next_gamma_factor(a["gamma_factor"], a["accepted"] > 0)
            assert b["templates"] > 0
        assert r["accepted"] == sum(e["accepted"] for e in log)
        assert r["poses"].shape[1:] == (sb["ref_pos"].shape[0], 3)
    # each system's rounds are the ones redock gives it alone (accept counts, thresholds, template pools)
    for (sb, kw), r in zip(systems, res):
        solo = redock(model, sb, **dict(common, **kw))
        assert r["rounds"] == solo["rounds"] and r["accepted"] == solo["accepted"] and r["gamma_factor"] == solo["gamma_factor"]
    # results in input order, invariant under a permutation of the input list
    perm = [3, 1, 0, 2]
    rp = redock_many(model, [systems[i] for i in perm], group=3, **common)
    for j, i in enumerate(perm):
        assert rp[j]["rounds"] == res[i]["rounds"] and rp[j]["poses"].shape == res[i]["poses"].shape


def _differing_leaves(a, b, path="result"):
    """the paths at which two result trees differ: another key set, a tensor leaf that is not torch.equal (a NaN equals a NaN in the
    same place), any other leaf that is not =="""
    if isinstance(a, dict) or isinstance(b, dict):
        if not (isinstance(a, dict) and isinstance(b, dict)) or set(a) != set(b):
            return [path + ": keys"]
        return [d for k in a for d in _differing_leaves(a[k], b[k], f"{path}[{k!r}]")]
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)) or a.shape != b.shape or a.dtype != b.dtype or a.device != b.device:
            return [path + ": tensor kind"]
        if a.dtype.is_floating_point:
            same = bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())
        else:
            same = torch.equal(a, b)
        return [] if same else [path]
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b) and type(a) is type(b):
        return [d for i, (u, w) in enumerate(zip(a, b)) for d in _differing_leaves(u, w, f"{path}[{i}]")]
    return [] if a == b else [path]


def test_a_group_of_one_returns_what_redock_returns(small):
    """redock_many(group=1) against redock for one seeded system with physics correction, ranking and the pose scorers: the same key
    tree, every tensor leaf torch.equal (NaN = NaN in place), every other leaf ==.  (A group of one samples bit-identically to
    sample_diffusion, test_one_system_equals_sample_diffusion, and both callers run the same per-system rules, driver._RedockState.)
    One leaf is cut before the comparison: sdf["bytes"] is a buffer of the records' upper bound whose bytes behind offsets[n] are
    never written (`SdfTemplate.format`), so only the SD file itself, bytes[:offsets[n]], is compared."""
    from physdock_amd import BestFitRmsd, PoseClusters, TorsionFingerprint
    from physdock_amd.driver import ligand_atom_mask, redock, redock_many
    from physdock_amd.interactions import InteractionFingerprint
    from physdock_amd.scoring import VinaScore
    from physdock_amd.sdfio import SdfTemplate
    from physdock_amd.shape import ShapeOverlap, ShapeSpec
    from physdock_amd.synthetic import make_batch, reference_conformers
    from physdock_amd.validity import PoseValidity
    model, cfg, P = small
    raw = make_batch(18, 5, 6, 8, seed=70)
    b = to_dev(raw)
    lig = torch.nonzero(ligand_atom_mask(b)).flatten()
    chain = [(i, i + 1) for i in range(int(lig.numel()) - 1)]
    kw = dict(physics_correction=True, ranking=True, seed=100, ref_mol_poses=reference_conformers(raw, n_conf=6, seed=80),
              accept_fn=lambda x: float(x[0, 0]) > 0.0, max_samples=4, max_rounds=3, num_samples_per_round=3, steps=6,
              validity=PoseValidity.from_batch(b, chain), validity_filter=True, conformer_rmsd=BestFitRmsd(lig),
              torsions=TorsionFingerprint.from_batch(b, chain), clusters=PoseClusters(0.5), vina=VinaScore.from_batch(b, chain),
              interactions=InteractionFingerprint.from_batch(b, chain), shape=ShapeOverlap(ShapeSpec.from_batch(b, chain)),
              sdf=SdfTemplate.from_batch(b, chain, title="one"))
    solo = redock(model, b, **kw)
    (grouped,) = redock_many(model, [b], group=1, **kw)
    assert {"validity", "conformer_rmsd", "torsions", "clusters", "vina", "interactions", "shape", "sdf", "ranking"} <= set(solo)
    assert solo["ranking"] is not None and len(solo["rounds"]) >= 2 and all("invalid" in r for r in solo["rounds"])
    assert {"nearest_template", "pool_to_gt"} <= set(solo["conformer_rmsd"]) and "nearest_template_tfd" in solo["torsions"]
    for r in (grouped, solo):
        r["sdf"] = dict(r["sdf"], bytes=r["sdf"]["bytes"][:int(r["sdf"]["offsets"][-1])])
    assert _differing_leaves(grouped, solo) == []
