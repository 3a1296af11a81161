"""The float64 references of tests/trunk_glue_ref.py are right, the inputs of tests/test_trunk_glue_kernels_gpu.py are well posed, and
every bounded check has power.  CPU only: each reference against the committed fp32 oracle (at the tolerance tests/test_oracle_golden.py
uses for that oracle function), the conditions the GPU cases rely on, asserted on the real generators so that a badly chosen input
shows up here first, and - through the very comparison function the GPU tests call - the float64 reference rounded to fp32 (passes)
next to deliberately wrong variants computed on the CPU (rejected)."""
import pytest
import torch
import torch.nn.functional as F

import physdock_oracle as orc
import test_trunk_glue_kernels_gpu as gk
import trunk_glue_ref as tr
from conftest import golden_weights, load_golden

TOL = dict(rtol=2e-4, atol=2e-4)          # tests/test_oracle_golden.py
F32 = torch.float32


def close(a, b, **kw):
    torch.testing.assert_close(a.float(), b, **{**TOL, **kw})


def rejected(kernel, case, dev, ref, bound):
    with pytest.raises(AssertionError):
        tr.assert_within_bound(kernel, case, dev, ref, bound)
    return True


# ------------------------------------------------------------------ references against the committed oracle
def test_pair_init_z64_on_g1_rel_pos():
    g = load_golden("g1_rel_pos")
    W = golden_weights(g)["linear.weight"]
    T, CZ = g["asym_id"].shape[0], W.shape[0]
    zero = torch.zeros(T, CZ)
    z = tr.pair_init_z64(zero, zero, W, torch.zeros(CZ), g, torch.zeros(T, T))
    close(z, orc.linear({"m.linear.weight": W}, "m.linear", orc.rel_pos_features(g)))
    close(z, g["y"])


def test_pair_init_z64_atom_pair_init64_and_template_mask64_on_the_small_model(small_model_inputs):
    cfg, P, batch = small_model_inputs
    dc = cfg.model.diffusion_conditioning
    ae, te = "diffusion_conditioning.atom_embedder", "diffusion_conditioning.token_embedder"
    with torch.no_grad():
        a, _ = orc.atom_embedder(P, ae, batch, dc.inf, dc.eps)
        _, _, parts = orc.token_embedder(P, te, batch, a, dc.inf, dc.eps, return_parts=True)
        si, sj = orc.linear(P, te + ".linear_s_i", parts["s0"]), orc.linear(P, te + ".linear_s_j", parts["s0"])
        assert te + ".linear_bonds.bias" not in P and te + ".rel_pos_embedder.linear.bias" not in P
        z = tr.pair_init_z64(si, sj, P[te + ".rel_pos_embedder.linear.weight"], P[te + ".linear_bonds.weight"], batch,
                             batch["token_bonds_feature"])
        close(z, parts["z0"])
        # the AtomEmbedder's pair tensor before its FFN, from the oracle's own lines (atom_embedder)
        ref_pos, uid = batch["ref_pos"], batch["ref_space_uid"]
        d = ref_pos[:, None, :] - ref_pos[None, :, :]
        v = (uid[:, None] == uid[None, :]).to(ref_pos.dtype)[..., None]
        p = orc.linear(P, ae + ".linear_p", d) * v
        p = p + orc.linear(P, ae + ".linear_d", 1 / (1 + torch.norm(d, dim=-1)[..., None])) * v
        p = p + orc.linear(P, ae + ".linear_v", v) * v
        ra = F.relu(orc.linear(P, ae + ".linear_c", batch["ref_feat"]))
        cl, cm = orc.linear(P, ae + ".linear_c_l", ra), orc.linear(P, ae + ".linear_c_m", ra)
        assert not any(ae + f".linear_{k}.bias" in P for k in "pdv")
        ap = tr.atom_pair_init64(ref_pos, uid, cl, cm, P[ae + ".linear_p.weight"], P[ae + ".linear_d.weight"], P[ae + ".linear_v.weight"])
        close(ap, cl[:, None, :] + cm[None, :, :] + p)
        # the template mask line of template_pair_embedder
        tf, asym = batch["templ_feat"], batch["asym_id"]
        close(tr.template_mask64(batch["z_mask"], tf, asym), batch["z_mask"] * tf[..., 39] * (asym[None] == asym[:, None]).to(tf.dtype))
    c = gk.template_mask_case(24, 40)
    want = c["z_mask"] * c["templ_feat"][..., 39] * (c["asym"][None] == c["asym"][:, None]).float()
    assert torch.equal(tr.template_mask64(**c, dtype=F32), want) and 0.1 < float((want != 0).float().mean()) < 0.9


def test_segment_pool64_against_the_oracle(small_model_inputs):
    _, _, batch = small_model_inputs
    g = gk.gen(1)
    for chunks in (batch["token_id_to_chunk_sizes"], torch.tensor([9, 1, 17, 8, 16, 7, 1, 1])):      # (the oracle needs >= 1 atom per token)
        ts = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(chunks, 0)])
        u = torch.randn(3, int(ts[-1]), 8, generator=g)
        close(tr.segment_pool64(u, ts), orc.segment_mean_pool(u, chunks), atol=1e-5)
        add = torch.randn(chunks.numel(), 8, generator=g)
        close(tr.segment_pool64(u, ts, add), orc.segment_mean_pool(u, chunks) + add, atol=1e-5)


def test_gathers_and_axpby_known_answers():
    ba = torch.arange(12.0).reshape(1, 3, 4)
    us = torch.tensor([[[100.0] * 4, [200.0] * 4]])
    assert torch.equal(tr.unpool_add64(ba, us, [1, 0, 1]), ba.double() + torch.tensor([200.0, 100.0, 200.0])[None, :, None])
    y, x = torch.ones(3, 4), torch.tensor([[10.0] * 4, [20.0] * 4])
    assert torch.equal(tr.gather_rows_add64(y, x, [1, 1, 0], dtype=F32), torch.tensor([21.0, 21.0, 11.0])[:, None].expand(3, 4))
    ap, zt = torch.zeros(2, 2, 4), torch.arange(16.0).reshape(2, 2, 4)
    assert torch.equal(tr.pair_gather_add64(ap, zt, [1, 0], dtype=F32), zt.flip(0).flip(1))           # [l, m] <- zt[a2t[l], a2t[m]]
    a, b = torch.tensor([1.0, 2.0]), torch.tensor([4.0, 8.0])
    assert torch.equal(tr.axpby64(a, -0.5, b, torch.tensor([0.5]), 0.25), torch.tensor([0.0, 0.0], dtype=torch.float64))
    assert torch.equal(tr.axpby64(a, -0.5, None, torch.tensor([0.5]), 0.25), torch.tensor([-0.5, -1.0], dtype=torch.float64))
    assert torch.equal(tr.axpby64(a, 1.0, b, None, 0.25), torch.tensor([2.0, 4.0], dtype=torch.float64))


# ------------------------------------------------------------------ the conditions the GPU cases rely on
@pytest.mark.parametrize("T", sorted({t for t, _ in gk.PAIR_Z_CASES}))
def test_pair_init_z_inputs_reach_every_class(T):
    c = gk.pair_init_z_case(T, 32)
    ids = c["ids"]
    asym, sym, ent, res = (ids[k].long() for k in ("asym_id", "sym_id", "entity_id", "residue_index"))
    same_chain, same_ent = asym[:, None] == asym[None], ent[:, None] == ent[None]
    off = (res[:, None] - res[None])[same_chain]
    for cond in (off < -32, off == -32, off == 0, off == 32, off > 32):
        assert cond.any()
    assert (~same_chain).any()                                                  # d_res class 65
    d_chain = torch.where(same_chain | ~same_ent, torch.tensor(5), torch.clamp(sym[:, None] - sym[None] + 2, 0, 4))
    assert set(d_chain.flatten().tolist()) == {0, 1, 2, 3, 4, 5}
    assert same_ent.any() and (~same_ent).any() and (same_ent & ~same_chain).any()
    assert 0.1 < float((c["bonds"] != 0).float().mean()) < 0.5
    assert float(c["si"].abs().min()) > 0 and float(c["sj"].abs().min()) > 0 and float(c["wb"].abs().min()) > 0
    assert len(set(asym.tolist())) == len(gk._CHAINS) and not torch.equal(asym, asym.sort().values)


def test_pair_init_z_cases_cover_the_key_split_and_the_block_sizes():
    assert {t for t, _ in gk.PAIR_Z_CASES} == {24, 63, 64, 65, 80, 97}
    assert {cz for _, cz in gk.PAIR_Z_CASES} == {32, 128, 160} and (65, 160) in gk.PAIR_Z_CASES
    chunks = lambda T: -(-T // -(-T // 16))                # key chunks of ceil(T / 16) that hold a key
    assert chunks(65) == 13 and chunks(97) == 14           # both leave empty trailing chunks
    assert 97 % -(-97 // 16) == 6                          # and 97 a short last chunk
    assert chunks(64) == 16 and chunks(80) == 16 and 80 % 16 == 0


def test_pool_tables_hold_the_boundaries_of_the_eight_wide_load():
    tabs = gk.pool_tables()
    assert len(tabs) == gk.POOL_G and len({tuple(t[0].tolist()) for t in tabs}) == gk.POOL_G          # different tables
    for ts, a2t, n in tabs:
        assert ts.dtype == torch.int32 and ts.shape == (gk.POOL_T + 1,) and a2t.shape == (gk.POOL_A,)
        assert torch.equal((ts[1:] - ts[:-1]).long(), n) and int(ts[0]) == 0
        assert {0, 1, 7, 8, 9, 16, 17} <= set(n.tolist())
        a_real, t_real = int(ts[-1]), int(torch.nonzero(n)[-1]) + 1
        assert int(ts[t_real]) == a_real and n[t_real - 1] > 0                  # the last real token ends at the last real atom
        assert a_real < gk.POOL_A                                               # padded atoms behind it
        assert t_real <= gk.POOL_T - 2 and (ts[t_real:] == a_real).all()        # padded tokens with start == end
        assert (n[:t_real] == 0).any()                                          # and a token without atoms among the real ones
        assert (a2t[a_real:] == 0).all()
        for t in range(gk.POOL_T):
            assert (a2t[int(ts[t]):int(ts[t + 1])] == t).all()
    c = gk.pool_case(4, 3)
    for gi, (ts, _, _) in enumerate(tabs):
        u = c["u"][gi * 3:(gi + 1) * 3]
        assert torch.isnan(u[:, int(ts[-1]):]).all() and torch.isfinite(u[:, :int(ts[-1])]).all()


@pytest.mark.parametrize("A", gk.ATOM_PAIR_A)
def test_atom_pair_init_inputs(A):
    c = gk.atom_pair_init_case(A, 16)
    same = tr.atom_pair_same_uid(c["uid"])
    assert same.diagonal().all()
    d = (c["pos"][:, None] - c["pos"][None]).norm(dim=-1)
    if A > 1:
        offd = ~torch.eye(A, dtype=torch.bool)
        assert (same & offd).any() and (~same & offd).any()                      # both uid outcomes off the diagonal
        assert ((d == 0) & same & offd).any()                                    # a coincident pair: d = 0, 1 / (1 + |d|) = 1
        assert not torch.equal(c["uid"], c["uid"].sort().values)
    else:
        assert float(d) == 0.0


def test_gather_and_mask_inputs():
    for A, T in ((70, 24), (259, 24), (70, 1)):
        a2t = gk.pair_gather_add_case(A, T, 8)["a2t"]
        assert (a2t[-5:] == 0).all() and a2t.dtype == torch.int64 and len(set(a2t.tolist())) < A
        if T > 1:
            assert len(set(a2t.tolist())) > T // 2 and not torch.equal(a2t, a2t.sort().values)
    zt = gk.pair_gather_add_case(70, 24, 8)["zt"]
    assert not torch.equal(zt, zt.transpose(0, 1))
    for R in (70, 259):
        c = gk.gather_rows_case(R, 4)
        idx = c["idx"]
        assert c["x"].shape[0] < R and len(set(idx.tolist())) < R and not torch.equal(idx, idx.sort().values)
    for T, D in ((24, 40), (65, 7)):
        c = gk.template_mask_case(T, D)
        zm = c["z_mask"]
        assert ((zm != 0) & (zm != 1)).any() and (zm == 0).any() and len(set(c["asym"].tolist())) == 3
        assert not torch.equal(c["templ_feat"][..., -1], c["templ_feat"][..., -2])


# ------------------------------------------------------------------ every bound is tight against its signal; every check has power
def _tight(ref, bound):
    """the bound is at least 50 x smaller than the mean magnitude of the output it guards"""
    return 50 * float(bound.max()) <= float(ref.abs().mean())


@pytest.mark.parametrize("T,CZ", gk.PAIR_Z_CASES)
def test_pair_init_z_check_has_power(T, CZ):
    c = gk.pair_init_z_case(T, CZ)
    ref, bound = gk.pair_init_z_expected(T, CZ)
    assert _tight(ref, bound)
    tr.assert_within_bound("pair_init_z (fp32 of the reference)", f"T={T} CZ={CZ}", ref.float(), ref, bound)
    W63 = c["W"].clone()
    W63[:, 64] = W63[:, 63]                                # d_res clamped at 63: offsets >= +32 take the class of +31
    assert rejected("pair_init_z (d_res clamped at 63)", T, tr.pair_init_z64(**{**c, "W": W63}).float(), ref, bound)
    wrong_row = tr.pair_init_z64(**{**c, "si": c["si"] + c["sj"], "sj": torch.zeros_like(c["sj"])})      # sj[i] in the place of sj[j]
    assert rejected("pair_init_z (sj row i)", T, wrong_row.float(), ref, bound)


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("C,B", [(4, 1), (4, 3), (256, 1), (256, 3)])
def test_segment_pool_check_has_power(C, B, with_add):
    c = gk.pool_case(C, B)
    ref, bound = gk.pool_expected(C, B, with_add)
    assert _tight(ref, bound)
    tr.assert_within_bound("segment_pool (fp32 of the reference)", f"C={C} B={B} add={with_add}", ref.float(), ref, bound)
    by_n, dropped = [], []
    for gi, (ts, _, n) in enumerate(gk.pool_tables()):
        u, add = c["u"][gi * B:(gi + 1) * B], c["add"][gi] if with_add else None
        pooled = tr.segment_pool64(u, ts)
        nn = n.double()[None, :, None]
        w = torch.where(nn > 0, pooled * (nn + 1e-3) / nn.clamp(min=1), pooled)                      # divided by n, not n + 1e-3
        by_n.append(w if add is None else w + add.double()[None])
        u9 = u.clone()
        for t in torch.nonzero(n == 9).flatten().tolist():                                            # the ninth atom never added
            u9[:, int(ts[t + 1]) - 1] = 0
        dropped.append(tr.segment_pool64(u9, ts, add))
    assert rejected("segment_pool (/ n)", C, torch.cat(by_n).float(), ref, bound)
    assert rejected("segment_pool (ninth atom dropped)", C, torch.cat(dropped).float(), ref, bound)


@pytest.mark.parametrize("n", gk.AXPBY_N)
def test_axpby_check_has_power(n):
    c = gk.axpby_case(n)
    for v in gk.axpby_variants():
        kw = gk.axpby_args(c, *v)
        ref, bound = tr.axpby64(**kw), tr.axpby_bound(**kw)
        assert _tight(ref, bound)
        tr.assert_within_bound("axpby (fp32 of the reference)", f"n={n} {v}", ref.float(), ref, bound)
        if n % 4:
            stale = ref.float().clone()
            stale[n - n % 4:] = 0.0                        # the tail elements left unwritten (a zeroed output buffer)
            assert rejected("axpby (tail unwritten)", n, stale, ref, bound)
            stale[n - n % 4:] = float("nan")               # (a NaN-filled one)
            assert rejected("axpby (tail unwritten)", n, stale, ref, bound)


@pytest.mark.parametrize("C", gk.C_AP)
@pytest.mark.parametrize("A", gk.ATOM_PAIR_A)
def test_atom_pair_init_check_has_power(A, C):
    c = gk.atom_pair_init_case(A, C)
    ref, bound, ref32 = gk.atom_pair_init_expected(A, C)
    assert _tight(ref, bound)
    tr.assert_within_bound("atom_pair_init (fp32 of the reference)", f"A={A} c_ap={C}", ref.float(), ref, bound)
    tr.assert_within_bound("atom_pair_init (torch fp32)", f"A={A} c_ap={C}", ref32, ref, bound)
    other = ~tr.atom_pair_same_uid(c["uid"])
    assert torch.equal(ref32[other], (c["cl"][:, None] + c["cm"][None])[other])
    no_inv = tr.atom_pair_init64(**{**c, "Wd": torch.zeros_like(c["Wd"])})                            # the 1 / (1 + |d|) term lost
    assert rejected("atom_pair_init (no Wd term)", A, no_inv.float(), ref, bound)
    if A > 1:
        swapped = tr.atom_pair_init64(**{**c, "cl": c["cm"], "cm": c["cl"]})                          # cl / cm rows exchanged
        assert rejected("atom_pair_init (cl <-> cm)", A, swapped.float(), ref, bound)
