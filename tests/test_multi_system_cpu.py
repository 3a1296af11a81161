"""Several systems in one sampler call (PhysDock.sample_diffusion_many, driver.redock_many(group=)): the host-side parts -
group padding, argument checks, the grouping order, the ABI fields of grouped attention.  No GPU needed."""
import pytest
import torch

from physdock_amd import PhysDock, _lib
from physdock_amd.synthetic import make_batch


def _prep(batch):
    return PhysDock._prepare_batch(batch)


def test_group_padding_masks_and_token_table():
    small, big = _prep(make_batch(14, 5, 5, 8, seed=1)), _prep(make_batch(18, 5, 6, 8, seed=2))
    A1, T1 = small["ref_pos"].shape[0], small["target_feat"].shape[0]
    A2, T2 = big["ref_pos"].shape[0], big["target_feat"].shape[0]
    assert A1 < A2 and T1 < T2
    p_small, p_big = PhysDock._pad_to_group([small, big])
    assert p_big is big                                   # a system with the group shape is not touched
    assert p_small["ref_pos"].shape[0] == A2 and p_small["target_feat"].shape[0] == T2
    assert p_small["_A_real"] == small["_A_real"] and p_small["_T_real"] == small["_T_real"]
    # padded atoms / tokens are masked and own nothing
    assert float(p_small["a_mask"][A1:].abs().sum()) == 0 and torch.equal(p_small["a_mask"][:A1], small["a_mask"])
    assert float(p_small["ap_mask"][A1:].abs().sum()) == 0 and float(p_small["ap_mask"][:, A1:].abs().sum()) == 0
    assert float(p_small["z_mask"][T1:].abs().sum()) == 0 and float(p_small["z_mask"][:, T1:].abs().sum()) == 0
    ts = p_small["_tok_start"]
    assert ts.shape[0] == T2 + 1 and torch.equal(ts[:T1 + 1], small["_tok_start"])
    assert torch.all(ts[T1:] == small["_tok_start"][-1])   # padded tokens: empty segments
    assert torch.all(p_small["atom_id_to_token_id"][A1:] == 0)
    assert p_small["msa_feat"].shape[1] == T2 and p_small["templ_feat"].shape[:2] == (T2, T2)
    for k in ("ref_feat", "ref_pos", "target_feat", "msa_feat", "ref_space_uid", "asym_id"):
        assert p_small[k].is_contiguous(), k
    # the uids of padded atoms are new, as _prepare_batch pads
    assert int(p_small["ref_space_uid"][A1:].min()) > int(small["ref_space_uid"].max())


def test_group_padding_of_equal_shapes_is_a_no_op():
    a, b = _prep(make_batch(18, 5, 6, 8, seed=3)), _prep(make_batch(18, 5, 6, 8, seed=4))
    out = PhysDock._pad_to_group([a, b])
    assert out[0] is a and out[1] is b


def test_argument_checks():
    from physdock_amd.configs import small_config
    m = PhysDock(small_config())
    b = make_batch(18, 5, 6, 8, seed=0)
    assert m.sample_diffusion_many([]) == []
    with pytest.raises(ValueError, match="entries for 2 systems"):
        m.sample_diffusion_many([b, b], ode_step_scale_eta=[1.0, 1.0, 1.5])
    with pytest.raises(ValueError, match="one entry per system"):
        m.sample_diffusion_many([b, b], ref_mol_poses=torch.zeros(2, 6, 3))
    with pytest.raises(ValueError, match="for every system or for none"):
        m.sample_diffusion_many([b, b], noises=[None, {}])
    with pytest.raises(ValueError, match="host"):
        m.sample_diffusion_many([b], ref_mol=[object()], relax_fn=lambda *a: None)


def test_host_relaxers_are_refused(monkeypatch):
    from physdock_amd import physics
    from physdock_amd.configs import small_config
    monkeypatch.setattr(physics, "resolve_relaxer", lambda m, f, backend="auto": physics.Relaxer("host", fn=lambda *a: None, ref_mol=m))
    with pytest.raises(ValueError, match="serialise the group"):
        PhysDock(small_config()).sample_diffusion_many([make_batch(18, 5, 6, 8, seed=0)], ref_mol=["mol"])


def test_group_order():
    from physdock_amd.driver import group_order
    shapes = [(1856, 228), (2048, 256), (1856, 228), (1920, 240), (2048, 256)]
    assert group_order(shapes, 3) == [[1, 4, 3], [0, 2]]
    assert group_order(shapes, 1) == [[1], [4], [3], [0], [2]]
    assert group_order([], 2) == []
    assert sorted(i for g in group_order(shapes, 2) for i in g) == list(range(5))
    with pytest.raises(ValueError):
        group_order(shapes, 0)


def test_grouped_attention_abi_fields():
    names = [f[0] for f in _lib.AttnArgs._fields_]
    assert names[-3:] == ["group_samples", "bias_gstride", "nk_group"]
    a = _lib.AttnArgs()
    assert a.group_samples == 0 and a.bias_gstride == 0 and not a.nk_group      # zero-initialised: today's behaviour
    assert _lib.ABI_VERSION >= 10
    decl = _lib.header_symbols()
    L = _lib.lib()                       # the built library exports every declared entry point (build() checks the same)
    for s in ("pd_precond_g", "pd_segment_pool_g", "pd_unpool_add_g", "pd_downscale_pool_g"):
        assert s in decl and hasattr(L, s), s
    assert L.pd_abi_version() == _lib.ABI_VERSION


def test_tail_keys_are_the_same_for_one_system_and_for_slot_0_of_a_group():
    """sampling.tail_key / tail_kind: the single-system loop and slot 0 of a group key a plan entry alike apart from `common`
    (a group's starts with "many" and carries the group's fields); a device relaxer's table signature, mmff_iters, the ligand
    atom count and the pool's size are part of the key"""
    from types import SimpleNamespace as NS
    from physdock_amd import sampling
    from physdock_amd.configs import small_config
    m = PhysDock(small_config())
    sig, plan = m._step_plan(6, 0.8, 1.0, 1.5, 1.0, 6.0, True, 1000)
    assert [p["align"] for p in plan] == [True] * 3 + [False] * 3 and [p["mmff"] for p in plan] == [False] * 3 + [True] * 3
    _, bare = m._step_plan(6, 0.8, 1.0, 1.5, 1.0, 6.0, True, 1000, relaxes=False)
    assert not any(p["mmff"] for p in bare)                  # no molecule: the relaxation branch is unreachable

    def slot(sig_="abc", n_lig=6, n_conf=4, kind="device", poses=True, plan=plan):
        terms = NS(signature=lambda: (n_lig, sig_))
        return NS(g=0, plan=plan, relaxer=NS(kind=kind, terms=terms), n_lig=n_lig, n_conf=n_conf, poses=object() if poses else None)
    sched = sampling.sched_id(6, sig, 0.8, 1.0, 1000)
    one = (3, 96, 24, 96, 24, sched, False, 1.003, 2)
    many = ("many", 1, 3, 96, 24, (96,), (24,), 8, sched, False, 1.003, (2,))
    for i in range(6):
        k1, kg = sampling.tail_key(one, slot(), i, 5), sampling.tail_key(many, slot(), i, 5)
        assert k1[0] is one and kg[0] is many and kg[0][0] == "many" and k1[1] == kg[1] == "T"
        assert k1[1:] == kg[1:]
    assert sampling.tail_kind(plan[0], slot(), 5) == ("align", (4, 6))
    assert sampling.tail_kind(plan[0], slot(poses=False), 5) == ("align", False)
    assert sampling.tail_kind(plan[5], slot(), 5) == ("mmff", ("device", (6, "abc"), 5, 6))
    assert sampling.tail_kind(bare[5], slot(kind="none"), 5) == ("plain",)
    k = sampling.tail_key(one, slot(), 5, 5)
    assert k != sampling.tail_key(one, slot(sig_="abd"), 5, 5)         # another table
    assert k != sampling.tail_key(one, slot(), 5, 6)                   # another iteration count
    assert k != sampling.tail_key(one, slot(kind="host"), 5, 5)
    assert sampling.tail_key(one, slot(), 0, 5) != sampling.tail_key(one, slot(n_conf=5), 0, 5)
