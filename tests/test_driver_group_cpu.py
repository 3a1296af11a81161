"""driver._redock_group (the lockstep round loop of redock_many(group=)) against driver.redock, system by system, with recording
fake samplers: the two callers share the per-system rules (driver._RedockState) and may differ only where sample_diffusion and
sample_diffusion_many differ.  The device pieces are replaced by stand-ins as in test_driver_cpu, so this runs without a GPU."""
import pytest
import torch

from physdock_amd import driver

A, T, L, C = 12, 5, 4, 9


def poses_of_call(n_call, n):
    return (100.0 * n_call + torch.arange(n, dtype=torch.float32))[:, None, None].expand(n, A, 3).clone()


class FakeModel:
    """test_driver_cpu.FakeModel plus the grouped entry points: every sampler call returns 100 x its call number + arange per system"""

    def __init__(self, reuse=False):
        self.calls, self.many_calls = [], []
        if reuse:
            self.supports_conditioning_reuse = True

    def sample_diffusion(self, batch, **kw):
        self.calls.append(dict(kw, msa_tag=float(batch["msa_feat"].flatten()[0])))
        x = poses_of_call(len(self.calls), kw["num_sample"])
        return (x, ("a", "ap", "s", len(self.calls))) if kw.get("return_conditioning") else x

    def _prepare_batch(self, batch):
        return dict(batch, target_feat=torch.zeros(T, 1))

    @staticmethod
    def _pad_to_group(pbatches):
        return pbatches

    def sample_diffusion_many(self, pbatches, **kw):
        assert all(pb["target_feat"].shape[0] == T for pb in pbatches)
        self.many_calls.append(dict(kw, msa_tags=[float(pb["msa_feat"].flatten()[0]) for pb in pbatches]))
        xs = [poses_of_call(len(self.many_calls), kw["num_sample"]) for _ in pbatches]
        return (xs, [("a", "ap", "s", len(self.many_calls)) for _ in pbatches]) if kw.get("return_conditioning") else xs


@pytest.fixture
def setup(monkeypatch):
    batch = {"is_ligand": torch.tensor([0, 0, 0, 0, 1.0]), "atom_id_to_token_id": torch.tensor([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4]),
             "pocket_res_feat": torch.ones(T), "x_gt": torch.zeros(A, 3), "msa_feat": torch.zeros(2, T, 34),
             "batch_msa_feat": torch.arange(10, dtype=torch.float32)[:, None, None, None].expand(10, 2, T, 34).clone()}
    poses = torch.arange(C, dtype=torch.float32)[:, None, None].expand(C, L, 3).clone()
    monkeypatch.setattr(driver, "weighted_rigid_align", lambda x_gt, x, w: x)
    monkeypatch.setattr(driver, "select_reference_templates",
                        lambda x_pred, ligand_idx, ref, k: torch.arange(ref.shape[0] - 1, -1, -1)[:max(k, 0)])
    return batch, poses


def verdicts(seq):
    it = iter(seq)
    return lambda x: next(it)


def same_tensor(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


def assert_same_result(got, solo):
    assert got["rounds"] == solo["rounds"] and got["accepted"] == solo["accepted"] and got["gamma_factor"] == solo["gamma_factor"]
    assert torch.equal(got["poses"], solo["poses"]) and set(got) == set(solo)


def assert_same_calls(many_calls, slots, calls):
    """round by round, what reached the grouped sampler for one system (its slot in each call, None: not in it) and the single sampler"""
    mine = [(m, s) for m, s in zip(many_calls, slots) if s is not None]
    assert len(mine) == len(calls)
    for (m, s), c in zip(mine, calls):
        assert m["mmff_gamma_0_factor"][s] == c["mmff_gamma_0_factor"] and m["ode_step_scale_eta"][s] == c["ode_step_scale_eta"]
        assert m["align_ref_pos"] is c["align_ref_pos"] and same_tensor(m["ref_mol_poses"][s], c["ref_mol_poses"])
        assert m["seeds"][s] == c["seed"] and m["msa_tags"][s] == c["msa_tag"]
        assert m["num_sample"] == c["num_sample"] and m["steps"] == c["steps"]
        assert m["karras_noise_schedule_power"] == c["karras_noise_schedule_power"] and m["ref_mol"][s] is c["ref_mol"]


def test_a_group_of_one_runs_the_rounds_of_redock(setup):
    batch, poses = setup
    seq = [False] * 4 + [True, False, False, True] + [True] * 4                    # round 0 none, round 1 two, round 2 all
    common = dict(physics_correction=True, max_samples=5, max_rounds=10, num_samples_per_round=4, steps=7, ranking=False)
    kw = dict(ref_mol_poses=poses, seed=11)
    grouped, single = FakeModel(), FakeModel()
    (got,) = driver._redock_group(grouped, [(batch, dict(kw, accept_fn=verdicts(seq)))], common)
    solo = driver.redock(single, batch, **common, **kw, accept_fn=verdicts(seq))
    assert [r["accepted"] for r in solo["rounds"]] == [0, 2, 4] and len(single.calls) == 3
    assert_same_result(got, solo)
    assert_same_calls(grouped.many_calls, [0, 0, 0], single.calls)
    assert [c["seed"] for c in single.calls] == [11, 12, 13] and [c["msa_tag"] for c in single.calls] == [0.0, 1.0, 2.0]
    assert [c["ref_mol_poses"] is None for c in single.calls] == [True, False, False]


def test_reject_top_up(setup):
    batch, poses = setup
    common = dict(physics_correction=True, accept_fn=lambda x: False, max_samples=3, max_rounds=8, num_samples_per_round=2,
                  mmff_gamma_0_factor_start=1.2, ranking=False, ref_mol_poses=poses, seed=4)
    grouped, single = FakeModel(), FakeModel()
    (got,) = driver._redock_group(grouped, [(batch, {})], common)
    solo = driver.redock(single, batch, **common)
    assert solo["accepted"] == 0 and torch.equal(solo["poses"][:, 0, 0], torch.tensor([701.0, 800.0, 801.0]))
    assert_same_result(got, solo)
    assert_same_calls(grouped.many_calls, [0] * 8, single.calls)


def test_a_system_that_is_done_leaves_the_group(setup):
    """two systems, the first reaches max_samples a round before the second: it is not in the third call, and the second still gets
    exactly the rounds redock gives it alone"""
    batch, poses = setup
    b2 = dict(batch, msa_feat=batch["msa_feat"] + 7.0, batch_msa_feat=batch["batch_msa_feat"] + 20.0)
    seqs = [[True] * 4, [True, False, True, False, True, True]]
    common = dict(physics_correction=True, max_samples=4, max_rounds=6, num_samples_per_round=2, ranking=False, ref_mol_poses=poses)
    kws = [dict(seed=3), dict(seed=50, mmff_gamma_0_factor_start=2.0)]
    grouped = FakeModel()
    res = driver._redock_group(grouped, [(b, dict(kw, accept_fn=verdicts(s))) for b, kw, s in zip((batch, b2), kws, seqs)], common)
    assert [len(m["seeds"]) for m in grouped.many_calls] == [2, 2, 1]
    assert grouped.many_calls[2]["seeds"] == [52] and grouped.many_calls[2]["msa_tags"] == [22.0]
    for i, (b, kw, s) in enumerate(zip((batch, b2), kws, seqs)):
        single = FakeModel()
        solo = driver.redock(single, b, **common, **kw, accept_fn=verdicts(s))
        assert len(solo["rounds"]) == 2 + i
        assert_same_result(res[i], solo)
        assert_same_calls(grouped.many_calls, [i, i, 0 if i else None], single.calls)


def test_shared_conditioning_is_taken_and_released_alike(setup):
    """without re-sampled MSAs the rounds share round 0's conditioning: both callers ask for it in round 0, hand the same object on in
    every later round and ask for no other"""
    batch, poses = setup
    batch = {k: v for k, v in batch.items() if k != "batch_msa_feat"}
    common = dict(physics_correction=True, accept_fn=lambda x: False, max_samples=3, max_rounds=3, num_samples_per_round=2,
                  ranking=False, ref_mol_poses=poses, seed=1)
    grouped, single = FakeModel(reuse=True), FakeModel(reuse=True)
    (got,) = driver._redock_group(grouped, [(batch, {})], common)
    solo = driver.redock(single, batch, **common)
    assert_same_result(got, solo)
    cond = ("a", "ap", "s", 1)
    assert [bool(c.get("return_conditioning")) for c in single.calls] == [True, False, False]
    assert [c.get("conditioning") for c in single.calls] == [None, cond, cond]
    assert [bool(m["return_conditioning"]) for m in grouped.many_calls] == [True, False, False]
    assert [m["conditionings"] for m in grouped.many_calls] == [[None], [cond], [cond]]
    for reuse_model in (grouped, single):
        reuse_model.calls.clear(), reuse_model.many_calls.clear()
    driver._redock_group(grouped, [(batch, {})], dict(common, reuse_conditioning=False))
    driver.redock(single, batch, **dict(common, reuse_conditioning=False))
    assert all("conditioning" not in c and "return_conditioning" not in c for c in single.calls) and len(single.calls) == 3
    assert all(m["conditionings"] == [None] and not m["return_conditioning"] for m in grouped.many_calls) and len(grouped.many_calls) == 3


def test_group_refuses_what_it_cannot_pass_on(setup):
    batch, poses = setup
    with pytest.raises(TypeError):
        driver._redock_group(FakeModel(), [(batch, {"surfaces": object()})], {})
    with pytest.raises(TypeError):
        driver.redock(FakeModel(), batch, surfaces=object())
    with pytest.raises(ValueError, match="relax_fn.*not supported by grouped sampling"):
        driver._redock_group(FakeModel(), [(batch, {"sampler_kwargs": {"relax_fn": lambda *a: None}})], {})
    assert "relax_fn" not in driver._MANY_SAMPLER_KEYS and "seed" in driver._MANY_SAMPLER_KEYS
