"""The float64 references of tests/sampler_ref.py are right, and the inputs of tests/test_sampler_kernels_gpu.py are well posed.
CPU only: Philox known answers, the moments of the Box-Muller normals, every reference against the committed fp32 oracle on the
existing golden vectors (at the tolerance tests/test_oracle_golden.py uses for that oracle function), and the conditions the GPU
cases rely on, asserted on the real generators so that a badly chosen input shows up here first."""
import numpy as np
import pytest
import torch

import physdock_oracle as orc
import sampler_ref as sr
import test_sampler_kernels_gpu as gk
from conftest import golden_weights, load_golden

TOL = dict(rtol=2e-4, atol=2e-4)          # tests/test_oracle_golden.py


def close(a, b, **kw):
    torch.testing.assert_close(a.float(), b, **{**TOL, **kw})


# ------------------------------------------------------------------ Philox and the uniforms
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    assert tuple(int(v) for v in sr.philox4x32_10(counter, key)) == want


def test_philox_is_vectorised_over_counters_and_keys():
    c0 = np.array([0, 0x243f6a88], dtype=np.uint64)
    out = sr.philox4x32_10((c0, [0, 0x85a308d3], [0, 0x13198a2e], [0, 0x03707344]), ([0, 0xa4093822], [0, 0x299f31d0]))
    assert out.shape == (2, 4)
    assert [int(v) for v in out[0]] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(v) for v in out[1]] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_u01_range():
    bits = np.array([0, 1, 255, 256, 0x7fffffff, 0x80000000, 0xfffffeff, 0xffffff00, 0xffffffff], dtype=np.uint64)
    u = sr.u01(bits)
    assert u.dtype == np.float32
    assert (u > 0).all() and (u <= 1).all()
    assert u[0] == np.float32(0.5 * 2.0 ** -24)
    assert sr.u01(0xffffffff) == np.float32(1.0)            # 2^24 - 1 + 0.5 rounds to 2^24
    rng = np.random.default_rng(0)
    assert (sr.u01(rng.integers(0, 2 ** 32, size=1 << 16, dtype=np.uint64)) > 0).all()


def test_seed_key_split():
    assert sr.seed_key(7) == (7, 0)
    assert sr.seed_key(2 ** 32 + 7) == (7, 1)
    assert sr.seed_key(2 ** 63 + 12345) == (12345, 0x80000000)


def _assert_moments(v):
    mean, var, kurt = sr.moments(v)
    n = np.asarray(v).size
    assert abs(mean) <= 5 / np.sqrt(n), mean
    assert abs(var - 1) <= 0.01, var
    assert abs(kurt - 3) <= 0.05, kurt


def test_normals4_moments():
    n = sr.normals4((np.arange(1 << 20, dtype=np.uint64), 3, 11, 2), sr.seed_key(7))
    assert n.shape == (1 << 20, 4) and np.isfinite(n).all()
    _assert_moments(n)
    for k in range(4):
        _assert_moments(n[:, k])
    # r0 from word 0 with the angle of word 1, r1 from word 2 with the angle of word 3
    u = sr.u01(sr.philox4x32_10((np.arange(8, dtype=np.uint64), 3, 11, 2), sr.seed_key(7))).astype(np.float64)
    np.testing.assert_allclose(np.hypot(n[:8, 0], n[:8, 1]), np.sqrt(-2 * np.log(u[:, 0])), rtol=1e-12)
    np.testing.assert_allclose(np.hypot(n[:8, 2], n[:8, 3]), np.sqrt(-2 * np.log(u[:, 2])), rtol=1e-12)
    np.testing.assert_allclose(np.arctan2(n[:8, 1], n[:8, 0]) % (2 * np.pi), (2 * np.pi * u[:, 1]) % (2 * np.pi), atol=1e-9)
    np.testing.assert_allclose(np.arctan2(n[:8, 3], n[:8, 2]) % (2 * np.pi), (2 * np.pi * u[:, 3]) % (2 * np.pi), atol=1e-9)
    n32 = sr.normals4((np.arange(1 << 16, dtype=np.uint64), 3, 11, 2), sr.seed_key(7), np.float32)
    assert n32.dtype == np.float32 and np.abs(n32 - n[: 1 << 16]).max() < 1e-5


def test_draw_layouts():
    key = sr.seed_key(2 ** 32 + 7)
    x = sr.init_noise_draws(2 ** 32 + 7, 5, 2.0, 3, 4)
    np.testing.assert_array_equal(x[1, 2], 2.0 * sr.normals4((2, 6, 0xFFFFFFFF, 0), key)[:3])
    u = sr.augment_rot_uniforms(2 ** 32 + 7, 199, 5, 3)
    assert u.shape == (4, 3)
    np.testing.assert_array_equal(u[:, 1], sr.u01(sr.philox4x32_10((0, 6, 199, 1), key)))
    np.testing.assert_array_equal(sr.augment_trans_draws(2 ** 32 + 7, 199, 5, 3)[1], sr.normals4((1, 6, 199, 1), key)[:3])
    np.testing.assert_array_equal(sr.augment_noise_draws(2 ** 32 + 7, 199, 5, 3, 4)[1, 2], sr.normals4((2, 6, 199, 2), key)[:3])
    assert not np.array_equal(sr.init_noise_draws(7, 0, 1.0, 2, 3), sr.init_noise_draws(2 ** 32 + 7, 0, 1.0, 2, 3))


# ------------------------------------------------------------------ references against the fp32 oracle on the goldens
def test_augment64_and_kabsch64_on_g4():
    g = load_golden("g4_augment_align")
    y = sr.augment64(g["x"], 1.0, g["mask"], g["rot_u"], g["trans"], None, 1.0, 0.0)
    close(y, g["y"], atol=1e-5)
    close(y, orc.centre_random_augmentation(g["x"], g["mask"], g["rot_u"], g["trans"]), atol=1e-5)
    noise = torch.randn(g["x"].shape, generator=torch.Generator().manual_seed(0))
    close(sr.augment64(g["x"], 1.0, g["mask"], g["rot_u"], g["trans"], noise, 1.003, 2.0), g["y"] + 1.003 * noise * 2.0, atol=1e-5)
    for xp, xg, want in ((g["x_pred"], g["x_gt2d"], g["aligned2d"]), (g["x_pred"], g["x_gt3d"], g["aligned3d"]),
                         (g["x_pred_refl"], g["x_pred"][0], g["aligned_refl"])):
        out, sv = sr.kabsch64(xp, None, xg, g["w"])
        close(out, want, atol=1e-4)
        close(out, orc.weighted_rigid_align(xp, xg, g["w"]), atol=1e-4)
        assert sv.shape == (xp.shape[0], 3) and (sv[:, 0] >= sv[:, 1]).all() and (sv[:, 1] >= sv[:, 2]).all()
        m = torch.ones(xp.shape[1])
        m[::3] = 0
        out_m, _ = sr.kabsch64(xp, m, xg, g["w"])
        close(out_m, orc.weighted_rigid_align(xp * m[None, :, None], xg, g["w"]), atol=1e-4)


def test_kabsch64_returns_a_proper_rotation_for_a_mirrored_target():
    c = gk.kabsch_case(257, 4, False, True, "uniform", 0.0, "mirrored")
    out, _ = sr.kabsch64(c["x_pred"], None, c["x_gt"], c["w"])
    G = c["x_gt"].double()
    a, b = out - out.mean(1, keepdim=True), G - G.mean(1, keepdim=True)
    R = torch.linalg.lstsq(b, a).solution.transpose(1, 2)                  # out = R G + t
    assert ((torch.linalg.det(R) - 1).abs() < 1e-9).all()
    assert ((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs() < 1e-9).all()


def test_template_eps64_and_pose_dist64_on_g7():
    g = load_golden("g7_reselect")
    rd = sr.pose_dist64(g["ref_mol_poses"])
    close(rd, torch.norm(g["ref_mol_poses"][:, :, None] - g["ref_mol_poses"][:, None], dim=-1), atol=1e-6)
    e = sr.template_eps64(g["ligand_poses"], rd)
    close(e, g["eps_bc"], atol=1e-6)
    close(e, orc.template_epsilon(g["ligand_poses"], rd.float()), atol=1e-6)
    assert torch.equal(torch.argmin(e, -1), g["argmin_b"])


def test_timestep_embed64_on_g1():
    g = load_golden("g1_timestep_embeddings")
    emb = sr.timestep_embed64(g["tau"])
    assert emb.shape == (g["tau"].shape[0], 256)
    close(emb, gk._timestep32(g["tau"]), atol=1e-5)
    W = {k: v.double() for k, v in golden_weights(g).items()}
    h = torch.nn.functional.silu(emb @ W["timestep_embedder.linear_1.weight"].T + W["timestep_embedder.linear_1.bias"])
    close(h @ W["timestep_embedder.linear_2.weight"].T + W["timestep_embedder.linear_2.bias"], g["y"], atol=5e-4)


def test_elementwise_references_against_fp32_formulas():
    c = gk.denoise_case(3, 7, 36)
    close(sr.denoise64(c["ba"], c["x_hat"], c["nw"], c["nb"], c["Wr"], 1e-5, c["cs_b"], c["co_b"]),
          gk._denoise32(c, 1e-5, c["cs_b"][:, None, None], c["co_b"][:, None, None]))
    c = gk.precond_case(1, 5, 91, 64)
    close(sr.precond64(c["x_hat"], c["c_in_b"], c["Wx"], c["bx"], c["a"][0]),
          gk._precond32(c["x_hat"], c["c_in_b"][:, None, None], c["Wx"], c["bx"], c["a"][0]))
    c = gk.euler_case(5, 257)
    close(sr.euler64(c["x_hat"], c["x_den"], c["x_proj"], c["wfrac"], 2560.0, 1.5, -331.0),
          gk._euler32(c["x_hat"], c["x_den"], c["x_proj"], c["wfrac"], 2560.0, 1.5, -331.0))
    close(sr.euler64(c["x_hat"], c["x_den"], None, None, 2560.0, 1.0, -331.0),
          gk._euler32(c["x_hat"], c["x_den"], None, None, 2560.0, 1.0, -331.0))
    c = gk.rmsd_case(5, 65, True)
    (D, r), (D32, r32) = sr.pairwise_rmsd64(c["x"], c["idx"], c["ref"]), gk._rmsd32(c["x"], c["idx"], c["ref"])
    close(D, D32, atol=1e-5)
    close(r, r32, atol=1e-5)


# ------------------------------------------------------------------ the conditions the GPU cases rely on
@pytest.mark.parametrize("case", gk.KABSCH_CASES, ids=gk.KABSCH_IDS)
def test_kabsch_cases_are_well_conditioned(case):
    for c in (gk.kabsch_case(*case), gk.kabsch_moved_target(gk.kabsch_case(*case))):
        margin = sr.kabsch_margin64(c["x_pred"], c["mask"], c["x_gt"], c["w"])
        print(gk.KABSCH_IDS[gk.KABSCH_CASES.index(case)], [round(float(m), 3) for m in margin])
        assert (margin >= 0.05).all(), margin
        assert float(c["w"].sum()) > 0 and int((c["w"] > 0).sum()) >= 3
    A, B, masked, per_gt, weights, offset, kind = case
    c = gk.kabsch_case(*case)
    if masked:
        assert 0.05 <= float((c["mask"] == 0).float().mean()) <= 0.15
    if weights == "sparse":
        assert float((c["w"] > 0).float().mean()) <= 0.05
    if kind == "planar":
        assert (c["x_gt"][..., 2] == offset).all()
    if kind == "mirrored":                       # the unconstrained optimum is a reflection
        _, _, sign = sr._kabsch_parts(c["x_pred"], c["mask"], c["x_gt"], c["w"])
        assert (sign < 0).all()


@pytest.mark.parametrize("case", gk.KABSCH_CASES, ids=gk.KABSCH_IDS)
def test_kabsch_moved_target_keeps_the_answer(case):
    """A rigid move of the target does not change the aligned result.  The moved target is stored in fp32, half an ulp off per
    coordinate: that shifts each output point by as much and turns the rotation by about that over (margin sqrt(A)) - with the
    margins asserted above (>= 0.25 on these inputs, 0.05 required) a few ulps at the coordinate scale, inside the ulp floor."""
    c = gk.kabsch_case(*case)
    m = gk.kabsch_moved_target(c)
    assert not torch.equal(c["x_gt"], m["x_gt"])
    ref, _ = sr.kabsch64(c["x_pred"], c["mask"], c["x_gt"], c["w"])
    ref_m, _ = sr.kabsch64(m["x_pred"], m["mask"], m["x_gt"], m["w"])
    floor = torch.minimum(gk.kabsch_floor(c, ref), gk.kabsch_floor(m, ref_m))
    diff = (ref_m - ref).abs().flatten(1).amax(1)
    print([f"{float(d / f * gk.TOL_FLOOR_ULPS):.2f} ulp" for d, f in zip(diff, floor)])
    assert (diff <= floor).all(), (diff, floor)


def test_kabsch_cases_cover_every_variant():
    col = lambda i: {c[i] for c in gk.KABSCH_CASES}
    assert {(c[0], c[1]) for c in gk.KABSCH_CASES} >= {(a, b) for a in (3, 5, 255, 256, 257, 2056) for b in (1, 4)}
    assert col(2) == {False, True} and col(3) == {False, True} and col(4) == {"uniform", "random", "sparse"}
    assert col(5) == {0.0, 1000.0} and col(6) == {"plain", "planar", "mirrored"}


@pytest.mark.parametrize("Lg", [1, 7, 64, 200])
@pytest.mark.parametrize("Cn", [1, 3, 40])
@pytest.mark.parametrize("B", [1, 5])
def test_template_cases_have_a_clear_selection(B, Cn, Lg):
    """the expected conformer beats every conformer that is not its exact copy by far more than any fp32 evaluation can move eps
    (eps is a mean of values in (0, 1): its fp32 error is of order 1e-6)"""
    c = gk.template_case(Lg, Cn, B)
    sel, gap = gk.template_expected(c, sr.pose_dist64(c["poses"]))
    assert min(gap) >= 1e-3, gap
    if Cn >= 3 and Lg > 1:
        assert int(sel[0]) == Cn // 3 and torch.equal(c["poses"][Cn - 1], c["poses"][Cn // 3])       # the tie: lower index
    if Lg == 1:                                # one atom: every distance matrix is [[0]], all conformers tie
        assert (sel == 0).all()
    assert c["A"] > Lg and len(set(c["lig_idx"].tolist())) == Lg
    assert Lg == 1 or not torch.equal(c["lig_idx"], c["lig_idx"].sort().values)              # scattered AND unsorted


def test_pooled_init_noise_reference_passes_the_moment_checks():
    p = gk.POOL
    x = sr.init_noise_draws(p["seed"], 0, 1.0, p["B"], p["A"])
    _assert_moments(x)
    assert len({x[b].tobytes() for b in range(p["B"])}) == p["B"]


def test_augment_cases_read_rot_u_as_4_by_B():
    c = gk.augment_case(5, 257)
    assert c["rot_u"].shape == (4, 5) and not torch.equal(c["rot_u"], c["rot_u"].T.reshape(4, 5))
    assert (c["mask"] == 0).any() and float(c["x"].mean()) > 250
