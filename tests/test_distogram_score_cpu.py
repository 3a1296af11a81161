"""The float64 definition tests/distogram_score_ref.py against torch and against itself, the host-side errors of
physdock_amd.distogram.DistogramScore, the C ABI's declarations, and the distogram keyword of redock before anything is sampled."""
import ctypes
import re

import numpy as np
import pytest
import torch

import distogram_score_ref as ref


@pytest.fixture(scope="module")
def base():
    c = ref.make_case()
    return c, ref.Spec(c["logits"], c["pb"], c["is_ligand"], c["s_mask"])


def planted(c, x_gt, K=ref.NO_BINS, height=20.0):
    """logits that put `height` on the bin of x_gt's pseudo-beta distances and 0 elsewhere"""
    e, _ = ref.edges_centres(no_bins=K)
    bins, _ = ref.pair_bins(x_gt[c["pb"]], x_gt[c["pb"]], e)
    l = np.zeros(bins.shape + (K,), np.float32)
    np.put_along_axis(l, bins[..., None], np.float32(height), -1)
    return l


# ------------------------------------------------------------------ the definition
def test_ref_nll_is_the_cross_entropy_of_the_same_bins(base):
    c, spec = base
    x = c["x"][0]
    bins, _ = ref.pair_bins(x[c["pb"]], x[c["pb"]], spec.e)
    u = spec.lse[..., None] - c["logits"].astype(np.float64)
    mine = np.take_along_axis(u, bins[..., None], -1)[..., 0]
    ls = torch.log_softmax(torch.from_numpy(c["logits"]).double(), -1)
    theirs = -torch.gather(ls, -1, torch.from_numpy(bins)[..., None])[..., 0].numpy()
    assert abs(mine.mean() - theirs.mean()) <= 1e-12 and np.abs(mine - theirs).max() <= 1e-12
    # and class by class through the scoring path (every class enabled): the fp32 rounding of the same float64 mean
    full = ref.Spec(c["logits"], c["pb"], c["is_ligand"], c["s_mask"], receptor=True).score(c["x"][:1])
    lig, rec = spec.lig, spec.rec
    upper = lambda idx: theirs[np.ix_(idx, idx)][np.triu_indices(len(idx), 1)]
    parts = dict(nll_interface=theirs[np.ix_(lig, rec)].ravel(), nll_ligand=upper(lig), nll_receptor=upper(rec))
    for k, v in parts.items():
        assert abs(float(full[k][0]) - v.mean()) <= 2.0 ** -23 * v.mean(), k
    every = np.concatenate(list(parts.values()))
    assert abs(float(full["nll"][0]) - every.mean()) <= 2.0 ** -23 * every.mean()
    assert list(full["n_pairs"]) == [len(lig) * len(rec), len(lig) * (len(lig) - 1) // 2, len(rec) * (len(rec) - 1) // 2]
    assert list(spec.n_pairs) == [128, 28, 0] and np.isnan(spec.score(c["x"][:1])["nll_receptor"][0])


def test_ref_the_ground_truth_beats_a_moved_ligand_under_planted_logits(base):
    c, _ = base
    x_gt = c["x"][0]
    spec = ref.Spec(planted(c, x_gt), c["pb"], c["is_ligand"], c["s_mask"])
    moved = x_gt.copy()
    moved[c["pb"][c["is_ligand"] > 0]] += np.float32([3.0, 0, 0])
    out = spec.score(np.stack([x_gt, moved]))
    assert out["nll_interface"][0] < out["nll_interface"][1] and out["nll"][0] < out["nll"][1]
    assert out["nll_interface"][0] < 1e-6, "every pair sits in its planted bin"
    assert out["contact_recovery"][0] == 1.0 and out["n_contacts"][0] > 0 and out["contact_precision"][0] > 0.99
    assert spec.cstar == 3 and abs(spec.contact_edge - (3.25 + 3 * 47.5 / 37)) < 1e-12, "8 A falls inside the bin above 7.10 A"
    pot = spec.potential(np.stack([x_gt, moved]))["potential"]
    assert pot[0] < pot[1]


def test_ref_forces_are_the_finite_differences_of_the_potential(base):
    """Tolerance: V is piecewise linear in d, so a central difference is exact as long as no pair crosses a centre within the step
    (asserted: every pair is at least 1e-3 A from a centre, the step is 1e-5 A) - up to the second-order term of d(x), about
    h^2 / d^2 < 1e-10 relative, and the rounding of the two potentials, about 2^-52 V / h = 1e-10 of a potential of order 5 against
    contributions of order 1e-2.  Both are far below 1e-6 of abs_force, the magnitude of what a force is summed from."""
    c, spec = base
    xp = c["x"].astype(np.float64)[:, c["pb"]]
    d = np.sqrt(((xp[:, :, None] - xp[:, None]) ** 2).sum(-1))
    gap = np.abs(d[..., None] - spec.c).min(-1)
    pairs = (spec.cls[:, None] == 2) & (spec.cls[None] != 0) & ~np.eye(spec.T, dtype=bool)
    clear = [p for p in range(len(xp)) if gap[p][pairs].min() >= 1e-3][:2]          # the seeded poses that keep clear of every centre
    assert len(clear) == 2 and gap[clear][:, pairs].min() >= 1e-3, "fewer than two poses keep 1e-3 A from every centre: choose another seed"
    x = c["x"][clear].astype(np.float64)
    got = spec.potential(c["x"][clear], forces=True, rounded=False)
    assert np.abs(got["potential"] - spec.potential64(x)).max() <= 1e-14
    h, worst = 1e-5, 0.0
    for r, t in enumerate(spec.lig):
        for k in range(3):
            up, dn = x.copy(), x.copy()
            up[:, c["pb"][t], k] += h
            dn[:, c["pb"][t], k] -= h
            fd = -(spec.potential64(up) - spec.potential64(dn)) / (2 * h)
            err = np.abs(fd - got["forces"][:, r, k]) / got["abs_force"][:, r]
            worst = max(worst, float(err.max()))
    print(f"largest |finite difference - force| / abs_force: {worst:.3e}")
    assert worst <= 1e-6
    assert (got["abs_force"] > 0).all() and (np.abs(got["forces"]).sum(-1) <= got["abs_force"] * (1 + 1e-12)).all()


def test_ref_the_bin_convention_at_an_edge():
    case, want = ref.edge_pairs_case()
    spec = ref.Spec(case["logits"], case["pb"], case["is_ligand"], case["s_mask"])
    out = spec.score(case["x"], detail=True)
    assert out["bins"].shape == (1, 4, 6) and out["bins"].dtype == np.uint8
    assert list(out["bins"][0, :, 0]) == want == [0, 1, 38, 0]
    assert out["bins"][0, 3, 5] == 0 and out["bins"][0, 0, 2] == 0, "a token against itself: coincident atoms, bin 0"
    assert out["ok"][0] == 1 and np.isfinite(out["nll_interface"][0])
    assert spec.potential(case["x"], forces=True)["forces"].shape == (1, 4, 3)
    far = spec.potential(case["x"], forces=True, rounded=False)
    assert np.isfinite(far["forces"]).all(), "the coincident pair contributes its value and no gradient"


def test_ref_masked_tokens_poses_that_are_not_finite_and_an_empty_ligand(base):
    c, spec = base
    pb, sm = c["pb"].copy(), c["s_mask"].copy()
    pb[2], sm[5], sm[20] = -1, 0, 0
    s = ref.Spec(c["logits"], pb, c["is_ligand"], sm)
    assert list(s.n_pairs) == [7 * 14, 21, 0] and set(s.cls[[2, 5, 20]]) == {0}
    x = c["x"][:3].copy()
    x[1, c["pb"][0], 1] = np.nan                       # an active pseudo-beta atom
    x[2, c["pb"][0] + 1, 0] = np.nan                   # nobody's pseudo-beta atom
    x[2, c["pb"][2]] = np.inf                          # the pseudo-beta atom of a token that has none here
    out = s.score(x, detail=True)
    assert list(out["ok"]) == [1, 0, 1] and np.isnan(out["nll"][1]) and out["n_contacts"][1] == 0 and not out["bins"][1].any()
    assert np.isnan(out["token_nll"][1]).all() and np.isnan(out["token_nll"][0, [2, 5, 20]]).all()
    assert np.isfinite(np.delete(out["token_nll"][0], [2, 5, 20])).all() and (out["bins"][0][:, [2, 5, 20]] == 255).all()
    clean = s.score(c["x"][2:3])
    assert all(np.array_equal(out[k][2], clean[k][0], equal_nan=True) for k in ("nll", "token_nll", "expected_error", "n_contacts"))
    none = ref.Spec(c["logits"], c["pb"], np.zeros(24), c["s_mask"]).score(c["x"][:1])
    assert list(none["n_pairs"]) == [0, 0, 0] and np.isnan(none["nll_interface"][0]) and np.isnan(none["nll"][0])
    assert np.isnan(none["token_nll"]).all() and none["ok"][0] == 1


# ------------------------------------------------------------------ the Python class on the host
def batch_of(c):
    return {"token_id_to_pseudo_beta_atom_id": torch.from_numpy(c["pb"]), "is_ligand": torch.from_numpy(c["is_ligand"]),
            "s_mask": torch.from_numpy(c["s_mask"]), "x_gt": torch.from_numpy(c["x"][0])}


def test_the_spec_agrees_with_the_definition_and_is_immutable(base):
    from physdock_amd import DistogramScore, distogram
    c, spec = base
    s = DistogramScore.from_logits(torch.from_numpy(c["logits"]), batch_of(c))
    assert np.array_equal(s.edges, spec.e) and np.array_equal(s.centres, spec.c) and s.contact_bin == spec.cstar == 3
    assert s.contact_edge == spec.contact_edge and np.array_equal(s.token_class, spec.cls) and np.array_equal(s.n_pairs, spec.n_pairs)
    assert np.array_equal(s.rows, spec.lig) and s.n_pose_atoms == c["A"] and (s.no_bins, s.n_tokens) == (39, 24)
    both = DistogramScore.from_logits(torch.from_numpy(c["logits"]), batch_of(c), receptor=True, contact_cutoff=3.0)
    assert np.array_equal(both.rows, np.concatenate([spec.lig, spec.rec])) and both.contact_bin == -1 and np.isnan(both.contact_edge)
    with pytest.raises(AttributeError, match="immutable"):
        s.receptor = True
    e2, c2 = distogram.edges_centres(1.0, 5.0, 2)
    assert list(e2) == [1.0] and list(c2) == [-1.0, 3.0]
    lone = dict(batch_of(c), token_id_to_chunk_sizes=torch.from_numpy(c["chunk"]))
    del lone["token_id_to_pseudo_beta_atom_id"]
    first = DistogramScore.from_logits(torch.from_numpy(c["logits"]), lone)
    assert np.array_equal(first.pb_atom, np.cumsum(c["chunk"]) - c["chunk"]), "without the key: the first atom of every token"
    v = np.full((1, 24), np.nan)
    v[0, 16:] = [0.5, 2.0, 2.0, np.nan, 1.0, 3.0, 0.1, 0.2]
    assert s.describe({"token_nll": v}, 0) == [(21, 3.0), (17, 2.0), (18, 2.0), (20, 1.0), (16, 0.5), (23, 0.2), (22, 0.1)] + \
        [(19, pytest.approx(float("nan"), nan_ok=True))]


def test_shape_and_dtype_errors_are_raised_before_any_launch(base, monkeypatch):
    from physdock_amd import DistogramScore, ops
    c, _ = base
    monkeypatch.setattr(ops._lib, "init", lambda: pytest.fail("a launch was prepared"))
    l, b = torch.from_numpy(c["logits"]), batch_of(c)
    for bad in (l[:, :23], l[0], l.reshape(24, 24, 39, 1), c["logits"]):
        with pytest.raises(ValueError, match=r"must be a tensor \[T,T,no_bins\]"):
            DistogramScore.from_logits(bad, b)
    with pytest.raises(ValueError, match="must be fp32"):
        DistogramScore.from_logits(l.double(), b)
    for K in (1, 65):
        with pytest.raises(ValueError, match="2 .. 64 bins"):
            DistogramScore.from_logits(torch.zeros(24, 24, K), b)
    with pytest.raises(ValueError, match="the logits are over 23 tokens"):
        DistogramScore.from_logits(l[:23, :23].contiguous(), b)
    pb = c["pb"].copy()
    pb[7] = c["A"]
    with pytest.raises(ValueError, match=f"pseudo-beta atom id of {c['A']} with poses of {c['A']} atoms"):
        DistogramScore.from_logits(l, dict(b, token_id_to_pseudo_beta_atom_id=torch.from_numpy(pb)))
    with pytest.raises(ValueError, match="contact_cutoff must be finite"):
        DistogramScore.from_logits(l, b, contact_cutoff=float("nan"))
    with pytest.raises(ValueError, match="min_bin < max_bin"):
        DistogramScore.from_logits(l, b, min_bin=5.0, max_bin=5.0)
    s = DistogramScore.from_logits(l, b)
    for call in (s.score, s.potential):
        for x in (torch.zeros(2, c["A"] + 1, 3), torch.zeros(c["A"], 3), torch.zeros(2, c["A"], 2)):
            with pytest.raises(ValueError, match=f"over poses of {c['A']} atoms"):
                call(x)
        with pytest.raises(ValueError, match="0 poses"):
            call(torch.zeros(0, c["A"], 3))
        with pytest.raises(ValueError, match="must be on the GPU"):
            call(torch.zeros(2, c["A"], 3))
    with pytest.raises(ValueError, match="a row holds 24 values"):
        s.describe({"token_nll": np.zeros((1, 23))}, 0)


# ------------------------------------------------------------------ the C ABI
NEW = {"pd_distogram_tables": 9, "pd_distogram_score": 21, "pd_distogram_reduce": 22, "pd_distogram_potential": 19}


def test_the_header_declares_the_kernels_and_the_version_stays():
    from physdock_amd import _lib, distogram
    assert _lib.ABI_VERSION == 11 and set(NEW) <= set(_lib.header_symbols())
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "physdock_hip.h")).read()
    assert int(re.search(r"#define\s+PD_DISTOGRAM_MAX_BINS\s+(\d+)", hdr).group(1)) == distogram.MAX_BINS == 64
    assert int(re.search(r"#define\s+PD_DISTOGRAM_MAX_TOKENS\s+(\d+)", hdr).group(1)) == distogram.MAX_TOKENS == 4096
    assert int(re.search(r"#define\s+PD_DISTOGRAM_VALUES\s+(\d+)", hdr).group(1)) == len(distogram.VALUE_NAMES) == 7
    src = open(_lib.os.path.join(_lib._HERE, "csrc", "distogram_score.hip")).read()
    assert "atomic" not in src.replace("no atomics", "") and "fp contract(off)" in src and "block_sum_det<256>" in src
    for text in (hdr, src, distogram.__doc__):
        assert re.search(r"self-consistency, not accuracy", text) and re.search(r"not\s+(been\s+)?validated", text, flags=re.I)


def test_the_built_library_exports_binds_and_refuses():
    from physdock_amd import _lib
    L = _lib.lib()
    assert L.pd_abi_version() == 11
    assert all(hasattr(L, k) and len(_lib.SYMBOLS[k].argtypes) == n for k, n in NEW.items())
    f = 1 << 20                                                   # an aligned address that a refused call never follows
    host = (ctypes.c_double * 65)(*range(65))
    tables = lambda T, K, cb=0, lse=f: L.pd_distogram_tables(f, host, cb, lse, f, f, T, K, None)
    assert tables(4, 65) == tables(4097, 39) == -3 and tables(4, 1) == tables(0, 39) == tables(4, 39, 38) == tables(4, 39, -2) == -1
    assert tables(4, 39, 0, f + 4) == -1 and L.pd_distogram_tables(None, host, 0, f, f, f, 4, 39, None) == -1
    score = lambda P, T, K, nl=2, nr=2, ws=64: L.pd_distogram_score(f, f, f, f, f, f, f, f, host, 3, 20.0, f, f, ws, P, 8, T, K, nl, nr, None)
    assert score(65536, 4, 39) == score(1, 4097, 39) == score(1, 4, 65) == -3
    assert score(0, 4, 39) == score(1, 4, 39, 3, 2) == score(1, 4, 39, 2, 5) == score(2, 4, 39, 2, 2, 31) == -1
    reduce = lambda P, T, K, nl=2, nr=2, NR=2: L.pd_distogram_reduce(f, f, f, f, f, f, f, f, f, 64, f, f, f, f, P, 8, T, K, nl, nr, NR, None)
    assert reduce(65536, 4, 39) == reduce(1, 4, 65) == -3 and reduce(1, 4, 39, 2, 2, 3) == reduce(1, 4, 39, 3, 2, 3) == -1
    pot = lambda P, T, K, fo=f, ab=f, ws=64: L.pd_distogram_potential(f, f, f, f, f, f, host, f, ws, f, fo, ab, P, 8, T, K, 2, 2, None)
    assert pot(65536, 4, 39) == pot(1, 4097, 39) == pot(1, 4, 65) == -3 and pot(1, 4, 39, None, f) == pot(1, 4, 39, f, None) == pot(2, 4, 39, f, f, 19) == -1


# ------------------------------------------------------------------ redock before anything is sampled
class StubModel:
    def __init__(self, A):
        self.A, self.calls = A, 0

    def sample_diffusion(self, batch, **kw):
        self.calls += 1
        n = kw["num_sample"]
        return torch.arange(n, dtype=torch.float32)[:, None, None].expand(n, self.A, 3).clone()


def test_redock_raises_for_a_missing_prerequisite_before_sampling(monkeypatch):
    from physdock_amd import PoseClusters, driver
    from physdock_amd.sdfio import redock_items
    A, T = 12, 5
    batch = {"is_ligand": torch.tensor([0, 0, 0, 0, 1.0]), "atom_id_to_token_id": torch.tensor([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4]),
             "pocket_res_feat": torch.ones(T), "x_gt": torch.full((A, 3), 0.5), "msa_feat": torch.zeros(2, T, 34)}
    monkeypatch.setattr(driver, "weighted_rigid_align", lambda x_gt, x, w: x)
    kw = dict(max_samples=3, num_samples_per_round=5, ranking=False)
    model = StubModel(A)
    assert PoseClusters(by="distogram").by == "distogram"
    with pytest.raises(ValueError, match=r"by='distogram'\) needs distogram="):
        driver.redock(model, batch, clusters=PoseClusters(by="distogram"), **kw)
    with pytest.raises(ValueError, match=r"by='distogram'\) needs distogram="):
        driver.redock(model, batch, clusters=PoseClusters(by="distogram"), distogram=False, **kw)
    with pytest.raises(ValueError, match="distogram= needs a model whose sampler returns its conditioning"):
        driver.redock(model, batch, distogram=True, **kw)
    with pytest.raises(ValueError, match="distogram= needs a model whose sampler returns its conditioning"):
        driver.redock_many(model, [(batch, {"distogram": {"receptor": True}}), batch], **kw)
    with pytest.raises(ValueError, match="distogram= takes True or a dict"):
        driver.redock(model, batch, distogram="yes", **kw)
    with pytest.raises(ValueError, match=r"unknown DistogramScore.from_logits keyword arguments \['cutoff'\]"):
        driver.redock(model, batch, distogram={"cutoff": 8.0}, **kw)
    assert model.calls == 0, "raised before anything was sampled"
    plain = driver.redock(model, batch, **kw)
    assert set(plain) == {"poses", "accepted", "rounds", "gamma_factor", "ranking"} and model.calls == 1
    assert set(driver.redock(model, batch, distogram=False, **kw)) == set(plain) and set(driver.redock(model, batch, distogram=None, **kw)) == set(plain)
    with pytest.raises(TypeError):
        driver._RedockState(batch, batch, distograms=True)
    st = driver._RedockState(batch, batch, distogram={"receptor": True})
    assert st.distogram == {"receptor": True} and st.distogram_spec is None
    with pytest.raises(RuntimeError, match="returned no conditioning"):
        driver.score_distogram(None, plain["poses"], {})
    out = dict(plain, distogram={"nll_interface": torch.tensor([0.3, 0.1, 0.2])})
    assert list(redock_items(plain)) == ["pose"] and list(redock_items(out)) == ["pose", "distogram_nll"]
    assert "potential" in driver.DISTOGRAM_KEYS and "nll_interface" in driver.DISTOGRAM_KEYS
