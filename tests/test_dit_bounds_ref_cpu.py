"""The float64 statement of pd_dit_bounds (tests/dit_bounds_ref.py) is right, and its inputs can fail for the reasons they were
chosen for.  CPU only.

* the bounds are sound: nothing the float64 DiT block reaches over the adversarial input family exceeds exact64 (no margins);
* they are not vacuous: on shift = 0 rows the adversary reaches 0.95 of the v bound and sqrt((C - 1) / C) 0.999 of the y bound;
* each single fault a kernel could have - gate column in place of w, |W . s| dropped, last k-chunk dropped, last row group
  dropped, (w1, s1) used for the h bound, o[3] / o[4] swapped - applied to the float64 reference, is separated from the true
  bound on some case by more than the GPU test's tolerance, or is broken by the adversary;
* the generators' own conditions: distinct rows, extremes in the last chunk / last group and in the rows around the 64-row slab
  boundaries, no cancellation in |W . s| that would make the kernel's 1.001 margin an unfair demand.
"""
import math

import pytest
import torch

import dit_bounds_ref as dr

CASE_IDS = sorted(dr.CASES)
FAULTS = ["gate column for w", "|W.s| dropped", "last k-chunk dropped", "last row group dropped", "(w1, s1) for the h bound",
          "o[3] / o[4] swapped"]


def test_reference_on_a_hand_computed_block():
    C, hidden = 2, 1
    tab = torch.tensor([[1.0, -2.0, 2.0, 0.5, 9.0, 9.0, 0.5, 0.0, 1.0, -3.0, 9.0, 9.0]])
    wstack = torch.tensor([[[1.0, 2.0], [3.0, -1.0], [2.0, 1.0], [0.0, -1.0]]])
    consts = torch.tensor([[11.0, 13.0, 17.0, 19.0]])
    ref, exact = dr.dit_bounds64(tab, consts, wstack, C, hidden)
    r2 = math.sqrt(2.0)
    want = [11.0, 13.0, max(r2 * math.sqrt(5.0) + 3.0, r2 * math.sqrt(36.25) + 5.0), r2 * 2.0 + 2.0, r2 * 3.0 + 0.5,
            (r2 * math.sqrt(13.0) + 1.0) * (r2 * 3.0), 0.0, 0.0]
    assert exact.shape == (1, 1, 8)
    torch.testing.assert_close(exact[0, 0], torch.tensor(want, dtype=torch.float64), rtol=1e-14, atol=0)
    withm = [11.0, 13.0, dr.M1 * want[2], dr.M1 * r2 * 2.0 + 2.0, dr.M1 * r2 * 3.0 + 0.5, dr.M2 * want[5], 0.0, 0.0]
    torch.testing.assert_close(ref[0, 0], torch.tensor(withm, dtype=torch.float64), rtol=1e-14, atol=0)
    assert 1.001 - 1e-7 < dr.M1 < 1.001 + 1e-7 and 1.002 - 1e-7 < dr.M2 < 1.002 + 1e-7
    r32 = dr.dit_bounds32(tab, consts, wstack, C, hidden)
    assert r32.dtype == torch.float32
    torch.testing.assert_close(r32.double(), ref, rtol=1e-6, atol=0)


def test_layer_norm_of_a_one_hot_reaches_the_coordinate_limit():
    for C in (32, 40, 512):
        x = torch.zeros(C)
        x[C - 3] = 1.0
        xh = dr.layer_norm64(x)
        assert abs(float(xh[C - 3]) - math.sqrt(C - 1)) <= 1e-12 * math.sqrt(C)
        assert abs(float(xh.norm()) - math.sqrt(C)) <= 1e-12 * math.sqrt(C) and abs(float(xh.sum())) <= 1e-10


@pytest.mark.parametrize("case", CASE_IDS)
def test_adversary_never_exceeds_the_exact_bounds(case):
    _, exact64, _ = dr.case_reference(case)
    adv = dr.case_adversary(case)
    ratio = adv / exact64[..., 2:6]
    print(f"case {case}: worst achieved / exact bound  v {float(ratio[..., 0].max()):.4f}  y {float(ratio[..., 1].max()):.4f}  "
          f"y' {float(ratio[..., 2].max()):.4f}  h {float(ratio[..., 3].max()):.4f}")
    assert (adv <= exact64[..., 2:6] * (1 + 1e-12)).all(), float(ratio.max())


@pytest.mark.parametrize("case", CASE_IDS)
def test_reference_is_not_vacuous_on_shift0_rows(case):
    c = dr.bounds_case(case)
    _, exact64, _ = dr.case_reference(case)
    adv = dr.case_adversary(case)
    zero = c["kinds"] == dr.SHIFT0
    assert zero.any()
    C = c["C"]
    assert (adv[..., 0][zero] >= 0.95 * exact64[..., 2][zero]).all(), float((adv[..., 0] / exact64[..., 2])[zero].min())
    need = math.sqrt((C - 1) / C) * 0.999
    assert (adv[..., 1][zero] >= need * exact64[..., 3][zero]).all(), float((adv[..., 1] / exact64[..., 3])[zero].min())
    assert (adv[..., 2][zero] >= need * exact64[..., 4][zero]).all(), float((adv[..., 2] / exact64[..., 4])[zero].min())


# ------------------------------------------------------------------ single faults
def faulty_bounds(case, fault):
    """the float64 bounds (with margins) a kernel with one fault would produce"""
    c = dr.bounds_case(case)
    tab, consts, W, C, H, nb = c["tab"], c["consts"], c["wstack"], c["C"], c["hidden"], c["nblocks"]
    true = dr.case_reference(case)[0]

    def run(tab=tab, W=W):
        return dr.dit_bounds64(tab, consts, W, C, H)[0]

    def col(b, i):
        return slice((6 * b + i) * C, (6 * b + i + 1) * C)

    f = true.clone()
    if fault == "gate column for w":
        t = tab.clone()
        for b in range(nb):
            t[:, col(b, 1)], t[:, col(b, 4)] = tab[:, col(b, 2)], tab[:, col(b, 5)]
        f = run(tab=t)
    elif fault == "|W.s| dropped":
        t = tab.clone()
        for b in range(nb):
            t[:, col(b, 0)] = 0.0
            t[:, col(b, 3)] = 0.0
        g = run(tab=t)
        f[..., 2], f[..., 5] = g[..., 2], g[..., 5]
    elif fault == "last k-chunk dropped":
        Wm = W.clone()
        Wm[:, :, dr.last_group_start(C):] = 0.0
        f = run(W=Wm)
    elif fault == "last row group dropped":
        Wm = W.clone()
        Wm[:, dr.last_group_start(C):C] = 0.0
        Wm[:, C + dr.last_group_start(H):C + H] = 0.0
        Wm[:, C + H + dr.last_group_start(H):] = 0.0
        f = run(W=Wm)
    elif fault == "(w1, s1) for the h bound":
        t = tab.clone()
        for b in range(nb):
            t[:, col(b, 3)], t[:, col(b, 4)] = tab[:, col(b, 0)], tab[:, col(b, 1)]
        f[..., 5] = run(tab=t)[..., 5]
    elif fault == "o[3] / o[4] swapped":
        f[..., 3], f[..., 4] = true[..., 4], true[..., 3]
    else:
        raise KeyError(fault)
    return f


def separating_cases(fault):
    """per case: (some element differs from the true bound by more than the parity tolerance, the adversary exceeds the faulty bound)"""
    found = {}
    for case in CASE_IDS:
        ref64, _, ref32 = dr.case_reference(case)
        tol, _ = dr.parity_tolerance(ref32, ref64)
        f = faulty_bounds(case, fault)
        by_parity = bool(((f - ref64)[..., 2:6].abs() > tol).any())
        by_adversary = bool((dr.case_adversary(case) > f[..., 2:6]).any())
        if by_parity or by_adversary:
            found[case] = (by_parity, by_adversary)
    return found


@pytest.mark.parametrize("fault", FAULTS)
def test_each_single_fault_is_separated_by_some_case(fault):
    found = separating_cases(fault)
    print(f"fault '{fault}': " + ", ".join(f"case {k} ({'parity' if p else ''}{'+' if p and a else ''}{'adversary' if a else ''})"
                                          for k, (p, a) in found.items()))
    assert found, fault
    # the entries a fault leaves alone are the true ones: the check above cannot pass through an unrelated change
    for case in CASE_IDS:
        f, true = faulty_bounds(case, fault), dr.case_reference(case)[0]
        assert torch.equal(f[..., :2], true[..., :2]) and torch.equal(f[..., 6:], true[..., 6:])


def test_the_unfaulted_reference_is_not_separated_from_itself():
    for case in CASE_IDS:
        ref64, exact64, ref32 = dr.case_reference(case)
        tol, E = dr.parity_tolerance(ref32, ref64)
        assert tol.shape == ref64.shape[:2] + (1,) and (tol > 0).all()
        assert ((ref32.double() - ref64)[..., 2:6].abs() <= tol).all()
        assert (dr.case_adversary(case) <= ref64[..., 2:6]).all()
        assert (ref64[..., 2:6] > exact64[..., 2:6]).all()


# ------------------------------------------------------------------ the generators' own conditions
def test_special_rows():
    assert dr.special_rows(1) == [0]
    assert dr.special_rows(3) == [0, 2]
    assert dr.special_rows(64) == [0, 63]
    assert dr.special_rows(65) == [0, 63, 64]
    assert dr.special_rows(130) == [0, 63, 64, 65, 127, 128, 129]


def test_shapes_are_the_issue_s():
    want = {1: (32, 128, 2, 1, 0), 2: (40, 72, 3, 65, 7), 3: (64, 32, 1, 130, 0), 4: (128, 384, 2, 64, 0), 5: (512, 1408, 1, 3, 0)}
    for case, (C, H, nb, nrows, pad) in want.items():
        c = dr.bounds_case(case)
        assert (c["C"], c["hidden"], c["nblocks"], c["nrows"], c["ld"]) == (C, H, nb, nrows, 6 * C * nb + pad)
        assert c["tab"].shape == (nrows, c["ld"]) and c["wstack"].shape == (nb, C + 2 * H, C) and c["consts"].shape == (nb, 4)
        assert c["tab"].dtype == c["wstack"].dtype == c["consts"].dtype == torch.float32
    kinds = torch.cat([dr.bounds_case(k)["kinds"].flatten() for k in CASE_IDS])
    assert set(kinds.tolist()) == {dr.ORDINARY, dr.SHIFT0, dr.OUTLIER}


@pytest.mark.parametrize("case", CASE_IDS)
def test_generator_conditions(case):
    c = dr.bounds_case(case)
    tab, W, C, H, nb, nrows, kinds = c["tab"], c["wstack"], c["C"], c["hidden"], c["nblocks"], c["nrows"], c["kinds"]
    live = tab[:, :6 * C * nb]
    assert torch.isfinite(live).all() and torch.isfinite(W).all()
    assert torch.isnan(tab[:, 6 * C * nb:]).all() and (case != 2 or tab.shape[1] - 6 * C * nb == 7)
    # every table row differs, in every block and in each of the four vectors the kernel reads (SHIFT0 rows: in both gains)
    for b in range(nb):
        vec = dr.split_table(tab, b, C)
        for i in (1, 4):
            assert torch.unique(vec[i], dim=0).shape[0] == nrows
        nz = kinds[:, b] != dr.SHIFT0
        for i in (0, 3):
            assert torch.unique(vec[i][nz], dim=0).shape[0] == int(nz.sum())
            assert (vec[i][~nz] == 0).all() and (vec[i][nz].abs().amax(1) > 0).all()
        # the gates look nothing like the gains
        assert ((vec[2] - vec[1]).abs().amax(1) > 1).all() and ((vec[5] - vec[4]).abs().amax(1) > 1).all()
    # kinds: the special rows carry the outliers, one block each
    assert c["special"] == dr.special_rows(nrows)
    assert sorted((kinds == dr.OUTLIER).nonzero()[:, 0].tolist()) == c["special"]
    assert ((kinds == dr.OUTLIER).sum(1) <= 1).all()
    assert (kinds == dr.SHIFT0).any()
    # the outlier gains sit in the last k-chunk, the outlier weight rows in the last group of 32, and the maxima are really there
    k_last, nv_last, nh_last = dr.last_group_start(C), dr.last_group_start(C), dr.last_group_start(H)
    assert k_last <= c["k1"] < C and k_last <= c["k2"] < C and c["k1"] != c["k2"]
    assert nv_last <= c["nv"] < C and nh_last <= c["nh"] < H
    if case == 2:
        assert C % 32 != 0 and H % 32 != 0 and C < H          # a partial chunk and partial groups
    if case == 3:
        assert H < C
    _, exact64, _ = dr.case_reference(case)
    for b in range(nb):
        s1, w1, _, s2, w2, _ = (t.double() for t in dr.split_table(tab, b, C))
        Wv, W1, W3 = (t.double() for t in dr.split_weights(W, b, C, H))
        out = kinds[:, b] == dr.OUTLIER
        assert (w1[out].abs().argmax(1) == c["k1"]).all() and (w2[out].abs().argmax(1) == c["k2"]).all()
        Rv, Rh = dr.row_bound(Wv, w1, s1, C), dr.row_bound(W1, w2, s2, C) * dr.row_bound(W3, w2, s2, C)
        if b % 2 == 0:
            assert (Rv.argmax(1) == c["nv"]).all() and (Rh.argmax(1) == c["nh"]).all()
        # without the last chunk / the last group the maxima are smaller in every row: a guard bug there cannot hide
        Wc = W[b].double().clone()
        Wc[:, k_last:] = 0.0
        assert (dr.row_bound(Wc[:C], w1, s1, C).amax(1) < Rv.amax(1)).all()
        if b % 2 == 0:                                   # (a single group of rows: nothing is left without it)
            assert nv_last == 0 or (Rv[:, :nv_last].amax(1) < Rv.amax(1)).all()
            assert nh_last == 0 or (Rh[:, :nh_last].amax(1) < Rh.amax(1)).all()
        # rows 0, last and around the slab boundaries hold the extreme values of their block
        if out.any() and (~out).any():
            for j in (2, 3, 4, 5):
                assert exact64[out, b, j].min() > exact64[~out, b, j].max(), (b, j)
        # no cancellation pathology: fp32 |W_n . s| within 1e-4 R of the float64 value on every weight row
        for Wm, w, s in ((Wv, w1, s1), (W1, w2, s2), (W3, w2, s2)):
            d32 = (s.float() @ Wm.float().T).abs().double()
            d64 = (s @ Wm.T).abs()
            assert ((d32 - d64).abs() < 1e-4 * dr.row_bound(Wm, w, s, C)).all()


def test_cases_are_cached_and_deterministic():
    a = dr.bounds_case(2)
    assert dr.bounds_case(2) is a
    dr.bounds_case.cache_clear()
    b = dr.bounds_case(2)
    assert torch.equal(torch.nan_to_num(a["tab"]), torch.nan_to_num(b["tab"])) and torch.equal(a["wstack"], b["wstack"])
