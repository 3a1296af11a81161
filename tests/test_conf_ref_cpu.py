"""tests/conf_ref.py and tests/conf_cases.py without a GPU: the generalised references agree with the g17 / g18 fixtures through the
restatements of tests/test_confidence_loss_cpu.py and tests/test_metrics_cpu.py, every case holds its margins and contains the
rows its line in the docstring of conf_cases promises, and a reference with the fault a case was chosen for differs from the
right one by more than the bar tests/test_conf_kernels_gpu.py applies (or in an exact decision)."""
import numpy as np
import pytest

import conf_cases as cc
import conf_ref as cr
import test_confidence_loss_cpu as g17
import test_metrics_cpu as g18


# ------------------------------------------------------------------ the references against the fixtures
@pytest.mark.parametrize("name", g17.CONF_CASES)
def test_references_agree_with_the_g17_restatement(name):
    g = g17.load_conf(name)
    theirs, lddt = g17.restate(g)
    c = g["token_id_to_centre_atom_id"]
    poly = (g["is_ligand"] == 0).astype(np.float64)
    mine = cr.lddt(g["x_pred"], g["x_gt"], c, g["is_dna"], g["is_rna"], poly)[0]
    assert mine.dtype == np.float32 and np.array_equal(mine, lddt, equal_nan=True) and np.array_equal(mine, g["ref_lddt"], equal_nan=True)
    ex = g["x_exists"].astype(np.float64)
    bins = {"plddt": cr.plddt_bins(mine[0], 50)}
    masks = {"plddt": ex, "pde": np.outer(ex[c], ex[c]).reshape(-1), "pae": np.outer(ex[c], ex[c]).reshape(-1)}
    ids = [g[f"token_id_to_frame_atom_id_{k}"] for k in range(3)]
    fp, fg = cr.frames(g["x_pred"][0], ids)[0], cr.frames(g["x_gt"], ids)[0]
    bins["pde"] = cr.pair_bins(cr.pde_error(g["x_pred"][0], g["x_gt"], c), **g17.SETTINGS["pde"]).reshape(-1)
    bins["pae"] = cr.pair_bins(cr.pae_error(g["x_pred"][0], g["x_gt"], c, fp, fg), **g17.SETTINGS["pae"]).reshape(-1)
    for t in g17.TERMS:
        assert np.array_equal(bins[t], theirs[t][1].reshape(-1)) and np.array_equal(bins[t], g["bins_" + t].reshape(-1).astype(np.int64)), t
        p = g[g17.LOGITS[t]]
        loss, rows, grad = cr.ce(p.reshape(-1, p.shape[-1]), bins[t], masks[t])
        assert abs(loss - theirs[t][0]) <= 1e-12 * abs(loss) and abs(loss - float(g["f64_" + t])) <= 1e-10 * abs(loss), t
        np.testing.assert_allclose(grad[g["grow_" + t]], g["g64_" + t], rtol=1e-10, atol=1e-18)
        assert abs(rows @ masks[t] / (1e-9 + masks[t].sum()) - loss) <= 1e-12 * abs(loss)


@pytest.mark.parametrize("name", g18.METRICS_CASES)
def test_references_agree_with_the_g18_restatement(name):
    g = g18.load_metrics(name)
    theirs = g18.restate(g)
    pl, pa = (g[k] if g["p_pae"].ndim == 4 else g[k][None] for k in ("p_plddt", "p_pae"))
    atom, mean = cr.plddt(pl)
    tm = cr.pae_tm(pa, g18.centres(64), g["s_mask"], g["asym_id"])
    for k, v in (("atom_plddts", atom), ("mean_plddt", mean), ("pae", tm["pae"]), ("ptm", tm["ptm"]), ("iptm", tm["iptm"])):
        assert v.shape == theirs[k].shape and np.abs(v - theirs[k]).max() <= 1e-12 * np.abs(v).max() + 1e-300, k
    assert np.array_equal(tm["rows"], theirs["rows"]) and np.array_equal(tm["rows"], g["f64_rows"])
    np.testing.assert_allclose(tm["gaps"], g["f64_gaps"], atol=1e-9)
    a2t = g["atom_id_to_token_id"]
    uniq, chain = np.unique(g["asym_id"][a2t], return_inverse=True)
    counts, has, has_skip, closest = cr.clash(g["x_pred"], g["a_mask"], chain, (g["is_ligand"] == 0)[a2t], len(uniq))
    assert np.array_equal(has, theirs["has_clash"]) and np.array_equal(has_skip, theirs["has_clash_skip"]) and closest > 1e-4
    rank = cr.ranking(tm["ptm"], tm["iptm"], has[:len(tm["ptm"])])
    assert np.abs(rank - theirs["ranking_confidence"]).max() <= 1e-12
    if "n_clash" in g:
        live = np.nonzero(counts[0].diagonal())[0]                  # the chains with eligible atoms: each atom counts itself
        assert np.array_equal(counts[:, live][:, :, live], g["n_clash"])


# ------------------------------------------------------------------ margins and contents
@pytest.mark.parametrize("name", cc.LDDT)
def test_lddt_cases(name):
    c, ref = cc.lddt(name), cc.lddt_ref(name)
    B, A, T = cc.LDDT[name]
    assert c.x_pred.shape == (B, A, 3) and c.x_gt.shape == (A, 3) and c.centre.shape == (T,) and ref.shape == (B, A)
    assert c.closest["d_gt"] >= cc.MARGIN and c.closest["d_lm"] >= cc.MARGIN and c.is_polymer[-1] == 1
    # the fp32 evaluation takes the same decisions: the same bits
    num32, den32 = g17.lddt_sums(c.x_pred, c.x_gt, c.is_dna, c.is_rna, c.is_polymer, c.centre)
    assert np.array_equal(g17.lddt_bin(num32, den32, 1)[0], ref, equal_nan=True)
    if name == "mixed":
        assert c.is_dna.sum() and c.is_rna.sum() and (c.is_polymer == 0).sum()
        assert np.isnan(ref[:, c.far[0]]).all() and np.isnan(ref).sum() == B
        d_gt = cr.norm(c.x_gt.astype(np.float64)[:, None] - c.x_gt.astype(np.float64)[c.centre][None])
        nuc = (c.is_dna + c.is_rna) > 0
        assert ((d_gt[:, nuc] > 15) & (d_gt[:, nuc] < 30)).any()    # the 30 A cut includes what the 15 A cut would not
    else:
        assert not np.isnan(ref).any()
    if name == "1":
        assert (ref == 1.0).all()
    if name == "256":
        assert sorted(c.centre.tolist()) == list(range(256))
    if T > 1:
        live = ref[~np.isnan(ref)]
        assert len(np.unique(live)) > 50 and live.max() - live.min() > 0.3 and live.max() < 1


@pytest.mark.parametrize("T", cc.FRAMES)
def test_frames_cases(T):
    c = cc.frames(T)
    f64, f32 = cc.frames_ref(T)
    assert f64.shape == (T, 13) and np.isfinite(f64).all() and np.isfinite(f32).all()
    assert c.closest["cos"] >= cc.COS_MARGIN and c.closest["bisector"] >= cc.MIN_BISECTOR
    assert np.array_equal(f64[:, 12], f32[:, 12]) and np.array_equal(f32[:, 9:12], c.x[c.ids[1]])
    if T > 1:
        assert c.ids[0][1] == c.ids[1][1] != c.ids[2][1] and f64[1, 12] == 1 and not f64[1, 6:9].any()     # a = b: w1 = 0, e1 = e2
        assert (f64[:, 12] == 0).sum() >= T // 8 and (f64[:, 12] == 1).sum() >= T // 2
    if T > 256:
        assert np.abs(f64[256:, :9]).max() > 0.5
    if T == 600:
        assert (f64[256:, 12] == 0).any() and (f64[256:, 12] == 1).any()


@pytest.mark.parametrize("A,nb", cc.PLDDT_LOSS)
def test_plddt_loss_cases(A, nb):
    c = cc.plddt_loss(A, nb)
    assert c.logits.shape == (A, nb) and c.bins.min() >= 0 and c.bins.max() <= nb - 1
    if A >= 15:
        assert np.isnan(c.lddt[[0, 4]]).all() and c.bins[0] == 0 and c.lddt[1] == 1.0 and c.bins[1] == nb - 1
        assert c.x_exists[2] == 0 == c.x_exists[4] and c.x_exists.sum() == A - 2 and np.abs(c.logits[5]).max() > 16
        assert c.bins[3] == int(np.float32(0.6) * np.float32(nb))
        if nb > 1:
            assert len(np.unique(c.bins)) >= min(nb, A) // 3
    (loss, rows, g), _ = cc.plddt_loss_ref(A, nb)
    assert (loss == 0.0 and not g.any()) if nb == 1 else (loss > 0 and not g[c.x_exists == 0].any())


@pytest.mark.parametrize("name", cc.PAIRS)
def test_pairs_cases(name):
    c = cc.pairs(name)
    T, nb, lo, hi = cc.PAIRS[name]
    assert c.logits["pde"].shape == (T, T, nb) and c.frames_pred.shape == (T, 13) and c.frames_pred.dtype == np.float32
    vp, vg = c.frames_pred[:, 12], c.frames_gt[:, 12]
    for m in cc.MODES:
        e, e32 = c.errors[m], cc.pair_errors(c, np.float32)[m]
        assert c.closest[m] >= cc.MARGIN and np.abs(e32 - e).max() < 0.2 * cc.MARGIN
        assert np.array_equal(cr.pair_bins(e32.astype(np.float64), lo, hi, nb), c.bins[m])          # fp32 decides the same
        below, above = int((e < lo).sum()), int((e > hi).sum())
        print(f"pairs {name} {m}: {below} errors below min_bin {lo}, {above} above max_bin {hi}, {len(np.unique(c.bins[m]))} bins of {nb} in use")
        if T >= 8:
            assert above >= 2 and (c.bins[m] == nb - 1).sum() >= above
            assert below >= (2 if lo > 0 else 0) and (c.bins[m] == 0).sum() >= below
        if T >= 9 and nb > 1:
            assert len(np.unique(c.bins[m])) >= min(nb // 3, T)
    if T >= 8:
        assert ((vp == 0) & (vg == 1)).sum() >= 1 and ((vp == 1) & (vg == 0)).sum() >= 1 and ((vp == 1) & (vg == 1)).sum() >= 2
        assert not c.errors["pae"][(vp == 0) | (vg == 0)].any()
        assert (c.mask == 0).sum() == 2 * T - 1 and c.x_exists[c.centre].sum() == T - 1
    if name == "9x33":
        assert lo == 2.0 and hi == 30.0 and nb % 2 == 1


@pytest.mark.parametrize("P,A,nb", cc.PLDDT)
def test_metrics_plddt_cases(P, A, nb):
    c = cc.plddt(P, A, nb)
    (atom, mean), (atom32, _) = cc.plddt_ref(P, A, nb)
    assert c.logits.shape == (P, A, nb) and atom.shape == (P, A) and mean.shape == (P,)
    assert atom.min() > 0 and atom.max() < 100 and (atom.max() - atom.min() > 20 or A == 1)
    assert (nb % 4 == 0 and 4 * 15 >= nb) == (nb == 48)             # the vector path with idle lanes


@pytest.mark.parametrize("name", cc.PAE_TM)
def test_pae_tm_cases(name):
    c = cc.pae_tm(name)
    P, T, nb = cc.PAE_TM[name]
    r64, r32 = cc.pae_tm_ref(name)
    assert c.logits.shape == (P, T, T, nb) and c.logits.dtype == np.float32 and c.centres.shape == (nb,)
    assert c.geometry == cc.PAE_TM_GEOMETRY[name], (name, c.geometry)
    assert r64["gaps"].min() >= cc.GAP_MARGIN and np.array_equal(r64["rows"], r32["rows"])
    assert r64["rows"][:, 0].tolist() == c.best == r64["rows"][:, 1].tolist()
    assert len(np.unique(c.asym)) == 3 and (c.weights == 0).sum() >= 1 and c.weights[T - 1] == 1
    s = float(c.weights.astype(np.float64).sum())
    assert abs(s - round(s)) >= cc.SUM_MARGIN or s == round(s)
    if name == "2x40x48":
        assert (c.weights % 1 != 0).sum() >= 5 and s != round(s)
    if name == "1x17x7":
        assert s < 19
    if name == "8x257x64":
        assert np.array_equal(c.logits[cc.SLICE], cc.pae_tm("1x257x64").logits[0])
        assert {0, 256} <= set(c.best) and cc.tm_split(64, 256) == (1, 256, 4) and cc.tm_split(1, 512)[0] == 4


def test_tm_split_rule_on_the_fixture_shapes():
    """every g18 shape gives chunks of 64: the iteration loop of pae_tm_kernel runs once per wave there"""
    assert [cc.tm_split(P, T)[1:] for P, T in ((1, 107), (3, 221), (1, 24), (1, 18))] == [(64, 1)] * 4
    assert cc.tm_split(1, 107)[0] == 2 and cc.tm_split(3, 221)[0] == 4


@pytest.mark.parametrize("rows,T", (((0, 256), 257), ((200, 256), 257), ((3, 259), 260)))
def test_tie_cases(rows, T):
    c = cc.tie(*rows, T=T)
    r = cr.pae_tm(c.logits, c.centres, c.weights, c.asym)
    for q in range(2):
        sel = r["per_alignment"][0, q] * c.weights
        assert sel[rows[0]] == sel[rows[1]] == sel.max() and (sel == sel.max()).sum() == 2 and r["rows"][0, q] == rows[0]
        assert np.sort(sel)[-3] < sel.max() - cc.GAP_MARGIN
    assert np.array_equal(c.logits[0, rows[0]], c.logits[0, rows[1]]) and c.asym[rows[0]] == c.asym[rows[1]] and c.weights[list(rows)].tolist() == [1, 1]
    assert rows[0] % 256 == rows[1] % 256 or rows[1] >= 256 > rows[0]        # one lane's two rows, or a one-row lane against a second row


@pytest.mark.parametrize("name", cc.CLASH)
def test_clash_cases(name):
    c = cc.clash(name)
    B, A, nc = cc.CLASH[name]
    counts, has, has_skip, closest = cc.clash_ref(name)
    assert c.x_pred.shape == (B, A, 3) and counts.shape == (B, nc, nc) and closest >= cc.MARGIN
    print(f"clash {name}: close ordered pairs per pose {counts.sum((1, 2)).tolist()}, has_clash {has.tolist()}, a < c only {has_skip.tolist()}")
    if A == 1:
        assert counts.tolist() == [[[1]]] and has.tolist() == has_skip.tolist() == [0]
        return
    assert (c.chain == -1).sum() == 2 and (c.chain == nc).sum() == 2 and (c.a_mask == 0).sum() >= 10 and (c.a_mask == 0.5).sum() == 1
    assert (c.polymer == 0).sum() >= 10 and (counts * (1 - np.eye(nc, dtype=np.int64))).sum((1, 2)).min() > 0
    assert np.array_equal(counts, counts.transpose(0, 2, 1)) and has.tolist() == [1] * B       # three or more chains: a middle chain against itself
    assert set(has_skip.tolist()) == {0, 1}
    # the excluded atoms are close to others: a kernel that counted them would differ
    every = cr.clash(c.x_pred, np.ones(A), np.clip(c.chain, 0, nc - 1), np.ones(A), nc)[0]
    assert (every.sum((1, 2)) > counts.sum((1, 2))).all()


# ------------------------------------------------------------------ sensitivity: the faults the cases were chosen for
@pytest.mark.parametrize("name", ("257", "513"))
def test_lddt_without_the_tokens_past_256_differs(name):
    c, ref = cc.lddt(name), cc.lddt_ref(name)
    for keep in (256, c.T - 1):                                     # the second round dropped; the partial last round dropped
        wrong = cr.lddt(c.x_pred, c.x_gt, c.centre[:keep], c.is_dna[:keep], c.is_rna[:keep], c.is_polymer[:keep])[0]
        differ = ~np.isclose(wrong, ref, rtol=0, atol=0, equal_nan=True)
        print(f"lddt {name}: tokens >= {keep} dropped, {differ.sum()} of {ref.size} values change")
        assert differ.sum() >= 10


@pytest.mark.parametrize("T", (257, 600))
def test_frames_left_at_zero_past_256_differ(T):
    c = cc.frames(T)
    f64, f32 = cc.frames_ref(T)
    wrong = cr.frames_zero_past(c.x, c.ids)
    assert np.abs(wrong[:, :9] - f64[:, :9]).max() > 100 * cr.bar(f32[:, :9], f64[:, :9])[1]
    assert not np.array_equal(wrong[256:, 12], f64[256:, 12]) or T == 257
    assert not np.array_equal(wrong[:, 9:12], f64[:, 9:12])


@pytest.mark.parametrize("name", ("32x65x64", "8x257x64"))
def test_ptm_without_the_pairs_past_64_of_a_chunk_differs(name):
    c = cc.pae_tm(name)
    r64, r32 = cc.pae_tm_ref(name)
    keep = (np.arange(c.T) % c.geometry[1]) < 64
    wrong = cr.pae_tm(c.logits[:2], c.centres, c.weights, c.asym, keep=keep)
    for k in ("ptm", "iptm", "per_alignment"):
        bar = cr.bar(r32[k], r64[k])[1]
        diff = np.abs(wrong[k] - r64[k][:2]).reshape(2, -1).max(-1).min()
        print(f"{name} {k}: dropping j >= 64 of a chunk moves it by {diff:.3e}, bar {bar:.3e}")
        assert diff > 100 * bar, (name, k)


@pytest.mark.parametrize("rows,T", (((0, 256), 257), ((200, 256), 257), ((3, 259), 260)))
def test_last_maximum_rule_differs(rows, T):
    c = cc.tie(*rows, T=T)
    wrong = cr.pae_tm(c.logits, c.centres, c.weights, c.asym, tie="last")
    assert wrong["rows"].tolist() == [[rows[1], rows[1]]]


def test_softmax_over_64_lanes_with_zeros_differs():
    for A, nb in ((15, 1), (16, 37), (65, 50)):
        c = cc.plddt_loss(A, nb)
        (loss, _, g), _ = cc.plddt_loss_ref(A, nb)
        wl, _, wg = cr.ce(c.logits, c.bins, c.x_exists, lanes=64)
        print(f"plddt loss {A}x{nb}: zeros for -inf move the loss by {abs(wl - loss):.3e} (bar {cc.TOL * abs(loss):.3e})")
        assert abs(wl - loss) > 100 * cc.TOL * abs(loss) and (nb == 1 or np.abs(wg - g).max() > 100 * cc.TOL * np.abs(g).max())
    for name in ("8x1", "9x33"):
        c = cc.pairs(name)
        for m in cc.MODES:
            loss = cc.pairs_ref(name, m)[0][0]
            wl = cr.ce(c.logits[m].reshape(-1, c.nb), c.bins[m].reshape(-1), c.mask.reshape(-1), lanes=64)[0]
            assert abs(wl - loss) > 100 * cc.TOL * abs(loss)
    for shape in ((3, 61, 48), (1, 64, 7), (2, 257, 50)):           # the idle lanes of metrics.hip
        c = cc.plddt(*shape)
        (atom, mean), (atom32, mean32) = cc.plddt_ref(*shape)
        wa, wm = cr.plddt(c.logits, lanes=64)
        assert np.abs(wa - atom).max() > 100 * cr.bar(atom32, atom)[1] and np.abs(wm - mean).min() > 100 * cr.bar(mean32, mean)[1]


def test_ignoring_min_bin_differs():
    c = cc.pairs("9x33")
    for m in cc.MODES:
        wrong = cr.pair_bins(c.errors[m], c.min_bin, c.max_bin, c.nb, use_min_bin=False)
        n = int((wrong != c.bins[m]).sum())
        print(f"pairs 9x33 {m}: {n} of {wrong.size} bins change when min_bin is ignored")
        assert n >= c.T
