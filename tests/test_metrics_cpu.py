"""get_metrics (physdock_amd/metrics.py, csrc/metrics.hip), the parts that need no GPU: the committed fixtures
(tests/golden/g18_metrics_*.npz, tools/make_golden_metrics.py) are pinned to the formulas by an independent float64 restatement
written here from the reference's code (PhysDock/data/tools/get_metrics.py), their margins hold, the C ABI has the new entry
points and the public interface is in place."""
import inspect
import os
import re

import numpy as np
import pytest

from physdock_amd.synthetic import metrics_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METRICS_CASES = ("small", "frac", "onechain", "chains3", "clash", "mid")
QUANTITIES = ("atom_plddts", "mean_plddt", "pae", "ptm", "iptm", "ranking_confidence")
NEW_SYMBOLS = ("pd_metrics_workspace_numel", "pd_metrics_plddt", "pd_metrics_pae_tm", "pd_metrics_clash")
FEAT_KEYS = ("s_mask", "asym_id", "a_mask", "atom_id_to_token_id", "is_ligand")
MAX_BYTES = 288475                  # the largest g17_* fixture
_cache = {}


def load_metrics(name):
    """fixture + inputs as numpy arrays; the logits are rebuilt from the integer hash and checked against the stored checksums.
    Loaded once per session and shared (read-only)."""
    if name not in _cache:
        g = dict(np.load(os.path.join(GOLDEN, f"g18_metrics_{name}.npz")))
        o, f, _ = metrics_case(str(g["case"]), stored=g)
        for k in ("p_plddt", "p_pae"):
            v = o[k].numpy().astype(np.float64)
            np.testing.assert_allclose([v.sum(), (v ** 2).sum()], g["checksum_" + k], rtol=1e-13, err_msg=k)
            g[k] = o[k].numpy()
        for k in FEAT_KEYS:
            assert k in g, k
        _cache[name] = g
    return _cache[name]


def bound(g, q):
    """the tolerance of a quantity: max(4 e32, 8 ulp32 of its scale)"""
    return max(4 * float(g["e32_" + q]), 8 * float(np.spacing(np.float32(np.abs(g["f64_" + q]).max()))))


# ------------------------------------------------------------------ float64 restatement of the reference's functions
def softmax(l):
    e = np.exp(l - l.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def centres(nb, max_bin=32.0):
    """_calculate_bin_centers on get_metrics' torch.linspace(0, 32, 63), with its fp32 operations"""
    import torch
    breaks = torch.linspace(0., max_bin, nb - 1).numpy()
    step = breaks[1] - breaks[0]
    c = breaks + step / 2
    return np.concatenate([c, [c[-1] + step]], axis=0).astype(np.float64)


def tm_score(logits, w, asym, interface):
    """predicted_tm_score: (value, row, top-two gap of per_alignment * w)"""
    c = centres(logits.shape[-1])
    d0 = 1.24 * (max(int(np.sum(w)), 19) - 15) ** (1. / 3) - 1.8
    term = (softmax(logits) * (1. / (1 + np.square(c) / np.square(d0)))).sum(-1)
    mask = np.ones_like(term)
    if interface:
        mask = mask * (asym[:, None] != asym[None, :])
    term = term * mask
    pw = mask * (w[None, :] * w[:, None])
    per = (term * (pw / (1e-8 + pw.sum(-1, keepdims=True)))).sum(-1)
    sel = np.sort(per * w)
    return per[(per * w).argmax()], int((per * w).argmax()), sel[-1] - sel[-2]


def has_clash(x, mask, asym_atom, poly, self_pairs=True):
    """get_has_clash; self_pairs=False restricts the reference's loop to a < b"""
    flag = (mask == 1) & (poly == 1)
    x, asym_atom = x[flag].astype(np.float64), asym_atom[flag]
    uniq = np.unique(asym_atom)
    if len(uniq) == 1:
        return 0, np.inf
    closest = np.inf
    out = 0
    for a in uniq[:-1]:
        for b in uniq[1:]:
            if not self_pairs and not a < b:
                continue
            p1, p2 = x[asym_atom == a], x[asym_atom == b]
            d = np.sqrt(((p1[None] - p2[:, None]) ** 2).sum(-1))
            if a != b:
                closest = min(closest, np.abs(d - 1.1).min())
            n = (d < 1.1).sum()
            if n > 100 or n / min(len(p1), len(p2)) > 0.5:
                out = 1
    return out, closest


def restate(g):
    pl, pa = g["p_plddt"].astype(np.float64), g["p_pae"].astype(np.float64)
    if pa.ndim == 3:
        pl, pa = pl[None], pa[None]
    w, asym = g["s_mask"].astype(np.float64), g["asym_id"]
    nb = pl.shape[-1]
    atom = (softmax(pl) * np.arange(0.5 / nb, 1.0, 1.0 / nb)).sum(-1) * 100
    out = {"atom_plddts": atom, "mean_plddt": atom.mean(-1), "pae": (softmax(pa) * centres(pa.shape[-1])).sum(-1)}
    tm = [[tm_score(pa[p], w, asym, q) for q in (False, True)] for p in range(pa.shape[0])]
    out["ptm"], out["iptm"] = (np.asarray([t[q][0] for t in tm]) for q in (0, 1))
    out["rows"] = np.asarray([[t[q][1] for q in (0, 1)] for t in tm])
    out["gaps"] = np.asarray([[t[q][2] for q in (0, 1)] for t in tm])
    a2t = g["atom_id_to_token_id"]
    poly = (g["is_ligand"] == 0)[a2t]
    cl = [has_clash(x, g["a_mask"], asym[a2t], poly) for x in g["x_pred"]]
    out["has_clash"] = np.asarray([c[0] for c in cl])
    out["has_clash_skip"] = np.asarray([has_clash(x, g["a_mask"], asym[a2t], poly, self_pairs=False)[0] for x in g["x_pred"]])
    out["closest"] = min(c[1] for c in cl)
    out["ranking_confidence"] = 0.8 * out["iptm"] + 0.2 * out["ptm"] - out["has_clash"][:len(out["ptm"])]
    return out


def test_fixture_set_is_complete():
    shapes = {}
    for name in METRICS_CASES:
        path = os.path.join(GOLDEN, f"g18_metrics_{name}.npz")
        assert os.path.getsize(path) < MAX_BYTES
        g = np.load(path)
        for k in g.files:                                   # only data: numeric arrays and a short string
            assert g[k].dtype.kind in "fiubU", (k, g[k].dtype)
        for q in QUANTITIES:
            assert {"ref_" + q, "f64_" + q, "e32_" + q} <= set(g.files), (name, q)
        assert g["is_ligand"].dtype == np.bool_
        shapes[name] = (g["x_pred"].shape, g["s_mask"].shape[0], g["f64_ptm"].shape[0])
    assert shapes == {"small": ((3, 61, 3), 24, 1), "frac": ((3, 61, 3), 24, 1), "onechain": ((2, 61, 3), 24, 1),
                      "chains3": ((2, 63, 3), 18, 1), "clash": ((5, 450, 3), 107, 1), "mid": ((3, 1805, 3), 221, 3)}


@pytest.mark.parametrize("name", METRICS_CASES)
def test_float64_restatement_agrees_with_the_fixture(name):
    g = load_metrics(name)
    mine = restate(g)
    for q in QUANTITIES:
        v, f64, ref = mine[q], g["f64_" + q], g["ref_" + q]
        if q == "pae":
            np.testing.assert_allclose([v.sum(), (v ** 2).sum()], g["sum_f64_pae"], rtol=1e-12)
            v = v[:, g["pae_rows"]]
        assert v.shape == f64.shape == ref.shape, q
        scale = np.abs(f64).max()
        print(f"{name} {q}: max|f64| {scale:.6g} restated vs f64 {np.abs(v - f64).max():.3e} ref vs f64 {np.abs(ref - f64).max():.3e} "
              f"e32 {float(g['e32_' + q]):.3e} bound {bound(g, q):.3e}")
        assert np.abs(v - f64).max() <= 1e-9 * max(scale, 1e-30) + 1e-300, q
        assert np.abs(ref.astype(np.float64) - f64).max() <= bound(g, q), q        # the reference within its own tolerance
    # decisions and their margins
    assert np.array_equal(mine["rows"], g["f64_rows"])
    np.testing.assert_allclose(mine["gaps"], g["f64_gaps"], atol=1e-9)
    if name == "onechain":
        assert len(np.unique(g["asym_id"])) == 1 and (g["f64_iptm"] == 0).all() and (g["ref_iptm"] == 0).all() and (g["f64_rows"][:, 1] == 0).all()
        assert g["f64_gaps"][:, 0].min() >= 1e-4
    else:
        assert g["f64_gaps"].min() >= 1e-4
    assert np.array_equal(mine["has_clash"], g["ref_has_clash"]) and np.array_equal(mine["has_clash_skip"], g["f64_has_clash_skip"])
    assert mine["closest"] > 1e-4 and float(g["closest_clash"]) > 1e-4
    sw = float(g["s_mask"].astype(np.float64).sum())
    if name == "frac":
        assert (g["s_mask"] % 1 != 0).any() and (g["s_mask"] >= 0).all() and (g["s_mask"] <= 1).all() and abs(sw - round(sw)) >= 1e-3
    if name in ("small", "frac", "onechain"):
        assert (g["s_mask"] == 0).sum() >= 3 and sw < 19 and g["p_plddt"].shape == (61, 50) and 61 % 4       # the clip of d0
        assert (g["a_mask"] == 0).any()
    if name in ("small", "frac"):
        assert g["is_ligand"].any() and len(np.unique(g["asym_id"][~g["is_ligand"]])) == 2
    if name == "mid":
        assert g["p_pae"].shape == (3, 221, 221, 64) and g["p_plddt"].shape == (3, 1805, 50) and len(g["pae_rows"]) < 221
        assert len({tuple(r) for r in g["f64_rows"]}) == 3                           # the three logit sets decide differently


def test_chains3_documents_the_self_pair_quirk():
    g = load_metrics("chains3")
    poly_chains = np.unique(g["asym_id"][~g["is_ligand"]])
    assert len(poly_chains) == 3 and float(g["closest_clash"]) > 30             # three chains, tens of Angstrom apart
    assert g["n_clash"].shape == (2, 3, 3) and not (g["n_clash"] * (1 - np.eye(3, dtype=np.int64))).any()
    assert (g["n_clash"][:, 1, 1] == g["n_atoms"][1]).all()                     # the middle chain against itself: its N self-distances
    assert g["ref_has_clash"].tolist() == [1, 1] and g["f64_has_clash_skip"].tolist() == [0, 0]
    assert (g["ref_ranking_confidence"] < -0.9).all()


def test_clash_case_covers_each_rule():
    g = load_metrics("clash")
    a2t, asym = g["atom_id_to_token_id"], g["asym_id"]
    poly = (g["is_ligand"] == 0)[a2t]
    assert g["n_clash_pose"].tolist() == [0, 80, 101, 100, 0] and g["n_min_pose"].tolist() == [202, 150, 202, 200, 202]
    assert np.array_equal(g["a_mask_pose"][0], g["a_mask"]) and np.array_equal(g["a_mask_pose"][2], g["a_mask"])
    mine = [has_clash(g["x_pred"][b], g["a_mask_pose"][b], asym[a2t], poly)[0] for b in range(5)]
    assert mine == g["ref_has_clash_pose"].tolist() == [0, 1, 1, 0, 0] == g["f64_has_clash_pose_skip"].tolist()
    assert g["ref_has_clash"].tolist() == [0, 0, 1, 0, 0]
    for b in range(5):                                       # at least 202 eligible atoms per chain under the main mask
        el = (g["a_mask"] == 1) & poly
        assert min((asym[a2t][el] == c).sum() for c in (1, 2)) >= 202
    # pose 4: the overlapping atoms are masked or ligand atoms only
    x = g["x_pred"][4].astype(np.float64)
    d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    ca = asym[a2t]
    i, j = np.nonzero((d < 1.1) & (ca[:, None] != ca[None, :]))
    el = (g["a_mask"] == 1) & poly
    assert len(i) == 36 and not (el[i] & el[j]).any()


def test_abi_header_and_signatures_agree():
    from physdock_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "physdock_hip.h")).read()
    assert int(re.search(r"#define\s+PD_ABI_VERSION\s+(\d+)", hdr).group(1)) == 11 == _lib.ABI_VERSION
    assert set(NEW_SYMBOLS) <= set(_lib.header_symbols())
    src = open(os.path.join(_lib._HERE, "_lib.py")).read()
    for s in NEW_SYMBOLS:
        assert f'sig("{s}"' in src, s
        n_hdr = len(re.search(rf"int\s+{s}\s*\(([^;]*)\)\s*;", hdr).group(1).split(","))
        n_sig = len(re.search(rf'sig\("{s}",([^\n#]*)\)', src).group(1).split(","))
        assert n_hdr == n_sig, (s, n_hdr, n_sig)


def test_library_exports_the_metrics_symbols():
    from physdock_amd import _lib, build
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) and not os.path.exists(_lib.LIB_PATH):
        pytest.skip("hipcc not available")
    build.build(verbose=False)
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.SYMBOLS and hasattr(L, s)
    # the documented formula: 64 + 2 P T ceil(T / 16)
    assert L.pd_metrics_workspace_numel(1, 256) == 64 + 2 * 256 * 16
    assert L.pd_metrics_workspace_numel(3, 221) == 64 + 2 * 3 * 221 * 14
    assert L.pd_metrics_workspace_numel(0, 24) < 0 and L.pd_metrics_workspace_numel(1, 0) < 0


def test_public_interface_and_cpu_tensors_are_refused():
    import torch
    import physdock_amd
    from physdock_amd import metrics
    for n in ("get_metrics", "compute_plddt", "compute_predicted_aligned_error", "predicted_tm_score", "get_has_clash"):
        assert getattr(physdock_amd, n) is getattr(metrics, n) and n in metrics.__all__
    sp = inspect.signature(metrics.get_metrics).parameters
    assert list(sp)[:2] == ["output", "batch"] and sp["all_poses"].kind is sp["all_poses"].KEYWORD_ONLY and sp["all_poses"].default is False
    assert sp["skip_self_pairs"].kind is sp["skip_self_pairs"].KEYWORD_ONLY and sp["skip_self_pairs"].default is False
    sp = inspect.signature(metrics.predicted_tm_score).parameters
    assert list(sp) == ["logits", "residue_weights", "asym_id", "interface", "max_bin", "return_row"]
    assert (sp["interface"].default, sp["max_bin"].default, sp["return_row"].default) == (False, 32.0, False)
    assert list(inspect.signature(metrics.get_has_clash).parameters)[:4] == ["atom_pos", "atom_mask", "asym_id", "is_polymer_chain"]
    g = load_metrics("small")
    o = {k: torch.from_numpy(g[k]) for k in ("p_plddt", "p_pae", "x_pred")}
    f = {k: torch.from_numpy(g[k]) for k in FEAT_KEYS}
    msg = r"runs on an MI355X \(HIP\) device only"
    with pytest.raises(RuntimeError, match=msg):
        metrics.get_metrics(o, f)
    with pytest.raises(RuntimeError, match=msg):
        metrics.compute_plddt(o["p_plddt"])
    with pytest.raises(RuntimeError, match=msg):
        metrics.predicted_tm_score(o["p_pae"], f["s_mask"])
    with pytest.raises(RuntimeError, match=msg):
        metrics.get_has_clash(o["x_pred"][0], f["a_mask"], f["asym_id"][f["atom_id_to_token_id"]], ~f["is_ligand"][f["atom_id_to_token_id"]])
    # the device table of bin centres is built with the reference's own torch fp32 operations
    assert np.array_equal(metrics._centres_cpu(32.0, 64).numpy().astype(np.float64), centres(64))
