"""The confidence losses (cal_lddt, plddt_loss, pde_loss, pae_loss; physdock_amd/loss.py, csrc/confidence_loss.hip), the parts that
need no GPU: the committed fixtures (tests/golden/g17_conf_loss_*.npz, tools/make_golden_confidence_loss.py) are pinned to the
formulas by an independent float64 restatement written here from the reference's code (PhysDock/models/loss.py:184-207,320-532),
the C ABI has the new entry points, and the new kernels compile without scratch."""
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONF_CASES = ("small", "mid", "ragged", "empty")
TERMS = ("plddt", "pde", "pae")
LOGITS = {"plddt": "p_plddt", "pde": "p_pde", "pae": "p_pae"}
SETTINGS = {"plddt": {"no_bins": 50}, "pde": {"min_bin": 0, "max_bin": 32, "no_bins": 64}, "pae": {"min_bin": 0, "max_bin": 32, "no_bins": 64}}
NEW_SYMBOLS = ("pd_conf_loss_workspace_numel", "pd_lddt_atoms", "pd_conf_frames", "pd_conf_loss_plddt", "pd_conf_loss_pairs")
_cache = {}


def load_conf(name):
    """fixture + inputs as numpy arrays; the logits are rebuilt from the integer hash and checked against the stored checksums.
    Loaded once per session and shared (read-only)."""
    if name not in _cache:
        from physdock_amd.synthetic import CONF_FEAT_KEYS, confidence_loss_case
        g = dict(np.load(os.path.join(GOLDEN, f"g17_conf_loss_{name}.npz")))
        o, f, _ = confidence_loss_case(str(g["case"]), stored=g)
        for k in LOGITS.values():
            v = o[k].numpy().astype(np.float64)
            np.testing.assert_allclose([v.sum(), (v ** 2).sum()], g["checksum_" + k], rtol=1e-13, err_msg=k)
            assert abs(v).max() <= 4.0
            g[k] = o[k].numpy()
        for k in CONF_FEAT_KEYS:
            assert k in g, k
        _cache[name] = g
    return _cache[name]


# ------------------------------------------------------------------ float64 restatement of the reference's four functions
def norm(v):
    return np.sqrt((v * v).sum(-1))


def lddt_sums(x_pred, x_gt, is_dna, is_rna, is_polymer, centre):
    """cal_lddt (loss.py:346-370) up to its last line: (sum(mask_R * score), sum(mask_R)) per pose and atom"""
    d_pred = norm(x_pred[:, :, None, :] - x_pred[:, centre][:, None, :, :])
    d_gt = norm(x_gt[:, None, :] - x_gt[centre][None, :, :])
    d_lm = np.abs(d_pred - d_gt)
    score = 0.25 * ((d_lm < 0.5) * 1.0 + (d_lm < 1.0) * 1.0 + (d_lm < 2.0) * 1.0 + (d_lm < 4.0) * 1.0)
    nuc = (is_dna + is_rna)[None, :]
    mask = ((d_gt < 30) * nuc + (d_gt < 15) * (1 - nuc)) * is_polymer[None, :]
    return (mask * score).sum(-1), np.broadcast_to(mask.sum(-1), score.shape[:2])


def lddt_bin(num, den, no_bins):
    """the last line of cal_lddt and loss.py:408 as the reference's fp32 evaluates them.  num and den are sums of multiples of 0.25
    and exact in fp32, so one IEEE fp32 division and one fp32 product give the reference's bits; where lddt * no_bins is an integer
    (0.6 * 50) a float64 product could truncate to the other side.  NaN (0 / 0) -> the most negative integer -> clamp -> 0."""
    with np.errstate(invalid="ignore", divide="ignore"):
        lddt = num.astype(np.float32) / den.astype(np.float32)
        v = lddt * np.float32(no_bins)
    return lddt, np.where(np.isnan(v), 0, np.clip(np.trunc(np.nan_to_num(v)), 0, no_bins - 1)).astype(np.int64)


def in_frame(x, fr):
    """express_coordinates_in_frame (loss.py:184-207): x [T,3] tokens, fr [T,3,3] frame atoms -> ([F,T,3], valid [F])"""
    a, b, c = fr[:, 0], fr[:, 1], fr[:, 2]
    w1 = (a - b) / norm(a - b + 1e-6)[:, None]
    w2 = (c - b) / norm(c - b + 1e-6)[:, None]
    valid = (w1 * w2).sum(-1) < 0.906308
    e1 = (w1 + w2) / norm(w1 + w2 + 1e-6)[:, None]
    e2 = (w2 - w1) / norm(w2 - w1 + 1e-6)[:, None]
    R = np.stack([e1, e2, np.cross(e1, e2)], axis=1)                  # rows e1, e2, e3
    d = x[None, :, :] - b[:, None, :]
    return np.einsum("fij,faj->fai", R, d), valid


def binned(e, min_bin, max_bin, no_bins):
    return np.clip(np.trunc((e - min_bin) / (max_bin - min_bin) * no_bins), 0, no_bins - 1).astype(np.int64)


def masked_ce(logits, bins, mask):
    """softmax_cross_entropy(p * m, onehot * m) and masked_mean(m, .) (loss.py:21-26, tensor_utils.masked_mean, eps 1e-9)"""
    z = logits.astype(np.float64) * mask[..., None]
    z = z - z.max(-1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(-1, keepdims=True))
    onehot = (np.arange(z.shape[-1]) == bins[..., None]) * mask[..., None]
    return float((mask * -(onehot * logp).sum(-1)).sum() / (1e-9 + mask.sum()))


def restate(g):
    """{term: (value, bins)} and the lDDT of all poses, from the fixture's inputs"""
    xp, xg, ex = (g[k].astype(np.float64) for k in ("x_pred", "x_gt", "x_exists"))
    c = g["token_id_to_centre_atom_id"]
    poly = (g["is_ligand"] == 0).astype(np.float64)
    num, den = lddt_sums(xp, xg, g["is_dna"].astype(np.float64), g["is_rna"].astype(np.float64), poly, c)
    lddt, b = lddt_bin(num, den, 50)
    out = {"plddt": (masked_ce(g["p_plddt"], b[0], ex), b[0])}
    mask = np.outer(ex[c], ex[c])
    d_diff = np.abs(norm(xp[0][c][:, None] - xp[0][c][None]) - norm(xg[c][:, None] - xg[c][None]))
    b = binned(d_diff, **SETTINGS["pde"])
    out["pde"] = (masked_ce(g["p_pde"], b, mask), b)
    ids = np.stack([g[f"token_id_to_frame_atom_id_{k}"] for k in range(3)], -1)
    eg, vg = in_frame(xg[c], xg[ids])
    ep, vp = in_frame(xp[0][c], xp[0][ids])
    err = norm(ep - eg) * vg[:, None] * vp[:, None]
    b = binned(err, **SETTINGS["pae"])
    out["pae"] = (masked_ce(g["p_pae"], b, mask), b)
    return out, lddt


def test_fixture_set_is_complete():
    for name in CONF_CASES:
        path = os.path.join(GOLDEN, f"g17_conf_loss_{name}.npz")
        assert os.path.getsize(path) < (1 << 20)
        g = np.load(path)
        for k in g.files:                                   # only data: numeric arrays and a short string
            assert g[k].dtype.kind in "fiubU", (k, g[k].dtype)
        for k in ("closest_d_gt", "closest_d_lm", "closest_e_pde", "closest_e_pae"):
            assert float(g[k]) > 1e-4, (name, k)
        assert float(g["closest_cos"]) > 1e-5 and float(g["smallest_bisector"]) >= 0.1, name
    shapes = {n: (np.load(os.path.join(GOLDEN, f"g17_conf_loss_{n}.npz"))["x_pred"].shape,
                  np.load(os.path.join(GOLDEN, f"g17_conf_loss_{n}.npz"))["is_ligand"].shape[0]) for n in CONF_CASES}
    assert shapes == {"small": ((3, 96, 3), 24), "empty": ((3, 96, 3), 24), "mid": ((2, 437, 3), 71), "ragged": ((2, 1805, 3), 221)}


@pytest.mark.parametrize("name", CONF_CASES)
def test_float64_restatement_agrees_with_the_fixture(name):
    g = load_conf(name)
    mine, lddt = restate(g)
    ref = g["ref_lddt"]
    assert lddt.shape == ref.shape and np.array_equal(np.isnan(lddt), np.isnan(ref))
    assert np.array_equal(lddt[~np.isnan(ref)], ref[~np.isnan(ref)])              # the reference's fp32 lDDT, bit for bit
    for t in TERMS:
        v, b = mine[t]
        f64, r32 = float(g["f64_" + t]), float(g["ref_" + t])
        print(f"{name} {t}: restated {v!r} fixture f64 {f64!r} reference fp32 {r32!r} stored rel {float(g['ref_vs_f64_rel_' + t]):.3e}")
        assert np.array_equal(b, g["bins_" + t].astype(np.int64)), t
        assert abs(v - f64) <= 1e-10 * abs(f64), t
        assert abs(r32 - v) <= (float(g["ref_vs_f64_rel_" + t]) + 1e-7) * abs(v), t
        assert float(g["e_ref_" + t]) < 5e-6 and float(g["ref_vs_f64_rel_" + t]) < 5e-6
    assert (g["x_exists"][g["token_id_to_centre_atom_id"]] == 0).sum() == 1      # a masked centre: masked token pairs exist
    if name in ("small", "empty"):
        assert (g["x_exists"] == 0).sum() == 1 and g["is_dna"].sum() and g["is_rna"].sum() and g["is_ligand"].sum()
    if name == "empty":                                      # one atom without a polymer centre in range: NaN, bin 0
        a = g["x_gt"].shape[0] - 1
        assert np.isnan(ref[:, a]).all() and np.isnan(ref).sum() == ref.shape[0] and mine["plddt"][1][a] == 0
    else:
        assert not np.isnan(ref).any()
    if name in ("mid", "ragged"):
        assert g["x_gt"].shape[0] % 64 and g["is_ligand"].shape[0] % 16 and (g["is_ligand"].shape[0] ** 2) % 64
    assert len(np.unique(mine["plddt"][1])) >= 10 and len(np.unique(mine["pae"][1])) >= 20      # lDDT spreads over many bins
    invalid = (mine["pae"][1] == 0).all(-1).sum()
    assert invalid >= 1                                      # near-collinear frames occur


def test_gradient_rows_are_the_analytic_gradient():
    """g64 on the stored rows = m^3 (softmax(m p) - onehot) / (1e-9 + sum m), recomputed here"""
    g = load_conf("small")
    mine, _ = restate(g)
    ex = g["x_exists"].astype(np.float64)
    c = g["token_id_to_centre_atom_id"]
    for t in TERMS:
        m = ex if t == "plddt" else np.outer(ex[c], ex[c]).reshape(-1)
        p = g[LOGITS[t]].astype(np.float64).reshape(m.shape[0], -1)
        z = p * m[:, None]
        sm = np.exp(z - z.max(-1, keepdims=True))
        sm /= sm.sum(-1, keepdims=True)
        want = (m ** 3)[:, None] * (sm - (np.arange(p.shape[1]) == mine[t][1].reshape(-1)[:, None])) / (1e-9 + m.sum())
        np.testing.assert_allclose(g["g64_" + t], want[g["grow_" + t]], rtol=1e-10, atol=1e-18)
        np.testing.assert_allclose(g["sum_g64_" + t], [want.sum(), (want ** 2).sum()], rtol=1e-9, atol=1e-14)   # the sum itself is ~ 0: rows of softmax - onehot
        assert abs(float(g["absmax_" + t]) - np.abs(want).max()) <= 1e-12


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


def test_library_exports_the_confidence_loss_symbols():
    from physdock_amd import _lib, build
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) and not os.path.exists(_lib.LIB_PATH):
        pytest.skip("hipcc not available")
    build.build(verbose=False)
    L = _lib.lib()
    assert L.pd_abi_version() == 11
    for s in NEW_SYMBOLS:
        assert s in _lib.SYMBOLS and hasattr(L, s)
    # the documented formula: 4 + ceil(max(A, T^2) / 64)
    assert L.pd_conf_loss_workspace_numel(64, 2048, 256) == 4 + 1024
    assert L.pd_conf_loss_workspace_numel(1, 1805, 7) == 4 + 29
    assert L.pd_conf_loss_workspace_numel(2, 437, 71) == 4 + 79
    assert L.pd_conf_loss_workspace_numel(1, 0, 64) < 0 and L.pd_conf_loss_workspace_numel(1, 64, 0) < 0


def test_public_interface():
    import physdock_amd
    from physdock_amd import loss
    assert physdock_amd.ConfidenceLoss is loss.ConfidenceLoss
    for n in ("cal_lddt", "plddt_loss", "pde_loss", "pae_loss"):
        fn = getattr(physdock_amd, n)
        assert fn is getattr(loss, n) and n in loss.__all__
        assert any(p.kind is p.VAR_KEYWORD for p in inspect.signature(fn).parameters.values()), n
    assert list(inspect.signature(loss.cal_lddt).parameters)[:6] == ["x_pred", "x_gt", "is_dna", "is_rna", "is_polymer", "token_id_to_centre_atom_id"]
    assert list(inspect.signature(loss.plddt_loss).parameters)[:2] == ["p_plddt", "no_bins"]
    sp = inspect.signature(loss.pde_loss).parameters
    assert (sp["min_bin"].default, sp["max_bin"].default, sp["no_bins"].default) == (0.0, 32.0, 64)
    sp = inspect.signature(loss.pae_loss).parameters
    assert (sp["min_bin"].default, sp["max_bin"].default, sp["no_bins"].default) == (0, 32, 64)
    for m in ("terms", "grads", "forward"):
        assert callable(getattr(loss.ConfidenceLoss, m))


def test_cpu_tensors_are_refused():
    import torch
    from physdock_amd import ConfidenceLoss, PhysDockConfig, loss
    from physdock_amd.synthetic import CONF_FEAT_KEYS
    g = load_conf("small")
    o = {k: torch.from_numpy(g[k]) for k in ("p_plddt", "p_pde", "p_pae", "x_pred")}
    f = {k: torch.from_numpy(g[k]) for k in CONF_FEAT_KEYS}
    msg = r"runs on an MI355X \(HIP\) device only"
    with pytest.raises(RuntimeError, match=msg):
        ConfidenceLoss(PhysDockConfig())(o, f)
    with pytest.raises(RuntimeError, match=msg):
        loss.cal_lddt(o["x_pred"], f["x_gt"], f["is_dna"], f["is_rna"], f["is_ligand"] == 0, f["token_id_to_centre_atom_id"])
    with pytest.raises(RuntimeError, match=msg):
        loss.plddt_loss(no_bins=50, **o, **f)
    with pytest.raises(RuntimeError, match=msg):
        loss.pde_loss(**o, **f)
    with pytest.raises(RuntimeError, match=msg):
        loss.pae_loss(**o, **f)


def test_missing_frame_keys_with_a_pae_weight_is_a_key_error():
    import torch
    from physdock_amd import ConfidenceLoss, PhysDockConfig
    from physdock_amd.synthetic import CONF_FEAT_KEYS
    g = load_conf("small")
    o = {k: torch.from_numpy(g[k]) for k in ("p_plddt", "p_pde", "p_pae", "x_pred")}
    f = {k: torch.from_numpy(g[k]) for k in CONF_FEAT_KEYS if "frame" not in k}
    cfg = PhysDockConfig()
    cfg.loss.pae_loss.weight = 0.5
    with pytest.raises(KeyError, match="token_id_to_frame_atom_id_0"):
        ConfidenceLoss(cfg)(o, f)


def test_confidence_loss_kernels_have_no_scratch():
    """device assembly of confidence_loss.hip with the library's own flags: a zero private segment and zero spill counts in every
    kernel (the metadata fields only)"""
    from physdock_amd import build
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    src = os.path.join(build.CSRC, "confidence_loss.hip")
    assert src in build.sources()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "confidence_loss.s")
        r = subprocess.run(build.compile_cmd(src, out, mode=("-S", "--cuda-device-only")), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(out).read()
    assert "gfx950" in text
    meta = {m.group(1): m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n((?:\s+\.\w+:.*\n)+)", text)}
    kernels = [k for k in meta if re.search(r"lddt_atoms_kernel|conf_frames_kernel|conf_ce_", k) and not k.endswith(".kd")]
    assert len(kernels) == 7, kernels                        # lDDT, frames, coef, final, three modes of the cross entropy
    for k in kernels:
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta[k]), k
        assert re.search(r"\.vgpr_spill_count:\s+0\b", meta[k]) and re.search(r"\.sgpr_spill_count:\s+0\b", meta[k]), k
