"""PhysDockLoss, the parts that need no GPU: the committed fixtures (tests/golden/g15_loss_*.npz, tools/make_golden_loss.py) are
pinned to the formulas by an independent float64 restatement, the configuration carries the reference's loss block, the C ABI
(header, ctypes signatures, built library) has the new entry points, and the smooth-lDDT kernel compiles without scratch."""
import glob
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TERMS = ("weighted_mse_loss", "smooth_lddt_loss", "bond_loss", "key_res_loss", "distogram_loss")
CASES = sorted(os.path.basename(p)[len("g15_loss_"):-4] for p in glob.glob(os.path.join(GOLDEN, "g15_loss_*.npz")))
NEW_SYMBOLS = ("pd_loss_workspace_numel", "pd_loss_smooth_lddt", "pd_loss_centre_pairs", "pd_loss_distogram", "pd_loss_weighted_mse")


def load_case(name):
    """fixture + all its inputs as numpy arrays; outputs too large to commit are rebuilt from the stored arrays (integer-hash noise,
    bit-identical on every machine) and checked against their stored checksums"""
    g = dict(np.load(os.path.join(GOLDEN, f"g15_loss_{name}.npz")))
    from physdock_amd.synthetic import LOSS_FEAT_KEYS, LOSS_OUT_KEYS, loss_case
    o, f, _ = loss_case(str(g["case"]), stored=g)
    for k in LOSS_OUT_KEYS:
        v = o[k].numpy().astype(np.float64)
        np.testing.assert_allclose([np.nansum(v), np.nansum(v ** 2)], g["checksum_" + k], rtol=1e-13, err_msg=k)
        g[k] = o[k].numpy()
    for k in LOSS_FEAT_KEYS:
        assert k in g, k
    return g


def eps4(d):
    s = 0.0
    for c in (0.5, 1.0, 2.0, 4.0):
        s = s + 1.0 / (1.0 + np.exp(-(d - c)))
    return s / 4.0


def pairdist(x):
    d = x[:, None, :] - x[None, :, :]
    return np.sqrt(np.einsum("ijk,ijk->ij", d, d))


def restate_f64(g, cfg):
    """the five terms written from the reference's code (loss.py:78-181,245-318,535-559) in float64"""
    xd, xg, ex, t = (g[k].astype(np.float64) for k in ("x_denoised", "x_gt", "x_exists", "t_hat"))
    B, A = xd.shape[:2]
    out = {}
    # weighted_mse_loss
    c = cfg.weighted_mse_loss
    w = (1 + g["is_dna"] * c.alpha_dna + g["is_rna"] * c.alpha_rna + g["is_ligand"] * c.alpha_ligand)[g["atom_id_to_token_id"]] * ex
    sq = np.zeros((B, A))
    for b in range(B):
        xp = xd[b] * ex[:, None]
        if not np.isfinite(xp).all():
            sq[b] = np.nan
            continue
        mu_p, mu_g = w @ xp / w.sum(), w @ xg / w.sum()
        H = (xg - mu_g).T @ (w[:, None] * (xp - mu_p))
        U, _, Vh = np.linalg.svd(H)
        R = U @ Vh
        if np.linalg.det(R) < 0:
            R = U @ np.diag([1.0, 1.0, -1.0]) @ Vh
        sq[b] = np.sum((xd[b] - ((xg - mu_g) @ R + mu_p)) ** 2, -1)
    mm = np.sum(w[None] * sq) / (1e-9 + B * w.sum())
    v = np.mean((t ** 2 + 16.0 ** 2) / (t * 16.0) ** 2 * mm / 3)
    out["weighted_mse_loss"] = v if np.isnan(v) else min(v, 10000.0)
    # smooth_lddt_loss
    dgt = pairdist(xg)
    m = (dgt < cfg.smooth_lddt_loss.max_clamp_distance) * np.outer(ex, ex)
    out["smooth_lddt_loss"] = np.mean([np.sum(m * eps4(np.abs(pairdist(xd[b]) - dgt))) / (1e-9 + m.sum()) for b in range(B)])
    # bond_loss / key_res_loss
    ci = g["token_id_to_centre_atom_id"]
    dgc = pairdist(xg[ci])
    diffs = [pairdist(xd[b][ci]) - dgc for b in range(B)]
    tb = g["token_bonds"].astype(np.float64)
    km = np.outer(g["is_key_res"], g["is_ligand"]).astype(np.float64)
    sd = cfg.bond_loss.sigma_data
    out["bond_loss"] = np.mean((t ** 2 + sd ** 2) / (t * sd) ** 2 * np.mean([np.sum(tb * d ** 2) / (tb.sum() + 1e-9) for d in diffs]))
    sd = cfg.key_res_loss.sigma_data
    out["key_res_loss"] = np.mean(np.mean([np.sum(km * eps4(np.abs(d)) ** 2) / (km.sum() + 1e-9) for d in diffs])
                                  * (t ** 2 + sd ** 2) / (t * sd) ** 2)
    # distogram_loss
    c = cfg.distogram_loss
    pb = g["token_id_to_pseudo_beta_atom_id"]
    bounds = np.linspace(c.min_bin, c.max_bin, c.no_bins - 1) ** 2
    d2 = pairdist(xg[pb]) ** 2
    bins = np.sum(d2[..., None] > bounds, -1)
    md = np.outer(ex[pb], ex[pb])
    logits = g["p_distogram"].astype(np.float64) * md[..., None]
    logits = logits - logits.max(-1, keepdims=True)
    logp = logits - np.log(np.exp(logits).sum(-1, keepdims=True))
    onehot = (np.arange(c.no_bins) == bins[..., None]) * md[..., None]
    err = -np.sum(onehot * logp, -1)
    out["distogram_loss"] = np.sum(md * err) / (1e-9 + md.sum())
    return {k: float(v) for k, v in out.items()}


def test_fixture_set_is_complete():
    assert {"small", "ragged", "cfg1", "degenerate", "nan"} <= set(CASES)
    for name in CASES:
        path = os.path.join(GOLDEN, f"g15_loss_{name}.npz")
        assert os.path.getsize(path) < (1 << 20)
        g = np.load(path)
        assert float(g["closest_clamp_rel"]) > 1e-5 and float(g["closest_bin_rel"]) > 1e-5, name
        # only data: numeric arrays and two short strings
        for k in g.files:
            assert g[k].dtype.kind in "fiubU", (k, g[k].dtype)


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_agrees_with_the_reference_values(name):
    from physdock_amd import PhysDockConfig
    cfg = PhysDockConfig(model_name="medium").loss
    g = load_case(name)
    mine = restate_f64(g, cfg)
    total = 0.0
    for k, t in enumerate(TERMS):
        ref, f64 = float(g["ref_" + t]), float(g["f64_" + t])
        print(f"{name} {t}: restated {mine[t]!r} fixture f64 {f64!r} reference fp32 {ref!r} stored rel {float(g['ref_vs_f64_rel_' + t]):.3e}")
        if np.isnan(ref):
            assert np.isnan(mine[t]) and np.isnan(f64), t
            continue
        assert abs(mine[t] - f64) <= 1e-10 * abs(f64), t                       # two float64 evaluations of one formula
        # the reference's fp32 value sits where the fixture says it does (float32 rounding of the stored value allowed for)
        assert abs(ref - mine[t]) <= (float(g["ref_vs_f64_rel_" + t]) + 1e-7) * abs(mine[t]) + 0.0, t
        total += float(g["weights"][k]) * mine[t]
    assert abs(total - float(g["f64_loss"])) <= 1e-10 * abs(total)
    assert abs(float(g["ref_loss"]) - total) <= (float(g["ref_vs_f64_rel_loss"]) + 1e-7) * abs(total)
    if name == "degenerate":
        assert g["token_bonds"].sum() == 0 and g["is_key_res"].sum() == 0 and mine["bond_loss"] == 0 and mine["key_res_loss"] == 0
    if name == "small":
        assert (g["x_exists"] == 0).sum() == 1 and g["is_dna"].sum() and g["is_rna"].sum() and g["is_ligand"].sum()
        assert g["is_key_res"].sum() and g["token_bonds"].sum()
    if name == "ragged":
        assert g["x_gt"].shape[0] % 4 and g["is_ligand"].shape[0] % 4
    if name == "cfg1":
        assert g["x_denoised"].shape == (48, 2048, 3) and g["p_distogram"].shape == (256, 256, 39)


def test_config_has_the_reference_loss_block():
    from physdock_amd import PhysDockConfig, small_config
    want = {
        "weighted_mse_loss": {"weight": 4, "sigma_data": 16.0, "alpha_dna": 5.0, "alpha_rna": 5.0, "alpha_ligand": 10.0},
        "smooth_lddt_loss": {"weight": 4, "max_clamp_distance": 15.0},
        "bond_loss": {"weight": 0, "sigma_data": 16.0},
        "key_res_loss": {"weight": 0, "sigma_data": 16.0},
        "distogram_loss": {"weight": 3e-2, "min_bin": 3.25, "max_bin": 50.75, "no_bins": 39, "eps": 1e-9},
        "plddt_loss": {"weight": 1e-4, "no_bins": 50},
        "pae_loss": {"weight": 0.0},
        "pde_loss": {"weight": 1e-4, "min_bin": 0, "max_bin": 32, "no_bins": 64},
    }
    for cfg in (PhysDockConfig(model_name="medium"), small_config()):
        assert cfg.loss.to_dict() == want
    c = PhysDockConfig(alpha_diffusion=2, alpha_bond=0.5, alpha_distogram=0.1, sigma_data=8.0).loss
    assert c.bond_loss.weight == 1.0 and c.key_res_loss.weight == 1.0 and c.smooth_lddt_loss.weight == 2
    assert c.distogram_loss.weight == 0.1 and c.weighted_mse_loss.sigma_data == 8.0
    for name in CASES:       # the weights the fixtures were made with are the defaults
        g = np.load(os.path.join(GOLDEN, f"g15_loss_{name}.npz"))
        assert list(g["weights"]) == [want[t]["weight"] for t in TERMS]


def test_public_interface():
    import inspect
    import physdock_amd
    from physdock_amd import loss
    assert physdock_amd.PhysDockLoss is loss.PhysDockLoss
    for t in TERMS:
        assert callable(getattr(loss, t))
        assert any(p.kind is p.VAR_KEYWORD for p in inspect.signature(getattr(loss, t)).parameters.values()), t
    assert "return_loss" in inspect.signature(physdock_amd.PhysDock.forward).parameters
    assert inspect.signature(physdock_amd.PhysDock.forward).parameters["return_loss"].default is False


def test_cpu_tensors_are_refused():
    import torch
    from physdock_amd import PhysDockConfig, PhysDockLoss
    g = load_case("small")
    o = {k: torch.from_numpy(g[k]) for k in ("x_denoised", "t_hat", "p_distogram")}
    f = {k: torch.from_numpy(g[k]) for k in ("x_gt", "x_exists", "atom_id_to_token_id", "token_id_to_centre_atom_id",
                                             "token_id_to_pseudo_beta_atom_id", "token_bonds", "is_dna", "is_rna", "is_ligand", "is_key_res")}
    with pytest.raises(RuntimeError, match=r"runs on an MI355X \(HIP\) device only"):
        PhysDockLoss(PhysDockConfig())(o, f)


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


def test_library_exports_the_loss_symbols():
    from physdock_amd import _lib, build
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) and not os.path.exists(_lib.LIB_PATH):
        pytest.skip("hipcc not available")
    build.build(verbose=False)
    L = _lib.lib()
    assert L.pd_abi_version() == 11
    for s in NEW_SYMBOLS:
        assert s in _lib.SYMBOLS and hasattr(L, s)
    # the documented formula: max(n (n + 1) / 2 * (B + 1), 2 T B, 2 ceil(T^2 / 256), B), n = ceil(A / 64)
    assert L.pd_loss_workspace_numel(48, 2048, 256) == 528 * 49
    assert L.pd_loss_workspace_numel(2, 64, 512) == 2 * 1024
    assert L.pd_loss_workspace_numel(0, 64, 64) < 0


def test_smooth_lddt_kernel_has_no_scratch():
    """device assembly of loss.hip with the library's own flags: no spills, no private segment in any of its kernels, the hot
    kernel keeps one exponential and four reciprocals per pair term"""
    from physdock_amd import build
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    src = os.path.join(build.CSRC, "loss.hip")
    assert src in build.sources()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "loss.s")
        r = subprocess.run(build.compile_cmd(src, out, mode=("-S", "--cuda-device-only")), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "scratch" not in r.stderr.lower() and "spill" not in r.stderr.lower(), r.stderr
        text = open(out).read()
    assert "gfx950" in text
    meta = {m.group(1): m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n((?:\s+\.\w+:.*\n)+)", text)}
    kernels = [k for k in meta if "kernel" in k or "final" in k]
    assert any("smooth_lddt_kernel" in k for k in kernels) and len(kernels) == 8, kernels
    for k in kernels:
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta[k]), k
        assert re.search(r"\.vgpr_spill_count:\s+0\b", meta[k]) and re.search(r"\.sgpr_spill_count:\s+0\b", meta[k]), k
    body = text[text.index("smooth_lddt_kernel"):]
    body = body[:body.index("s_endpgm")]
    assert "scratch_" not in body
    assert body.count("v_exp_f32") == 16 and body.count("v_rcp_f32") == 64, (body.count("v_exp_f32"), body.count("v_rcp_f32"))
