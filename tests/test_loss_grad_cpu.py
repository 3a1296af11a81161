"""PhysDockLoss gradients, the parts that need no GPU: the committed gradient fixtures (tests/golden/g16_loss_grad_*.npz,
tools/make_golden_loss_grad.py) against central finite differences of the float64 forward, their sign-tie allowance cap, and
the C ABI of the four gradient launchers (header, ctypes signatures, built library; ABI version unchanged)."""
import glob
import os
import re

import numpy as np
import pytest

from test_loss_cpu import GOLDEN, TERMS, load_case, restate_f64

GRAD_CASES = ("small", "ragged", "cfg1", "degenerate", "nan", "clamped", "shared-centre", "grad-only-p")
GRAD_SYMBOLS = ("pd_loss_grad_workspace_numel", "pd_loss_weighted_mse_grad", "pd_loss_smooth_lddt_grad", "pd_loss_centre_pairs_grad",
                "pd_loss_distogram_grad")
X_TERMS = TERMS[:4]


def load_grad(name):
    """(gradient fixture, inputs as numpy arrays): the g15 cases take their inputs from the g15 fixture, the others store theirs"""
    g = dict(np.load(os.path.join(GOLDEN, f"g16_loss_grad_{name}.npz")))
    if str(g["base"]) == name:
        return g, load_case(name)
    return g, g


def test_fixture_set_is_complete():
    have = {os.path.basename(p)[len("g16_loss_grad_"):-4] for p in glob.glob(os.path.join(GOLDEN, "g16_loss_grad_*.npz"))}
    assert set(GRAD_CASES) <= have
    for name in GRAD_CASES:
        path = os.path.join(GOLDEN, f"g16_loss_grad_{name}.npz")
        assert os.path.getsize(path) < (1 << 20)
        g = np.load(path)
        for k in g.files:
            assert g[k].dtype.kind in "fiubU", (k, g[k].dtype)


@pytest.mark.parametrize("name", GRAD_CASES)
def test_allowance_cap(name):
    """sign ties: per sample, the allowance sums to at most 1 % of ||g64||_1 (computed by the generator over the full arrays,
    re-checked here on the stored rows).  Measured: smooth lDDT 1.0e-4 (ragged) to 2.7e-3 (cfg1); key-res 0 on the small cases
    and 7.1e-3 on cfg1, where the samples with a small t_hat put many key-residue / ligand pairs below tau = 6.1e-5."""
    g, _ = load_grad(name)
    for t in ("smooth_lddt_loss", "key_res_loss"):
        if not g["has_" + t]:
            continue
        assert float(g["ratio_" + t]) <= 0.01, (t, float(g["ratio_" + t]))
        a, g64 = g["allow_" + t], g["g64_" + t]
        for b in range(a.shape[0]):
            assert a[b].sum() <= 0.01 * np.abs(g64[b]).sum() + 0.0, (t, b)
        print(f"{name} {t}: ratio {float(g['ratio_' + t]):.2e}")


def test_clamped_and_special_cases_are_what_they_claim():
    g, _ = load_grad("clamped")
    assert float(g["pre_clamp_weighted_mse"]) > 1e4 and not np.abs(g["g64_weighted_mse_loss"]).any()
    g, inp = load_grad("shared-centre")
    ci = inp["token_id_to_centre_atom_id"]
    assert len(set(ci.tolist())) <= len(ci) - 2
    g, _ = load_grad("grad-only-p")
    assert not g["need_x"] and not any(g["has_" + t] for t in X_TERMS) and g["has_distogram_loss"]
    g, _ = load_grad("nan")
    assert not any(g["has_" + t] for t in X_TERMS) and g["has_distogram_loss"]


def test_float64_gradients_agree_with_finite_differences():
    """small case: central differences (h = 1e-6) of the float64 restatement of the forward (test_loss_cpu.restate_f64) at
    coordinates of atoms that sit in no pair with |d - d_gt| < 1e-3 (no kink of |.| or sign() within reach), and at logits"""
    from physdock_amd import PhysDockConfig
    cfg = PhysDockConfig(model_name="medium").loss
    g, inp = load_grad("small")
    base = {k: np.array(v) for k, v in inp.items()}
    xd = base["x_denoised"].astype(np.float64)
    B, A = xd.shape[:2]
    ci = base["token_id_to_centre_atom_id"]

    def loss_at(x=None, p=None):
        h = dict(base)
        if x is not None:
            h["x_denoised"] = x
        if p is not None:
            h["p_distogram"] = p
        return restate_f64(h, cfg)

    def pd(x):
        return np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))

    dgt = pd(base["x_gt"].astype(np.float64))
    rng = np.random.RandomState(0)
    picked = []
    for b in range(B):
        dl = np.abs(pd(xd[b]) - dgt)
        np.fill_diagonal(dl, np.inf)
        ok = np.nonzero(dl.min(1) > 1e-3)[0]
        dlc = np.abs(pd(xd[b][ci]) - dgt[np.ix_(ci, ci)])
        np.fill_diagonal(dlc, np.inf)
        okc = [int(ci[k]) for k in range(len(ci)) if dlc[k].min() > 1e-3]
        picked += [(b, int(i), int(rng.randint(3))) for i in rng.choice(ok, 3, replace=False)]
        picked += [(b, i, int(rng.randint(3))) for i in rng.choice(okc, 2, replace=False)]
    h = 1e-6
    for t in X_TERMS:
        g64 = g["g64_" + t]
        scale = np.abs(g64).max()
        for (b, i, c) in picked:
            xp, xm = xd.copy(), xd.copy()
            xp[b, i, c] += h
            xm[b, i, c] -= h
            fd = (loss_at(x=xp)[t] - loss_at(x=xm)[t]) / (2 * h)
            print(f"{t} ({b},{i},{c}): g64 {g64[b, i, c]!r} fd {fd!r}")
            assert abs(fd - g64[b, i, c]) <= 1e-5 * scale, (t, b, i, c, fd, g64[b, i, c])
    p = base["p_distogram"].astype(np.float64)
    g64 = g["g64_distogram_loss"]
    for (i, j, k) in [(0, 1, 0), (3, 7, 5), (10, 2, 38), (23, 23, 12), (5, 19, 20)]:
        pp, pm = p.copy(), p.copy()
        pp[i, j, k] += h
        pm[i, j, k] -= h
        fd = (loss_at(p=pp)["distogram_loss"] - loss_at(p=pm)["distogram_loss"]) / (2 * h)
        print(f"distogram ({i},{j},{k}): g64 {g64[i, j, k]!r} fd {fd!r}")
        assert abs(fd - g64[i, j, k]) <= 1e-5 * np.abs(g64).max()


def test_abi_version_is_still_11_and_header_declares_the_launchers():
    from physdock_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "physdock_hip.h")).read()
    assert int(re.search(r"#define\s+PD_ABI_VERSION\s+(\d+)", hdr).group(1)) == 11 == _lib.ABI_VERSION
    assert set(GRAD_SYMBOLS) <= set(_lib.header_symbols())
    src = open(os.path.join(_lib._HERE, "_lib.py")).read()
    for s in GRAD_SYMBOLS:
        n_hdr = len(re.search(rf"int\s+{s}\s*\(([^;]*)\)\s*;", hdr).group(1).split(","))
        n_sig = len(re.search(rf'sig\("{s}",([^\n#]*)\)', src).group(1).split(","))
        assert n_hdr == n_sig, (s, n_hdr, n_sig)


def test_library_exports_the_gradient_launchers():
    from physdock_amd import _lib, build
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) and not os.path.exists(_lib.LIB_PATH):
        pytest.skip("hipcc not available")
    build.build(verbose=False)
    L = _lib.lib()
    assert L.pd_abi_version() == 11
    for s in GRAD_SYMBOLS:
        assert s in _lib.SYMBOLS and hasattr(L, s)
    # max(3 B A + ceil(A / 64), 4 + 3 B T, B + 1)
    assert L.pd_loss_grad_workspace_numel(48, 2048, 256) == 3 * 48 * 2048 + 32
    assert L.pd_loss_grad_workspace_numel(2, 64, 512) == 4 + 3 * 2 * 512
    assert L.pd_loss_grad_workspace_numel(0, 64, 64) < 0
    assert L.pd_loss_workspace_numel(48, 2048, 256) == 528 * 49           # the forward's is unchanged


def test_public_interface_has_grads():
    import inspect
    from physdock_amd import PhysDockLoss
    assert list(inspect.signature(PhysDockLoss.grads).parameters) == ["self", "outputs", "feats", "grad_scale"]
    from physdock_amd import loss
    assert "Forward values only" not in loss.__doc__
