"""Kernel-level tests of csrc/mmff.hip (pd_mmff_energy_grad, pd_mmff_relax) against the vectorised float64 reference
tests/mmff_ref.py, at every ligand size where the kernel changes its parallel shape:

    L              threads per atom   atom passes            matvec_sym (relaxation, dim = 3 L)
    1, 2, 4        8                  1                      split, 85 / 42 / 21 parts (most of them empty)
    12             8                  1                      split, 7 parts of 6, last clamped
    28 / 29        8                  1                      split, 3 parts of 28 / 2 parts of 44 with the last clamped
    32 / 33        8 / 4              1                      (energy only)
    42 / 43        4                  1                      split, 2 parts of 63 / plain
    64 / 65        4 / 2              1                      (energy only)
    85 / 86        2                  1                      plain, dim 255 / 258: one round of outputs / a second round
    128 / 129      2 / 1              1                      plain
    130            1                  1                      (checks without a reference)
    256 / 257      1                  1 / 2 (1 atom ragged)  (energy only)
    300            1                  2, the last ragged     plain, 2 iterations

The relaxation cases, their starts and their reference results live in tests/mmff_cases.py; tests/test_mmff_ref_cpu.py asserts on the
CPU that every optimiser decision of every case has a margin, which branches the cases reach (and lists the ones they do not, with the
reason), that the converged start leaves the loop early, and that the reference itself moves by at most 2e-6 A under another summation
order - a tenth of the 2e-5 A asserted here.  Every test prints the figure it asserts (pytest -s).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mmff_cases as mc
import mmff_ref as mr

pytestmark = pytest.mark.gpu

PD_ERR_ARG = -1
SENTINEL = -777.25
ENERGY_SIZES = (1, 2, 4, 32, 33, 64, 65, 128, 129, 256, 257, 300)


# ------------------------------------------------------------------ plumbing
def lib():
    from physdock_amd import ops
    return ops._lib.init()


def stream():
    from physdock_amd import ops
    return ops.stream()


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))
    return (t if dtype is None else t.to(dtype)).cuda()


def conformations(L, seed=1):
    """[3, L, 3]: equilibrium, 0.05 A and 0.3 A of noise"""
    _, _, coords = mc.molecule(L, seed)
    rng = np.random.default_rng(seed)
    return np.stack([coords + s * rng.normal(size=coords.shape) for s in (0.0, 0.05, 0.3)])


def raw_energy_grad(struct, pos, want_energy=True, want_grad=True, B=None):
    """pd_mmff_energy_grad straight on the C ABI; outputs it is not asked for stay None, the others start as SENTINEL"""
    p = dev(pos)
    B = p.shape[0] if B is None else B
    E = torch.full((p.shape[0],), SENTINEL, dtype=torch.float64, device="cuda")
    G = torch.full_like(p, SENTINEL)
    rc = lib().pd_mmff_energy_grad(C.byref(struct), p.data_ptr(), E.data_ptr() if want_energy else None,
                                   G.data_ptr() if want_grad else None, B, stream())
    torch.cuda.synchronize()
    return rc, E.cpu().numpy(), G.cpu().numpy()


def assert_matches_reference(terms, pos, what):
    t = mr.prepare(terms.as_numpy())
    E, G = terms.energy_grad(dev(pos))
    E, G = E.cpu().numpy(), G.cpu().numpy()
    assert np.isfinite(E).all() and np.isfinite(G).all()
    for b in range(len(pos)):
        e, g = mr.energy_and_grad(pos[b], t)
        de, dg = abs(E[b] - e) / max(1.0, abs(e)), np.abs(G[b] - g).max() / max(1.0, np.abs(g).max())
        print(f"{what} conformation {b}: energy {e:.6f}, relative error {de:.1e}; gradient error {dg:.1e} of max(1, |g|max)")
        assert de <= 1e-10, (what, b, E[b], e)
        assert dg <= 1e-9, (what, b, dg)
    return E, G


def hand_terms(n, bonds=(), angles=(), strbnd=(), oops=(), tors=(), vdw=(), ele=()):
    """tables built by hand: bonds [(i, j, kb, r0)], angles [(i, j, k, ka, theta0, linear)], strbnd [(i, j, k, kijk, kkji, r0ij, r0kj,
    theta0)], oops [(i, j, k, l, koop)], tors [(i, j, k, l, v1, v2, v3)], vdw [(i, j, R*, eps)], ele [(i, j, qq)]"""
    from physdock_amd import mmff
    R, eps, qq = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    for i, j, r, e in vdw:
        R[i, j] = R[j, i] = r
        eps[i, j] = eps[j, i] = e
    for i, j, q in ele:
        qq[i, j] = qq[j, i] = q

    def split(rows, k):
        return [r[:k] for r in rows], [r[k:] for r in rows]
    return mmff.MMFFTerms(n, *split(bonds, 2), *split(angles, 3), *split(strbnd, 3), *split(oops, 4), *split(tors, 4), R, eps, qq)


# ------------------------------------------------------------------ energy / gradient
@pytest.mark.parametrize("L", ENERGY_SIZES)
def test_energy_gradient_vs_reference(L):
    terms, _, _ = mc.molecule(L, 1)
    pos = conformations(L)
    E, G = assert_matches_reference(terms, pos, f"L={L}")
    # either output alone gives the same bits as both together
    s, _ = terms.device_tables(torch.device("cuda", torch.cuda.current_device()))
    rc, e_only, g_untouched = raw_energy_grad(s, pos, want_grad=False)
    assert rc == 0 and np.array_equal(e_only, E) and (g_untouched == SENTINEL).all()
    rc, e_untouched, g_only = raw_energy_grad(s, pos, want_energy=False)
    assert rc == 0 and np.array_equal(g_only, G) and (e_untouched == SENTINEL).all()


@pytest.fixture(scope="module", params=(43, 130))
def selfcheck(request):
    """(terms, one noisy conformation, its energy and gradient from the kernel)"""
    L = request.param
    terms, _, coords = mc.molecule(L, 2)
    p = coords + 0.15 * np.random.default_rng(L).normal(size=coords.shape)
    E, G = terms.energy_grad(dev(p[None]))
    return terms, p, float(E[0]), G[0].cpu().numpy()


def test_gradient_is_the_derivative_of_the_kernels_own_energy(selfcheck):
    terms, p, _, g = selfcheck
    L, h = terms.n_atoms, 1e-6
    disp = np.repeat(p[None], 6 * L, axis=0).reshape(2, 3 * L, 3 * L)       # [sign, coordinate, 3 L]
    disp[0, np.arange(3 * L), np.arange(3 * L)] += h
    disp[1, np.arange(3 * L), np.arange(3 * L)] -= h
    E, _ = terms.energy_grad(dev(disp.reshape(6 * L, L, 3)))                 # one launch of 6 L blocks
    E = E.cpu().numpy().reshape(2, 3 * L)
    num = ((E[0] - E[1]) / (2 * h)).reshape(L, 3)
    err = np.abs(num - g).max() / max(1.0, np.abs(g).max())
    print(f"L={L}: central differences of the kernel's energy vs its gradient: {err:.1e} of max(1, |g|max)")
    assert err < 1e-5


def test_net_force_and_torque_vanish(selfcheck):
    terms, p, _, g = selfcheck
    scale = max(1.0, np.abs(g).max())
    force, torque = np.abs(g.sum(0)).max(), np.abs(np.cross(p, g).sum(0)).max()
    print(f"L={terms.n_atoms}: net force {force / scale:.1e}, net torque {torque / (scale * np.abs(p).max()):.1e} (relative)")
    assert force < 1e-8 * scale
    assert torque < 1e-8 * scale * np.abs(p).max()


def test_relabelled_atoms_give_the_same_energy_and_gradient(selfcheck):
    terms, p, e, g = selfcheck
    L = terms.n_atoms
    perm = np.random.default_rng(5 + L).permutation(L)
    q = np.empty_like(p)
    q[perm] = p
    E2, G2 = mr.relabel(terms, perm).energy_grad(dev(q[None]))
    e2, g2 = float(E2[0]), G2[0].cpu().numpy()[perm]
    de, dg = abs(e2 - e) / max(1.0, abs(e)), np.abs(g2 - g).max() / np.abs(g).max()
    print(f"L={L}: relabelled energy {de:.1e}, gradient {dg:.1e} (relative)")
    assert de <= 1e-10 and dg <= 1e-9


# ------------------------------------------------------------------ degenerate tables
def test_collinear_torsion_contributes_nothing():
    terms = hand_terms(4, tors=[(0, 1, 2, 3, 0.7, 1.3, 0.4)])
    pos = np.array([[[0.0, 0, 0], [1.5, 0, 0], [3.0, 0, 0], [3.5, 1.2, 0.3]],          # i, j, k exactly collinear
                    [[0.3, 1.0, 0], [0, 0, 0], [1.5, 0, 0], [3.0, 0, 0]]])               # j, k, l exactly collinear
    E, G = terms.energy_grad(dev(pos))
    assert torch.isfinite(E).all() and torch.isfinite(G).all()
    assert (E == 0).all() and (G == 0).all()
    assert_matches_reference(terms, pos, "collinear torsion")


def test_atom_without_bonded_terms_and_fragment_without_pairs():
    # 0-1-2 bonded with an angle; 3 has no bonded term (only pairs with 0, 1 and 2); 4-5 is a bonded fragment no pair table mentions
    terms = hand_terms(6, bonds=[(0, 1, 5.0, 1.5), (1, 2, 4.2, 1.4), (4, 5, 6.1, 1.2)], angles=[(0, 1, 2, 0.8, 109.5, 0.0)],
                       vdw=[(0, 3, 3.6, 0.07), (1, 3, 3.4, 0.05)], ele=[(0, 3, -0.12), (2, 3, 0.08)])
    assert terms.inc_ptr[3] == terms.inc_ptr[4]
    rng = np.random.default_rng(0)
    base = np.array([[0.0, 0, 0], [1.55, 0, 0], [2.1, 1.3, 0], [0.5, 3.2, 1.0], [6.0, 0, 0], [6.0, 1.25, 0]])
    pos = np.stack([base, base + 0.1 * rng.normal(size=base.shape)])
    _, G = assert_matches_reference(terms, pos, "isolated atom / bare fragment")
    assert np.abs(G[:, 3]).max() > 0 and np.abs(G[:, 4:]).max() > 0


def test_tables_without_oop_and_torsions():
    terms = hand_terms(3, bonds=[(0, 1, 5.0, 1.5), (1, 2, 4.2, 1.4)], angles=[(0, 1, 2, 0.8, 109.5, 0.0)],
                       strbnd=[(0, 1, 2, 0.3, 0.2, 1.5, 1.4, 109.5)])
    s, keep = terms.device_tables(torch.device("cuda", torch.cuda.current_device()))
    assert s.n_oop == 0 and s.n_tors == 0 and keep["oop_idx"].numel() == 4 and keep["tors_par"].numel() == 4      # the dummy buffers
    base = np.array([[0.0, 0, 0], [1.55, 0, 0], [2.1, 1.3, 0]])
    pos = np.stack([base, base + 0.1 * np.random.default_rng(1).normal(size=base.shape)])
    assert_matches_reference(terms, pos, "no oop, no torsion")


# ------------------------------------------------------------------ relaxation
@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_relaxation_vs_reference(case):
    terms, _, _ = mc.molecule(case.L, case.seed)
    start = mc.starts(case)
    ref, traces = mc.reference(case)
    x = dev(start)
    out = terms.relax(x, max_iters=case.iters)
    again = terms.relax(x, max_iters=case.iters)
    assert torch.equal(out, again)                                      # no atomics: bit-reproducible
    assert np.array_equal(x.cpu().numpy(), start)
    out = out.cpu().numpy()
    assert np.isfinite(out).all()
    for b, kind in enumerate(case.starts):
        err = np.abs(out[b] - ref[b]).max()
        print(f"{mc.case_id(case)} {kind:5s}: exit {traces[b]['exit']} after {traces[b]['iters']} iterations, moved "
              f"{np.abs(ref[b] - start[b]).max():.1e} A, kernel - reference {err:.1e} A")
        assert err < mc.TOL_A, (b, kind, err)
    if case.iters == 0:
        assert np.array_equal(out, start)                               # bit-identical to the float32 input


def test_relax_plumbing_subset_rows_and_poisoned_workspace():
    """A > L with the ligand on a shuffled subset of rows; workspace NaN-filled and longer than needed"""
    case = next(c for c in mc.CASES if c.L == 43)
    terms, _, _ = mc.molecule(case.L, case.seed)
    ref, _ = mc.reference(case)
    L, B, A, extra = case.L, 4, 61, 1000
    rng = np.random.default_rng(11)
    rows = rng.permutation(A)[:L]
    x_np = rng.normal(size=(B, A, 3)).astype(np.float32) * 7.0
    x_np[:, rows] = mc.starts(case)
    x = dev(x_np)
    x_ref = torch.full_like(x, float("nan"))
    need = terms.workspace_numel(B)
    ws = torch.full((need + extra,), float("nan"), dtype=torch.float64, device="cuda")
    terms.launch_relax(terms.device_tables(x.device), x, dev(rows.astype(np.int32)), x_ref, ws, B, A, case.iters, stream())
    torch.cuda.synchronize()
    out = x_ref.cpu().numpy()
    err = np.abs(out[:, rows] - ref).max()
    print(f"ligand on rows {rows[:4]}... of {A}: kernel - reference {err:.1e} A")
    assert err < mc.TOL_A
    other = np.setdiff1d(np.arange(A), rows)
    assert np.array_equal(out[:, other], x_np[:, other])
    assert np.array_equal(x.cpu().numpy(), x_np)
    assert torch.isnan(ws[need:]).all()
    # the poisoned workspace changes nothing: the kernel initialises whatever it reads
    plain = terms.relax(dev(mc.starts(case)), max_iters=case.iters).cpu().numpy()
    assert np.array_equal(out[:, rows], plain)


# ------------------------------------------------------------------ refusals
def clone(struct, **changes):
    from physdock_amd import mmff
    c = mmff.MMFFTermsStruct()
    for name, _ in struct._fields_:
        setattr(c, name, changes.get(name, getattr(struct, name)))
    return c


def test_refused_calls_return_err_arg_and_write_nothing():
    L, B = 12, 2
    terms, _, coords = mc.molecule(L, 1)
    s, _ = terms.device_tables(torch.device("cuda", torch.cuda.current_device()))
    pos = np.stack([coords, coords + 0.1])

    def energy(struct=s, **kw):
        rc, E, G = raw_energy_grad(struct, pos, **kw)
        assert (E == SENTINEL).all() and (G == SENTINEL).all(), kw
        return rc
    rcs = {"n_atoms 0": energy(clone(s, n_atoms=0)), "n_atoms 1025": energy(clone(s, n_atoms=1025)),
           "null vdw_R": energy(clone(s, vdw_R=None)), "null bond_idx": energy(clone(s, bond_idx=None)),
           "no output": energy(want_energy=False, want_grad=False), "B 0": energy(B=0)}
    assert s.n_bond > 0

    A = L + 3
    x = torch.randn(B, A, 3, device="cuda")
    idx = torch.arange(L, dtype=torch.int32, device="cuda")
    need = terms.workspace_numel(B)
    ws = torch.full((need,), SENTINEL, dtype=torch.float64, device="cuda")

    def relax(struct=s, ws_doubles=need, B=B, A=A, max_iters=3):
        out = torch.full_like(x, SENTINEL)
        rc = lib().pd_mmff_relax(C.byref(struct), x.data_ptr(), idx.data_ptr(), out.data_ptr(), ws.data_ptr(), ws_doubles, B, A,
                                 max_iters, stream())
        torch.cuda.synchronize()
        assert (out == SENTINEL).all() and (ws == SENTINEL).all()
        return rc
    rcs.update({"relax n_atoms 0": relax(clone(s, n_atoms=0)), "relax n_atoms 1025": relax(clone(s, n_atoms=1025)),
                "relax null vdw_R": relax(clone(s, vdw_R=None)), "relax null bond_idx": relax(clone(s, bond_idx=None)),
                "relax B 0": relax(B=0), "A < n_atoms": relax(A=L - 1), "max_iters -1": relax(max_iters=-1),
                "workspace one short": relax(ws_doubles=need - 1)})
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), rcs
    # and the same call with nothing wrong is accepted
    out = torch.full_like(x, SENTINEL)
    assert lib().pd_mmff_relax(C.byref(s), x.data_ptr(), idx.data_ptr(), out.data_ptr(), ws.data_ptr(), need, B, A, 0, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, x)
