"""The definition of the distance-geometry conformers (tests/conformers_ref.py) and the host side of physdock_amd/conformers.py."""
import numpy as np
import pytest

import conformers_ref as cr
from physdock_amd import conformers as pc

SMALL = ("chain2", "chain3", "chain4", "centre5", "toluene7", "phenyl14")


def _x4(c):
    return np.concatenate([c["x_ref"], np.zeros((c["n_atoms"], 1))], axis=1)


@pytest.mark.parametrize("name", cr.CASES)
def test_reference_conformer_has_zero_error(name):
    c, t = cr.make_case(name), cr.case_tables(name)
    for w_chi, w_4d in cr.STAGES:
        e, g = cr.error_and_grad(t, _x4(c), w_chi, w_4d)
        assert e == 0.0 and not g.any()
    assert cr.max_violation(t, c["x_ref"]) == 0.0


@pytest.mark.parametrize("name", cr.CASES)
def test_bounds_are_ordered_and_triangle_smoothed(name):
    t = cr.case_tables(name)
    lo, up = t["lo"], t["up"]
    assert (lo <= up).all() and (lo == lo.T).all() and (up == up.T).all()
    off = ~np.eye(lo.shape[0], dtype=bool)
    assert (lo[off] > 0).all()
    assert (up[:, None, :] <= up[:, :, None] + up[None, :, :] + 1e-12).all()              # up_ij <= up_ik + up_kj
    assert (lo[:, None, :] >= lo[:, :, None] - up[None, :, :] - 1e-12).all()              # lo_ij >= lo_ik - up_kj


@pytest.mark.parametrize("name", cr.CASES)
def test_package_tables_equal_the_definition(name):
    c, t = cr.make_case(name), cr.case_tables(name)
    ens = pc.ConformerEnsemble.from_bonds(c["n_atoms"], c["bonds"], c["x_ref"], c["elements"], bond_orders=c["bond_orders"],
                                          planar_groups=c["planar_groups"], centres=c["centres"])
    np.testing.assert_allclose(ens.lo, t["lo"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ens.up, t["up"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ens.vol_lo, t["vol_lo"], rtol=1e-14)
    np.testing.assert_allclose(ens.vol_hi, t["vol_hi"], rtol=1e-14)
    assert ens.centres.tolist() == t["centres"].tolist() and abs(ens.box - t["box"]) < 1e-12


def test_package_perceives_groups_and_centres_itself():
    c = cr.make_case("phenyl14")
    ens = pc.ConformerEnsemble.from_bonds(c["n_atoms"], c["bonds"], c["x_ref"], c["elements"], bond_orders=c["bond_orders"])
    assert ens.centres.tolist() == [[8, 7, 9, 11]]
    lo, up, kind = cr.raw_bounds(c["n_atoms"], c["bonds"], c["x_ref"], c["elements"], c["planar_groups"])
    assert kind[0, 3] == 3 and kind[1, 4] == 3                                          # para pairs of the ring: planar, not 1-4
    d = np.linalg.norm(c["x_ref"][0] - c["x_ref"][3])
    assert abs(ens.up[0, 3] - (d + 0.05)) < 1e-9 and abs(ens.lo[0, 3] - (d - 0.05)) < 1e-9


def test_the_1_4_closed_forms_agree_with_a_brute_rotation():
    rng = np.random.default_rng(5)
    for _ in range(20):
        a, b, c = rng.uniform(1.0, 2.0, 3)
        th1, th2 = rng.uniform(np.deg2rad(95.0), np.deg2rad(150.0), 2)
        i = np.array([a * np.cos(th1), a * np.sin(th1), 0.0])
        phi = np.linspace(0.0, np.pi, 2001)
        l = np.stack([b - c * np.cos(th2) + 0 * phi, c * np.sin(th2) * np.cos(phi), c * np.sin(th2) * np.sin(phi)], axis=1)
        d = np.linalg.norm(l - i, axis=1)
        cis, trans = cr.d14(a, b, c, th1, th2)
        assert abs(d.min() - cis) < 1e-12 and abs(d.max() - trans) < 1e-12 and d.argmin() == 0 and d.argmax() == 2000
    t = cr.case_tables("chain4")                                                           # and in a table
    c = cr.make_case("chain4")
    x = c["x_ref"]
    ang = lambda p, q, r: np.arccos(np.dot(x[p] - x[q], x[r] - x[q]) / np.linalg.norm(x[p] - x[q]) / np.linalg.norm(x[r] - x[q]))
    cis, trans = cr.d14(*(np.linalg.norm(x[k] - x[k + 1]) for k in range(3)), ang(0, 1, 2), ang(1, 2, 3))
    assert cis - 0.05 - 1e-12 <= t["lo"][0, 3] and abs(t["up"][0, 3] - min(trans + 0.05, t["up"][0, 1] + t["up"][1, 3], t["up"][0, 2] + t["up"][2, 3])) < 1e-12


@pytest.mark.parametrize("name", SMALL)
def test_gradient_agrees_with_central_differences(name):
    t = cr.case_tables(name)
    pts = cr.parity_points(name, 6)
    for (w_chi, w_4d) in cr.STAGES:
        for x in pts:
            e, g = cr.error_and_grad(t, x, w_chi, w_4d)
            num = np.zeros_like(x)
            h = 1e-6
            for idx in np.ndindex(*x.shape):
                xp, xm = x.copy(), x.copy()
                xp[idx] += h; xm[idx] -= h
                num[idx] = (cr.error_and_grad(t, xp, w_chi, w_4d, False) - cr.error_and_grad(t, xm, w_chi, w_4d, False)) / (2 * h)
            assert np.abs(num - g).max() <= 2e-6 * max(1.0, np.abs(g).max()), (name, np.abs(num - g).max(), np.abs(g).max())


def test_parity_points_cover_every_branch():
    """pairs under, inside and above their bounds for every kind of bound a case has (0 other, 1 bonded, 2 1-3, 3 planar, 4 1-4), and
    volumes under, inside and above their range"""
    for name, kinds in (("centre5", (1, 2)), ("toluene7", (0, 1, 2, 3, 4)), ("phenyl14", (0, 1, 2, 3, 4)), ("chain63", (0, 1, 2, 4))):
        c, t = cr.make_case(name), cr.case_tables(name)
        kind = cr.raw_bounds(c["n_atoms"], c["bonds"], c["x_ref"], c["elements"], c["planar_groups"])[2]
        assert sorted(set(kind[kind >= 0].tolist())) == sorted(kinds), name
        pts = cr.parity_points(name, 6)
        d2 = ((pts[:, :, None] - pts[:, None]) ** 2).sum(-1)
        for k in kinds:
            m = kind == k
            over, under = (d2 > t["up"] ** 2)[:, m], (d2 < t["lo"] ** 2)[:, m]
            assert over.any() and under.any() and (~over & ~under).any(), (name, k)
    for name in ("centre5", "phenyl14"):
        t = cr.case_tables(name)
        V = np.stack([cr.signed_volumes(p, t["centres"]) for p in cr.parity_points(name, 6)])
        assert (V < t["vol_lo"]).any() and (V > t["vol_hi"]).any() and ((V >= t["vol_lo"]) & (V <= t["vol_hi"])).any()


def test_relabelling_spread_of_the_reference():
    """the reference against itself with the atoms renamed: the yardstick of the kernel parity tests (NOTES.md)"""
    worst_e = worst_g = 0.0
    for name in cr.CASES:
        c, t = cr.make_case(name), cr.case_tables(name)
        L = c["n_atoms"]
        perm = np.random.default_rng(L).permutation(L)
        inv = np.argsort(perm)
        t2 = dict(t, lo=t["lo"][np.ix_(inv, inv)], up=t["up"][np.ix_(inv, inv)], centres=perm[t["centres"]])
        for x in cr.parity_points(name, 6):
            x2 = np.empty_like(x); x2[perm] = x
            for w_chi, w_4d in cr.STAGES:
                e, g = cr.error_and_grad(t, x, w_chi, w_4d)
                e2, g2 = cr.error_and_grad(t2, x2, w_chi, w_4d)
                if e:
                    worst_e = max(worst_e, abs(e - e2) / abs(e))
                if g.any():
                    worst_g = max(worst_g, np.abs(g2[perm] - g).max() / np.abs(g).max())
    print(f"relabelling spread: E {worst_e:.3e}, gradient {worst_g:.3e}")
    assert 0.0 < max(worst_e, worst_g) <= cr.RELABEL_SPREAD


def test_philox_start_is_the_stated_formula():
    assert cr.philox4x32((0, 0), (0, 0, 0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]     # Random123 known answer
    seed, box = (0x12345678 << 32) | 0x9abcdef0, 3.5
    s = cr.start(seed, 5, 3, box)
    for a in range(3):
        r = cr.philox4x32((0x9abcdef0, 0x12345678), (5, a, 0, 0))
        assert s[a].tolist() == [(2.0 * ((k + 0.5) * 2.0 ** -32) - 1.0) * box for k in r]
    assert (np.abs(s) < box).all() and np.abs(cr.start(seed, 6, 3, box) - s).min() > 0


@pytest.mark.parametrize("name", SMALL)
def test_reference_embeds_the_case(name):
    """Without a stereocentre every conformer is accepted.  With one, the only rejection tolerated is the trap of the module docstring
    of conformers_ref: the centre's fourth neighbour on the wrong side of the three the volume sees.  A random start puts it on either
    side with equal chance and the trap needs the wrong one, so at least half of the conformers must be accepted."""
    c, t = cr.make_case(name), cr.case_tables(name)
    res = cr.embed(t, 16, seed=11)
    n_ok = sum(r["ok"] for r in res)
    print(f"{name}: the reference accepts {n_ok} of 16")
    if not c["centres"]:
        assert n_ok == 16, [r["max_violation"] for r in res]
    else:
        assert n_ok >= 8, [r["max_violation"] for r in res]
        centre, listed = c["centres"][0][0], set(c["centres"][0][1:])
        (fourth,) = {j for b in c["bonds"] if centre in b for j in b} - listed - {centre}
    for r in res:
        assert all(s in (0, 1, 2) for s in r["status"]) and all(0 <= i <= 400 for i in r["iterations"])
        if r["ok"]:
            viol, signs, _ = cr.accept_checks(t, r["x"].astype(np.float64))
            assert viol <= 0.1 + 1e-5 and signs and np.abs(r["x4"][:, 3]).max() <= 0.1
            assert np.abs(r["x"].mean(0)).max() < 1e-5
            continue
        assert not r["x"].any()
        x3 = r["x4"][:, :3]
        d = np.linalg.norm(x3[:, None] - x3[None], axis=-1)
        short, long_ = t["lo"] - d > 0.1, d - t["up"] > 0.1
        np.fill_diagonal(short, False); np.fill_diagonal(long_, False)
        pairs = {tuple(sorted(p)) for p in np.argwhere(short).tolist()}
        assert pairs == {tuple(sorted((fourth, n))) for n in listed}, pairs          # the fourth neighbour's three 1-3 distances
        long_[centre, fourth] = long_[fourth, centre] = False                         # (its bond may be stretched with them)
        assert not long_.any() and np.abs(r["x4"][:, 3]).max() <= 1e-3
        assert (cr.signed_volumes(x3, t["centres"]) * t["vol_lo"] > 0).all()          # the volume the term sees has the right sign
    if name == "phenyl14":                                                                 # the pool is diverse
        ok = [r["x"].astype(np.float64) for r in res if r["ok"]]
        dm = [np.linalg.norm(x[:, None] - x[None], axis=-1) for x in ok]
        rms = [np.sqrt(((dm[i] - dm[j]) ** 2).mean()) for i in range(len(dm)) for j in range(i)]
        assert np.mean(rms) > 0.3, np.mean(rms)


def test_short_run_cases_keep_their_margins():
    """the GPU tests skip a short run whose reference decides within 1e-9 of a threshold: at most one may"""
    near = []
    for name, iters, kind in cr.SHORT_RUNS:
        ref = cr.short_reference(name, iters, kind)[2]
        assert sum(ref["iterations"]) > 0, name
        if min(v for _, v in ref["margins"]) < cr.MARGIN_FLOOR:
            near.append(name)
    assert len(near) <= 1, near


def test_mirror_reference_gives_mirror_centres():
    c = cr.make_case("centre5")
    m = dict(c, x_ref=c["x_ref"] * np.array([1.0, 1.0, -1.0]))
    t, tm = cr.case_tables("centre5"), cr.tables(m["n_atoms"], m["bonds"], m["x_ref"], m["elements"], m["planar_groups"], m["centres"])
    assert np.array_equal(t["lo"], tm["lo"]) and np.allclose(tm["vol_lo"], -t["vol_hi"])
    a, b = cr.embed(t, 4, seed=2), cr.embed(tm, 4, seed=2)
    for r, s in zip(a, b):
        if r["ok"] and s["ok"]:
            assert cr.signed_volumes(r["x"].astype(np.float64), t["centres"])[0] * cr.signed_volumes(s["x"].astype(np.float64), t["centres"])[0] < 0


def test_constructors_refuse():
    c = cr.make_case("centre5")
    F = pc.ConformerEnsemble.from_bonds
    args = (c["n_atoms"], c["bonds"], c["x_ref"], c["elements"])
    with pytest.raises(ValueError, match="atoms"):
        F(129, [], np.zeros((129, 3)), [6] * 129)
    with pytest.raises(ValueError, match="x_ref"):
        F(5, c["bonds"], c["x_ref"][:4], c["elements"])
    with pytest.raises(ValueError, match="bond"):
        F(5, [(0, 5)], c["x_ref"], c["elements"])
    with pytest.raises(ValueError, match="elements"):
        F(5, c["bonds"], c["x_ref"], c["elements"][:4])
    flat = c["x_ref"].copy(); flat[:, 2] = 0.0
    with pytest.raises(ValueError, match="flat"):
        F(5, c["bonds"], flat, c["elements"], centres=c["centres"])
    tiny = cr.chain(5, length=0.5)                                                         # four 0.5 A bonds cannot span a C .. C contact
    with pytest.raises(ValueError, match="lo > up"):
        F(5, tiny["bonds"], tiny["x_ref"], tiny["elements"])
    with pytest.raises(ValueError, match="lo > up"):
        cr.tables(5, tiny["bonds"], tiny["x_ref"], tiny["elements"])
    with pytest.raises(ValueError, match="centres"):
        F(*args, centres=[(0, 1, 2, 3)] * 65)
    with pytest.raises(ValueError, match="centre"):
        F(*args, centres=[(0, 1, 2, 7)])
    ens = F(*args, centres=c["centres"])
    T = pc.ConformerEnsemble.from_tables
    T(ens.lo, ens.up, ens.centres, ens.vol_lo, ens.vol_hi)
    with pytest.raises(ValueError, match="square"):
        T(ens.lo[:4], ens.up)
    with pytest.raises(ValueError, match="symmetric"):
        lo = ens.lo.copy(); lo[0, 1] += 0.001
        T(lo, ens.up)
    with pytest.raises(ValueError, match="lo <= up"):
        T(ens.up * 1.1, ens.up)
    with pytest.raises(ValueError, match="volume bounds"):
        T(ens.lo, ens.up, ens.centres)
    with pytest.raises(ValueError, match="one sign"):
        T(ens.lo, ens.up, ens.centres, -np.abs(ens.vol_lo), np.abs(ens.vol_hi))
    with pytest.raises(ValueError, match="twice"):
        T(ens.lo, ens.up, [(0, 1, 1, 2)], ens.vol_lo, ens.vol_hi)
    with pytest.raises(ValueError, match="atoms"):
        T(np.zeros((129, 129)), np.zeros((129, 129)))
    with pytest.raises(ValueError, match="conformers"):
        ens.embed(4097, 0)
    with pytest.raises(ValueError, match="keep"):
        ens.embed(4, 0, keep="all")
    with pytest.raises(ValueError, match="pos4"):
        import torch
        ens.error(torch.zeros(2, 4, 4), 1.0, 0.1)
