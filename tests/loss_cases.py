"""The cases tests/test_loss_kernels_gpu.py runs through the ten launchers of csrc/loss.hip and csrc/loss_grad.hip, with their
float64 references (tests/loss_ref.py) - CPU only, built once per process and never modified.  tests/test_loss_ref_cpu.py asserts
on the reference alone what the GPU comparison relies on (margins to the clamp radius and the bin edges, the tie-allowance cap,
the margin of the weighted MSE to its clamp) and that the shapes reach the branches named below.

Inputs are seeded and use uniform draws and correctly rounded arithmetic only (no libm call decides a bit), so every machine
builds the same arrays.  x_gt is a random walk of 1.5 A steps (distances on both sides of the 15 A clamp); x_denoised is x_gt plus
noise whose size differs per sample (0.05 .. 2 A), with no pair left at a sign tie (see `untie`); centre / pseudo-beta indices are a non-monotone map into the atoms; t_hat spans
0.4 .. 40.  Among the pairs of a few hundred atoms some always lie within a relative 1e-5 of the clamp radius or a bin edge; as
synthetic.clear_thresholds does for the fixtures, the offending atoms are redrawn (moved by ~0.01 A from the same stream) until the
closest approach exceeds 2e-5.

Smooth lDDT (LT = 64 atoms per tile, LBC = 12 samples per forward block, GB = 4 samples / GQ = 4 column tiles per gradient block):
    A    B    forward                                        gradient
    1    1    one tile, one atom, the pair (0, 0) only       1 tile < GQ: waves with tj >= nt from the first trip; B % 4 = 1
   63    2    one ragged tile                                B % 4 = 2
   64    3    exactly one tile                               B % 4 = 3
   65    4    second tile holds one atom; off-diagonal x 2   2 tiles < GQ
  128    5    two full tiles                                 second sample block holds one sample
  129   11    3 tiles, chunk of 11                           3 tiles; B % 4 = 3 with three blocks
  257   12    5 tiles, a full chunk                          5 tiles: second trip with one live tile
  320   13    second chunk holds one sample                  5 tiles, four sample blocks, the last with one sample
  513   25    9 tiles, 45 pairs, 3 chunks (12, 12, 1)        9 tiles: third trip with one live tile; the largest gradient case
   70   65    smooth_lddt_final's second block of 64 samples 17 sample blocks
 2881    1    46 tiles, 1081 pairs: second trip of `p += 1024` in smooth_lddt_final (forward only)
  half        130 x 5 with x_exists = 0.5 on atoms 3 and 64 (mask products 0.5 and 0.25)
  tile-off    200 x 5 with atoms 64 .. 127 masked out (x_exists = 0)
  far-tile    192 x 5 with atoms 128 .. 191 moved 200 A away: every pair of tiles (0, 2), (1, 2) beyond the clamp, `act == 0`
  near-in     130 x 2, predicted atoms 10 and 11 at the origin 1e-20 apart along x (gradient only)
  near-edge   130 x 2, predicted atoms 63 and 64 likewise: a pair across the tile edge (gradient only)

Centre pairs (one wave per (token, sample), lanes over j in steps of 64; 4 samples per block; scatter blocks of 256 tokens):
    T    B
    1    1    one token, bonded to itself and both key and ligand: bond term 0 by construction, key term eps(0)^2
   63    3    lane loop one ragged trip; no bond and no key residue: both terms 0, denominators eps only
   64    4    lane loop exactly one trip; asymmetric bonds; token 5 both key and ligand
   65    5    second trip with one lane; asymmetric bonds; tokens 7 and 40 (bonded, key / ligand) predicted at one point
  130    9    third trip ragged; asymmetric bonds; B % 4 = 1 with three blocks
  257    2    second scatter block, second trip of the T-loops of the coefficient kernel, T * T = 66049 > 256 * 256;
              tokens 3, 100 and 256 share one centre atom (3 and 256 in different scatter blocks)

Distogram (256 pairs per block, LDS row stride no_bins | 1): no_bins x T from {2, 3, 38, 39, 62, 63} x {1, 15, 16, 17, 33}, every
value at least twice; T = 16 gives T * T = 256 exactly, T = 33 five blocks.  Where T >= 15: token 2 is masked (x_exists = 0) with
logits 1e30 in its row and column, token 4 has x_exists = 0.5 (mask 0.5 and 0.25: m, m^2 and m^3 differ).

Weighted MSE (one block per sample, `b += 256` loops in the second pass): (A, B) = (1, 1), (63, 2), (257, 3), (40, 257), (40, 300),
each with the residual scaled to a pre-clamp value of about 0.9e4 ("lo": the gradient passes) and 1.1e4 ("hi": value 1e4,
gradient 0); weights hold zeros.
"""
import functools
import types

import numpy as np

import loss_ref as lr

CLAMP, SD_BOND, SD_KEY, EPS = 15.0, 16.0, 8.0, 1e-9
MIN_BIN, MAX_BIN = 3.25, 50.75
MARGIN = 2e-5                 # the cases are built to this; the condition asserted is 1e-5
TOL = 2e-5                    # the kernels' bar (tests/test_loss_gpu.py, tests/test_loss_grad_gpu.py)

SMOOTH_SHAPES = ((1, 1), (63, 2), (64, 3), (65, 4), (128, 5), (129, 11), (257, 12), (320, 13), (513, 25), (70, 65))
SMOOTH_SPECIAL = ("half", "tile-off", "far-tile")
SMOOTH_NEAR = ("near-in", "near-edge")
SMOOTH_FWD_ONLY = ((2881, 1),)
CENTRE_SHAPES = ((1, 1), (63, 3), (64, 4), (65, 5), (130, 9), (257, 2))
DISTO_SHAPES = ((2, 1), (2, 16), (3, 15), (3, 33), (38, 16), (38, 17), (39, 1), (39, 33), (62, 15), (62, 17), (63, 16), (63, 33),
                (63, 17))
MSE_SHAPES = ((1, 1), (63, 2), (257, 3), (40, 257), (40, 300))

SMOOTH_GRAD = tuple(f"{a}x{b}" for a, b in SMOOTH_SHAPES) + SMOOTH_SPECIAL + SMOOTH_NEAR
SMOOTH_FWD = tuple(f"{a}x{b}" for a, b in SMOOTH_SHAPES + SMOOTH_FWD_ONLY) + SMOOTH_SPECIAL
CENTRE = tuple(f"{t}x{b}" for t, b in CENTRE_SHAPES)
DISTO = tuple(f"{n}x{t}" for n, t in DISTO_SHAPES)
MSE = tuple(f"{a}x{b}-{s}" for a, b in MSE_SHAPES for s in ("lo", "hi"))


def tile_pairs(A):
    nt = -(-A // 64)
    return nt * (nt + 1) // 2


def _rng(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return np.random.RandomState(seed)


def _normal(rng, *shape):
    """mean 0, variance 1, from twelve uniforms (additions only)"""
    return rng.random_sample((12,) + shape).sum(0) - 6.0


def walk(rng, A, step=1.5):
    d = rng.random_sample((A, 3)) * 2 - 1
    d *= step / np.sqrt((d * d).sum(1))[:, None]
    x = np.cumsum(d, 0)
    return (x - x.mean(0)).astype(np.float32)


def clear(x, rng, clamp=None, pb=None, b2=None):
    """redraw the atoms of x [A,3] fp32 that sit in a pair within MARGIN of the clamp radius or (pseudo-beta atoms) a bin edge"""
    x = x.copy()
    for _ in range(200):
        x64 = x.astype(np.float64)
        bad = set()
        if clamp is not None:
            d = lr.pairdist(x64)
            bad |= set(np.nonzero(np.abs(d - clamp) < MARGIN * clamp)[1].tolist())
        if pb is not None:
            d2 = lr.pairdist2(x64[pb])
            bad |= set(pb[np.nonzero((np.abs(d2[..., None] - b2) < MARGIN * b2).any(-1))[1]].tolist())
        if not bad:
            return x
        for a in sorted(bad):
            x[a] += (0.02 * (rng.random_sample(3) - 0.5)).astype(np.float32)
    raise RuntimeError("could not clear the decision thresholds")


def noisy(rng, xg, B):
    """x_gt + noise of a size that differs per sample (0.05 .. 2 A)"""
    s = 0.05 + 1.95 * (np.arange(B) / (B - 1.0)) ** 2 if B > 1 else np.array([0.7])
    return (xg[None].astype(np.float64) + s[rng.permutation(B)][:, None, None] * _normal(rng, B, xg.shape[0], 3)).astype(np.float32)


def untie(xd, xg, pairmask, rng, atoms=None, fixed=()):
    """move (by ~0.01 A) atoms of x_denoised [B,A,3] until no pair of `pairmask` [n,n] (over `atoms`, default all) has
    0 < d_pred and |d_pred - d_gt| < 2 tau: below tau two fp32 evaluations may disagree on sign(d_pred - d_gt), and a flipped sign
    moves a pair by TWICE its contribution while the allowance holds it once (NOTES.md, "PhysDockLoss backward"); the fixture tests
    absorb that in 4 e_ref, the kernel-level bar has no such term, so the cases carry no tie at all"""
    idx = np.arange(xd.shape[1]) if atoms is None else np.asarray(atoms)
    dgt = lr.pairdist(xg[idx].astype(np.float64))
    thr = 2 * lr.tau_of(xd, xg)
    for b in range(xd.shape[0]):
        for _ in range(200):
            D = lr.pairdist(xd[b][idx].astype(np.float64))
            bad = np.argwhere(pairmask & (D > 0) & (np.abs(D - dgt) < thr))
            if not len(bad):
                break
            for i in sorted({int(i) if idx[i] not in fixed else int(j) for i, j in bad if i < j}):
                xd[b, idx[i]] += (0.02 * (rng.random_sample(3) - 0.5)).astype(np.float32)
        else:
            raise RuntimeError("could not clear the sign ties")
    assert lr.tau_of(xd, xg) <= thr / 2
    return xd


def t_hat(rng, B):
    """spread over two decades, 0.4 .. 40"""
    u = (np.arange(B) + 0.5) / B
    return (0.4 + 39.6 * u[rng.permutation(B)] ** 3).astype(np.float32)


def index_map(rng, A, T):
    """T distinct atoms in no particular order"""
    m = rng.permutation(A)[:T].astype(np.int64)
    if T > 2 and (np.diff(m) > 0).all():
        m[[0, 1]] = m[[1, 0]]
    return m


# ------------------------------------------------------------------ smooth lDDT
@functools.lru_cache(maxsize=None)
def smooth(name):
    special = {"half": (130, 5), "tile-off": (200, 5), "far-tile": (192, 5), "near-in": (130, 2), "near-edge": (130, 2)}
    A, B = special[name] if name in special else (int(v) for v in name.split("x"))
    rng = _rng(1, A, B, sorted(special).index(name) + 1 if name in special else 0)
    xg = walk(rng, A)
    ex = np.ones(A, np.float32)
    if A >= 63 and name not in special:
        ex[[5, A - 2]] = 0.0
    if name == "half":
        ex[[3, 64]] = 0.5
    if name == "tile-off":
        ex[64:128] = 0.0
    if name == "far-tile":
        xg[128:] += np.float32([200.0, 0.0, 0.0])
    near = {"near-in": (10, 11), "near-edge": (63, 64)}.get(name)
    if near:
        xg = (xg.astype(np.float64) - xg[near[0]].astype(np.float64)).astype(np.float32)      # atom i of x_gt at the origin
    xg = clear(xg, rng, clamp=CLAMP)
    xd = noisy(rng, xg, B)
    if near:
        xd[:, near[0]] = 0.0
        xd[:, near[1]] = np.float32([1e-20, 0.0, 0.0])
    xd = untie(xd, xg, lr.lddt_mask(xg, ex, CLAMP)[1] > 0, rng, fixed=near or ())
    return types.SimpleNamespace(name=name, A=A, B=B, x_gt=xg, x_exists=ex, x_denoised=xd, near=near)


@functools.lru_cache(maxsize=None)
def smooth_ref(name, grad=True):
    c = smooth(name)
    r = types.SimpleNamespace(value=lr.smooth_lddt(c.x_denoised, c.x_gt, c.x_exists, CLAMP), clamp_margin=lr.clamp_margin(c.x_gt, CLAMP))
    if grad:
        r.tau = lr.tau_of(c.x_denoised, c.x_gt)
        r.g, r.allow = lr.smooth_lddt_grad(c.x_denoised, c.x_gt, c.x_exists, CLAMP, r.tau)
    return r


# ------------------------------------------------------------------ centre pairs
@functools.lru_cache(maxsize=None)
def centre(name):
    T, B = (int(v) for v in name.split("x"))
    A = T + 7
    rng = _rng(2, T, B)
    xg = walk(rng, A)
    ci = index_map(rng, A, T)
    bonds = (rng.random_sample((T, T)) < min(0.08, 4.0 / T)).astype(np.float32)
    np.fill_diagonal(bonds, 0.0)
    key, lig = np.zeros(T, np.float32), np.zeros(T, np.float32)
    if T >= 63:
        p = rng.permutation(T)
        key[p[:6]] = 1.0
        lig[p[6:14]] = 1.0
    note = ""
    if T == 1:
        bonds[0, 0] = key[0] = lig[0] = 1.0
    if T == 63:
        bonds[:] = 0.0
        key[:] = 0.0
    if T == 64:
        key[5] = lig[5] = 1.0
    if T == 257:
        ci[100] = ci[256] = ci[3]
        key[3], lig[256], lig[100] = 1.0, 1.0, 1.0
        bonds[3, 100] = bonds[256, 7] = 1.0
    xd = noisy(rng, xg, B)
    if T == 65:
        bonds[7, 40], bonds[40, 7] = 1.0, 0.0
        key[7], lig[40] = 1.0, 1.0
        xd[:, ci[40]] = xd[:, ci[7]]
    if T >= 64:
        assert (bonds != bonds.T).any()
    km = np.outer(key, lig)
    xd = untie(xd, xg, (km + km.T) > 0, rng, atoms=ci, fixed=(ci[7], ci[40]) if T == 65 else ())
    return types.SimpleNamespace(name=name, T=T, A=A, B=B, x_gt=xg, x_denoised=xd, centre=ci, token_bonds=bonds, is_key_res=key,
                                 is_ligand=lig, t_hat=t_hat(rng, B))


def centre_args(c):
    return (c.x_denoised, c.x_gt, c.centre, c.token_bonds, c.is_key_res, c.is_ligand, c.t_hat, SD_BOND, SD_KEY, EPS)


@functools.lru_cache(maxsize=None)
def centre_ref(name):
    c = centre(name)
    r = types.SimpleNamespace(tau=lr.tau_of(c.x_denoised, c.x_gt))
    r.bond, r.key = lr.centre_pairs(*centre_args(c))
    r.g_bond, r.g_key, r.allow = lr.centre_pairs_grad(*centre_args(c), r.tau)
    return r


# ------------------------------------------------------------------ distogram
@functools.lru_cache(maxsize=None)
def disto(name):
    nb, T = (int(v) for v in name.split("x"))
    A = 4 * T + 5
    rng = _rng(3, nb, T)
    xg = walk(rng, A)
    pb = index_map(rng, A, T)
    b2 = (np.linspace(MIN_BIN, MAX_BIN, nb - 1, dtype=np.float32) ** 2).astype(np.float32)     # loss.distogram_boundaries_sq
    xg = clear(xg, rng, pb=pb, b2=b2.astype(np.float64))
    ex = np.ones(A, np.float32)
    p = (3.0 * _normal(rng, T, T, nb)).astype(np.float32)
    if T >= 15:
        ex[pb[2]] = 0.0
        p[2, :, :] = p[:, 2, :] = 1e30
        ex[pb[4]] = 0.5
    elif nb == 39:
        ex[pb[0]] = 0.5
    return types.SimpleNamespace(name=name, no_bins=nb, T=T, A=A, x_gt=xg, x_exists=ex, pseudo_beta=pb, boundaries_sq=b2, p_distogram=p)


def disto_args(c):
    return (c.p_distogram, c.x_gt, c.x_exists, c.pseudo_beta, c.boundaries_sq, c.no_bins)


@functools.lru_cache(maxsize=None)
def disto_ref(name):
    c = disto(name)
    return types.SimpleNamespace(value=lr.distogram(*disto_args(c)), g=lr.distogram_grad(*disto_args(c)),
                                 bin_margin=lr.bin_margin(c.x_gt, c.pseudo_beta, c.boundaries_sq))


# ------------------------------------------------------------------ weighted MSE
@functools.lru_cache(maxsize=None)
def mse(name):
    shape, side = name.split("-")
    A, B = (int(v) for v in shape.split("x"))
    rng = _rng(4, A, B)
    al = (walk(rng, A)[None].astype(np.float64) + 0.3 * _normal(rng, B, A, 3)).astype(np.float32)
    w = np.float32([0.0, 1.0, 6.0, 11.0])[rng.randint(0, 4, A)]
    w[0] = 6.0
    if A > 1:
        w[1] = 0.0
    t = t_hat(rng, B)
    r0 = _normal(rng, B, A, 3)
    v0 = lr.weighted_mse_pre_clamp(al.astype(np.float64) + r0, al, w, t)
    s = np.sqrt({"lo": 0.9e4, "hi": 1.1e4}[side] / v0)
    xd = (al.astype(np.float64) + s * r0).astype(np.float32)
    return types.SimpleNamespace(name=name, A=A, B=B, side=side, x_denoised=xd, x_gt_aligned=al, weights=w, t_hat=t)


def mse_args(c):
    return (c.x_denoised, c.x_gt_aligned, c.weights, c.t_hat)


@functools.lru_cache(maxsize=None)
def mse_ref(name):
    c = mse(name)
    return types.SimpleNamespace(pre_clamp=lr.weighted_mse_pre_clamp(*mse_args(c)), value=lr.weighted_mse(*mse_args(c)),
                                 g=lr.weighted_mse_grad(*mse_args(c)))


# ------------------------------------------------------------------ probes: one atom of one sample moved by 1 A, else x_denoised = x_gt
PROBE_SMOOTH = types.SimpleNamespace(A=66, B=14, atoms=(0, 63, 64, 65), samples=(0, 11, 13))       # 11: last sample of the first chunk of 12
PROBE_CENTRE = types.SimpleNamespace(T=66, B=6, tokens=(0, 63, 64, 65), samples=(0, 3, 5))         # 3: last sample of the first block of 4


@functools.lru_cache(maxsize=None)
def probe_smooth_base():
    P = PROBE_SMOOTH
    rng = _rng(5, P.A, P.B)
    xg = clear(walk(rng, P.A), rng, clamp=CLAMP)
    return types.SimpleNamespace(A=P.A, B=P.B, x_gt=xg, x_exists=np.ones(P.A, np.float32))


def probe_smooth_xd(atom=None, sample=None):
    c = probe_smooth_base()
    xd = np.repeat(c.x_gt[None], c.B, 0).copy()
    if atom is not None:
        xd[sample, atom, 0] += np.float32(1.0)
    return xd


@functools.lru_cache(maxsize=None)
def probe_smooth_ref(atom=None, sample=None):
    c = probe_smooth_base()
    return lr.smooth_lddt(probe_smooth_xd(atom, sample), c.x_gt, c.x_exists, CLAMP)


@functools.lru_cache(maxsize=None)
def probe_centre_base():
    P = PROBE_CENTRE
    rng = _rng(6, P.T, P.B)
    A = P.T + 7
    c = types.SimpleNamespace(T=P.T, A=A, B=P.B, x_gt=walk(rng, A), centre=index_map(rng, A, P.T), t_hat=t_hat(rng, P.B))
    c.token_bonds = (rng.random_sample((P.T, P.T)) < 0.06).astype(np.float32)
    np.fill_diagonal(c.token_bonds, 0.0)
    c.is_key_res, c.is_ligand = np.zeros(P.T, np.float32), np.zeros(P.T, np.float32)
    p = rng.permutation(P.T)
    c.is_key_res[p[:5]] = 1.0
    c.is_ligand[p[5:12]] = 1.0
    # every probed token is bonded in one orientation only and takes part in the key / ligand mask
    c.token_bonds[0, 9], c.token_bonds[9, 0] = 1.0, 0.0
    c.token_bonds[20, 63], c.token_bonds[63, 20] = 1.0, 0.0
    c.token_bonds[64, 30], c.token_bonds[30, 64] = 1.0, 0.0
    c.token_bonds[65, 0], c.token_bonds[0, 65] = 1.0, 0.0
    c.is_key_res[[0, 64]] = 1.0
    c.is_ligand[[63, 65]] = 1.0
    return c


def probe_centre_xd(token=None, sample=None):
    c = probe_centre_base()
    xd = np.repeat(c.x_gt[None], c.B, 0).copy()
    if token is not None:
        xd[sample, c.centre[token], 0] += np.float32(1.0)
    return xd


@functools.lru_cache(maxsize=None)
def probe_centre_ref(token=None, sample=None):
    c = probe_centre_base()
    return lr.centre_pairs(probe_centre_xd(token, sample), c.x_gt, c.centre, c.token_bonds, c.is_key_res, c.is_ligand, c.t_hat,
                           SD_BOND, SD_KEY, EPS)
