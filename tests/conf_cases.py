"""The cases of tests/test_conf_kernels_gpu.py: seeded numpy inputs for the nine launchers of csrc/confidence_loss.hip and
csrc/metrics.hip, each the smallest shape that reaches a branch the g17 / g18 fixtures (T <= 221, 50 and 64 bins, min_bin 0)
never reach.  tests/test_conf_ref_cpu.py checks, without a GPU, that every case holds its margins and contains what its line
here promises, and that a reference with the fault a case was chosen for differs from the right one by more than the GPU bar.

Margins (those of the g17 / g18 fixtures), held by construction: after drawing, every decision quantity is evaluated in float64
on the fp32 inputs and the offending atoms / tokens are redrawn until
  |d_pred - d_gt| is >= 1e-4 A from 0.5 / 1 / 2 / 4, d_gt >= 1e-4 A from 15 / 30, every PDE / PAE error >= 1e-4 A from an inner bin
  edge, every frame cosine >= 1e-5 from 0.906308, |w1 +- w2| >= 0.1, every distance of two eligible atoms >= 1e-4 A from 1.1,
  the argmax gap of per_alignment_i w_i >= 1e-4 (the tie cases apart), a fractional sum of weights >= 1e-3 from an integer.
No element is excluded from a comparison.

pd_lddt_atoms (B, A, T), LC = 256 token centres per LDS round
  257     (2, 300, 257)  one full round and a round of one token: the second round's leading barrier, n < LC
  513     (2, 600, 513)  two full rounds and one token; three atom tiles, the last one partial
  256     (1, 256, 256)  exact fit of one round and one atom tile; the centres are a permutation of all atoms
  1       (3, 1, 1)      one atom that is its own centre: lDDT 1.0 in every pose
  mixed   (2, 150, 70)   DNA / RNA tokens (30 A cut), ligand tokens (weight 0), one atom beyond 30 A of every token: NaN
  (257, 513 and mixed all carry DNA, RNA and ligand tokens; the last token is always a protein token)
pd_conf_frames, T in 1, 256, 257, 600 (256 lanes per block): one block; exact fit; a second block with one live lane; three
  blocks.  From T = 256 on a quarter of the frames is invalid (angle 8 .. 22 degrees) and token 1 has frame atoms a = b (w1 = 0,
  finite through the + 1e-6 inside the norms).
pd_conf_loss_plddt (A, nb), 16 rows per wave, 64 per block
  1x50 one row; 15x1 one bin (loss exactly 0); 16x37 a full wave, odd nb; 17x64 a second wave with one row, every lane a bin;
  64x50 a full block; 65x50 a second block with one row; 437x64 seven blocks, the last partial.
  From A = 15 on: row 0 lDDT NaN (bin 0), row 1 lDDT 1.0 (clamped to nb - 1), row 2 x_exists 0, row 3 lDDT 0.6 (0.6 * 50 lands on
  an integer in fp32), row 4 NaN and masked, row 5 logits up to 32.
pd_conf_loss_pairs, both modes, (T, nb, min_bin, max_bin), A = 3 T (token t = atoms 3t, 3t+1, 3t+2, centre 3t+1)
  1x64 one pair; 8x1 one bin; 9x33 odd nb, min_bin 2 and max_bin 30 with errors below 2 and above 30 (both clamps of to_bin);
  257x64 66049 rows = 1032 blocks and one row, i = r / T and j = r % T over rows of 257.
  From T = 8 on: one token 45 A away in the pose (errors above max_bin), a masked centre atom, tokens whose predicted frame alone
  and whose ground-truth frame alone is invalid (PAE error 0 for the whole row).
pd_metrics_plddt (P, A, nb): 1x1x50 one row, scalar loads; 3x61x48 vector loads with idle lanes (4 sub >= 48); 2x65x64 vector
  loads, a second block; 1x64x7 scalar, two live lanes per row; 2x257x50 scalar, five blocks.  The 64-bin input is also read
  through a view one float past a 16-byte boundary (scalar loads at nb % 4 == 0).
pd_metrics_pae_tm (P, T, nb) and the launch it reaches (`geometry`: nsplit, chunk, most iterations of a wave)
  32x65x64  (1, 128, 2)  unsplit rows, the second iteration holds one pair
  8x257x64  (1, 320, 5)  unsplit rows of five iterations; tm_final lanes with two rows (0 and 256)
  1x257x64  (5, 64, 1)   the same T fully split; its logits are slice 5 of 8x257x64
  1x65x50   (2, 64, 1)   scalar loads, split
  2x40x48   (1, 64, 1)   vector loads with idle lanes; fractional weights
  1x17x7    (1, 64, 1)   scalar loads, two live lanes per pair; sum of weights below 19 (the clip of d0)
  Every case: three chains, tokens of weight 0, a best row per set (rows 0, 3, 64, 130, 200, 255 and 256 among them).
pd_metrics_clash (B, A, nc), 256 atoms per tile: 1x1x1; 2x257x3 two tiles, the second one atom; 3x513x64 three tiles, the
  most chains.  Chain ids -1 and nc, atoms with a_mask 0 and 0.5, ligand atoms; the poses are one cloud at several scales."""
import functools
from types import SimpleNamespace

import numpy as np

import conf_ref as cr

MARGIN, COS_MARGIN, MIN_BISECTOR, GAP_MARGIN, SUM_MARGIN = 1e-4, 1e-5, 0.1, 1e-4, 1e-3
TOL = 2e-5                                  # the bar of tests/test_confidence_loss_gpu.py on cross entropies and their gradients
BOX = 36.0

LDDT = {"257": (2, 300, 257), "513": (2, 600, 513), "256": (1, 256, 256), "1": (3, 1, 1), "mixed": (2, 150, 70)}
FRAMES = (1, 256, 257, 600)
PLDDT_LOSS = ((1, 50), (15, 1), (16, 37), (17, 64), (64, 50), (65, 50), (437, 64))
PAIRS = {"1x64": (1, 64, 0.0, 32.0), "8x1": (8, 1, 0.0, 32.0), "9x33": (9, 33, 2.0, 30.0), "257x64": (257, 64, 0.0, 32.0)}
MODES = {"pde": 0, "pae": 1}
PLDDT = ((1, 1, 50), (3, 61, 48), (2, 65, 64), (1, 64, 7), (2, 257, 50))
PAE_TM = {"32x65x64": (32, 65, 64), "8x257x64": (8, 257, 64), "1x257x64": (1, 257, 64), "1x65x50": (1, 65, 50),
          "2x40x48": (2, 40, 48), "1x17x7": (1, 17, 7)}
PAE_TM_GEOMETRY = {"32x65x64": (1, 128, 2), "8x257x64": (1, 320, 5), "1x257x64": (5, 64, 1), "1x65x50": (2, 64, 1),
                   "2x40x48": (1, 64, 1), "1x17x7": (1, 64, 1)}
BEST_ROWS = {"32x65x64": [(7 * p + 3) % 65 for p in range(31)] + [64], "8x257x64": [5, 130, 64, 255, 3, 256, 200, 0],
             "1x257x64": [256], "1x65x50": [64], "2x40x48": [39, 16], "1x17x7": [9]}
SLICE = 5                                   # 1x257x64 is this slice of 8x257x64
CLASH = {"1x1x1": (1, 1, 1), "2x257x3": (2, 257, 3), "3x513x64": (3, 513, 64)}


def name_of(shape):
    return "x".join(str(s) for s in shape)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------ pd_lddt_atoms
def lddt_margins(c):
    """closest approaches of the decisions of cal_lddt, and the offending (atom, token) pairs"""
    xp, xg = c.x_pred.astype(np.float64), c.x_gt.astype(np.float64)
    d_gt = cr.norm(xg[:, None] - xg[c.centre][None])
    d_lm = np.abs(cr.norm(xp[:, :, None] - xp[:, c.centre][:, None]) - d_gt[None])
    near_gt = np.minimum(np.abs(d_gt - 15.0), np.abs(d_gt - 30.0))
    near_lm = np.min([np.abs(d_lm - t) for t in (0.5, 1.0, 2.0, 4.0)], axis=0).min(0)
    return {"d_gt": float(near_gt.min()), "d_lm": float(near_lm.min())}, np.nonzero((near_gt < MARGIN) | (near_lm < MARGIN))


@functools.lru_cache(None)
def lddt(name):
    B, A, T = LDDT[name]
    rng = np.random.RandomState(1000 + A)
    c = SimpleNamespace(name=name, B=B, A=A, T=T)
    c.centre = (rng.permutation(A)[:T] if name == "256" else np.sort(rng.permutation(A)[:T])).astype(np.int64)
    kind = rng.choice(4, T, p=[0.6, 0.15, 0.15, 0.1]) if name in ("257", "513", "mixed") else np.zeros(T, np.int64)
    kind[-1] = 0
    c.is_dna, c.is_rna, c.is_polymer = f32(kind == 1), f32(kind == 2), f32(kind != 3)
    sigma = np.asarray([0.4, 1.5, 0.9][:B])[:, None]
    far = [int(np.setdiff1d(np.arange(A), c.centre)[0])] if name == "mixed" else []
    c.far = far
    c.x_gt, c.x_pred = np.zeros((A, 3), np.float32), np.zeros((B, A, 3), np.float32)

    def draw(a):
        c.x_gt[a] = (150.0 if a in far else 0.0) + rng.uniform(0, BOX, 3)
        c.x_pred[:, a] = c.x_gt[a][None] + sigma * rng.randn(B, 3)
    for a in range(A):
        draw(a)
    for _ in range(200):
        c.closest, (bad, _) = lddt_margins(c)
        if not len(bad):
            return c
        for a in sorted(set(bad.tolist())):
            draw(a)
    raise RuntimeError(f"lddt {name}: could not clear the thresholds")


@functools.lru_cache(None)
def lddt_ref(name):
    c = lddt(name)
    return cr.lddt(c.x_pred, c.x_gt, c.centre, c.is_dna, c.is_rna, c.is_polymer)[0]


# ------------------------------------------------------------------ frames
def triple(rng, theta, box):
    """three atoms a, b, c with the angle theta at b, bonds of 1.2 .. 1.6 A"""
    b = rng.uniform(0, box, 3)
    u = rng.randn(3)
    u /= np.linalg.norm(u)
    v = np.cross(u, rng.randn(3))
    v /= np.linalg.norm(v)
    r1, r2 = rng.uniform(1.2, 1.6, 2)
    return np.stack([b + r1 * u, b, b + r2 * (np.cos(theta) * u + np.sin(theta) * v)])


def angle(rng, valid):
    return np.deg2rad(rng.uniform(30, 165) if valid else rng.uniform(8, 22))


def frame_margins(x, ids):
    _, cos, bis = cr.frames(x, ids)
    return np.abs(cos - cr.COS_VALID), bis.min(0)


@functools.lru_cache(None)
def frames(T):
    rng = np.random.RandomState(2000 + T)
    c = SimpleNamespace(name=str(T), T=T, A=3 * T)
    perm = rng.permutation(T)
    c.ids = [np.ascontiguousarray(3 * perm + k, dtype=np.int64) for k in range(3)]
    if T > 1:
        c.ids[0][1] = c.ids[1][1]                                   # token 1: a = b
    want = rng.uniform(size=T) >= (0.25 if T > 1 else 0.0)
    c.x = np.zeros((c.A, 3), np.float32)
    bad = np.arange(T)
    for _ in range(50):
        for t in bad:
            c.x[3 * perm[t]:3 * perm[t] + 3] = triple(rng, angle(rng, want[t]), BOX)
        dcos, bis = frame_margins(c.x, c.ids)
        bad = np.nonzero((dcos < COS_MARGIN) | (bis < MIN_BISECTOR))[0]
        if not len(bad):
            c.closest = {"cos": float(dcos.min()), "bisector": float(bis.min())}
            return c
    raise RuntimeError(f"frames {T}: could not clear the thresholds")


@functools.lru_cache(None)
def frames_ref(T):
    """(frames [T,13] float64, the same from a plain fp32 evaluation)"""
    c = frames(T)
    return cr.frames(c.x, c.ids)[0], cr.frames(c.x, c.ids, np.float32)[0]


# ------------------------------------------------------------------ pd_conf_loss_plddt
def logits(rng, shape):
    return f32(rng.uniform(-4, 4, shape))


@functools.lru_cache(None)
def plddt_loss(A, nb):
    rng = np.random.RandomState(3000 + 100 * A + nb)
    c = SimpleNamespace(name=f"{A}x{nb}", A=A, nb=nb, logits=logits(rng, (A, nb)), lddt=f32(rng.uniform(0, 1, A)), x_exists=np.ones(A, np.float32))
    if A >= 15:
        c.lddt[[0, 4]] = np.nan
        c.lddt[1], c.lddt[3] = 1.0, 0.6
        c.x_exists[[2, 4]] = 0
        c.logits[5] *= 8
    c.bins = cr.plddt_bins(c.lddt, nb)
    return c


@functools.lru_cache(None)
def plddt_loss_ref(A, nb):
    """((loss, rows, gradient at scale 1) in float64, the same in fp32)"""
    c = plddt_loss(A, nb)
    return cr.ce(c.logits, c.bins, c.x_exists), cr.ce(c.logits, c.bins, c.x_exists, dtype=np.float32)


# ------------------------------------------------------------------ pd_conf_loss_pairs
def pair_errors(c, dtype=np.float64):
    return {"pde": cr.pde_error(c.x_pred0, c.x_gt, c.centre, dtype), "pae": cr.pae_error(c.x_pred0, c.x_gt, c.centre, c.frames_pred, c.frames_gt, dtype)}


@functools.lru_cache(None)
def pairs(name):
    T, nb, lo, hi = PAIRS[name]
    rng = np.random.RandomState(4000 + 10 * T + nb)
    c = SimpleNamespace(name=name, T=T, A=3 * T, nb=nb, min_bin=lo, max_bin=hi, centre=np.arange(T, dtype=np.int64) * 3 + 1)
    c.ids = [np.arange(T, dtype=np.int64) * 3 + k for k in range(3)]
    box, shifts = (BOX, (0.3, 1.5, 4.0)) if T > 100 else (14.0, (0.5, 4.0, 9.0))      # few pairs: spread their errors over the bins
    # category of a token: 0 both frames valid, 1 the predicted frame alone invalid, 2 the ground-truth frame alone, 3 both
    cat = rng.choice(4, T, p=[0.7, 0.1, 0.1, 0.1]) if T >= 8 else np.zeros(T, np.int64)
    far = np.zeros(T, bool)
    if T >= 8:
        cat[:4] = (0, 1, 2, 3)
        far[5] = True
    c.category, c.far_token = cat, far
    c.x_gt, c.x_pred0 = np.zeros((c.A, 3), np.float32), np.zeros((c.A, 3), np.float32)

    def draw(t):
        # the pose is the ground-truth triple with its own angle, moved as a whole by one of `shifts` A (45 A more for the far
        # token) and by 0.3 A per atom; a frame the noise turned the other way is drawn again, so that the categories hold exactly
        while True:
            g = triple(rng, angle(rng, cat[t] in (0, 1)), box)
            b, u, w = g[1], g[0] - g[1], g[2] - g[1]
            th = angle(rng, cat[t] in (0, 2))
            v = w - (w @ u) / (u @ u) * u
            p = np.stack([b + u, b, b + np.linalg.norm(w) * (np.cos(th) * u / np.linalg.norm(u) + np.sin(th) * v / np.linalg.norm(v))])
            p = p + 0.3 * rng.randn(3, 3) + rng.choice(shifts) * rng.randn(3)[None, :] + (45.0 if far[t] else 0.0)
            c.x_gt[3 * t:3 * t + 3], c.x_pred0[3 * t:3 * t + 3] = g, p
            one = [np.arange(3 * t + k, 3 * t + k + 1) for k in range(3)]
            ok = []
            for x, valid in ((c.x_gt, cat[t] in (0, 1)), (c.x_pred0, cat[t] in (0, 2))):
                fr, cos, bis = cr.frames(x, one)
                ok.append(bool(fr[0, 12]) == valid and abs(cos[0] - cr.COS_VALID) >= COS_MARGIN and bis.min() >= MIN_BISECTOR)
            if all(ok):
                return
    for t in range(T):
        draw(t)
    c.x_exists = np.ones(c.A, np.float32)
    if T >= 8:
        c.x_exists[[3 * 6 + 1, 2]] = 0                              # the centre of token 6 and a non-centre atom
    c.logits = {m: logits(rng, (T, T, nb)) for m in MODES}
    for _ in range(300):
        c.frames_pred, c.frames_gt = f32(cr.frames(c.x_pred0, c.ids)[0]), f32(cr.frames(c.x_gt, c.ids)[0])
        e = pair_errors(c)
        near = np.minimum(cr.edge_margin(e["pde"], lo, hi, nb), cr.edge_margin(e["pae"], lo, hi, nb))
        bad = sorted(set(np.nonzero(near < MARGIN)[1].tolist()))
        if not bad:
            c.closest = {m: float(cr.edge_margin(e[m], lo, hi, nb).min()) for m in MODES}
            c.errors = e
            c.bins = {m: cr.pair_bins(e[m], lo, hi, nb) for m in MODES}
            c.mask = np.outer(c.x_exists[c.centre], c.x_exists[c.centre])
            return c
        for t in bad:
            draw(t)
    raise RuntimeError(f"pairs {name}: could not clear the bin edges")


@functools.lru_cache(None)
def pairs_ref(name, mode):
    c = pairs(name)
    args = (c.logits[mode].reshape(-1, c.nb), c.bins[mode].reshape(-1), c.mask.reshape(-1))
    return cr.ce(*args), cr.ce(*args, dtype=np.float32)


# ------------------------------------------------------------------ pd_metrics_plddt
@functools.lru_cache(None)
def plddt(P, A, nb):
    rng = np.random.RandomState(5000 + 100 * A + nb)
    c = SimpleNamespace(name=name_of((P, A, nb)), P=P, A=A, nb=nb, logits=logits(rng, (P, A, nb)))
    c.logits[:, ::7] *= 6                                           # peaked rows among the flat ones
    return c


@functools.lru_cache(None)
def plddt_ref(P, A, nb):
    c = plddt(P, A, nb)
    return cr.plddt(c.logits), cr.plddt(c.logits, np.float32)


# ------------------------------------------------------------------ pd_metrics_pae_tm
def tm_split(P, T):
    """(nsplit, chunk, most iterations of a wave): the rule above tm_split in metrics.hip - about 2048 blocks where P T rows alone
    give fewer, chunks of a multiple of 64 pairs, a wave taking 16 pairs of every 64"""
    ceil = lambda a, b: -(-a // b)
    rows = P * T
    want = min(1 if rows >= 2048 else ceil(2048, rows), ceil(T, 64))
    chunk = ceil(ceil(T, want), 64) * 64
    return ceil(T, chunk), chunk, ceil(min(chunk, T), 64)


def pae_logits(T, nb, seed, best):
    rng = np.random.default_rng(seed)
    l = rng.random((T, T, nb), dtype=np.float32) * np.float32(8) - np.float32(4)
    k = np.arange(nb, dtype=np.float32)[None, :] * np.float32(64.0 / nb)
    l[best] = np.float32(0.25) * l[best] - np.float32(0.5) * k                          # mass on the low-error bins: the best row
    second = (best + T // 2) % T
    l[second] = np.float32(0.25) * l[second] - np.float32(0.3) * k
    return l


@functools.lru_cache(None)
def pae_tm(name):
    P, T, nb = PAE_TM[name]
    rng = np.random.RandomState(6000 + 10 * T + nb)
    c = SimpleNamespace(name=name, P=P, T=T, nb=nb, geometry=tm_split(P, T), best=BEST_ROWS[name])
    if name == "8x257x64":
        one = pae_tm("1x257x64")
        c.weights, c.asym, c.centres = one.weights, one.asym, one.centres
        c.logits = np.stack([one.logits[0] if p == SLICE else pae_logits(T, nb, 6100 + p, c.best[p]) for p in range(P)])
        return c
    w = (rng.uniform(size=T) >= 0.08).astype(np.float32)
    if name == "2x40x48":
        w = np.where(rng.uniform(size=T) < 0.3, rng.uniform(0.2, 0.9, T), w).astype(np.float32)
    best = BEST_ROWS["8x257x64"] if T == 257 else c.best          # the stack of eight shares these weights
    live = sorted(set(best) | {T - 1})
    w[live] = 1.0
    w[np.setdiff1d(np.arange(T), live)[:2]] = 0.0
    c.weights = w
    c.asym = np.ascontiguousarray(np.asarray([1, 2, 5])[(3 * np.arange(T)) // T], dtype=np.int32)
    c.centres = f32(cr.centres(nb))
    c.logits = np.stack([pae_logits(T, nb, 6200 + 97 * T + p, c.best[p]) for p in range(P)])
    return c


@functools.lru_cache(None)
def pae_tm_ref(name):
    """(float64, fp32) evaluations; the stack of eight is evaluated once per process"""
    c = pae_tm(name)
    return cr.pae_tm(c.logits, c.centres, c.weights, c.asym), cr.pae_tm(c.logits, c.centres, c.weights, c.asym, np.float32)


def tie_logits(base, rows):
    """[T,T,nb] with `rows` bit-identical and the best by far"""
    l = base.copy()
    nb = l.shape[-1]
    l[rows[0]] = np.float32(0.1) * l[rows[0]] - np.float32(0.9) * np.arange(nb, dtype=np.float32)[None, :]
    for r in rows[1:]:
        l[r] = l[rows[0]]
    return l


@functools.lru_cache(None)
def tie(first, second, T=257):
    """rows `first` < `second` tied for the best: both on one chain, both of weight 1.  T = 257: (0, 256) are the two rows of
    lane 0 of tm_final_kernel, (200, 256) a one-row lane against the second row of lane 0.  T = 260: (3, 259) are the two rows
    of lane 3."""
    one = pae_tm("1x257x64")
    c = SimpleNamespace(name=f"tie {first}={second} T {T}", P=1, T=T, nb=64, centres=one.centres, rows=(first, second))
    c.weights = np.ones(T, np.float32)
    c.weights[[10, 77]] = 0
    c.asym = np.ascontiguousarray(np.where(np.arange(T) < 150, 1, 2), dtype=np.int32)
    c.asym[[first, second]] = 7                                     # the tied rows: a chain of their own
    base = one.logits[0] if T == 257 else pae_logits(T, 64, 6300 + T, 0)
    c.logits = tie_logits(base, (first, second))[None]
    return c


# ------------------------------------------------------------------ pd_metrics_clash
@functools.lru_cache(None)
def clash(name):
    B, A, nc = CLASH[name]
    rng = np.random.RandomState(7000 + A)
    c = SimpleNamespace(name=name, B=B, A=A, nc=nc)
    c.chain = np.ascontiguousarray(rng.randint(0, nc, A), dtype=np.int32)
    c.a_mask, c.polymer = np.ones(A, np.float32), np.ones(A, np.float32)
    if A > 1:
        c.chain[[3, 200]], c.chain[[8, 256]] = -1, nc
        c.a_mask[rng.permutation(A)[:A // 12]] = 0
        c.a_mask[11] = 0.5
        c.polymer[rng.permutation(A)[:A // 10]] = 0
    side = (A * 5.6) ** (1.0 / 3.0)                                 # about one neighbour within 1.1 A at scale 1
    scale = np.asarray([1.0, 0.55, 3.0][:B])[:, None]
    base = rng.uniform(0, side, (A, 3))
    for _ in range(200):
        c.x_pred = f32(base[None] * scale[:, :, None])
        el = np.nonzero((c.a_mask == 1) & (c.polymer != 0) & (c.chain >= 0) & (c.chain < nc))[0]
        xe = c.x_pred[:, el].astype(np.float64)
        near = np.abs(cr.norm(xe[:, :, None] - xe[:, None]) - cr.CLASH_DIST) + np.eye(len(el))[None]
        bad = sorted(set(el[np.nonzero(near < MARGIN)[1]].tolist()))
        if not bad:
            c.ptm, c.iptm = f32(rng.uniform(0.2, 0.9, B)), f32(rng.uniform(0.2, 0.9, B))
            return c
        base[bad] = rng.uniform(0, side, (len(bad), 3))
    raise RuntimeError(f"clash {name}: could not clear 1.1 A")


@functools.lru_cache(None)
def clash_ref(name):
    """(counts [B,nc,nc], has_clash [B] of the reference's loop, has_clash [B] of the a < c loop, closest approach to 1.1 A)"""
    c = clash(name)
    return cr.clash(c.x_pred, c.a_mask, c.chain, c.polymer, c.nc)
