"""Float64 restatement of pd_vina_score (csrc/vina.hip) with the fp32 error bound of every output, and the seeded cases the GPU
tests run.  Nothing here imports the package: the radii, weights and type bits are written out again.

The bound is derived, not fitted.  With u = 2^-24 (half an fp32 ulp, relative):

* the distance.  dx = x_i - x_j carries u; dx*dx another u on top of 2u; the two fmaf roundings u each: r^2 is within 5u, r after the
  correctly rounded sqrtf within 3.5u r.  R_i + R_j: the two fp32 radii u each and the addition u.  d = r - (R_i + R_j): u |d|.
  Together |d_fp32 - d| <= EPS_D_UNITS u (r + R_i + R_j) with EPS_D_UNITS = 5.
* a term t(d) moves by |t'(d)| eps_d, plus its own arithmetic: gauss1 = expf(-(2d)^2): the square rounds (u q^2 in the argument,
  so u q^2 relative in the value) and expf is documented to 1 ulp = 2u; gauss2 = expf(-((d-3)/2)^2): the subtraction adds 2u q^2
  more; repulsion d*d: u; the hydrophobic slope 1.5 - d: u; the hbond slope -d / 0.7f: the constant and the division, 2u.  A result
  below the smallest normal number may be flushed: 2^-126 per pair.
* a sum of n terms in any order is within n u sum|t| of the exact sum of the rounded terms; n is the number of pairs of the atom
  plus the 9 steps of the block reduction, and the number of ligand atoms for the sums over atoms.
* the weighted sums: a weight u, a product u, four additions: 6u sum|w t|; the score's denominator 1 + 0.0585 n_rot 3u and the
  division u.
* the force of a pair is (sum_k w_k t_k'(d)) (x_i - x_j) / r: the bracket moves by sum |w_k| |t_k''| eps_d plus the arithmetic of
  the derivatives (the gaussians' own error and up to six roundings), the division by r and the product with dx 6u more.

`margin` is the smallest distance of any (active ligand atom, receptor atom) pair to the cutoff r = 8 or to a kink
d in {-0.7, 0, 0.5, 1.5}: the score jumps at the first and the gradient at the others, so a case must keep MARGIN = 1e-4 A clear
of them (a condition on the inputs, checked on the CPU; the committed seeds pass it)."""
import numpy as np

U = 2.0 ** -24
EPS_D_UNITS = 5.0
EXPF_ULPS = 1.0
FLUSH = 2.0 ** -126
MARGIN = 1e-4

TERM_NAMES = ("gauss1", "gauss2", "repulsion", "hydrophobic", "hbond")
WEIGHTS = np.array([-0.0356, -0.00516, 0.840, -0.0351, -0.587])
CLASS_RADII = np.array([1.9, 1.8, 1.7, 2.1, 2.0, 1.5, 1.8, 2.0, 2.2] + [1.2] * 7)          # C N O P S F Cl Br I, then anything else
HYDROPHOBIC, DONOR, ACCEPTOR = 16, 32, 64
CUTOFF, ROT_WEIGHT = 8.0, 0.0585
KINKS = (-0.7, 0.0, 0.5, 1.5)
C_H, N_DA, O_A, N_D = 0 | HYDROPHOBIC, 1 | DONOR | ACCEPTOR, 2 | ACCEPTOR, 1 | DONOR


def pair_terms(d, hydrophobic, hbond):
    """the five terms t [5, ...], their first and second derivatives in d, and the bound of each one's own fp32 arithmetic"""
    d = np.asarray(d, dtype=np.float64)
    q1, q2 = d / 0.5, (d - 3.0) / 2.0
    g1, g2 = np.exp(-q1 * q1), np.exp(-q2 * q2)
    neg = d < 0
    hs, hb_s = hydrophobic & (d > 0.5) & (d < 1.5), hbond & (d > -0.7) & (d < 0)
    t = np.stack([g1, g2, np.where(neg, d * d, 0.0), np.where(hydrophobic, np.where(d <= 0.5, 1.0, np.where(hs, 1.5 - d, 0.0)), 0.0),
                  np.where(hbond, np.where(d <= -0.7, 1.0, np.where(hb_s, -d / 0.7, 0.0)), 0.0)])
    t1 = np.stack([-8.0 * d * g1, -q2 * g2, np.where(neg, 2.0 * d, 0.0), np.where(hs, -1.0, 0.0), np.where(hb_s, -1.0 / 0.7, 0.0)])
    t2 = np.stack([(-8.0 + 64.0 * d * d) * g1, (-0.5 + q2 * q2) * g2, np.where(neg, 2.0, 0.0), np.zeros_like(d), np.zeros_like(d)])
    rel1, rel2 = q1 * q1 + 2.0 * EXPF_ULPS, 3.0 * q2 * q2 + 2.0 * EXPF_ULPS          # the gaussians' relative error, in units of u
    arith = U * np.stack([g1 * rel1, g2 * rel2, t[2], np.where(hs, np.abs(1.5 - d), 0.0), 2.0 * np.where(hb_s, t[4], 0.0)]) + FLUSH
    arith1 = U * np.abs(t1) * np.stack([rel1 + 6.0, rel2 + 6.0, np.full_like(d, 4.0), np.full_like(d, 4.0), np.full_like(d, 4.0)])
    return t, t1, t2, arith, arith1


def vina(x, lig_idx, types, rec_mask, lig_active, n_rot):
    """x [P,A,3] -> dict of float64 arrays: atom_terms [P,L,5], terms [P,5], inter [P], score [P], per_atom [P,L], forces [P,L,3];
    `bound`: the same keys, the fp32 error bound of each element; `margin`; `n_pairs` [P] counted pairs; `pair_force` [P,L,A,3]"""
    x = np.asarray(x, dtype=np.float64)
    lig_idx, types = np.asarray(lig_idx, dtype=np.int64), np.asarray(types, dtype=np.int64)
    rec, act = np.asarray(rec_mask) > 0, np.asarray(lig_active) > 0
    radius = CLASS_RADII[types & 15]
    tl, rl = types[lig_idx], radius[lig_idx]
    diff = x[:, lig_idx][:, :, None, :] - x[:, None, :, :]                               # [P,L,A,3]
    r = np.sqrt((diff ** 2).sum(-1))
    rsum = rl[:, None] + radius[None, :]
    d = r - rsum[None]
    pairs = np.broadcast_to(act[None, :, None] & rec[None, None, :], r.shape)
    count = pairs & (r < CUTOFF)
    margin = np.inf
    near = pairs & (r < CUTOFF + 1.0)
    if pairs.any():
        margin = float(np.abs(r[pairs] - CUTOFF).min())
    if near.any():
        margin = min([margin] + [float(np.abs(d[near] - k).min()) for k in KINKS])
    hyd = ((tl[:, None] & types[None, :] & HYDROPHOBIC) > 0)[None] & count
    hb = ((((tl[:, None] & DONOR) > 0) & ((types[None, :] & ACCEPTOR) > 0)) | (((tl[:, None] & ACCEPTOR) > 0) & ((types[None, :] & DONOR) > 0)))[None] & count
    t, t1, t2, arith, arith1 = pair_terms(d, hyd, hb)
    c = count[None]
    t, t1, t2, arith, arith1 = (np.where(c, v, 0.0) for v in (t, t1, t2, arith, arith1))
    eps_d = np.where(count, EPS_D_UNITS * U * (r + rsum[None]), 0.0)
    n_i = count.sum(-1)                                                                # [P,L]
    steps = (n_i + 9)[None]
    atom_terms = t.sum(-1)                                                             # [5,P,L]
    b_atom = (np.abs(t1) * eps_d[None] + arith).sum(-1) + steps * U * np.abs(t).sum(-1)
    L = len(lig_idx)
    terms = atom_terms.sum(-1)                                                         # [5,P]
    b_terms = b_atom.sum(-1) + L * U * np.abs(atom_terms).sum(-1)
    w = WEIGHTS[:, None, None]
    per_atom = (w * atom_terms).sum(0)
    b_per_atom = (np.abs(w) * b_atom).sum(0) + 6.0 * U * np.abs(w * atom_terms).sum(0)
    inter = (WEIGHTS[:, None] * terms).sum(0)
    b_inter = (np.abs(WEIGHTS[:, None]) * b_terms).sum(0) + 6.0 * U * np.abs(WEIGHTS[:, None] * terms).sum(0)
    den = 1.0 + ROT_WEIGHT * float(n_rot)
    score = inter / den
    b_score = b_inter / den + 4.0 * U * np.abs(score)
    # forces: -d inter / d x_i = -sum_j de (x_i - x_j) / r, a pair with r == 0 contributing nothing
    w4 = WEIGHTS[:, None, None, None]
    de = (w4 * t1).sum(0)                                                              # [P,L,A]
    b_de = (np.abs(w4) * (np.abs(t2) * eps_d[None] + arith1)).sum(0) + 5.0 * U * np.abs(w4 * t1).sum(0)
    ok = count & (r > 0)
    unit = np.where(ok[..., None], diff / np.where(r > 0, r, 1.0)[..., None], 0.0)
    pair_force = -de[..., None] * unit
    b_pair = (b_de + 6.0 * U * np.abs(de))[..., None] * np.abs(unit)
    forces = pair_force.sum(2)
    b_forces = b_pair.sum(2) + (n_i + 9)[..., None] * U * np.abs(pair_force).sum(2)
    tr = lambda v: np.moveaxis(v, 0, -1)
    return dict(atom_terms=tr(atom_terms), terms=tr(terms), inter=inter, score=score, per_atom=per_atom, forces=forces,
                bound=dict(atom_terms=tr(b_atom), terms=tr(b_terms), inter=b_inter, score=b_score, per_atom=b_per_atom, forces=b_forces),
                margin=margin, n_pairs=count.sum((1, 2)), pair_force=pair_force, pair_terms=t)


def energy(x, lig_idx, types, rec_mask, lig_active):
    """inter [P] alone (for finite differences)"""
    return vina(x, lig_idx, types, rec_mask, lig_active, 0.0)["inter"]


# ------------------------------------------------------------------ the seeded cases of tests/test_vina_gpu.py
ALL_TYPES = [c | f for c in range(10) for f in (0, HYDROPHOBIC, DONOR, ACCEPTOR, DONOR | ACCEPTOR, HYDROPHOBIC | DONOR, HYDROPHOBIC | ACCEPTOR,
                                                HYDROPHOBIC | DONOR | ACCEPTOR)]

#: name -> (poses, pose atoms, ligand atoms as pose indices, inactive ligand atom or None, seed)
CASES = {
    "P3_A300_L5": (3, 300, (7, 130, 131, 256, 299), 2, 1),
    "P2_A65_L1": (2, 65, (64,), None, 2),
    "P2_A257_L3": (2, 257, (0, 200, 256), None, 3),
}


def make_case(name):
    """a jittered 3.8 A lattice of receptor atoms with the ligand inside it: dict(x fp32 [P,A,3], lig_idx, types, rec_mask, lig_active,
    n_rot).  Every radius class (the nine elements and a metal) and every flag combination occurs among the type bytes; the ligand
    atoms are C_H, a donor/acceptor N, an acceptor O ... so that every term is non-zero; rec_mask has holes."""
    n, A, lig, inactive, seed = CASES[name]
    rng = np.random.default_rng(9100 + seed)
    lig = np.asarray(lig)
    side = int(np.ceil(A ** (1.0 / 3.0)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    centre = (side - 1) / 2.0
    order = np.argsort(((grid - centre) ** 2).sum(-1), kind="stable")                   # the sites closest to the centre first
    sites = (grid[order[:A]] - centre) * 3.8
    x = np.empty((n, A, 3))
    rec_atoms = np.setdiff1d(np.arange(A), lig)
    for p in range(n):
        x[p, rec_atoms] = sites[len(lig):][rng.permutation(len(rec_atoms))] + rng.uniform(-0.6, 0.6, (len(rec_atoms), 3))
        x[p, lig] = sites[:len(lig)] + rng.uniform(-0.9, 0.9, (len(lig), 3))
    types = np.asarray(ALL_TYPES)[rng.permutation(len(ALL_TYPES))[np.arange(A) % len(ALL_TYPES)]] if A >= len(ALL_TYPES) else \
        rng.choice(ALL_TYPES, A)
    types = np.asarray(types, dtype=np.uint8)
    types[lig] = np.resize(np.asarray([C_H, N_DA, O_A, C_H, N_D], dtype=np.uint8), len(lig))
    if len(lig) == 1:
        types[lig] = C_H | DONOR | ACCEPTOR                                             # one atom that sees every term
    rec_mask = np.ones(A, dtype=np.uint8)
    rec_mask[lig] = 0
    rec_mask[rec_atoms[rng.permutation(len(rec_atoms))[:max(len(rec_atoms) // 10, 2)]]] = 0   # holes
    active = np.ones(len(lig), dtype=np.uint8)
    if inactive is not None:
        active[inactive] = 0
    return dict(x=x.astype(np.float32), lig_idx=lig.astype(np.int32), types=types, rec_mask=rec_mask, lig_active=active, n_rot=3.0)
