"""Float64 restatement of pd_plif_fingerprint, pd_plif_compare and pd_plif_pairwise (csrc/plif.hip), and the seeded cases the GPU
tests run.  Nothing here imports the package: the kinds, the type and charge bits and the default thresholds are written out again.

The acceptance rule.  A compare `r < t` cannot be bit-matched between fp32 and float64, so `restate` returns two fingerprints: `lo`,
the bits set with every threshold lowered by MARGIN = 1e-4 A, and `hi`, the bits set with every threshold raised by MARGIN.  The
device must satisfy lo <= dev <= hi bit by bit for `bits` and `ligand_bits`; its `counts` must be the popcounts of its own `bits`.
The seeded cases are chosen so that lo == hi in every byte (a condition on the inputs, asserted on the CPU by
tests/test_plif_cpu.py): no bit is left open and the device must equal the restatement exactly.  MARGIN is far above the fp32 error
of r derived below (3.5 u r is 2e-6 A at r = 10 A).

The bound of `min_dist`, derived, not fitted.  With u = 2^-24 and r = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))) on fp32
coordinates: dx = x_i - x_j carries a relative error u; dx * dx carries 2 u from dx and u of its own rounding, 3 u.  fmaf(dy, dy, .)
adds the exact product dy^2 (2 u from dy) to a term within 3 u - all terms are positive, so the sum is within 3 u - and rounds once:
4 u.  The second fmaf likewise: r^2 is within 5 u.  The square root halves that, 2.5 u, and the correctly rounded sqrtf adds u:
|r_fp32 - r| <= 3.5 u r, plus the products of these roundings (below 16 u^2 r) and, should dx * dx fall below the smallest normal
number, a flush of at most 2^-63 in r.  A minimum is exact and monotone, so the minimum of the fp32 distances lies within the same
bound of the minimum of the exact ones: the device's minimum is at most the fp32 distance of the pair that is exactly closest, and it
is the fp32 distance of a pair that is exactly no closer than that.  `bound` = R_UNITS u min_dist + 16 u^2 min_dist + 2^-63 is
applied element by element with no factor; +inf must match exactly."""
import numpy as np

U = 2.0 ** -24
R_UNITS = 3.5
FLUSH_R = 2.0 ** -63
MARGIN = 1e-4

KIND_NAMES = ("contact", "hydrophobic", "hbond_donor", "hbond_acceptor", "cationic", "anionic")
THRESHOLDS = (4.0, 4.5, 3.5, 4.5)                       # contact, hydrophobic, hbond, ionic
KIND_THRESHOLD = (0, 1, 2, 2, 3, 3)                     # which threshold a kind compares with
HYDROPHOBIC, DONOR, ACCEPTOR = 16, 32, 64               # bits of a type byte
CATION, ANION = 1, 2                                    # bits of a charge byte
PAIR_TILE = 16                                          # poses per side of a block of plif_pairwise_kernel


def allowed(lig_type, lig_charge, rec_type, rec_charge):
    """bool [6, L, A]: do the types of the pair (ligand atom, pose atom) allow kind k?"""
    lt, lq = np.asarray(lig_type, dtype=np.int64)[:, None], np.asarray(lig_charge, dtype=np.int64)[:, None]
    rt, rq = np.asarray(rec_type, dtype=np.int64)[None, :], np.asarray(rec_charge, dtype=np.int64)[None, :]
    one = np.ones(np.broadcast(lt, rt).shape, dtype=bool)
    return np.stack([one, ((lt & HYDROPHOBIC) > 0) & ((rt & HYDROPHOBIC) > 0), ((lt & DONOR) > 0) & ((rt & ACCEPTOR) > 0),
                     ((lt & ACCEPTOR) > 0) & ((rt & DONOR) > 0), ((lq & CATION) > 0) & ((rq & ANION) > 0),
                     ((lq & ANION) > 0) & ((rq & CATION) > 0)])


def popcounts(bits):
    """int [P, 6]: the number of residues whose byte has bit k"""
    b = np.asarray(bits, dtype=np.int64)
    return np.stack([((b >> k) & 1).sum(-1) for k in range(6)], -1)


def fingerprint(c, x=None, shift=0.0):
    """the definition in float64 with every threshold moved by `shift`: dict(bits uint8 [P,R], ligand_bits uint8 [P,L], min_dist
    float64 [P,R], counts int [P,6])"""
    x = np.asarray(c["x"] if x is None else x, dtype=np.float64)
    lig = np.asarray(c["lig_idx"], dtype=np.int64)
    types, charges = np.asarray(c["types"], dtype=np.int64), np.asarray(c["charges"], dtype=np.int64)
    rec, act = np.asarray(c["rec_mask"]) > 0, np.asarray(c["lig_active"]) > 0
    res, R = np.asarray(c["residue_of"], dtype=np.int64), int(c["n_residues"])
    n = x.shape[0]
    diff = x[:, lig][:, :, None, :] - x[:, None, :, :]
    r = np.sqrt((diff ** 2).sum(-1))                                                   # [P,L,A]
    pair = act[:, None] & rec[None, :]                                                 # [L,A]
    allow = allowed(types[lig], charges[lig], types, charges) & pair[None]
    byte = np.zeros(r.shape, dtype=np.int64)
    for k in range(6):
        byte |= ((r < c["thresholds"][KIND_THRESHOLD[k]] + shift) & allow[k][None]).astype(np.int64) << k
    ligand_bits = np.bitwise_or.reduce(byte, axis=2)
    rr = np.where(pair[None], r, np.inf)
    bits, min_dist = np.zeros((n, R), dtype=np.int64), np.full((n, R), np.inf)
    for s in range(R):
        sel = rec & (res == s)
        if sel.any():
            bits[:, s] = np.bitwise_or.reduce(byte[:, :, sel].reshape(n, -1), axis=1)
            min_dist[:, s] = rr[:, :, sel].reshape(n, -1).min(1)
    return dict(bits=bits.astype(np.uint8), ligand_bits=ligand_bits.astype(np.uint8), min_dist=min_dist, counts=popcounts(bits))


def restate(c, x=None):
    """dict(lo, hi: `fingerprint` with the thresholds lowered / raised by MARGIN; min_dist; bound: its fp32 error bound; open_bytes:
    the number of bytes of bits and ligand_bits in which lo != hi; n_bytes)"""
    lo, hi = fingerprint(c, x, -MARGIN), fingerprint(c, x, +MARGIN)
    m = lo["min_dist"]
    finite = np.isfinite(m)
    bound = np.where(finite, (R_UNITS * U + 16.0 * U * U) * np.where(finite, m, 0.0) + FLUSH_R, 0.0)
    open_bytes = int((lo["bits"] != hi["bits"]).sum() + (lo["ligand_bits"] != hi["ligand_bits"]).sum())
    return dict(lo=lo, hi=hi, min_dist=m, bound=bound, open_bytes=open_bytes, n_bytes=int(lo["bits"].size + lo["ligand_bits"].size))


def ratio(num, den):
    """one fp32 division of two integers; 1 where the denominator is 0"""
    num, den = np.asarray(num, dtype=np.int64), np.asarray(den, dtype=np.int64)
    return np.where(den == 0, np.float32(1.0), num.astype(np.float32) / np.where(den == 0, 1, den).astype(np.float32)).astype(np.float32)


def popcount8(a):
    a = np.asarray(a, dtype=np.int64)
    return sum((a >> k) & 1 for k in range(8))


def compare(bits, ref, mask=63):
    """integer numpy of pd_plif_compare: dict(shared [P], n_pose [P], n_reference, recovery fp32 [P], tanimoto fp32 [P])"""
    b, r = np.asarray(bits, dtype=np.int64) & mask, np.asarray(ref, dtype=np.int64) & mask
    shared, n_pose, n_ref = popcount8(b & r[None]).sum(-1), popcount8(b).sum(-1), int(popcount8(r).sum())
    return dict(shared=shared, n_pose=n_pose, n_reference=n_ref, recovery=ratio(shared, n_ref), tanimoto=ratio(shared, n_pose + n_ref - shared))


def pairwise(bits, mask=63):
    """integer numpy of pd_plif_pairwise: fp32 [P,P]"""
    b = np.asarray(bits, dtype=np.int64) & mask
    shared = popcount8(b[:, None, :] & b[None, :, :]).sum(-1)
    n = popcount8(b).sum(-1)
    return ratio(shared, n[:, None] + n[None, :] - shared)


# ------------------------------------------------------------------ the seeded cases of tests/test_plif_gpu.py
FLAGS = [0, HYDROPHOBIC, DONOR, ACCEPTOR, DONOR | ACCEPTOR, HYDROPHOBIC | DONOR, HYDROPHOBIC | ACCEPTOR, HYDROPHOBIC | DONOR | ACCEPTOR]

#: name -> (poses, pose atoms, ligand atoms as pose indices, inactive ligand atom or None, residues, residue layout, seed)
CASES = {
    "a_P3_A300_L5_R40": (3, 300, (7, 130, 131, 256, 299), 2, 40, "runs", 3),
    "b_P2_A65_L1_R3": (2, 65, (64,), None, 3, "modulo", 2),
    "c_P2_A257_L3_R257": (2, 257, (0, 200, 256), None, 257, "single", 5),
    "d_P66_A65_L2_R9": (66, 65, (20, 64), None, 9, "modulo", 2),
}
#: (type flags, charge) of the ligand atoms by ligand size: between them they can show every kind
LIGAND_ATOMS = {
    5: [(HYDROPHOBIC, 0), (DONOR | ACCEPTOR, CATION), (ACCEPTOR, 0), (ACCEPTOR, ANION), (HYDROPHOBIC | DONOR, 0)],
    3: [(HYDROPHOBIC | DONOR, CATION), (ACCEPTOR, ANION), (HYDROPHOBIC, 0)],
    2: [(HYDROPHOBIC | DONOR, CATION), (ACCEPTOR, ANION)],
    1: [(HYDROPHOBIC | DONOR | ACCEPTOR, CATION | ANION)],
}
#: case a: the residue block whose atoms are all masked out of the receptor
MASKED_BLOCK = 3


def make_case(name):
    """a jittered 3.8 A lattice of receptor atoms with the ligand inside it: dict(x fp32 [P,A,3], lig_idx, types, charges,
    lig_active, rec_mask, residue_of, n_residues, thresholds).  Every flag combination and every charge occur among the receptor's
    bytes and rec_mask has holes.  Residue layouts: "runs" - blocks of eight consecutive atoms (atoms 252 .. 259 form one: a run
    that crosses atom 256) under a permutation of the ids, twelve pairs of atoms then swap ids (interleaved ids), one id stays
    without any atom and the atoms of block MASKED_BLOCK are all masked; "modulo" - atom j belongs to residue j mod R; "single" -
    one atom per residue, the ids a permutation of the atoms."""
    n, A, lig, inactive, R, layout, seed = CASES[name]
    rng = np.random.default_rng(7300 + seed)
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
    types = (rng.integers(0, 10, A) | np.asarray(FLAGS)[rng.permutation(A) % len(FLAGS)]).astype(np.uint8)
    charges = np.asarray([0, 0, CATION, ANION])[rng.permutation(A) % 4].astype(np.uint8)
    for i, (flags, q) in enumerate(LIGAND_ATOMS[len(lig)]):
        types[lig[i]] = (types[lig[i]] & 15) | flags
        charges[lig[i]] = q
    rec_mask = np.ones(A, dtype=np.uint8)
    rec_mask[lig] = 0
    rec_mask[rec_atoms[rng.permutation(len(rec_atoms))[:max(len(rec_atoms) // 10, 2)]]] = 0   # holes
    if layout == "runs":
        block = (np.arange(A) + 4) // 8
        assert block.max() + 1 < R, "one id must stay without atoms"
        residue_of = rng.permutation(R)[block]
        for a, b in rng.permutation(A)[:24].reshape(12, 2):
            if block[a] != MASKED_BLOCK and block[b] != MASKED_BLOCK:
                residue_of[a], residue_of[b] = residue_of[b], residue_of[a]
        rec_mask[block == MASKED_BLOCK] = 0
    elif layout == "modulo":
        residue_of = np.arange(A) % R
    else:
        residue_of = rng.permutation(A)
    active = np.ones(len(lig), dtype=np.uint8)
    if inactive is not None:
        active[inactive] = 0
    return dict(x=x.astype(np.float32), lig_idx=lig.astype(np.int32), types=types, charges=charges, lig_active=active, rec_mask=rec_mask,
                residue_of=residue_of.astype(np.int32), n_residues=R, thresholds=THRESHOLDS)


def csr(c):
    """(res_start int32 [R + 1], res_atom int32 [N]) of a case: its receptor atoms sorted by residue, ascending inside one"""
    atoms = np.nonzero(c["rec_mask"])[0]
    res = np.asarray(c["residue_of"], dtype=np.int64)[atoms]
    start = np.concatenate([[0], np.cumsum(np.bincount(res, minlength=int(c["n_residues"])))])
    return start.astype(np.int32), atoms[np.argsort(res, kind="stable")].astype(np.int32)
