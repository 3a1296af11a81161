"""Float64 restatement of pd_plif_rings (csrc/plif_rings.hip) and the seeded cases the GPU tests run.  Nothing here imports the
package: the kinds, the type and charge bits and the default thresholds are written out again.  This file is the written definition;
the header comment of csrc/plif_rings.hip and the docstring of physdock_amd/ring_interactions.py repeat it.

Ring.  A ring is a list of k pose-atom indices in cyclic order, 3 <= k <= 8.  For a pose, with a_i the ring's atoms:
    centroid  c = (a_0 + ... + a_{k-1}) / k                 (summed in list order, one division per coordinate)
    normal    N = sum_i (a_i - c) x (a_{i+1} - c), indices mod k;  n = N / |N|
A ring with |N| zero or not finite, or with a coordinate that is not finite, is degenerate: it takes part in nothing and reports
n = 0.  The sign of n is never looked at, only |n . m| and squares, so nothing changes when the list is rotated or reversed.

Five kinds; bit k of a byte is kind k of RING_KIND_NAMES.  Thresholds in the order of THRESHOLD_NAMES (five distances in A, three
angles in degrees; the host turns the angles into cosines in double, the kernel compares cosines):
    0 pi_parallel   ligand ring g, receptor ring h: d = |c_g - c_h| < stack_dist (5.5); min(off_gh, off_hg) < stack_offset (2.0);
                    |n_g . n_h| > cos(parallel_angle) (30)
    1 pi_tshaped    the same distance and offset; |n_g . n_h| < cos(t_angle) (60)
    2 pi_cation     ligand ring g, receptor CATION atom j: |x_j - c_g| < pication_dist (6.0); the offset of x_j on the plane of g
                    < pication_offset (2.0)
    3 cation_pi     ligand CATION atom i (active), receptor ring h: the same with the roles swapped
    4 halogen_bond  ligand halogen X (active) with its heavy neighbour C, receptor ACCEPTOR atom j: |x_X - x_j| < halogen_dist
                    (4.0); cos(C - X ... j) < cos(halogen_angle) (135)
off_gh = sqrt(max(0, d^2 - ((c_h - c_g) . n_g)^2)) is the distance from c_g to the projection of c_h onto the plane of g; the offset
of a point is the same with the point in place of c_h.  Bits 5 - 7 are always 0.  Receptor atoms are those of rec_mask; CATION is bit
0 of the charge byte, ACCEPTOR bit 6 of the type byte.

Outputs for P poses, R residues, L ligand atoms, G_l ligand rings, G_r receptor rings (G = G_l + G_r, the ligand's rings first, the
receptor's in ascending order of their residue): bits [P,R] the OR over the residue's rings, cations and acceptors; ligand_bits [P,L]
the OR per ligand atom (a ring's bits go to all of its atoms, a halogen bond to X, cation_pi to the cation; an inactive atom has 0);
ring_bits [P,G_l] the OR per ligand ring; centroid, normal [P,G,3]; min_centroid_dist [P,R] the smallest distance between a ligand
ring's and one of the residue's rings' centroids (degenerate rings left out; +inf when there is none), counts [P,5] residues per kind.

The acceptance rule.  `restate` returns two fingerprints: `lo` with every distance threshold lowered by MARGIN = 1e-4 A and every
cosine window shrunk by CMARGIN = 1e-4 (cos(parallel_angle) raised, cos(t_angle) and cos(halogen_angle) lowered), `hi` with all of
them moved the other way.  Every test is monotone in its thresholds, so lo <= hi bit by bit, and the device must satisfy lo <= dev <=
hi for bits, ligand_bits and ring_bits; its counts must be the popcounts of its own bits.  In the seeded cases lo == hi in every byte
(a condition on the inputs, asserted on the CPU), so the device must equal the restatement.

The float64 error, from the operation count (u = 2^-53; M the largest |coordinate| of a ring's atoms, rho its largest |a_i - c|, k its
size; all bounds per component and to first order in u).  The coordinates are fp32 numbers and are converted exactly.
  * centroid: k - 1 additions of partial sums below k M, each within u k M, then one division: |dc| <= k u M =: E_C.
  * r_i = a_i - c: the rounding u |r_i| <= 2 u M plus dc: |dr| <= (k + 2) u M =: E_R.
  * one component of a cross product, r_y s_z - r_z s_y: each product is perturbed by at most 2 rho E_R and rounded within u rho^2,
    the difference is rounded within 2 u rho^2: 4 rho E_R + 4 u rho^2.  The sum of k of them, each partial sum below k rho^2:
    |dN| <= k (4 rho E_R + 4 u rho^2) + k^2 u rho^2 =: E_N.  (A fused multiply-add rounds once where this counts twice.)
  * n = N / |N|: the length moves by at most sqrt(3) E_N, so |dn| <= 2 sqrt(3) E_N / |N| + 3 u =: E_n.
  * a centroid distance d: |dd| <= 2 sqrt(3) E_C + 3 u d =: E_d.
At M = 100 A, k = 6, rho = 1.4 A, |N| = 10 A^2 (a benzene): E_C = 7e-14, E_R = 9e-14, E_N = 3e-12, E_n = 1e-12, E_d = 3e-13 A - nine
orders below MARGIN.  A cosine |n_g . n_h| is within 6 E_n + 5 u = 6e-12 - seven orders below CMARGIN; the cosine of the halogen
angle, from three fp32 points, is within 20 u.  A plane distance p = v . n is within |v| sqrt(3) E_n + sqrt(3) (E_C + E_d) = 1.3e-11
at |v| = 6 A; q = d^2 - p^2 is within 2 d E_d + 2 |p| 1.3e-11 = 1.6e-10, and the offset sqrt(q) within 1.6e-10 / (2 offset) = 4e-11 A
at the default threshold of 2 A - six orders below MARGIN - and, since |sqrt(a) - sqrt(b)| <= sqrt|a - b|, never beyond 1.3e-5 A,
still below MARGIN, whatever the threshold is.  Nothing here is fitted.

Bounds of the float outputs, applied element by element with no factor.  Both sides are float64 evaluations, each within the bound
of the exact value, so the device's centroid lies within 2 E_C of the restatement's and its normal within 2 E_n (`frame_bounds`;
rho and |N| are taken from the restatement).  min_centroid_dist is the float64 minimum rounded once to fp32: within 2^-24 m + 2 E_d
of the restatement's m; +inf matches exactly.  NaN centroids (a ring with a NaN coordinate) must be NaN on both sides."""
import numpy as np

U64 = 2.0 ** -53
U32 = 2.0 ** -24
MARGIN = 1e-4
CMARGIN = 1e-4

RING_KIND_NAMES = ("pi_parallel", "pi_tshaped", "pi_cation", "cation_pi", "halogen_bond")
THRESHOLD_NAMES = ("stack_dist", "stack_offset", "pication_dist", "pication_offset", "halogen_dist", "parallel_angle", "t_angle",
                   "halogen_angle")
THRESHOLDS = (5.5, 2.0, 6.0, 2.0, 4.0, 30.0, 60.0, 135.0)
HYDROPHOBIC, DONOR, ACCEPTOR = 16, 32, 64               # bits of a type byte
CATION, ANION = 1, 2                                    # bits of a charge byte
#: the launch geometry of csrc/plif_rings.hip that case d crosses: rings per block of plif_rings_frame_kernel, receptor entities
#: (rings, then list entries) per block of plif_rings_receptor_kernel, the stride of plif_rings_ligand_kernel over the receptor's
#: rings and list entries (one wave per ligand entity), the stride of plif_rings_fold_kernel over residues and ligand atoms
FRAME_BLOCK, RECEPTOR_BLOCK, LIGAND_BLOCK, FOLD_BLOCK = 64, 256, 64, 64


def popcounts(bits):
    """int [P, 5]: the number of residues whose byte has bit k"""
    b = np.asarray(bits, dtype=np.int64)
    return np.stack([((b >> k) & 1).sum(-1) for k in range(5)], -1)


def frames(x, rings):
    """x float64 [P,A,3], rings: lists of atom indices -> (centroid [P,G,3], normal [P,G,3] (0 for a degenerate ring), ok bool
    [P,G], |N| [P,G], rho [P,G])"""
    n, G = x.shape[0], len(rings)
    c, nrm, ok = np.zeros((n, G, 3)), np.zeros((n, G, 3)), np.zeros((n, G), dtype=bool)
    length, rho = np.zeros((n, G)), np.zeros((n, G))
    with np.errstate(all="ignore"):
        for g, ring in enumerate(rings):
            a = x[:, list(ring)]                                                        # [P,k,3]
            k = a.shape[1]
            s = a[:, 0].copy()
            for i in range(1, k):
                s = s + a[:, i]
            c[:, g] = s / k
            r = a - c[:, g][:, None]
            N = np.zeros((n, 3))
            for i in range(k):
                N = N + np.cross(r[:, i], r[:, (i + 1) % k])
            ln = np.sqrt((N ** 2).sum(-1))
            good = np.isfinite(a).all((1, 2)) & np.isfinite(ln) & (ln > 0)
            ok[:, g] = good
            nrm[:, g] = np.where(good[:, None], N / np.where(good, ln, 1.0)[:, None], 0.0)
            length[:, g] = np.where(good, ln, 0.0)
            rho[:, g] = np.where(good, np.sqrt((r ** 2).sum(-1)).max(1), 0.0)
    return c, nrm, ok, length, rho


def plane_offset(v, n):
    """(|v|, the distance of v's end from the axis through the origin along the unit vector n): [...], [...]"""
    d2 = (v ** 2).sum(-1)
    p = (v * n).sum(-1)
    return np.sqrt(d2), np.sqrt(np.maximum(0.0, d2 - p * p))


def fingerprint(c, x=None, sign=0):
    """the definition in float64 with every threshold moved by `sign` margins (-1: lo, +1: hi): dict(bits uint8 [P,R], ligand_bits
    uint8 [P,L], ring_bits uint8 [P,G_l], centroid, normal float64 [P,G,3], ok bool [P,G], min_centroid_dist float64 [P,R], counts
    int [P,5], length, rho [P,G])"""
    x = np.asarray(c["x"] if x is None else x, dtype=np.float64)
    lig = np.asarray(c["lig_idx"], dtype=np.int64)
    types, charges = np.asarray(c["types"], dtype=np.int64), np.asarray(c["charges"], dtype=np.int64)
    rec, act = np.asarray(c["rec_mask"]) > 0, np.asarray(c["lig_active"]) > 0
    res, R = np.asarray(c["residue_of"], dtype=np.int64), int(c["n_residues"])
    lig_rings, rec_rings, ring_res = list(c["lig_rings"]), list(c["rec_rings"]), list(c["rec_ring_residue"])
    assert ring_res == sorted(ring_res), "the receptor's rings come in ascending order of their residue"
    t = [float(v) for v in c["thresholds"]]
    stack_dist, stack_off, pc_dist, pc_off, hal_dist = (v + sign * MARGIN for v in t[:5])
    cos_par = np.cos(np.deg2rad(t[5])) - sign * CMARGIN
    cos_t = np.cos(np.deg2rad(t[6])) + sign * CMARGIN
    cos_hal = np.cos(np.deg2rad(t[7])) + sign * CMARGIN
    n, L, Gl, Gr = x.shape[0], len(lig), len(lig_rings), len(rec_rings)
    local = {int(a): i for i, a in enumerate(lig)}
    cen, nrm, ok, length, rho = frames(x, lig_rings + rec_rings)
    bits, ligand_bits, ring_bits = np.zeros((n, R), np.int64), np.zeros((n, L), np.int64), np.zeros((n, Gl), np.int64)
    mcd = np.full((n, R), np.inf)
    rec_cations = [j for j in np.nonzero(rec)[0] if charges[j] & CATION]
    rec_acceptors = [j for j in np.nonzero(rec)[0] if types[j] & ACCEPTOR]
    lig_cations = [i for i in range(L) if act[i] and charges[lig[i]] & CATION]
    with np.errstate(all="ignore"):
        for g in range(Gl):
            for hh in range(Gr):
                h, s = Gl + hh, ring_res[hh]
                both = ok[:, g] & ok[:, h]
                v = cen[:, h] - cen[:, g]
                d, off_g = plane_offset(v, nrm[:, g])
                _, off_h = plane_offset(v, nrm[:, h])
                cosang = np.abs((nrm[:, g] * nrm[:, h]).sum(-1))
                near = both & (d < stack_dist) & (np.minimum(off_g, off_h) < stack_off)
                b = (near & (cosang > cos_par)).astype(np.int64) | (near & (cosang < cos_t)).astype(np.int64) << 1
                bits[:, s] |= b
                ring_bits[:, g] |= b
                mcd[:, s] = np.where(both, np.minimum(mcd[:, s], d), mcd[:, s])
            for j in rec_cations:
                d, off = plane_offset(x[:, j] - cen[:, g], nrm[:, g])
                b = (ok[:, g] & (d < pc_dist) & (off < pc_off)).astype(np.int64) << 2
                bits[:, res[j]] |= b
                ring_bits[:, g] |= b
        for i in lig_cations:
            for hh in range(Gr):
                h = Gl + hh
                d, off = plane_offset(x[:, lig[i]] - cen[:, h], nrm[:, h])
                b = (ok[:, h] & (d < pc_dist) & (off < pc_off)).astype(np.int64) << 3
                bits[:, ring_res[hh]] |= b
                ligand_bits[:, i] |= b
        for xl, cl in c["halogens"]:
            if not act[xl]:
                continue
            px, pc = x[:, lig[xl]], x[:, lig[cl]]
            u = pc - px
            for j in rec_acceptors:
                w = x[:, j] - px
                d2 = (w ** 2).sum(-1)
                cosang = (u * w).sum(-1) / np.sqrt((u ** 2).sum(-1) * d2)
                b = ((np.sqrt(d2) < hal_dist) & (cosang < cos_hal)).astype(np.int64) << 4
                bits[:, res[j]] |= b
                ligand_bits[:, xl] |= b
    for g, ring in enumerate(lig_rings):
        for a in ring:
            ligand_bits[:, local[int(a)]] |= ring_bits[:, g]
    ligand_bits[:, ~act] = 0
    return dict(bits=bits.astype(np.uint8), ligand_bits=ligand_bits.astype(np.uint8), ring_bits=ring_bits.astype(np.uint8), centroid=cen,
                normal=nrm, ok=ok, min_centroid_dist=mcd, counts=popcounts(bits), length=length, rho=rho)


def frame_bounds(c, f, x=None):
    """(2 E_C [P,G,1], 2 E_n [P,G,1]) of the module docstring for the frames `f` = fingerprint(c, x); 0 where a ring is degenerate"""
    x = np.asarray(c["x"] if x is None else x, dtype=np.float64)
    rings = list(c["lig_rings"]) + list(c["rec_rings"])
    n, G = f["ok"].shape
    e_c, e_n = np.zeros((n, G, 1)), np.zeros((n, G, 1))
    with np.errstate(all="ignore"):
        for g, ring in enumerate(rings):
            k = len(ring)
            M = np.abs(x[:, list(ring)]).max((1, 2))
            rho, ln, ok = f["rho"][:, g], f["length"][:, g], f["ok"][:, g]
            E_C = k * U64 * M
            E_R = (k + 2) * U64 * M
            E_N = k * (4 * rho * E_R + 4 * U64 * rho ** 2) + k * k * U64 * rho ** 2
            E_n = 2 * np.sqrt(3.0) * E_N / np.where(ok, ln, 1.0) + 3 * U64
            e_c[:, g, 0] = np.where(ok, 2 * E_C, 0.0)
            e_n[:, g, 0] = np.where(ok, 2 * E_n, 0.0)
    return e_c, e_n


def restate(c, x=None):
    """dict(lo, hi: `fingerprint` with the thresholds moved against / with the margins; mid: with the thresholds as given (its
    frames and min_centroid_dist are the reference values); centroid_bound, normal_bound, min_bound; open_bytes: the number of bytes
    of bits, ligand_bits and ring_bits in which lo != hi; n_bytes)"""
    lo, mid, hi = fingerprint(c, x, -1), fingerprint(c, x, 0), fingerprint(c, x, +1)
    e_c, e_n = frame_bounds(c, mid, x)
    xs = np.asarray(c["x"] if x is None else x, dtype=np.float64)
    M = np.nanmax(np.abs(np.where(np.isfinite(xs), xs, 0.0)), axis=(1, 2))[:, None] if xs.shape[1] else np.zeros((xs.shape[0], 1))
    m = mid["min_centroid_dist"]
    fin = np.isfinite(m)
    mz = np.where(fin, m, 0.0)
    min_bound = np.where(fin, U32 * mz + 2 * (2 * np.sqrt(3.0) * 8 * U64 * M + 3 * U64 * mz), 0.0)
    keys = ("bits", "ligand_bits", "ring_bits")
    return dict(lo=lo, mid=mid, hi=hi, centroid_bound=e_c, normal_bound=e_n, min_bound=min_bound,
                open_bytes=int(sum((lo[k] != hi[k]).sum() for k in keys)), n_bytes=int(sum(lo[k].size for k in keys)))


# ------------------------------------------------------------------ tables as the C entry takes them
def csr(c):
    """(res_start int32 [R + 1], res_atom int32 [N]) of a case: its receptor atoms sorted by residue, ascending inside one"""
    atoms = np.nonzero(c["rec_mask"])[0]
    res = np.asarray(c["residue_of"], dtype=np.int64)[atoms]
    start = np.concatenate([[0], np.cumsum(np.bincount(res, minlength=int(c["n_residues"])))])
    return start.astype(np.int32), atoms[np.argsort(res, kind="stable")].astype(np.int32)


def ring_tables(c):
    """(ring_start int32 [G + 1], ring_atom int32, ring_residue int32 [G], halogen int32 [H,2]): the ligand's rings first (residue
    -1), then the receptor's in the case's order, which ascends in the residue"""
    rings = [list(r) for r in c["lig_rings"]] + [list(r) for r in c["rec_rings"]]
    start = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
    atom = np.asarray([a for r in rings for a in r], dtype=np.int32)
    residue = np.asarray([-1] * len(c["lig_rings"]) + list(c["rec_ring_residue"]), dtype=np.int32)
    return start, atom, residue, np.asarray(c["halogens"], dtype=np.int32).reshape(-1, 2)


# ------------------------------------------------------------------ construction of the seeded cases
JITTER = 0.05
RADIUS = {5: 1.20, 6: 1.39}


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v ** 2).sum())


def polygon(k, centre, normal, phase=0.0):
    """the k corners of a regular ring around `centre` in the plane across `normal`, in cyclic order"""
    nz = unit(normal)
    e1 = unit(np.cross(nz, [0.0, 0.0, 1.0] if abs(nz[2]) < 0.9 else [1.0, 0.0, 0.0]))
    e2 = np.cross(nz, e1)
    ang = phase + 2 * np.pi * np.arange(k) / k
    return np.asarray(centre, dtype=np.float64) + RADIUS[k] * (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2)


def rotation(axis, degrees):
    a, t = unit(axis), np.deg2rad(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


#: the ligand of cases a, e and f in its own frame (z = 0 plane): local index -> what it is
LIG6, LIG5, LIG_CATION, LIG_CL, LIG_BR, LIG_BR_C, LIG_H = list(range(0, 6)), list(range(6, 11)), 11, 12, 13, 14, 15
LIG_CL_C = 2


def ligand_frame():
    """float64 [16,3]: a benzene around the origin (atoms 0 - 5), a five-ring around (7, 0, 0) (6 - 10), a cation (11), a chlorine
    (12) on ring atom 2, a bromine (13) on the aliphatic carbon 14, an inactive hydrogen (15); (type, charge) per atom"""
    xl = np.zeros((16, 3))
    xl[LIG6] = polygon(6, [0, 0, 0], [0, 0, 1])
    xl[LIG5] = polygon(5, [7, 0, 0], [0, 0, 1])
    xl[LIG_CATION] = [3.5, 3.0, 0.0]
    xl[LIG_CL] = xl[LIG_CL_C] * (1.39 + 1.74) / 1.39
    xl[LIG_BR_C] = [3.5, -2.5, 0.0]
    xl[LIG_BR] = [3.5, -4.4, 0.0]
    xl[LIG_H] = [3.5, -2.0, 0.9]
    kinds = [(HYDROPHOBIC, 0)] * 11 + [(DONOR, CATION), (HYDROPHOBIC, 0), (HYDROPHOBIC, 0), (HYDROPHOBIC, 0), (0, 0)]
    return xl, kinds


def designed_receptor():
    """the receptor of case a in the ligand's frame: a list of (residue, kind, coordinates [m,3], (type, charge) per atom, ring or
    None).  Residues: 0 PHE stacked 3.8 A above the benzene (pi_parallel); 1 TYR across the benzene's axis 5.0 A below it
    (pi_tshaped); 2 HIS parallel to the five-ring, 3.6 A above and 3.0 A to the side (rejected by the offset alone); 3 TRP, its
    five-ring 4.0 A below the ligand's five-ring and tilted by 45 degrees (neither parallel nor T), its six-ring beside it; 4 LYS NZ
    4.0 A above the five-ring (pi_cation); 5 ARG: a cation in the benzene's plane 4.6 A out (offset too large); 6 an acceptor on the
    C - Cl axis at 3.3 A and 170 degrees (halogen_bond); 7 an acceptor 3.3 A from the bromine at 100 degrees; 8 PHE 4.0 A above the
    ligand's cation (cation_pi); 9, 10: carbons only; 11: backbone far away; 12, 13: no atoms (13 is the ligand's own)."""
    xl, _ = ligand_frame()
    hyd, out = (HYDROPHOBIC, 0), []
    out.append((0, polygon(6, [0, 0, 3.8], [0, 0, 1], 0.3), [hyd] * 6, True))
    out.append((1, polygon(6, [0, 0, -5.0], [1, 0, 0], 0.1), [hyd] * 6, True))
    out.append((2, polygon(5, [10.0, 0, 3.6], [0, 0, 1], 0.2), [hyd] * 5, True))
    tilt = [np.sin(np.pi / 4), 0, np.cos(np.pi / 4)]
    out.append((3, polygon(5, [7.0, 0, -4.0], tilt, 0.0), [hyd] * 5, True))
    out.append((3, polygon(6, [7.0 + 2.2 * np.cos(np.pi / 4), 0, -4.0 - 2.2 * np.sin(np.pi / 4)], tilt, 0.4), [hyd] * 6, True))
    out.append((4, np.array([[7.0, 0, 4.0], [7.0, 1.2, 4.9]]), [(DONOR, CATION), hyd], None))
    out.append((5, np.array([[-4.5, -1.0, 0.0], [-5.6, -1.6, 0.6]]), [(DONOR, CATION), hyd], None))
    cl, c2 = xl[LIG_CL], xl[LIG_CL_C]
    out.append((6, np.array([cl + 3.3 * (rotation([0, 0, 1], 10.0) @ unit(cl - c2)), cl + 4.4 * unit(cl - c2) + [0, 0, 0.8]]),
                [(ACCEPTOR, 0), hyd], None))
    br, cb = xl[LIG_BR], xl[LIG_BR_C]
    out.append((7, np.array([br + 3.3 * (rotation([0, 0, 1], 100.0) @ unit(cb - br)), br + [4.2, -1.5, 0.5]]), [(ACCEPTOR, 0), hyd], None))
    out.append((8, polygon(6, [3.5, 3.0, 4.0], [0, 0, 1], 0.5), [hyd] * 6, True))
    out.append((9, np.array([[-3.0, 5.0, 6.0], [-4.0, 6.0, 6.5], [-5.0, 5.5, 7.5]]), [hyd] * 3, None))
    out.append((10, np.array([[12.0, -6.0, -6.0], [13.0, -7.0, -6.5]]), [hyd] * 2, None))
    out.append((11, np.array([[0.0, 12.0, 0.0], [1.2, 12.5, 0.3], [2.0, 13.5, 0.0], [2.5, 13.0, 1.2]]),
                [(DONOR, 0), hyd, hyd, (ACCEPTOR, 0)], None))
    return out


def assemble(n_poses, ligand_kinds, lig_rings_local, halogens, receptor, n_residues, lig_pose, rng, fillers=0, inactive=(LIG_H,),
             exact=()):
    """put a case together.  lig_pose(p) -> float64 [L,3] the ligand of pose p in the receptor's frame; the receptor's atoms come
    first (A = receptor + fillers + L), `fillers` further atoms - every type and charge among them - lie on a jittered shell 9 - 14 A
    from (3.5, 0, 0) in the residues 10 and 11; every atom of every pose is then moved by a seeded JITTER (uniform per coordinate),
    except the y and z of the ligand atoms listed in `exact`."""
    rec_x, types, charges, residue_of, rec_rings, ring_res = [], [], [], [], [], []
    for s, xyz, kinds, ring in sorted(receptor, key=lambda e: e[0]):
        if ring:
            rec_rings.append(list(range(len(rec_x), len(rec_x) + len(xyz))))
            ring_res.append(s)
        for p, (t, q) in zip(xyz, kinds):
            rec_x.append(p); types.append(t | 1); charges.append(q); residue_of.append(s)
    flags = [0, HYDROPHOBIC, DONOR, ACCEPTOR, DONOR | ACCEPTOR, HYDROPHOBIC | ACCEPTOR]
    for f in range(fillers):
        v = rng.normal(size=3)
        rec_x.append(unit(v) * rng.uniform(9.0, 14.0) + [3.5, 0, 0])
        types.append(flags[f % len(flags)] | 2); charges.append([0, 0, CATION, ANION][f % 4]); residue_of.append(10 + f % 2)
    n_rec, L = len(rec_x), len(ligand_kinds)
    A = n_rec + L
    lig_idx = np.arange(n_rec, A)
    x = np.zeros((n_poses, A, 3))
    for p in range(n_poses):
        if n_rec:
            x[p, :n_rec] = np.asarray(rec_x)
        x[p, n_rec:] = lig_pose(p)
    jit = rng.uniform(-JITTER, JITTER, x.shape)
    for i in exact:
        jit[:, n_rec + i, 1:] = 0.0
    x = x + jit
    types = np.asarray(types + [t | 1 for t, _ in ligand_kinds], dtype=np.uint8)
    charges = np.asarray(charges + [q for _, q in ligand_kinds], dtype=np.uint8)
    residue_of = np.asarray(residue_of + [n_residues - 1] * L, dtype=np.int32)
    rec_mask = np.zeros(A, dtype=np.uint8)
    rec_mask[:n_rec] = 1
    active = np.ones(L, dtype=np.uint8)
    active[list(inactive)] = 0
    return dict(x=x.astype(np.float32), lig_idx=lig_idx.astype(np.int32), types=types, charges=charges, lig_active=active,
                rec_mask=rec_mask, residue_of=residue_of, n_residues=n_residues, thresholds=THRESHOLDS,
                lig_rings=[[n_rec + i for i in ring] for ring in lig_rings_local], rec_rings=rec_rings, rec_ring_residue=ring_res,
                halogens=[tuple(h) for h in halogens])


def rigid(xl, R=None, t=(0.0, 0.0, 0.0)):
    return xl @ (np.eye(3) if R is None else R).T + np.asarray(t, dtype=np.float64)


def case_a_poses(xl):
    """pose 0: the designed geometry; pose 1: the ligand slid 3 A along y (the stack is lost to the offset); pose 2: the ligand
    turned by 90 degrees about x and lifted"""
    return [xl, rigid(xl, None, (0.0, 3.0, 0.0)), rigid(xl, rotation([1, 0, 0], 90.0), (0.5, 0.0, -0.8))]


def random_rings(n_rings, first_residue, rng, radius=11.0):
    """n_rings receptor six- and five-rings with seeded centres (3 .. radius A from (3.5, 0, 0)) and normals, one residue each"""
    out = []
    for h in range(n_rings):
        centre = unit(rng.normal(size=3)) * rng.uniform(3.0, radius) + [3.5, 0, 0]
        k = 6 if h % 3 else 5
        out.append((first_residue + h, polygon(k, centre, rng.normal(size=3), rng.uniform(0, 6.28)), [(HYDROPHOBIC, 0)] * k, True))
    return out


CASES = ("a_P3_L16_R14", "b_no_ligand_ring", "b_no_receptor_ring", "c_no_receptor_atom", "d_P2_A700", "e_P66", "f_degenerate_and_nan")
#: case f: the ligand ring (local atoms) that is three collinear atoms, the pose and the ligand atom with the NaN
F_NAN_POSE, F_NAN_ATOM = 1, 4


def make_case(name):
    """one of CASES: dict(x fp32 [P,A,3], lig_idx, types, charges, lig_active, rec_mask, residue_of, n_residues, thresholds (five
    distances, three angles in degrees), lig_rings, rec_rings (lists of pose-atom indices), rec_ring_residue, halogens (pairs of
    ligand-local indices X, C))"""
    rng = np.random.default_rng(9100 + CASES.index(name))
    xl, kinds = ligand_frame()
    rings, halogens = [LIG6, LIG5], [(LIG_CL, LIG_CL_C), (LIG_BR, LIG_BR_C)]
    if name == "a_P3_L16_R14":
        poses = case_a_poses(xl)
        return assemble(3, kinds, rings, halogens, designed_receptor(), 14, lambda p: poses[p], rng, fillers=160 - 16 - 52)
    if name == "b_no_ligand_ring":
        # an aliphatic ligand: a chain with a cation above the PHE of residue 8 and a chlorine on the C - Cl axis of case a
        chain = np.array([xl[LIG_CATION], [2.6, 1.8, 0.2], xl[LIG_CL_C] + [0.9, 0.5, 0.0], xl[LIG_CL_C], xl[LIG_CL]])
        ck = [(DONOR, CATION), (HYDROPHOBIC, 0), (HYDROPHOBIC, 0), (HYDROPHOBIC, 0), (HYDROPHOBIC, 0)]
        poses = [chain, rigid(chain, None, (0.0, 0.0, 9.0))]
        return assemble(2, ck, [], [(4, 3)], designed_receptor(), 14, lambda p: poses[p], rng, fillers=20, inactive=())
    if name == "b_no_receptor_ring":
        receptor = [(s, xyz, k, None) for s, xyz, k, ring in designed_receptor()]
        poses = case_a_poses(xl)
        return assemble(2, kinds, rings, halogens, receptor, 14, lambda p: poses[p], rng, fillers=20)
    if name == "c_no_receptor_atom":
        poses = case_a_poses(xl)
        return assemble(2, kinds, rings, halogens, [], 3, lambda p: poses[p], rng)
    if name == "d_P2_A700":
        # 6 + 62 receptor rings, 3 + 270 acceptors, 2 + 30 cations: tests/test_plif_rings_cpu.py asserts the counts against the blocks
        receptor = designed_receptor() + random_rings(62, 14, rng)
        acc = []
        for k in range(270):
            acc.append((76 + k % 20, (unit(rng.normal(size=3)) * rng.uniform(4.0, 10.0) + [3.5, 0, 0])[None], [(ACCEPTOR, CATION if k % 9 == 0 else 0)],
                        None))
        # the ligand grows by 56 carbons on a lattice 9 A and more from the rings: L = 72 crosses FOLD_BLOCK
        tail = np.array([[-4.0 + 1.5 * (i % 8), -9.0 - 1.5 * (i // 8), 3.0] for i in range(56)])
        xd, kd = np.concatenate([xl, tail]), kinds + [(HYDROPHOBIC, 0)] * 56
        poses = [xd, rigid(xd, rotation([1, 2, 0.5], 40.0), (0.5, -0.5, 0.7))]
        return assemble(2, kd, rings, halogens, receptor + acc, 97, lambda p: poses[p], rng, fillers=0)
    if name == "e_P66":
        # 66 poses: seeded rigid motions of the ligand of up to 25 degrees and 1.5 A about the designed geometry; pose 0 is it
        moves = [(np.eye(3), np.zeros(3))] + [(rotation(rng.normal(size=3), rng.uniform(-25, 25)), rng.uniform(-1.5, 1.5, 3)) for _ in range(65)]
        return assemble(66, kinds, rings, halogens, designed_receptor(), 14, lambda p: rigid(xl, *moves[p]), rng)
    if name == "f_degenerate_and_nan":
        # three more ligand atoms on a line along x, listed as a ring (their y and z are not jittered: they stay exactly collinear);
        # poses 0 and 1 are the designed geometry, pose 2 the slid one; pose F_NAN_POSE has a NaN in the benzene's atom F_NAN_ATOM
        xf = np.concatenate([xl, [[2.0, 6.5, 1.25], [3.5, 6.5, 1.25], [5.0, 6.5, 1.25]]])
        kf = kinds + [(HYDROPHOBIC, 0)] * 3
        poses = [xf, xf, case_a_poses(xf)[1]]
        c = assemble(3, kf, rings + [[16, 17, 18]], halogens, designed_receptor(), 14, lambda p: poses[p], rng, fillers=12, exact=(16, 17, 18))
        c["x"][F_NAN_POSE, c["lig_idx"][F_NAN_ATOM], 1] = np.nan
        return c
    raise KeyError(name)
