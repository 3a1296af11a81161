"""Float64 restatement of pd_buried_surface (csrc/sasa.hip) and the seeded cases the GPU tests run.  Nothing here imports the package:
the point formula, the radii and the defaults are written out again.

The definition.  Over the A atoms of a pose: cls (0 ignored, 1 receptor, 2 ligand), radius (fp32 values), probe, and n unit vectors,
the golden spiral computed in float64 and rounded to fp32: t = k + 0.5, z = 1 - 2 t / n, phi = t pi (3 - sqrt 5), u_k = (sqrt(1 - z^2)
cos phi, sqrt(1 - z^2) sin phi, z).  For atom i of class c != 0 with R_i = radius_i + probe: the point p_ik = x_i + R_i u_k is covered
by atom j iff j != i (by index), cls_j != 0 and |p_ik - x_j| < R_j; same_k: a covering j has class c; other_k: one has the other
class; n_free = #{k: !same_k}, n_bound = #{k: !same_k && !other_k}, n_buried = n_free - n_bound; an atom's area per point is
4 pi R_i^2 / n.

The acceptance rule (as in tests/plif_ref.py).  A compare `d < R` cannot be bit-matched between fp32 and float64, so `restate`
evaluates every point's same / other flag twice: with all covering radii R_j moved by -MARGIN and by +MARGIN, MARGIN = 1e-4 A.  A
case is CLOSED when no flag of any point of any atom differs between the two; every seeded case is closed (tests/test_sasa_cpu.py
asserts it on the CPU), and then the device's integer counts must equal the restatement exactly.

Why MARGIN covers the fp32 evaluation.  u = 2^-24; the cases keep |coordinate| <= X = 64 A, R <= 3.6 A (radius <= 2.1, probe 1.4
plus a little).  The device forms R_i = radius_i + probe (error <= u R_i <= 2.2e-7, and the fp32 probe differs from 1.4 by at most
1.4 u = 8.4e-8), then per coordinate fmaf(R_i, u_k, x_i): one rounding of a number below X + 3.6, <= 68 u = 4.1e-6; the unit table
entry is within u = 6e-8 of the float64 spiral, times R_i: 2.2e-7 (the restatement uses the rounded table, so this term is spare).  Per
coordinate the point is within 4.1e-6 + 2.2e-7 + 8.4e-8 + 2.2e-7 < 4.7e-6 of the exact one, as a vector within sqrt(3) 4.7e-6 =
8.1e-6 A.  The squared distance fmaf(dz, dz, fmaf(dy, dy, dx * dx)) of the fp32 point: each difference carries u, the chain as derived
in tests/plif_ref.py leaves d^2 within 5 u relative, d within 2.5 u d; a pair matters only where d is near R_j <= 3.6: 5.4e-7.  The
other side of the compare is R_j * R_j with R_j = fl(radius_j + probe): u from the sum and from the probe, u / 2 from the product, in
terms of R_j: 2.5 u R_j = 5.4e-7.  Sum: 8.1e-6 + 5.4e-7 + 5.4e-7 < 9.3e-6 A, a factor ten below MARGIN.  (`distance_error_bound`
returns the figure for a case's own coordinate range; the CPU test asserts it is below MARGIN for every case.)

Areas and sums are compared with the float64 value computed from the DEVICE'S OWN counts.  area(m, i) on the device is
(float)m * ((12.566370614359172f * (R_i * R_i)) / (float)n): roundings - the sum R_i (u) and the fp32 probe (<= u of R_i), both doubled
by the square (4 u), the square (u), the constant (u) and the product with it (u), the division (u), the product with m (u; m and n
are exact): TERM_UNITS = 9 u relative, plus their products (below 64 u^2).  An ascending fp32 sum of m non-negative terms adds at most
(m - 1) u relative of the total (each partial sum is rounded once and never exceeds the total).  So a sum of m terms lies within
((9 + m - 1) u + 64 u^2) of its float64 value; the fraction adds both sums' bounds and u of the division; the interface area adds u
of its addition (the halving is exact).  Derived, not fitted."""
import numpy as np

U = 2.0 ** -24
MARGIN = 1e-4
TERM_UNITS = 9.0
SECOND_ORDER = 64.0 * U * U
PROBE = 1.4
DEFAULT_POINTS = 96
LIST = 256                                              # entries after which sasa_point_kernel walks its neighbour list
VDW_RADII = {1: 1.2, 6: 1.7, 7: 1.6, 8: 1.55, 9: 1.5, 15: 1.95, 16: 1.8, 17: 1.8, 35: 1.9, 53: 2.1}
DEFAULT_RADIUS = 2.0
TOTAL_NAMES = ("ligand_free", "ligand_bound", "ligand_buried", "buried_fraction", "buried_polar", "buried_apolar", "receptor_buried",
               "interface_area")


def sphere_points(n):
    """float64 [n,3]: the golden spiral, not rounded"""
    t = np.arange(int(n), dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * t / int(n)
    phi = t * (np.pi * (3.0 - np.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], -1)


def radii_of(elements, radii=None):
    table = dict(VDW_RADII)
    table.update(radii or {})
    return np.asarray([table.get(int(z), DEFAULT_RADIUS) for z in elements], dtype=np.float32)


def classes(c):
    """uint8 [A] of a case: 0 ignored, 1 receptor, 2 ligand - from receptor_mask, a_mask, ligand_active and the elements (hydrogens
    are ignored)"""
    A = len(c["elements"])
    heavy = np.asarray(c["elements"]) != 1
    am = np.asarray(c["a_mask"]) > 0
    cls = np.where((np.asarray(c["receptor_mask"]) > 0) & am & heavy, 1, 0).astype(np.uint8)
    lig = np.asarray(c["lig_idx"])
    cls[lig] = np.where((np.asarray(c["lig_active"]) > 0) & am[lig] & heavy[lig], 2, 0)
    assert cls.shape == (A,)
    return cls


def flags(x, cls, radius, probe, n, shift=0.0):
    """(same, other) bool [A,n] of ONE pose x [A,3] in float64, every covering radius moved by `shift`; rows of ignored atoms are
    False"""
    x = np.asarray(x, dtype=np.float64)
    cls = np.asarray(cls)
    R = np.asarray(radius, dtype=np.float64) + float(probe)
    unit = sphere_points(n).astype(np.float32).astype(np.float64)
    A = x.shape[0]
    same, other = np.zeros((A, n), dtype=bool), np.zeros((A, n), dtype=bool)
    live = np.nonzero(cls != 0)[0]
    for i in live:
        pts = x[i] + R[i] * unit                                                        # [n,3]
        js = live[live != i]
        near = js[((x[js] - x[i]) ** 2).sum(-1) < (R[i] + R[js] + 1.0) ** 2]            # the others cannot cover a point
        if len(near) == 0:
            continue
        d = np.sqrt(((pts[:, None, :] - x[near][None, :, :]) ** 2).sum(-1))             # [n,J]
        cover = d < (R[near] + shift)[None, :]
        mine = cls[near] == cls[i]
        same[i] = cover[:, mine].any(1)
        other[i] = cover[:, ~mine].any(1)
    return same, other


def counts_of(same, other):
    """(n_free, n_bound, n_buried) int [A] from the flags of one pose; ignored atoms count 0 (their rows are masked by the caller)"""
    n_free = (~same).sum(1)
    n_bound = (~same & ~other).sum(1)
    return n_free, n_bound, n_free - n_bound


def restate(c, x=None):
    """dict(n_free, n_bound, n_buried: int [P,A] (0 for ignored atoms), open_flags: the number of flags that differ between the
    covering radii moved by -MARGIN and by +MARGIN, n_flags)"""
    x = np.asarray(c["x"] if x is None else x, dtype=np.float64)
    cls, n = classes(c), int(c["n_points"])
    out = {k: np.zeros(x.shape[:2], dtype=np.int64) for k in ("n_free", "n_bound", "n_buried")}
    open_flags = 0
    live = cls != 0
    for p in range(x.shape[0]):
        lo, hi = flags(x[p], cls, c["radius"], c["probe"], n, -MARGIN), flags(x[p], cls, c["radius"], c["probe"], n, +MARGIN)
        open_flags += int((lo[0] != hi[0]).sum() + (lo[1] != hi[1]).sum())
        f, b, d = counts_of(*lo)
        out["n_free"][p], out["n_bound"][p], out["n_buried"][p] = f * live, b * live, d * live
    out.update(open_flags=open_flags, n_flags=int(2 * x.shape[0] * live.sum() * n))
    return out


def distance_error_bound(c, x=None):
    """the fp32 error of the compare |p_ik - x_j| < R_j in A (module docstring) for the case's own coordinate and radius range"""
    x = np.abs(np.asarray(c["x"] if x is None else x, dtype=np.float64)).max()
    R = float(np.max(c["radius"])) + float(c["probe"])
    per_coordinate = (x + R) * U + R * U + 1.4 * U + R * U
    return np.sqrt(3.0) * per_coordinate + 2.5 * U * R + 2.5 * U * R


def csr(c):
    """(res_start int32 [R + 1], res_atom int32 [N]): the receptor atoms (class 1) sorted by residue, ascending inside one"""
    atoms = np.nonzero(classes(c) == 1)[0]
    res = np.asarray(c["residue_of"], dtype=np.int64)[atoms]
    start = np.concatenate([[0], np.cumsum(np.bincount(res, minlength=int(c["n_residues"])))])
    return start.astype(np.int32), atoms[np.argsort(res, kind="stable")].astype(np.int32)


def areas(c, free_points, buried_points):
    """the float outputs in float64 from integer counts (free_points [P,L], buried_points [P,A]) with their derived fp32 bounds:
    dict name -> (value, bound) for per_atom [P,L], the eight totals [P], residue_buried [P,R]; and interface_residues int [P]"""
    cls = classes(c)
    n, lig = int(c["n_points"]), np.asarray(c["lig_idx"])
    R = np.asarray(c["radius"], dtype=np.float64) + float(c["probe"])
    app = 4.0 * np.pi * R * R / n                                                       # area per point [A]
    fr, bu = np.asarray(free_points, dtype=np.float64), np.asarray(buried_points, dtype=np.float64)
    pol = np.asarray(c["polar"]) > 0
    L, rec = len(lig), cls == 1
    term = TERM_UNITS * U + SECOND_ORDER
    rel = lambda m: term + max(m - 1, 0) * U
    out = {}
    per_atom = bu[:, lig] * app[lig]
    out["per_atom"] = (per_atom, term * per_atom)
    free = (fr * app[lig]).sum(1)
    buried = per_atom.sum(1)
    bound = ((fr - bu[:, lig]) * app[lig]).sum(1)
    polar, apolar = per_atom[:, pol].sum(1), per_atom[:, ~pol].sum(1)
    receptor = (bu[:, rec] * app[rec]).sum(1)
    out["ligand_free"], out["ligand_bound"], out["ligand_buried"] = (free, rel(L) * free), (bound, rel(L) * bound), (buried, rel(L) * buried)
    out["buried_polar"], out["buried_apolar"] = (polar, rel(L) * polar), (apolar, rel(L) * apolar)
    out["receptor_buried"] = (receptor, rel(int(rec.sum())) * receptor)
    frac = np.where(free > 0, buried / np.where(free > 0, free, 1.0), 0.0)
    out["buried_fraction"] = (frac, (2 * rel(L) + U + SECOND_ORDER) * frac)
    iface = (buried + receptor) / 2
    out["interface_area"] = (iface, (rel(L) * buried + rel(int(rec.sum())) * receptor) / 2 + U * iface)
    start, atom = csr(c)
    res = np.zeros((fr.shape[0], int(c["n_residues"])))
    res_bound = np.zeros_like(res)
    for s in range(res.shape[1]):
        run = atom[start[s]:start[s + 1]]
        res[:, s] = (bu[:, run] * app[run]).sum(1)
        res_bound[:, s] = rel(len(run)) * res[:, s]
    out["residue_buried"] = (res, res_bound)
    out["interface_residues"] = (res > 0).sum(1)
    return out


# ------------------------------------------------------------------ the seeded cases of tests/test_sasa_gpu.py
CENTRE = np.array([20.0, 21.0, 19.0])
BALL = 6.6                                              # radius (A) of the ball the 70 atoms of a case are packed into
SPACING = 1.3                                           # smallest distance between two atoms of a pose
ELEMENTS = (6, 6, 6, 7, 8, 16)

#: name -> (poses, pose atoms, ligand atoms as pose indices, points, site, special, seed); every seed was found by a short search for
#: a closed case (tests/test_sasa_cpu.py asserts it).  site "core": the ligand's atoms are those closest to the centre of the ball
#: (buried); "rim": those closest to a point of its surface (half exposed).  special: see make_case.
CASES = {
    "a_P3_A70_L9_n96": (3, 70, (0, 5, 17, 18, 33, 40, 41, 63, 69), 96, "core", None, 9),
    "b_P3_A70_L9_n257": (3, 70, (0, 5, 17, 18, 33, 40, 41, 63, 69), 257, "core", None, 6),
    "c_P3_A70_L9_n1": (3, 70, (0, 5, 17, 18, 33, 40, 41, 63, 69), 1, "core", None, 0),
    "d_P3_A70_L1_n96": (3, 70, (69,), 96, "core", None, 1),
    "e_P3_A70_L9_n96_rim": (3, 70, (0, 5, 17, 18, 33, 40, 41, 63, 69), 96, "rim", None, 3),
    "f_P3_A70_L9_n96_special": (3, 70, (0, 5, 17, 18, 33, 40, 41, 63, 69), 96, "core", "special", 9),
    "g_P1_A530_L1_n96_cluster": (1, 530, (529,), 96, "core", "cluster", 8),
}
#: case f: the atom a_mask removes, the inactive ligand atom (position in lig_idx), the receptor atom no ligand atom reaches, and the
#: pair at identical coordinates (the second takes the first's place; a carbon and an oxygen: the radii differ by 0.15 A)
F_HOLE, F_INACTIVE, F_FAR, F_TWIN = 7, 3, 50, (20, 21)
#: case g: LIST + 5 receptor atoms within reach of the ligand atom - LIST of them in the first run of 256 atoms, so the list is walked
#: after it, and five at 520 .. 524, behind a run that adds nothing, for the second walk; every other atom is far away
G_CLUSTER = tuple(range(LIST)) + tuple(range(520, 525))


def packed(rng, n, centre, radius):
    """n points in a ball, no two closer than SPACING"""
    pts = []
    while len(pts) < n:
        q = rng.uniform(-radius, radius, 3)
        if (q ** 2).sum() <= radius ** 2 and all(((q - w) ** 2).sum() >= SPACING ** 2 for w in pts):
            pts.append(q)
    return np.asarray(pts) + centre


def make_case(name):
    """dict(x fp32 [P,A,3], elements, radius fp32 [A], lig_idx, lig_active, receptor_mask, a_mask, polar, residue_of, n_residues,
    probe, n_points).  Every pose is its own packing of the ball; the atoms closest to the site become the ligand.  "special" (case
    f): atom F_HOLE has a_mask 0, ligand atom F_INACTIVE is inactive, receptor atom F_FAR sits 30 A away, atom F_TWIN[1] lies on atom
    F_TWIN[0].  "cluster" (case g): G_CLUSTER around the ligand atom, the rest on a distant lattice."""
    n_pose, A, lig, n_points, site, special, seed = CASES[name]
    rng = np.random.default_rng(9100 + seed)
    lig = np.asarray(lig)
    rec_atoms = np.setdiff1d(np.arange(A), lig)
    elements = np.asarray(ELEMENTS)[rng.integers(0, len(ELEMENTS), A)]
    x = np.empty((n_pose, A, 3))
    if special == "cluster":
        cluster = np.asarray(G_CLUSTER)
        rest = np.setdiff1d(rec_atoms, cluster)
        for p in range(n_pose):
            x[p, lig] = CENTRE
            v = rng.normal(size=(len(cluster), 3))
            x[p, cluster] = CENTRE + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(3.0, 5.8, (len(cluster), 1))
            grid = np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(-1, 3)[:len(rest)]
            x[p, rest] = CENTRE + np.array([14.0, -12.0, -12.0]) + 3.9 * grid + rng.uniform(-0.3, 0.3, (len(rest), 3))
    else:
        target = CENTRE + (np.array([BALL, 0.0, 0.0]) if site == "rim" else 0.0)
        for p in range(n_pose):
            pts = packed(rng, A, CENTRE, BALL)
            order = np.argsort(((pts - target) ** 2).sum(-1), kind="stable")
            x[p, lig] = pts[order[:len(lig)]]
            x[p, rec_atoms] = pts[order[len(lig):]][rng.permutation(len(rec_atoms))]
    a_mask, lig_active = np.ones(A, dtype=np.uint8), np.ones(len(lig), dtype=np.uint8)
    if special == "special":
        a_mask[F_HOLE] = 0
        lig_active[F_INACTIVE] = 0
        x[:, F_FAR] += np.array([0.0, 30.0, 0.0])
        elements[F_TWIN[0]], elements[F_TWIN[1]] = 6, 8
        x[:, F_TWIN[1]] = x[:, F_TWIN[0]]
    receptor_mask = np.ones(A, dtype=np.uint8)
    receptor_mask[lig] = 0
    n_residues = max(A // 8, 1)
    residue_of = (np.arange(A) // 4) % n_residues                     # residues of eight atoms in two runs of four
    return dict(x=x.astype(np.float32), elements=elements, radius=radii_of(elements), lig_idx=lig.astype(np.int32), lig_active=lig_active,
                receptor_mask=receptor_mask, a_mask=a_mask, polar=((elements[lig] == 7) | (elements[lig] == 8)).astype(np.uint8),
                residue_of=residue_of.astype(np.int32), n_residues=n_residues, probe=PROBE, n_points=n_points)
