"""Float64 restatement of pd_pocket_grid (csrc/pocket.hip) and the seeded cases the GPU tests run.  Nothing here imports the package:
the lattice, the predicates, the radii and the defaults are written out again.

The definition.  Over the A atoms of a pose: cls (0 ignored, 1 receptor, 2 ligand), radius (fp32 values); h, probe and lining are fp32
values, everything below is evaluated in float64 from them.
  centre    given, or the mean of the active ligand atoms' coordinates summed sequentially in lig_idx order and rounded once to fp32;
            with snap each coordinate c becomes fl32(h * rint(c / h))
  lattice   n points per axis; o = centre - h (n - 1) / 2; point (i, j, k) is g = o + (i, j, k) h with linear index (i n + j) n + k
  solid(g)  some receptor atom j has d(g, x_j) < radius_j + probe;   inside(g)  some active ligand atom i has d(g, x_i) < radius_i;
  near(g,j) d(g, x_j) < radius_j + lining for a receptor atom j;      d = sqrt of the sum of the three squared differences
  buried(g) the number of the seven DIRECTIONS in which a solid point lies within floor(reach / (h |d|)) lattice steps of g in the +
            sense and also in the - sense; leaving the lattice is not a hit
  pocket    not solid and buried >= min_enclosed; pocket points form 6-connected components, ranked by their smallest linear index; a
            pocket point with inside is occupied; the site is the union of the components that hold an occupied point
  classes   0 solid, 1 free but not pocket, 2 pocket outside the site, 3 site and empty, 4 site and occupied
  counts    n_solid, n_free (every non-solid point), n_pocket, n_site, n_occupied, n_ligand (non-solid points with inside),
            n_components, n_site_components;   truncated: a site point lies on a face of the lattice
  values    site_volume = n_site h^3, unfilled_volume = (n_site - n_occupied) h^3, pocket_volume = n_pocket h^3, filled_fraction =
            n_occupied / n_site, ligand_in_site = n_occupied / n_ligand (0 where the divisor is 0), ligand_enclosure = the mean of
            atom_buried / 7 over the ligand atoms that have a point (0 when none has)
  per ligand atom: atom_class / atom_buried of the lattice point rint((x - o) / h); 255 for an inactive atom or one outside the lattice
  per residue: lining_points = the site points g with near(g, j) for some receptor atom j of the residue; lining_residues = the number
            of residues with a count above 0
  ok        0 for a pose with a non-finite coordinate in an atom of class != 0 or a non-finite centre: counts 0, floats NaN, bytes 255

The acceptance rule (as in tests/sasa_ref.py).  The device evaluates the predicates in float64 - fp32 only filters the pairs far from a
threshold - so `restate` evaluates every predicate twice, with its threshold moved by -MARGIN and by +MARGIN, MARGIN = 1e-9 A: float64
evaluation of a distance below 10^3 A is good to 1e-12 A whatever the order of the operations.  A case is CLOSED when no flag (solid,
inside, and near per residue, of any point) differs between the two; every seeded case is closed (tests/test_pocket_cpu.py asserts
it), and then every integer of the device must EQUAL the restatement.  `band` counts the (point, atom) pairs within 1e-5 A of their
threshold: the population of the kernel's fp32 guard band.

Floats are compared with the float64 value computed from the DEVICE'S OWN counts: a volume is one product rounded once to fp32 (the
float64 product itself adds 2^-52), bound U = 2^-24 relative; a fraction is one quotient, bound 2 U (the issue allows two roundings).
Derived, not fitted."""
import numpy as np

U = 2.0 ** -24
MARGIN = 1e-9
BAND = 1e-5
F32 = lambda v: float(np.float32(v))
H, N, PROBE, LINING, REACH, MIN_ENCLOSED = 1.0, 32, F32(1.4), F32(2.4), 12.0, 5
VDW_RADII = {1: 1.2, 6: 1.7, 7: 1.6, 8: 1.55, 9: 1.5, 15: 1.95, 16: 1.8, 17: 1.8, 35: 1.9, 53: 2.1}
DEFAULT_RADIUS = 2.0
DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1))
COUNT_NAMES = ("n_solid", "n_free", "n_pocket", "n_site", "n_occupied", "n_ligand", "n_components", "n_site_components")
VALUE_NAMES = ("site_volume", "unfilled_volume", "pocket_volume", "filled_fraction", "ligand_in_site", "ligand_enclosure")


def radii_of(elements, radii=None):
    table = dict(VDW_RADII)
    table.update(radii or {})
    return np.asarray([table.get(int(z), DEFAULT_RADIUS) for z in elements], dtype=np.float32)


def classes(c):
    """uint8 [A] of a case: 0 ignored, 1 receptor, 2 ligand (hydrogens, a_mask == 0 and inactive ligand atoms are ignored)"""
    heavy = np.asarray(c["elements"]) != 1
    am = np.asarray(c["a_mask"]) > 0
    cls = np.where((np.asarray(c["receptor_mask"]) > 0) & am & heavy, 1, 0).astype(np.uint8)
    lig = np.asarray(c["lig_idx"])
    cls[lig] = np.where((np.asarray(c["lig_active"]) > 0) & am[lig] & heavy[lig], 2, 0)
    return cls


def csr(c):
    """(res_start int32 [R + 1], res_atom int32 [N]): the receptor atoms (class 1) sorted by residue, ascending inside one"""
    atoms = np.nonzero(classes(c) == 1)[0]
    res = np.asarray(c["residue_of"], dtype=np.int64)[atoms]
    start = np.concatenate([[0], np.cumsum(np.bincount(res, minlength=int(c["n_residues"])))])
    return start.astype(np.int32), atoms[np.argsort(res, kind="stable")].astype(np.int32)


def step_table(reach, h):
    """int [7]: floor(reach / (h |d|)) per direction"""
    return [int(np.floor(float(reach) / (float(h) * np.sqrt(float(sum(v * v for v in d)))))) for d in DIRECTIONS]


def centre_of(x, cls, lig_idx, h, centre=None, snap=True):
    """the used centre of ONE pose x [A,3] (fp32 values) as float64 [3] of fp32 values; NaN where it is not finite"""
    with np.errstate(all="ignore"):
        if centre is None:
            s, cnt = np.zeros(3), 0
            for a in np.asarray(lig_idx):
                if cls[a] == 2:
                    s, cnt = s + np.asarray(x[a], dtype=np.float64), cnt + 1
            c = (s / cnt if cnt else np.full(3, np.nan)).astype(np.float32).astype(np.float64)
        else:
            c = np.asarray(centre, dtype=np.float32).astype(np.float64)
        if snap:
            c = (float(h) * np.rint(c / float(h))).astype(np.float32).astype(np.float64)
    return c


def spheres(x, atoms, thr, o, h, n, shift):
    """bool [n,n,n]: the points within thr[a] + shift of some atom a of `atoms`; and the number of (point, atom) pairs within BAND
    of the threshold"""
    out, band = np.zeros((n, n, n), dtype=bool), 0
    for a, T in zip(atoms, thr):
        xa = np.asarray(x[a], dtype=np.float64)
        lo = np.clip(np.floor((xa - T - 1.0 - o) / h), 0, n).astype(int)
        hi = np.clip(np.ceil((xa + T + 1.0 - o) / h), -1, n - 1).astype(int)
        if (lo > hi).any():
            continue
        ax = [o[d] + np.arange(lo[d], hi[d] + 1) * h for d in range(3)]
        g = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
        d = np.sqrt(((g - xa) ** 2).sum(-1))
        out[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] |= d < T + shift
        band += int((np.abs(d - T) < BAND).sum())
    return out, band


def enclosure(solid, steps):
    """int [n,n,n]: the number of directions enclosed at every point"""
    n = solid.shape[0]
    pad = n
    big = np.zeros((3 * n,) * 3, dtype=bool)
    big[pad:pad + n, pad:pad + n, pad:pad + n] = solid

    def hit(d, S):
        out = np.zeros_like(solid)
        for s in range(1, min(S, n) + 1):
            out |= big[pad + s * d[0]:pad + s * d[0] + n, pad + s * d[1]:pad + s * d[1] + n, pad + s * d[2]:pad + s * d[2] + n]
        return out
    total = np.zeros(solid.shape, dtype=np.int64)
    for d, S in zip(DIRECTIONS, steps):
        total += hit(d, S) & hit(tuple(-v for v in d), S)
    return total


def components(pocket):
    """int [n,n,n]: the component id of every pocket point (6-connected, ranked by the smallest linear index), -1 elsewhere"""
    n = pocket.shape[0]
    lab = np.full(pocket.shape, -1, dtype=np.int64)
    nxt = 0
    for i, j, k in zip(*np.nonzero(pocket)):                         # ascending linear index
        if lab[i, j, k] >= 0:
            continue
        lab[i, j, k] = nxt
        stack = [(i, j, k)]
        while stack:
            a, b, c = stack.pop()
            for da, db, dc in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                q = (a + da, b + db, c + dc)
                if min(q) >= 0 and max(q) < n and pocket[q] and lab[q] < 0:
                    lab[q] = nxt
                    stack.append(q)
        nxt += 1
    return lab


def pose(c, x, centre, shift):
    """every output of ONE pose with all thresholds moved by `shift`: dict (maps flat [n^3]); near: bool [R, n^3]"""
    n, h, L, R = int(c["n"]), float(c["h"]), len(c["lig_idx"]), int(c["n_residues"])
    cls, lig = classes(c), np.asarray(c["lig_idx"])
    x32 = np.asarray(x, dtype=np.float32)
    live = cls != 0
    ctr = centre_of(x32, cls, lig, h, centre, c["snap"])
    out = dict(centre=ctr)
    if not (np.isfinite(x32[live]).all() and np.isfinite(ctr).all()):
        out.update(ok=0, centre=np.full(3, np.nan), classes=np.full(n ** 3, 255), buried=np.full(n ** 3, 255), counts=np.zeros(8, dtype=np.int64),
                   truncated=0, atom_class=np.full(L, 255), atom_buried=np.full(L, 255), lining_points=np.zeros(R, dtype=np.int64),
                   lining_residues=0, band=0, flags=np.zeros(0, dtype=bool))
        return out
    xd = x32.astype(np.float64)
    rad = np.asarray(c["radius"], dtype=np.float32).astype(np.float64)
    o = ctr - h * (n - 1) / 2
    rec, act = np.nonzero(cls == 1)[0], np.nonzero(cls == 2)[0]
    solid, b1 = spheres(xd, rec, rad[rec] + c["probe"], o, h, n, shift)
    inside, b2 = spheres(xd, act, rad[act], o, h, n, shift)
    buried = np.where(solid, 0, enclosure(solid, step_table(c["reach"], h)))
    pocket = ~solid & (buried >= int(c["min_enclosed"]))
    comp = components(pocket)
    occupied = pocket & inside
    site_ids = np.unique(comp[occupied])
    site = pocket & np.isin(comp, site_ids)
    cl = np.where(solid, 0, np.where(~pocket, 1, np.where(~site, 2, np.where(inside, 4, 3))))
    face = np.zeros_like(solid)
    face[0], face[-1], face[:, 0], face[:, -1], face[:, :, 0], face[:, :, -1] = True, True, True, True, True, True
    counts = np.array([solid.sum(), (~solid).sum(), pocket.sum(), site.sum(), (site & inside).sum(), (~solid & inside).sum(),
                       comp.max() + 1, len(site_ids)], dtype=np.int64)
    atom_class, atom_buried = np.full(L, 255), np.full(L, 255)
    for s, a in enumerate(lig):
        if cls[a] == 2:
            q = np.rint((xd[a] - o) / h)
            if (q >= 0).all() and (q <= n - 1).all():
                q = q.astype(int)
                atom_class[s], atom_buried[s] = cl[tuple(q)], buried[tuple(q)]
    start, atom = csr(c)
    near = np.zeros((R, n ** 3), dtype=bool)
    band = b1 + b2
    for r in range(R):
        run = atom[start[r]:start[r + 1]]
        m, b = spheres(xd, run, rad[run] + c["lining"], o, h, n, shift)
        near[r], band = m.reshape(-1), band + b
    lining_points = (near & site.reshape(-1)[None]).sum(1)
    out.update(ok=1, classes=cl.reshape(-1), buried=buried.reshape(-1), counts=counts, truncated=int((site & face).any()), atom_class=atom_class,
               atom_buried=atom_buried, lining_points=lining_points, lining_residues=int((lining_points > 0).sum()), band=band,
               flags=np.concatenate([solid.reshape(-1), inside.reshape(-1), near.reshape(-1)]))
    return out


def restate(c, x=None, centre="case", margin=MARGIN):
    """dict of [P, ...] arrays - ok, centre, classes, buried, counts, truncated, atom_class, atom_buried, lining_points, lining_residues -
    with every threshold moved by -margin; open_flags: the number of flags that differ from the evaluation at +margin; band: the pairs
    within BAND of a threshold"""
    x = np.asarray(c["x"] if x is None else x)
    centre = c["centre"] if isinstance(centre, str) else centre
    rows, open_flags, band = [], 0, 0
    for p in range(x.shape[0]):
        ctr = None if centre is None else np.asarray(centre, dtype=np.float64).reshape(-1, 3)[p if np.ndim(centre) == 2 else 0]
        lo, hi = pose(c, x[p], ctr, -margin), pose(c, x[p], ctr, +margin)
        open_flags += int((lo["flags"] != hi["flags"]).sum())
        band += lo["band"]
        rows.append(lo)
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0] if k not in ("flags", "band")}
    out.update(open_flags=open_flags, band=band)
    return out


def values_of(c, counts, atom_buried):
    """the six floats in float64 from integer outputs (counts [P,8], atom_buried [P,L]) with their derived fp32 bounds: name -> (value
    [P], bound [P]).  (A pose with ok = 0 is not covered: its floats are NaN.)"""
    counts = np.asarray(counts, dtype=np.float64)
    h3 = float(c["h"]) ** 3
    site, occ, pocket, ligand = counts[:, 3], counts[:, 4], counts[:, 2], counts[:, 5]
    has = np.asarray(atom_buried) != 255
    num, den = np.where(has, atom_buried, 0).sum(1).astype(np.float64), 7.0 * has.sum(1)
    ratio = lambda a, b: np.where(b > 0, a / np.where(b > 0, b, 1.0), 0.0)
    out = {"site_volume": site * h3, "unfilled_volume": (site - occ) * h3, "pocket_volume": pocket * h3}
    out = {k: (v, (U + 2.0 ** -50) * v) for k, v in out.items()}
    for k, v in (("filled_fraction", ratio(occ, site)), ("ligand_in_site", ratio(occ, ligand)), ("ligand_enclosure", ratio(num, den))):
        out[k] = (v, 2 * U * v)
    return out


# ------------------------------------------------------------------ the seeded cases of tests/test_pocket_gpu.py
CENTRE = np.array([20.0, 21.0, 19.0])
BALL = 6.6                                              # radius (A) of the ball the 70 atoms of case a are packed into
CAVITY = 5.2                                            # radius of the cavity carved out of it
SPACING = 1.3                                           # smallest distance between two atoms of a packed pose
PITCH = 1.6                                             # pitch of the jittered atom grid the larger receptors are cut from
ELEMENTS = (6, 6, 6, 7, 8, 16)
LIG9 = (0, 5, 17, 18, 33, 40, 41, 63, 69)

#: name -> seed; every seed was found by a short search for a closed case (tests/test_pocket_cpu.py asserts it)
CASES = {"a": 1, "b": 1, "c": 1, "d": 0, "e": 1, "f": 1, "g": 1, "h": 1}
#: case g: the atom a_mask removes, the inactive ligand atom (position in lig_idx), the hydrogen (a receptor atom), the ligand atom
#: (position) moved outside the lattice, and the (pose, receptor atom) that holds a NaN
G_HOLE, G_INACTIVE, G_HYDROGEN, G_OUTSIDE, G_NAN = 7, 3, 11, 6, (1, 30)
#: case h: the receptor atoms replaced by planted ones: four at the solid threshold (radius + probe) of a cavity point, -+ 1e-6 A, and
#: two at the lining threshold (radius + lining)
H_PLANTED = (1, 2, 3, 4, 6, 8)
#: ... and the lattice points they are planted for, as offsets from the centre point of the lattice (n = 9: the centre is a point)
H_TARGETS = ((0, 0, 0), (0, 1, 0), (0, -1, 1), (0, 0, -1), (-1, 1, 1), (-1, -1, 0))
PLANT = 1e-6


def packed(rng, n, centre, lo, hi, taken=()):
    """n points in the shell lo <= |q| <= hi around `centre`, no two (nor one of `taken`) closer than SPACING"""
    pts = [np.asarray(t) - centre for t in taken]
    k = len(pts)
    while len(pts) < k + n:
        q = rng.uniform(-hi, hi, 3)
        if lo ** 2 <= (q ** 2).sum() <= hi ** 2 and all(((q - w) ** 2).sum() >= SPACING ** 2 for w in pts):
            pts.append(q)
    return np.asarray(pts[k:]) + centre


def atom_grid(rng, keep, extent):
    """the points of a cubic grid of pitch PITCH around CENTRE, jittered by 0.1 A, for which keep(offset from CENTRE) holds"""
    m = int(extent / PITCH) + 1
    q = np.stack(np.meshgrid(*[np.arange(-m, m + 1) * PITCH] * 3, indexing="ij"), -1).reshape(-1, 3)
    q = q + rng.uniform(-0.1, 0.1, q.shape)
    return q[np.asarray([bool(keep(v)) for v in q])] + CENTRE


def tunnel_points():
    """case d: a serpentine of lattice points (i, j, k) in the plane k = 8 of a 16^3 lattice, one point wide, in walking order"""
    pts = []
    for r, i in enumerate(range(2, 14, 2)):
        js = list(range(2, 14)) if r % 2 == 0 else list(range(13, 1, -1))
        pts += [(i, j, 8) for j in js]
        if i + 2 < 14:
            pts.append((i + 1, js[-1], 8))
    return pts


def build(x, elements, lig, n, centre=None, radius=None, **kw):
    """a case from poses x [P,A,3], elements [A] and the ligand's atoms: the defaults, residues of eight atoms in two runs of four"""
    P_, A = x.shape[:2]
    lig = np.asarray(lig)
    receptor_mask = np.ones(A, dtype=np.uint8)
    receptor_mask[lig] = 0
    n_residues = min(max(A // 8, 1), 4096)
    c = dict(x=np.asarray(x, dtype=np.float32), elements=np.asarray(elements), radius=radii_of(elements) if radius is None else
             np.asarray(radius, dtype=np.float32), lig_idx=lig.astype(np.int32), lig_active=np.ones(len(lig), dtype=np.uint8),
             receptor_mask=receptor_mask, a_mask=np.ones(A, dtype=np.uint8), residue_of=((np.arange(A) // 4) % n_residues).astype(np.int32),
             n_residues=n_residues, h=H, n=n, probe=PROBE, lining=LINING, reach=REACH, min_enclosed=MIN_ENCLOSED, snap=True, centre=centre)
    c.update(kw)
    return c


def ball_poses(rng, n_pose, A, lig, offset):
    """case a: per pose its own packing - the ligand's atoms in a ball of 1.9 A around CENTRE + offset, the others in the shell CAVITY ..
    BALL around CENTRE"""
    x = np.empty((n_pose, A, 3))
    rec = np.setdiff1d(np.arange(A), lig)
    for p in range(n_pose):
        x[p, lig] = packed(rng, len(lig), CENTRE + offset, 0.0, 1.9)
        x[p, rec] = packed(rng, len(rec), CENTRE, CAVITY, BALL)
    return x


def plant(c):
    """case h: replace the receptor atoms H_PLANTED of every pose by atoms on the +x axis of a lattice point of the cavity, at the solid
    threshold (the first four: -, +, -, +) or the lining threshold (the last two: -, +) moved by PLANT, on the fp32 grid"""
    cls, lig = classes(c), c["lig_idx"]
    for p in range(c["x"].shape[0]):
        ctr = centre_of(c["x"][p], cls, lig, c["h"])
        for m, (a, t) in enumerate(zip(H_PLANTED, H_TARGETS)):
            g = ctr + np.asarray(t) * c["h"]                          # the lattice has an odd n: its centre is a point
            T = float(c["radius"][a]) + (c["probe"] if m < 4 else c["lining"])
            want = T + (-PLANT if m % 2 == 0 else PLANT)
            xa = np.float32(g[0] + want)
            best = min((np.nextafter(xa, np.float32(-1e9)), xa, np.nextafter(xa, np.float32(1e9))),
                       key=lambda v: abs((float(v) - g[0]) - want))
            c["x"][p, a] = (best, np.float32(g[1]), np.float32(g[2]))
    return c


def make_case(name):
    """dict(x fp32 [P,A,3], elements, radius fp32 [A], lig_idx, lig_active, receptor_mask, a_mask, residue_of, n_residues, h, n, probe,
    lining, reach, min_enclosed, snap, centre (None: the ligand's))"""
    rng = np.random.default_rng(4100 + 17 * CASES[name] + ord(name))
    if name in "aegh":
        A, lig = 70, np.asarray(LIG9)
        elements = np.asarray(ELEMENTS)[rng.integers(0, len(ELEMENTS), A)]
        x = ball_poses(rng, 3, A, lig, np.array([0.7, 0.0, 0.0]))
        if name == "e":
            x[:, lig] += np.array([0.0, 30.0, 0.0])                   # the ligand far outside the receptor
        c = build(x, elements, lig, 9)
        if name == "g":
            c["a_mask"][G_HOLE] = 0
            c["lig_active"][G_INACTIVE] = 0
            c["elements"][G_HYDROGEN] = 1
            c["radius"] = radii_of(c["elements"])
            c["x"][:, lig[G_OUTSIDE]] = (CENTRE + np.array([7.5, 0.0, 0.0])).astype(np.float32)
        if name == "h":
            plant(c)
        return c
    if name == "b":                                                  # two cavities 6.6 A apart in a ball of 9.5 A, the ligand in the first
        holes = np.array([[-3.3, 0.0, 0.0], [3.3, 0.0, 0.0]])
        rec = atom_grid(rng, lambda v: (v ** 2).sum() <= 9.5 ** 2 and (((v - holes) ** 2).sum(-1) >= 4.7 ** 2).all(), 9.5)
        ligx = packed(rng, 5, CENTRE + holes[0], 0.0, 1.2)
        x = np.concatenate([ligx, rec])[None]
        elements = np.asarray(ELEMENTS)[rng.integers(0, len(ELEMENTS), x.shape[1])]
        return build(x, elements, np.arange(5), 16, centre=CENTRE)
    if name == "c":                                                  # n = 33, A = 530: one cavity in a ball cut to 521 receptor atoms
        rec = atom_grid(rng, lambda v: CAVITY ** 2 <= (v ** 2).sum() <= 11.0 ** 2, 11.0)
        rec = rec[np.argsort(((rec - CENTRE) ** 2).sum(-1), kind="stable")][:521]
        assert len(rec) == 521
        x = np.stack([np.concatenate([packed(rng, 9, CENTRE + np.array([0.7, 0.0, 0.0]), 0.0, 1.9), rec]) for _ in range(2)])
        elements = np.asarray(ELEMENTS)[rng.integers(0, len(ELEMENTS), 530)]
        return build(x, elements, np.arange(9), 33)
    if name == "d":                                                  # a block of atoms ON the lattice points, the tunnel carved out
        n = 16
        o = CENTRE - (n - 1) / 2                                     # half integers: every lattice point is an fp32 number
        tun = tunnel_points()
        hole = np.zeros((n, n, n), dtype=bool)
        hole[tuple(np.asarray(tun).T)] = True
        rec = o + np.stack(np.nonzero(~hole), -1)
        ligx = o + np.asarray(tun[:2], dtype=np.float64)              # two ligand atoms on the first two points of the tunnel
        x = np.concatenate([ligx, rec])[None]
        A = x.shape[1]
        return build(x, np.full(A, 6), np.arange(2), n, centre=CENTRE, radius=np.full(A, 0.3), probe=F32(0.3), lining=F32(1.2))
    if name == "f":                                                  # a tube along x through the whole lattice; a point on a face has
        # at most two enclosed directions (the five with a component along the face's normal leave the lattice), hence min_enclosed = 2
        rec = atom_grid(rng, lambda v: abs(v[0]) <= 8.0 and 4.7 ** 2 <= v[1] ** 2 + v[2] ** 2 <= 8.0 ** 2, 8.0)
        ligx = packed(rng, 5, CENTRE, 0.0, 1.2)
        x = np.concatenate([ligx, rec])[None]
        elements = np.asarray(ELEMENTS)[rng.integers(0, len(ELEMENTS), x.shape[1])]
        return build(x, elements, np.arange(5), 9, min_enclosed=2)
    raise KeyError(name)
