"""Float64 restatement of the receptor-geometry checks (kernels pd_receptor_geometry, pd_receptor_dihedrals) in plain numpy - the
yardstick of tests/test_receptor_geometry_cpu.py and tests/test_receptor_geometry_gpu.py - and a NeRF builder of test peptides from
nominal internal coordinates.  Nothing of physdock_amd is imported here.

Tables (`t`, the host arrays of a `ReceptorGeometry`): radius_signed [A] (negative = the atom takes no part), excl_start / excl_atom (CSR
per atom over the excluded partners with a higher index), term_atoms [T,10] (-1 padded) and term_ref [T] in the order bonds, 1-3 pairs,
centres, peptide terms, groups (`term_counts`), res_term_start / res_term and res_atom_start / res_atom (CSR per residue).  Per pose:

    bond, 1-3 term (a, b; l)       value d(a, b) / l, bit 0 / 1 unless lo <= value <= hi; not finite -> +inf, fails
    centre (c, a, b, e; s)         value s (a - c) . ((b - c) x (e - c)), bit 2 unless > 0; a coordinate not finite -> -inf, fails
    peptide (CA, C, N', CA'; tr)   w = dihedral; value min(|w|, 180 - |w|), bit 3 when > twist; bit 4 when tr and |w| < cis; w NaN -> +inf, bit 3
    group                          value = largest distance to the least-squares plane (np.linalg.eigh; 0 when the second eigenvalue
                                   is at most 1e-10 of the largest), bit 5 when > planarity; a coordinate not finite -> +inf, fails
    clash pair i < j               both radii > 0, not excluded: q = d / (r_i + r_j), bit 6 when < clash; a coordinate not finite -> q = 0

    val[p] = (min, max bond value; min, max 1-3 value; min q; max group value; max peptide value; number of failing centres) with 1 for
    no bonds / 1-3 pairs, +inf for no pair, 0 for no group / peptide; worst[p] the first pair in (i, j) order that attains min q;
    counts[p,b] failing terms (pairs) of bit b; flags bit b = counts > 0; residue_flags[p,r] = OR of the bits of the terms of r, bit 6
    when one of its atoms is in a failing pair; atom_clash[p,i] likewise.

`fp32=True` evaluates the bond, 1-3 and clash values in numpy float32 (every operation rounded); the rest is float64 always.
dihedral(p0..p3) = atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3)) in degrees, NaN when an index is -1, a coordinate is not finite
or a cross product is shorter than 1e-6."""
import numpy as np

CHECK_NAMES = ("bond_lengths", "bond_angles", "chirality", "peptide_twist", "cis_flip", "planarity", "clash")
DEFAULT_THRESHOLDS = {"bond_lo": 0.75, "bond_hi": 1.25, "angle_lo": 0.75, "angle_hi": 1.25, "clash": 0.7, "planarity": 0.25, "twist": 30.0,
                      "cis": 30.0, "trans": 150.0}
COLLINEAR = 1e-10


def dihedral(x, idx):
    """x [..., A, 3], idx [..., 4] -> degrees, float64 (x is rounded to fp32 first: what the device is given)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0).all(-1)
    p = x[..., np.where(idx >= 0, idx, 0), :]
    b1, b2, b3 = p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 1, :], p[..., 3, :] - p[..., 2, :]
    with np.errstate(invalid="ignore"):
        m, n = np.cross(b1, b2), np.cross(b2, b3)
        w = np.degrees(np.arctan2(np.linalg.norm(b2, axis=-1) * (b1 * n).sum(-1), (m * n).sum(-1)))
        ok = ok & np.isfinite(p).all((-1, -2)) & (np.linalg.norm(m, axis=-1) >= 1e-6) & (np.linalg.norm(n, axis=-1) >= 1e-6)
    return np.where(ok, w, np.nan)


def wrap(diff, pi_periodic=False):
    """an angle difference in degrees wrapped to (-180, 180], or to (-90, 90] for a pi-periodic angle"""
    period = 180.0 if pi_periodic else 360.0
    w = np.remainder(diff, period)
    return w - period if w > period / 2 else w


def chi_recovery(angles, chi_ref, pi_periodic, tolerance=40.0, residues=None):
    """angles [P,R,7], chi_ref [R,4], pi_periodic [R,4] -> (matched [P], compared [P], rotamer_ok [P,R])"""
    P, R = angles.shape[:2]
    matched, compared, ok = np.zeros(P, int), np.zeros(P, int), np.zeros((P, R), bool)
    sel = np.ones(R, bool) if residues is None else np.isin(np.arange(R), residues)
    for p in range(P):
        for r in np.nonzero(sel)[0]:
            good = []
            for k in range(4):
                a, b = float(angles[p, r, 3 + k]), float(chi_ref[r, k])
                if not (np.isnan(a) or np.isnan(b)):
                    good.append(abs(wrap(a - b, bool(pi_periodic[r, k]))) <= tolerance)
            matched[p] += sum(good)
            compared[p] += len(good)
            ok[p, r] = bool(good) and all(good)
    return matched, compared, ok


def plane_distance(pts):
    pts = np.asarray(pts, dtype=np.float64)
    c = pts - pts.mean(0)
    w, v = np.linalg.eigh(c.T @ c / len(pts))
    if not w[1] > COLLINEAR * w[2]:
        return 0.0
    return float(np.abs(c @ v[:, 0]).max())


def _dist(a, b):
    d = a - b
    return np.sqrt((d * d).sum(-1))


def receptor_geometry(x, t, thresholds=None, fp32=False):
    """-> dict(val [P,8], worst [P,2], counts [P,7], flags [P], residue_flags [P,R], atom_clash [P,A], term_val [P,T], term_fail [P,T],
    ratio [P,A,A]: q of every counted pair i < j, +inf elsewhere)"""
    thr = dict(DEFAULT_THRESHOLDS)
    thr.update(thresholds or {})
    ft = np.float32 if fp32 else np.float64
    x = np.asarray(x, dtype=np.float32)
    P, A = x.shape[:2]
    r = np.asarray(t["radius_signed"], dtype=np.float32)
    nb, na, nc, npep, ng = t["term_counts"]
    o = np.cumsum([nb, na, nc, npep, ng])
    atoms, ref = np.asarray(t["term_atoms"], dtype=np.int64).reshape(-1, 10), np.asarray(t["term_ref"], dtype=np.float32)
    T, R = int(o[-1]), len(t["res_term_start"]) - 1
    excluded = np.zeros((A, A), bool)
    for i in range(A):
        excluded[i, t["excl_atom"][t["excl_start"][i]:t["excl_start"][i + 1]]] = True
    counted = np.triu(np.ones((A, A), bool), 1) & (r > 0)[:, None] & (r > 0)[None, :] & ~excluded
    val, worst = np.zeros((P, 8)), -np.ones((P, 2), np.int64)
    counts, tv, tf = np.zeros((P, 7), np.int64), np.zeros((P, T)), np.zeros((P, T), np.int64)
    rflags, aclash, ratios = np.zeros((P, R), np.int64), np.zeros((P, A), np.int64), np.full((P, A, A), np.inf)
    lim = {k: ft(v) for k, v in thr.items()}
    for p in range(P):
        xf, xd = x[p].astype(ft), x[p].astype(np.float64)
        finite = np.isfinite(x[p]).all(-1)
        for k in range(T):
            at = atoms[k][atoms[k] >= 0]
            ok = bool(finite[at].all())
            if k < o[1]:
                bond = k < o[0]
                with np.errstate(invalid="ignore", over="ignore"):
                    q = float(_dist(xf[at[0]], xf[at[1]]) / ref[k].astype(ft)) if ok else np.inf
                q = q if np.isfinite(q) else np.inf
                lo, hi = (lim["bond_lo"], lim["bond_hi"]) if bond else (lim["angle_lo"], lim["angle_hi"])
                tv[p, k], tf[p, k] = q, 0 if (ft(q) >= lo and ft(q) <= hi) else (1 if bond else 2)
            elif k < o[2]:
                if ok:
                    v = xd[at[1:]] - xd[at[0]]
                    s = float(v[0] @ np.cross(v[1], v[2])) * float(ref[k])
                tv[p, k], tf[p, k] = (s, 0 if s > 0 else 4) if ok else (-np.inf, 4)
            elif k < o[3]:
                w = float(dihedral(x[p], at))
                if np.isnan(w):
                    tv[p, k], tf[p, k] = np.inf, 8
                else:
                    tw = min(abs(w), 180.0 - abs(w))
                    tv[p, k] = tw
                    tf[p, k] = (8 if tw > float(np.float32(thr["twist"])) else 0) | (16 if ref[k] > 0.5 and abs(w) < float(np.float32(thr["cis"])) else 0)
            else:
                d = plane_distance(xd[at]) if ok else np.inf
                tv[p, k], tf[p, k] = d, 32 if np.float32(d) > np.float32(thr["planarity"]) else 0
        with np.errstate(invalid="ignore", over="ignore"):
            q = (_dist(xf[:, None, :], xf[None, :, :]) / (r.astype(ft)[:, None] + r.astype(ft)[None, :])).astype(np.float64)
        q[~finite, :] = 0.0
        q[:, ~finite] = 0.0
        q = np.where(counted, q, np.inf)
        ratios[p] = q
        fail = counted & (q < float(lim["clash"]))
        aclash[p] = fail.any(0) | fail.any(1)
        for b in range(6):
            counts[p, b] = int(((tf[p] >> b) & 1).sum())
        counts[p, 6] = int(fail.sum())
        seg = lambda a, b: tv[p, a:b]
        val[p, 0], val[p, 1] = (seg(0, o[0]).min(), seg(0, o[0]).max()) if nb else (1, 1)
        val[p, 2], val[p, 3] = (seg(o[0], o[1]).min(), seg(o[0], o[1]).max()) if na else (1, 1)
        val[p, 4] = q.min() if counted.any() else np.inf
        if counted.any():
            k = int(np.argmin(q))
            worst[p] = (k // A, k % A)
        val[p, 5] = seg(o[3], o[4]).max() if ng else 0.0
        val[p, 6] = seg(o[2], o[3]).max() if npep else 0.0
        val[p, 7] = counts[p, 2]
        for s in range(R):
            for k in t["res_term"][t["res_term_start"][s]:t["res_term_start"][s + 1]]:
                rflags[p, s] |= tf[p, k]
            if aclash[p, t["res_atom"][t["res_atom_start"][s]:t["res_atom_start"][s + 1]]].any():
                rflags[p, s] |= 64
    flags = sum((counts[:, b] > 0).astype(np.int64) << b for b in range(7))
    return {"val": val, "worst": worst, "counts": counts, "flags": flags, "residue_flags": rflags, "atom_clash": aclash, "term_val": tv,
            "term_fail": tf, "ratio": ratios}


def term_thresholds(t, thresholds=None):
    """per term the thresholds its value is compared with: [T,2] (NaN = no second threshold)"""
    thr = dict(DEFAULT_THRESHOLDS)
    thr.update(thresholds or {})
    nb, na, nc, npep, ng = t["term_counts"]
    rows = [(thr["bond_lo"], thr["bond_hi"])] * nb + [(thr["angle_lo"], thr["angle_hi"])] * na + [(0.0, np.nan)] * nc + \
        [(thr["twist"], np.nan)] * npep + [(thr["planarity"], np.nan)] * ng
    return np.asarray(rows, dtype=np.float64).reshape(-1, 2)


# ------------------------------------------------------------------ test peptides
def place(a, b, c, length, angle, torsion):
    """NeRF: the point d with |d - c| = length, angle(b, c, d) = angle and dihedral(a, b, c, d) = torsion (degrees)"""
    th, ta = np.radians(angle), np.radians(torsion)
    bc = (c - b) / np.linalg.norm(c - b)
    n = np.cross(b - a, bc)
    n /= np.linalg.norm(n)
    m = np.cross(n, bc)
    return c + length * (-np.cos(th) * bc + np.sin(th) * np.cos(ta) * m + np.sin(th) * np.sin(ta) * n)


# side chains beyond CB: (atom, a, b, c, length, angle, torsion) with torsion = (chi number or 0, offset in degrees)
def _ring6(first, prev2, prev1):
    """a regular hexagon CG CD1 CE1 CZ CE2 CD2 hanging on CB"""
    return [("CD1", prev2, prev1, first, 1.39, 120.0, (2, 0.0)), ("CD2", prev2, prev1, first, 1.39, 120.0, (2, 180.0)),
            ("CE1", prev1, first, "CD1", 1.39, 120.0, (0, 180.0)), ("CE2", prev1, first, "CD2", 1.39, 120.0, (0, 180.0)),
            ("CZ", first, "CD1", "CE1", 1.39, 120.0, (0, 0.0))]


_CHAIN = lambda name, a, b, c, k, length=1.53, angle=111.0: (name, a, b, c, length, angle, (k, 0.0))
SIDE_CHAINS = {
    "GLY": [], "ALA": [], "SER": [_CHAIN("OG", "N", "CA", "CB", 1, 1.42)], "CYS": [_CHAIN("SG", "N", "CA", "CB", 1, 1.81, 114.0)],
    "VAL": [_CHAIN("CG1", "N", "CA", "CB", 1), ("CG2", "N", "CA", "CB", 1.53, 111.0, (1, 120.0))],
    "THR": [_CHAIN("OG1", "N", "CA", "CB", 1, 1.43), ("CG2", "N", "CA", "CB", 1.53, 111.0, (1, -120.0))],
    "LEU": [_CHAIN("CG", "N", "CA", "CB", 1, 1.53, 116.0), _CHAIN("CD1", "CA", "CB", "CG", 2), ("CD2", "CA", "CB", "CG", 1.53, 111.0, (2, 120.0))],
    "ILE": [_CHAIN("CG1", "N", "CA", "CB", 1), ("CG2", "N", "CA", "CB", 1.53, 111.0, (1, -120.0)), _CHAIN("CD1", "CA", "CB", "CG1", 2, 1.53, 114.0)],
    "MET": [_CHAIN("CG", "N", "CA", "CB", 1, 1.53, 114.0), _CHAIN("SD", "CA", "CB", "CG", 2, 1.81, 112.7), _CHAIN("CE", "CB", "CG", "SD", 3, 1.79, 100.9)],
    "PRO": [("CG", "N", "CA", "CB", 1.50, 104.5, (0, 30.0)), ("CD", "CA", "CB", "CG", 1.50, 105.0, (0, -36.0))],
    "PHE": [_CHAIN("CG", "N", "CA", "CB", 1, 1.50, 114.0)] + _ring6("CG", "CA", "CB"),
    "TYR": [_CHAIN("CG", "N", "CA", "CB", 1, 1.50, 114.0)] + _ring6("CG", "CA", "CB") + [("OH", "CD1", "CE1", "CZ", 1.38, 120.0, (0, 180.0))],
    # a regular pentagon CG CD1 NE1 CE2 CD2 and a regular hexagon CD2 CE2 CZ2 CH2 CZ3 CE3 sharing the edge CD2 - CE2
    "TRP": [_CHAIN("CG", "N", "CA", "CB", 1, 1.50, 114.0), ("CD1", "CA", "CB", "CG", 1.39, 126.0, (2, 0.0)),
            ("CD2", "CA", "CB", "CG", 1.39, 126.0, (2, 180.0)), ("NE1", "CB", "CG", "CD1", 1.39, 108.0, (0, 180.0)),
            ("CE2", "CG", "CD1", "NE1", 1.39, 108.0, (0, 0.0)), ("CE3", "CD1", "CG", "CD2", 1.39, 132.0, (0, 180.0)),
            ("CZ2", "CD1", "NE1", "CE2", 1.39, 132.0, (0, 180.0)), ("CZ3", "CG", "CD2", "CE3", 1.39, 120.0, (0, 180.0)),
            ("CH2", "CD2", "CE3", "CZ3", 1.39, 120.0, (0, 0.0))],
    "HIS": [_CHAIN("CG", "N", "CA", "CB", 1, 1.50, 114.0), ("ND1", "CA", "CB", "CG", 1.38, 126.0, (2, 0.0)),
            ("CD2", "CA", "CB", "CG", 1.38, 126.0, (2, 180.0)), ("CE1", "CB", "CG", "ND1", 1.38, 108.0, (0, 180.0)),
            ("NE2", "CG", "ND1", "CE1", 1.38, 108.0, (0, 0.0))],
    "ASP": [_CHAIN("CG", "N", "CA", "CB", 1, 1.52, 113.0), _CHAIN("OD1", "CA", "CB", "CG", 2, 1.25, 119.0), ("OD2", "CA", "CB", "CG", 1.25, 119.0, (2, 180.0))],
    "ASN": [_CHAIN("CG", "N", "CA", "CB", 1, 1.52, 113.0), _CHAIN("OD1", "CA", "CB", "CG", 2, 1.23, 121.0), ("ND2", "CA", "CB", "CG", 1.33, 116.0, (2, 180.0))],
    "GLU": [_CHAIN("CG", "N", "CA", "CB", 1, 1.52, 114.0), _CHAIN("CD", "CA", "CB", "CG", 2, 1.52, 113.0), _CHAIN("OE1", "CB", "CG", "CD", 3, 1.25, 119.0),
            ("OE2", "CB", "CG", "CD", 1.25, 119.0, (3, 180.0))],
    "GLN": [_CHAIN("CG", "N", "CA", "CB", 1, 1.52, 114.0), _CHAIN("CD", "CA", "CB", "CG", 2, 1.52, 113.0), _CHAIN("OE1", "CB", "CG", "CD", 3, 1.23, 121.0),
            ("NE2", "CB", "CG", "CD", 1.33, 116.0, (3, 180.0))],
    "LYS": [_CHAIN("CG", "N", "CA", "CB", 1, 1.52, 114.0), _CHAIN("CD", "CA", "CB", "CG", 2), _CHAIN("CE", "CB", "CG", "CD", 3),
            _CHAIN("NZ", "CG", "CD", "CE", 4, 1.49, 111.7)],
    "ARG": [_CHAIN("CG", "N", "CA", "CB", 1, 1.52, 114.0), _CHAIN("CD", "CA", "CB", "CG", 2), _CHAIN("NE", "CB", "CG", "CD", 3, 1.46, 112.0),
            _CHAIN("CZ", "CG", "CD", "NE", 4, 1.33, 124.0), ("NH1", "CD", "NE", "CZ", 1.33, 120.0, (0, 0.0)), ("NH2", "CD", "NE", "CZ", 1.33, 120.0, (0, 180.0))],
}
ALL_TYPES = tuple(SIDE_CHAINS)
#: the chi angles a built side chain takes unless `chis` says otherwise: chi1 .. chi4
DEFAULT_CHIS = (-65.0, 95.0, 180.0, 180.0)
CB_TORSION = -122.6          # dihedral(C, N, CA, CB) of an L residue


def build_peptide(sequence, phi=-120.0, psi=130.0, omega=180.0, chis=None, oxt=False, origin=(0.0, 0.0, 0.0)):
    """An extended peptide from nominal internal coordinates -> (res_names, atom_names, residue_of, x [A,3] float64).  `chis`:
    {residue position: (chi1, ...)} overriding DEFAULT_CHIS."""
    res_names, atom_names, residue_of, xyz = [], [], [], []
    n = np.asarray(origin, dtype=np.float64)
    ca = n + [1.458, 0.0, 0.0]
    c = place(n + [0.0, 1.0, 0.0], n, ca, 1.525, 111.0, 180.0)
    for s, name in enumerate(sequence):
        at = {"N": n, "CA": ca, "C": c}
        n_next = place(n, ca, c, 1.329, 116.2, psi)
        at["O"] = place(n, ca, c, 1.231, 120.5, psi + 180.0)
        if name != "GLY":
            at["CB"] = place(c, n, ca, 1.53, 110.5, CB_TORSION)
        chi = list((chis or {}).get(s, ())) + list(DEFAULT_CHIS)[len((chis or {}).get(s, ())):]
        for atom, a, b, cc, length, angle, (k, offset) in SIDE_CHAINS[name]:
            at[atom] = place(at[a], at[b], at[cc], length, angle, (chi[k - 1] if k else 0.0) + offset)
        if oxt and s == len(sequence) - 1:
            at["OXT"] = n_next
        for atom, pos in at.items():
            res_names.append(name); atom_names.append(atom); residue_of.append(s); xyz.append(pos)
        ca_next = place(ca, c, n_next, 1.458, 121.7, omega)
        c_next = place(c, n_next, ca_next, 1.525, 111.0, phi)
        n, ca, c = n_next, ca_next, c_next
    return res_names, atom_names, np.asarray(residue_of), np.asarray(xyz)


def atom_index(res_names, atom_names, residue_of):
    """{(residue id, atom name): index}"""
    return {(int(r), a): k for k, (r, a) in enumerate(zip(residue_of, atom_names))}


def rotate_about(x, p, q, degrees, moving):
    """a copy of x with the atoms `moving` rotated by `degrees` about the axis p -> q (right-handed)"""
    x = x.copy()
    u = (q - p) / np.linalg.norm(q - p)
    a = np.radians(degrees)
    v = x[moving] - q
    x[moving] = q + v * np.cos(a) + np.cross(u, v) * np.sin(a) + np.outer(v @ u, u) * (1 - np.cos(a))
    return x


def mirror_through(x, atom, a, b, c):
    """a copy of x with `atom` reflected through the plane of a, b, c"""
    x = x.copy()
    n = np.cross(x[b] - x[a], x[c] - x[a])
    n /= np.linalg.norm(n)
    x[atom] = x[atom] - 2.0 * ((x[atom] - x[a]) @ n) * n
    return x
