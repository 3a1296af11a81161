"""Float64 restatement of the pose-validity checks (kernel pd_pose_validity) in plain numpy - the yardstick of
tests/test_validity_cpu.py and tests/test_validity_gpu.py.  Nothing of physdock_amd is imported here.

Per pose p, with x_a the position of ligand atom a (pose atom lig_idx[a]), r a van der Waals radius and d(.,.) a distance:

    val[p,0], val[p,1]  min, max over the bonded pairs (a, b) of d(a, b) / d12_ref
    val[p,2], val[p,3]  min, max over the 1-3 pairs (a, b) of d(a, b) / d13_ref
    val[p,4]            min over a < b with far[a, b], both active, of d(a, b) / (r_a + r_b)
    val[p,5]            min over active ligand atoms a and receptor atoms j (rec_mask) of d(a, j) / (r_a + r_j)
    val[p,6]            min over the same pairs of d(a, j)
    val[p,7]            max over planar groups and their atoms of the distance to the group's least-squares plane: the plane through
                        the centroid whose normal is the eigenvector of the smallest eigenvalue of the covariance matrix
                        (np.linalg.eigh); 0 for a group whose second eigenvalue is at most 1e-10 of its largest
    worst[p]            the (a, j) that attains val[p,5], the lexicographically smallest on a tie; (-1, -1) without a pair

Empty sets give 1 (columns 0 - 3), +inf (4 - 6) and 0 (7).  `fp32=True` evaluates the distances and ratios of columns 0 - 6 in
numpy float32 (differences, squares, their sum, sqrt, the quotient: every operation rounded to fp32); column 7 is float64 always.
"""
import numpy as np

#: bit order of the flags, and the thresholds in the order of pd_validity_thresholds
CHECK_NAMES = ("bond_lengths", "bond_angles", "internal_clash", "receptor_clash", "planarity", "detached")
DEFAULT_THRESHOLDS = {"bond_lo": 0.75, "bond_hi": 1.25, "angle_lo": 0.75, "angle_hi": 1.25, "internal_clash": 0.7,
                      "receptor_clash": 0.75, "planarity": 0.25, "detached": 8.0}
COLLINEAR = 1e-10


def _dist(a, b):
    d = a - b
    return np.sqrt((d * d).sum(-1))


def plane_distance(pts):
    """largest distance of the points [n,3] to their least-squares plane, float64 -> (distance, eigenvalues ascending)"""
    pts = np.asarray(pts, dtype=np.float64)
    c = pts - pts.mean(0)
    w, v = np.linalg.eigh(c.T @ c / len(pts))
    if not w[1] > COLLINEAR * w[2]:
        return 0.0, w
    return float(np.abs(c @ v[:, 0]).max()), w


def pose_validity(x, lig_idx, radius, rec_mask, lig_active, pair12, d12_ref, pair13, d13_ref, far, planar, fp32=False):
    """-> dict(val [P,8] float64, worst [P,2] int64, rec [P,L,A] the ratios behind column 5 (+inf where a pair does not count),
    eig [P,G,3] the eigenvalues of the planar groups)"""
    ft = np.float32 if fp32 else np.float64
    x = np.asarray(x, dtype=np.float32)
    P, A = x.shape[:2]
    lig_idx = np.asarray(lig_idx, dtype=np.int64)
    L = len(lig_idx)
    r = np.asarray(radius, dtype=np.float32).astype(ft)
    rec = np.asarray(rec_mask).astype(bool)
    act = np.asarray(lig_active).astype(bool)
    pair12, pair13 = np.asarray(pair12, dtype=np.int64).reshape(-1, 2), np.asarray(pair13, dtype=np.int64).reshape(-1, 2)
    far = np.asarray(far).astype(bool).reshape(L, L)
    planar = np.asarray(planar, dtype=np.int64).reshape(-1, 8)
    val = np.zeros((P, 8), dtype=np.float64)
    worst = -np.ones((P, 2), dtype=np.int64)
    rec_all = np.full((P, L, A), np.inf)
    eig = np.zeros((P, len(planar), 3))
    iu, ju = np.triu_indices(L, 1)
    far_ok = far[iu, ju] & act[iu] & act[ju]
    for p in range(P):
        xl = x[p, lig_idx].astype(ft)
        for col, pairs, ref in ((0, pair12, d12_ref), (2, pair13, d13_ref)):
            if len(pairs):
                q = _dist(xl[pairs[:, 0]], xl[pairs[:, 1]]) / np.asarray(ref, dtype=np.float32).astype(ft)
                val[p, col], val[p, col + 1] = q.min(), q.max()
            else:
                val[p, col] = val[p, col + 1] = 1.0
        q = _dist(xl[iu[far_ok]], xl[ju[far_ok]]) / (r[lig_idx][iu[far_ok]] + r[lig_idx][ju[far_ok]])
        val[p, 4] = q.min() if q.size else np.inf
        d = _dist(xl[:, None, :], x[p].astype(ft)[None, :, :])                       # [L, A]
        ok = act[:, None] & rec[None, :]
        ratio = np.where(ok, (d / (r[lig_idx][:, None] + r[None, :])).astype(np.float64), np.inf)
        rec_all[p] = ratio
        if ok.any():
            k = int(np.argmin(ratio))                                               # the first minimum in (a, j) order
            worst[p] = (k // A, k % A)
            val[p, 5] = ratio.reshape(-1)[k]
            val[p, 6] = np.where(ok, d.astype(np.float64), np.inf).min()
        else:
            val[p, 5] = val[p, 6] = np.inf
        for g, row in enumerate(planar):
            dist, eig[p, g] = plane_distance(x[p, lig_idx[row[row >= 0]]])
            val[p, 7] = max(val[p, 7], dist)
    return {"val": val, "worst": worst, "rec": rec_all, "eig": eig}


def flags(val, thresholds=None):
    """the bit mask of failed checks of val [P,8] (any float type; compared as given)"""
    t = dict(DEFAULT_THRESHOLDS)
    t.update(thresholds or {})
    v = np.asarray(val)
    t = {k: v.dtype.type(x) for k, x in t.items()}
    bits = [(v[:, 0] < t["bond_lo"]) | (v[:, 1] > t["bond_hi"]), (v[:, 2] < t["angle_lo"]) | (v[:, 3] > t["angle_hi"]),
            v[:, 4] < t["internal_clash"], v[:, 5] < t["receptor_clash"], v[:, 7] > t["planarity"],
            (v[:, 6] > t["detached"]) & np.isfinite(v[:, 6])]
    return sum(b.astype(np.int64) << i for i, b in enumerate(bits))


def margins(val, thresholds=None):
    """distance of every compared value of val [P,8] to the threshold it is compared with: [P,8] (column 6: to `detached`)"""
    t = dict(DEFAULT_THRESHOLDS)
    t.update(thresholds or {})
    v = np.asarray(val, dtype=np.float64)
    thr = [(t["bond_lo"],), (t["bond_hi"],), (t["angle_lo"],), (t["angle_hi"],), (t["internal_clash"],), (t["receptor_clash"],),
           (t["detached"],), (t["planarity"],)]
    return np.stack([np.abs(v[:, c] - thr[c][0]) for c in range(8)], -1)
