"""Float64 definition of the best-fit (superposed) symmetry-corrected ligand RMSD (kernel pd_bestfit_rmsd, csrc/bestfit_rmsd.hip) in
plain numpy - the yardstick of tests/test_bestfit_rmsd_cpu.py and tests/test_bestfit_rmsd_gpu.py.  Nothing of physdock_amd is imported.

    a, b [L,3]      two ligands, each centred on its unweighted centroid in float64; G = sum of squared norms
    msd(a, b, m)  = min over PROPER rotations R of (1/L) sum_k |R a[k] - b[perm[m][k]]|^2
                  = (G_a + G_b - 2 lambda_max(N(a, b o perm_m))) / L                                        (Horn 1987)
    bestfit(a, b) = sqrt(max(0, min_m msd)), the smallest m wins a tie; without a table the identity alone

The permutation acts on the b side.  A mirror image is not a match.  L = 1 gives 0.  A non-finite coordinate in either structure gives
NaN for the value, -1 for the row and NaN for the quaternion.  The optimal rotation is the unit quaternion (w, x, y, z), the eigenvector
of lambda_max, first non-zero component positive: R(q) a ~ b o perm_m.

Two independent restatements of msd: `msd_svd` (the 3x3 SVD with the determinant correction, Kabsch) and `msd_horn` (eigvalsh of the
4x4 matrix).  Their difference E is what float64 arithmetic alone costs on an input; `bound` turns it into the tolerance

    B = 4 E + (L + 64) 2^-52 (G_a + G_b) / L      in msd        |D - sqrt(msd_ref)| <= sqrt(B) + 1 ulp32(sqrt(msd_ref))

(the second term: the first-order forward bound of L-term fixed-order float64 sums plus the eigen-solve; sqrt(B) from
|sqrt(x) - sqrt(y)| <= sqrt(|x - y|))."""
import numpy as np

EPS52 = 2.0 ** -52


def centred(a):
    a = np.asarray(a, dtype=np.float64)
    return a - a.mean(0, keepdims=True)


def horn_matrix(S):
    """Horn's symmetric 4x4 matrix of the covariance S[x][y] = sum_k a[k][x] b[k][y]"""
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    return np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                     [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                     [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                     [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]], dtype=np.float64)


def msd_horn(a, b):
    """a, b [L,3] CENTRED -> the msd over proper rotations, not clamped (may be a few ulp of G / L below 0)"""
    G = (a * a).sum() + (b * b).sum()
    return (G - 2.0 * np.linalg.eigvalsh(horn_matrix(a.T @ b))[-1]) / a.shape[0]


def msd_svd(a, b):
    """the same by Kabsch: singular values of the covariance, the smallest negated when the best orthogonal map is a reflection"""
    G = (a * a).sum() + (b * b).sum()
    U, s, Vt = np.linalg.svd(a.T @ b)
    d = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    return (G - 2.0 * (s[0] + s[1] + (d if d != 0 else 1.0) * s[2])) / a.shape[0]


def quaternion(a, b):
    """the unit eigenvector (w, x, y, z) of lambda_max, first non-zero component positive"""
    w, v = np.linalg.eigh(horn_matrix(a.T @ b))
    q = v[:, -1] / np.linalg.norm(v[:, -1])
    nz = np.nonzero(q)[0]
    return q if not len(nz) or q[nz[0]] > 0 else -q


def rotation(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def msd_of_quaternion(a, b, q):
    """(1/L) sum |R(q) a - b|^2 of CENTRED a, b, evaluated directly"""
    d = a @ rotation(np.asarray(q, dtype=np.float64)).T - b
    return (d * d).sum() / a.shape[0]


def bound(E, L, G):
    """B of the module docstring, in msd; G = G_a + G_b"""
    return 4.0 * E + (L + 64) * EPS52 * G / L


def ulp32(v):
    s = np.float32(abs(v))
    return float(np.nextafter(s, np.float32(np.inf)) - s)


def value_bound(B, rmsd):
    return float(np.sqrt(B)) + ulp32(rmsd)


def bestfit(a, b, perms=None):
    """a, b [L,3] (not centred) -> dict(rmsd, row, quat [4], msd [M] (msd_horn per table row), msd_svd [M], E, B, G).  E is the difference
    of the two restatements' minima, B the bound of that comparison."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    L = a.shape[0]
    perms = np.arange(L)[None] if perms is None else np.asarray(perms, dtype=np.int64)
    M = perms.shape[0]
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        nan = np.full(M, np.nan)
        return dict(rmsd=np.nan, row=-1, quat=np.full(4, np.nan), msd=nan, msd_svd=nan, E=np.nan, B=np.nan, G=np.nan)
    a, b = centred(a), centred(b)
    G = float((a * a).sum() + (b * b).sum())
    horn = np.array([msd_horn(a, b[p]) for p in perms])
    svd = np.array([msd_svd(a, b[p]) for p in perms])
    row = int(np.argmin(np.maximum(horn, 0.0)))                       # the first of equal (clamped) minima
    E = float(abs(svd.min() - horn.min()))
    return dict(rmsd=float(np.sqrt(max(0.0, horn[row]))), row=row, quat=quaternion(a, b[perms[row]]), msd=horn, msd_svd=svd, E=E,
                B=bound(E, L, G), G=G)


def gather(x, idx, L):
    x = np.asarray(x)
    return x[:, np.arange(L) if idx is None else np.asarray(idx, dtype=np.int64)].astype(np.float64)


def cross(xa, idx_a, xb, idx_b, perms=None, L=None):
    """xa [na,Aa,3], xb [nb,Ab,3] -> a [na][nb] list of lists of `bestfit` dicts: rows fixed, columns permuted"""
    L = int(np.asarray(perms).shape[1] if perms is not None else (len(idx_a) if idx_a is not None else L))
    a, b = gather(xa, idx_a, L), gather(xb, idx_b, L)
    return [[bestfit(p, q, perms) for q in b] for p in a]


def field(res, key):
    """one entry of every dict of `cross` as an array [na,nb(,..)]"""
    return np.array([[r[key] for r in row] for row in res])


def pairwise(x, idx, perms=None, L=None):
    """the symmetric form: i < j computed (pose i fixed, pose j permuted) and mirrored, the diagonal zero -> D [n,n], B [n,n]"""
    res = cross(x, idx, x, idx, perms, L)
    n = len(res)
    D, B = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            D[i, j] = D[j, i] = res[i][j]["rmsd"]
            B[i, j] = B[j, i] = res[i][j]["B"]
    return D, B
