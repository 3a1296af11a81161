"""Float64 restatement of the symmetry-corrected ligand RMSD (kernel pd_sym_rmsd) in plain numpy - the yardstick of
tests/test_symmetry_cpu.py and tests/test_sym_rmsd_gpu.py.  Nothing of physdock_amd is imported here.

    cost[m] = (1/L) sum_a |p[a] - q[perms[m][a]]|^2        value = sqrt(min_m cost[m])

`dtype=np.float32` evaluates the same formula in fp32 (numpy's own summation order): the E of the tolerance rule."""
import numpy as np


def perm_costs(p, q, perms, dtype=np.float64):
    """p, q [L,3] -> cost [M] of matching atom a of p with atom perms[m][a] of q"""
    p, q = np.asarray(p, dtype=dtype), np.asarray(q, dtype=dtype)
    d = p[None, :, :] - q[np.asarray(perms, dtype=np.int64)]           # [M,L,3]
    return (d * d).sum(-1).sum(-1) / dtype(p.shape[0])


def sym_rmsd(p, q, perms, dtype=np.float64):
    return np.sqrt(perm_costs(p, q, perms, dtype).min())


def plain_rmsd(p, q, dtype=np.float64):
    return sym_rmsd(p, q, np.arange(len(p))[None], dtype)


def sym_rmsd_matrix(x, idx, ref, perms, dtype=np.float64):
    """x [n,A,3], idx [L] or None (atoms 0 .. L-1, L = perms.shape[1]), ref [A,3] or None, perms [M,L] ->
    (D [n,n], rmsd_ref [n] or None, ref_costs [n,M] or None).  D[i,j] for i < j has pose i fixed and pose j permuted and is
    mirrored (a table that is not a group is not symmetric in the two poses); the diagonal is zero."""
    x = np.asarray(x)
    perms = np.asarray(perms, dtype=np.int64)
    L = perms.shape[1]
    sel = np.arange(L) if idx is None else np.asarray(idx, dtype=np.int64)
    lig = x[:, sel].astype(dtype)
    n = lig.shape[0]
    D = np.zeros((n, n), dtype=dtype)
    for i in range(n):
        for j in range(i + 1, n):
            D[i, j] = D[j, i] = np.sqrt(perm_costs(lig[i], lig[j], perms, dtype).min())
    if ref is None:
        return D, None, None
    rl = np.asarray(ref)[sel].astype(dtype)
    costs = np.stack([perm_costs(lig[i], rl, perms, dtype) for i in range(n)])
    return D, np.sqrt(costs.min(1)), costs
