"""Float64 restatement of the symmetry-aware lDDT-PLI (kernels pd_lddt_pli_counts / pd_lddt_pli_select) in plain numpy - the
yardstick of tests/test_lddt_pli_cpu.py and tests/test_lddt_pli_gpu.py.  Nothing of physdock_amd is imported here.

    N(i)      = { receptor atoms j : |x_gt[lig[i]] - x_gt[j]| < radius },  d_gt(i,j) stored as fp32     (`contacts`)
    c_t(i,k)  = #{ j in N(i) : | |x[lig[k]] - x[j]| - d_gt(i,j) | < t }                                  (`pair_counts`)
    C_t(m)    = sum_i c_t(i, perms[m][i]);   m* = the smallest m that maximises sum_t C_t(m)            (`select`)
    lddt_pli  = sum_t C_t(m*) / (4 sum_i |N(i)|),   0 without contacts

Brute force: `pair_counts` holds every pair (i, k), `select` walks all permutations.  A threshold compare cannot be bit-matched
between fp32 and float64, so `pair_counts` also returns `lo` (counted with t - delta) and `hi` (t + delta): a device count is
right when lo <= count <= hi.  DELTA = 1e-4 A: coordinates stay inside a +-32 A box, only distances below about 10 A can lie
within reach of a threshold, the fp32 error of such a distance computed from the same fp32 inputs is below 5e-6 A, two of them
(the pose's distance and the stored d_gt) give 1e-5 A, and DELTA is ten times that."""
import numpy as np

RADIUS = 6.0
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
DELTA = 1e-4


def contacts(x_gt, lig, rec_mask, radius=RADIUS, lig_mask=None):
    """the contact table by a naive double loop -> (start int64 [L+1], atom int64 [n], dist fp32 [n]); rec_mask [A] bool
    (ligand atoms are left out whatever it says); lig_mask [L] bool (False: the ligand atom has no contacts)"""
    x = np.asarray(x_gt, dtype=np.float64)
    lig = [int(a) for a in lig]
    start, atom, dist = [0], [], []
    for i, a in enumerate(lig):
        if lig_mask is None or lig_mask[i]:
            for j in range(len(x)):
                if rec_mask[j] and j not in lig:
                    d = float(np.sqrt(((x[a] - x[j]) ** 2).sum()))
                    if d < radius:
                        atom.append(j); dist.append(d)
        start.append(len(atom))
    return np.asarray(start, np.int64), np.asarray(atom, np.int64), np.asarray(dist, np.float64).astype(np.float32)


def pair_counts(x, lig, start, atom, dist, thresholds=THRESHOLDS, delta=DELTA):
    """x [P,A,3]; the contact table (dist as the fp32 table the device gets) -> dict of int64 [P,L,L,4]: `c` = c_t(i,k) for every
    ligand atom i and every candidate k, `lo` / `hi` the same counted with t - delta / t + delta"""
    x = np.asarray(x, dtype=np.float64)
    lig = np.asarray(lig, dtype=np.int64)
    P, L = x.shape[0], len(lig)
    out = {k: np.zeros((P, L, L, 4), np.int64) for k in ("c", "lo", "hi")}
    xl = x[:, lig]                                                              # [P,L,3]
    for i in range(L):
        j = np.asarray(atom[start[i]:start[i + 1]], dtype=np.int64)
        if not len(j):
            continue
        d = np.sqrt(((xl[:, :, None, :] - x[:, None, j, :]) ** 2).sum(-1))      # [P,k,contacts]
        diff = np.abs(d - np.asarray(dist[start[i]:start[i + 1]], dtype=np.float64)[None, None, :])
        for t, thr in enumerate(thresholds):
            out["c"][:, i, :, t] = (diff < thr).sum(-1)
            out["lo"][:, i, :, t] = (diff < thr - delta).sum(-1)
            out["hi"][:, i, :, t] = (diff < thr + delta).sum(-1)
    return out


def candidates(perms):
    """perms [M,L] -> (cand_start [L+1], cand_atom, slot [L,M]): the distinct images of every atom in ascending order, and the
    position of perms[m][i] among the images of i"""
    perms = np.asarray(perms, dtype=np.int64)
    M, L = perms.shape
    start, atom, slot = [0], [], np.zeros((L, M), np.int64)
    for i in range(L):
        images = sorted(set(perms[:, i].tolist()))
        for m in range(M):
            slot[i, m] = images.index(int(perms[m, i]))
        atom += images
        start.append(len(atom))
    return np.asarray(start, np.int64), np.asarray(atom, np.int64), slot


def by_candidate(pairs, perms):
    """[P,L,L,4] over (i, k) -> [P,n_cand,4] in the candidate order of `candidates`"""
    start, atom, _ = candidates(perms)
    i_of = np.repeat(np.arange(len(start) - 1), np.diff(start))
    return pairs[:, i_of, atom, :]


def select(counts, perms, atom_contacts):
    """counts [P,n_cand,4] (candidate order) -> dict: totals int64 [P,M] (sum_t C_t(m)), best_perm [P] (the smallest maximiser),
    conserved int64 [P,4], per_atom fp32 [P,L], lddt_pli fp32 [P] - the divisions as ONE fp32 division of the two integers"""
    counts = np.asarray(counts, dtype=np.int64)
    perms = np.asarray(perms, dtype=np.int64)
    start, _, slot = candidates(perms)
    n_i = np.asarray(atom_contacts, dtype=np.int64)
    M, L = perms.shape
    P = counts.shape[0]
    picked = counts[:, (start[:-1, None] + slot).T, :]                           # [P,M,L,4]
    totals = picked.sum((-1, -2))
    best = totals.argmax(1)                                                      # numpy's argmax names the first maximum
    chosen = picked[np.arange(P), best]                                          # [P,L,4]
    conserved = chosen.sum(1)
    per_atom = np.zeros((P, L), np.float32)
    has = n_i > 0
    per_atom[:, has] = chosen.sum(-1)[:, has].astype(np.float32) / (4 * n_i[has]).astype(np.float32)[None]
    n = int(n_i.sum())
    lddt = conserved.sum(-1).astype(np.float32) / np.float32(4 * n) if n else np.zeros(P, np.float32)
    return {"totals": totals, "best_perm": best, "conserved": conserved, "per_atom": per_atom, "lddt_pli": lddt.astype(np.float32)}


def lddt_pli(x, x_gt, lig, rec_mask, perms=None, radius=RADIUS, thresholds=THRESHOLDS, lig_mask=None):
    """the whole definition in one call (float64 compares, delta = 0) -> the dict of `select` plus n_contacts and pairs"""
    perms = np.arange(len(lig))[None] if perms is None else np.asarray(perms)
    start, atom, dist = contacts(x_gt, lig, rec_mask, radius, lig_mask)
    pairs = pair_counts(x, lig, start, atom, dist, thresholds, 0.0)
    out = select(by_candidate(pairs["c"], perms), perms, np.diff(start))
    out.update(n_contacts=int(start[-1]), pairs=pairs["c"])
    return out
