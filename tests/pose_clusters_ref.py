"""NumPy restatement of PoseClusters (physdock_amd/clustering.py, csrc/cluster.hip): greedy leader clustering of n poses on a distance
matrix, best pose first - the way Vina, AutoDock, GNINA and rDock report binding modes.  Nothing here imports the package.  This file
is the written definition: the kernel follows it.

Inputs.  D fp32 [n,n], symmetric, zero diagonal (an RMSD matrix, or 1 - Tanimoto); order int32 [n], pose ids best first, a
permutation of 0 .. n-1; cutoff fp32, finite, not negative; valid uint8 [n] (optional, all valid without it); score fp32 [n]
(optional).

Assignment.  labels[:] = -1, k = 0.  For r = 0 .. n-1 take i = order[r]; an i outside 0 .. n-1, an invalid i and a labelled i are
skipped.  Otherwise i leads cluster k: i itself and every valid, still unlabelled j with D[i,j] <= cutoff get label k - the comparison
in fp32, inclusive, false for a NaN - and k += 1.  So invalid poses keep -1 and count nowhere, cluster 0 holds the best-ranked valid
pose, leaders are pairwise further apart than the cutoff and every member lies within it of its leader.

Per cluster k < n_clusters (arrays of length n; behind n_clusters ids are -1, sizes 0, floats NaN):
    leader       the leading pose                      size     the number of members
    radius       the largest D[leader, member]: an exact fp32 maximum
    medoid       the member i with the smallest s_i, s_i = the sum of (double)D[i,j] over the OTHER members j in ascending j, IEEE fp64;
                 a NaN s_i counts as +inf; ties go to the smallest pose id
    spread       (float)((sum of s_i over the members in ascending i, fp64) / (double)(size (size - 1))); 0 for a singleton
    mean_score   (float)((sum of (double)score[i] over the members in ascending i) / (double)size); NaN without score
Per pose: labels int32 [n]; dist_to_leader fp32 [n] = D[leader of i, i], NaN for label -1.  n_clusters int32 [1].

Every float is a maximum, a copy, or an fp64 sum in a stated order followed by one division and one rounding to fp32: the device is
expected to give the same BITS.
"""
import numpy as np

INT_KEYS = ("labels", "leader", "size", "medoid", "n_clusters")
FLOAT_KEYS = ("dist_to_leader", "radius", "spread", "mean_score")
KEYS = INT_KEYS + FLOAT_KEYS


def restate(D, order, cutoff, valid=None, score=None):
    D = np.asarray(D)
    assert D.dtype == np.float32 and D.ndim == 2 and D.shape[0] == D.shape[1]
    n = D.shape[0]
    order = np.asarray(order)
    cutoff = np.float32(cutoff)
    ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid).astype(bool)
    labels = np.full(n, -1, dtype=np.int32)
    dist = np.full(n, np.nan, dtype=np.float32)
    leader, size, medoid = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    radius, spread, mean_score = (np.full(n, np.nan, dtype=np.float32) for _ in range(3))
    k = 0
    for r in range(n):
        i = int(order[r])
        if not 0 <= i < n or not ok[i] or labels[i] >= 0:
            continue
        with np.errstate(invalid="ignore"):
            join = ok & (labels < 0) & (D[i] <= cutoff)                 # fp32, inclusive, a NaN never joins
        join[i] = True
        labels[join] = k
        dist[join] = D[i, join]
        leader[k], size[k], radius[k] = i, int(join.sum()), np.max(D[i, join])
        k += 1
    # s_i: one running fp64 sum per pose over the other members of its cluster, the columns taken in ascending j
    s = np.zeros(n, dtype=np.float64)
    Dd = D.astype(np.float64)
    for j in range(n):
        if labels[j] < 0:
            continue
        rows = labels == labels[j]
        rows[j] = False
        s[rows] = s[rows] + Dd[rows, j]
    for c in range(k):
        members = np.nonzero(labels == c)[0]                            # ascending pose id
        key = np.where(np.isnan(s[members]), np.inf, s[members])
        medoid[c] = members[int(np.argmin(key))]                        # argmin returns the first (smallest id) of equal keys
        total, sc = np.float64(0.0), np.float64(0.0)
        for i in members:
            total = total + s[i]
            if score is not None:
                sc = sc + np.float64(np.float32(score[i]))
        m = len(members)
        spread[c] = np.float32(total / np.float64(m * (m - 1))) if m > 1 else np.float32(0.0)
        if score is not None:
            mean_score[c] = np.float32(sc / np.float64(m))
    return dict(labels=labels, dist_to_leader=dist, leader=leader, size=size, radius=radius, medoid=medoid, spread=spread,
                mean_score=mean_score, n_clusters=np.array([k], dtype=np.int32))


def same_bits(a, b):
    """two fp32 arrays hold the same values bit for bit, a NaN matching any NaN"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in INT_KEYS) and all(same_bits(a[k], b[k]) for k in FLOAT_KEYS)


def check_invariants(D, order, cutoff, res, valid=None):
    """what the definition promises, asserted on a result (of the restatement or of the device)"""
    n = D.shape[0]
    ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid).astype(bool)
    K = int(res["n_clusters"][0])
    labels, leader = res["labels"], res["leader"]
    assert ((labels >= 0) == ok).all() and (labels < K).all()
    assert (leader[:K] >= 0).all() and (leader[K:] == -1).all() and (res["size"][K:] == 0).all() and (res["medoid"][K:] == -1).all()
    assert all(np.isnan(res[f][K:]).all() for f in ("radius", "spread", "mean_score"))
    assert np.isnan(res["dist_to_leader"][~ok]).all()
    rank = {int(p): r for r, p in enumerate(order)}
    lead = leader[:K]
    assert len(set(lead.tolist())) == K and all(int(p) in rank for p in lead), "leaders appear in order"
    assert [rank[int(p)] for p in lead] == sorted(rank[int(p)] for p in lead), "clusters are numbered in the order of their leaders"
    if K:
        first_valid = next(int(p) for p in order if ok[int(p)])
        assert lead[0] == first_valid, "cluster 0 holds the best-ranked valid pose"
    for a in range(K):
        for b in range(a + 1, K):
            assert not D[lead[a], lead[b]] <= np.float32(cutoff), "leaders are pairwise beyond the cutoff"
    for i in np.nonzero(ok)[0]:
        c = labels[i]
        assert labels[lead[c]] == c
        assert i == lead[c] or D[lead[c], i] <= np.float32(cutoff), "a member lies within the cutoff of its leader"
        assert same_bits(res["dist_to_leader"][i], D[lead[c], i])
    for c in range(K):
        members = np.nonzero(labels == c)[0]
        assert res["size"][c] == len(members) and labels[res["medoid"][c]] == c
        assert same_bits(res["radius"][c], np.max(D[lead[c], members]))
    assert int(res["size"].sum()) == int(ok.sum())


# ------------------------------------------------------------------ seeded cases
def symmetric(M):
    M = np.triu(M, 1)
    return np.ascontiguousarray((M + M.T).astype(np.float32))


def random_matrix(n, seed, lo=0.25, hi=6.0):
    """positive off-diagonal distances without structure"""
    rng = np.random.default_rng(seed)
    return symmetric(rng.uniform(lo, hi, size=(n, n)))


def planted(n, modes, seed, spread=0.3, sep=8.0):
    """points of `modes` well separated groups on a line with jitter in three dimensions, the groups interleaved in pose id (pose i
    belongs to group i % modes); D = their fp32 distances, symmetric by construction"""
    rng = np.random.default_rng(seed)
    centre = np.zeros((n, 3))
    centre[:, 0] = sep * (np.arange(n) % modes)
    x = centre + rng.uniform(-spread, spread, size=(n, 3))
    d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    return symmetric(d)


def permutation(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.int32)


#: the hand-worked case.  cutoff 2.0, order 3, 0, 1, 2, 4:  pose 3 leads cluster 0 and takes 1 (2.0, inclusive) and 4 (1.5), not 0
#: (2.5) nor 2 (3.0); pose 0 leads cluster 1 and takes 2 (1.0).  Cluster 0 = {1, 3, 4}: s_1 = 2.0 + 0.5 = 2.5, s_3 = 2.0 + 1.5 = 3.5,
#: s_4 = 0.5 + 1.5 = 2.0 -> medoid 4, spread = 8.0 / 6; radius 2.0.  Cluster 1 = {0, 2}: s_0 = s_2 = 1.0 -> medoid 0 (the tie goes to
#: the smaller id), spread = 2.0 / 2 = 1.0; radius 1.0.
HAND_D = np.array([[0.0, 4.0, 1.0, 2.5, 5.0],
                   [4.0, 0.0, 4.5, 2.0, 0.5],
                   [1.0, 4.5, 0.0, 3.0, 6.0],
                   [2.5, 2.0, 3.0, 0.0, 1.5],
                   [5.0, 0.5, 6.0, 1.5, 0.0]], dtype=np.float32)
HAND_ORDER = np.array([3, 0, 1, 2, 4], dtype=np.int32)
HAND_CUTOFF = 2.0
HAND_SCORE = np.array([-7.0, -6.5, -7.0, -9.0, -8.25], dtype=np.float32)
HAND = dict(labels=[1, 0, 1, 0, 0], leader=[3, 0, -1, -1, -1], size=[3, 2, 0, 0, 0], medoid=[4, 0, -1, -1, -1], n_clusters=[2],
            dist_to_leader=[0.0, 2.0, 1.0, 0.0, 1.5], radius=[2.0, 1.0], spread=[np.float32(8.0 / 6.0), 1.0],
            mean_score=[np.float32(-23.75 / 3.0), -7.0])


def hand_case():
    return dict(D=HAND_D.copy(), order=HAND_ORDER.copy(), cutoff=HAND_CUTOFF, valid=None, score=HAND_SCORE.copy())


def make_case(name):
    """dict(D, order, cutoff, valid, score) of a named case; BLOCK = 1024 threads walk a row, so 1030 takes two sweeps with a tail"""
    if name == "n1":
        return dict(D=np.zeros((1, 1), np.float32), order=np.zeros(1, np.int32), cutoff=2.0, valid=None, score=np.array([-3.5], np.float32))
    if name == "n5_hand":
        return hand_case()
    if name in ("n70_random", "n257_random", "n1030_random"):
        n = int(name[1:].split("_")[0])
        rng = np.random.default_rng(n)
        return dict(D=random_matrix(n, seed=n), order=permutation(n, n + 1), cutoff=1.0, valid=None,
                    score=rng.normal(-7, 1, n).astype(np.float32))
    if name in ("n70_planted", "n257_planted", "n1030_planted"):
        n = int(name[1:].split("_")[0])
        rng = np.random.default_rng(n + 7)
        return dict(D=planted(n, modes=7, seed=n), order=permutation(n, n + 2), cutoff=2.0, valid=None,
                    score=rng.normal(-7, 1, n).astype(np.float32))
    if name == "n257_one_cluster":
        return dict(D=random_matrix(257, seed=11), order=permutation(257, 12), cutoff=1.0e30, valid=None, score=None)
    if name == "n1030_singletons":                                      # K = n: the longest chain of leaders
        return dict(D=random_matrix(1030, seed=13), order=permutation(1030, 14), cutoff=0.0, valid=None, score=None)
    if name == "n70_at_cutoff":                                         # every entry is 2.0 or 2.5: the inclusive comparison decides
        rng = np.random.default_rng(15)
        return dict(D=symmetric(np.where(rng.random((70, 70)) < 0.3, 2.0, 2.5)), order=permutation(70, 16), cutoff=2.0, valid=None, score=None)
    if name == "n70_nan_pair":                                          # poses 3 and 5 of one planted group, their distance unknown
        D = planted(70, modes=2, seed=17)
        D[3, 5] = D[5, 3] = np.nan
        return dict(D=D, order=np.arange(70, dtype=np.int32), cutoff=2.0, valid=None, score=None)
    if name == "n70_nan_leader":                                        # the NaN sits in a leader's row: pose 2 does not join pose 0
        D = planted(70, modes=2, seed=18)
        D[0, 2] = D[2, 0] = np.nan
        return dict(D=D, order=np.arange(70, dtype=np.int32), cutoff=2.0, valid=None, score=None)
    if name == "n70_best_invalid":
        order = permutation(70, 19)
        valid = (np.random.default_rng(20).random(70) < 0.7).astype(np.uint8)
        valid[order[0]] = 0
        valid[order[1]] = 1
        return dict(D=planted(70, modes=3, seed=21), order=order, cutoff=2.0, valid=valid, score=None)
    if name == "n70_all_invalid":
        return dict(D=planted(70, modes=3, seed=22), order=permutation(70, 23), cutoff=2.0, valid=np.zeros(70, np.uint8), score=None)
    if name == "n257_score_ties":                                       # scores from a set of four values
        rng = np.random.default_rng(24)
        return dict(D=planted(257, modes=5, seed=25), order=permutation(257, 26), cutoff=2.0, valid=None,
                    score=rng.choice(np.array([-8.0, -7.5, -7.5, -6.25], np.float32), 257))
    raise KeyError(name)


CASES = ("n1", "n5_hand", "n70_random", "n70_planted", "n257_random", "n257_planted", "n1030_random", "n1030_planted",
         "n257_one_cluster", "n1030_singletons", "n70_at_cutoff", "n70_nan_pair", "n70_nan_leader", "n70_best_invalid",
         "n70_all_invalid", "n257_score_ties")
