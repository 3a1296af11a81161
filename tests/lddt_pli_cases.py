"""The seeded cases of tests/test_lddt_pli_cpu.py and tests/test_lddt_pli_gpu.py: the smallest shapes at which the lDDT-PLI kernels
can still go wrong.  A case is a dict: x_gt [A,3] and x [P,A,3] (fp32, inside a +-32 A box), lig [L], rec_mask [A] and lig_mask [L]
(bool), perms [M,L] (None: no symmetry) - and, once `reference` has run, the float64 restatement's tables and counts, computed
once per session and shared (read only) by the tests."""
import functools
import math

import numpy as np

import lddt_pli_ref as ref

BOX = 32.0


def _ball(rng, n, r_lo, r_hi):
    """n points with a uniformly drawn distance in [r_lo, r_hi) from the origin"""
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(r_lo, r_hi, (n, 1))


def _assemble(rng, lig_xyz, rec_xyz, P, perms=None, n_masked_rec=0, masked_lig=(), pose_perm=None, centre=(3.0, -5.0, 8.0)):
    """scatter the ligand through a pose of len(lig_xyz) + len(rec_xyz) atoms; pose p is the ground truth plus noise of
    0.05 .. 1.5 A (so every threshold has contacts on both sides), its ligand relabelled by the table row pose_perm[p]"""
    L, R = len(lig_xyz), len(rec_xyz)
    A = L + R
    order = rng.permutation(A)
    lig, rec = order[:L], np.sort(order[L:])
    x_gt = np.zeros((A, 3))
    x_gt[lig], x_gt[rec] = lig_xyz, rec_xyz
    x_gt += np.asarray(centre)
    rec_mask = np.zeros(A, bool)
    rec_mask[rec] = True
    if n_masked_rec:                                     # the receptor atoms nearest to the ligand's centre: they would be contacts
        near = rec[np.argsort(np.linalg.norm(x_gt[rec] - x_gt[lig].mean(0), axis=1))]
        rec_mask[near[1:2 * n_masked_rec:2]] = False
    lig_mask = np.ones(L, bool)
    lig_mask[list(masked_lig)] = False
    sigma = np.geomspace(0.05, 1.5, P) if P > 1 else np.array([0.4])
    x = x_gt[None] + sigma[:, None, None] * rng.normal(size=(P, A, 3))
    if pose_perm is not None:
        for p, m in enumerate(pose_perm):                # atom perms[m][i] sits where atom i belongs: row m restores the match
            moved = x[p].copy()
            moved[lig[np.asarray(perms[m])]] = x[p][lig]
            x[p] = moved
    case = dict(x_gt=x_gt.astype(np.float32), x=x.astype(np.float32), lig=lig.astype(np.int64), rec_mask=rec_mask, lig_mask=lig_mask,
                perms=None if perms is None else np.asarray(perms, dtype=np.int64))
    assert np.abs(case["x"]).max() < BOX and np.abs(case["x_gt"]).max() < BOX
    return case


def ring_with_substituents():
    """(xyz [12,3], bonds, elements, bond orders): a six-ring (0 - 5) with one substituent each (6 - 11): 12 automorphisms"""
    ring = np.array([[1.39 * math.cos(k * math.pi / 3), 1.39 * math.sin(k * math.pi / 3), 0.0] for k in range(6)])
    xyz = np.concatenate([ring, ring * (1.39 + 1.74) / 1.39])
    bonds = [(k, (k + 1) % 6) for k in range(6)] + [(k, k + 6) for k in range(6)]
    return xyz, bonds, [6] * 6 + [17] * 6, [1.5] * 6 + [1.0] * 6


def four_cf3():
    """(xyz [20,3], bonds, elements): a chain of four different atoms, a carbon with three fluorines on each: 6^4 = 1296"""
    rng = np.random.default_rng(41)
    xyz, bonds, elements = [], [], [7, 6, 8, 16]
    for k in range(4):
        xyz.append([1.5 * k, 0.4 * (k % 2), 0.0])
    for k in range(4):
        c = len(xyz)
        xyz.append([1.5 * k, 0.4 * (k % 2) + 1.5 * (1 if k % 2 == 0 else -1), 0.9])
        elements.append(6)
        bonds.append((k, c))
        for f in range(3):
            xyz.append((np.array(xyz[c]) + 1.35 * _ball(rng, 1, 1.0, 1.0001)[0]).tolist())
            elements.append(9)
            bonds.append((c, len(xyz) - 1))
    bonds += [(0, 1), (1, 2), (2, 3)]
    return np.array(xyz), bonds, elements


def _perms(n, bonds, elements, orders=None):
    from physdock_amd.symmetry import automorphisms
    perms, complete = automorphisms(n, bonds, elements, orders)
    assert complete
    return perms.astype(np.int64)


def _pocket(rng, n, half):
    return rng.uniform(-half, half, (n, 3))


def case_empty():
    rng = np.random.default_rng(101)
    return _assemble(rng, np.zeros((1, 3)), _ball(rng, 4, 6.5, 12.0), 1)


def case_three():
    rng = np.random.default_rng(102)
    return _assemble(rng, np.zeros((1, 3)), np.concatenate([_ball(rng, 3, 2.5, 5.5), _ball(rng, 3, 6.5, 12.0)]), 1)


def case_ring():
    """P=5, A=333, L=12, 12 automorphisms, about 40 contacts per atom; poses 1 - 4 are relabelled by a row of the table"""
    rng = np.random.default_rng(103)
    xyz, bonds, el, orders = ring_with_substituents()
    perms = _perms(12, bonds, el, orders)
    assert perms.shape == (12, 12)
    return _assemble(rng, xyz, _pocket(rng, 321, 9.7), 5, perms, pose_perm=[0, 5, 11, 3, 7])


def case_cf3():
    """M = 1296: more than one stride of a 256-thread block and no multiple of 256"""
    rng = np.random.default_rng(104)
    xyz, bonds, el = four_cf3()
    perms = _perms(20, bonds, el)
    assert perms.shape == (1296, 20)
    return _assemble(rng, xyz, _pocket(rng, 180, 8.0) + [2.2, 0, 0], 2, perms, pose_perm=[1295, 517])


def case_dense():
    """one ligand atom with exactly 700 contacts: more than one tile of the counts kernel, more than two strides of its block"""
    rng = np.random.default_rng(105)
    return _assemble(rng, np.zeros((1, 3)), np.concatenate([_ball(rng, 700, 1.0, 5.9), _ball(rng, 40, 6.1, 10.0)]), 2)


def case_masked():
    """the ring with two ligand atoms masked out in the ground truth and eight receptor atoms of the pocket masked out"""
    rng = np.random.default_rng(106)
    xyz, bonds, el, orders = ring_with_substituents()
    return _assemble(rng, xyz, _pocket(rng, 150, 7.5), 3, _perms(12, bonds, el, orders), n_masked_rec=8, masked_lig=(2, 9),
                     pose_perm=[0, 4, 9])


def case_tie():
    """atoms 0, 1 (on atom 4) and atoms 2, 3 (on atom 5) are equivalent pairs: rows (id, swap 2-3, swap 0-1, both).  Pose 0 has
    atoms 0 and 1 exchanged and atoms 2 and 3 on ONE point: rows 2 and 3 tie above rows 0 and 1, row 2 must win.  Pose 1 keeps 0 and
    1 in place: rows 0 and 1 tie, row 0 must win."""
    rng = np.random.default_rng(107)
    xyz = np.array([[-1.2, 1.1, 0.0], [-1.2, -1.1, 0.0], [2.7, 1.2, 0.0], [2.7, -1.2, 0.0], [0.0, 0.0, 0.0], [1.5, 0.0, 0.0]])
    perms = _perms(6, [(4, 0), (4, 1), (5, 2), (5, 3), (4, 5)], [9, 9, 17, 17, 6, 16])
    assert perms.tolist() == [[0, 1, 2, 3, 4, 5], [0, 1, 3, 2, 4, 5], [1, 0, 2, 3, 4, 5], [1, 0, 3, 2, 4, 5]]
    case = _assemble(rng, xyz, _pocket(rng, 90, 6.5), 2, perms)
    lig, x = case["lig"], case["x"]
    x[:] = case["x_gt"][None] + (0.2 * rng.normal(size=x.shape)).astype(np.float32)
    x[0, lig[[0, 1]]] = x[0, lig[[1, 0]]]
    x[:, lig[2]] = x[:, lig[3]] = 0.5 * (case["x_gt"][lig[2]] + case["x_gt"][lig[3]])
    return case


def case_wide():
    """L * L candidates, more than the selection kernel keeps in LDS (the bound is the package's constant): the table holds every
    cyclic shift of L atoms"""
    from physdock_amd.lddt_pli import LDS_CANDIDATES as lds_candidates
    rng = np.random.default_rng(108)
    L = math.isqrt(int(lds_candidates)) + 1
    perms = (np.arange(L)[None, :] + np.arange(L)[:, None]) % L
    case = _assemble(rng, _pocket(rng, L, 3.0), _pocket(rng, 160, 7.5), 2, perms, pose_perm=[7, L - 1])
    assert L * L > lds_candidates
    return case


CASES = {"empty": case_empty, "three": case_three, "ring": case_ring, "cf3": case_cf3, "dense": case_dense, "masked": case_masked,
         "tie": case_tie, "wide": case_wide}


def rigid_copy(x, seed=9):
    """every pose of x [P,A,3] rotated about its centroid by its own random rotation and shifted by up to 3 A (float64, then fp32)"""
    rng = np.random.default_rng(seed)
    out = np.empty_like(x)
    for p in range(len(x)):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        q *= np.sign(np.linalg.det(q))
        c = x[p].astype(np.float64).mean(0)
        out[p] = ((x[p].astype(np.float64) - c) @ q.T + c + rng.uniform(-3, 3, 3)).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the case with the restatement's view of it: perms (the identity when the case has none), start / atom / dist (contact
    table), cand_start / cand_atom / slot, and c / lo / hi [P,n_cand,4] in candidate order"""
    case = dict(CASES[name]())
    L = len(case["lig"])
    perms = np.arange(L)[None] if case["perms"] is None else case["perms"]
    start, atom, dist = ref.contacts(case["x_gt"], case["lig"], case["rec_mask"], lig_mask=case["lig_mask"])
    pairs = ref.pair_counts(case["x"], case["lig"], start, atom, dist)
    cand_start, cand_atom, slot = ref.candidates(perms)
    case.update(table_perms=perms, start=start, atom=atom, dist=dist, cand_start=cand_start, cand_atom=cand_atom, slot=slot,
                **{k: ref.by_candidate(v, perms) for k, v in pairs.items()})
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def uncertain_share(r, lo=None, hi=None):
    """sum(hi - lo) over 4 * (the number of (pose, candidate, contact) triples): the share of compares DELTA leaves open"""
    lo, hi = r["lo"] if lo is None else lo, r["hi"] if hi is None else hi
    per_cand = np.repeat(np.diff(r["start"]), np.diff(r["cand_start"]))
    n = 4 * r["x"].shape[0] * int(per_cand.sum())
    return (float((hi - lo).sum()) / n if n else 0.0), n
