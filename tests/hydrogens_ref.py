"""Float64 restatement of pd_place_hydrogens and pd_hydrogen_bonds (csrc/hydrogens.hip) and the seeded cases the GPU tests run.
Nothing here imports the package: the definition is written down a second time, in plain numpy.  This file is the written definition;
the header comment of csrc/hydrogens.hip and the docstring of physdock_amd/hydrogens.py repeat it.

One system: A atoms, poses x [P,A,3] in fp32; `lig_idx [L]`, `lig_active [L]`, `rec_mask [A]`, `residue_of [A]` / `n_residues` R as
InteractionFingerprint takes them; `types [A]`, the type bytes of VinaScore (bit 6 ACCEPTOR; bits 0 - 3 the radius class: 1 N, 2 O,
4 S).  Hydrogen table `table`, H rows: parent, ref [3] (-1 unused), mode, length (fp32, A), a, b (fp32, radians), group (rotor id or
-1); side = 1 where the parent is a ligand atom.

Placement, float64 on the fp32 values, rounded once to fp32.  p = the parent, u_i = unit(n_i - p), unit(v) = v / |v|:
    TRI     H = p + length unit(-(u1 + u2 + u3))
    BISECT  bis = unit(-(u1 + u2)), w = unit(u1 x u2);  H = p + length (cos a bis + sin a w)
    NERF    bc = unit(p - n1), n = unit((n1 - n2) x bc), m = n x bc;  H = p + length (-cos a bc + sin a (cos b m + sin b n))
    LINEAR  H = p + length unit(p - n1)
Not placed (x_h NaN, placed 0, part of nothing): a vector about to be normalised is shorter than TINY = 1e-6, a coordinate read is
not finite, a ref the mode needs is -1.

Rotor groups (orient): the rows of one group (1 row: 12 candidates, 3 rows: 4) share parent, n1, n2 and are NERF.  Candidate k adds
k * 30 deg to every b.  Acceptors of a group: the acceptor-typed heavy atoms A of the other molecule, finite, with |A - p| <= d_da.
score(k) = the smallest |A - H| over the group's hydrogens (float64, not rounded) and those acceptors; the smallest score wins, a tie
goes to the smaller k, no acceptor gives 0.  A group with a row that is not placed keeps its default angles and reports 0.

Hydrogen bond: h placed, its parent D of class N, O or S; A an acceptor of the other molecule (receptor: rec_mask and ACCEPTOR;
ligand: lig_active and ACCEPTOR); |D - A| <= d_da; (D - H) . (A - H) <= cos(angle_min) |D - H| |A - H|, on the fp32 x_h as stored.
    bits[p][s]         bit 0: a ligand hydrogen bonds to an acceptor of residue s; bit 1: a hydrogen of residue s bonds to a ligand acceptor
    ligand_bits[p][i]  bit 0: a hydrogen on ligand atom i donates; bit 1: ligand atom i accepts
    h_bits[p][h]       1 for a ligand hydrogen that bonds, 2 for a receptor hydrogen that bonds
    counts[p]          the (hydrogen, acceptor) pairs of the two kinds
"""
import functools

import numpy as np

HBOND_KIND_NAMES = ("hbond_donor", "hbond_acceptor")
THRESHOLD_NAMES = ("d_da", "angle_min")
THRESHOLDS = (4.1, 100.0)
LENGTHS = {6: 1.09, 7: 1.01, 8: 0.96, 16: 1.34}
TRI, BISECT, NERF, LINEAR = 0, 1, 2, 3
ACCEPTOR = 64
CLASS_C, CLASS_N, CLASS_O, CLASS_S = 0, 1, 2, 4
POLAR_CLASSES = (CLASS_N, CLASS_O, CLASS_S)
TINY = 1.0e-6
STEP = np.pi / 6.0
TETRAHEDRAL = float(np.arccos(-1.0 / 3.0))
HALF_TETRAHEDRAL = TETRAHEDRAL / 2.0
HYDROXYL, TRIGONAL = float(np.deg2rad(109.5)), float(np.deg2rad(120.0))
#: the launch geometry of csrc/hydrogens.hip that case c crosses: rows per block of hydrogens_place_kernel, lanes that stride the
#: acceptors in hydrogens_rotor_kernel and hydrogens_hbond_kernel, and the stride of hydrogens_fold_kernel over residues, ligand atoms
#: and rows
PLACE_BLOCK, ROTOR_BLOCK, HBOND_BLOCK, FOLD_BLOCK = 128, 64, 64, 64

CASES = ("a_hand_P2", "b_seeded_P3", "c_blocks_P2")
#: case a: what the hand-placed acceptors were built for
A_OH_CHOICE, A_NH3_CHOICE = (9, 2), (1, 3)
#: case b: the poisoned pose
B_NAN_POSE = 1


# ------------------------------------------------------------------ placement
def _norm(v):
    return float(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))


def _unit(v):
    """(v / |v|, |v| >= TINY)"""
    n = _norm(v)
    with np.errstate(all="ignore"):
        return v / n, bool(n >= TINY)


def _atom(xp, i):
    """(float64 position, usable) of atom i of a pose; -1 and non-finite coordinates are not usable"""
    if i < 0:
        return None, False
    v = xp[i].astype(np.float64)
    return v, bool(np.isfinite(v).all())


def place_row(xp, parent, ref, mode, length, a, b):
    """one hydrogen in float64, or None when it is not placed; length, a, b: float64 values of the fp32 table entries"""
    p, ok = _atom(xp, parent)
    n1, ok1 = _atom(xp, ref[0])
    if not (ok and ok1):
        return None
    if mode == LINEAR:
        d, good = _unit(p - n1)
    elif mode == NERF:
        n2, ok2 = _atom(xp, ref[1])
        if not ok2:
            return None
        bc, g1 = _unit(p - n1)
        n, g2 = _unit(np.cross(n1 - n2, bc))
        m = np.cross(n, bc)
        d, good = -np.cos(a) * bc + np.sin(a) * (np.cos(b) * m + np.sin(b) * n), g1 and g2
    elif mode == BISECT:
        n2, ok2 = _atom(xp, ref[1])
        if not ok2:
            return None
        (u1, g1), (u2, g2) = _unit(n1 - p), _unit(n2 - p)
        (bis, g3), (w, g4) = _unit(-(u1 + u2)), _unit(np.cross(u1, u2))
        d, good = np.cos(a) * bis + np.sin(a) * w, g1 and g2 and g3 and g4
    elif mode == TRI:
        (n2, ok2), (n3, ok3) = _atom(xp, ref[1]), _atom(xp, ref[2])
        if not (ok2 and ok3):
            return None
        (u1, g1), (u2, g2), (u3, g3) = _unit(n1 - p), _unit(n2 - p), _unit(n3 - p)
        d, g4 = _unit(-(u1 + u2 + u3))
        good = g1 and g2 and g3 and g4
    else:
        return None
    return p + length * d if good else None


def sides(c):
    """uint8 [H]: 1 where the parent is a ligand atom"""
    return np.isin(c["table"]["parent"], c["lig_idx"]).astype(np.uint8)


def acceptors(c):
    """(receptor acceptors sorted by residue, ligand acceptors as pose atoms, ligand acceptors as local indices)"""
    order = np.argsort(c["residue_of"], kind="stable")
    rec = order[(c["rec_mask"][order] > 0) & ((c["types"][order] & ACCEPTOR) > 0)]
    local = np.nonzero((c["lig_active"] > 0) & ((c["types"][c["lig_idx"]] & ACCEPTOR) > 0))[0]
    return rec.astype(np.int32), c["lig_idx"][local].astype(np.int32), local


def groups(c):
    """int32 [G,3]: the rows of every rotor group (ids dense, in the order of first appearance), -1 behind a single row"""
    g = c["table"]["group"]
    ids = []
    for v in g[g >= 0].tolist():
        if v not in ids:
            ids.append(v)
    out = np.full((len(ids), 3), -1, dtype=np.int32)
    for k, v in enumerate(ids):
        rows = np.nonzero(g == v)[0]
        out[k, :len(rows)] = rows
    return out


def place(c, orient=True):
    """-> dict: x_h fp32 [P,H,3] (NaN: not placed), x_h64 (before the rounding), placed uint8 [P,H], rotor_choice int32 [P,G],
    rotor_scores float64 [P,G,12] (inf: no acceptor, or behind the group's candidates) and rotor_margin float64 [P,G]: the
    second-smallest minus the smallest score (inf when no acceptor is in range)"""
    t, x = c["table"], c["x"]
    P, H = x.shape[0], len(t["parent"])
    f64 = lambda k: t[k].astype(np.float64)
    length, a, b = f64("length"), f64("a"), f64("b")
    grp, side = groups(c), sides(c)
    rec_acc, lig_acc, _ = acceptors(c)
    d_da = float(c["thresholds"][0])
    x64 = np.full((P, H, 3), np.nan)
    placed = np.zeros((P, H), dtype=np.uint8)
    choice = np.zeros((P, len(grp)), dtype=np.int32)
    scores = np.full((P, len(grp), 12), np.inf)
    for p in range(P):
        xp = x[p]
        for h in range(H):
            pos = place_row(xp, int(t["parent"][h]), t["ref"][h], int(t["mode"][h]), length[h], a[h], b[h])
            if pos is not None:
                x64[p, h], placed[p, h] = pos, 1
        if not orient:
            continue
        for g, rows in enumerate(grp):
            rows = rows[rows >= 0]
            if not placed[p, rows].all():
                continue
            par = xp[t["parent"][rows[0]]].astype(np.float64)
            acc = xp[rec_acc if side[rows[0]] else lig_acc].astype(np.float64)
            acc = acc[np.isfinite(acc).all(1)]
            acc = acc[np.sqrt(((acc - par) ** 2).sum(1)) <= d_da] if len(acc) else acc
            n_cand = 12 // len(rows)
            cand = np.zeros((n_cand, len(rows), 3))
            for k in range(n_cand):
                for i, h in enumerate(rows):
                    cand[k, i] = place_row(xp, int(t["parent"][h]), t["ref"][h], NERF, length[h], a[h], b[h] + k * STEP)
                if len(acc):
                    scores[p, g, k] = np.sqrt(((acc[None, :, :] - cand[k][:, None, :]) ** 2).sum(-1).min())
            k = int(np.argmin(scores[p, g, :n_cand]))                 # the first of equal minima: the smallest k
            choice[p, g] = k
            x64[p, rows] = cand[k]
    srt = np.sort(scores, axis=-1)
    with np.errstate(invalid="ignore"):
        margin = np.where(np.isfinite(srt[..., 0]), srt[..., 1] - srt[..., 0], np.inf)
    return {"x_h": x64.astype(np.float32), "x_h64": x64, "placed": placed, "rotor_choice": choice, "rotor_scores": scores,
            "rotor_margin": margin}


# ------------------------------------------------------------------ hydrogen bonds
def polar_rows(c):
    """(the ligand's rows on N, O or S; the receptor's, sorted by the residue of the parent)"""
    t, side = c["table"], sides(c)
    is_polar = np.isin(c["types"][t["parent"]] & 15, POLAR_CLASSES)
    lig = np.nonzero(is_polar & (side == 1))[0]
    rec = np.nonzero(is_polar & (side == 0))[0]
    return lig.astype(np.int32), rec[np.argsort(c["residue_of"][t["parent"][rec]], kind="stable")].astype(np.int32)


def hbonds(c, x_h, placed):
    """the bonds of the hydrogens x_h fp32 [P,H,3] / placed [P,H] (the restatement's or the device's own) -> dict: bits uint8 [P,R],
    ligand_bits uint8 [P,L], h_bits uint8 [P,H], counts int32 [P,2] and margin: the smallest relative distance of any tested
    condition from its threshold (|r - d_da| / d_da; |dot - cos |D - H| |A - H|| / (|D - H| |A - H|))"""
    t, x = c["table"], c["x"]
    P, H, R, L = x.shape[0], len(t["parent"]), int(c["n_residues"]), len(c["lig_idx"])
    d_da, cos_min = float(c["thresholds"][0]), float(np.cos(np.deg2rad(c["thresholds"][1])))
    rec_acc, lig_acc, lig_acc_local = acceptors(c)
    lig_rows, rec_rows = polar_rows(c)
    local = {int(a): i for i, a in enumerate(c["lig_idx"])}
    bits, ligand_bits = np.zeros((P, R), dtype=np.uint8), np.zeros((P, L), dtype=np.uint8)
    h_bits, counts = np.zeros((P, H), dtype=np.uint8), np.zeros((P, 2), dtype=np.int32)
    margin = np.inf
    for p in range(P):
        xp = x[p].astype(np.float64)
        for kind, rows, acc in ((0, lig_rows, rec_acc), (1, rec_rows, lig_acc)):
            for h in rows:
                D, Hp = xp[t["parent"][h]], x_h[p, h].astype(np.float64)
                if not placed[p, h] or not np.isfinite(D).all() or not np.isfinite(Hp).all() or not len(acc):
                    continue
                Ap = xp[acc]
                fin = np.isfinite(Ap).all(1)
                with np.errstate(invalid="ignore"):
                    r = np.sqrt(((D - Ap) ** 2).sum(1))
                    dh, ah = D - Hp, Ap - Hp
                    ndh, nah = np.sqrt((dh * dh).sum()), np.sqrt((ah * ah).sum(1))
                    dots = ah @ dh
                    hit = fin & (r <= d_da) & (dots <= cos_min * ndh * nah)
                    rel = np.concatenate([np.abs(r[fin] - d_da) / d_da, (np.abs(dots - cos_min * ndh * nah) / (ndh * nah))[fin & (nah > 0)]])
                if len(rel):
                    margin = min(margin, float(rel.min()))
                if not hit.any():
                    continue
                counts[p, kind] += int(hit.sum())
                h_bits[p, h] = 1 << kind
                if kind == 0:
                    ligand_bits[p, local[int(t["parent"][h])]] |= 1
                    bits[p, c["residue_of"][acc[hit]]] |= 1
                else:
                    bits[p, c["residue_of"][t["parent"][h]]] |= 2
                    ligand_bits[p, lig_acc_local[hit]] |= 2
    return {"bits": bits, "ligand_bits": ligand_bits, "h_bits": h_bits, "counts": counts, "margin": margin}


def derived(c):
    """the tables the C entries take beyond the hydrogen table, restated: side, group_h, acc / NA_r / NA_l, racc_start, lig_acc_slot,
    polar / HP_l / HP_r, rh_start, polar_slot"""
    t = c["table"]
    R, L, H = int(c["n_residues"]), len(c["lig_idx"]), len(t["parent"])
    rec_acc, lig_acc, lig_acc_local = acceptors(c)
    lig_rows, rec_rows = polar_rows(c)
    csr = lambda ids: np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=R))]).astype(np.int32)
    slot = np.full(L, -1, dtype=np.int32)
    slot[lig_acc_local] = np.arange(len(lig_acc_local))
    polar = np.concatenate([lig_rows, rec_rows]).astype(np.int32)
    polar_slot = np.full(H, -1, dtype=np.int32)
    polar_slot[polar] = np.arange(len(polar))
    return {"side": sides(c), "group_h": groups(c), "acc": np.concatenate([rec_acc, lig_acc]).astype(np.int32), "NA_r": len(rec_acc),
            "NA_l": len(lig_acc), "racc_start": csr(c["residue_of"][rec_acc]), "lig_acc_slot": slot, "polar": polar, "HP_l": len(lig_rows),
            "HP_r": len(rec_rows), "rh_start": csr(c["residue_of"][t["parent"][rec_rows]]), "polar_slot": polar_slot}


# ------------------------------------------------------------------ the cases
class _Table:
    def __init__(self):
        self.rows, self.n_groups = [], 0

    def add(self, parent, refs, mode, length, a=0.0, b=0.0, group=-1):
        self.rows.append((parent, tuple((list(refs) + [-1, -1, -1])[:3]), mode, length, a, b, group))

    def new_group(self):
        self.n_groups += 1
        return self.n_groups - 1

    def table(self):
        cols = list(zip(*self.rows))
        return {"parent": np.asarray(cols[0], np.int32), "ref": np.asarray(cols[1], np.int32).reshape(-1, 3), "mode": np.asarray(cols[2], np.uint8),
                "length": np.asarray(cols[3], np.float32), "a": np.asarray(cols[4], np.float32), "b": np.asarray(cols[5], np.float32),
                "group": np.asarray(cols[6], np.int32)}


def _rotation(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _case_a():
    """Hand-placed.  Ligand atoms 0 - 8 and 14: C0 a methine on C1, C2, C3 (TRI); C1 a CH2 between C0 and C4 (BISECT, both slots); C4
    an aromatic C-H between C1 and C5 (BISECT in the plane); C2 a methyl (NERF, three slots); O6 a hydroxyl on C3 (a rotor); C7 an sp
    C-H on C5 (LINEAR); N8 a planar NH2 on C5 (NERF, cis and trans); O14 a lone acceptor.  Receptor: CD 9, CE 10, NZ 11 an NH3+ (a
    rotor of three; residue 0); O12 an acceptor with C13 (residue 1); O15 an acceptor far away (residue 2).  O12 sits 2.8 A from O6
    along the hydroxyl H at the dihedral 180 + 30 k deg, k = A_OH_CHOICE[pose]; O14 sits 2.9 A from NZ along an ammonium H at 60 +
    30 k deg, k = A_NH3_CHOICE[pose].  Pose 1 is pose 0 moved rigidly, with the two acceptors placed anew."""
    x0 = np.zeros((16, 3))
    x0[:12] = [[0.0, 0.0, 0.0], [1.25, 0.75, -0.40], [-1.30, 0.70, -0.30], [0.05, -1.20, -0.90], [2.55, 0.10, 0.05], [3.70, 0.85, 0.50],
               [0.10, -2.40, -0.20], [4.90, 0.30, 0.35], [3.75, 2.20, 0.95], [10.0, 0.0, 0.0], [10.9, 1.2, 0.2], [10.3, 2.5, 0.6]]
    x0[15] = [30.0, 30.0, 30.0]
    t = _Table()
    t.add(0, (1, 2, 3), TRI, 1.09)
    t.add(1, (0, 4), BISECT, 1.09, HALF_TETRAHEDRAL)
    t.add(1, (0, 4), BISECT, 1.09, -HALF_TETRAHEDRAL)
    t.add(4, (1, 5), BISECT, 1.09, 0.0)
    for b in (60.0, 180.0, 300.0):
        t.add(2, (0, 1), NERF, 1.09, TETRAHEDRAL, np.deg2rad(b))
    t.add(6, (3, 0), NERF, 0.96, HYDROXYL, np.pi, t.new_group())
    t.add(7, (5,), LINEAR, 1.09)
    t.add(8, (5, 4), NERF, 1.01, TRIGONAL, 0.0)
    t.add(8, (5, 4), NERF, 1.01, TRIGONAL, np.pi)
    g = t.new_group()
    for b in (60.0, 180.0, 300.0):
        t.add(11, (10, 9), NERF, 1.01, TETRAHEDRAL, np.deg2rad(b), g)
    R1 = _rotation((1.0, 2.0, -0.5), 0.9)
    poses = []
    for p in range(2):
        xp = (x0 if p == 0 else x0 @ R1.T + np.array([1.5, -2.0, 0.75])).astype(np.float32)
        for parent, refs, a, b0, k, far, acc in ((6, (3, 0), HYDROXYL, np.pi, A_OH_CHOICE[p], 2.8, 12), (11, (10, 9), TETRAHEDRAL, np.deg2rad(60.0), A_NH3_CHOICE[p], 2.9, 14)):
            xp[acc] = place_row(xp, parent, refs, NERF, far, a, b0 + k * STEP).astype(np.float32)
        xp[13] = xp[12] + np.array([1.2, 0.2, 0.1], dtype=np.float32)
        poses.append(xp)
    types = np.array([0, 0, 0, 0, 0, 0, CLASS_O | ACCEPTOR, 0, CLASS_N, 0, 0, CLASS_N, CLASS_O | ACCEPTOR, 0, CLASS_O | ACCEPTOR,
                      CLASS_O | ACCEPTOR], dtype=np.uint8)
    lig_idx = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 14], dtype=np.int32)
    rec_mask = np.ones(16, dtype=np.uint8)
    rec_mask[lig_idx] = 0
    residue_of = np.array([0] * 9 + [0, 0, 0, 1, 1, 0, 2], dtype=np.int32)
    return dict(x=np.stack(poses), lig_idx=lig_idx, lig_active=np.ones(10, dtype=np.uint8), rec_mask=rec_mask, residue_of=residue_of, n_residues=3,
                types=types, table=t.table(), thresholds=THRESHOLDS)


def _seeded(seed, n_lig, n_rec, R, P, p_acc_lig, p_acc_rec, p_parent):
    """A ligand cloud (sigma 3 A) inside a receptor cloud (sigma 6 A); every pose moves the ligand a little and jitters every atom.
    A parent's refs are its nearest atoms of the same molecule in pose 0 (n2: the atom nearest to n1 other than the parent); the modes
    cycle TRI, BISECT in the plane, BISECT both slots, methyl, hydroxyl rotor, ammonium rotor, LINEAR."""
    rng = np.random.default_rng(seed)
    A = n_lig + n_rec
    lig_idx = np.sort(rng.choice(A, n_lig, replace=False)).astype(np.int32)
    is_lig = np.zeros(A, dtype=bool)
    is_lig[lig_idx] = True
    x0 = np.where(is_lig[:, None], rng.normal(0.0, 3.0, (A, 3)), rng.normal(0.0, 6.0, (A, 3)))
    poses = []
    for p in range(P):
        xp = x0 + rng.normal(0.0, 0.1, (A, 3))
        xp[is_lig] = xp[is_lig] @ _rotation(rng.normal(size=3), 0.2 * p).T + rng.normal(0.0, 0.3, 3)
        poses.append(xp)
    x = np.stack(poses)
    residue_of = rng.integers(0, R, A).astype(np.int32)
    cls = rng.choice([CLASS_C, CLASS_C, CLASS_N, CLASS_O, CLASS_S], A).astype(np.uint8)
    lig_active, rec_mask = np.ones(n_lig, dtype=np.uint8), (~is_lig).astype(np.uint8)
    lig_active[n_lig // 2] = 0                                       # one ligand atom takes no part, one receptor atom does not exist
    rec_mask[np.nonzero(~is_lig)[0][n_rec // 2]] = 0
    usable = np.zeros(A, dtype=bool)
    usable[lig_idx[lig_active > 0]] = True
    usable |= rec_mask > 0
    t = _Table()
    turn = 0
    for parent in range(A):
        if not usable[parent] or rng.random() >= p_parent:
            continue
        same = np.nonzero((is_lig == is_lig[parent]) & usable & (np.arange(A) != parent))[0]
        near = same[np.argsort(((x0[same] - x0[parent]) ** 2).sum(1))]
        n1 = int(near[0])
        rest = same[same != n1]
        n2 = int(rest[np.argmin(((x0[rest] - x0[n1]) ** 2).sum(1))])
        kind = turn % 7
        turn += 1
        if kind == 4:
            cls[parent] = CLASS_O
        if kind == 5:
            cls[parent] = CLASS_N
        length = LENGTHS[{CLASS_C: 6, CLASS_N: 7, CLASS_O: 8, CLASS_S: 16}[int(cls[parent])]]
        if kind == 0:
            t.add(parent, near[:3].tolist(), TRI, length)
        elif kind == 1:
            t.add(parent, near[:2].tolist(), BISECT, length, 0.0)
        elif kind == 2:
            t.add(parent, near[:2].tolist(), BISECT, length, HALF_TETRAHEDRAL)
            t.add(parent, near[:2].tolist(), BISECT, length, -HALF_TETRAHEDRAL)
        elif kind == 3:
            for b in (60.0, 180.0, 300.0):
                t.add(parent, (n1, n2), NERF, length, TETRAHEDRAL, np.deg2rad(b))
        elif kind == 4:
            t.add(parent, (n1, n2), NERF, length, HYDROXYL, np.pi, t.new_group())
        elif kind == 5:
            g = t.new_group()
            for b in (60.0, 180.0, 300.0):
                t.add(parent, (n1, n2), NERF, length, TETRAHEDRAL, np.deg2rad(b), g)
        else:
            t.add(parent, (n1,), LINEAR, length)
    acc = np.where(is_lig, rng.random(A) < p_acc_lig, rng.random(A) < p_acc_rec)
    types = (cls | np.where(acc, ACCEPTOR, 0)).astype(np.uint8)
    return dict(x=x.astype(np.float32), lig_idx=lig_idx, lig_active=lig_active, rec_mask=rec_mask, residue_of=residue_of, n_residues=R,
                types=types, table=t.table(), thresholds=THRESHOLDS)


def _case_b():
    """Seeded: a 24-atom ligand and a 40-atom receptor in 6 residues, P = 3.  Pose B_NAN_POSE has a NaN coordinate on a ref atom; the
    parent of the first BISECT row lies exactly between its two refs in every pose (u1 + u2 = 0: not placed); the last receptor
    hydroxyl is moved 40 A away with its refs, so that rotor has no acceptor in range."""
    c = _seeded(11, 24, 40, 6, 3, 0.4, 0.4, 0.7)
    t, x = c["table"], c["x"]
    h = int(np.nonzero(t["mode"] == BISECT)[0][0])
    par, r1, r2 = int(t["parent"][h]), int(t["ref"][h, 0]), int(t["ref"][h, 1])
    x[:, par] = np.round(x[:, par] * 8.0) / 8.0                       # exact in fp32, so that the two unit vectors cancel exactly
    x[:, r1] = x[:, par] + np.float32([1.0, 0.5, 0.25])
    x[:, r2] = x[:, par] - np.float32([1.0, 0.5, 0.25])
    side = sides(c)
    lone = [g for g in groups(c) if g[1] < 0 and not side[g[0]]][-1][0]
    moved = [int(t["parent"][lone]), int(t["ref"][lone, 0]), int(t["ref"][lone, 1])]
    x[:, moved] += np.float32([40.0, 0.0, 0.0])
    nan_h = int(np.nonzero((t["mode"] == TRI) & ~np.isin(t["parent"], [par] + moved))[0][0])
    x[B_NAN_POSE, int(t["ref"][nan_h, 2]), 1] = np.nan
    c.update(degenerate_row=h, lone_rotor_row=int(lone), nan_row=nan_h)
    return c


def _case_c():
    """Crosses every block size and stride of the kernels at P = 2: more rows than PLACE_BLOCK, more than ROTOR_BLOCK = HBOND_BLOCK
    acceptors on either side (a wave strides them at least twice), more residues and more ligand atoms than FOLD_BLOCK, rotor groups of
    one and of three on both sides."""
    return _seeded(23, 90, 260, 70, 2, 0.85, 0.4, 0.45)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """a case: dict of x fp32 [P,A,3], lig_idx, lig_active, rec_mask, residue_of, n_residues, types, table, thresholds (read-only by
    convention: the cases are shared between the tests)"""
    return {"a_hand_P2": _case_a, "b_seeded_P3": _case_b, "c_blocks_P2": _case_c}[name]()


@functools.lru_cache(maxsize=None)
def reference(name, orient=True):
    """`place` of a case and `hbonds` of its own hydrogens, computed once"""
    c = make_case(name)
    placed = place(c, orient)
    return {**placed, **hbonds(c, placed["x_h"], placed["placed"])}
