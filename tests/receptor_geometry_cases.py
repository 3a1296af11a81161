"""The test systems shared by tests/test_receptor_geometry_cpu.py and tests/test_receptor_geometry_gpu.py: peptides built by
receptor_geometry_ref.build_peptide, their ReceptorGeometry tables (the reference structure of a case is the built peptide itself) and
hand-made defects with known answers."""
import numpy as np

import receptor_geometry_ref as ref

#: all 20 types twice: 40 residues, about 320 atoms - past one 256-atom tile and no multiple of 64
SEQ40 = ("ALA", "ARG", "ASN", "ASP", "CYS", "GLN", "GLU", "GLY", "HIS", "ILE", "LEU", "LYS", "MET", "PHE", "PRO", "SER", "THR", "TRP", "TYR", "VAL",
         "LEU", "GLY", "TRP", "ALA", "LYS", "SER", "PHE", "THR", "GLU", "VAL", "ARG", "CYS", "TYR", "ILE", "ASP", "MET", "HIS", "ASN", "PRO", "GLN")
DEFECTS = ("none", "mirror_ca", "omega_90", "omega_0", "ring_lifted", "bond_stretched", "leu_superposed")


def host_tables(g):
    """the restatement's view of a ReceptorGeometry"""
    keys = ("radius_signed", "excl_start", "excl_atom", "term_atoms", "term_ref", "res_term_start", "res_term", "res_atom_start", "res_atom")
    return dict({k: getattr(g, k) for k in keys}, term_counts=g.term_counts)


def geometry(names, x, device=None, **kw):
    from physdock_amd.receptor_geometry import ReceptorGeometry
    res, atoms, rid = names
    return ReceptorGeometry.from_names(res, atoms, rid, x, device=device, **kw)


def peptide40():
    """(names, x [A,3] float64, index {(residue, atom): k})"""
    res, atoms, rid, x = ref.build_peptide(SEQ40, oxt=True)
    return (res, atoms, rid), x, ref.atom_index(res, atoms, rid)


def defect(kind, names, x, at):
    """one defect of the 40-residue peptide -> (x', the residues it is expected to mark, the bit it must set)"""
    rid = names[2]
    if kind == "none":
        return x.copy(), [], None
    if kind == "mirror_ca":                       # a D residue: CA through the plane of N, C and CB of ASN 2
        return ref.mirror_through(x, at[2, "CA"], at[2, "N"], at[2, "C"], at[2, "CB"]), [2], 2
    if kind in ("omega_90", "omega_0"):           # the peptide bond 8 - 9 (omega_90) or 27 - 28 (omega_0): everything behind it turns
        s = 8 if kind == "omega_90" else 27
        moving = np.nonzero(rid > s)[0]
        return ref.rotate_about(x, x[at[s, "C"]], x[at[s + 1, "N"]], -90.0 if kind == "omega_90" else 180.0, moving), [s, s + 1], \
            3 if kind == "omega_90" else 4
    if kind == "ring_lifted":                     # CZ of PHE 13 half an Angstrom out of the ring's plane
        y = x.copy()
        n = np.cross(x[at[13, "CD1"]] - x[at[13, "CG"]], x[at[13, "CD2"]] - x[at[13, "CG"]])
        y[at[13, "CZ"]] += 0.5 * n / np.linalg.norm(n)
        return y, [13], 5
    if kind == "bond_stretched":                  # CE - NZ of LYS 24 stretched x 1.4
        y = x.copy()
        y[at[24, "NZ"]] = x[at[24, "CE"]] + 1.4 * (x[at[24, "NZ"]] - x[at[24, "CE"]])
        return y, [24], 0
    if kind == "leu_superposed":                  # the side chain of LEU 20 onto that of LEU 10, a little further off atom by atom
        y = x.copy()
        for k, a in enumerate(("CB", "CG", "CD1", "CD2")):
            y[at[20, a]] = x[at[10, a]] + [0.3 + 0.07 * k, 0.0, 0.0]
        return y, [10, 20], 6
    raise ValueError(kind)


def single_defect_poses():
    """(names, x_ref, poses [7,A,3] float32 in DEFECTS order, expectations)"""
    names, x, at = peptide40()
    made = [defect(k, names, x, at) for k in DEFECTS]
    return names, x, np.stack([m[0] for m in made]).astype(np.float32), [(m[1], m[2]) for m in made]


def combined_poses():
    """(names, x_ref, poses [3,A,3] float32): pose 0 untouched, the six defects spread over poses 1 and 2"""
    names, x, at = peptide40()
    poses = [x.copy(), x.copy(), x.copy()]
    for p, kinds in ((1, ("mirror_ca", "omega_90", "ring_lifted")), (2, ("omega_0", "bond_stretched", "leu_superposed"))):
        for k in kinds:
            poses[p] = defect(k, names, poses[p], at)[0]
    return names, x, np.stack(poses).astype(np.float32)


def two_chain_case():
    """two chains with a break between them, an unknown residue, a masked-out atom and a disulfide ->
    (names, x, mask, chain_of, residue_number, index)"""
    a = ref.build_peptide(("ALA", "CYS", "SER", "MET", "GLY", "LEU"))
    a = (["MSE" if r == 3 else n for n, r in zip(a[0], a[2])],) + a[1:]           # residue 3 has no table: selenomethionine by name
    # the second chain: shifted so that its CYS SG lies 2.05 A from the first chain's
    b = ref.build_peptide(("VAL", "CYS", "THR", "PHE"))
    ia, ib = ref.atom_index(*a[:3]), ref.atom_index(*b[:3])
    shift = a[3][ia[1, "SG"]] + [0.0, 0.0, 2.05] - b[3][ib[1, "SG"]]
    res = a[0] + b[0]
    atoms = a[1] + b[1]
    rid = np.concatenate([a[2], b[2] + 6])
    x = np.concatenate([a[3], b[3] + shift])
    chain = (rid >= 6).astype(np.int64)
    number = np.where(rid >= 6, rid - 6 + 1, rid + 1)
    at = ref.atom_index(res, atoms, rid)
    mask = np.ones(len(rid), bool)
    mask[at[5, "CD2"]] = False
    return (res, atoms, rid), x, mask, chain, number, at


def margins_hold(r64, t, bounds, thresholds=None):
    """the condition of the exact comparisons: every term value and every pair ratio of the float64 restatement lies further from its
    threshold than the bound of its kind, and the smallest pair ratio is unique beyond that bound (0, the sentinel of a pair without a
    position, ties exactly).  bounds: dict(ratio, double).  -> the smallest margin / bound seen"""
    thr = dict(ref.DEFAULT_THRESHOLDS)
    thr.update(thresholds or {})
    tt = ref.term_thresholds(t, thresholds)
    nb, na = t["term_counts"][:2]
    worst = np.inf
    for p in range(r64["term_val"].shape[0]):
        v = r64["term_val"][p]
        fin = np.isfinite(v)
        bound = np.where(np.arange(len(v)) < nb + na, bounds["ratio"], bounds["double"])
        for c in range(2):
            m = np.abs(v - tt[:, c])[fin & ~np.isnan(tt[:, c])] / bound[fin & ~np.isnan(tt[:, c])]
            assert m.size == 0 or m.min() > 1.0, ("a term value sits on its threshold", p, c, m.min())
            worst = min(worst, m.min() if m.size else np.inf)
        q = np.sort(r64["ratio"][p][np.isfinite(r64["ratio"][p])])
        if q.size:
            m = np.abs(q - thr["clash"]).min() / bounds["ratio"]
            assert m > 1.0, ("a pair ratio sits on the clash threshold", p, m)
            worst = min(worst, m)
            if q.size > 1 and q[0] > 0:
                assert q[1] - q[0] > bounds["ratio"], ("the smallest pair ratio is not unique", p, q[:2])
    return worst
