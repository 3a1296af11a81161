"""Integer / float64 definition of the ligand features and of the ideal bounds (TEST INFRASTRUCTURE ONLY).

This is the package's OWN definition of `pd_ligand_features` (physdock_amd/ligand.py, csrc/ligand_features.hip), written in numpy with
whole matrices where the kernel walks bit masks.  It is not RDKit's: no aromaticity perception, ring sizes are those of chordless
cycles, hybridisation and conjugation are the short rules below.

    d_token             Floyd-Warshall over the bond matrix, min(30, d); unreachable pairs 30
    bond_type           order 1 -> 0, 2 -> 1, 3 -> 2, 1.5 -> 3, anything else 4; bond_as_double = int(order); bond_is_aromatic = order 1.5
    bond_in_ring        the ends stay connected when the bond is taken out (Floyd-Warshall again)
    ref_in_ring_of_n    some cycle of n distinct atoms through the atom spans exactly n bonds (an induced cycle), n = 3 .. 8
    pi atom             an atom with a bond of order >= 1.5;  donor  N, O, S, not pi, charge <= 0
    bond_is_conjugated  aromatic; or single between pi-pi or pi-donor; or order >= 2 (not aromatic) with such a single bond at an end
    ref_hybridization   v = h + floor(sum of non-aromatic orders) + (aromatic bonds + 1 if any); lone = max(0, electrons - charge - v) // 2;
                        n = degree + h + lone -> 0, 0, 1, 2, 3, 4, 5, 6 ...; a donor with n = 4 at a conjugated single bond -> 2
    ref_feat [L,167]    0 0 0, charge, eye128[Z - 1], aromatic, eye9[degree], eye7[hybridisation], eye9[h], eye3[chirality], rings 3 .. 8
    rel_tok_feat [L,L,42]  eye32[d_token], eye5[bond_type], token_bonds, bond_as_double, bond_in_ring, conjugated, aromatic
"""
from __future__ import annotations

import numpy as np

FAR = 30
#: valence electrons of the elements the tests use (main group: the group's)
ELECTRONS = {1: 1, 5: 3, 6: 4, 7: 5, 8: 6, 9: 7, 11: 1, 14: 4, 15: 5, 16: 6, 17: 7, 34: 6, 35: 7, 53: 7}
BOND_TYPE = {1.0: 0, 2.0: 1, 3.0: 2, 1.5: 3}
ATOM_TABLES = ("ref_charge", "ref_element", "ref_is_aromatic", "ref_degree", "ref_hybridization", "ref_implicit_valence", "ref_chirality",
               "ref_in_ring_of_3", "ref_in_ring_of_4", "ref_in_ring_of_5", "ref_in_ring_of_6", "ref_in_ring_of_7", "ref_in_ring_of_8")
PAIR_TABLES = ("d_token", "token_bonds", "bond_type", "bond_as_double", "bond_in_ring", "bond_is_conjugated", "bond_is_aromatic")


def _distances(A):
    L = A.shape[0]
    d = np.where(A > 0, 1, 10 ** 6).astype(np.int64)
    np.fill_diagonal(d, 0)
    for k in range(L):
        d = np.minimum(d, d[:, k, None] + d[None, k, :])
    return d


def _induced_cycle_sizes(A, lo=3, hi=8):
    """[L, hi + 1] bool: atom a lies on an induced cycle of n atoms"""
    L = A.shape[0]
    nbr = [np.nonzero(A[a])[0].tolist() for a in range(L)]
    out = np.zeros((L, hi + 1), dtype=bool)
    for s in range(L):
        stack = [(s, (s,))]
        while stack:
            last, path = stack.pop()
            for w in nbr[last]:
                if w == s and len(path) >= lo:
                    idx = np.asarray(path)
                    if int(A[np.ix_(idx, idx)].sum()) // 2 == len(path):      # exactly the cycle's own bonds: no chord
                        out[s, len(path)] = True
                elif w not in path and len(path) < hi:
                    stack.append((w, path + (w,)))
    return out


def features(rec):
    """rec: a `parse_smiles` record (or any dict with elements, bonds, bond_orders, charges, h_count, aromatic, chiral) -> dict of the
    int8 tables under the reference's names, `ref_feat` and `rel_tok_feat` (float32)"""
    z = np.asarray(rec["elements"], dtype=np.int64)
    L = len(z)
    q, h = np.asarray(rec["charges"], dtype=np.int64), np.asarray(rec["h_count"], dtype=np.int64)
    written_arom, chiral = np.asarray(rec["aromatic"], dtype=bool), np.asarray(rec["chiral"], dtype=np.int64)
    order = np.zeros((L, L))
    for (i, j), o in zip(np.asarray(rec["bonds"]).reshape(-1, 2).tolist(), np.asarray(rec["bond_orders"], dtype=np.float64)):
        order[i, j] = order[j, i] = o
    A = (order > 0).astype(np.int64)
    arom_b = order == 1.5
    single = order == 1.0
    multiple = (order >= 2.0)
    d = np.minimum(_distances(A), FAR)
    in_ring = np.zeros((L, L), dtype=bool)
    for i, j in np.argwhere(np.triu(A) > 0).tolist():
        cut = A.copy()
        cut[i, j] = cut[j, i] = 0
        in_ring[i, j] = in_ring[j, i] = _distances(cut)[i, j] < 10 ** 6
    sizes = _induced_cycle_sizes(A)
    pi = (order >= 1.5).any(axis=1)
    donor = np.isin(z, (7, 8, 16)) & ~pi & (q <= 0)
    conj_single = single & ((pi[:, None] & pi[None]) | (pi[:, None] & donor[None]) | (donor[:, None] & pi[None]))
    at_conj = conj_single.any(axis=1)
    conj = arom_b | conj_single | (multiple & (at_conj[:, None] | at_conj[None]))
    degree = A.sum(axis=1)
    n_arom = arom_b.sum(axis=1)
    v = h + np.floor(np.where(arom_b, 0.0, order).sum(axis=1)).astype(np.int64) + np.where(n_arom > 0, n_arom + 1, 0)
    lone = np.maximum(0, np.asarray([ELECTRONS[int(e)] for e in z]) - q - v) // 2
    n = degree + h + lone
    hyb = np.clip(n - 1, 0, 6)
    hyb[donor & (n == 4) & at_conj] = 2
    t = {"ref_charge": q, "ref_element": z - 1, "ref_is_aromatic": written_arom | (n_arom > 0), "ref_degree": np.minimum(degree, 8),
         "ref_hybridization": hyb, "ref_implicit_valence": np.minimum(h, 8), "ref_chirality": np.select([chiral == 2, chiral == 1], [0, 1], 2),
         "d_token": d, "token_bonds": A, "bond_type": np.vectorize(lambda o: BOND_TYPE.get(float(o), 4) if o > 0 else 0)(order),
         "bond_as_double": order.astype(np.int64), "bond_in_ring": in_ring, "bond_is_conjugated": conj, "bond_is_aromatic": arom_b}
    for k in range(3, 9):
        t[f"ref_in_ring_of_{k}"] = sizes[:, k]
    t = {k: np.asarray(a).astype(np.int8) for k, a in t.items()}
    eye = lambda k, idx: np.eye(k, dtype=np.float32)[idx.astype(np.int64)]
    col = lambda a: a.astype(np.float32)[..., None]
    t["ref_feat"] = np.concatenate([np.zeros((L, 3), dtype=np.float32), col(t["ref_charge"]), eye(128, t["ref_element"]),
                                    col(t["ref_is_aromatic"]), eye(9, t["ref_degree"]), eye(7, t["ref_hybridization"]),
                                    eye(9, t["ref_implicit_valence"]), eye(3, t["ref_chirality"])]
                                   + [col(t[f"ref_in_ring_of_{k}"]) for k in range(3, 9)], axis=-1)
    t["rel_tok_feat"] = np.concatenate([eye(32, t["d_token"]), eye(5, t["bond_type"]), col(t["token_bonds"]), col(t["bond_as_double"]),
                                        col(t["bond_in_ring"]), col(t["bond_is_conjugated"]), col(t["bond_is_aromatic"])], axis=-1)
    assert t["ref_feat"].shape == (L, 167) and t["rel_tok_feat"].shape == (L, L, 42)
    return t


def bond_table(rec, t, name):
    """{(i, j): value} of a pair table over the record's bonds, i < j"""
    return {(min(i, j), max(i, j)): int(t[name][i, j]) for i, j in np.asarray(rec["bonds"]).reshape(-1, 2).tolist()}


#: the ligands of the GPU parity test: 1 .. 24 atoms, every bond type, charges, both chirality marks, rings of 3 .. 9 atoms, a bridge
#: between rings, fused and spiro rings
PARITY_SMILES = ("[Na+]", "CCO", "CC#N", "c1ccccc1", "CC(=O)Nc1ccc(O)cc1", "C[N+](C)(C)C", "[O-]C(=O)c1ccc[nH]1", "C1CC1", "CS(=O)(=O)C",
                 "N[C@@H](C)C(=O)O", "N[C@H](C)C(=O)O", "c1ccc2ccccc2c1", "C1CCCCCCCC1", "C1CC12CCC2", "C1CCCCCC1C1CCCCCCC1",
                 "c1cccc(c1C#N)NC(=S)NC(=O)c2ccc(o2)-c3ccc(Br)cc3", "F/C=C/F", "C12C3C4C1C5C2C3C45")
#: L = 128: a ladder of 63 fused four-rings - two rails of 64 atoms, a rung at every atom - and a plain chain
LADDER_128 = "".join(f"C%{10 + k}" for k in range(63)) + "CC" + "".join(f"C%{10 + k}" for k in reversed(range(63)))
CHAIN_128 = "C" * 128
