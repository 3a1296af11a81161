"""The case set of the `CanonicalForm` tests (test_canonical_cpu.py, test_canonical_gpu.py): name -> `Ligand`."""
import aromaticity_ref as ar
from physdock_amd.ligand import Ligand


def poly_p_phenylene(rings):
    """`rings` benzene rings joined para by single bonds: 6 * rings atoms"""
    return "c1ccc(cc1)-" + "c1ccc(cc1)-" * (rings - 2) + "c1ccccc1"


def _cage(bonds, n):
    return Ligand.from_graph(["C"] * n, bonds, None)


CAGES = {
    "prismane": ([(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3), (0, 3), (1, 4), (2, 5)], 6),
    "cubane": ([(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)], 8),
    # pentacyclo[3.3.0.0(2,4).0(3,7).0(6,8)]octane: the ring 0 .. 7, the bond 0-4 and the bridges 1-3, 2-6, 5-7
    "cuneane": ([(k, (k + 1) % 8) for k in range(8)] + [(0, 4), (1, 3), (2, 6), (5, 7)], 8),
}
#: the molecules of the issue's step table: name -> (SMILES, steps of the full search)
STEP_TABLE = {
    "neopentane": ("CC(C)(C)C", 4),
    "benzene": ("c1ccccc1", 19),
    "coronene": ("c1cc2ccc3ccc4ccc5ccc6ccc1c7c2c3c4c5c67", 19),
    "adamantane": ("C1C2CC3CC1CC(C2)C3", 41),
    "tri-t-butylbenzene": ("CC(C)(C)c1cc(C(C)(C)C)cc(C(C)(C)C)c1", 46),
    "hexaphenylbenzene": ("c1ccccc1-c1c(-c2ccccc2)c(-c2ccccc2)c(-c2ccccc2)c(-c2ccccc2)c1-c1ccccc1", 1531),
    "p-decaphenyl": (poly_p_phenylene(10), 4095),
}
CAGE_STEPS = {"prismane": 19, "cubane": 81, "cuneane": 17}
CHAIN_21 = poly_p_phenylene(21)                                    # 126 atoms: runs out of 65536 steps
PLAIN = ("C1CC12CCC2", "C1CCC2CCCCC2C1", "C1CCCC2CCCC2C1", "[Na+]", "CC#N", "[13CH4]", "C[N+](C)(C)C")
#: families of stereo spellings: lists of groups, the members of one group are one molecule and the groups differ
ALANINES = (("N[C@@H](C)C(=O)O", "C[C@H](N)C(=O)O", "OC(=O)[C@@H](N)C"), ("N[C@H](C)C(=O)O", "C[C@@H](N)C(=O)O", "OC(=O)[C@H](N)C"))
#: seen along the same frame (O, H, COOH, the other centre) the second centre of `[C@H]...[C@H]` is `@` too: the two chiral acids
#: carry equal marks, the meso acid opposite ones
TARTARIC = (("O[C@H](C(=O)O)[C@H](O)C(=O)O",), ("O[C@@H](C(=O)O)[C@@H](O)C(=O)O",),
            ("O[C@H](C(=O)O)[C@@H](O)C(=O)O", "O[C@@H](C(=O)O)[C@H](O)C(=O)O"))
DIFLUOROETHENES = (("F/C=C/F", "F\\C=C\\F", "C(\\F)=C/F"), ("F/C=C\\F",))
PROPANOLS = (("C[C@H](C)O", "C[C@@H](C)O", "CC(C)O"),)
HEXADIENE = "C/C=C/C=C\\C"
FAMILIES = {"alanine": ALANINES, "tartaric": TARTARIC, "difluoroethene": DIFLUOROETHENES, "propan-2-ol": PROPANOLS}


def all_cases():
    """name -> Ligand, without the 126-atom chain"""
    out = {name: Ligand.from_smiles(s) for name, (s, _) in STEP_TABLE.items()}
    out.update({name: _cage(*spec) for name, spec in CAGES.items()})
    for s in ar.DEMO_SMILES + PLAIN + (HEXADIENE,):
        out[s] = Ligand.from_smiles(s)
    for groups in FAMILIES.values():
        for group in groups:
            for s in group:
                out[s] = Ligand.from_smiles(s)
    return out
