"""The SMARTS reader (physdock_amd/smarts.py), the restatement of a match (tests/substructure_ref.py) against networkx, the anchors
checked by hand and every host-side refusal of the public interface (physdock_amd/substructure.py).  No GPU."""
import numpy as np
import pytest
import torch

import aromaticity_ref as ar
import substructure_ref as sr
from physdock_amd.ligand import Ligand, LigandLibrary
from physdock_amd.smarts import BOND_ALL, BOND_DEFAULT, BOND_RING, MAX_OPS, MAX_QUERY_ATOMS, OPS, bond_state
from physdock_amd.substructure import (PHARMACOPHORE_SMARTS, SmartsPattern, SubstructureMatches, SubstructureQueries, parse_smarts,
                                       pharmacophore_invariants)

SINGLE, DOUBLE, TRIPLE, AROMATIC, OTHER = 0x003, 0x00C, 0x030, 0x0C0, 0x300


def op(name, arg=0):
    return (OPS[name], arg)


def ligand(name):
    if name == "SF6":
        return Ligand.from_graph(("S", "F", "F", "F", "F", "F", "F"), [(0, k) for k in range(1, 7)], None)
    if name == "star128":
        return Ligand.from_graph(["C"] + ["F"] * 127, [(0, k) for k in range(1, 128)], None, h_count=[0] * 128)
    return Ligand.from_smiles(name)


def graph(name):
    return sr.Graph(*sr.tables(ligand(name)))


# ------------------------------------------------------------------ the reader
@pytest.mark.parametrize("text,program", (
    ("C", [op("element_aliphatic", 6)]), ("c", [op("element_aromatic", 6)]), ("Cl", [op("element_aliphatic", 17)]),
    ("*", [op("true")]), ("a", [op("aromatic")]), ("A", [op("aliphatic")]),
    ("[C]", [op("element_aliphatic", 6)]), ("[se]", [op("element_aromatic", 34)]), ("[as]", [op("element_aromatic", 33)]),
    ("[Co]", [op("element_aliphatic", 27)]), ("[Hg]", [op("element_aliphatic", 80)]), ("[#6]", [op("z", 6)]), ("[*]", [op("true")]),
    ("[a]", [op("aromatic")]), ("[A]", [op("aliphatic")]), ("[D3]", [op("degree", 3)]), ("[D]", [op("degree", 1)]),
    ("[H2]", [op("h_count", 2)]), ("[CH]", [op("element_aliphatic", 6), op("h_count", 1), op("and")]), ("[X4]", [op("connectivity", 4)]),
    ("[X]", [op("connectivity", 1)]), ("[R]", [op("ring")]), ("[R0]", [op("ring"), op("not")]), ("[+]", [op("charge", 129)]),
    ("[-]", [op("charge", 127)]), ("[+2]", [op("charge", 130)]), ("[-3]", [op("charge", 125)]), ("[H0]", [op("h_count", 0)]),
    ("[!C]", [op("element_aliphatic", 6), op("not")]), ("[!!C]", [op("element_aliphatic", 6), op("not"), op("not")]),
    ("[N-]", [op("element_aliphatic", 7), op("charge", 127), op("and")]),
    ("[nH]", [op("element_aromatic", 7), op("h_count", 1), op("and")]),
))
def test_every_atom_primitive(text, program):
    p = parse_smarts(text)
    assert isinstance(p, SmartsPattern) and p.n_atoms == 1 and p.bonds == () and p.parents == (-1,) and list(p.programs[0]) == program


def test_precedence_of_the_atom_logic():
    C, N, H1 = op("element_aliphatic", 6), op("element_aliphatic", 7), op("h_count", 1)
    assert list(parse_smarts("[C,N;H1]").programs[0]) == [C, N, op("or"), H1, op("and")]
    assert list(parse_smarts("[C,N&H1]").programs[0]) == [C, N, H1, op("and"), op("or")]
    assert list(parse_smarts("[C,NH1]").programs[0]) == [C, N, H1, op("and"), op("or")]
    assert list(parse_smarts("[!C&!N;H1,H2]").programs[0]) == [C, op("not"), N, op("not"), op("and"), H1, op("h_count", 2), op("or"),
                                                              op("and")]
    g = graph("CNC")                                                                # CH3, NH, CH3
    assert [sr.evaluate(parse_smarts("[C,N;H1]").programs[0], g, a) for a in range(3)] == [False, True, False]
    assert [sr.evaluate(parse_smarts("[C,N&H1]").programs[0], g, a) for a in range(3)] == [True, True, True]


@pytest.mark.parametrize("text,mask", (
    ("CC", BOND_DEFAULT), ("C-C", SINGLE), ("C=C", DOUBLE), ("C#C", TRIPLE), ("C:C", AROMATIC), ("C~C", BOND_ALL), ("C@C", BOND_RING),
    ("C!@C", BOND_ALL & ~BOND_RING), ("C-,=C", SINGLE | DOUBLE), ("C-@C", SINGLE & BOND_RING), ("C-&@C", SINGLE & BOND_RING),
    ("C-,=;@C", (SINGLE | DOUBLE) & BOND_RING), ("C-,=&@C", SINGLE | (DOUBLE & BOND_RING)), ("C!-C", BOND_ALL & ~SINGLE),
    ("C!-!@C", BOND_ALL & ~SINGLE & ~BOND_RING), ("C!:;!-C", BOND_ALL & ~AROMATIC & ~SINGLE),
))
def test_bond_expressions_fold_to_masks(text, mask):
    assert BOND_DEFAULT == SINGLE | AROMATIC and parse_smarts(text).bonds == ((0, 1, mask),)


def test_bond_states():
    assert [bond_state(o2, False) for o2 in (2, 4, 6, 3, 1, 8)] == [0, 2, 4, 6, 8, 8] and bond_state(3, True) == 7


def test_structure_branches_and_ring_closures():
    p = parse_smarts("C1(=O)CC=1")                                                  # the closing end carries the bond
    assert p.n_atoms == 4 and p.bonds == ((0, 1, DOUBLE), (0, 2, BOND_DEFAULT), (2, 3, BOND_DEFAULT), (0, 3, DOUBLE))
    assert p.parents == (-1, 0, 0, 0)
    assert parse_smarts("C=1CC1").bonds[-1] == (0, 2, DOUBLE) and parse_smarts("C=1CC=1").bonds[-1] == (0, 2, DOUBLE)
    p = parse_smarts("C%12CC%12C1CC1")
    assert p.bonds == ((0, 1, BOND_DEFAULT), (1, 2, BOND_DEFAULT), (0, 2, BOND_DEFAULT), (2, 3, BOND_DEFAULT), (3, 4, BOND_DEFAULT),
                       (4, 5, BOND_DEFAULT), (3, 5, BOND_DEFAULT))
    assert p.parents == (-1, 0, 0, 2, 3, 3)
    p = parse_smarts("c1ccc2ccccc2c1")                                              # the parent is the LOWEST earlier neighbour
    assert p.parents == (-1, 0, 1, 2, 3, 4, 5, 6, 3, 0) and len(p.bonds) == 11
    assert parse_smarts("  CC ").text == "CC"


def test_recursive_environments_are_kept_by_text():
    p = parse_smarts("[N;!$(N-C=O);$(N-a),$(N-C=O)]C[$(N-a)]")
    assert p.inner == ("N-C=O", "N-a") and [q.n_atoms for q in p.inner_patterns] == [3, 2]
    assert list(p.programs[0]) == [op("element_aliphatic", 7), op("class", 0), op("not"), op("and"), op("class", 1), op("class", 0),
                                   op("or"), op("and")]
    assert list(p.programs[2]) == [op("class", 1)]
    assert parse_smarts("[$(C(C)[O-])]").inner == ("C(C)[O-]",)                     # branches and brackets inside
    qs = SubstructureQueries(["[$(N-a)]", p, "[$(C=O),$(N-a)]"])
    assert [q.text for q in qs.inner.patterns] == ["N-a", "N-C=O", "C=O"] and qs.inner.inner is None
    ops_ = qs._packed["q_ops"].tolist()
    assert ops_[0] == OPS["class"] | 0 << 8                                         # renumbered over the set
    assert ops_[1:9] == [OPS["element_aliphatic"] | 7 << 8, OPS["class"] | 1 << 8, OPS["not"], OPS["and"], OPS["class"], OPS["class"] | 1 << 8,
                         OPS["or"], OPS["and"]]
    assert ops_[-3:] == [OPS["class"] | 2 << 8, OPS["class"], OPS["or"]]


def test_the_packed_tables():
    qs = SubstructureQueries(["C1CC=1", "[O-]", parse_smarts("N~*")])
    t = qs._packed
    assert t["q_atom_start"].tolist() == [0, 3, 4, 6] and t["q_op_start"].tolist() == [0, 1, 2, 3, 6, 7, 8]
    assert t["q_bond_start"].tolist() == [0, 3, 3, 4]
    assert t["q_bonds"].tolist() == [[0, 1, BOND_DEFAULT, 0], [1, 2, BOND_DEFAULT, 0], [0, 2, DOUBLE, 0], [0, 1, BOND_ALL, 0]]      # by the later atom
    assert all(v.dtype == np.int32 for v in t.values()) and len(qs) == 3 and qs.inner is None
    with pytest.raises(AttributeError):
        qs.n_queries = 2
    with pytest.raises(AttributeError):
        parse_smarts("C").text = "N"


@pytest.mark.parametrize("text,at", (
    ("C.C", 1), ("C/C", 1), ("C\\C", 1), ("[C@H]", 2), ("[C@@]", 2), ("[13C]", 1), ("[C:1]", 2), ("[r5]", 1), ("[R1]", 1), ("[CR2]", 2),
    ("[x2]", 1), ("[v3]", 1), ("[h1]", 1), ("(C)C", 0), ("(C).(C)", 0), ("[H]", 1), ("[H+]", 1), ("[#1]", 1), ("C[$(C[$(C)])]", 6),
    ("[C++]", 3), ("[N--]", 3), ("C1CC", 1), ("C(", 1), ("C)", 1), ("[C", 0), ("C=", 1), ("=C", 0),("CC=1CC-1", 7), ("C11", 2),
    ("C12CC12", 6),("[$C]", 1), ("[$(C]", 1), ("[C,]", 3), ("[]", 1), ("[C;]", 3), ("[#]", 1), ("[#300]", 2),
    ("C%1C", 1), ("Cx", 1), ("C()C", 1), ("", 0), ("  ", 0), ("[C&]", 3), ("C!C", 2),
))
def test_what_is_refused_names_its_position(text, at):
    with pytest.raises(ValueError, match=rf"parse_smarts: position {at}:"):
        parse_smarts(text)


def test_positions_count_leading_blanks_and_inner_patterns():
    with pytest.raises(ValueError, match="position 4:"):
        parse_smarts("  CC.C")
    with pytest.raises(ValueError, match="position 7:"):                            # inside the $(): still a position of the whole text
        parse_smarts("C[$(C-[r5])]")
    with pytest.raises(ValueError, match="a str expected"):
        parse_smarts(None)


def test_the_limits():
    assert parse_smarts("C" * MAX_QUERY_ATOMS).n_atoms == 32
    with pytest.raises(ValueError, match="position 32: more than 32 atoms"):
        parse_smarts("C" * 33)
    assert len(parse_smarts("[" + ",".join(["C"] * 16) + "]").programs[0]) == 31
    assert len(parse_smarts("[!" + ",".join(["C"] * 16) + "]").programs[0]) == MAX_OPS
    with pytest.raises(ValueError, match="position 1: an atom expression of 33 ops"):
        parse_smarts("C[" + ",".join(["C"] * 17) + "]")

    def dense(extra):
        """32 atoms in a chain (31 bonds), atom 0 closed onto the atoms 2 .. 31 (30 bonds) and atom 1 onto `extra` of the atoms from 3"""
        s = "*" + "".join(f"%{10 + k}" for k in range(30)) + "*" + "".join(f"%{40 + k}" for k in range(extra))
        return s + "".join(f"*%{10 + k}" + (f"%{39 + k}" if 1 <= k <= extra else "") for k in range(30))

    assert len(parse_smarts(dense(3)).bonds) == 64 and parse_smarts(dense(3)).n_atoms == 32
    with pytest.raises(ValueError, match="more than 64 bonds"):
        parse_smarts(dense(4))
    inner = [f"[$([#{z}])]" for z in range(2, 35)]
    assert SubstructureQueries(inner[:32]).inner.n_queries == 32
    with pytest.raises(ValueError, match="33 distinct"):
        SubstructureQueries(inner)
    with pytest.raises(ValueError, match=r"more than 32 distinct \$\(\) patterns"):
        parse_smarts("[" + ",".join(f"$([#{z}])" for z in range(2, 35)) + "]")
    assert SubstructureQueries(["C"] * 1024).n_queries == 1024
    with pytest.raises(ValueError, match="1025 queries"):
        SubstructureQueries(["C"] * 1025)
    with pytest.raises(ValueError, match="0 queries"):
        SubstructureQueries([])


# ------------------------------------------------------------------ the restatement
ORACLE_QUERIES = ("c1ccccc1", "C~C~C", "*~*", "*~*~*~*", "C(=O)N", "[#6]~[#7,#8]", "c:c-[N,S]", "*@*!@*", "C1CC1", "[D3](~*)(~*)~*",
                  "[R0;!H0]~[R]", "NC(=S)N", "[C,N;H1]~[c,n]", "c1ccoc1", "F~C~F", "*~1~*~*~*~1", "F~S(~F)(~F)(~F)(~F)~F")
ORACLE_LIGANDS = ("CC", "C1CC1", "CC1CC1", "c1ccccc1", "C1=CC=CC=C1", "c1ccc(cc1)-c1ccccc1", "C[N+](C)(C)C", "[O-]C(=O)c1ccc[nH]1",
                  "FC(F)(F)C(F)(F)F", "C12C3C1C23") + ar.DEMO_SMILES[1:3]


def test_the_restatement_counts_what_networkx_counts():
    nx = pytest.importorskip("networkx")
    from networkx.algorithms.isomorphism import GraphMatcher
    patterns = [parse_smarts(s) for s in ORACLE_QUERIES]
    n_checked = 0
    for name in ORACLE_LIGANDS + ("SF6",):
        g = graph(name)
        target = nx.Graph()
        target.add_nodes_from((a, {"a": a}) for a in range(g.n))
        target.add_edges_from((i, j, {"state": s}) for (i, j), s in g.state.items() if i < j)
        for pat in patterns:
            got = sr.search(pat, g, 10 ** 9, keep=True)
            assert got["status"] == 0
            query = nx.Graph()
            query.add_nodes_from((k, {"k": k}) for k in range(pat.n_atoms))
            query.add_edges_from((lo, hi, {"mask": mask}) for lo, hi, mask in pat.bonds)
            matcher = GraphMatcher(target, query, node_match=lambda t, q: sr.evaluate(pat.programs[q["k"]], g, t["a"]),
                                   edge_match=lambda t, q: bool(q["mask"] >> t["state"] & 1))
            maps = [tuple(sorted(m, key=m.get)) for m in matcher.subgraph_monomorphisms_iter()]      # (t(0), t(1), ..)
            assert got["n_embeddings"] == len(maps), (name, pat.text)
            assert got["n_unique"] == len({frozenset(m) for m in maps}), (name, pat.text)
            assert got["embeddings"] == sorted(maps), (name, pat.text)              # and in lexicographic order
            assert got["atom_hits"] == [any(a in m for m in maps) for a in range(g.n)]
            assert got["anchor_hits"] == [any(a == m[0] for m in maps) for a in range(g.n)]
            n_checked += len(maps)
    assert n_checked > 1500


@pytest.mark.parametrize("query,name,n,unique", (
    ("c1ccccc1", "c1ccc(cc1)-c1ccccc1", 24, 2), ("C~C~C", "C1CC1", 6, 1), ("*~*", "CC", 2, 1), ("F~S(~F)(~F)(~F)(~F)~F", "SF6", 720, 1),
    ("F~C~F", "star128", 16002, 8001), ("c1ccccc1", "C1=CC=CC=C1", 0, 0), ("C", "C", 1, 1), ("[O-]", "CC", 0, 0),
))
def test_anchors_checked_by_hand(query, name, n, unique):
    got = sr.search(parse_smarts(query), graph(name))
    assert (got["n_embeddings"], got["n_unique"], got["status"]) == (n, unique, 0)


def test_the_budget_of_the_restatement():
    """`*~*~*` on propane: anchor 0 tries 0, 1, 2 (3 steps, one embedding), anchor 1 tries 1, 0, 2 - the third candidate is due when
    2 steps are spent"""
    pat, g = parse_smarts("*~*~*"), graph("CCC")
    assert [sr.search(pat, g, m)["n_embeddings"] for m in range(5)] == [0, 0, 0, 2, 2]
    assert [sr.search(pat, g, m)["status"] for m in range(5)] == [2, 2, 2, 0, 0]
    spent = sr.search(pat, g, 2)
    assert spent["anchor_hits"] == [False] * 3 and sr.search(pat, g, 3)["atom_hits"] == [True] * 3
    rows, n = sr.matches(parse_smarts("C~C~C"), graph("C1CC1"), 4, unique=False)
    assert n == 4 and rows.tolist() == [[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0]]
    rows, n = sr.matches(parse_smarts("C~C~C"), graph("C1CC1"), 4, unique=True)
    assert n == 1 and rows.tolist() == [[0, 1, 2]] + [[-1] * 3] * 3


def test_recursive_environments_partition_the_amide_nitrogens():
    for s in ar.DEMO_SMILES:
        g = graph(s)
        amide, other = (sr.search(parse_smarts(q), g)["anchor_hits"] for q in ("[N;$(N-C=O)]", "[N;!$(N-C=O)]"))
        nitrogens = [z == 7 and not ar_ for z, ar_ in zip(g.z, g.aromatic)]
        assert [a or b for a, b in zip(amide, other)] == nitrogens and not any(a and b for a, b in zip(amide, other))
    assert sum(sr.search(parse_smarts("[N;$(N-C=O)]"), graph(ar.DEMO_SMILES[0]))["anchor_hits"]) == 2


def test_the_pharmacophore_table_reads():
    assert [name for name, _ in PHARMACOPHORE_SMARTS] == ["donor", "acceptor", "aromatic", "halogen", "basic", "acidic"]
    qs = SubstructureQueries([s for _, s in PHARMACOPHORE_SMARTS])
    assert qs.n_queries == 6 and all(p.n_atoms == 1 for p in qs.patterns) and qs.inner.n_queries == 6
    g = graph("CC(=O)Nc1ccc(O)cc1")                                                 # paracetamol
    bits = [sum(int(sr.search(p, g)["anchor_hits"][a]) << c for c, p in enumerate(qs.patterns)) for a in range(g.n)]
    assert bits == [0, 0, 2, 1, 4, 4, 4, 4, 3, 4, 4]
    g = graph("NCC(=O)[O-]")
    assert [sum(int(sr.search(p, g)["anchor_hits"][a]) << c for c, p in enumerate(qs.patterns)) for a in range(g.n)] == [19, 0, 0, 2, 34]
    for text in pharmacophore_invariants.__doc__.split("\n"):
        assert not text.strip()[:1].isdigit() or text.split()[2] == PHARMACOPHORE_SMARTS[int(text.split()[0])][1]


# ------------------------------------------------------------------ the host checks of the public interface
def test_every_host_check_is_made_without_a_gpu():
    lib = LigandLibrary.from_smiles(["CCO", "c1ccccc1"])
    for queries, why in ((["C.C"], "query 0: parse_smarts: position 1"), (["C", "[r5]"], "query 1: parse_smarts: position 1"),
                         ([], "0 queries"), (["C"] * 1025, "1025 queries"), ([3], "query 0 is a int"), (7, "a sequence of SMARTS")):
        with pytest.raises(ValueError, match="LigandLibrary.substructure: SubstructureQueries: " + why):
            lib.substructure(queries)
    for max_steps in (-1, 2 ** 31, 1.5, True, None):
        with pytest.raises(ValueError, match="max_steps"):
            lib.substructure("C", max_steps=max_steps)
    with pytest.raises(ValueError, match="aromatize"):
        lib.ligands[0].substructure("C", aromatize=1)
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    out = {"n_embeddings": zeros(2, 2), "n_unique": zeros(2, 2), "status": zeros(2, 2), "atom_hits": zeros(9, 1), "anchor_hits": zeros(9, 1)}
    out["n_embeddings"][1, 0] = 3
    out["atom_hits"][4, 0] = 2
    found = SubstructureMatches(lib, SubstructureQueries(["c", "O"]), {}, None, 100, torch.device("cpu"), out, None, None)
    assert found.has.tolist() == [[False, False], [True, False]] and found.select(0) == [1] and found.select(1) == []
    assert found.atoms(1).tolist() == [False] * 4 + [True] + [False] * 4 and not found.atoms(0).any() and not found.anchors(1).any()
    with pytest.raises(AttributeError):
        found.status = None
    for call in (lambda: found.atoms(2), lambda: found.anchors(-1), lambda: found.select(True), lambda: found.matches(2),
                 lambda: found.matches("0")):
        with pytest.raises(ValueError, match="query"):
            call()
    for m in (0, 257, 2.0, False):
        with pytest.raises(ValueError, match="max_matches"):
            found.matches(0, m)
    with pytest.raises(ValueError, match="unique"):
        found.matches(0, 4, unique=1)
    with pytest.raises(ValueError, match="atom_invariants of shape"):
        lib.fingerprints(atom_invariants=np.zeros(8, dtype=np.int64))
