"""pd_substructure_search and pd_substructure_matches against tests/substructure_ref.py on an MI355X.  Everything is integer work in a
fixed order, so every comparison is EXACT - exhausted budgets included - and every case but the budget test must end with status 0:
a cap may not hide a failure.  The budgets were chosen on the CPU: with `MAX_STEPS` the restatement finishes every case here."""
import numpy as np
import pytest
import torch

import aromaticity_ref as ar
import fingerprint_ref as fr
import substructure_ref as sr
from physdock_amd import SubstructureQueries, parse_smarts, pharmacophore_invariants
from physdock_amd.ligand import Ligand, LigandLibrary
from physdock_amd.substructure import PHARMACOPHORE_SMARTS

pytestmark = pytest.mark.gpu

MAX_STEPS = 65536
SF6 = ("S", "F", "F", "F", "F", "F", "F")
CASES = ("C", "CC", "c1ccccc1", "C1=CC=CC=C1", "CC1CC1", "[Na+]", "C[N+](C)(C)C", "[O-]C(=O)c1ccc[nH]1") + ar.DEMO_SMILES
NAMES = CASES + ("SF6", "star128", ar.POLYPHENYLENE_128)
#: 33 queries: the hit rows cross a word boundary.  Every primitive, every bond symbol, rings, branches, $() and a miss
QUERIES = ("c1ccccc1", "C~C~C", "*~*", "F~S(~F)(~F)(~F)(~F)~F", "F~C~F", "C", "[#6]", "*", "a", "A", "[N;!$(N-C=O)]", "[N;$(N-C=O)]",
           "[C,N;H1]", "[C,N&H1]", "C=O", "C#N", "[O-,N-]", "[nH]", "c:c", "c-c", "C!@C", "*@*", "[R0;D3]", "[X4]", "[+]", "[Na+]", "Br",
           "[C;X4](F)(F)F", "NC(=S)N", "[$(c1ccccc1),$(C=O)]~[#7,#8,#16]", "C1CCCCC1", "[se,as,S,s;R]", "c1ccc(cc1)-,:*")
#: 32 atoms: the methyl end of the polyphenylene, five of its rings and one atom of the sixth
LONG_QUERY = "Cc1ccc(cc1)" + "-c1ccc(cc1)" * 4 + "-c"
CHAIN_QUERY = "~".join("*" * 32)


def _ligand(name):
    if name == "SF6":
        return Ligand.from_graph(SF6, [(0, k) for k in range(1, 7)], None)
    if name == "star128":
        return Ligand.from_graph(["C"] + ["F"] * 127, [(0, k) for k in range(1, 128)], None, h_count=[0] * 128)
    return Ligand.from_smiles(name)


@pytest.fixture(scope="module")
def ligands():
    return {s: _ligand(s) for s in NAMES}


@pytest.fixture(scope="module")
def queries():
    assert len(QUERIES) == 33
    return SubstructureQueries(QUERIES)


@pytest.fixture(scope="module")
def want(ligands, queries):
    """the restatement of every ligand alone against every query, computed once: name -> the rows of `library_search`"""
    out = {}
    for name, lig in ligands.items():
        out[name] = sr.library_search([lig], queries.patterns, MAX_STEPS)
        assert not out[name]["status"].any(), name                                  # the restatement itself finishes
    return out


def _got(found):
    for key in ("n_embeddings", "n_unique", "status", "atom_hits", "anchor_hits"):
        v = getattr(found, key)
        assert v.is_cuda and v.dtype == torch.int32, key
    return {"n_embeddings": found.n_embeddings.cpu().numpy(), "n_unique": found.n_unique.cpu().numpy(), "status": found.status.cpu().numpy(),
            "atom_hits": found.atom_hits.cpu().numpy().view(np.uint32), "anchor_hits": found.anchor_hits.cpu().numpy().view(np.uint32)}


def _same(got, names, ligands, want, what=""):
    """the rows of a library's result against the restatement of each ligand alone"""
    a = 0
    for g, name in enumerate(names):
        L, w = ligands[name].n_atoms, want[name]
        for key in ("n_embeddings", "n_unique", "status"):
            assert np.array_equal(got[key][g], w[key][0]), (what, name, key, got[key][g].tolist(), w[key][0].tolist())
        for key in ("atom_hits", "anchor_hits"):
            assert np.array_equal(got[key][a:a + L], w[key]), (what, name, key)
        a += L
    assert a == got["atom_hits"].shape[0] and not got["status"].any()


# ------------------------------------------------------------------ the search kernel against the restatement
@pytest.mark.parametrize("name", NAMES)
def test_a_ligand_alone_equals_the_definition(name, ligands, queries, want):
    found = ligands[name].substructure(queries, max_steps=MAX_STEPS, device="cuda")
    got = _got(found)
    assert got["n_embeddings"].shape == (1, 33) and got["atom_hits"].shape == (ligands[name].n_atoms, 2)
    _same(got, [name], ligands, want, what=name)
    n, u = dict(zip(QUERIES, got["n_embeddings"][0].tolist())), dict(zip(QUERIES, got["n_unique"][0].tolist()))
    if name == "C":                                                                 # B == 0: a null bond pointer
        assert (n["C"], n["*"], n["*~*"], n["[X4]"]) == (1, 1, 0, 1)
    if name == "CC":
        assert (n["*~*"], u["*~*"]) == (2, 1)
    if name == "SF6":
        assert (n[QUERIES[3]], u[QUERIES[3]]) == (720, 1)
    if name == "star128":
        assert (n["F~C~F"], u["F~C~F"]) == (16002, 8001) and n["*~*"] == 254
    if name == "C1=CC=CC=C1":
        assert (n["c1ccccc1"], n["C1CCCCC1"]) == (0, 0) and n["*@*"] == 12
    if name == ar.POLYPHENYLENE_128:
        assert (n["c1ccccc1"], u["c1ccccc1"]) == (12 * 21, 21) and bool(found.has[0, 0]) and not bool(found.has[0, 1])
    assert found.has.dtype == torch.bool and torch.equal(found.has, found.n_embeddings > 0)


def test_a_mixed_library_does_not_depend_on_the_position(ligands, queries, want):
    """each ligand's rows equal its rows alone - first, last and in the middle of a library"""
    names = list(NAMES)
    for order in (names, names[::-1], names[5:] + names[:5]):
        lib = LigandLibrary([ligands[s] for s in order])
        found = lib.substructure(queries, max_steps=MAX_STEPS, device="cuda")
        _same(_got(found), order, ligands, want, what=order[0])
        again = lib.substructure(queries, max_steps=MAX_STEPS, device="cuda")       # two launches: identical bytes
        for key in ("n_embeddings", "n_unique", "status", "atom_hits", "anchor_hits"):
            assert torch.equal(getattr(found, key), getattr(again, key)), key
    q = QUERIES.index("C#N")
    assert found.select(q) == [g for g, s in enumerate(order) if want[s]["n_embeddings"][0, q] > 0] and len(found.select(q)) == 4
    atoms = found.atoms(q).cpu().numpy()
    assert atoms.dtype == bool and int(atoms.sum()) == 8 and int(found.anchors(q).sum()) == 4


def test_a_ligand_is_found_by_its_own_smiles(ligands):
    for s in ar.DEMO_SMILES:
        lig, pat = ligands[s], parse_smarts(s)
        assert pat.n_atoms == lig.n_atoms
        found = LigandLibrary([ligands["c1ccccc1"], lig]).substructure([pat], max_steps=MAX_STEPS, device="cuda")
        w = sr.search(pat, sr.Graph(*sr.tables(lig)), MAX_STEPS)
        assert found.n_embeddings.tolist() == [[0], [w["n_embeddings"]]] and w["n_embeddings"] >= 1 and w["status"] == 0
        assert found.n_unique.tolist() == [[0], [1]] and found.status.tolist() == [[0], [0]]
        assert bool(found.atoms(0)[6:].all()) and not bool(found.atoms(0)[:6].any())
    assert [ligands[s].n_atoms for s in ar.DEMO_SMILES].count(23) >= 1


def test_a_query_of_32_atoms(ligands):
    pat = parse_smarts(LONG_QUERY)
    assert pat.n_atoms == 32
    lig = ligands[ar.POLYPHENYLENE_128]
    found = lig.substructure([pat, "C"], max_steps=MAX_STEPS, device="cuda")
    w = sr.search(pat, sr.Graph(*sr.tables(lig)), MAX_STEPS)
    assert w["status"] == 0 and w["n_embeddings"] > 0
    assert found.n_embeddings[0].tolist() == [w["n_embeddings"], 2] and found.n_unique[0].tolist() == [w["n_unique"], 2]      # two methyls
    assert found.status[0].tolist() == [0, 0]
    assert found.atoms(0).tolist() == w["atom_hits"] and found.anchors(0).tolist() == w["anchor_hits"]


# ------------------------------------------------------------------ individual behaviours
def test_aromatize_perceives_before_it_searches():
    lib = LigandLibrary.from_smiles(["C1=CC=CC=C1", "c1ccccc1"])
    plain, seen = lib.substructure("c1ccccc1", device="cuda"), lib.substructure("c1ccccc1", aromatize=True, device="cuda")
    assert plain.n_embeddings.tolist() == [[0], [12]] and seen.n_embeddings.tolist() == [[12], [12]]
    assert seen.n_unique.tolist() == [[1], [1]] and seen.status.tolist() == [[0], [0]]
    assert plain.aromaticity_status is None and seen.aromaticity_status.tolist() == [0, 0]
    assert lib.substructure("C1=CC=CC=C1", aromatize=True, device="cuda").n_embeddings.tolist() == [[0], [0]]


def test_recursive_environments_partition_the_amide_nitrogens(ligands):
    chosen = [ligands[s] for s in ar.DEMO_SMILES]
    lib = LigandLibrary(chosen)
    found = lib.substructure(["[N;!$(N-C=O)]", "[N;$(N-C=O)]", "N"], device="cuda")
    assert found.inner_status.shape == (5, 1) and not found.inner_status.any() and not found.status.any()
    other, amide, all_n = (found.anchors(q) for q in range(3))
    assert torch.equal(other | amide, all_n) and not bool((other & amide).any()) and int(amide.sum()) > 0 and int(other.sum()) > 0
    a = 0
    for g, lig in enumerate(chosen):
        graph = sr.Graph(*sr.tables(lig))
        for q, pat in enumerate(found.queries.patterns):
            w = sr.search(pat, graph)
            assert found.anchors(q)[a:a + lig.n_atoms].tolist() == w["anchor_hits"] and int(found.n_embeddings[g, q]) == w["n_embeddings"]
        a += lig.n_atoms


def test_an_exhausted_budget_equals_the_restatement(ligands):
    """a chain of 32 any-atoms on the polyphenylene: anchors spend their 300 steps and stop with what they found, and the counts
    are those of the restatement under the same budget"""
    lig, pat = ligands[ar.POLYPHENYLENE_128], parse_smarts(CHAIN_QUERY)
    assert pat.n_atoms == 32
    graph = sr.Graph(*sr.tables(lig))
    for max_steps in (0, 31, 300):
        w = sr.search(pat, graph, max_steps)
        found = lig.substructure([pat, "c"], max_steps=max_steps, device="cuda")
        assert w["status"] == 2 and found.status[0].tolist() == [2, 2 if max_steps == 0 else 0]
        assert int(found.n_embeddings[0, 0]) == w["n_embeddings"] and int(found.n_unique[0, 0]) == w["n_unique"]
        assert found.atoms(0).tolist() == w["atom_hits"] and found.anchors(0).tolist() == w["anchor_hits"]
        assert int(found.n_embeddings[0, 1]) == (0 if max_steps == 0 else 126)      # the aromatic atoms; the two methyls are not
    assert w["n_embeddings"] > 0
    rows = found.matches(0, 8, unique=False)
    want_rows, n = sr.matches(pat, graph, 8, False, 300)
    assert rows["n_written"].tolist() == [n] and np.array_equal(rows["atoms"][0].cpu().numpy(), want_rows)


@pytest.mark.parametrize("query,name", (("c1ccccc1", "c1ccc(cc1)-c1ccccc1"), ("C~C~C", "C1CC1"), ("F~S(~F)(~F)(~F)(~F)~F", "SF6"),
                                        ("F~C~F", "star128"), ("[N;$(N-C=O)]", ar.DEMO_SMILES[0]), ("[O-]", "CC")))
def test_matches_come_in_the_stated_order(query, name):
    lig = _ligand(name)
    lib = LigandLibrary([_ligand("CC"), lig, lig])
    found = lib.substructure(["*", query], max_steps=MAX_STEPS, device="cuda")
    pat = found.queries.patterns[1]
    both = [sr.search(pat, sr.Graph(*sr.tables(x)), MAX_STEPS, keep=True) for x in lib.ligands[:2]]      # the restatement, once

    def want(g, M, unique):
        rows = [e for e, u in zip(both[g]["embeddings"], both[g]["unique"]) if u or not unique][:M]
        out = np.full((M, pat.n_atoms), -1, dtype=np.int32)
        out[:len(rows)] = np.asarray(rows, dtype=np.int32).reshape(len(rows), pat.n_atoms)
        return out, len(rows)

    total = {False: int(found.n_embeddings[1, 1]), True: int(found.n_unique[1, 1])}
    assert total == {False: both[1]["n_embeddings"], True: both[1]["n_unique"]}
    for unique in (False, True):
        for M in sorted({1, max(total[unique] - 1, 1), max(total[unique], 1), min(total[unique] + 3, 256), 16}):
            if M > 256:
                continue
            got = found.matches(1, M, unique=unique)
            want_rows, n = want(1, M, unique)
            assert n == min(total[unique], M)
            assert got["atoms"].dtype == torch.int32 and got["atoms"].shape == (3, M, pat.n_atoms)
            assert got["n_written"].tolist()[1:] == [n, n], (unique, M)
            for g in (1, 2):
                assert np.array_equal(got["atoms"][g].cpu().numpy(), want_rows), (unique, M, g)
            assert bool((got["atoms"][1, n:] == -1).all()) and bool((got["atoms"][1, :n] >= 0).all())
            w0, n0 = want(0, M, unique)
            assert int(got["n_written"][0]) == n0 and np.array_equal(got["atoms"][0].cpu().numpy(), w0)
    one = found.matches(0, 256, unique=False)                                       # a one-atom query, the largest M
    assert one["n_written"].tolist() == [2, lig.n_atoms, lig.n_atoms] and one["atoms"][1, :lig.n_atoms, 0].tolist() == list(range(lig.n_atoms))


def test_pharmacophore_invariants_feed_the_fingerprints(ligands):
    names = list(ar.DEMO_SMILES) + ["[O-]C(=O)c1ccc[nH]1", "C[N+](C)(C)C", "C1=CC=CC=C1"]
    chosen = [ligands[s] for s in names]
    lib = LigandLibrary(chosen)
    inv = pharmacophore_invariants(lib, device="cuda")
    assert inv.is_cuda and inv.dtype == torch.int32 and inv.shape == (lib.n_atoms,)
    patterns = SubstructureQueries([s for _, s in PHARMACOPHORE_SMARTS]).patterns
    want_inv = []
    for lig in chosen:
        graph = sr.Graph(*sr.tables(lig))
        hits = [sr.search(p, graph)["anchor_hits"] for p in patterns]
        want_inv += [sum(int(hits[c][a]) << c for c in range(6)) for a in range(lig.n_atoms)]
    assert inv.tolist() == want_inv and 0 < max(want_inv) < 64
    fp = lib.fingerprints(2, 1024, atom_invariants=inv, device="cuda")
    a = 0
    for g, lig in enumerate(chosen):
        w = fr.fingerprint(lig, 2, 1024, want_inv[a:a + lig.n_atoms])
        assert np.array_equal(fp.bits[g].cpu().numpy().view(np.uint32), w["bits"]), g
        assert np.array_equal(fp.ids[a:a + lig.n_atoms].cpu().numpy().view(np.uint32), w["ids"]), g
        a += lig.n_atoms
    assert torch.equal(lib.fingerprints(2, 1024, atom_invariants=inv.cpu().numpy(), device="cuda").bits, fp.bits)      # the host route
    seen = pharmacophore_invariants(LigandLibrary([chosen[-1]]), aromatize=True, device="cuda")
    assert seen.tolist() == [4] * 6 and inv[-6:].tolist() == [0] * 6
    with pytest.raises(ValueError, match="atom_invariants of shape"):
        lib.fingerprints(atom_invariants=inv[:-1])


def test_rejected_calls_launch_nothing(queries):
    from physdock_amd import ops
    L_ = ops._lib.init()
    lib = LigandLibrary.from_smiles(["CCO", "c1ccccc1"])
    t = lib.tables("cuda")
    qs = SubstructureQueries(["CO", "c:c", "O"])
    ptrs, sizes = qs._args(torch.device("cuda", torch.cuda.current_device()))
    sentinel = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")
    outs = [sentinel(2, 3), sentinel(2, 3), sentinel(2, 3), sentinel(9, 1), sentinel(9, 1)]
    rows, n_written = sentinel(2, 4, 2), sentinel(2)
    s = ops.stream()
    lig = [ops.ptr(t["atom_start"]), ops.ptr(t["bond_start"]), ops.ptr(t["atoms"]), ops.ptr(t["bonds"])]
    out_p = [ops.ptr(v) for v in outs]
    G, N, B = 2, 9, 8

    def search(lig=lig, ptrs=ptrs, cls=None, out_p=out_p, dims=(G, N, B), sizes=sizes, max_steps=100):
        return L_.pd_substructure_search(*lig, *ptrs, cls, *out_p, *dims, *sizes, max_steps, s)

    def matches(lig=lig, ptrs=ptrs, out=(ops.ptr(rows), ops.ptr(n_written)), dims=(G, N, B), sizes=sizes, q=0, nq=2, M=4, unique=1,
                max_steps=100):
        return L_.pd_substructure_matches(*lig, *ptrs, None, *out, *dims, *sizes, q, nq, M, unique, max_steps, s)

    swap = lambda seq, k, v: [v if i == k else x for i, x in enumerate(seq)]
    for k in (0, 1, 2, 3):
        assert search(lig=swap(lig, k, None)) == -1 and matches(lig=swap(lig, k, None)) == -1
    for k in range(5):
        assert search(ptrs=swap(ptrs, k, None)) == -1 and matches(ptrs=swap(ptrs, k, None)) == -1
        assert search(out_p=swap(out_p, k, None)) == -1
    assert search(lig=swap(lig, 2, lig[2] + 2)) == -1 and search(out_p=swap(out_p, 0, out_p[0] + 1)) == -1      # misaligned
    assert search(cls=out_p[3] + 2) == -1 and matches(out=(ops.ptr(rows) + 2, ops.ptr(n_written))) == -1
    assert matches(out=(None, ops.ptr(n_written))) == -1 and matches(out=(ops.ptr(rows), None)) == -1
    assert search(dims=(0, N, B)) == -1 and search(dims=(G, 1, B)) == -1 and search(dims=(G, N, -1)) == -1
    assert search(sizes=swap(sizes, 0, 0)) == -1 and search(max_steps=-1) == -1 and matches(max_steps=-1) == -1
    assert search(sizes=swap(sizes, 1, 3 * 32 + 1)) == -1 and search(sizes=swap(sizes, 1, 2)) == -1      # beyond the limits
    assert search(sizes=swap(sizes, 2, 5 * 32 + 1)) == -1 and search(sizes=swap(sizes, 3, 3 * 64 + 1)) == -1
    assert search(sizes=swap(sizes, 3, -1)) == -1
    assert search(dims=(65536, 65536, B)) == -3 and search(sizes=[1025, 1025, 1025, 0]) == -3 and search(dims=(G, 2 * 128 + 1, B)) == -3
    for bad in (dict(q=-1), dict(q=3), dict(nq=0), dict(nq=33), dict(M=0), dict(M=257), dict(unique=2), dict(unique=-1)):
        assert matches(**bad) == -1, bad
    assert matches(dims=(65536, 65536, B)) == -3
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in outs + [rows, n_written])
    assert search() == 0 and matches() == 0                                         # and the same arguments, accepted
    torch.cuda.synchronize()
    assert outs[0].tolist() == [[1, 0, 1], [0, 12, 0]] and outs[2].tolist() == [[0] * 3] * 2 and n_written.tolist() == [1, 0]
    assert rows[0].tolist() == [[1, 2]] + [[-1, -1]] * 3
