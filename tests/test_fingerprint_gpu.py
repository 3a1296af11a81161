"""pd_morgan_fingerprint, pd_fingerprint_tanimoto, pd_fingerprint_nearest and pd_fingerprint_maxmin against tests/fingerprint_ref.py
on an MI355X.  Everything is compared BIT FOR BIT, the fp32 quotients included: the kernels are integer work and one IEEE division,
so there is no tolerance anywhere."""
import numpy as np
import pytest
import torch

import aromaticity_ref as ar
import fingerprint_ref as fr
from physdock_amd import MorganFingerprint, PoseClusters
from physdock_amd.ligand import Ligand, LigandLibrary

pytestmark = pytest.mark.gpu

SF6 = ("S", "F", "F", "F", "F", "F", "F")
CASES = ("C", "CC", "c1ccccc1", "C1=CC=CC=C1", "CC1CC1", "[Na+]", "C[N+](C)(C)C", "[O-]C(=O)c1ccc[nH]1") + ar.DEMO_SMILES
KEYS = ("ids", "kept", "bits", "n_features", "popcount")


def _ligand(name):
    if name == "SF6":
        return Ligand.from_graph(SF6, [(0, k) for k in range(1, 7)], None)
    if name == "star128":                                  # the highest degree a Ligand can have: 127 neighbours of one atom
        return Ligand.from_graph(["C"] + ["F"] * 127, [(0, k) for k in range(1, 128)], None, h_count=[0] * 128)
    return Ligand.from_smiles(name)


def _got(fp):
    out = {"ids": fp.ids.cpu().numpy().view(np.uint32), "kept": fp.kept.cpu().numpy(), "bits": fp.bits.cpu().numpy().view(np.uint32),
           "n_features": fp.n_features.cpu().numpy(), "popcount": fp.popcount.cpu().numpy()}
    assert fp.bits.is_cuda and fp.bits.dtype == torch.int32 and fp.kept.dtype == torch.uint8 and fp.n_features.dtype == torch.int32
    return out


_WANT = {}


def _want(lig, radius, n_bits):
    """the restatement of a ligand alone, computed once per (ligand, radius, width)"""
    key = (id(lig), radius, n_bits)
    if key not in _WANT:
        _WANT[key] = (lig, fr.fingerprint(lig, radius, n_bits))
    return _WANT[key][1]


def _same(got, ligands, radius, n_bits, invariants=None, what=""):
    """the rows of a library's result against the restatement of each ligand alone"""
    a = 0
    for g, lig in enumerate(ligands):
        want = _want(lig, radius, n_bits) if invariants is None else fr.fingerprint(lig, radius, n_bits, invariants[a:a + lig.n_atoms])
        L = lig.n_atoms
        assert np.array_equal(got["ids"][a:a + L], want["ids"]), (what, g, "ids")
        assert np.array_equal(got["kept"][a:a + L], want["kept"]), (what, g, "kept")
        assert np.array_equal(got["bits"][g], want["bits"]), (what, g, "bits")
        assert got["n_features"][g] == want["n_features"] and got["popcount"][g] == want["popcount"], (what, g)
        a += L
    assert a == got["ids"].shape[0] and got["ids"].shape[1] == radius + 1 and got["bits"].shape == (len(ligands), n_bits // 32)


@pytest.fixture(scope="module")
def ligands():
    return {s: _ligand(s) for s in CASES + ("SF6", "star128", ar.POLYPHENYLENE_128)}


@pytest.fixture(scope="module")
def rows():
    """random bit rows with planted structure: row 1 is empty, rows 2 and 3 are equal, row 5 is row 4 with one bit more"""
    rng = np.random.default_rng(7)
    out = {}
    for W in (16, 128):
        a = (rng.integers(0, 2 ** 32, (64, W), dtype=np.uint64) & rng.integers(0, 2 ** 32, (64, W), dtype=np.uint64)).astype(np.uint32)
        a[1] = 0
        a[3] = a[2]
        a[5] = a[4]
        a[5, 0] = np.uint32((int(a[4, 0]) | (~int(a[4, 0]) & (int(a[4, 0]) + 1))) & 0xFFFFFFFF)      # the lowest clear bit set
        a[40:48] &= a[40:48] >> np.uint32(3)                # sparser rows
        out[W] = a
    return out


# ------------------------------------------------------------------ the fingerprint kernel
@pytest.mark.parametrize("name", CASES + ("SF6", "star128"))
def test_a_ligand_alone_equals_the_definition(name, ligands):
    lig = ligands[name]
    radius = 3 if name == "c1ccccc1" else 2
    got = _got(LigandLibrary([lig]).fingerprints(radius, device="cuda"))
    _same(got, [lig], radius, 2048, what=name)
    if name == "C":                                                                 # B = 0: a null bond pointer
        assert got["kept"].tolist() == [[1, 1, 0]] and got["n_features"].tolist() == [2]
    if name == "CC":
        assert got["kept"].sum(axis=0).tolist() == [2, 1, 0]
    if name == "c1ccccc1":
        assert got["kept"].sum(axis=0).tolist() == [6, 6, 6, 1] and [len(set(got["ids"][:, r].tolist())) for r in range(4)] == [1] * 4
    if name == "SF6":
        assert got["kept"].sum(axis=0).tolist() == [7, 7, 0]
    if name == "star128":
        assert got["kept"].sum(axis=0).tolist() == [128, 128, 0]


def test_the_largest_ligand(ligands):
    lig = ligands[ar.POLYPHENYLENE_128]
    assert lig.n_atoms == 128
    fp = lig.fingerprint(4, 4096, device="cuda")
    _same(_got(fp), [lig], 4, 4096, what="polyphenylene")
    assert int(fp.kept[64:].sum()) > 0


@pytest.mark.parametrize("radius", range(5))
def test_every_radius_and_width_in_a_mixed_library(radius, ligands):
    """each ligand's rows equal its rows alone - first, last and in the middle of a library"""
    names = list(CASES) + ["SF6", ar.POLYPHENYLENE_128]
    for n_bits, order in zip(fr.N_BITS, (names, names[::-1], names[5:] + names[:5], names[::2] + names[1::2])):
        chosen = [ligands[s] for s in order]
        got = _got(LigandLibrary(chosen).fingerprints(radius, n_bits, device="cuda"))
        _same(got, chosen, radius, n_bits, what=(radius, n_bits))


def test_atom_invariants_are_taken_as_given(ligands):
    chosen = [ligands[s] for s in ("CC", ar.DEMO_SMILES[0], "c1ccccc1")]
    lib = LigandLibrary(chosen)
    inv = np.concatenate([lig.elements for lig in chosen]).astype(np.int64)
    inv[0] = -1                                                                     # 0xFFFFFFFF
    fp = lib.fingerprints(2, 1024, atom_invariants=inv, device="cuda")
    got = _got(fp)
    _same(got, chosen, 2, 1024, invariants=inv.tolist(), what="invariants")
    assert got["ids"][0, 0] == 0xFFFFFFFF and got["ids"][2:, 0].tolist() == inv[2:].tolist()


def test_ten_renumberings_give_the_same_bits(ligands):
    rng = np.random.default_rng(11)
    chosen = [ligands[s] for s in ar.DEMO_SMILES]
    want = LigandLibrary(chosen).fingerprints(3, device="cuda")
    for _ in range(10):
        shuffled = []
        for lig in chosen:
            atoms, bonds, _ = fr.renumbered(lig, rng)
            atoms, bonds = np.asarray(atoms), np.asarray(bonds)
            shuffled.append(Ligand(atoms[:, 0], bonds[:, :2], 0.5 * bonds[:, 2], atoms[:, 1], atoms[:, 2], atoms[:, 3] & 1, None))
        fp = LigandLibrary(shuffled).fingerprints(3, device="cuda")
        assert torch.equal(fp.bits, want.bits) and torch.equal(fp.n_features, want.n_features) and torch.equal(fp.popcount, want.popcount)


def test_kekule_and_aromatic_spellings_meet_only_when_aromatized():
    lib = LigandLibrary.from_smiles(["c1ccccc1", "C1=CC=CC=C1"])
    plain, seen = lib.fingerprints(device="cuda"), lib.fingerprints(aromatize=True, device="cuda")
    assert plain.aromaticity_status is None and seen.aromaticity_status.tolist() == [0, 0]
    assert not torch.equal(plain.bits[0], plain.bits[1]) and torch.equal(seen.bits[0], seen.bits[1])
    assert torch.equal(seen.bits[0], plain.bits[0])
    assert seen.pairwise().tolist() == [[1.0, 1.0], [1.0, 1.0]] and float(plain.pairwise()[0, 1]) < 1.0
    aromatic = lib.aromatized("cuda").fingerprints(device="cuda")                   # the two-step route gives the same rows
    assert torch.equal(aromatic.bits, seen.bits)


def test_explain_names_the_features_of_a_bit(ligands):
    lig = ligands[ar.DEMO_SMILES[1]]
    fp = LigandLibrary([ligands["CC"], lig]).fingerprints(2, 512)                   # the defaults: the current device
    assert fp.bits.device.index == torch.cuda.current_device() and (fp.radius, fp.n_bits, fp.n_ligands) == (2, 512, 2)
    want = fr.fingerprint(lig, 2, 512)
    seen = []
    for bit in range(512):
        feats = fp.explain(1, bit)
        assert bool(feats) == bool(want["bits"][bit >> 5] >> np.uint32(bit & 31) & np.uint32(1))
        assert all(want["kept"][a, r] and want["ids"][a, r] == i and i % 512 == bit for a, r, i in feats)
        seen += feats
    assert len(seen) == want["n_features"]


# ------------------------------------------------------------------ Tanimoto, nearest, MaxMin
@pytest.mark.parametrize("W", (16, 128))
@pytest.mark.parametrize("shape", ((1, 1), (17, 33), (64, 5)))
def test_tanimoto_is_the_fp32_quotient(shape, W, rows):
    n, m = shape
    a, b = rows[W][:n], rows[W][64 - m:][::-1].copy()
    if n > 1:
        b[m // 2] = 0                                                               # an all-zero row on each side (a[1] is one)
    fa, fb = MorganFingerprint.from_bits(a, "cuda"), MorganFingerprint.from_bits(b, "cuda")
    want_sim, want_common = fr.tanimoto(a, b)
    sim, common = fa.cross(fb, common=True)
    assert sim.dtype == torch.float32 and common.dtype == torch.int32 and sim.shape == (n, m)
    assert np.array_equal(sim.cpu().numpy().view(np.uint32), want_sim.view(np.uint32))
    assert np.array_equal(common.cpu().numpy(), want_common)
    assert torch.equal(fa.cross(fb), sim)
    if n > 1:
        assert float(sim[1, m // 2]) == 1.0 and float(sim[0, m // 2]) == 0.0         # an empty union is 1, as pd_plif_pairwise


@pytest.mark.parametrize("W", (16, 128))
def test_pairwise_is_symmetric_with_a_unit_diagonal(W, rows):
    fp = MorganFingerprint.from_bits(rows[W][:50], "cuda")
    sim = fp.pairwise()
    assert torch.equal(sim, sim.T) and bool((sim.diagonal() == 1).all()) and float(sim[2, 3]) == 1.0
    assert np.array_equal(sim.cpu().numpy().view(np.uint32), fr.tanimoto(rows[W][:50], rows[W][:50])[0].view(np.uint32))


@pytest.mark.parametrize("W", (16, 128))
def test_nearest_orders_by_the_exact_fraction(W, rows):
    """k = 1, k = 16 = m and between; rows 2 and 3 of b are equal and 40 .. 47 are sparse, so ties occur and the lower column wins.
    Two distinct fractions that round to one fp32 do not exist up to 4096 bits (`fingerprint_ref.colliding_fractions`: they differ
    by at least 1 / (4096 * 4095) > 2^-24), so that case is not constructed; the kernel compares cross-products all the same."""
    assert fr.colliding_fractions(4096) is None
    a = rows[W]
    fa = MorganFingerprint.from_bits(a, "cuda")
    for m, k in ((16, 1), (16, 16), (16, 5), (64, 16), (64, 7)):
        b = a[:m]
        fb = MorganFingerprint.from_bits(b, "cuda")
        for exclude in (False, True):
            if exclude and k > m - 1:
                continue
            src = fb if exclude else fa
            out = src.neighbours(k) if exclude else fa.nearest(fb, k)
            index, sim, common = fr.nearest(b if exclude else a, b, k, exclude_self=exclude)
            assert np.array_equal(out["index"].cpu().numpy(), index), (W, m, k, exclude)
            assert np.array_equal(out["similarity"].cpu().numpy().view(np.uint32), sim.view(np.uint32)), (W, m, k, exclude)
            assert np.array_equal(out["common"].cpu().numpy(), common), (W, m, k, exclude)
            if exclude:
                assert not (out["index"].cpu().numpy() == np.arange(m)[:, None]).any()
    tie = fa.nearest(MorganFingerprint.from_bits(a[:16], "cuda"), 2)["index"].cpu().numpy()
    assert tie[2].tolist() == [2, 3] and tie[3].tolist() == [2, 3] and tie[1, 0] == 1       # equal rows; the empty row finds itself


def test_nearest_with_constructed_ties():
    b = np.zeros((6, 16), dtype=np.uint32)
    b[:, 3] = [0b0001, 0b1111, 0b0010, 0b0, 0b0011, 0b110011]                        # 1/2, 2/4, 1/2, 0, 1, 2/4 against 0b0011
    a = np.zeros((1, 16), dtype=np.uint32)
    a[0, 3] = 0b0011
    out = MorganFingerprint.from_bits(a, "cuda").nearest(MorganFingerprint.from_bits(b, "cuda"), 6)
    index, sim, common = fr.nearest(a, b, 6)
    assert index.tolist() == [[4, 0, 1, 2, 5, 3]] and out["index"].tolist() == index.tolist()
    assert common.tolist() == [[2, 1, 2, 1, 2, 0]] and out["common"].tolist() == common.tolist()
    assert out["similarity"].tolist() == sim.tolist() == [[1.0, 0.5, 0.5, 0.5, 0.5, 0.0]]


@pytest.mark.parametrize("W", (16, 128))
def test_maxmin_picks_a_diverse_subset(W, rows):
    a = rows[W][:48].copy()
    a[10] = a[9]
    a[11] = a[9]                                                                    # duplicated rows: ties
    fp = MorganFingerprint.from_bits(a, "cuda")
    for n_pick, first in ((1, 0), (1, 5), (7, 0), (12, 9), (48, 0), (48, 47)):
        out = fp.maxmin(n_pick, first)
        picks, far = fr.maxmin(a, n_pick, first)
        assert out["picks"].dtype == torch.int32 and out["picks"].tolist() == picks.tolist(), (W, n_pick, first)
        assert np.array_equal(out["max_similarity"].cpu().numpy().view(np.uint32), far.view(np.uint32)), (W, n_pick, first)
    assert sorted(fp.maxmin(48)["picks"].tolist()) == list(range(48))


def test_the_distance_matrix_goes_to_pose_clusters_as_it_is(ligands):
    names = list(ar.DEMO_SMILES) + ["c1ccccc1", "C1=CC=CC=C1", "CC", "C", "CC1CC1", ar.DEMO_SMILES[1]]
    fp = LigandLibrary([ligands[s] for s in names]).fingerprints(device="cuda")
    want_sim = fr.tanimoto(*[np.stack([fr.fingerprint(ligands[s])["bits"] for s in names])] * 2)[0]
    sim = fp.pairwise()
    assert np.array_equal(sim.cpu().numpy().view(np.uint32), want_sim.view(np.uint32))
    clusters = PoseClusters(cutoff=0.6)
    got = clusters.cluster(1 - sim)
    want = clusters.cluster(torch.from_numpy(np.float32(1) - want_sim).cuda())
    for key in want:
        assert got[key].cpu().numpy().tobytes() == want[key].cpu().numpy().tobytes(), key
    labels = got["labels"].tolist()
    assert labels[1] == labels[-1] and 1 < int(got["n_clusters"]) < len(names)      # the same ligand twice; methane is alone


def test_rejected_calls_launch_nothing(rows):
    from physdock_amd import ops
    L_ = ops._lib.init()
    a = torch.from_numpy(rows[16][:8].view(np.int32)).cuda()
    sim = torch.full((8, 8), -7.0, device="cuda")
    index = torch.full((8, 4), -7, dtype=torch.int32, device="cuda")
    s = ops.stream()
    assert L_.pd_fingerprint_tanimoto(ops.ptr(a), ops.ptr(a), ops.ptr(sim), None, 8, 8, 129, s) == -1
    assert L_.pd_fingerprint_tanimoto(ops.ptr(a), None, ops.ptr(sim), None, 8, 8, 16, s) == -1
    assert L_.pd_fingerprint_nearest(ops.ptr(a), ops.ptr(a), ops.ptr(index), ops.ptr(sim), ops.ptr(index), 8, 8, 16, 8, 1, s) == -1
    assert L_.pd_fingerprint_nearest(ops.ptr(a), ops.ptr(a), ops.ptr(index), ops.ptr(sim), ops.ptr(index), 8, 8, 16, 17, 0, s) == -1
    assert L_.pd_fingerprint_maxmin(ops.ptr(a), ops.ptr(index), 32, ops.ptr(index), ops.ptr(sim), 8, 16, 9, 0, s) == -1
    assert L_.pd_fingerprint_maxmin(ops.ptr(a), ops.ptr(index), 26, ops.ptr(index), ops.ptr(sim), 8, 16, 4, 0, s) == -1      # a short workspace
    lib = LigandLibrary.from_smiles(["CCO"])
    t = lib.tables("cuda")
    args = (ops.ptr(t["atom_start"]), ops.ptr(t["bond_start"]), ops.ptr(t["atoms"]), ops.ptr(t["bonds"]), None, ops.ptr(index), ops.ptr(index),
            ops.ptr(sim), ops.ptr(index), ops.ptr(index), 1, 3, 2)
    assert L_.pd_morgan_fingerprint(*args, 5, 2048, s) == -1 and L_.pd_morgan_fingerprint(*args, 2, 1000, s) == -1
    torch.cuda.synchronize()
    assert bool((sim == -7).all()) and bool((index == -7).all())
