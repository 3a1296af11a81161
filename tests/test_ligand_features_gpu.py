"""pd_ligand_features against tests/ligand_features_ref.py on an MI355X: every int8 table and both float blocks must be EXACTLY equal
(the kernel is integer work; there is no tolerance to choose), a ligand's bits must not depend on the library around it, and the joins
- the reference conformer, `into_batch` - do what they say."""
import numpy as np
import pytest
import torch

import ligand_features_ref as ref
from physdock_amd.ligand import ATOM_COLUMNS, PAIR_COLUMNS, Ligand, LigandLibrary
from physdock_amd.smiles import parse_smiles

pytestmark = pytest.mark.gpu

ALL_SMILES = ref.PARITY_SMILES + (ref.LADDER_128, ref.CHAIN_128)
NAMES = ATOM_COLUMNS + PAIR_COLUMNS + ("ref_feat", "rel_tok_feat")


@pytest.fixture(scope="module")
def expected():
    return {s: ref.features(parse_smiles(s)) for s in ALL_SMILES}


@pytest.fixture(scope="module")
def alone():
    return {s: {k: v.cpu().numpy() for k, v in Ligand.from_smiles(s).features("cuda").items()} for s in ALL_SMILES}


def _same(got, want, what):
    for name in NAMES:
        g, w = np.asarray(got[name]), want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4].tolist())


@pytest.mark.parametrize("smiles", ref.PARITY_SMILES)
def test_tables_and_blocks_equal_the_restatement(smiles, expected, alone):
    n = len(parse_smiles(smiles)["elements"])
    assert 1 <= n <= 26
    _same(alone[smiles], expected[smiles], smiles)


def test_a_single_atom(expected, alone):
    got = alone["[Na+]"]
    assert got["ref_feat"].shape == (1, 167) and got["rel_tok_feat"].shape == (1, 1, 42)
    assert got["ref_charge"][0] == 1 and got["ref_element"][0] == 10 and got["ref_hybridization"][0] == 0 and got["d_token"][0, 0] == 0
    assert got["rel_tok_feat"][0, 0, 0] == 1.0 and got["rel_tok_feat"][0, 0].sum() == 2.0          # eye32[0] and eye5[0]


@pytest.mark.parametrize("smiles", [ref.LADDER_128, ref.CHAIN_128], ids=["ladder128", "chain128"])
def test_the_largest_ligand(smiles, expected, alone):
    assert len(parse_smiles(smiles)["elements"]) == 128
    _same(alone[smiles], expected[smiles], smiles[:12])
    if smiles == ref.CHAIN_128:
        assert alone[smiles]["d_token"][0, 127] == 30 and alone[smiles]["d_token"][0, 29] == 29
    else:
        assert alone[smiles]["ref_in_ring_of_4"].all() and not alone[smiles]["ref_in_ring_of_6"].any()


def test_a_nine_ring_has_no_size_flag_but_ring_bonds(alone):
    got = alone["C1CCCCCCCC1"]
    assert not any(got[f"ref_in_ring_of_{k}"].any() for k in range(3, 9))
    assert got["bond_in_ring"].sum() == 18 and (got["bond_in_ring"] == got["token_bonds"]).all()


def test_one_launch_for_a_library_gives_each_ligand_its_own_bits(alone):
    ligands = [Ligand.from_smiles(s) for s in ALL_SMILES]
    for order in (list(range(len(ligands))), list(reversed(range(len(ligands))))):
        lib = LigandLibrary([ligands[k] for k in order])
        out = lib.features("cuda")
        assert out["atom_table"].shape == (lib.n_atoms, 16) and out["rel_tok_feat"].shape == (lib.n_pairs, 42)
        for g, k in enumerate(order):
            got = {name: v.cpu().numpy() for name, v in lib.split(out, g).items()}
            for name in NAMES:
                assert np.array_equal(got[name], alone[ALL_SMILES[k]][name]), (ALL_SMILES[k][:16], name, g)
        assert not out["atom_table"][:, 13:].any() and not out["pair_table"][:, 7].any()


def _cb_side(pos):
    """(CB - CA) . ((N - CA) x (C - CA)) of alanine written N, CA, CB, C, O, O"""
    n, ca, cb, c = (pos[k].astype(np.float64) for k in range(4))
    return float((cb - ca) @ np.cross(n - ca, c - ca))


def test_embed_reference_and_handedness():
    sides = {}
    for smiles in ("N[C@@H](C)C(=O)O", "N[C@H](C)C(=O)O", "CC(=O)Nc1ccc(O)cc1"):
        lig = Ligand.from_smiles(smiles)
        out = lig.embed_reference(seed=0, C=32, device="cuda")
        pos = out["ref_pos"].cpu().numpy()
        assert pos.shape == (lig.n_atoms, 3) and np.isfinite(pos).all()
        assert out["max_violation"] <= 0.1 and out["n_accepted"] >= 1
        assert torch.equal(out["ref_feat"][:, :3], out["ref_pos"]) and torch.equal(out["ref_feat"][:, 3:], lig.features("cuda")["ref_feat"][:, 3:])
        sides[smiles] = _cb_side(pos) if smiles.startswith("N[") else None
    assert sides["N[C@@H](C)C(=O)O"] > 0.0 > sides["N[C@H](C)C(=O)O"]          # L-alanine is positive in this convention


def test_into_batch_writes_the_ligand_and_nothing_else():
    from physdock_amd.driver import ligand_atom_mask
    from physdock_amd.synthetic import small_batch
    batch = {k: v.to("cuda") for k, v in small_batch(0).items()}
    before = {k: v.clone() for k, v in batch.items()}
    atoms, tokens = ligand_atom_mask(batch), batch["is_ligand"].bool()
    assert int(atoms.sum()) == 6
    with pytest.raises(ValueError, match="atoms"):
        Ligand.from_smiles("CCO").into_batch(batch, ref_pos=torch.zeros(3, 3))
    assert all(torch.equal(batch[k], before[k]) for k in batch)
    lig = Ligand.from_smiles("CC(=O)NCO")
    pos = torch.arange(18, dtype=torch.float32, device="cuda").view(6, 3)
    lig.into_batch(batch, ref_pos=pos)
    f = lig.features("cuda")
    want = f["ref_feat"].clone()
    want[:, :3] = pos
    assert torch.equal(batch["ref_feat"][atoms], want) and torch.equal(batch["ref_pos"][atoms], pos)
    assert torch.equal(batch["rel_tok_feat"][tokens][:, tokens], f["rel_tok_feat"])
    assert torch.equal(batch["token_bonds_feature"][tokens][:, tokens], f["token_bonds"].float())
    outside = ~(tokens[:, None] & tokens[None])
    assert torch.equal(batch["ref_feat"][~atoms], before["ref_feat"][~atoms]) and torch.equal(batch["ref_pos"][~atoms], before["ref_pos"][~atoms])
    assert torch.equal(batch["rel_tok_feat"][outside], before["rel_tok_feat"][outside])
    assert torch.equal(batch["token_bonds_feature"][outside], before["token_bonds_feature"][outside])
    for k in batch:
        if k not in ("ref_feat", "ref_pos", "rel_tok_feat", "token_bonds_feature"):
            assert torch.equal(batch[k], before[k]), k


def test_refusals_on_the_host_before_any_launch():
    with pytest.raises(ValueError, match="129"):
        Ligand.from_smiles("C" * 129)
    with pytest.raises(ValueError, match="129"):
        Ligand.from_graph([6] * 129, [(k, k + 1) for k in range(128)], [1.0] * 128)
    with pytest.raises(ValueError, match="0 ligands"):
        LigandLibrary([])
    with pytest.raises(ValueError, match="not connected"):
        Ligand.from_graph([6, 6, 8], [(0, 1)], [1.0])


def test_the_defaults_run_on_the_current_device(expected):
    lig = Ligand.from_smiles("CCO")
    got = lig.features()
    assert got["ref_feat"].is_cuda and got["ref_feat"].device.index == torch.cuda.current_device()
    _same({k: v.cpu().numpy() for k, v in got.items()}, expected["CCO"], "CCO, device=None")
    got["ref_feat"].fill_(7.0)                                                  # a caller's copy: the ligand's own result is not touched
    assert torch.equal(lig.features()["ref_feat"].cpu(), torch.from_numpy(expected["CCO"]["ref_feat"]))
    out = lig.embed_reference()
    assert out["ref_pos"].is_cuda and tuple(out["ref_pos"].shape) == (3, 3) and out["max_violation"] <= 0.1
    assert torch.equal(out["ref_feat"][:, 3:].cpu(), torch.from_numpy(expected["CCO"]["ref_feat"][:, 3:]))
    meta, label = lig.conf_meta()
    assert np.isfinite(meta["ref_feat"]).all() and np.array_equal(meta["ref_feat"][:, :3], label["x_gt"])
    lib = LigandLibrary.from_smiles(["CCO", "c1ccccc1"])
    res = lib.features()
    for g, s in enumerate(("CCO", "c1ccccc1")):
        _same({k: v.cpu().numpy() for k, v in lib.split(res, g).items()}, expected[s], s)


def test_conf_meta_is_the_reference_s_entry(expected):
    lig = Ligand.from_smiles("CCO")
    pos = np.asarray([[0.0, 0.5, 1.0], [1.5, 0.25, -1.0], [2.5, 1.0, 0.125]], dtype=np.float32)
    meta, label = lig.conf_meta(ref_pos=torch.from_numpy(pos).cuda())
    want = expected["CCO"]
    assert sorted(meta) == ["ref_atom_name_chars", "ref_element", "ref_feat", "rel_tok_feat", "token_bonds"]
    assert meta["ref_atom_name_chars"] == ["C0  ", "C1  ", "O2  "]
    assert meta["ref_feat"].shape == (3, 167) and meta["ref_feat"].dtype == np.float32 and np.array_equal(meta["ref_feat"][:, :3], pos)
    assert np.array_equal(meta["ref_feat"][:, 3:], want["ref_feat"][:, 3:])
    assert meta["rel_tok_feat"].shape == (3, 3, 42) and np.array_equal(meta["rel_tok_feat"], want["rel_tok_feat"])
    assert meta["ref_element"].dtype == np.int8 and meta["ref_element"].tolist() == [5, 5, 7] and np.array_equal(meta["ref_element"], want["ref_element"])
    assert meta["token_bonds"].dtype == np.int8 and meta["token_bonds"].tolist() == [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
    assert np.array_equal(meta["token_bonds"], want["token_bonds"])
    # the label features of get_features_from_ref_mol: one residue of class 20, the atoms in one chunk
    assert sorted(label) == ["a_mask", "atom_id_to_conformer_atom_id", "conformer_id_to_chunk_sizes", "residue_index", "restype", "x_exists", "x_gt"]
    assert label["x_gt"].dtype == np.float32 and np.array_equal(label["x_gt"], pos)
    for name, value in (("x_exists", [1, 1, 1]), ("a_mask", [1, 1, 1]), ("restype", [20]), ("residue_index", [0]),
                        ("atom_id_to_conformer_atom_id", [0, 1, 2]), ("conformer_id_to_chunk_sizes", [3])):
        assert label[name].dtype == np.int64 and label[name].tolist() == value, name
    names = Ligand.from_smiles("c1cccc(c1C#N)NC(=S)NC(=O)c2ccc(o2)-c3ccc(Br)cc3").conf_meta(ref_pos=np.zeros((26, 3)))[0]["ref_atom_name_chars"]
    assert names[0] == "C0  " and names[10] == "S10 " and names[23] == "Br23" and all(len(n) == 4 for n in names)
