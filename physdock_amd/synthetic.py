"""Synthetic feature dicts in the layout FeatureLoader.load produces.

The reference's featuriser cannot run here (missing CCD metadata), so
benches and parity tests use synthetic crops with the key set the hot path reads
(reference: diffusion_conditioning.py:38-42,67-71,111-114,169,179-184;
transformers.py:245-248; model.py:176-183) and the loader's dtypes
(feature_loader.py:278-279,377-381,620-628,789-791,982-997).

cfg1 = 224 protein tokens x 9 atoms + 32 ligand atoms (T=256, A=2048)
cfg2 = 448 x 9 + 64 (T=512, A=4096);  S = 128 MSA rows   
"""
from __future__ import annotations

import math

import torch


def make_batch(n_protein=224, atoms_per_res=9, n_ligand=32, n_msa=128, seed=0,
               dtype=torch.float32):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)

    def randn(*s):
        return torch.randn(*s, generator=g, dtype=torch.float32)

    def randint(lo, hi, s):
        return torch.randint(lo, hi, s, generator=g)

    T = n_protein + n_ligand
    A = n_protein * atoms_per_res + n_ligand
    chunk = torch.cat([torch.full((n_protein,), atoms_per_res), torch.ones(n_ligand)]).long()
    a2t = torch.repeat_interleave(torch.arange(T), chunk)

    # x_gt: 3.8 A random-walk CA trace + N(0,1.5^2) side atoms, ligand near centroid
    steps = randn(n_protein, 3)
    steps = 3.8 * steps / steps.norm(dim=-1, keepdim=True)
    ca = torch.cumsum(steps, 0)
    prot = (ca[:, None, :] + 1.5 * randn(n_protein, atoms_per_res, 3)).reshape(-1, 3)
    lig = ca.mean(0, keepdim=True) + 1.5 * randn(n_ligand, 3)
    x_gt = torch.cat([prot, lig], 0)

    # ref_pos: per-token centred conformer, randomly rotated per conformer; ligand = one conformer
    ref_pos = 1.5 * randn(A, 3)
    uid = torch.cat([a2t[: n_protein * atoms_per_res],
                     torch.full((n_ligand,), n_protein)]).long()
    for u in range(int(uid.max()) + 1):
        m = uid == u
        ref_pos[m] -= ref_pos[m].mean(0, keepdim=True)

    # ref_feat: [pos(3) | charge(1) | element one-hot(128) | aromatic(1) | 9 | 7 | 9 | 3 | 6]
    ref_feat = torch.zeros(A, 167)
    ref_feat[:, :3] = ref_pos
    ref_feat[:, 3] = (randint(0, 10, (A,)) == 0).float() * 0.5
    ref_feat[torch.arange(A), 4 + randint(0, 16, (A,))] = 1.0
    ref_feat[:, 132] = (randint(0, 4, (A,)) == 0).float()
    off = 133
    for w in (9, 7, 9, 3, 6):
        ref_feat[torch.arange(A), off + randint(0, w, (A,))] = 1.0
        off += w
    assert off == 167

    restype = torch.cat([randint(0, 20, (n_protein,)), torch.full((n_ligand,), 31)])
    target_feat = torch.zeros(T, 65)
    target_feat[torch.arange(T), restype] = 1.0
    target_feat[:, 32:64] = torch.softmax(randn(T, 32), -1)   # profile
    target_feat[:, 64] = 0.1 * torch.rand(T, generator=g)     # deletion mean

    key_res_feat = torch.zeros(T, 7)
    kr = randint(0, n_protein, (6,))
    key_res_feat[kr, randint(0, 7, (6,))] = 1.0
    pocket = torch.zeros(T)
    d_lig = (ca - lig.mean(0)).norm(dim=-1)
    pocket[:n_protein][d_lig < d_lig.kthvalue(min(24, n_protein)).values] = 1.0

    # ligand graph: random tree + a few ring closures -> rel_tok_feat block & token bonds
    rel_tok = torch.zeros(T, T, 42)
    bonds = torch.zeros(T, T)
    if n_ligand > 1:
        adj = torch.zeros(n_ligand, n_ligand, dtype=torch.bool)
        for i in range(1, n_ligand):
            j = int(randint(max(0, i - 4), i, (1,)))
            adj[i, j] = adj[j, i] = True
        for _ in range(max(1, n_ligand // 10)):
            i, j = [int(v) for v in randint(0, n_ligand, (2,))]
            if i != j:
                adj[i, j] = adj[j, i] = True
        dist = torch.full((n_ligand, n_ligand), 30.0)
        dist[adj] = 1.0
        dist.fill_diagonal_(0.0)
        for k in range(n_ligand):  # Floyd-Warshall on a small graph
            dist = torch.minimum(dist, dist[:, k:k + 1] + dist[k:k + 1, :])
        dist = dist.clamp(max=30).long()
        blk = torch.zeros(n_ligand, n_ligand, 42)
        blk.scatter_(-1, dist[..., None], 1.0)                       # one-hot32 graph distance
        btype = randint(0, 5, (n_ligand, n_ligand))
        btype = torch.triu(btype, 1)
        btype = btype + btype.T
        oh = torch.zeros(n_ligand, n_ligand, 5).scatter_(-1, btype[..., None], 1.0)
        blk[..., 32:37] = oh * adj[..., None]
        blk[..., 37] = adj.float()
        blk[..., 38] = adj.float() * (1 + (btype == 2).float())
        ring = (randint(0, 3, (n_ligand,)) == 0).float()
        blk[..., 39] = adj.float() * ring[:, None] * ring[None, :]
        blk[..., 40] = adj.float() * (btype == 3).float()
        blk[..., 41] = blk[..., 39] * (btype == 4).float()
        rel_tok[n_protein:, n_protein:] = blk
        bonds[n_protein:, n_protein:] = adj.float()

    msa = torch.zeros(n_msa, T, 34)
    aa = randint(0, 32, (n_msa, T))
    aa[0] = restype
    msa.scatter_(-1, aa[..., None], 1.0)
    msa[..., 32] = (randint(0, 8, (n_msa, T)) == 0).float()
    msa[..., 33] = msa[..., 32] * torch.rand(n_msa, T, generator=g)

    # template: 39-bin distogram of pseudo-beta + mask, protein-protein only
    cb = torch.cat([ca, lig], 0)
    dm = (cb[:, None] - cb[None]).norm(dim=-1)
    edges = torch.linspace(3.25, 50.75, 39)
    lower = edges ** 2
    upper = torch.cat([lower[1:], torch.tensor([1e8])])
    dgram = ((dm[..., None] ** 2 > lower) & (dm[..., None] ** 2 < upper)).float()
    prot2d = torch.zeros(T, T)
    prot2d[:n_protein, :n_protein] = 1.0
    templ = torch.cat([dgram * prot2d[..., None], prot2d[..., None]], -1)

    asym = torch.cat([torch.zeros(n_protein), torch.ones(n_ligand)]).int()
    batch = {
        "ref_feat": ref_feat, "ref_pos": ref_pos, "ref_space_uid": uid,
        "a_mask": torch.ones(A), "ap_mask": torch.ones(A, A),
        "atom_id_to_token_id": a2t, "token_id_to_chunk_sizes": chunk,
        "target_feat": target_feat, "key_res_feat": key_res_feat, "pocket_res_feat": pocket,
        "token_bonds_feature": bonds, "rel_tok_feat": rel_tok, "msa_feat": msa,
        "templ_feat": templ, "t_mask": torch.tensor(1.0), "z_mask": torch.ones(T, T),
        "asym_id": asym, "sym_id": torch.zeros(T).int(), "entity_id": asym.clone(),
        "residue_index": torch.cat([torch.arange(n_protein), torch.arange(n_ligand)]).long(),
        "is_ligand": torch.cat([torch.zeros(n_protein), torch.ones(n_ligand)]),
        "x_gt": x_gt, "x_exists": torch.ones(A),
    }
    for k, v in batch.items():
        if v.is_floating_point():
            batch[k] = v.to(dtype)
    return batch


def cfg1_batch(seed=0):
    return make_batch(224, 9, 32, 128, seed)


def cfg2_batch(seed=0):
    return make_batch(448, 9, 64, 128, seed)


def system(n_protein=224, atoms_per_res=9, n_ligand=32, n_msa=128, seed=0, n_conf=40):
    """One synthetic docking SYSTEM as the drivers see it (redocking.py:156-232 / screening.py:100-116 after featurisation):
    the feature dict, reference conformers of its ligand, and the loader's naming tables for PDB output.  Different
    (n_protein, n_ligand) give different - generally ragged - token / atom counts."""
    batch = make_batch(n_protein, atoms_per_res, n_ligand, n_msa, seed)
    meta = pdb_meta({k: batch[k].numpy() for k in ("token_id_to_chunk_sizes", "asym_id", "is_ligand", "residue_index")}, seed=seed)
    return {"batch": batch, "ref_mol_poses": reference_conformers(batch, n_conf=n_conf, seed=seed + 1), "infer_meta_data": meta,
            "name": f"syn_p{n_protein}_l{n_ligand}_s{seed}"}


def small_batch(seed=0):
    """T=24 (20 protein x 4 atoms... ) sized for the committed fixtures: T=24, A=96, S=8."""
    return make_batch(18, 5, 6, 8, seed)


def reference_conformers(batch, n_conf=8, seed=1):
    """Synthetic stand-in for RDKit ETKDG conformers: jittered, randomly rotated copies of the ligand."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    lig = batch["is_ligand"][batch["atom_id_to_token_id"]].bool()
    x = batch["x_gt"][lig]
    x = x - x.mean(0, keepdim=True)
    out = []
    for _ in range(n_conf):
        q = torch.randn(4, generator=g)
        q = q / q.norm()
        w, a, b, c = q.tolist()
        R = torch.tensor([[1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)],
                          [2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)],
                          [2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)]])
        out.append((x + 0.3 * torch.randn(x.shape, generator=g)) @ R.T)
    return torch.stack(out, 0).to(batch["x_gt"].dtype)


def toy_relax_fn(ref_mol, ligand_pos, mmff_iters=5):
    """Deterministic stand-in for the reference's `get_next_step_pos(ref_mol, pos, mmff_iters)` (model.py:26-52) used by
    the parity fixtures: pulls every sample's ligand a fixed fraction towards a target conformer placed at the sample's
    own centroid.  Pure torch, so the identical function can be patched into the reference (tools/make_golden.py G8/G9),
    the oracle and the HIP path (`relax_fn=`).  `ref_mol` is the dict {"conf": [L,3]} the fixtures pass as the molecule."""
    tgt = ref_mol["conf"].to(ligand_pos.device, ligand_pos.dtype)
    tgt = tgt - tgt.mean(0, keepdim=True)
    centre = ligand_pos.mean(1, keepdim=True)
    return ligand_pos + (0.02 * mmff_iters) * (tgt[None] + centre - ligand_pos)


def confidence_inputs(batch, c_s, c_z, seed=5, n_pose=2):
    """Inputs of ConfidenceModule.forward (reference confidence_module.py:56-66) for a synthetic batch: the centre atom of
    every token (its first atom), trunk-like s / z activations and `n_pose` predicted poses around x_gt.  Seeded on the CPU
    generator so that tools/make_golden.py (reference side) and the tests (HIP / oracle side) build identical tensors."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    T, A = batch["target_feat"].shape[0], batch["ref_pos"].shape[0]
    chunk = batch["token_id_to_chunk_sizes"].long()
    centre = torch.cumsum(chunk, 0) - chunk
    s = torch.randn(T, c_s, generator=g)
    z = torch.randn(T, T, c_z, generator=g)
    x_pred = batch["x_gt"].float()[None] + 0.5 * torch.randn(n_pose, A, 3, generator=g)
    return {"token_id_to_centre_atom_id": centre, "s": s, "z": z, "x_pred": x_pred}


def raw_features(seed=0, n_res=(14, 9), n_lig=(7, 5), n_msa=24, atoms_per_res=5):
    """Synthetic *raw* (pre-`FeatureLoader.transform`, reference feature_loader.py:970-998) features of a small complex:
    two protein chains and two ligand chains (one token per ligand atom), numpy arrays in the loader's layout.  Built so that
    the inter-chain token-bond search (feature_loader.py:853-911) meets every case: ligand 0 has an atom 1.9 A from a protein
    atom (bond), ligand 1 sits 2.1 A from ligand 0 (ligand-ligand bond) and far from the proteins, the two protein chains
    touch at 1.5 A (protein-protein pairs are skipped), and the closest protein-ligand atom pair of all is masked out."""
    import numpy as np
    rng = np.random.default_rng(seed)
    chunks, asym, is_prot, is_lig = [], [], [], []
    for c, n in enumerate(n_res):
        chunks += [atoms_per_res] * n
        asym += [c] * n
        is_prot += [1.0] * n
        is_lig += [0.0] * n
    for c, n in enumerate(n_lig):
        chunks += [1] * n
        asym += [len(n_res) + c] * n
        is_prot += [0.0] * n
        is_lig += [1.0] * n
    chunks = np.asarray(chunks, dtype=np.int64)
    T, A = len(chunks), int(chunks.sum())
    a2t = np.repeat(np.arange(T), chunks)
    asym = np.asarray(asym, dtype=np.int32)
    atom_asym = asym[a2t]
    x = np.zeros((A, 3), dtype=np.float32)
    origin = {0: (0, 0, 0), 1: (40, 0, 0), 2: (0, 30, 0), 3: (0, 30, 25)}
    for c in range(len(n_res) + len(n_lig)):
        m = atom_asym == c
        walk = np.cumsum(rng.normal(0, 1.6, size=(int(m.sum()), 3)), axis=0)
        x[m] = (walk - walk.mean(0) + np.asarray(origin.get(c, (20 * c, 50, 0)), dtype=np.float64)).astype(np.float32)
    first = {c: int(np.argmax(atom_asym == c)) for c in range(len(n_res) + len(n_lig))}
    p0, p1, l0, l1 = first[0], first[1], first[2], first[3]
    x[l0 + 2] = x[p0 + 7] + np.float32([1.9, 0, 0])           # protein 0 - ligand 0 contact -> token bond
    x[l1 + 1] = x[l0 + 4] + np.float32([0, 2.1, 0])           # ligand 0 - ligand 1 contact -> token bond
    x[p1 + 3] = x[p0 + 11] + np.float32([0, 0, 1.5])          # protein - protein contact: never searched
    x[l0 + 5] = x[p1 + 9] + np.float32([0.4, 0, 0])           # would be the closest pair (protein 1 - ligand 0) ...
    a_mask = np.ones(A, dtype=np.float32)
    a_mask[p1 + 9] = 0.0                                      # ... but the protein atom is unresolved; next best is > 2.4 A
    s_mask = np.ones(T, dtype=np.float32)
    s_mask[3] = 0.0
    restype = np.where(np.asarray(is_prot) > 0, rng.integers(0, 20, T), 20 + rng.integers(0, 12, T)).astype(np.int64)
    profile = rng.random((T, 32)).astype(np.float32)
    profile /= profile.sum(-1, keepdims=True)
    msa = rng.integers(0, 32, (n_msa, T)).astype(np.int64)
    msa[0] = restype
    deletion = np.where(rng.random((n_msa, T)) < 0.15, rng.integers(1, 9, (n_msa, T)), 0).astype(np.float32)
    tb = np.zeros((T, T), dtype=np.float32)
    lig_tok = np.nonzero(np.asarray(is_lig) > 0)[0]
    for i, j in zip(lig_tok[:-1], lig_tok[1:]):
        if asym[i] == asym[j]:
            tb[i, j] = tb[j, i] = 1.0                         # within-conformer bonds already present before the search
    is_short = np.zeros(T, dtype=np.float32)
    is_short[lig_tok[-2:]] = 1.0                              # last ligand chain's tail flagged as short polymer
    pb = (np.cumsum(chunks) - chunks + np.minimum(1, chunks - 1)).astype(np.int64)
    return {
        "restype": restype, "profile": profile, "deletion_mean": deletion.mean(0).astype(np.float32), "msa": msa,
        "deletion_matrix": deletion, "asym_id": asym, "atom_id_to_token_id": a2t.astype(np.int64),
        "is_ligand": np.asarray(is_lig, dtype=np.float32), "is_protein": np.asarray(is_prot, dtype=np.float32),
        "is_short_poly": is_short, "x_gt": x, "a_mask": a_mask, "s_mask": s_mask, "token_bonds": tb,
        "token_id_to_pseudo_beta_atom_id": pb, "token_id_to_chunk_sizes": chunks,
        "residue_index": np.concatenate([np.arange(n) for n in n_res] + [np.zeros(n, dtype=np.int64) for n in n_lig]).astype(np.int64),
    }


def pdb_meta(raw, seed=0):
    """`infer_meta_data` of FeatureLoader.write_pdb_block (reference feature_loader.py:1230-1283) for `raw_features`: one
    conformer per protein residue and one per ligand chain, atom names of 2-4 characters, two-letter elements."""
    import numpy as np
    rng = np.random.default_rng(seed)
    chunks, asym = raw["token_id_to_chunk_sizes"], raw["asym_id"]
    is_lig = raw["is_ligand"] > 0
    res3 = ["ALA", "GLY", "SER", "LEU", "LYS", "ASP", "PHE", "HIS"]
    ccds, conf_chunks, chain_class, res_index, conf_asym = [], [], [], [], []
    meta = {}
    t = 0
    T = len(chunks)
    while t < T:
        if not is_lig[t]:
            ccd = res3[int(rng.integers(0, len(res3)))]
            n = int(chunks[t])
            ccds.append(ccd); conf_chunks.append(n); chain_class.append("protein")
            res_index.append(int(raw["residue_index"][t])); conf_asym.append(int(asym[t]))
            if ccd not in meta:
                names = ["N", "CA", "C", "O", "CB", "CG", "HD11", "OXT", "CD", "CE", "NZ", "OG", "SD", "HE21"]
                meta[ccd] = {"ref_atom_name_chars": names, "ref_element": [6, 5, 5, 7, 5, 5, 0, 7, 5, 5, 6, 7, 15, 0]}
            t += 1
        else:
            c = asym[t]
            n = int((asym == c).sum())
            ccd = f"L{int(c):02d}X" if c % 2 else "7Z4"     # a 4-character id (only its last three are printed) and a 3-character one
            ccds.append(ccd); conf_chunks.append(n); chain_class.append("ligand")
            res_index.append(0); conf_asym.append(int(c))
            meta[ccd] = {"ref_atom_name_chars": [f"C{i + 1}" if i % 3 else f"CL{i + 1}" for i in range(n)],
                         "ref_element": [5 if i % 3 else 16 for i in range(n)]}
            t += n
    inner = np.concatenate([np.arange(n) if cls == "ligand" else rng.permutation(max(n, 8))[:n]
                            for n, cls in zip(conf_chunks, chain_class)]).astype(np.int64)
    return {"ccds": ccds, "atom_id_to_conformer_atom_id": inner, "conformer_id_to_chunk_sizes": np.asarray(conf_chunks),
            "CHAIN_CLASS": chain_class, "CONF_META_DATA": meta, "residue_index": np.asarray(res_index),
            "asym_id": np.asarray(conf_asym)}


def replay_draws(seed, B, steps, A, n_noisy):
    """The reference sampler's random draws for (B samples, `steps` steps, the first n_noisy of them with noise injection),
    regenerated from torch's global CPU generator in the reference's call order (model.py:148, tensor_utils.py:549-557,582,
    model.py:77): initial noise, then per step four uniform vectors (rotation), the translation, and - noisy steps only - the
    diffusion noise.  Lets a fixture store a seed instead of megabytes of draws (tools/make_golden.py checks the replay against
    the recorded draws bit for bit)."""
    state = torch.get_rng_state()
    try:
        torch.manual_seed(seed)
        init = torch.normal(mean=0, std=1, size=(B, A, 3), dtype=torch.float32)
        rot, trans, dif = [], [], []
        for i in range(steps):
            rot.append(torch.stack([torch.rand([B], dtype=torch.float32) for _ in range(4)]))
            trans.append(torch.normal(mean=0, std=1, size=(B, 3), dtype=torch.float32))
            if i < n_noisy:
                dif.append(torch.normal(mean=0, std=1, size=(B, A, 3), dtype=torch.float32))
    finally:
        torch.set_rng_state(state)
    return {"init": init, "rot_u": torch.stack(rot), "trans": torch.stack(trans),
            "diffuse": torch.stack(dif) if dif else torch.zeros(0, B, A, 3)}


def loss_features(batch, seed=0, n_dna=0, n_rna=0, n_key=6, masked_atoms=(), bonds=True):
    """The reference's loss features (models/loss.py keyword names) that `make_batch` does not carry, derived from a batch:
    centre / pseudo-beta atom of every token (second / fifth atom of a residue, the atom itself for one-atom tokens), token
    bonds (the ligand graph), DNA / RNA flags on the first protein tokens, `n_key` key residues, and `x_exists` with the
    atoms `masked_atoms` switched off.  Returns a new dict: the batch plus these keys."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    chunk = batch["token_id_to_chunk_sizes"].long()
    T = chunk.shape[0]
    start = torch.cumsum(chunk, 0) - chunk
    is_lig = batch["is_ligand"].float()
    n_prot = int((is_lig == 0).sum())
    out = dict(batch)
    out["token_id_to_centre_atom_id"] = start + torch.clamp(chunk - 1, max=1)
    out["token_id_to_pseudo_beta_atom_id"] = start + torch.clamp(chunk - 1, max=4)
    out["token_bonds"] = batch["token_bonds_feature"].float().clone() if bonds else torch.zeros(T, T)
    is_dna, is_rna = torch.zeros(T), torch.zeros(T)
    is_dna[:n_dna] = 1.0
    is_rna[n_dna:n_dna + n_rna] = 1.0
    out["is_dna"], out["is_rna"] = is_dna, is_rna
    key = torch.zeros(T)
    if n_key:
        key[torch.randperm(n_prot, generator=g)[:n_key]] = 1.0
    out["is_key_res"] = key
    ex = torch.ones(batch["x_gt"].shape[0])
    for a in masked_atoms:
        ex[a] = 0.0
    out["x_exists"] = ex
    return out


def hashed_uniform(n, seed):
    """n float32 values in (-0.5, 0.5) from a counter hash (splitmix64) in integer arithmetic only: the same bits on every
    machine and library version, which a seeded normal draw (log / cos inside) is not.  The loss fixtures store checksums of
    arrays too large to commit and rebuild them from this."""
    import numpy as np
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(seed + 1) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24) - np.float32(0.5)


def loss_outputs(feats, B, seed=0, t_hat=None):
    """Stand-in for the `outputs` of `PhysDock.forward` at B samples: per-sample noise levels t_hat drawn as the reference draws
    them (model.py:87-97) unless given, x_denoised = x_gt + 0.1 t_hat u with u uniform of unit variance, symmetric uniform
    distogram logits in (-4, 4).  Given t_hat and x_gt, the result is bit-identical everywhere (hashed_uniform)."""
    import numpy as np
    A, T = feats["x_gt"].shape[0], feats["is_ligand"].shape[0]
    if t_hat is None:
        g = torch.Generator(device="cpu")
        g.manual_seed(seed)
        t_hat = torch.exp(torch.randn(B, generator=g) * 1.5 - 1.2) * 16.0
    t_hat = t_hat.float()
    u = torch.from_numpy(hashed_uniform(B * A * 3, 2 * seed).reshape(B, A, 3)) * np.float32(3.4641016)
    xd = feats["x_gt"].float()[None] + u * (t_hat * np.float32(0.1))[:, None, None]
    pd = torch.from_numpy(hashed_uniform(T * T * 39, 2 * seed + 1).reshape(T, T, 39)) * np.float32(4.0)
    return {"x_denoised": xd, "t_hat": t_hat, "p_distogram": pd + pd.transpose(0, 1)}


LOSS_FEAT_KEYS = ("x_gt", "x_exists", "atom_id_to_token_id", "token_id_to_centre_atom_id", "token_id_to_pseudo_beta_atom_id",
                  "token_bonds", "is_dna", "is_rna", "is_ligand", "is_key_res")
LOSS_OUT_KEYS = ("x_denoised", "t_hat", "p_distogram")


def clear_thresholds(feats, clamp=15.0, min_bin=3.25, max_bin=50.75, no_bins=39, margin=3e-5, seed=0):
    """Nudge (by ~0.01 A, seeded) the few atoms of x_gt that form a pair within a relative `margin` of a decision threshold of
    the loss - the smooth-lDDT clamp on the distance, a distogram bin edge on the squared pseudo-beta distance - until no such
    pair is left: among 4e6 pairs a few always are, and two fp32 implementations may put them on either side."""
    import numpy as np
    rng = np.random.RandomState(seed)
    x = feats["x_gt"].numpy().astype(np.float32).copy()
    pb = feats["token_id_to_pseudo_beta_atom_id"].numpy()
    b2 = np.linspace(min_bin, max_bin, no_bins - 1) ** 2
    for _ in range(200):
        x64 = x.astype(np.float64)
        d = np.sqrt(((x64[:, None] - x64[None]) ** 2).sum(-1))
        bad = set(np.nonzero(np.abs(d - clamp) < margin * clamp)[1].tolist())
        d2 = ((x64[pb][:, None] - x64[pb][None]) ** 2).sum(-1)
        bad |= set(pb[np.nonzero((np.abs(d2[..., None] - b2) < margin * b2).any(-1))[1]].tolist())
        if not bad:
            out = dict(feats)
            out["x_gt"] = torch.from_numpy(x)
            return out
        for a in sorted(bad):
            x[a] += (0.01 * rng.randn(3)).astype(np.float32)
    raise RuntimeError("could not clear the decision thresholds")


def loss_case(name, B_cfg1=48, stored=None):
    """(outputs, feats, note) of the loss fixture tests/golden/g15_loss_<name>.npz (tools/make_golden_loss.py).  A fixture
    stores its features and t_hat and, where they fit, the other outputs; with `stored` (the loaded fixture) the arrays too
    large to commit ([48, 2048, 3], [T, T, 39]) are rebuilt from the stored ones, bit for bit (loss_outputs)."""
    if stored is not None:
        f = {k: torch.from_numpy(stored[k]) for k in LOSS_FEAT_KEYS}
        seed = {"small": 2, "ragged": 5, "cfg1": 7, "degenerate": 10, "nan": 13}[name]
        o = loss_outputs(f, int(stored["t_hat"].shape[0]), seed=seed, t_hat=torch.from_numpy(stored["t_hat"]))
        o = {k: (torch.from_numpy(stored[k]) if k in stored else o[k]) for k in LOSS_OUT_KEYS}
        return o, f, str(stored["note"])
    note = ""
    if name == "small":             # the small test configuration's shape (T = 24, A = 96)
        f = loss_features(make_batch(18, 5, 6, 8, seed=0), seed=1, n_dna=2, n_rna=2, n_key=4, masked_atoms=(7,))
        o = loss_outputs(f, 4, seed=2)
    elif name == "ragged":          # T = 221, A = 1805: multiples of no tile size
        f = clear_thresholds(loss_features(make_batch(198, 9, 23, 8, seed=3), seed=4, n_dna=5, n_rna=7, n_key=6, masked_atoms=(11, 900)))
        assert f["x_gt"].shape[0] == 1805 and f["is_ligand"].shape[0] == 221
        o = loss_outputs(f, 5, seed=5)
    elif name == "cfg1":            # T = 256, A = 2048
        f = clear_thresholds(loss_features(make_batch(224, 9, 32, 8, seed=0), seed=6, n_dna=0, n_rna=0, n_key=6))
        o = loss_outputs(f, B_cfg1, seed=7)
        note = f"B = {B_cfg1}"
    elif name == "degenerate":      # no token bonds, no key residues: the eps denominators
        f = loss_features(make_batch(18, 5, 6, 8, seed=8), seed=9, n_key=0, bonds=False)
        o = loss_outputs(f, 4, seed=10)
    elif name == "nan":             # a NaN in one sample: the reference's skip-and-warn path
        f = loss_features(make_batch(18, 5, 6, 8, seed=11), seed=12, n_dna=2, n_rna=2, n_key=4)
        o = loss_outputs(f, 4, seed=13)
        o["x_denoised"][2, int(f["token_id_to_centre_atom_id"][-1]), 1] = float("nan")
        note = ("x_denoised[2, centre atom of the last (ligand) token, 1] = NaN.  On the CPU the reference's weighted_mse_loss raises "
                "(torch.linalg.svd refuses the non-finite matrix) - recorded as NaN with ref_raised set - and PhysDockLoss with it; "
                "ref_loss is the weighted sum of the terms the reference does return as finite")
    else:
        raise ValueError(name)
    f = {k: f[k] for k in LOSS_FEAT_KEYS}
    o = {k: o[k] for k in LOSS_OUT_KEYS}
    return o, f, note


CONF_FEAT_KEYS = ("x_gt", "x_exists", "token_id_to_centre_atom_id", "is_dna", "is_rna", "is_ligand", "token_id_to_frame_atom_id_0",
                  "token_id_to_frame_atom_id_1", "token_id_to_frame_atom_id_2")
CONF_OUT_KEYS = ("p_plddt", "p_pde", "p_pae", "x_pred")
CONF_SEEDS = {"small": 21, "mid": 23, "ragged": 25, "empty": 27}
#: margins of the decision thresholds of the confidence losses (Angstrom; cos theta of a frame; |w1 + w2| of a frame)
CONF_MARGIN, CONF_COS_MARGIN, CONF_MIN_BISECTOR = 1e-4, 1e-5, 0.1


def frame_atom_ids(feats):
    """token_id_to_frame_atom_id_{0,1,2}: atoms 0, 1, 2 of a residue token; previous / self / next atom of a one-atom (ligand)
    token (the last atom takes the one before the previous).  The reference's loader never makes them."""
    chunk = feats["token_id_to_chunk_sizes"].long()
    start = torch.cumsum(chunk, 0) - chunk
    A = int(chunk.sum())
    one = chunk < 3
    nxt = torch.where(start + 1 < A, start + 1, start - 2)
    return (torch.where(one, start - 1, start), torch.where(one, start, start + 1), torch.where(one, nxt, start + 2))


def confidence_frames64(x, ids):
    """express_coordinates_in_frame (reference loss.py:184-207) in float64: e1, e2, e3 [T,3] each, origin b, cos theta, |w1 + w2|"""
    import numpy as np
    a, b, c = x[ids[0]], x[ids[1]], x[ids[2]]
    w1 = (a - b) / np.linalg.norm(a - b + 1e-6, axis=-1, keepdims=True)
    w2 = (c - b) / np.linalg.norm(c - b + 1e-6, axis=-1, keepdims=True)
    e1 = (w1 + w2) / np.linalg.norm(w1 + w2 + 1e-6, axis=-1, keepdims=True)
    e2 = (w2 - w1) / np.linalg.norm(w2 - w1 + 1e-6, axis=-1, keepdims=True)
    return e1, e2, np.cross(e1, e2), b, (w1 * w2).sum(-1), np.linalg.norm(w1 + w2, axis=-1)


def confidence_decisions64(xp, xg, feats, no_bins_plddt=50, step=0.5):
    """Every hard decision of the confidence losses in float64 (numpy), with the distance of its argument to the nearest
    threshold.  Returns a dict: `d_gt` [A,T], `d_lm` [B,A,T], `include` [A,T] weights, `e_pde`, `e_pae` [T,T] of pose 0,
    `cos` [2,T] (pose 0, x_gt), `bisector` [2,T], `num`, `den` [B,A] of the lDDT ratio."""
    import numpy as np
    xp, xg = np.asarray(xp, np.float64), np.asarray(xg, np.float64)
    c = np.asarray(feats["token_id_to_centre_atom_id"])
    ids = [np.asarray(feats[f"token_id_to_frame_atom_id_{k}"]) for k in range(3)]
    nuc = (np.asarray(feats["is_dna"], np.float64) + np.asarray(feats["is_rna"], np.float64))[None]
    poly = (np.asarray(feats["is_ligand"]) == 0).astype(np.float64)[None]
    d_gt = np.linalg.norm(xg[:, None] - xg[c][None], axis=-1)
    d_pred = np.linalg.norm(xp[:, :, None] - xp[:, c][:, None], axis=-1)
    d_lm = np.abs(d_pred - d_gt[None])
    w = ((d_gt < 30) * nuc + (d_gt < 15) * (1 - nuc)) * poly
    score = 0.25 * sum((d_lm < t).astype(np.float64) for t in (0.5, 1.0, 2.0, 4.0))
    out = {"d_gt": d_gt, "d_lm": d_lm, "include": w, "num": (w[None] * score).sum(-1), "den": np.broadcast_to(w.sum(-1), d_lm.shape[:2])}
    out["e_pde"] = d_lm[0][c]
    fr = [confidence_frames64(x, ids) for x in (xp[0], xg)]
    u = [np.einsum("kti,tji->tjk", np.stack(f[:3]), x[c][None] - f[3][:, None]) for f, x in zip(fr, (xp[0], xg))]
    valid = [(f[4] < 0.906308) for f in fr]
    out["e_pae"] = np.linalg.norm(u[0] - u[1], axis=-1) * (valid[0] & valid[1])[:, None]
    out["cos"], out["bisector"] = np.stack([f[4] for f in fr]), np.stack([f[5] for f in fr])
    return out


def lddt_bins32(num, den, no_bins):
    """clamp(long(lddt * no_bins), 0, no_bins - 1) as the reference's fp32 expression evaluates it on the exact sums num, den (both
    are sums of multiples of 0.25, exact in fp32 in any order): one IEEE fp32 division, one fp32 product, truncation; NaN -> 0"""
    import numpy as np
    with np.errstate(invalid="ignore", divide="ignore"):
        v = (np.asarray(num, np.float32) / np.asarray(den, np.float32)) * np.float32(no_bins)
    return np.where(np.isnan(v), 0, np.clip(np.nan_to_num(v, nan=0.0), 0, no_bins - 1)).astype(np.int64)


def confidence_closest(dec, no_bins_plddt=50, step=0.5):
    """closest approaches of a confidence case to its decision thresholds, and the atoms to nudge for those inside the margins:
    (dict of distances, set of atoms of x_gt)"""
    import numpy as np
    def to_grid(e):
        return np.abs(e - np.round(e / step) * step)
    d_gt, d_lm = dec["d_gt"], dec["d_lm"]
    near = {"d_gt": np.minimum(np.abs(d_gt - 15.0), np.abs(d_gt - 30.0)),
            "d_lm": np.min([np.abs(d_lm - t) for t in (0.5, 1.0, 2.0, 4.0)], axis=0).min(0),
            "e_pde": to_grid(dec["e_pde"]), "e_pae": to_grid(dec["e_pae"])}
    # zero errors (the diagonal, invalid frames) are exact zeros in every implementation, not near a threshold
    near["e_pde"] = np.where(dec["e_pde"] == 0, np.inf, near["e_pde"])
    near["e_pae"] = np.where(dec["e_pae"] == 0, np.inf, near["e_pae"])
    cos = np.abs(dec["cos"] - 0.906308)
    # lddt * no_bins on an integer although the ratio is not a dyadic rational: fp32 and float64 may truncate it differently
    with np.errstate(invalid="ignore", divide="ignore"):
        q = dec["num"] / dec["den"]
        v = q * no_bins_plddt
        tie = (np.abs(v - np.round(v)) < 1e-9) & (q.astype(np.float32).astype(np.float64) != q)
    close = {"closest_d_gt": float(near["d_gt"].min()), "closest_d_lm": float(near["d_lm"].min()),
             "closest_e_pde": float(near["e_pde"].min()), "closest_e_pae": float(near["e_pae"].min()),
             "closest_cos": float(cos.min()), "smallest_bisector": float(dec["bisector"].min()), "lddt_integer_ties": int(tie.sum())}
    return close, near, cos, tie


def clear_confidence_thresholds(x_gt, noise, feats, seed=0, rounds=500):
    """Nudge (0.01 A, seeded) atoms of x_gt until no decision of the confidence losses of (x_pred = x_gt + noise, x_gt) lies
    within CONF_MARGIN of a threshold in float64 (confidence_closest).  The non-centre atom of an offending atom-centre pair is
    moved: that redraws T pairs, a centre A + T.  Integer ties of lddt * no_bins are counted, not cleared: a 0.01 A nudge does
    not move a ratio of counts, and the tie is decided by the fp32 expression on exact operands (lddt_bins32), the same bits in
    every IEEE implementation.  Returns (x_gt, x_pred, closest approaches, rounds used)."""
    import numpy as np
    rng = np.random.RandomState(seed)
    x = np.asarray(x_gt, np.float32).copy()
    c = np.asarray(feats["token_id_to_centre_atom_id"])
    ids = [np.asarray(feats[f"token_id_to_frame_atom_id_{k}"]) for k in range(3)]
    is_centre = np.zeros(x.shape[0], bool)
    is_centre[c] = True
    for r in range(rounds):
        xp = x[None] + noise
        dec = confidence_decisions64(xp, x, feats)
        close, near, cos, tie = confidence_closest(dec)
        bad = set()
        m = (near["d_gt"] < CONF_MARGIN) | (near["d_lm"] < CONF_MARGIN)
        for a, t in zip(*np.nonzero(m)):
            bad.add(int(c[t]) if (is_centre[a] and not is_centre[c[t]]) else int(a))
        for k in ("e_pde", "e_pae"):
            bad |= set(c[np.nonzero(near[k] < CONF_MARGIN)[1]].tolist())
        fbad = (cos < CONF_COS_MARGIN).any(0) | (dec["bisector"] < CONF_MIN_BISECTOR).any(0)
        bad |= set(ids[0][fbad].tolist())
        if not bad:
            return x, xp.astype(np.float32), close, r
        for a in sorted(bad):
            x[a] += (0.01 * rng.randn(3)).astype(np.float32)
    raise RuntimeError("could not clear the decision thresholds of the confidence losses")


def confidence_logits(A, T, seed, bins_plddt=50, bins_pair=64):
    """hashed-uniform logits in (-4, 4): p_plddt [A,bins], p_pde, p_pae [T,T,bins] (bit-identical everywhere)"""
    import numpy as np
    mk = lambda n, s, shape: torch.from_numpy(hashed_uniform(n, s).reshape(shape)) * np.float32(8.0)
    return {"p_plddt": mk(A * bins_plddt, 3 * seed, (A, bins_plddt)), "p_pde": mk(T * T * bins_pair, 3 * seed + 1, (T, T, bins_pair)),
            "p_pae": mk(T * T * bins_pair, 3 * seed + 2, (T, T, bins_pair))}


def confidence_loss_case(name, stored=None):
    """(outputs, feats, info) of the confidence-loss fixture tests/golden/g17_conf_loss_<name>.npz
    (tools/make_golden_confidence_loss.py).  outputs: p_plddt [A,50], p_pde, p_pae [T,T,64] (hashed uniform in (-4, 4)) and
    x_pred [B,A,3] = x_gt + 0.6 u (u uniform of unit variance); feats: CONF_FEAT_KEYS.  A fixture stores feats and x_pred; with
    `stored` (the loaded fixture) the logits are rebuilt bit for bit.  Without it the case is built and its decision thresholds
    cleared (clear_confidence_thresholds); info then holds the closest approaches."""
    import numpy as np
    seed = CONF_SEEDS[name]
    if stored is not None:
        f = {k: torch.from_numpy(np.asarray(stored[k])) for k in CONF_FEAT_KEYS}
        A, T = f["x_gt"].shape[0], f["is_ligand"].shape[0]
        return {**confidence_logits(A, T, seed), "x_pred": torch.from_numpy(np.asarray(stored["x_pred"]))}, f, {}
    # the first masked atom is the centre atom of token 1, so that token pairs are masked too, not only an atom
    shape, B, kw = {"small": ((18, 5, 6, 8), 3, dict(n_dna=2, n_rna=2, masked_atoms=(6,))),
                    "empty": ((18, 5, 6, 8), 3, dict(n_dna=2, n_rna=2, masked_atoms=(6,))),
                    "mid": ((61, 7, 10, 8), 2, dict(n_dna=3, n_rna=3, masked_atoms=(8, 200))),
                    "ragged": ((198, 9, 23, 8), 2, dict(n_dna=5, n_rna=7, masked_atoms=(10, 900)))}[name]
    f = loss_features(make_batch(*shape, seed=seed), seed=seed + 1, n_key=0, **kw)
    for k, v in enumerate(frame_atom_ids(f)):
        f[f"token_id_to_frame_atom_id_{k}"] = v
    f = {k: f[k] for k in CONF_FEAT_KEYS}
    A, T = f["x_gt"].shape[0], f["is_ligand"].shape[0]
    x = f["x_gt"].numpy().astype(np.float32).copy()
    if name == "empty":            # the last ligand atom far from every polymer centre: empty inclusion set, lDDT = 0 / 0
        x[A - 1] += np.float32(200.0)
    noise = hashed_uniform(B * A * 3, 3 * seed + 7).reshape(B, A, 3) * np.float32(3.4641016) * np.float32(0.6)
    fn = {k: v.numpy() for k, v in f.items()}
    x, xp, close, used = clear_confidence_thresholds(x, noise, fn, seed=seed)
    f["x_gt"] = torch.from_numpy(x)
    return {**confidence_logits(A, T, seed), "x_pred": torch.from_numpy(xp)}, f, {**close, "rounds": used, "make_batch": shape, "B": B}


# ------------------------------------------------------------------ get_metrics fixtures (tests/golden/g18_metrics_*.npz)
METRICS_FEAT_KEYS = ("s_mask", "asym_id", "a_mask", "atom_id_to_token_id", "is_ligand")
METRICS_CASES = ("small", "frac", "onechain", "chains3", "clash", "mid")
METRICS_SEEDS = {"small": 31, "frac": 33, "onechain": 35, "chains3": 37, "clash": 39, "mid": 41}
#: chains of a case: (tokens, atoms per token (cycled), is_ligand, asym_id).  asym ids are not dense on purpose.
METRICS_LAYOUT = {
    "small": [(10, (2, 3, 4), 0, 3), (9, (2, 3, 4), 0, 5), (5, (1,), 1, 9)],
    "frac": [(10, (2, 3, 4), 0, 3), (9, (2, 3, 4), 0, 5), (5, (1,), 1, 9)],
    "onechain": [(19, (2, 3, 4), 0, 7), (5, (1,), 1, 7)],
    "chains3": [(6, (3, 4), 0, 2), (6, (3, 4), 0, 4), (6, (3, 4), 0, 8)],
    "clash": [(53, (4,), 0, 1), (46, (5,), 0, 2), (8, (1,), 1, 6)],
    "mid": [(120, (9,), 0, 1), (78, (9,), 0, 2), (23, (1,), 1, 3)],
}
METRICS_POSES = {"small": 3, "frac": 3, "onechain": 2, "chains3": 2, "clash": 5, "mid": 3}
METRICS_STACKED = {"mid": 3}                      # P stacked logit sets (x_pred then has P rows)
METRICS_BEST_ROW = {"small": 7, "frac": 7, "onechain": 5, "chains3": 11, "clash": 40, "mid": 150}
CLASH_DIST, CLASH_MARGIN, TM_GAP, FRAC_MARGIN = 1.1, 1e-4, 1e-4, 1e-3


def metrics_logits(A, T, seed, P=None, best_row=0, bins_plddt=50, bins_pae=64):
    """p_plddt [A,bins] hashed uniform in (-4, 4); p_pae [T,T,bins] = the same minus a per-row slope g_i 6 k / bins that favours
    the low-error bins, g_i hashed in (0, 1) and 1.5 for `best_row`, so that per_alignment differs from row to row (plain uniform
    logits give every row the same expectation and no argmax gap).  With P a leading dimension [P, ...] (set p: seed + 100 p,
    best row best_row + p).  IEEE fp32 products and differences of hashed integers only: bit-identical everywhere."""
    import numpy as np
    def one(s, row):
        pl = hashed_uniform(A * bins_plddt, 3 * s).reshape(A, bins_plddt) * np.float32(8.0)
        g = hashed_uniform(T, 3 * s + 1) + np.float32(0.5)
        g[row] = np.float32(1.5)
        ramp = np.arange(bins_pae, dtype=np.float32) * np.float32(6.0 / bins_pae)
        pa = hashed_uniform(T * T * bins_pae, 3 * s + 2).reshape(T, T, bins_pae) * np.float32(8.0) - g[:, None, None] * ramp[None, None, :]
        return pl, pa
    if P is None:
        pl, pa = one(seed, best_row)
    else:
        pl, pa = (np.stack(v) for v in zip(*[one(seed + 100 * p, best_row + p) for p in range(P)]))
    return {"p_plddt": torch.from_numpy(pl), "p_pae": torch.from_numpy(pa)}


def _lattice(n, origin, seed, spacing=3.0, jitter=0.2):
    """n points of a cubic lattice (spacing 3, hashed jitter +- 0.2: no two closer than 2.6)"""
    import numpy as np
    m = int(np.ceil(n ** (1.0 / 3.0)))
    idx = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)[:n]
    return (np.asarray(origin, np.float32)[None] + idx.astype(np.float32) * np.float32(spacing)
            + hashed_uniform(3 * n, seed).reshape(n, 3) * np.float32(2 * jitter))


def metrics_case(name, stored=None):
    """(output, batch, info) of the fixture tests/golden/g18_metrics_<name>.npz (tools/make_golden_metrics.py): output = p_plddt,
    p_pae (metrics_logits), x_pred [B,A,3]; batch = METRICS_FEAT_KEYS (is_ligand bool, asym_id int32, s_mask / a_mask fp32).
    With `stored` (the loaded fixture) the features and x_pred come from it and the logits are rebuilt bit for bit.
    Geometry: every chain on its own jittered lattice 50 A from the others (no contact).  `clash` then moves atoms of chain 1 to
    0.4 - 0.6 A of atoms of chain 0, exactly one pair each: pose 0 none, pose 1 80 pairs, pose 2 101, pose 3 100, pose 4 ten onto
    MASKED atoms of chain 0 plus the eight ligand atoms onto chain 1.  info["a_mask_pose"] [5,A] are the per-pose atom masks
    that turn those counts into the rules (chain 0 has 212 atoms, the main mask a_mask = a_mask_pose[0] hides ten, leaving 202):
    pose 1 leaves 150 (ratio rule alone: 80 <= 100, 160 > 150), pose 2 the main mask (count rule alone: 101, 202 <= 202),
    pose 3 leaves 200 (the boundary: 100, ratio exactly 0.5, no clash), pose 4 the main mask."""
    import numpy as np
    seed, layout = METRICS_SEEDS[name], METRICS_LAYOUT[name]
    P = METRICS_STACKED.get(name)
    if stored is not None:
        f = {k: torch.from_numpy(np.asarray(stored[k])) for k in METRICS_FEAT_KEYS}
        A, T = f["a_mask"].shape[0], f["s_mask"].shape[0]
        return {**metrics_logits(A, T, seed, P, METRICS_BEST_ROW[name]), "x_pred": torch.from_numpy(np.asarray(stored["x_pred"]))}, f, {}
    chunk, lig, asym, start_atom, pos = [], [], [], [], []
    for c, (nt, per, is_lig, aid) in enumerate(layout):
        sizes = [per[t % len(per)] for t in range(nt)]
        start_atom.append(int(sum(chunk)))
        chunk += sizes
        lig += [is_lig] * nt
        asym += [aid] * nt
        origin = [(50.0 * c, 0.0, 0.0), (0.0, 50.0 * c, 0.0), (0.0, 0.0, 50.0 * c)][c % 3]
        pos.append(_lattice(sum(sizes), origin, 7 * seed + c))
    chunk = np.asarray(chunk)
    T, A, B = len(chunk), int(chunk.sum()), METRICS_POSES[name]
    x0 = np.concatenate(pos).astype(np.float32)
    x = np.stack([x0 + hashed_uniform(3 * A, 11 * seed + b).reshape(A, 3) * np.float32(0.2) for b in range(B)])
    a_mask, s_mask = np.ones(A, np.float32), np.ones(T, np.float32)
    info = {}
    if name in ("small", "frac", "onechain"):
        s_mask[[1, 4, 8, 13, 17, 22]] = 0.0                  # sum w = 18 < 19: the clip of d0
        a_mask[[5, 30]] = 0.0
    if name == "frac":
        live = s_mask > 0
        s_mask[live] = (hashed_uniform(T, seed)[live] * np.float32(0.9) + np.float32(0.55))      # (0.1, 1.0)
        s_mask[0] = 1.0
    if name == "clash":
        a0, b0, l0 = start_atom
        main = a_mask.copy()
        main[a0 + 202:a0 + 212] = 0.0
        masks = np.stack([main] * 5)
        masks[1, a0 + 150:a0 + 202] = 0.0
        masks[3, a0 + 200:a0 + 202] = 0.0
        off = hashed_uniform(3 * A, 13 * seed).reshape(A, 3) * np.float32(0.2) + np.asarray([0.5, 0.0, 0.0], np.float32)
        for b, n in ((1, 80), (2, 101), (3, 100)):
            x[b, b0:b0 + n] = x[b, a0:a0 + n] + off[:n]
        x[4, b0:b0 + 10] = x[4, a0 + 202:a0 + 212] + off[:10]
        x[4, l0:l0 + 8] = x[4, b0 + 20:b0 + 28] + off[:8]
        a_mask = main
        info["a_mask_pose"] = masks
    f = {"s_mask": torch.from_numpy(s_mask), "asym_id": torch.from_numpy(np.asarray(asym, np.int32)), "a_mask": torch.from_numpy(a_mask),
         "atom_id_to_token_id": torch.from_numpy(np.repeat(np.arange(T), chunk).astype(np.int64)),
         "is_ligand": torch.from_numpy(np.asarray(lig, bool))}
    info.update(layout=layout, B=B)
    return {**metrics_logits(A, T, seed, P, METRICS_BEST_ROW[name]), "x_pred": torch.from_numpy(x.astype(np.float32))}, f, info


def metrics_eval(o, f, dtype, skip_self_pairs=False, a_mask=None, max_bin=32.0):
    """get_metrics restated in numpy at `dtype` (float64: the fixtures' f64_*; float32: a plain fp32 evaluation, whose distance
    from the former is e32_*).  o: p_plddt [A,nb] / p_pae [T,T,nb] (or with a leading P), x_pred [B,A,3]; returns the reference's
    keys with leading dim P (has_clash for every pose: [B]), plus rows [P,2], per_alignment [P,2,T], gaps [P,2] (top two of
    per_alignment_i w_i), closest (eligible inter-chain distance nearest to 1.1) and n_clash [B,n,n] / n_atoms [n]."""
    import numpy as np
    pl, pa, x = (np.asarray(o[k]) for k in ("p_plddt", "p_pae", "x_pred"))
    if pa.ndim == 3:
        pl, pa = pl[None], pa[None]
    w = np.asarray(f["s_mask"]).astype(dtype)
    asym = np.asarray(f["asym_id"])
    nb = pa.shape[-1]
    def softmax(l):
        e = np.exp(l - l.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)
    cp = ((np.arange(pl.shape[-1]) + 0.5) / pl.shape[-1]).astype(dtype)
    atom = (softmax(pl.astype(dtype)) * cp).sum(-1) * dtype(100)
    centres = _metrics_centres(max_bin, nb).astype(dtype)
    probs = softmax(pa.astype(dtype))
    pae = (probs * centres).sum(-1)
    n = max(int(np.asarray(f["s_mask"]).astype(np.float64).sum()), 19)
    d0 = dtype(1.24 * (n - 15) ** (1.0 / 3.0) - 1.8)
    tm = (probs * (dtype(1) / (dtype(1) + centres * centres / (d0 * d0)))).sum(-1)
    out = {"atom_plddts": atom, "mean_plddt": atom.mean(-1), "pae": pae}
    rows, pas, gaps, vals = [], [], [], []
    for m in (np.ones((len(w), len(w)), dtype), (asym[:, None] != asym[None, :]).astype(dtype)):
        pw = m * (w[None, :] * w[:, None])
        per = (tm * m * (pw / (dtype(1e-8) + pw.sum(-1, keepdims=True)))).sum(-1)
        sel = per * w
        r = sel.argmax(-1)
        top = np.sort(sel, -1)
        rows.append(r)
        pas.append(per)
        gaps.append(top[:, -1] - top[:, -2])
        vals.append(np.take_along_axis(per, r[:, None], -1)[:, 0])
    out["ptm"], out["iptm"] = vals
    out["rows"], out["per_alignment"], out["gaps"] = np.stack(rows, -1), np.stack(pas, 1), np.stack(gaps, -1)
    # clash: integer decisions on float64 distances (the fixtures keep every distance CLASH_MARGIN from 1.1)
    a2t = np.asarray(f["atom_id_to_token_id"])
    am = np.asarray(f["a_mask"] if a_mask is None else a_mask)
    el = (am == 1) & (np.asarray(f["is_ligand"]) == 0)[a2t]
    ca = asym[a2t][el]
    uniq = np.unique(ca)
    xe = x[:, el].astype(np.float64)
    d = np.sqrt(((xe[:, :, None] - xe[:, None]) ** 2).sum(-1))
    cross = ca[:, None] != ca[None, :]
    out["closest"] = float(np.abs(d[:, cross] - CLASH_DIST).min()) if cross.any() else float("inf")
    nat = np.asarray([(ca == u).sum() for u in uniq])
    ncl = np.asarray([[[(d[b][ca == u][:, ca == v] < CLASH_DIST).sum() for v in uniq] for u in uniq] for b in range(x.shape[0])]).reshape(x.shape[0], len(uniq), len(uniq))
    has = np.zeros(x.shape[0], np.int64)
    for b in range(x.shape[0]):
        for i in range(len(uniq) - 1):
            for j in range(1, len(uniq)):
                if skip_self_pairs and not i < j:
                    continue
                if ncl[b, i, j] > 100 or 2 * ncl[b, i, j] > min(nat[i], nat[j]):
                    has[b] = 1
    out["has_clash"], out["n_clash"], out["n_atoms"] = has, ncl, nat
    hc = has.astype(dtype) if len(has) == len(vals[0]) else has[:1].astype(dtype)
    out["ranking_confidence"] = dtype(0.8) * out["iptm"] + dtype(0.2) * out["ptm"] - hc
    return out


def _metrics_centres(max_bin, no_bins):
    """the reference's bin centres from its own torch fp32 operations (physdock_amd.metrics builds the device table the same way)"""
    breaks = torch.linspace(0., float(max_bin), no_bins - 1)
    step = breaks[1] - breaks[0]
    c = breaks + step / 2
    return torch.cat([c, (c[-1] + step)[None]]).numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# G19: the confidence head over several poses of one system (ConfidenceModule.forward_poses / score_poses)
CONF_POSES_CASES = {"small": dict(n=(4, 5, 32, 8), seed=11, poses=5), "ragged": dict(n=(17, 5, 6, 8), seed=4, poses=3)}
CONF_POSES_FEAT_KEYS = ("s_mask", "asym_id", "a_mask", "atom_id_to_token_id", "is_ligand")


def confidence_poses_case(name):
    """(config block, batch, inputs) of a G19 fixture: a synthetic system (small: T 36 / A 52; ragged: T 23 / A 91, neither a
    multiple of 4), trunk-like s / z and P poses around x_gt that differ where the confidence head looks - 0: lightly noised;
    1: the ligand rotated by 90 degrees about its centroid and shifted; last: the second protein chain pushed onto the first
    (0.3 A from its atoms: a clear chain clash); the others (with three poses: pose 1 as well): the whole complex dilated, so that
    centre distances reach the far bins, with the ligand shifted.  The metrics' chain features are set here (the protein split into two chains, then the
    ligand), since the confidence head itself reads none of them."""
    c = CONF_POSES_CASES[name]
    from .configs import small_config
    cm = dict(small_config().model.confidence_module)
    batch = dict(make_batch(*c["n"], seed=c["seed"]))
    inp = confidence_inputs(batch, cm["c_s"], cm["c_z"], seed=5 + c["seed"], n_pose=1)
    batch["token_id_to_centre_atom_id"] = inp["token_id_to_centre_atom_id"]
    n_prot, apr, n_lig = c["n"][0], c["n"][1], c["n"][2]
    T, A = n_prot + n_lig, n_prot * apr + n_lig
    half = n_prot // 2
    batch["asym_id"] = torch.tensor([0] * half + [1] * (n_prot - half) + [2] * n_lig, dtype=torch.int32)
    batch["is_ligand"] = torch.tensor([False] * n_prot + [True] * n_lig)
    batch["s_mask"], batch["a_mask"] = torch.ones(T), torch.ones(A)
    g = torch.Generator(device="cpu")
    g.manual_seed(103 + c["seed"])
    x0 = batch["x_gt"].float()
    lig = torch.arange(A) >= n_prot * apr
    ch0, ch1 = torch.arange(0, half * apr), torch.arange(half * apr, n_prot * apr)
    poses = []
    for p in range(c["poses"]):
        x = x0 + 0.3 * torch.randn(A, 3, generator=g)
        if p == c["poses"] - 1:
            n = min(len(ch0), len(ch1))
            x[ch1[:n]] = x[ch0[:n]] + torch.tensor([0.3, 0.0, 0.0])
        else:
            if p == 1:
                cen = x[lig].mean(0)
                rot = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
                x[lig] = (x[lig] - cen) @ rot.t() + cen + torch.tensor([4.0, -2.0, 1.0])
            if p >= 2 or (p == 1 and c["poses"] <= 3):
                x = (x - x.mean(0)) * (1.0 + 0.5 * max(p, 2)) + x.mean(0)
                x[lig] += torch.tensor([0.0, 3.0 * p, -2.0])
        poses.append(x)
    inp["x_pred"] = torch.stack(poses, 0)
    return cm, batch, inp


CONF_POSES_WD_SCALE = 12.0


def confidence_poses_weights(cm):
    """the G12 weights (seed 3) with linear_d - the only weight that sees the pose on the pair track - scaled up, so that the poses'
    scores lie well apart (seeded weights of unit scale leave the random z in charge and every pose with nearly the same pTM)"""
    from .params import confidence_param_shapes, seeded_state_dict
    sd = seeded_state_dict(confidence_param_shapes(**cm), seed=3)
    sd["linear_d.weight"] = sd["linear_d.weight"] * CONF_POSES_WD_SCALE
    return sd
