"""The references of tests/entry_kernels_ref.py are right, the inputs of tests/test_entry_kernels_gpu.py are well posed, and every
check has power.  CPU only: each reference against the committed oracles where those restate the same thing (features_oracle
make_feats, dgram_from_positions, make_token_bonds, write_pdb_block; physdock_oracle one_hot_nearest), the conditions the GPU cases
rely on - every planted tie, midpoint and edge exact in fp32, every chirality centre clear of its rounding bound, none left out -,
and deliberately wrong variants of the operations (last-minimum argmin, <= on a bin edge, round-half-up formatting, a tie going to
the upper bin, centres beyond 64 ignored), which the comparisons of the GPU tests must reject on these very inputs."""
import numpy as np
import pytest
import torch

import entry_kernels_ref as er
import features_oracle as fo
import physdock_oracle as orc
import test_sampler_kernels_gpu as ts

F32, F64 = torch.float32, torch.float64


def exact32(v):
    return float(np.float32(v)) == float(v)


# ------------------------------------------------------------------ references against the oracles
@pytest.mark.parametrize("R,T", [(1, 1), (3, 7), (5, 7)])
def test_target_and_msa_feat_against_make_feats(R, T):
    m, t = er.msa_case(R, T, 32), er.target_case(T, 32)
    # the oracle's F.one_hot refuses an index outside the classes, which the kernel turns into a row of zeros: compare without those
    restype = t["restype"].clamp(0, 31)
    msa = torch.where(m["msa"] < 32, m["msa"], torch.zeros_like(m["msa"]))
    feats = fo.make_feats(dict(restype=restype, profile=t["profile"], deletion_mean=t["deletion_mean"], msa=msa,
                               deletion_matrix=m["deletion"]), m["inds"])
    assert torch.equal(er.target_feat(restype, t["profile"], t["deletion_mean"], 32), feats["target_feat"])
    assert torch.equal(er.msa_feat_exact(msa, m["deletion"], m["inds"], 32), feats["msa_feat"][..., :33])
    ref32 = er.msa_feat_atan(m["deletion"], m["inds"], er.TWO_OVER_PI, F32)
    torch.testing.assert_close(ref32, feats["msa_feat"][..., 33], rtol=0, atol=1.2e-7)
    # and what the clamp leaves out of the oracle's reach: all-zero rows
    assert float(er.one_hot_eq(torch.tensor([32, -1, 37]), 32).abs().sum()) == 0.0
    assert (er.msa_feat_exact(**m)[..., :32].sum(-1) == (m["msa"][m["inds"]] < 32).float()).all()


def test_msa_case_reaches_both_ends_of_the_clamp_and_every_index_pattern():
    c = er.msa_case(5, 7, 32)
    used = c["deletion"][c["inds"]]
    assert set(used.flatten().tolist()) == set(torch.tensor(er.DELETION_VALUES).tolist())
    assert c["inds"].tolist() == [5, 3, 3, 1, 0] and c["msa"].shape[0] == 6
    assert er.msa_case(1, 1, 32)["inds"].tolist() == [5]
    sel = c["msa"][c["inds"]]
    assert (sel == 32).any() and (sel > 32).any() and set(range(32)) <= set(c["msa"].flatten().tolist())
    ref64 = er.msa_feat_atan(c["deletion"], c["inds"], er.TWO_OVER_PI)
    assert float(ref64.min()) < -0.3 and float(ref64.max()) > 0.9999 and torch.isfinite(ref64).all()
    ts.check_close("msa_feat atan (torch fp32)", "R=5 T=7", er.msa_feat_atan(c["deletion"], c["inds"], er.TWO_OVER_PI, F32),
                   er.msa_feat_atan(c["deletion"], c["inds"], er.TWO_OVER_PI, F32), ref64)
    with pytest.raises(AssertionError):                                   # atan(d) / 3 in the place of atan(d / 3)
        wrong = torch.atan(used.double()) / 3 * er.TWO_OVER_PI
        ts.check_close("msa_feat atan (wrong)", "R=5 T=7", wrong.float(), er.msa_feat_atan(c["deletion"], c["inds"], er.TWO_OVER_PI, F32), ref64)
    assert er.msa_case(3, 7, 3)["n_class"] + 2 == 5


def test_template_feat_against_dgram_from_positions():
    c = er.template_random_case()
    got = er.template_feat(**c)
    xpb = c["x"][c["pb"]]
    prot2d = c["is_protein"][None] * c["is_protein"][:, None]
    mask = c["z_mask"] * prot2d
    want = torch.cat([fo.dgram_from_positions(xpb) * prot2d[..., None] * c["z_mask"][..., None] * mask[..., None], mask[..., None]], dim=-1)
    # torch.sum over the last axis may add the three squares in another order than (dx^2 + dy^2) + dz^2: a pair within one rounding of
    # an edge could differ, the case has none
    d2 = er.dist2(xpb[:, None], xpb[None, :])
    assert float((d2[..., None] - c["lower"]).abs().min()) > 1e-3
    assert torch.equal(got, want)
    assert 0.2 < float(got[..., :39].sum() / got[..., 39].sum()) <= 1.0 and (got[..., :39].sum((0, 1)) > 0).sum() > 10


def test_nearest_bin_against_one_hot_nearest():
    d = torch.cat([torch.tensor(er.CENTRE_AXIS), torch.rand(200, generator=er.gen(1)) * 30])
    assert torch.equal(torch.nn.functional.one_hot(er.nearest_bin(d), 13).float(), orc.one_hot_nearest(d, er.BIN_CENTRES.float()))
    assert torch.equal(er.BIN_CENTRES.float(), torch.linspace(3.375, 24.375, 13))


def test_chain_contacts_against_make_token_bonds():
    c, asym = er.chain_contacts_oracle_case()
    mins, args, between = er.chain_contacts(**c)
    t = fo.make_token_bonds(dict(atom_id_to_token_id=c["a2t"], asym_id=asym, is_ligand=torch.ones_like(asym), x_gt=c["x"],
                                 a_mask=c["a_mask"], token_bonds=torch.zeros(c["T"], c["T"])), threshold=c["threshold"])
    assert torch.equal(between, t["token_bonds"])
    assert (mins < 2.4).sum() >= 2 and (mins > 2.4).sum() >= 2 and float((mins - 2.4).abs().min()) > 1e-3
    assert (c["a_mask"] == 0).any() and torch.equal(between, between.T) and 2 <= int(between.sum()) <= 2 * len(mins)


def test_pdb_format_against_write_pdb_block():
    g = er.gen(2)
    meta = dict(atom_id_to_conformer_atom_id=[0, 1, 2, 0, 1, 2, 3], ccds=["ALA", "LIG"], conformer_id_to_chunk_sizes=torch.tensor([3, 4]),
                residue_index=torch.tensor([4, 0]), asym_id=torch.tensor([0, 1]), CHAIN_CLASS=["protein", "ligand"],
                CONF_META_DATA={"ALA": dict(ref_atom_name_chars=["N", "CA", "C"], ref_element=[6, 5, 5]),
                                "LIG": dict(ref_atom_name_chars=["C1", "O1", "CL12", "N1"], ref_element=[5, 7, 16, 6])})
    x = torch.rand(2, 7, 3, generator=g) * 400 - 200
    x[0, 0] = torch.tensor([0.0005, -0.0005, 2.0625])
    x[1, 3] = torch.tensor([9999.0, -999.0, -0.0001])
    blank = fo.write_pdb_block(torch.zeros(7, 3), meta).split("\n")[1:8]
    rows = torch.tensor([list((line + "\n").encode()) for line in blank], dtype=torch.uint8)
    out, bad = er.pdb_format(x, rows, torch.arange(7))
    assert bad == 0
    for b in range(2):
        assert bytes(out[b].flatten().tolist()).decode() == "\n".join(fo.write_pdb_block(x[b], meta).split("\n")[1:8]) + "\n"


# ------------------------------------------------------------------ chain_contacts: planted ties and the threshold
def test_chain_contacts_planted_values_are_exact_and_placed_where_the_loop_splits():
    c, expect = er.chain_contacts_case()
    mins, args, between = er.chain_contacts(**c)
    mins64, args64, _ = er.chain_contacts(**c, dtype=F64)
    cs = c["chain_start"].tolist()
    for p, ((name, ni, nj, planted, want), (ci, cj)) in enumerate(zip(er.CONTACT_SCENARIOS, c["pairs"].tolist())):
        assert (cs[ci + 1] - cs[ci], cs[cj + 1] - cs[cj]) == (ni, nj)
        if ni * nj == 0:
            assert int(args[p]) == -1 and float(mins[p]) == er.INF
            continue
        v32 = er.chain_pair_matrix(c["x"], c["a_mask"], cs[ci], cs[ci + 1], cs[cj], cs[cj + 1]).reshape(-1)
        v64 = er.chain_pair_matrix(c["x"], c["a_mask"], cs[ci], cs[ci + 1], cs[cj], cs[cj + 1], F64).reshape(-1)
        for k, dist in planted:                                           # exact: fp32 and float64 give the very same number
            assert exact32(dist) and float(v32[k]) % 1000 == dist and (float(v64[k]) % 1000 == dist or dist != int(dist))
        if want is not None:
            assert int(args[p]) == want == int(args64[p])
        others = torch.ones(ni * nj, dtype=torch.bool)
        others[[k for k, _ in planted]] = False
        assert not others.any() or float(v32[others].min()) > 40.0       # nothing else comes near
    names = [s[0] for s in er.CONTACT_SCENARIOS]
    tie = lambda n: [k for k, _ in er.CONTACT_SCENARIOS[names.index(n)][3]]
    a, b = tie("same thread, trips 0 and 1")
    assert a % 256 == b % 256 and (a // 256, b // 256) == (0, 1) and 17 * 16 == 272 > 256
    a, b = tie("thread 200 trip 0 against thread 4 trip 1")
    assert a < b and a % 256 > b % 256 and (a // 256, b // 256) == (0, 1)
    a, b = tie("thread 200 trip 1 against thread 4 trip 2")
    assert a < b and a % 256 > b % 256 and (a // 256, b // 256) == (1, 2)       # the lower k in the higher thread's second trip
    a, b = tie("thread 4 trip 1 against thread 200 trip 2")
    assert a < b and a % 256 < b % 256 and (a // 256, b // 256) == (1, 2)       # and the other way round
    a, b, d = tie("three equal minima")
    assert len({a % 256, b % 256, d % 256}) == 2 and a % 256 == b % 256
    # the threshold: 2.5 itself does not bond, the next fp32 number below it does
    on, below = names.index("on the threshold"), names.index("one step below the threshold")
    assert float(mins[on]) == 2.5 and float(mins[below]) == float(np.nextafter(np.float32(2.5), np.float32(0)))
    tok = lambda p: (int(c["a2t"][cs[c["pairs"][p][0]]]), int(c["a2t"][cs[c["pairs"][p][1]]]))
    assert between[tok(on)] == 0 and between[tok(below)] == 1
    # masks: the masked minimum loses; the fully masked chain sits above 1000 and bonds nothing
    masked = names.index("closest pair masked")
    assert float(mins[masked]) == 2.0 and int(args[masked]) == 150
    full = names.index("second chain fully masked")
    assert float(mins[full]) == 1001.0
    # the exchanged search of the first scenario sets the same token pair, and several atoms share a token
    assert expect[-1] == int(args[-1]) == 85 and c["pairs"][-1].tolist() == [1, 0]
    assert int(between.sum()) == 2 * 8 - 2 and torch.equal(between, between.T)
    assert len(set(c["a2t"].tolist())) < c["a2t"].numel()


def test_chain_contacts_wrong_variants_are_caught():
    c, expect = er.chain_contacts_case()
    mins, args, between = er.chain_contacts(**c)
    _, args_last, between_last = er.chain_contacts(**c, argmin=er.last_argmin)
    wrong = [p for p in range(len(args)) if int(args[p]) != int(args_last[p])]
    assert len(wrong) == 6 and not torch.equal(between, between_last)     # the five ties and the exchanged search
    _, _, between_le = er.chain_contacts(**c, below=torch.le)             # <= threshold: the pair on the threshold bonds
    assert not torch.equal(between, between_le)


# ------------------------------------------------------------------ chirality
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nc", er.CHIRALITY_N)
def test_every_chirality_centre_clears_its_bound(nc, B):
    c = er.chirality_case(nc, B)
    assert c["centres"].shape == (nc, 4) and c["x"].shape == (B, 4 * nc + 3, 3)
    assert len(set(c["centres"].flatten().tolist())) == 4 * nc           # every centre owns its atoms
    ref_sign, ref_ok = er.chirality_sign(c["x_ref"][None], c["centres"])
    sign, decided = er.chirality_sign(c["x"], c["centres"])
    assert ref_ok.all() and decided.all()                                 # zero centres left out
    vol, bound = er.chirality64(c["x"], c["centres"])
    if nc:
        assert float((vol[:2].abs() / bound[:2]).min()) > 100             # and by a wide margin
        assert (ref_sign != 0).all() and (nc == 1 or ((ref_sign == 1).any() and (ref_sign == -1).any()))
        assert torch.equal(sign[0], ref_sign[0])                          # rotated and translated: the same hand
    if nc and B == 3:
        assert torch.equal(sign[1], -ref_sign[0])                         # the mirror image
        assert (sign[2] == 0).all() and (bound[2] == 0).all() and (c["x"][2, :, 2] == 0).all()    # flat: every product is zero
        # ... in fp32 as well: the kernel's expression on the flat pose, each product on its own
        x = c["x"][2]
        o = x[c["centres"][:, 0].long()]
        a, b, d = (x[c["centres"][:, k].long()] - o for k in (1, 2, 3))
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0), (1, 0, 2), (2, 0, 1), (2, 1, 0)):
            assert (a[:, p] * b[:, q] * d[:, r] == 0).all()


def test_chirality_flip_case_flips_one_centre_per_pose_and_the_check_sees_centres_beyond_64():
    c = er.chirality_flip_case()
    ref_sign, _ = er.chirality_sign(c["x_ref"][None], c["centres"])
    sign, decided = er.chirality_sign(c["x"], c["centres"])
    assert decided.all() and c["flipped"] == (None, 0, 64, 129)
    for p, k in enumerate(c["flipped"]):
        assert (sign[p] != ref_sign[0]).nonzero().flatten().tolist() == ([] if k is None else [k])
    accept = er.chirality_accept(sign, ref_sign[0])
    assert accept.tolist() == [1, 0, 0, 0]
    assert er.chirality_accept(sign, ref_sign[0], limit=64).tolist() == [1, 0, 1, 1]          # centres beyond 64 ignored: caught
    assert er.chirality_accept(sign, ref_sign[0], limit=128).tolist() == [1, 0, 0, 1]         # the third trip dropped: caught
    assert er.CHIRALITY_K == 3 + 1 + 1 + 1 + 2


# ------------------------------------------------------------------ template_feat
@pytest.mark.parametrize("NB", [1, 4, 39])
@pytest.mark.parametrize("T", [1, 17])
def test_template_edges_are_hit_exactly(T, NB):
    c = er.template_edges_case(T, NB)
    got = er.template_feat(**c)
    assert got.shape == (T, T, NB + 1)
    m = c["z_mask"] * (c["is_protein"][:, None] * c["is_protein"][None, :])
    assert torch.equal(got[..., NB], m)
    assert float(c["lower"][0]) > 0 and (got[torch.arange(T), torch.arange(T), :NB] == 0).all()                  # i == j: d2 = 0, no bin
    if T == 17:
        assert sorted(set(c["pb"].tolist())) == list(range(14)) and len(c["pb"]) == 17                            # permuted, repeated
        assert ((m != 0) & (m != 1)).any() and (m == 0).any() and (m == 1).any()
        xp = c["x"][c["pb"]]
        d2 = er.dist2(xp[:, None], xp[None, :])
        if NB == 4:
            for edge in er.TEMPLATE_LOWER:                                # d2 on every edge: no bin at all, the mask channel still m
                on = d2 == edge
                assert on.any() and (got[on][:, :NB] == 0).all()
            step = float(np.nextafter(np.float32(1), np.float32(2)) ** 2)
            assert (d2 == np.float32(step)).any() and ((d2 > 0.99) & (d2 < 1)).any()                              # one step either side
            assert (d2 == 1e8).any() and (got[d2 == 1e8][:, :NB] == 0).all() and exact32(1e8)                    # d2 == inf: no last bin
            wrong = er.template_feat(**c, above=torch.ge)                 # <= in the place of < on the lower edge
            assert not torch.equal(wrong, got)
        assert (got[..., :NB].sum(-1) <= m).all()


# ------------------------------------------------------------------ confidence
def test_confidence_midpoints_are_exact_and_go_to_the_lower_bin():
    axis = torch.tensor(er.CENTRE_AXIS)
    assert all(exact32(v) for v in er.CENTRE_AXIS) and torch.equal(axis.double(), torch.tensor(er.CENTRE_AXIS, dtype=F64))
    assert all(m in er.CENTRE_AXIS for m in er.MIDPOINTS) and er.MIDPOINTS[0] == 4.25 and er.MIDPOINTS[-1] == 23.5
    x = torch.zeros(len(axis), 3)
    x[:, 0] = axis
    d = er.centre_distance(x, torch.arange(len(axis)))
    assert torch.equal(d[0], axis)                                        # sqrt(fl(v * v)) == v
    e = (d[0][:, None] - er.BIN_CENTRES.float()).abs()
    for k, mid in enumerate(er.MIDPOINTS):                                # an exact tie between bins k and k + 1
        row = e[er.CENTRE_AXIS.index(mid)]
        assert float(row[k]) == float(row[k + 1]) == 0.875 == float(row.min())
    bins = er.nearest_bin(d[0])
    assert bins.tolist() == [0, 0] + list(range(12)) + [12, 12, 12] and set(bins.tolist()) == set(range(13))
    upper = er.nearest_bin(d[0], er.last_argmin)                          # a tie going to the upper bin: caught at all 12 midpoints
    assert int((upper != bins).sum()) == 12
    for T, C in er.CONF_SHAPES:
        c = er.confidence_case(T, C)
        for centre in (er.centre_rows() if T == 9 else (torch.tensor([2]),)):
            a = (c["z"], c["si"], c["sj"], c["WdT"], c["x"].reshape(-1, 3), centre)
            assert (er.confidence_pair_init(*a) != er.confidence_pair_init(*a, argmin=er.last_argmin)).any() == (T == 9)
    rows = er.centre_rows()
    assert set(rows[0].tolist()) | set(rows[1].tolist()) == set(range(17)) and len(set(rows[2].tolist())) < 9
    assert -(-9 * 9 * 36 // 4 // 256) * 256 != 9 * 9 * 36 // 4              # the last block is not full


def test_pose_layouts_and_embed_case():
    c = er.confidence_case(9, 36, P=3, pad=5)
    assert c["stride"] == 65 and c["x"].numel() == 2 * 65 + 60 and int(torch.isnan(c["x"]).sum()) == 10
    poses = er.pose_coordinates(c["x"], c["stride"], c["A"], 3)
    assert torch.isfinite(poses).all() and not torch.equal(poses[0], poses[1])
    b = [er.nearest_bin(er.centre_distance(p, er.centre_rows()[2])) for p in poses]
    assert not torch.equal(b[0], b[1]) and not torch.equal(b[1], b[2])
    same = er.pose_coordinates(er.confidence_case(9, 36)["x"], 0, c["A"], 3)
    assert torch.equal(same[0], same[2])
    for A in (9, 23):
        e = er.embed_case(A, 16, P=3, pad=5)
        x = er.pose_coordinates(e["x"], e["stride"], A, 3)
        assert torch.equal(x[:, 0], x[:, 1]) and float(x.min()) > 250 and not torch.equal(x[0], x[1])
        out = er.atom_dist_embed(x[0], e["w"], e["b"])
        assert torch.equal(out[0, 1], e["b"]) and torch.equal(out, out.transpose(0, 1))
        ref64 = er.atom_dist_embed(x[0], e["w"], e["b"], F64)
        assert float((out.double() - ref64).abs().max()) < 1e-3          # coordinates near 300 cost digits; the fp32 chain is the contract
        assert torch.equal(er.atom_dist_embed(x[0], e["w"]), er.atom_dist_embed(x[0], e["w"], torch.zeros(16)))
    z = torch.randn(9, 9, 4, generator=er.gen(3))
    s = er.pair_symmetrize(z)
    assert torch.equal(s, s.transpose(0, 1)) and torch.equal(torch.diagonal(s), 2 * torch.diagonal(z))


# ------------------------------------------------------------------ target_feat, outer_mask
def test_target_and_outer_mask_cases():
    for T in (1, 5, 300):
        for NP in (0, 32):
            c = er.target_case(T, NP)
            out = er.target_feat(**c)
            assert out.shape == (T, 33 + NP) and torch.equal(out, er.target_feat(**c, dtype=F64).float())
            assert c["restype"][:4].tolist() == [0, 31, 32, -1][:T]
            assert torch.equal(out[:, :32].sum(-1), ((c["restype"] >= 0) & (c["restype"] < 32)).float())
            assert torch.equal(out[:, -1], c["deletion_mean"]) and torch.equal(out[:, 32:32 + NP], c["profile"])
    assert (300 * 65) % 256 and (5 * 33) % 256
    for N in (1, 17, 257):
        m = er.outer_mask_case(N)
        assert m.shape == (N,) and (N == 1 or set(m.tolist()) == {0.0, 1.0, 0.5, -2.0})
        assert torch.equal(er.outer_mask(m), er.outer_mask(m, F64).float()) and torch.equal(er.outer_mask(m), torch.outer(m, m))
    assert (257 * 257) % 256 and 17 * 17 > 256


# ------------------------------------------------------------------ pdb_format
def test_pdb_cases_fields_and_limits():
    t = er.pdb_template(7)
    assert t.shape == (7, 81) and all(len(set(row[:80].tolist())) == 80 for row in t) and (t[:, 80] == 10).all() and (t != 0xA5).all()
    for B, N in ((1, 1), (3, 7)):
        c = er.pdb_case(B, N)
        assert (B * N * 81) % 256 and sorted(c["atom"].tolist()) != c["atom"].tolist() or N == 1
        assert len(set(c["atom"].tolist())) == N < c["A"]
        assert er.pdb_format(c["x"], c["tmpl"], c["atom"])[1] == 0
    # field limits, as the fp32 numbers the kernel is handed
    fits = lambda v: not er.pdb_field(np.float32(v))[1]
    assert fits(9999.9994) and fits(-999.9994) and not fits(-999.9995)
    assert float(np.float32(9999.9995)) == 9999.9990234375 and fits(9999.9995)       # fp32 has no number between 9999.999 and 10000
    assert not fits(10000.0) and not fits(-1000.0) and fits(np.nextafter(np.float32(10000), np.float32(0)))
    assert all(er.pdb_field(v) == (b"********", True) for v in er.BAD_VALUES)
    assert er.pdb_field(-0.0001)[0] == b"  -0.000" and er.pdb_field(np.float32(2.0625))[0] == b"   2.062"
    # round half up on the scaled value: caught by the exact half 2.0625 and by 0.0005 (below the half as an fp32 number)
    assert er.pdb_field(np.float32(2.0625), half_up=True)[0] == b"   2.063"
    c = er.pdb_case(3, 7)
    right, _ = er.pdb_format(c["x"], c["tmpl"], c["atom"])
    wrong, _ = er.pdb_format(c["x"], c["tmpl"], c["atom"], half_up=True)
    assert 0 in c["atom"].tolist() and not torch.equal(right, wrong)
    # the bad-field case: exactly one bad field in each of four records, one more from the limits, the rest of each record formatted
    c = er.pdb_bad_case()
    out, bad = er.pdb_format(c["x"], c["tmpl"], c["atom"])
    assert bad == 5
    stars = (out[:, :, 30:54] == ord("*")).reshape(3, 7, 3, 8).all(-1)
    assert int(stars.sum()) == 5 and [stars[k % 3, k].tolist() for k in range(4)] == [[f == k % 3 for f in range(3)] for k in range(4)]
    keep = [col for col in range(81) if not 30 <= col < 54]
    assert torch.equal(out[:, :, keep], c["tmpl"][None, :, keep].expand(3, 7, len(keep)))
