"""tests/pose_clusters_ref.py - the written definition of PoseClusters - against its own invariants, and the host-side validation of
`PoseClusters` and of `redock(clusters=)`.  No GPU: nothing here launches a kernel."""
import numpy as np
import pytest
import torch

import pose_clusters_ref as ref

SEEDED = ("n70_random", "n70_planted", "n257_random", "n257_planted", "n70_at_cutoff", "n70_nan_pair", "n70_nan_leader",
          "n70_best_invalid", "n70_all_invalid", "n257_score_ties")


def run(c):
    return ref.restate(c["D"], c["order"], c["cutoff"], valid=c["valid"], score=c["score"])


@pytest.mark.parametrize("name", SEEDED)
def test_invariants_of_the_restatement(name):
    c = ref.make_case(name)
    assert np.array_equal(c["D"], c["D"].T, equal_nan=True) and not np.diag(c["D"]).any() and c["D"].dtype == np.float32
    assert sorted(c["order"].tolist()) == list(range(len(c["order"])))
    res = run(c)
    ref.check_invariants(c["D"], c["order"], c["cutoff"], res, valid=c["valid"])
    assert np.isnan(res["mean_score"]).all() == (c["score"] is None) or int(res["n_clusters"][0]) == 0


def test_every_named_case_builds_and_is_well_formed():
    for name in ref.CASES:
        c = ref.make_case(name)
        n = c["D"].shape[0]
        assert c["D"].shape == (n, n) and c["order"].dtype == np.int32 and sorted(c["order"].tolist()) == list(range(n)), name


def test_planted_modes_are_found():
    c = ref.make_case("n257_planted")
    res = run(c)
    assert int(res["n_clusters"][0]) == 7
    for k in range(7):
        members = np.nonzero(res["labels"] == k)[0]
        assert len(set((members % 7).tolist())) == 1, "a cluster is one planted group, its members interleaved in pose id"
    assert sorted(res["size"][:7].tolist()) == sorted(np.bincount(np.arange(257) % 7).tolist())


def test_relabelling_the_poses_permutes_the_result():
    c = ref.make_case("n70_planted")
    c["score"] = np.random.default_rng(5).normal(-7, 1, 70).astype(np.float32)
    res = run(c)
    p = np.random.default_rng(6).permutation(70)                      # new id p[i] for pose i
    inv = np.argsort(p)
    D2 = np.ascontiguousarray(c["D"][np.ix_(inv, inv)])               # D2[p[i], p[j]] = D[i, j]
    res2 = ref.restate(D2, p[c["order"]].astype(np.int32), c["cutoff"], score=c["score"][inv])
    K = int(res["n_clusters"][0])
    assert int(res2["n_clusters"][0]) == K
    assert np.array_equal(res2["labels"][p], res["labels"]) and ref.same_bits(res2["dist_to_leader"][p], res["dist_to_leader"])
    assert np.array_equal(res2["leader"][:K], p[res["leader"][:K]]) and np.array_equal(res2["size"], res["size"])
    assert ref.same_bits(res2["radius"], res["radius"])
    # the sums run in another order under the new ids: spread and mean_score agree to rounding, not to the bit; the medoid is the
    # same pose wherever no second member comes within that rounding of its sum
    assert np.allclose(res2["spread"][:K], res["spread"][:K], rtol=1e-6) and np.allclose(res2["mean_score"][:K], res["mean_score"][:K], rtol=1e-6)
    assert np.array_equal(res2["medoid"][:K], p[res["medoid"][:K]])


def test_cutoff_extremes():
    D, order = ref.random_matrix(70, seed=3), ref.permutation(70, 4)
    one = ref.restate(D, order, 1.0e30)
    assert int(one["n_clusters"][0]) == 1 and (one["labels"] == 0).all() and one["leader"][0] == order[0] and one["size"][0] == 70
    assert ref.same_bits(one["radius"][0], D[order[0]].max())
    assert (D[~np.eye(70, dtype=bool)] > 0).all()
    single = ref.restate(D, order, 0.0)
    assert int(single["n_clusters"][0]) == 70 and np.array_equal(single["leader"], order) and (single["size"] == 1).all()
    assert np.array_equal(single["labels"][order], np.arange(70)) and np.array_equal(single["medoid"], order)
    assert not single["radius"].any() and not single["spread"].any() and not single["dist_to_leader"].any()


def test_the_hand_worked_case():
    c = ref.hand_case()
    res = run(c)
    assert res["labels"].tolist() == [1, 0, 1, 0, 0]
    assert res["leader"].tolist() == [3, 0, -1, -1, -1] and res["size"].tolist() == [3, 2, 0, 0, 0]
    assert res["medoid"].tolist() == [4, 0, -1, -1, -1] and res["n_clusters"].tolist() == [2]
    assert res["dist_to_leader"].tolist() == [0.0, 2.0, 1.0, 0.0, 1.5]
    assert res["radius"][:2].tolist() == [2.0, 1.0] and np.isnan(res["radius"][2:]).all()
    assert res["spread"][:2].tolist() == [float(np.float32(8.0 / 6.0)), 1.0] and np.isnan(res["spread"][2:]).all()
    assert res["mean_score"][:2].tolist() == [float(np.float32(-23.75 / 3.0)), -7.0] and np.isnan(res["mean_score"][2:]).all()
    for k, v in ref.HAND.items():                                      # the literals the GPU test compares with
        got = res[k] if k in ref.INT_KEYS or k == "dist_to_leader" else res[k][:2]
        assert np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(v, dtype=np.float64)), k
    assert np.isnan(ref.restate(c["D"], c["order"], c["cutoff"])["mean_score"]).all(), "no score, no mean"


def test_nan_and_invalid_poses():
    c = ref.make_case("n70_nan_leader")
    res = run(c)
    assert res["labels"][0] == 0 and res["labels"][2] != 0, "a NaN never joins"
    c = ref.make_case("n70_nan_pair")
    res = run(c)
    k = res["labels"][3]
    assert res["labels"][5] == k and res["medoid"][k] not in (3, 5) and np.isnan(res["spread"][k]), "a NaN sum is never the smallest"
    c = ref.make_case("n70_best_invalid")
    res = run(c)
    assert res["labels"][c["order"][0]] == -1 and res["leader"][0] == c["order"][1]
    res = run(ref.make_case("n70_all_invalid"))
    assert res["n_clusters"][0] == 0 and (res["labels"] == -1).all() and (res["leader"] == -1).all() and np.isnan(res["dist_to_leader"]).all()
    D = ref.random_matrix(5, seed=1)
    skipped = ref.restate(D, np.array([7, -1, 2, 0, 1], np.int32), 0.0)      # entries outside 0 .. n-1 are skipped
    assert skipped["leader"].tolist() == [2, 0, 1, -1, -1] and skipped["labels"].tolist() == [1, 2, 0, -1, -1]


# ------------------------------------------------------------------ host validation of PoseClusters
def test_spec_validation():
    from physdock_amd import PoseClusters
    from physdock_amd.clustering import MAX_POSES
    spec = PoseClusters()
    assert (spec.cutoff, spec.by, spec.metric) == (2.0, None, "rmsd") and MAX_POSES == 8192
    assert PoseClusters(0.4, by="vina_refined", metric="interactions").metric == "interactions"
    with pytest.raises(AttributeError):
        spec.cutoff = 3.0
    for bad in (dict(by="rmsd"), dict(by="score"), dict(metric="tanimoto"), dict(metric=None), dict(cutoff=-1.0),
                dict(cutoff=float("nan")), dict(cutoff=float("inf"))):
        with pytest.raises(ValueError):
            PoseClusters(**bad)


def test_cluster_rejects_wrong_shapes_and_dtypes_on_the_host():
    from physdock_amd import PoseClusters
    spec = PoseClusters()
    D = torch.zeros(4, 4)
    bad = [dict(D=torch.zeros(4, 5)), dict(D=torch.zeros(4)), dict(D=torch.zeros(4, 4, dtype=torch.float64)), dict(D=np.zeros((4, 4), np.float32)),
           dict(D=torch.zeros(0, 0)), dict(D=D, order=torch.arange(3)), dict(D=D, order=torch.arange(4).float()), dict(D=D, order=[0, 1, 2, 3]),
           dict(D=D, scores=torch.zeros(5)), dict(D=D, scores=torch.zeros(4, dtype=torch.int32)), dict(D=D, scores={"score": torch.zeros(3)}),
           dict(D=D, valid=torch.ones(5, dtype=torch.bool)), dict(D=D, valid=torch.ones(4))]
    for kw in bad:
        with pytest.raises(ValueError, match="PoseClusters.cluster"):
            spec.cluster(**kw)
    with pytest.raises(ValueError, match="8192"):
        spec.cluster(torch.zeros(1, 1).expand(8193, 8193))
    for kw in (dict(), dict(order=torch.arange(4)), dict(scores=torch.zeros(4), valid=torch.ones(4, dtype=torch.bool))):
        with pytest.raises(ValueError, match="D must be on the GPU"):      # well-formed, but on the host: no launch on host pointers
            spec.cluster(D, **kw)
    with pytest.raises(ValueError, match="x_pred"):
        spec.binding_modes(torch.zeros(4, 6), torch.arange(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="interactions"):
        PoseClusters(metric="interactions").binding_modes(torch.zeros(2, 6, 3), torch.arange(3, dtype=torch.int32))
    with pytest.raises(TypeError, match="cutoff"):
        spec.binding_modes(torch.zeros(2, 6, 3), torch.arange(3, dtype=torch.int32), cutoff=1.0)
    with pytest.raises(ValueError, match="per="):
        spec.representatives({}, per="centroid")


def test_redock_names_a_missing_prerequisite_before_the_model_is_touched():
    from physdock_amd import PoseClusters, driver

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name})")

    for spec, given, match in ((PoseClusters(by="vina"), {}, "vina="), (PoseClusters(by="confidence"), {}, "confidence="),
                               (PoseClusters(by="vina_refined"), {"vina": object()}, "refine="),
                               (PoseClusters(by="vina_refined"), {"refine": object()}, "vina="),
                               (PoseClusters(metric="interactions"), {}, "interactions="), ("rmsd", {}, "PoseClusters")):
        with pytest.raises(ValueError, match=match):
            driver.redock(Untouchable(), {}, clusters=spec, **given)
    with pytest.raises(ValueError, match="vina="):
        driver._RedockState({}, {}, clusters=PoseClusters(by="vina"))


def test_summary_reads_a_result_into_one_dict_per_mode():
    from physdock_amd import PoseClusters
    res = {k: torch.from_numpy(np.asarray(v)) for k, v in run(ref.hand_case()).items()}
    told = PoseClusters.summary(res)
    assert told == [dict(leader=3, medoid=4, size=3, members=[1, 3, 4], radius=2.0, spread=float(np.float32(8.0 / 6.0)),
                         mean_score=float(np.float32(-23.75 / 3.0))),
                    dict(leader=0, medoid=0, size=2, members=[0, 2], radius=1.0, spread=1.0, mean_score=-7.0)]
    assert PoseClusters.representatives(res).tolist() == [3, 0, -1, -1, -1]
    assert PoseClusters.representatives(res, per="medoid").tolist() == [4, 0, -1, -1, -1]
