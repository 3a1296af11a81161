"""VinaSearch on the host: the written definition tests/vina_search_ref.py against its own invariants, and the conditioning guard of
the GPU tests (tests/test_vina_search_gpu.py).  No GPU: nothing here launches a kernel.

The guard.  Each GPU case is a (case, seed, settings) tuple of `vina_search_ref.GPU_CASES`, and with it the settings of the "proposal
alone" test (steps = 1, max_iters = 0, temperature = inf).  For each, the reference run with ascending summation and its twin with
reversed summation must take identical decisions - entity, accept, new-best, the iterations and status of every descent - and end
within 1e-8 A of each other, the figure tests/test_vina_refine_cpu.py uses; every Metropolis test must have |u_4 - p| >= 1e-6, every
strict comparison of two energies a gap of at least 1e-9 kcal/mol.  These are conditions on the inputs, not tolerances: a seed that
does not meet them is replaced here, on the CPU.

One kind of exact tie is inherent and is not a small gap: a proposal that moves nothing (the rotation of the single atom of
P2_A65_L1_T0 about itself) from a converged point is minimised to the very same conformation, and its energy is then the same bits
as E_cur - on the device as well, where the same operations run on the same numbers.  The guard admits a gap of exactly 0.0 only
where the two conformations compared are bit-identical, in both runs; chains of one pose may tie exactly in the same way (all of them
at the start)."""
import numpy as np
import pytest
import torch

import vina_refine_ref as ref
import vina_search_ref as sr

PROPOSAL = dict(steps=1, max_iters=0, temperature=float("inf"))


@pytest.fixture(scope="module")
def cases():
    return {name: ref.make_case(name) for name in sr.GPU_CASES}


@pytest.fixture(scope="module")
def runs(cases):
    """(case, kind) -> (forward, reversed) searches; kind "trajectory": the case's settings, "proposal": the proposal alone"""
    out = {}
    for name, (seed, st) in sr.GPU_CASES.items():
        for kind, kw in (("trajectory", st), ("proposal", dict(st, **PROPOSAL))):
            out[name, kind] = (sr.search(cases[name], seed=seed, **kw), sr.search(cases[name], seed=seed, order=-1, **kw))
    return out


def test_philox_known_answer():
    # Random123 kat_vectors, philox4x32 10 rounds: all-zero counter and key; all-ones; the digits of pi
    assert sr.philox4x32((0, 0), (0, 0, 0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert sr.philox4x32((0xffffffff, 0xffffffff), (0xffffffff,) * 4) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert sr.philox4x32((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344)) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_the_cases_are_the_ones_the_gpu_tests_run(cases):
    assert set(sr.GPU_CASES) == {"P2_A257_L6_T2", "P3_A300_L12_T3", "P2_A65_L1_T0"}
    for name, (seed, st) in sr.GPU_CASES.items():
        assert st["chains"] == 3 and st["steps"] <= 6 and st["max_iters"] <= 10, name
    assert len(cases["P2_A65_L1_T0"]["rot"]) == 0 and len(cases["P2_A65_L1_T0"]["lig_idx"]) == 1


def test_entity_coverage(cases, runs):
    for name, (seed, st) in sr.GPU_CASES.items():
        c = cases[name]
        T = len(c["rot"])
        drawn = {sr.draw(seed, q, k, m, T)[0] for q in range(c["x"].shape[0]) for k in range(st["chains"]) for m in range(1, st["steps"] + 1)}
        assert drawn == set(range(2 + T)), (name, drawn)
        assert drawn == {e for row in runs[name, "trajectory"][0]["chains"] for r in row for e in r["entity"]}
        for u in sr.draw(seed, 0, 0, 1, T)[1]:
            assert 0.0 < u < 1.0


def test_proposals_are_a_cube_of_one_entity():
    for T in (0, 3):
        for e in range(2 + T):
            s = sr.proposal(e, [0.0, 0.75, 0.25, 1.0 - 2.0 ** -33, 0.5], T, 2.0, 0.5)
            lo, hi = (0, 3) if e == 0 else ((3, 6) if e == 1 else (6 + e - 2, 6 + e - 1))
            assert not s[:lo].any() and not s[hi:].any()
            amp = 2.0 if e == 0 else (0.5 if e == 1 else np.pi)
            assert s[lo] == amp * 0.5 and np.abs(s).max() <= amp


def test_conditioning_guard(runs):
    seen = dict(rejected=0, uphill=0, improved=0)
    for (name, kind), (a, b) in runs.items():
        assert a["best_chain"] == b["best_chain"], (name, kind)
        for p, (row_a, row_b) in enumerate(zip(a["chains"], b["chains"])):
            for k, (ra, rb) in enumerate(zip(row_a, row_b)):
                where = (name, kind, p, k)
                for key in ("entity", "accept", "new_best", "iterations", "status", "start_iterations", "start_status", "best_step", "accepted",
                            "evaluations"):
                    assert ra[key] == rb[key], (where, key, ra[key], rb[key])
                for key in ("y_best", "y_cur", "y_start"):
                    assert np.abs(ra[key] - rb[key]).max() <= 1e-8, (where, key, np.abs(ra[key] - rb[key]).max())
                for r in (ra, rb):
                    assert all(abs(u - q) >= sr.U_MARGIN for u, q in zip(r["u4"], r["p"])), (where, "Metropolis margin")
                    for gap, exact in zip(r["gaps"], r["exact"]):
                        assert gap >= sr.E_MARGIN or (gap == 0.0 and exact), (where, "energy gap", gap)
                if kind == "trajectory":
                    seen["rejected"] += len(ra["accept"]) - sum(ra["accept"])
                    seen["uphill"] += sum(1 for acc, q in zip(ra["accept"], ra["p"]) if acc and q < 1.0)
                else:
                    seen["improved"] += ra["best_step"]
            for r in (row_a, row_b):                                                   # the choice among the chains
                e = np.sort([v["energy"] for v in r])
                assert all(g >= sr.E_MARGIN or g == 0.0 for g in np.diff(e)), (name, kind, p, np.diff(e))
    assert seen["rejected"] >= 1 and seen["uphill"] >= 1, seen
    assert seen["improved"] >= 1, "no proposal lowers the energy: the proposal-alone test would see no proposal in x_chains"


def test_steps_zero_is_refine(cases):
    for name, (seed, st) in sr.GPU_CASES.items():
        c = cases[name]
        kw = {k: v for k, v in st.items() if k not in ("steps", "chains")}
        got = sr.search(c, chains=2, steps=0, seed=seed, **kw)
        for p in range(c["x"].shape[0]):
            want = ref.refine(c, c["x"][p].astype(np.float64), max_iters=st["max_iters"])
            for r in got["chains"][p]:
                assert np.array_equal(r["y_best"], want["y"]) and r["energy"] == want["energy"] == r["energy_start"]
                assert r["evaluations"] == want["evaluations"] and r["best_step"] == 0 and r["accepted"] == 0 and r["trace_energy"] == [want["energy"]]
            assert got["best_chain"][p] == 0 and np.array_equal(got["y"][p], want["y"])


def test_the_best_never_rises(runs):
    for (name, kind), (a, _) in runs.items():
        for row in a["chains"]:
            for r in row:
                tr = np.asarray(r["trace_energy"])
                assert r["energy"] == tr[np.isfinite(tr)].min() and r["energy"] <= r["energy_start"] == tr[0]
                best, cur = tr[0], tr[0]
                for m, (e, acc, nb) in enumerate(zip(tr[1:], r["accept"], r["new_best"]), 1):
                    assert nb == int(np.isfinite(e) and e < best)
                    best = min(best, e) if np.isfinite(e) else best
                    cur = e if acc else cur
                    assert best <= cur
                assert r["energy_cur"] == cur and r["accepted"] == sum(r["accept"])
                assert r["best_step"] == (int(np.argmin(tr)) if r["energy"] < tr[0] else 0)
        for p, row in enumerate(a["chains"]):
            assert a["energy"][p] == min(r["energy"] for r in row) == row[a["best_chain"][p]]["energy"]
            assert all(r["energy"] > a["energy"][p] for r in row[:a["best_chain"][p]])     # the lowest index on a tie


def test_a_chain_does_not_depend_on_the_number_of_chains_or_its_place(cases, runs):
    name = "P2_A257_L6_T2"
    c, (seed, st) = cases[name], sr.GPU_CASES[name]
    kw = {k: v for k, v in st.items() if k != "chains"}
    full = runs[name, "trajectory"][0]["chains"]
    one = sr.search(c, chains=1, seed=seed, **kw)["chains"]
    alone = sr.search(c, x=c["x"][1:2], chains=2, pose0=1, seed=seed, **kw)["chains"]
    for key in ("entity", "accept", "trace_energy", "best_step"):
        assert one[0][0][key] == full[0][0][key] and one[1][0][key] == full[1][0][key]
        assert alone[0][1][key] == full[1][1][key]
    assert np.array_equal(alone[0][1]["y_best"], full[1][1]["y_best"])
    other = sr.search(c, chains=1, seed=seed + 1, **kw)["chains"]
    assert [r[0]["entity"] for r in other] != [r[0]["entity"] for r in one]


def test_temperature_limits(cases):
    name = "P2_A65_L1_T0"
    c, (seed, st) = cases[name], sr.GPU_CASES[name]
    kw = {k: v for k, v in st.items() if k not in ("chains", "temperature")}
    hot = sr.search(c, chains=1, seed=seed, temperature=float("inf"), **kw)["chains"]
    cold = sr.search(c, chains=1, seed=seed, temperature=1e-12, **kw)["chains"]
    for (h,), (k,) in zip(hot, cold):
        assert all(h["accept"]) and h["accepted"] == st["steps"]
        tr = np.asarray(k["trace_energy"])
        cur = tr[0]
        for e, acc in zip(tr[1:], k["accept"]):                                         # nothing uphill is accepted
            assert acc == int(e <= cur)
            cur = e if acc else cur


def test_default_rotate_amp_is_vinas_scaling(cases):
    c = cases["P3_A300_L12_T3"]
    y = c["x"][0].astype(np.float64)[c["lig_idx"]]
    r = np.sqrt(((y - y.mean(0)) ** 2).sum(-1).mean())
    assert r > 1.0 and sr.default_rotate_amp(c, c["x"][0]) == 2.0 / r
    assert sr.default_rotate_amp(cases["P2_A65_L1_T0"], cases["P2_A65_L1_T0"]["x"][0]) == 2.0           # one atom: r_gyr = 0
    from physdock_amd.refine import VinaRefine
    from physdock_amd.scoring import VinaScore
    v = VinaScore.from_types(c["types"], c["lig_idx"], c["rec_mask"], c["n_rot"], ligand_active=c["lig_active"])
    got = VinaRefine.from_vina(v, c["bonds"]).default_rotate_amp(torch.from_numpy(c["x"]))
    assert abs(got - 2.0 / r) <= 1e-12


def test_argument_validation(cases):
    from physdock_amd.refine import VinaRefine
    from physdock_amd.scoring import VinaScore
    c = cases["P2_A257_L6_T2"]
    v = VinaScore.from_types(c["types"], c["lig_idx"], c["rec_mask"], 2.0, ligand_active=c["lig_active"])
    r = VinaRefine.from_vina(v, c["bonds"])
    x = torch.zeros(1, 257, 3)
    for bad in (dict(chains=0), dict(chains=65), dict(steps=-1), dict(pose0=-1), dict(temperature=0.0), dict(temperature=float("nan")),
                dict(translate_amp=-1.0), dict(rotate_amp=-0.1), dict(max_iters=-1), dict(grad_tol=-1.0), dict(max_step=0.0),
                dict(steps_per_launch=0)):
        with pytest.raises(ValueError, match="VinaRefine.search"):
            r.search(x, **bad)
    with pytest.raises(ValueError, match="pose atoms"):
        r.search(torch.zeros(1, 256, 3))
    import inspect
    sig = inspect.signature(VinaRefine.search).parameters
    assert {k: sig[k].default for k in sr.DEFAULTS} == sr.DEFAULTS and sig["rotate_amp"].default is None and sig["seed"].default == 0


def test_abi_symbols():
    from physdock_amd import _lib
    new = {"pd_vina_search", "pd_vina_search_select"}
    assert new <= set(_lib.header_symbols())
    L = _lib.lib()
    new |= {"pd_vina_search_workspace_numel"}
    assert new <= set(_lib.SYMBOLS) and all(hasattr(L, s) for s in new)
    assert _lib.ABI_VERSION == 11
    numel = L.pd_vina_search_workspace_numel
    assert numel(2, 3, 12, 3) == 2 * 3 * (81 + 108 + 8) and numel(1, 64, 1, 0) == 64 * (36 + 9 + 8)
    assert numel(65535, 1, 1024, 58) == 65535 * (4096 + 9216 + 8)
    assert numel(0, 1, 1, 0) == numel(1, 0, 1, 0) == numel(1, 1, 0, 0) == numel(1, 1, 1, -1) == -1
    assert numel(1, 65, 1, 0) == numel(1024, 64, 1, 0) == numel(1, 1, 1025, 0) == numel(1, 1, 1, 59) == -3


def test_redock_search_needs_refine_before_anything_is_sampled():
    from physdock_amd import driver

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name})")

    for search in (True, {"chains": 2}):
        with pytest.raises(ValueError, match="refine="):
            driver.redock(Untouchable(), {}, search=search)
        with pytest.raises(ValueError, match="refine="):
            driver._RedockState({}, {}, search=search)
    with pytest.raises(ValueError, match="search= takes"):
        driver.redock(Untouchable(), {}, search="yes", refine=object())
