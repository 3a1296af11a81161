"""FlexSearch on the host: the written definition tests/flex_search_ref.py against its own invariants and against the two definitions it
joins, and the conditioning guard of the GPU tests (tests/test_flex_search_gpu.py).  No GPU: nothing here launches a kernel.

The guard is that of tests/test_vina_search_cpu.py with the same numbers (vina_search_ref.U_MARGIN, E_MARGIN): for each (case, seed,
settings) of `flex_search_ref.GPU_CASES`, and for the settings of the "proposal alone" test, the run with ascending summation and its
twin with reversed summation take identical decisions and end within 1e-8 A of each other, every Metropolis test keeps |u_4 - p| >=
1e-6, every strict comparison of two energies a gap of at least 1e-9 kcal/mol - or compares identical bits (a proposal that moved
nothing from a converged point).  These are conditions on the inputs: a seed that does not meet them is replaced here, on the CPU."""
import numpy as np
import pytest
import torch

import flex_refine_ref as ref
import flex_search_ref as fs
import vina_refine_ref as vrr
import vina_search_ref as vs

PROPOSAL = dict(steps=1, max_iters=0, temperature=float("inf"))
DECISIONS = ("entity", "accept", "new_best", "iterations", "status", "start_iterations", "start_status", "best_step", "accepted", "evaluations")


@pytest.fixture(scope="module")
def cases():
    return {name: ref.make_case(name) for name in set(fs.GPU_CASES) | {fs.BEHAVIOUR[0]}}


@pytest.fixture(scope="module")
def runs(cases):
    """(case, kind) -> (forward, reversed) searches; kind "trajectory": the case's settings, "proposal": the proposal alone"""
    out = {}
    for name, (seed, st) in fs.GPU_CASES.items():
        for kind, kw in (("trajectory", st), ("proposal", dict(st, **PROPOSAL))):
            out[name, kind] = (fs.search(cases[name], seed=seed, **kw), fs.search(cases[name], seed=seed, order=-1, **kw))
    return out


def guard(a, b, where):
    assert a["best_chain"] == b["best_chain"], where
    for p, (row_a, row_b) in enumerate(zip(a["chains"], b["chains"])):
        for k, (ra, rb) in enumerate(zip(row_a, row_b)):
            for key in DECISIONS:
                assert ra[key] == rb[key], (where, p, k, key, ra[key], rb[key])
            for key in ("y_best", "y_cur", "y_start"):
                fin = np.isfinite(ra[key])
                assert np.array_equal(fin, np.isfinite(rb[key])) and np.abs(ra[key][fin] - rb[key][fin]).max() <= 1e-8, (where, p, k, key)
            for r in (ra, rb):
                assert all(abs(u - q) >= fs.U_MARGIN for u, q in zip(r["u4"], r["p"])), (where, p, k, "Metropolis margin")
                for gap, exact in zip(r["gaps"], r["exact"]):
                    assert gap >= fs.E_MARGIN or (gap == 0.0 and exact), (where, p, k, "energy gap", gap)
        for r in (row_a, row_b):                                                       # the choice among the chains
            e = np.sort([v["energy"] for v in r])
            assert all(g >= fs.E_MARGIN or g == 0.0 for g in np.diff(e)), (where, p, np.diff(e))


def test_the_cases_are_the_ones_the_issue_names(cases):
    assert set(fs.GPU_CASES) == {"small", "rigid_ligand", "no_flex", "over_block", "full_chart"}
    for name, (seed, st) in fs.GPU_CASES.items():
        assert st["chains"] == 3 and st["steps"] <= 6 and st["max_iters"] <= 10, name
    assert fs.GPU_CASES["full_chart"][1]["steps"] == 2 and fs.GPU_CASES["full_chart"][1]["max_iters"] == 3
    c = cases["small"]
    assert (c["x"].shape[0], c["x"].shape[1], c["T"], c["S"]) == (3, 96, 2, 4)
    assert cases["rigid_ligand"]["T"] == 0 and cases["no_flex"]["S"] == 0 and cases["no_flex"]["F"] == 0
    assert cases["over_block"]["L"] + cases["over_block"]["F"] > 256 and 6 + cases["full_chart"]["T"] + cases["full_chart"]["S"] == 64
    assert (fs.U_MARGIN, fs.E_MARGIN) == (vs.U_MARGIN, vs.E_MARGIN)


def test_conditioning_guard(cases, runs):
    seen = dict(rejected=0, uphill=0, improved=0, side_chain_shown=0)
    for (name, kind), (a, b) in runs.items():
        guard(a, b, (name, kind))
        T = cases[name]["T"]
        for row in a["chains"]:
            for r in row:
                if kind == "trajectory":
                    seen["rejected"] += len(r["accept"]) - sum(r["accept"])
                    seen["uphill"] += sum(1 for acc, q in zip(r["accept"], r["p"]) if acc and q < 1.0)
                else:
                    seen["improved"] += r["best_step"]
                    seen["side_chain_shown"] += int(r["best_step"] == 1 and r["entity"][0] >= 2 + T)
    assert seen["rejected"] >= 1 and seen["uphill"] >= 1 and seen["improved"] >= 1, seen
    assert seen["side_chain_shown"] >= 1, "no side-chain proposal lowers the energy: the proposal-alone test would show none in x_chains"


def test_without_flexible_residues_it_is_the_rigid_search(cases, runs):
    name = "P2_A257_L6_T2"
    assert ref.CASES["no_flex"]["base"] == name and fs.GPU_CASES["no_flex"][0] == 37
    seed, st = fs.GPU_CASES["no_flex"]
    rigid = vs.search(vrr.make_case(name), seed=seed, **{k: v for k, v in st.items() if k != "chi_amp"})
    got = runs["no_flex", "trajectory"][0]
    assert got["best_chain"] == rigid["best_chain"]
    for row_a, row_b in zip(got["chains"], rigid["chains"]):
        for ra, rb in zip(row_a, row_b):
            for key in DECISIONS:
                assert ra[key] == rb[key], key
            assert np.abs(ra["y_best"] - rb["y_best"]).max() <= 1e-8 and ra["moved_flex"] == 0.0
    assert np.abs(got["y"] - rigid["y"]).max() <= 1e-8


def test_entities_cover_the_chart_and_nothing_else(cases):
    for name in ("small", "rigid_ligand", "no_flex"):
        c = cases[name]
        T, S = c["T"], c["S"]
        drawn = [fs.draw(5, q, k, m, T, S) for q in range(4) for k in range(4) for m in range(1, 21)]
        assert {e for e, _, _ in drawn} == set(range(2 + T + S)), name
        for (e, u, w), (e0, u0, w0) in zip(drawn[:20], [vs.draw(5, 0, 0, m, T) for m in range(1, 21)]):
            assert u == u0 and w == w0 and (S > 0 or e == e0)                             # the words are VinaSearch's
    u = [0.0, 0.75, 0.25, 1.0 - 2.0 ** -33, 0.5]
    T, S = 2, 3
    for e in range(2 + T + S):
        s = fs.proposal(e, u, T, S, 2.0, 0.5, 0.25)
        lo, hi = (0, 3) if e == 0 else ((3, 6) if e == 1 else (6 + e - 2, 6 + e - 1))
        amp = 2.0 if e == 0 else (0.5 if e == 1 else (np.pi if e - 2 < T else 0.25))
        assert not s[:lo].any() and not s[hi:].any() and s[lo] == amp * 0.5 and np.abs(s).max() <= amp
    assert fs.proposal(4, u, 2, 3, 2.0, 0.5)[8] == np.pi * 0.5                            # the default chi_amp


def test_steps_zero_is_refine(cases):
    c = cases["small"]
    seed, st = fs.GPU_CASES["small"]
    got = fs.search(c, chains=2, steps=0, seed=seed, **{k: v for k, v in st.items() if k not in ("steps", "chains")})
    for p in range(c["x"].shape[0]):
        want = ref.refine(c, c["x"][p].astype(np.float64), max_iters=st["max_iters"])
        for r in got["chains"][p]:
            assert np.array_equal(r["y_best"], want["y"]) and r["energy"] == want["energy"] == r["energy_start"]
            assert r["evaluations"] == want["evaluations"] and r["best_step"] == 0 and r["accepted"] == 0
            assert r["moved"] == want["moved"] and r["moved_flex"] == want["moved_flex"]
        assert got["best_chain"][p] == 0


def test_a_side_chain_proposal_finds_what_the_local_refinement_cannot(cases):
    """the behaviour the feature is for, with the reference alone: in a chain of the `across` case the best comes from a chi proposal,
    ends more than 0.1 kcal/mol below FlexRefine.refine's minimum of the same pose and has moved the side chain by more than 0.1 A"""
    name, seed, st = fs.BEHAVIOUR
    c = cases[name]
    a, b = fs.search(c, seed=seed, **st), fs.search(c, seed=seed, order=-1, **st)
    guard(a, b, name)
    found = []
    for p, row in enumerate(a["chains"]):
        local = ref.refine(c, c["x"][p].astype(np.float64), max_iters=st["max_iters"])
        assert all(r["energy_start"] == local["energy"] for r in row)
        for k, r in enumerate(row):
            if r["best_step"] > 0 and r["entity"][r["best_step"] - 1] >= 2 + c["T"]:
                found.append((p, k, local["energy"] - r["energy"], r["moved_flex"]))
    assert any(gain > 0.1 and mf > 0.1 for _, _, gain, mf in found), found


def test_the_reference_on_a_non_finite_movable_coordinate(cases):
    """what the GPU test of a non-finite coordinate compares with.  A pair at a non-finite distance is no pair, so E stays finite and
    the Metropolis test goes on as ever; what the coordinate does is end every descent before its first step (status 2, no iteration,
    one evaluation).  The decisions are kept out of roundoff's reach as for every other case."""
    c = cases["small"]
    seed, st = fs.GPU_CASES["small"]
    for row in (3, c["L"] + 2):
        x = c["x"][:1].copy()
        x[0, c["mov_idx"][row]] = np.nan
        a, b = fs.search(c, x=x, seed=seed, **st), fs.search(c, x=x, seed=seed, order=-1, **st)
        guard(a, b, ("nan", row))
        for r in a["chains"][0]:
            assert r["start_status"] == 2 and r["start_iterations"] == 0 and set(r["status"]) == {2} and not any(r["iterations"])
            assert r["evaluations"] == st["steps"] + 1 and np.isfinite(r["trace_energy"]).all()


def flex_refine_of(c, device=None):
    from physdock_amd import FlexRefine
    return FlexRefine.from_tables(c["types"], c["lig_idx"], c["rec_mask"], c["lig_active"], c["n_rot"], c["rot"][:c["T"]], c["sets"][:c["T"]],
                                  c["intra"], c["rec_bonds"], c["residues"], device=device)


def test_argument_validation(cases):
    import inspect
    import math
    from physdock_amd import FlexRefine
    f = flex_refine_of(cases["small"])
    x = torch.zeros(1, 96, 3)
    for bad in (dict(chains=0), dict(chains=65), dict(steps=-1), dict(pose0=-1), dict(temperature=0.0), dict(temperature=float("nan")),
                dict(translate_amp=-1.0), dict(rotate_amp=-0.1), dict(chi_amp=-0.1), dict(chi_amp=float("nan")), dict(max_iters=-1),
                dict(grad_tol=-1.0), dict(max_step=0.0), dict(steps_per_launch=0), dict(workspace_bytes=0)):
        with pytest.raises(ValueError, match="FlexRefine.search"):
            f.search(x, **bad)
    with pytest.raises(ValueError, match="pose atoms"):
        f.search(torch.zeros(1, 95, 3))
    sig = inspect.signature(FlexRefine.search).parameters
    assert list(sig)[1:] == ["x_pred", "chains", "steps", "seed", "temperature", "translate_amp", "rotate_amp", "chi_amp", "max_iters", "grad_tol",
                             "max_step", "steps_per_launch", "pose0", "trace", "workspace_bytes"]
    assert {k: sig[k].default for k in fs.DEFAULTS} == fs.DEFAULTS and sig["chi_amp"].default == math.pi
    assert sig["rotate_amp"].default is None and sig["seed"].default == 0 and sig["steps_per_launch"].default is None
    assert sig["pose0"].default == 0 and sig["trace"].default is False and sig["workspace_bytes"].default == 256 << 20


def test_abi_symbols():
    from physdock_amd import _lib
    import os
    new = {"pd_vina_flex_search", "pd_vina_flex_search_select"}
    assert new <= set(_lib.header_symbols())                                            # (the parser lists the `int` functions)
    new |= {"pd_vina_flex_search_workspace_numel"}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "physdock_hip.h")).read()
    assert "long long pd_vina_flex_search_workspace_numel(int P, int K, int M, int N);" in header
    L = _lib.lib()
    assert new <= set(_lib.SYMBOLS) and all(hasattr(L, s) for s in new)
    assert _lib.ABI_VERSION == 11
    numel = L.pd_vina_flex_search_workspace_numel
    assert numel(2, 3, 22, 6) == 2 * 3 * (144 + 198 + 8) and numel(1, 1, 1024, 58) == 13320 and numel(1, 64, 1, 0) == 64 * (36 + 9 + 8)
    assert numel(65535, 1, 1024, 58) == 65535 * 13320                                   # no int holds the byte count
    assert numel(0, 1, 1, 0) == numel(1, 0, 1, 0) == numel(1, 1, 0, 0) == numel(1, 1, 1, -1) == -1
    assert numel(1, 65, 1, 0) == numel(1024, 64, 1, 0) == numel(1, 1, 1025, 0) == numel(1, 1, 1, 59) == -3


def test_redock_flex_search_needs_flex_before_anything_is_sampled():
    import inspect
    from physdock_amd import driver

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name})")

    for spec in (True, {"chains": 2}):
        with pytest.raises(ValueError, match="flex="):
            driver.redock(Untouchable(), {}, flex_search=spec)
        with pytest.raises(ValueError, match="flex="):
            driver._RedockState({}, {}, flex_search=spec)
    with pytest.raises(ValueError, match="flex_search= takes"):
        driver.redock(Untouchable(), {}, flex_search="yes", flex=object())
    assert inspect.signature(driver.redock).parameters["flex_search"].default is None
    assert inspect.signature(driver._RedockState.__init__).parameters["flex_search"].default is None
