"""pd_dit_bounds (csrc/sampler.hip: dit_bounds_rows_kernel + dit_bounds_kernel) at kernel level, straight on the C ABI.

The bounds it writes decide the operand scales of the two-part fp16 format of every DiT launch; one that is slightly too small
faults nowhere and turns nothing NaN until an operand happens to overflow.  The end-to-end guard (tests/test_bounds_guard_gpu.py)
feeds ordinary activations, which sit 2^3 .. 2^12 under the bound; here the kernel is compared with a float64 statement of the
formulas (tests/dit_bounds_ref.py, itself checked without a GPU by tests/test_dit_bounds_ref_cpu.py) on shapes that take every
guard of the kernel - table rows across three 64-row slabs, C and hidden that are no multiple of 32 in both orders, a row pitch
with NaN padding - and against an adversary that drives a float64 DiT block with the inputs that maximise each operand.

* parity: out[..., 2:6] against dit_bounds64 under the rule of tests/test_sampler_kernels_gpu.py,
  |dev - ref64| <= TOL_FACTOR E + TOL_FLOOR_ULPS ulp32(max|ref64|), E = max|ref32 - ref64| of the float32 twin per (row, block);
* soundness of the rounding: out[..., 2:6] >= the bounds WITHOUT margins in float64, everywhere, no tolerance - that is what the
  1.001 / 1.002 factors promise;
* soundness against the adversary: nothing it reaches exceeds out; the achieved-to-bound ratios are printed, not asserted;
* the parts without arithmetic (q / k constants, the two zero slots, sentinels), a dirty scratch buffer, reproducibility, row
  and weight-row permutations, slab invariance and the argument refusals are compared bit for bit.

Every output and scratch buffer is one row longer than needed and sentinel-filled.

Not covered:
* nrows > 65535, the grid.y limit of the second kernel: step counts are three orders of magnitude below it.
* Non-finite table or weight entries: fmaxf drops NaN, so a NaN table yields finite bounds; the first-call finite check of
  model.py is the guard for that and is not changed here.
* The host-side q / k constants (packing.dit_qk_bounds_host): plain Python, exercised end to end.
"""
import pytest
import torch

import dit_bounds_ref as dr
import test_sampler_kernels_gpu as gk
from test_sampler_kernels_gpu import P, S, body, dev, is_sentinel, ok, sentinel

pytestmark = pytest.mark.gpu

CASE_IDS = sorted(dr.CASES)
PD_ERR_ARG = gk.PD_ERR_ARG


@pytest.fixture(scope="module")
def L():
    from physdock_amd import ops
    return ops._lib.init()


def run(L, c, tab=None, wstack=None, vh_fill=0.0):
    """one pd_dit_bounds call on the case's shape (optionally with another table / other weights of that shape): the output rows
    [nrows, nblocks, 8] on the CPU, after the sentinel checks of both buffers.  The live part of vh is pre-filled with vh_fill."""
    tab = c["tab"] if tab is None else tab
    wstack = c["wstack"] if wstack is None else wstack
    nrows, ld = tab.shape
    nb, C, H = c["nblocks"], c["C"], c["hidden"]
    assert ld == c["ld"] and wstack.shape == (nb, C + 2 * H, C)
    tab_d, w_d, consts_d = dev(tab), dev(wstack), dev(c["consts"])
    out, vh = sentinel(nrows, nb, 8), sentinel(nrows, nb, 2)
    vh[:-1] = vh_fill
    ok(L.pd_dit_bounds(P(tab_d), nrows, ld, nb, C, H, P(consts_d), P(w_d), P(vh), P(out), S()), "pd_dit_bounds")
    o = body(out).cpu()
    assert is_sentinel(vh[-1]).all(), "the row behind the scratch buffer was written"
    return o


@pytest.mark.parametrize("case", CASE_IDS)
def test_parity_soundness_and_exact_parts(L, case):
    c = dr.bounds_case(case)
    ref64, exact64, ref32 = dr.case_reference(case)
    o = run(L, c)
    tag = f"case {case} C={c['C']} hidden={c['hidden']} nblocks={c['nblocks']} nrows={c['nrows']} ld={c['ld']}"
    # 1. parity, E and the ulp floor per (row, block)
    assert (gk.TOL_FACTOR, gk.TOL_FLOOR_ULPS) == (dr.TOL_FACTOR, dr.TOL_FLOOR_ULPS)
    flat = lambda t: t[..., 2:6].reshape(-1, 4)
    bound, _ = gk.tolerance(flat(ref32), flat(ref64), per_sample=True)
    assert torch.equal(bound.reshape(-1), dr.parity_tolerance(ref32, ref64)[0].reshape(-1))      # what the CPU mutation check used
    gk.check_close("pd_dit_bounds", tag, flat(o), flat(ref32), flat(ref64), per_sample=True)
    # 2. the margins cover the kernel's own rounding
    o64 = o.double()
    short = exact64[..., 2:6] - o64[..., 2:6]
    assert (short <= 0).all(), (tag, "below the exact bound by", float(short.max()), (short > 0).nonzero()[:4].tolist())
    # 3. nothing the adversary reaches exceeds the device bound
    adv = dr.case_adversary(case)
    ratio = adv / o64[..., 2:6]
    print(f"ADVERSARY | {tag} | achieved / device bound, worst  v {float(ratio[..., 0].max()):.4f} | y {float(ratio[..., 1].max()):.4f} | "
          f"y' {float(ratio[..., 2].max()):.4f} | h {float(ratio[..., 3].max()):.4f} |")
    assert (adv <= o64[..., 2:6]).all(), (tag, float(ratio.max()), (adv > o64[..., 2:6]).nonzero()[:4].tolist())
    # 4. the parts without arithmetic
    assert torch.equal(o[..., 0:2], c["consts"][None, :, 0:2].expand(c["nrows"], -1, -1))
    assert torch.equal(o[..., 6:8], torch.zeros(c["nrows"], c["nblocks"], 2))


@pytest.mark.parametrize("case", CASE_IDS)
def test_dirty_scratch_does_not_survive(L, case):
    c = dr.bounds_case(case)
    clean = run(L, c)
    assert torch.equal(run(L, c, vh_fill=1e30), clean)
    assert torch.equal(run(L, c, vh_fill=float("nan")), clean)          # 0x7fc00000: above every finite pattern as an integer
    assert torch.equal(run(L, c, vh_fill=-float("nan")), clean)


@pytest.mark.parametrize("case", CASE_IDS)
def test_reproducible_and_order_free(L, case):
    c = dr.bounds_case(case)
    C, H, nrows = c["C"], c["hidden"], c["nrows"]
    first = run(L, c)
    assert torch.equal(run(L, c), first)
    g = torch.Generator().manual_seed(40 + case)
    # table rows permuted: the output rows move with them
    rp = torch.randperm(nrows, generator=g)
    assert nrows == 1 or not torch.equal(rp, torch.arange(nrows))
    assert torch.equal(run(L, c, tab=c["tab"][rp].contiguous()), first[rp])
    # weight rows permuted within each stack (W1 and W3 by the same permutation: the h bound pairs row n of one with row n of the
    # other): maxima are order-free, and a row's sums do not depend on which wave or slot holds it
    pv, ph = torch.randperm(C, generator=g), torch.randperm(H, generator=g)
    idx = torch.cat([pv, C + ph, C + H + ph])
    assert not torch.equal(idx, torch.arange(C + 2 * H))
    assert torch.equal(run(L, c, wstack=c["wstack"][:, idx].contiguous()), first)


def test_slab_invariance(L):
    c = dr.bounds_case(3)
    assert c["nrows"] == 130
    full = run(L, c)
    assert torch.equal(run(L, c, tab=c["tab"][:64].contiguous()), full[:64])
    assert torch.equal(run(L, c, tab=c["tab"][129:130].contiguous()), full[129:130])


def test_argument_refusals(L):
    c = dr.bounds_case(1)
    nrows, ld, nb, C, H = c["nrows"], c["ld"], c["nblocks"], c["C"], c["hidden"]
    assert ld == nb * 6 * C
    tab, w, consts = dev(c["tab"]), dev(c["wstack"]), dev(c["consts"])
    out, vh = sentinel(nrows, nb, 8), sentinel(nrows, nb, 2)
    t, k, W, v, o, s = P(tab), P(consts), P(w), P(vh), P(out), S()
    f = L.pd_dit_bounds
    bad = {
        "null tab": f(None, nrows, ld, nb, C, H, k, W, v, o, s),
        "null consts": f(t, nrows, ld, nb, C, H, None, W, v, o, s),
        "null wstack": f(t, nrows, ld, nb, C, H, k, None, v, o, s),
        "null vh": f(t, nrows, ld, nb, C, H, k, W, None, o, s),
        "null out": f(t, nrows, ld, nb, C, H, k, W, v, None, s),
        "nrows=0": f(t, 0, ld, nb, C, H, k, W, v, o, s),
        "nrows=-1": f(t, -1, ld, nb, C, H, k, W, v, o, s),
        "nblocks=0": f(t, nrows, ld, 0, C, H, k, W, v, o, s),
        "nblocks=-1": f(t, nrows, ld, -1, C, H, k, W, v, o, s),
        "C=0": f(t, nrows, ld, nb, 0, H, k, W, v, o, s),
        "C=-32": f(t, nrows, ld, nb, -32, H, k, W, v, o, s),
        "hidden=0": f(t, nrows, ld, nb, C, 0, k, W, v, o, s),
        "hidden=-1": f(t, nrows, ld, nb, C, -1, k, W, v, o, s),
        "ld one short": f(t, nrows, nb * 6 * C - 1, nb, C, H, k, W, v, o, s),
    }
    wrong = {name: rc for name, rc in bad.items() if rc != PD_ERR_ARG}
    assert not wrong, wrong
    torch.cuda.synchronize()
    assert is_sentinel(out).all() and is_sentinel(vh).all()
    # a valid call right after still succeeds
    assert torch.equal(run(L, c), run(L, c))
