"""float64 statement of pd_dit_bounds (csrc/sampler.hip), an adversary that tries to break the bounds, and the test inputs.

pd_dit_bounds derives, from the AdaLN table of a sample_diffusion call and the (linear_v | w1 | w3) weights of every DiT block,
magnitude bounds that hold for ANY activation.  The table (packing.adaln) holds per block [shift1 | w1 | gate1 | shift2 | w2 | gate2],
C columns each, with the +1 of AdaLN-Zero already folded into w.  With x^ = LayerNorm(x) without affine (||x^||_2 <= sqrt(C),
|x^_k| <= sqrt(C - 1)) and y = w x^ + shift,

    R(W_n; w, s) = sqrt(C) ||W_n o w||_2 + |W_n . s|  >=  |W_n . y|            (Cauchy-Schwarz per output row)

and the eight entries per (table row, block) are

    [0], [1]  consts[b][0], consts[b][1]                  (q and k bounds, weight-only, computed on the host)
    [2]       1.001 max_n R(Wv_n; w1, s1)                 (|v_n|, and |o| as a convex combination of v rows)
    [3]       1.001 sqrt(C) max|w1| + max|s1|             (|y_k|)
    [4]       1.001 sqrt(C) max|w2| + max|s2|             (|y'_k|)
    [5]       1.002 max_n R(W1_n; w2, s2) R(W3_n; w2, s2) (|h_n| = |silu(a_n) b_n| <= |a_n| |b_n|)
    [6], [7]  0

1.001 and 1.002 are the kernel's float32 constants taken as doubles.  Nothing here follows the kernel's loops: the sums are
whole-tensor torch reductions in float64 (dit_bounds64) or float32 (dit_bounds32, the "what fp32 alone costs" twin of the
tolerance rule in tests/test_sampler_kernels_gpu.py).

adversary64 states the DiT block in float64 - LayerNorm without affine, y = w x^ + shift, v = Wv y, h = silu(W1 y') (W3 y') - and
pushes a fixed family of worst-case inputs through it; what it reaches must stay under the bounds, and on shift = 0 rows it reaches
them to within the centring loss, so a bound that is too small anywhere along the way is caught.

The ``bounds_case`` generator returns CPU tensors only; tests/test_dit_bounds_ref_cpu.py asserts its conditions without a GPU and
tests/test_dit_bounds_kernels_gpu.py runs the kernel on it.
"""
import functools
import math

import numpy as np
import torch

M1 = float(np.float32(1.001))          # the margins as the kernel holds them
M2 = float(np.float32(1.002))
GROUP = 32                             # k per staged chunk of the kernel, and weight rows per workgroup

ORDINARY, SHIFT0, OUTLIER = 0, 1, 2

#: the shapes of the issue; pad = table columns behind the last block (NaN, never read)
CASES = {
    1: dict(C=32, hidden=128, nblocks=2, nrows=1, pad=0),
    2: dict(C=40, hidden=72, nblocks=3, nrows=65, pad=7),
    3: dict(C=64, hidden=32, nblocks=1, nrows=130, pad=0),
    4: dict(C=128, hidden=384, nblocks=2, nrows=64, pad=0),
    5: dict(C=512, hidden=1408, nblocks=1, nrows=3, pad=0),
}


# ------------------------------------------------------------------ layout
def split_table(tab, b, C):
    """(shift1, w1, gate1, shift2, w2, gate2) of block b, each [..., C]"""
    return tuple(tab[..., (6 * b + i) * C:(6 * b + i + 1) * C] for i in range(6))


def split_weights(wstack, b, C, hidden):
    """(Wv [C, C], W1 [hidden, C], W3 [hidden, C]) of block b"""
    W = wstack[b]
    return W[:C], W[C:C + hidden], W[C + hidden:C + 2 * hidden]


def last_group_start(n):
    """first index of the last (possibly partial) group of 32 among n"""
    return GROUP * ((n - 1) // GROUP)


# ------------------------------------------------------------------ the bounds
def row_bound(W, w, s, C):
    """R(W_n; w, s) for every table row r and weight row n: [nrows, N] from W [N, C], w and s [nrows, C]"""
    norm = ((W[None] * w[:, None]) ** 2).sum(-1).sqrt()
    return math.sqrt(C) * norm + (s @ W.T).abs()


def _bounds(tab, consts, wstack, C, hidden, m1, m2):
    nrows, nb = tab.shape[0], wstack.shape[0]
    out = torch.zeros(nrows, nb, 8, dtype=tab.dtype)
    for b in range(nb):
        s1, w1, _, s2, w2, _ = split_table(tab, b, C)
        Wv, W1, W3 = split_weights(wstack, b, C, hidden)
        out[:, b, 0], out[:, b, 1] = consts[b, 0], consts[b, 1]
        out[:, b, 2] = m1 * row_bound(Wv, w1, s1, C).amax(1)
        out[:, b, 3] = m1 * math.sqrt(C) * w1.abs().amax(1) + s1.abs().amax(1)
        out[:, b, 4] = m1 * math.sqrt(C) * w2.abs().amax(1) + s2.abs().amax(1)
        out[:, b, 5] = m2 * (row_bound(W1, w2, s2, C) * row_bound(W3, w2, s2, C)).amax(1)
    return out


def dit_bounds64(tab, consts, wstack, C, hidden):
    """(bounds with the kernel's margins, exact64 = the same without margins), each [nrows][nblocks][8] float64"""
    t, c, W = tab.double(), consts.double(), wstack.double()
    return _bounds(t, c, W, C, hidden, M1, M2), _bounds(t, c, W, C, hidden, 1.0, 1.0)


def dit_bounds32(tab, consts, wstack, C, hidden):
    """the same formulas, with margins, in torch float32 on the CPU"""
    return _bounds(tab.float(), consts.float(), wstack.float(), C, hidden, M1, M2)


# ------------------------------------------------------------------ the adversary
def layer_norm64(x, eps=0.0):
    x = x.double()
    x = x - x.mean(-1, keepdim=True)
    return x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)


@functools.lru_cache(maxsize=None)
def _random_normalised(C):
    """a few hundred random inputs through LayerNorm (eps = 1e-5): Gaussian, and heavy-tailed (log-normal amplitudes, offsets)"""
    g = torch.Generator().manual_seed(77 + C)
    gauss = torch.randn(128, C, generator=g, dtype=torch.float64)
    heavy = torch.randn(128, C, generator=g, dtype=torch.float64) * torch.exp(2.0 * torch.randn(128, C, generator=g, dtype=torch.float64)) \
        + 10.0 * torch.randn(128, 1, generator=g, dtype=torch.float64)
    return layer_norm64(torch.cat([gauss, heavy]), 1e-5)


def _aligned(W, w, C):
    """+- the LayerNorm output that maximises (W_n o w) . x^ for every row n: centre(W_n o w) scaled to length sqrt(C)"""
    u = W * w[None]
    u = u - u.mean(-1, keepdim=True)
    nrm = u.norm(dim=-1, keepdim=True)
    keep = nrm[:, 0] > 0
    xh = math.sqrt(C) * u[keep] / nrm[keep]
    return torch.cat([xh, -xh])


def _one_hots(w, s, C):
    x = torch.zeros(2, C, dtype=torch.float64)
    x[0, int(w.abs().argmax())] = 1.0
    x[1, int(s.abs().argmax())] = 1.0
    xh = layer_norm64(x)
    return torch.cat([xh, -xh])


def adversary64(tab_row, block, wstack, C, hidden):
    """largest (|v_n|, |y_k|, |y'_k|, |h_n|) the float64 DiT block reaches over the input family of the module docstring,
    for one table row [ld] and one block: a float64 tensor [4]"""
    s1, w1, _, s2, w2, _ = split_table(tab_row.double(), block, C)
    Wv, W1, W3 = (W.double() for W in split_weights(wstack, block, C, hidden))
    rand = _random_normalised(C)
    x1 = torch.cat([_aligned(Wv, w1, C), _one_hots(w1, s1, C), rand])
    x2 = torch.cat([_aligned(W1, w2, C), _aligned(W3, w2, C), _one_hots(w2, s2, C), rand])
    y = x1 * w1 + s1
    v = y @ Wv.T
    y2 = x2 * w2 + s2
    h = torch.nn.functional.silu(y2 @ W1.T) * (y2 @ W3.T)
    return torch.stack([v.abs().max(), y.abs().max(), y2.abs().max(), h.abs().max()])


# ------------------------------------------------------------------ cases
def special_rows(nrows):
    """row 0, the last row and the rows on either side of every 64-row boundary"""
    rows = {0, nrows - 1}
    for m in range(64, nrows, 64):
        rows.update(r for r in (m - 1, m, m + 1) if r < nrows)
    return sorted(rows)


@functools.lru_cache(maxsize=None)
def bounds_case(case):
    """The inputs of one shape of CASES (shared and cached: do not write into the tensors).

    tab [nrows, ld] fp32: per (row, block) one of three kinds - ORDINARY (w = 1 + 0.3 N(0,1), shift = 0.3 N(0,1)), SHIFT0 (both shifts
    zero) and OUTLIER (ordinary, with w1[C - 3] and w2[C - 2] times 64: positions in the last k-chunk of 32).  The i-th special row
    (special_rows) is OUTLIER in block i mod nblocks; every other (row, block) alternates ORDINARY / SHIFT0.  Gates are 2 N(0,1);
    the padding behind a row is NaN.
    wstack [nblocks, C + 2 hidden, C] fp32: N(0, 1 / C) rows with their mean taken off; in even blocks row C - 2 of Wv and row hidden - 2 of W1 and of W3
    (the last group of 32 rows) are times 64, with entries of 1.5 * 64 / sqrt(C) at the two outlier columns so that an outlier gain
    always shows in them; odd blocks have no outlier row, so their maxima sit wherever the draw puts them.
    consts [nblocks, 4] fp32: distinct (q, k) bounds, and values in the two unused slots that must not reach the output."""
    p = CASES[case]
    C, hidden, nb, nrows, pad = p["C"], p["hidden"], p["nblocks"], p["nrows"], p["pad"]
    g = torch.Generator().manual_seed(9100 + case)
    ld = 6 * C * nb + pad
    k1, k2 = C - 3, C - 2
    kinds = torch.tensor([[(r + b) % 2 for b in range(nb)] for r in range(nrows)])
    special = special_rows(nrows)
    for i, r in enumerate(special):
        kinds[r, i % nb] = OUTLIER
    tab = torch.full((nrows, ld), float("nan"))
    for b in range(nb):
        blk = torch.randn(nrows, 6, C, generator=g)
        blk[:, (0, 3)] *= 0.3
        blk[:, (1, 4)] = 1.0 + 0.3 * blk[:, (1, 4)]
        blk[:, (2, 5)] *= 2.0
        zero = (kinds[:, b] == SHIFT0).nonzero()[:, 0]
        blk[zero, 0] = 0.0
        blk[zero, 3] = 0.0
        out = (kinds[:, b] == OUTLIER).nonzero()[:, 0]
        blk[out, 1, k1] *= 64.0
        blk[out, 4, k2] *= 64.0
        tab[:, 6 * C * b:6 * C * (b + 1)] = blk.reshape(nrows, 6 * C)
    wstack = torch.randn(nb, C + 2 * hidden, C, generator=g) / math.sqrt(C)
    # zero-mean rows: LayerNorm outputs have zero mean, so the mean of W_n o w is the part of the Cauchy-Schwarz bound that no input
    # can reach; with it near zero the adversary gets close to the bound at every C (the non-vacuity check of the CPU test)
    wstack -= wstack.mean(-1, keepdim=True)
    nv, nh = C - 2, hidden - 2
    for b in range(0, nb, 2):
        for n in (nv, C + nh, C + hidden + nh):
            wstack[b, n] *= 64.0
            sign = torch.sign(wstack[b, n, [k1, k2]])
            wstack[b, n, [k1, k2]] = torch.where(sign == 0, torch.ones(2), sign) * 1.5 * 64.0 / math.sqrt(C)
    consts = torch.tensor([[5.0 + b, 7.5 + 2 * b, 123.0 + b, 456.0 + b] for b in range(nb)])
    return dict(p, case=case, ld=ld, tab=tab.contiguous(), wstack=wstack.contiguous(), consts=consts, kinds=kinds, special=special,
                k1=k1, k2=k2, nv=nv, nh=nh)


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """(ref64 with margins, exact64, ref32), computed once per case and shared"""
    c = bounds_case(case)
    ref64, exact64 = dit_bounds64(c["tab"], c["consts"], c["wstack"], c["C"], c["hidden"])
    return ref64, exact64, dit_bounds32(c["tab"], c["consts"], c["wstack"], c["C"], c["hidden"])


@functools.lru_cache(maxsize=None)
def case_adversary(case):
    """adversary64 of every (row, block) of a case: [nrows, nblocks, 4] for (v, y, y', h), computed once and shared"""
    c = bounds_case(case)
    return torch.stack([torch.stack([adversary64(c["tab"][r], b, c["wstack"], c["C"], c["hidden"]) for b in range(c["nblocks"])])
                        for r in range(c["nrows"])])


# ------------------------------------------------------------------ the tolerance of the parity check
TOL_FACTOR = 4.0           # the two constants of tests/test_sampler_kernels_gpu.py (asserted equal in the GPU test)
TOL_FLOOR_ULPS = 8.0


def parity_tolerance(ref32, ref64):
    """|dev - ref64| <= TOL_FACTOR E + TOL_FLOOR_ULPS ulp32(max|ref64|) over entries 2 .. 5, E and the maximum per (row, block):
    (bound, E), each [nrows, nblocks, 1]"""
    r64 = ref64[..., 2:6]
    E = (ref32[..., 2:6].double() - r64).abs().amax(-1, keepdim=True)
    scale = r64.abs().amax(-1, keepdim=True).float()
    ulp = (torch.nextafter(scale, torch.full_like(scale, float("inf"))) - scale).double()
    return TOL_FACTOR * E + TOL_FLOOR_ULPS * ulp, E
