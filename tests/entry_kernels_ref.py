"""Plain references and test inputs of the model's entry kernels: csrc/features.hip (target_feat, msa_feat, outer_mask, chain_contacts,
pdb_format), csrc/confidence.hip (confidence_pair_init, pair_symmetrize, atom_dist_embed and their *_poses forms), template_feat of
csrc/pair.hip and chirality of csrc/sampler.hip.

torch / Python on the CPU, no device code.  Every function transcribes the formula in the comment above its kernel (or the line of
oracle/features_oracle.py it stands for) as whole-tensor algebra; none follows a kernel's loop structure (chain_contacts takes one
chain pair at a time: a pair is one independent problem, inside it the matrix is whole).  Two kinds of expectation, as in
tests/trunk_glue_ref.py:

* exact - index work, or one IEEE fp32 operation per element that the kernel keeps from contraction (`__f*_rn`), or additions only.
  The reference, taken with ``dtype=torch.float32``, IS that operation done by torch on the CPU; the device result must be
  torch.equal to it.  target_feat, outer_mask, template_feat (d2 = three _rn products, two _rn sums; m = two roundings), the one-hot
  and clamp columns of msa_feat, confidence_pair_init(_poses) with its bin, pair_symmetrize(_poses), pdb_format (Python's
  f"{v:>8.3f}"), chain_contacts (arg_out: the first minimum of the same fp32 expression; between; min_out), atom_dist_embed(_poses)
  (the last two: a chain of single roundings around one sqrtf, which the device rounds correctly; see sqrt_rn for the CPU side),
  and the sign / accept outputs of chirality wherever the float64 volume clears its rounding bound.
* bounded - the atan column of msa_feat only, under the rule of tests/test_sampler_kernels_gpu.py (check_close), unchanged:
  |dev - ref64| <= 4 E + 8 ulp32(max |ref64|), E = max |ref32 - ref64| of the same expression in fp32 on the CPU.

The ``*_case`` functions below are the inputs of tests/test_entry_kernels_gpu.py (CPU tensors only, cached: a case is computed once
and never modified); tests/test_entry_kernels_ref_cpu.py asserts, without a GPU, the conditions they rely on - every planted tie,
midpoint and edge is exact in fp32, every chirality centre clears its bound - and that wrong variants of the operations are caught.
"""
import functools
import math

import numpy as np
import torch

from trunk_glue_ref import F64, gamma

F32 = torch.float32
I64 = torch.int64
INF = float("inf")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _t(v, dtype):
    return torch.as_tensor(v).to(dtype)


def _idx(v):
    return torch.as_tensor(v).long()


def dist2(a, b, dtype=F32):
    """(dx^2 + dy^2) + dz^2 of a - b over the last axis, every product and sum one rounding of `dtype`"""
    sq = (_t(a, dtype) - _t(b, dtype)) ** 2
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def sqrt_rn(v):
    """the correctly rounded square root of `v` in v's own type.  torch.sqrt of an fp32 tensor on the CPU is not (one result in a
    few hundred is off by an ulp, and which one depends on the machine's vector unit), so fp32 goes through float64: a float64 root
    rounded once more to fp32 is the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits)"""
    return torch.sqrt(v.double()).to(v.dtype)


def first_argmin(v, dim=-1):
    """index of the first minimum along `dim` (what torch.argmin documents, spelled out so that nothing rests on it)"""
    n = v.shape[dim]
    shape = [1] * v.dim()
    shape[dim] = n
    pos = torch.arange(n).reshape(shape).expand_as(v)
    return torch.where(v == v.amin(dim, keepdim=True), pos, torch.full_like(pos, n)).amin(dim)


def last_argmin(v, dim=-1):
    """a wrong variant: the last minimum"""
    n = v.shape[dim]
    shape = [1] * v.dim()
    shape[dim] = n
    pos = torch.arange(n).reshape(shape).expand_as(v)
    return torch.where(v == v.amin(dim, keepdim=True), pos, torch.full_like(pos, -1)).amax(dim)


# ------------------------------------------------------------------ features.hip
def one_hot_eq(idx, n_class, dtype=F32):
    """[idx == c] for c in 0 .. n_class - 1: an index outside [0, n_class) gives a row of zeros"""
    return (_idx(idx)[..., None] == torch.arange(n_class)).to(dtype)


def target_feat(restype, profile, deletion_mean, n_class, dtype=F32):
    """[one_hot(restype, n_class) | profile | deletion_mean]"""
    return torch.cat([one_hot_eq(restype, n_class, dtype), _t(profile, dtype), _t(deletion_mean, dtype)[..., None]], dim=-1)


def msa_feat_exact(msa, deletion, inds, n_class, dtype=F32):
    """the first n_class + 1 columns of msa_feat: [one_hot(msa[inds], n_class) | clamp(deletion[inds], 0, 1)]"""
    inds = _idx(inds)
    return torch.cat([one_hot_eq(_idx(msa)[inds], n_class, dtype), _t(deletion, dtype)[inds].clamp(0, 1)[..., None]], dim=-1)


def msa_feat_atan(deletion, inds, two_over_pi, dtype=F64):
    """the last column: atan(deletion[inds] / 3) * two_over_pi, two_over_pi the fp32 number the kernel is handed"""
    s = torch.tensor(float(np.float32(two_over_pi)), dtype=dtype)
    return torch.atan(_t(deletion, dtype)[_idx(inds)] / 3) * s


def outer_mask(m, dtype=F32):
    m = _t(m, dtype)
    return m[:, None] * m[None, :]


def chain_pair_matrix(x, a_mask, i0, i1, j0, j1, dtype=F32):
    """|x_a - x_b| + (1 - mask_a mask_b) 1000 for a in [i0, i1), b in [j0, j1)"""
    d = sqrt_rn(dist2(_t(x, dtype)[i0:i1, None], _t(x, dtype)[None, j0:j1], dtype))
    am = _t(a_mask, dtype)
    return d + (1 - am[i0:i1, None] * am[None, j0:j1]) * 1000


def chain_contacts(x, a_mask, chain_start, pairs, a2t, threshold, T, dtype=F32, argmin=first_argmin, below=torch.lt):
    """(min [n_pairs], arg [n_pairs] int64, between [T, T]): per searched chain pair the smallest entry of chain_pair_matrix and its
    row-major position (first on ties; +inf and -1 for a pair with an empty chain); where min < threshold the tokens of the two
    atoms are bonded, symmetrically"""
    cs, a2t = _idx(chain_start).tolist(), _idx(a2t)
    mins, args, between = [], [], torch.zeros(T, T, dtype=dtype)
    thr = torch.tensor(float(np.float32(threshold)), dtype=dtype)
    for ci, cj in _idx(pairs).reshape(-1, 2).tolist():
        i0, i1, j0, j1 = cs[ci], cs[ci + 1], cs[cj], cs[cj + 1]
        v = chain_pair_matrix(x, a_mask, i0, i1, j0, j1, dtype).reshape(-1)
        if v.numel() == 0:
            mins.append(torch.tensor(INF, dtype=dtype))
            args.append(-1)
            continue
        k = int(argmin(v))
        mins.append(v[k])
        args.append(k)
        if bool(below(v[k], thr)):
            ti, tj = int(a2t[i0 + k // (j1 - j0)]), int(a2t[j0 + k % (j1 - j0)])
            between[ti, tj] = 1
            between[tj, ti] = 1
    return torch.stack(mins) if mins else torch.zeros(0, dtype=dtype), torch.tensor(args, dtype=I64), between


def pdb_field(v, half_up=False):
    """(8 bytes, bad): Python's f"{v:>8.3f}" of one coordinate; what does not fit eight characters, or is not finite, is eight '*'.
    half_up: a wrong variant that rounds the scaled decimal half up instead of converting correctly (half even on the exact value)"""
    v = float(v)
    if math.isfinite(v):
        s = f"{math.copysign(math.floor(abs(v) * 1000 + 0.5) / 1000, v):>8.3f}" if half_up else f"{v:>8.3f}"
        if len(s) == 8:
            return s.encode(), False
    return b"*" * 8, True


def pdb_format(x, tmpl, atom, half_up=False):
    """(out uint8 [B, N, 81], number of bad fields): every record is its template row with columns 31-54 replaced by the three
    coordinates of x[b, atom[n]]"""
    x, atom = _t(x, F32), _idx(atom).tolist()
    rows = torch.as_tensor(tmpl).reshape(-1, 81)
    out = rows[None].repeat(x.shape[0], 1, 1).clone()
    bad = 0
    for b in range(x.shape[0]):
        for n, a in enumerate(atom):
            for f in range(3):
                s, isbad = pdb_field(x[b, a, f], half_up)
                bad += isbad
                out[b, n, 30 + 8 * f:38 + 8 * f] = torch.frombuffer(bytearray(s), dtype=torch.uint8)
    return out, bad


# ------------------------------------------------------------------ pair.hip: template_feat
def template_feat(x, pb, z_mask, is_protein, lower, inf=1e8, dtype=F32, above=torch.gt):
    """[[lower_b < d2 < upper_b] m | m], d2 the squared distance of the pseudo-beta atoms, upper = lower[1:] | inf,
    m = z_mask * (is_protein_i * is_protein_j)"""
    xp = _t(x, dtype)[_idx(pb)]
    d2 = dist2(xp[:, None], xp[None, :], dtype)[..., None]
    lower = _t(lower, dtype)
    upper = torch.cat([lower[1:], torch.tensor([inf], dtype=dtype)])
    ip = _t(is_protein, dtype)
    m = (_t(z_mask, dtype) * (ip[:, None] * ip[None, :]))[..., None]
    return torch.cat([(above(d2, lower) & (d2 < upper)).to(dtype) * m, m], dim=-1)


# ------------------------------------------------------------------ confidence.hip
BIN_CENTRES = 3.375 + 1.75 * torch.arange(13, dtype=F64)                 # linspace(3.375, 24.375, 13), exact in fp32


def nearest_bin(d, argmin=first_argmin):
    d = torch.as_tensor(d)
    return argmin((d[..., None] - BIN_CENTRES.to(d.dtype)).abs(), -1)


def centre_distance(x, centre, dtype=F32):
    xc = _t(x, dtype)[_idx(centre)]
    return sqrt_rn(dist2(xc[:, None], xc[None, :], dtype))


def confidence_pair_init(z, si, sj, WdT, x, centre, dtype=F32, argmin=first_argmin):
    """((z[i, j] + si[i]) + sj[j]) + WdT[bin(|xc_i - xc_j|)], xc = x[centre]"""
    b = nearest_bin(centre_distance(x, centre, dtype), argmin)
    return ((_t(z, dtype) + _t(si, dtype)[:, None]) + _t(sj, dtype)[None, :]) + _t(WdT, dtype)[b]


def pair_symmetrize(z, dtype=F32):
    z = _t(z, dtype)
    return z + z.transpose(0, 1)


def atom_dist_embed(x, w, b=None, dtype=F32):
    """|x_i - x_j| w + b  (b None: + 0)"""
    x = _t(x, dtype)
    d = sqrt_rn(dist2(x[None, :], x[:, None], dtype))
    w = _t(w, dtype).reshape(-1)
    return d[..., None] * w + (torch.zeros_like(w) if b is None else _t(b, dtype).reshape(-1))


def pose_coordinates(x, stride, A, P):
    """[P, A, 3] as the *_poses kernels read them out of a flat array: pose p starts `stride` floats after pose p - 1"""
    flat = torch.as_tensor(x).reshape(-1)
    return torch.stack([flat[p * stride:p * stride + 3 * A].reshape(A, 3) for p in range(P)])


# ------------------------------------------------------------------ sampler.hip: chirality
CHIRALITY_K = 8


def chirality64(x, centres):
    """(vol64 [B, nc], bound [B, nc]) of V = (n1 - c) . ((n2 - c) x (n3 - c)) written out as its six triple products.
    bound = gamma_k S, S the float64 sum of the absolute values of the six products, k = 8 fp32 roundings on the longest chain of
    a product a_x b_y d_z: the three differences (3), b_y d_z (1), the inner difference (1), the product with a_x (1), the two outer
    sums (2).  A fused multiply-add only removes roundings from that chain."""
    x, c = _t(x, F64), _idx(centres).reshape(-1, 4)
    o = x[:, c[:, 0]]
    a, b, d = x[:, c[:, 1]] - o, x[:, c[:, 2]] - o, x[:, c[:, 3]] - o
    terms = []
    for (p, q, r), s in (((0, 1, 2), 1), ((0, 2, 1), -1), ((1, 2, 0), 1), ((1, 0, 2), -1), ((2, 0, 1), 1), ((2, 1, 0), -1)):
        terms.append(s * a[..., p] * b[..., q] * d[..., r])
    terms = torch.stack(terms)
    return terms.sum(0), gamma(CHIRALITY_K) * terms.abs().sum(0)


def chirality_sign(x, centres):
    """(sign [B, nc] int32, decided [B, nc] bool): the sign of the float64 volume where it clears the bound; the sign is 0 and
    decided where every one of the six products is exactly zero (S == 0: the kernel's fp32 expression is then exactly zero too)"""
    vol, bound = chirality64(x, centres)
    return torch.sign(vol).to(torch.int32), (vol.abs() > bound) | (bound == 0)


def chirality_accept(sign, ref_sign, limit=None):
    """[B] int32: 1 where every centre (a wrong variant: every centre below `limit`) has the reference sign"""
    same = sign == _t(ref_sign, torch.int32)[None, :]
    return same[:, :limit].all(dim=1).to(torch.int32)


# ================================================================== cases
# ------------------------------------------------------------------ chain_contacts
THRESHOLD = 2.5
_AXES = torch.tensor([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], dtype=F32)

#: (name, ni, nj, planted [(k, distance)], what): planted minima sit at row-major position k = a * nj + b of the ni x nj matrix; the
#: kernel gives pair k to thread k % 256 in loop trip k // 256
CONTACT_SCENARIOS = (
    ("same thread, trips 0 and 1", 17, 16, ((5, 2.0), (261, 2.0)), 5),
    ("thread 200 trip 0 against thread 4 trip 1", 17, 16, ((200, 2.0), (260, 2.0)), 200),
    ("thread 200 trip 1 against thread 4 trip 2", 40, 30, ((456, 2.0), (516, 2.0)), 456),
    ("thread 4 trip 1 against thread 200 trip 2", 40, 30, ((260, 2.0), (712, 2.0)), 260),
    ("three equal minima", 40, 30, ((100, 2.0), (356, 2.0), (700, 2.0)), 100),
    ("on the threshold", 1, 1, ((0, THRESHOLD),), 0),
    ("one step below the threshold", 1, 1, ((0, float(np.nextafter(np.float32(THRESHOLD), np.float32(0)))),), 0),
    ("empty first chain", 0, 17, (), -1),
    ("empty second chain", 17, 0, (), -1),
    ("closest pair masked", 17, 16, ((37, 1.0), (150, 2.0)), 150),
    ("second chain fully masked", 17, 16, ((37, 1.0),), None),
    ("no contact", 40, 30, (), None),
)


@functools.lru_cache(maxsize=None)
def chain_contacts_case():
    """One launch with every scenario of CONTACT_SCENARIOS as its own pair of chains, plus the first scenario searched a second time
    with its chains exchanged (two searched pairs that set the same token pair).  Atoms sit in clouds of radius < 9 around chain
    centres 60 apart, so every distance that is not planted exceeds 40; a planted pair (a, b) is moved to a site of its own far from
    everything: b to the site, a onto one axis through it at the planted distance (small integers and one-axis offsets: exact in
    fp32).  Three atoms share a token; the tokens of the chains follow each other."""
    g = gen(4100)
    x, a_mask, starts, pairs, expect = [], [], [0], [], []
    site = 0
    for s, (name, ni, nj, planted, want) in enumerate(CONTACT_SCENARIOS):
        ci = len(starts) - 1
        base = starts[-1]
        for c, n in enumerate((ni, nj)):
            centre = torch.tensor([60.0 * (2 * s + c), 0.0, 0.0])
            x.append(centre + (torch.rand(n, 3, generator=g) * 10 - 5).round(decimals=3))
            a_mask.append(torch.ones(n))
            starts.append(starts[-1] + n)
        xi, xj = x[-2], x[-1]
        used_b = {}
        for k, dist in planted:
            a, b = k // nj, k % nj
            if b not in used_b:
                used_b[b] = [torch.tensor([0.0, 1000.0 + 100.0 * site, 0.0]), 0]
                site += 1
                xj[b] = used_b[b][0]
            q, m = used_b[b]
            xi[a] = q + _AXES[m] * dist
            used_b[b][1] += 1
        if name == "closest pair masked":
            a_mask[-2][37 // nj] = 0.0
        if name == "second chain fully masked":
            a_mask[-1][:] = 0.0
        pairs.append((ci, ci + 1))
        expect.append(want)
    pairs.append((1, 0))
    expect.append(5 * 17 + 0)                                          # (b = 5, a = 0) before (b = 5, a = 16) in the exchanged order
    x, a_mask = torch.cat(x), torch.cat(a_mask)
    A = x.shape[0]
    a2t = torch.arange(A) // 3
    return dict(x=x, a_mask=a_mask, chain_start=torch.tensor(starts, dtype=torch.int32), pairs=torch.tensor(pairs, dtype=torch.int32),
                a2t=a2t.long(), threshold=THRESHOLD, T=int(a2t.max()) + 1), tuple(expect)


@functools.lru_cache(maxsize=None)
def chain_contacts_oracle_case():
    """what features_oracle.make_token_bonds can restate: chains of 17, 16, 40 and 30 atoms in atom order, all ligands (every chain
    pair is searched), tokens inside one chain, a few masked atoms, generic coordinates 1.5 apart per chain so that some chain
    pairs touch and some do not; threshold 2.4"""
    g = gen(4200)
    sizes = (17, 16, 40, 30)
    starts = [0]
    for n in sizes:
        starts.append(starts[-1] + n)
    A = starts[-1]
    x = torch.randn(A, 3, generator=g) * 1.2
    for c in range(len(sizes)):
        x[starts[c]:starts[c + 1]] += torch.tensor([3.0 * c, 0.0, 0.0])
    a_mask = (torch.rand(A, generator=g) < 0.85).float()
    a2t = torch.cat([torch.arange(n) // 3 + sum(-(-m // 3) for m in sizes[:c]) for c, n in enumerate(sizes)]).long()
    T = int(a2t.max()) + 1
    asym = torch.zeros(T, dtype=torch.long)
    for c in range(len(sizes)):
        asym[a2t[starts[c]:starts[c + 1]]] = 3 + 2 * c
    pairs = [(i, j) for i in range(len(sizes) - 1) for j in range(i + 1, len(sizes))]
    return dict(x=x, a_mask=a_mask, chain_start=torch.tensor(starts, dtype=torch.int32), pairs=torch.tensor(pairs, dtype=torch.int32),
                a2t=a2t, threshold=2.4, T=T), asym


# ------------------------------------------------------------------ chirality
CHIRALITY_N = (0, 1, 64, 65, 130)


def _rotation(g):
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=F64))
    q = q * torch.sign(torch.diagonal(r))
    return q * torch.sign(torch.linalg.det(q))


@functools.lru_cache(maxsize=None)
def chirality_case(nc, B):
    """centres (c, n1, n2, n3) int32 [nc, 4] over A = 4 nc + 3 atoms (every centre owns its four atoms, shuffled over the
    atom order), reference coordinates x_ref [A, 3] and x [B, A, 3]: pose 0 a rotated and translated copy (accepted), pose 1 the
    mirror image (every centre flipped), pose 2 flat in the z = 0 plane (every sign exactly 0)."""
    g = gen(4300 + 10 * nc + B)
    A = 4 * nc + 3
    perm = torch.randperm(A, generator=g)
    centres = perm[:4 * nc].reshape(nc, 4).int()
    x_ref = torch.randn(A, 3, generator=g) * 1.5
    R, t = _rotation(g), torch.tensor([11.0, -7.0, 3.0], dtype=F64)
    poses = [(x_ref.double() @ R.T + t).float(), x_ref * torch.tensor([1.0, 1.0, -1.0]), x_ref * torch.tensor([1.0, 1.0, 0.0])]
    return dict(centres=centres, x_ref=x_ref, x=torch.stack(poses[:B]), nc=nc, A=A)


@functools.lru_cache(maxsize=None)
def chirality_flip_case():
    """130 centres; poses: the reference, then one pose each whose only flipped centre is 0, 64 and 129 (two neighbours of that
    centre exchange places; no other centre holds those atoms)"""
    c = chirality_case(130, 1)
    poses = [c["x_ref"]]
    for k in (0, 64, 129):
        x = c["x_ref"].clone()
        n1, n2 = int(c["centres"][k, 1]), int(c["centres"][k, 2])
        x[[n1, n2]] = x[[n2, n1]]
        poses.append(x)
    return dict(c, x=torch.stack(poses), flipped=(None, 0, 64, 129))


# ------------------------------------------------------------------ template_feat
TEMPLATE_LOWER = (1.0, 4.0, 9.0, 16.0)


def production_lower(no_bins=39):
    return torch.linspace(3.25, 50.75, no_bins) ** 2


@functools.lru_cache(maxsize=None)
def template_edges_case(T, NB):
    """atoms on the x axis: 0, 1, 2, 3, 4 (d2 on every edge 1, 4, 9, 16), one fp32 step either side of 1, 2 and 3, and 10000 (d2 = 1e8,
    the `inf` of the last bin); pseudo_beta_atom a permutation of them with repeats (T = 1: one atom, d2 = 0); z_mask and is_protein
    hold 0, 0.5 and 1.  lower = the first NB of 1, 4, 9, 16 (NB = 39: the production edges)."""
    g = gen(4400 + 3 * T + NB)
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(1e9)))
    dn = lambda v: float(np.nextafter(np.float32(v), np.float32(0)))
    axis = [0.0, 1.0, 2.0, 3.0, 4.0, up(1), dn(1), up(2), dn(2), up(3), dn(3), 10000.0]
    x = torch.zeros(len(axis) + 2, 3)
    x[:len(axis), 0] = torch.tensor(axis)
    x[len(axis):] = torch.tensor([[0.5, 0.5, 0.5], [2.0, 1.0, 2.0]])                     # off the axis: all three products act
    pb = torch.cat([torch.randperm(x.shape[0], generator=g), torch.randint(0, x.shape[0], (T,), generator=g)])[:T].long()
    vals = torch.tensor([0.0, 0.5, 1.0, 1.0])
    z_mask = vals[torch.randint(0, 4, (T, T), generator=g)]
    is_protein = vals[torch.randint(0, 4, (T,), generator=g)]
    lower = production_lower() if NB == 39 else torch.tensor(TEMPLATE_LOWER[:NB])
    return dict(x=x, pb=pb, z_mask=z_mask, is_protein=is_protein, lower=lower)


@functools.lru_cache(maxsize=None)
def template_random_case(T=17):
    """generic protein-like coordinates against the production edges (features_oracle.dgram_from_positions)"""
    g = gen(4500 + T)
    x = torch.randn(2 * T, 3, generator=g) * 15
    return dict(x=x, pb=torch.randint(0, 2 * T, (T,), generator=g).long(), z_mask=(torch.rand(T, T, generator=g) < 0.8).float(),
                is_protein=(torch.rand(T, generator=g) < 0.8).float(), lower=production_lower())


# ------------------------------------------------------------------ confidence
#: positions on the x axis; against atom 0 they give the distances 0, 3.375 (the first centre), every midpoint 4.25 + 1.75 k between two
#: centres, 24.375 (the last centre) and two distances beyond it
CENTRE_AXIS = (0.0, 3.375, 4.25, 6.0, 7.75, 9.5, 11.25, 13.0, 14.75, 16.5, 18.25, 20.0, 21.75, 23.5, 24.375, 25.25, 100.0)
MIDPOINTS = tuple(4.25 + 1.75 * k for k in range(12))
CONF_SHAPES = ((1, 4), (1, 36), (9, 4), (9, 36), (9, 128))


@functools.lru_cache(maxsize=None)
def confidence_case(T, C, P=1, pad=0):
    """A = 20 atoms: the 17 of CENTRE_AXIS and three off the axis (`centre` is chosen by the test: centre_rows); poses p > 0 are
    pose 0 with the axis scaled by 1 + p (other distances, other bins).  x is flat: poses 3 A + pad floats apart, NaN in the
    padding."""
    g = gen(4600 + 7 * T + C + 100 * P + pad)
    A = len(CENTRE_AXIS) + 3
    x0 = torch.zeros(A, 3)
    x0[:len(CENTRE_AXIS), 0] = torch.tensor(CENTRE_AXIS)
    x0[len(CENTRE_AXIS):] = torch.randn(3, 3, generator=g) * 6
    stride = 3 * A + pad
    flat = torch.full(((P - 1) * stride + 3 * A,), float("nan"))
    for p in range(P):
        flat[p * stride:p * stride + 3 * A] = (x0 * torch.tensor([1.0 + p, 1.0, 1.0])).reshape(-1)
    return dict(z=torch.randn(T, T, C, generator=g), si=torch.randn(T, C, generator=g), sj=torch.randn(T, C, generator=g),
                WdT=torch.randn(13, C, generator=g), x=flat, A=A, stride=stride, P=P)


@functools.lru_cache(maxsize=None)
def centre_rows():
    """two `centre` vectors of 9 tokens that between them pair atom 0 with every atom of CENTRE_AXIS; the second repeats atoms"""
    return (torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 8]), torch.tensor([0, 9, 10, 11, 12, 13, 14, 15, 16]), torch.tensor([0, 2, 2, 16, 0, 13, 14, 15, 2]))


@functools.lru_cache(maxsize=None)
def embed_case(A, C, P=1, pad=0):
    """atoms 0 and 1 coincide when A > 1 (d = 0); coordinates near 300 A; poses differ"""
    g = gen(4700 + 5 * A + C + 100 * P + pad)
    stride = 3 * A + pad
    flat = torch.full(((P - 1) * stride + 3 * A,), float("nan"))
    for p in range(P):
        x = 300 + torch.randn(A, 3, generator=g) * 8
        if A > 1:
            x[1] = x[0]
        flat[p * stride:p * stride + 3 * A] = x.reshape(-1)
    return dict(x=flat, w=torch.randn(C, generator=g), b=torch.randn(C, generator=g), A=A, stride=stride, P=P)


# ------------------------------------------------------------------ msa_feat, target_feat, outer_mask
DELETION_VALUES = (-2.0, 0.0, 0.25, 1.0, 1.5, 3.0, 1e4, 1e30)
TWO_OVER_PI = float((2.0 / (torch.acos(torch.zeros(1)) * 2)).item())      # the fp32 number physdock_amd.features.transform passes


@functools.lru_cache(maxsize=None)
def msa_case(R, T, n_class):
    """S = 6 source rows; `inds` [R] descending with a repeat and starting at the last source row; the deletion matrix cycles through
    DELETION_VALUES from a seeded offset, msa holds every class, n_class itself and n_class + 5 (no class: an all-zero one-hot)"""
    g = gen(4800 + 11 * R + 3 * T + n_class)
    S = 6
    msa = torch.randint(0, n_class + 2, (S, T), generator=g).long()
    msa[msa == n_class + 1] = n_class + 5
    msa.reshape(-1)[:min(S * T, n_class)] = torch.arange(n_class)[:S * T]
    msa[5, 0] = n_class + 5
    msa[5, -1] = n_class
    vals = torch.tensor(DELETION_VALUES)
    deletion = vals[(torch.arange(S * T) + int(torch.randint(0, 8, (1,), generator=g))) % len(vals)].reshape(S, T)
    inds = torch.tensor([5, 3, 3, 1, 0][:R]).long()
    return dict(msa=msa, deletion=deletion, inds=inds, n_class=n_class)


@functools.lru_cache(maxsize=None)
def target_case(T, n_profile, n_class=32):
    """restype cycles through 0, n_class - 1, n_class, -1 and random classes"""
    g = gen(4900 + T + n_profile)
    restype = torch.randint(0, n_class, (T,), generator=g).long()
    edge = torch.tensor([0, n_class - 1, n_class, -1])
    restype[:min(T, 4)] = edge[:min(T, 4)]
    return dict(restype=restype, profile=torch.rand(T, n_profile, generator=g), deletion_mean=torch.randn(T, generator=g), n_class=n_class)


@functools.lru_cache(maxsize=None)
def outer_mask_case(N):
    g = gen(5000 + N)
    return torch.tensor([0.0, 1.0, 0.5, -2.0])[(torch.arange(N) + torch.randint(0, 4, (N,), generator=g)) % 4] if N > 4 \
        else torch.tensor([0.5, 1.0, -2.0, 0.0])[:N]


# ------------------------------------------------------------------ pdb_format
BAD_VALUES = (-1000.0, 10000.0, INF, float("nan"))
#: decimal field limits as the issue of this suite names them; the fp32 number nearest to each decides (see NOTES.md: fp32 has no
#: number between 9999.999 and 10000, so "9999.9995" IS 9999.9990234375 and fits; 10000 is the first positive value that does not)
LIMIT_VALUES = (9999.9994, -999.9994, 9999.9995, -999.9995)


def pdb_template(N):
    """N rows of 81 bytes, a distinct byte in every column of every row (33 + (7 n + col) % 90), the newline last"""
    n, col = torch.meshgrid(torch.arange(N), torch.arange(81), indexing="ij")
    t = (33 + (7 * n + col) % 90).to(torch.uint8)
    if N:
        t[:, 80] = 10
    return t


@functools.lru_cache(maxsize=None)
def pdb_case(B, N):
    """A = N + 4 atoms, `atom` a permuted subset; generic coordinates in (-999, 9999) with halves of the last printed digit (ties of
    the rounding) among them"""
    g = gen(5100 + 10 * B + N)
    A = N + 4
    x = (torch.rand(B, A, 3, generator=g) * 200 - 100)
    x[:, 0, :] = torch.tensor([0.0005, -0.0005, 2.0625])                  # exact and inexact halves; -0.000
    x[:, 1, :] = torch.tensor([9999.0, -999.0, 0.0])
    return dict(x=x, tmpl=pdb_template(N), atom=torch.randperm(A, generator=g)[:N].int(), A=A)


@functools.lru_cache(maxsize=None)
def pdb_bad_case():
    """B = 3, N = 7: record (b, n) = (k % 3, k) has exactly one bad field f = k % 3 for the k-th of BAD_VALUES; the four decimal limits
    sit in records 4 and 5 of pose 0"""
    c = pdb_case(3, 7)
    x = c["x"].clone()
    atom = c["atom"].long()
    for k, v in enumerate(BAD_VALUES):
        x[k % 3, atom[k], k % 3] = v
    x[0, atom[4], :2] = torch.tensor(LIMIT_VALUES[:2])
    x[0, atom[5], :2] = torch.tensor(LIMIT_VALUES[2:])
    return dict(c, x=x)
