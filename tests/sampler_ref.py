"""Plain high-precision references of the per-step sampler kernels (physdock_amd/csrc/sampler.hip) and of the Philox draws.

torch float64 / numpy on the CPU, no device code.  Every function transcribes the formula documented above its kernel (or in
oracle/physdock_oracle.py) as whole-tensor algebra; none of them follows a kernel's loop structure.  Shapes as the C ABI has them:
x [B, A, 3], mask / w [A], rot_u [4, B], trans [B, 3], Wx [C, 3], Wr [3, C], lig [B, L, 3], ref_dist [Cn, L, L], poses [Cn, L, 3].
"""
import math

import numpy as np
import torch

F64 = torch.float64


def _d(t):
    return None if t is None else torch.as_tensor(t).to(F64)


def _per_sample(v, B):
    """a scalar, or one value per sample [B], as a [B, 1, 1] float64 tensor"""
    v = torch.as_tensor(v, dtype=F64)
    return v.reshape(-1, 1, 1).expand(B, 1, 1) if v.dim() else v.reshape(1, 1, 1).expand(B, 1, 1)


# ------------------------------------------------------------------ augmentation
def _sphere_point64(u_phi, u_theta):
    phi = u_phi * 2 * math.pi
    theta = torch.acos(u_theta * 2 - 1)
    return torch.stack([torch.cos(phi) * torch.sin(theta), torch.sin(phi) * torch.sin(theta), torch.cos(theta)], dim=-1)


def rotation64(u):
    """rows e0, e1, e2 of the rotation the four uniforms u [4, B] define (Gram-Schmidt of two sphere points)"""
    u = _d(u)
    e0 = _sphere_point64(u[0], u[1])
    e1 = _sphere_point64(u[2], u[3])
    e1 = e1 - e0 * (e1 * e0).sum(-1, keepdim=True)
    e1 = e1 / torch.linalg.norm(e1, dim=-1, keepdim=True)
    return torch.stack([e0, e1, torch.linalg.cross(e0, e1, dim=-1)], dim=-2)


def augment64(x, x_scale, mask, u, trans, noise, lam, sdev):
    """R (x_scale x - mu) + t + (lam * noise) * sdev, mu the mask-weighted centroid"""
    x, mask, trans = _d(x) * float(x_scale), _d(mask), _d(trans)
    mu = (x * mask[None, :, None]).sum(-2, keepdim=True) / mask.sum()
    out = torch.einsum("bij,bkj->bki", rotation64(u), x - mu) + trans[:, None, :]
    if sdev != 0:
        out = out + (float(lam) * _d(noise)) * float(sdev)
    return out


# ------------------------------------------------------------------ precond / denoise
def precond64(x_hat, c_in, Wx, bx, a):
    """ba[b, l, :] = Wx . (x_hat[b, l] * c_in[b]) + bx + a[l, :];  c_in a scalar or [B]"""
    x_hat = _d(x_hat)
    xs = x_hat * _per_sample(c_in, x_hat.shape[0])
    return xs @ _d(Wx).T + _d(bx) + _d(a)[None]


def denoise64(ba, x_hat, nw, nb, Wr, eps, c_skip, c_out):
    """c_skip x_hat + c_out Wr . LayerNorm(ba) (biased variance, affine nw / nb);  c_skip / c_out scalars or [B]"""
    ba, x_hat = _d(ba), _d(x_hat)
    mean = ba.mean(-1, keepdim=True)
    var = ((ba - mean) ** 2).mean(-1, keepdim=True)
    y = (ba - mean) / torch.sqrt(var + float(eps)) * _d(nw) + _d(nb)
    B = x_hat.shape[0]
    return _per_sample(c_skip, B) * x_hat + _per_sample(c_out, B) * (y @ _d(Wr).T)


# ------------------------------------------------------------------ weighted Kabsch
def _kabsch_parts(x_pred, pred_mask, x_gt, w):
    P, G, w = _d(x_pred), _d(x_gt), _d(w)
    if pred_mask is not None:
        P = P * _d(pred_mask)[None, :, None]
    if G.dim() == 2:
        G = G[None].expand(P.shape[0], -1, -1)
    wsum = w.sum()
    mu_p = (P * w[None, :, None]).sum(-2) / wsum
    mu_g = (G * w[None, :, None]).sum(-2) / wsum
    Pc, Gc = P - mu_p[:, None], G - mu_g[:, None]
    H = torch.einsum("bij,bik->bjk", Gc * w[None, :, None], Pc)
    U, S, Vh = torch.linalg.svd(H)
    sign = torch.sign(torch.linalg.det(U @ Vh))
    Fm = torch.diag_embed(torch.stack([torch.ones_like(sign), torch.ones_like(sign), sign], dim=-1))
    R = (U @ Fm @ Vh).transpose(-1, -2)
    return torch.einsum("bij,bkj->bki", R, Gc) + mu_p[:, None], S, sign


def kabsch64(x_pred, pred_mask, x_gt, w):
    """x_gt moved onto x_pred * pred_mask by the optimal proper rotation under the weights w -> (aligned [B, A, 3], the
    singular values [B, 3] of H = sum_a w_a (g_a - mu_g)(p_a - mu_p)^T)"""
    out, S, _ = _kabsch_parts(x_pred, pred_mask, x_gt, w)
    return out, S


def kabsch_margin64(x_pred, pred_mask, x_gt, w):
    """(sigma_2 + s sigma_3) / sigma_1 per sample, s = sign det(U Vh): positive exactly when the proper rotation is unique"""
    _, S, sign = _kabsch_parts(x_pred, pred_mask, x_gt, w)
    return (S[:, 1] + sign * S[:, 2]) / S[:, 0]


# ------------------------------------------------------------------ template metric, conformer distances, pose RMSD
def pose_dist64(poses):
    p = _d(poses)
    return torch.linalg.norm(p[:, :, None] - p[:, None], dim=-1)


def template_eps64(lig, ref_dist):
    """eps[b, c] = mean_ij 1/4 sum_k sigmoid(|D_b,ij - Dref_c,ij| - {.5, 1, 2, 4})"""
    lig = _d(lig)
    dist = torch.linalg.norm(lig[:, :, None] - lig[:, None], dim=-1)
    delta = (dist[:, None] - _d(ref_dist)[None]).abs()
    e = 0.25 * sum(torch.sigmoid(delta - k) for k in (0.5, 1.0, 2.0, 4.0))
    return e.mean(dim=(-1, -2))


def pairwise_rmsd64(x, idx, ref):
    """D[i, j] = sqrt(mean_a |x_i[a] - x_j[a]|^2) over the atoms idx (None: all), and the same against ref (or None)"""
    x = _d(x)
    sel = slice(None) if idx is None else torch.as_tensor(idx).long()
    xs = x[:, sel]
    D = torch.sqrt(((xs[:, None] - xs[None]) ** 2).sum(-1).mean(-1))
    r = None if ref is None else torch.sqrt(((xs - _d(ref)[sel][None]) ** 2).sum(-1).mean(-1))
    return D, r


# ------------------------------------------------------------------ Euler update, timestep embedding
def euler64(x_hat, x_den, x_proj, w, t_hat, eta, dt):
    """x_hat + eta dt d,  d = (x_hat - x_den) / t_hat, mixed per atom with (x_hat - x_proj) / t_hat by w when x_proj is given"""
    x_hat = _d(x_hat)
    d = (x_hat - _d(x_den)) / float(t_hat)
    if x_proj is not None:
        wa = _d(w)[None, :, None]
        d = d * (1 - wa) + (x_hat - _d(x_proj)) / float(t_hat) * wa
    return x_hat + float(eta) * float(dt) * d


def timestep_embed64(tau):
    """[cos(tau f_k) | sin(tau f_k)], f_k = exp(-ln(1e4) k / 128), k < 128"""
    f = torch.exp(-math.log(10000.0) * torch.arange(128, dtype=F64) / 128)
    arg = _d(tau)[:, None] * f[None]
    return torch.cat([torch.cos(arg), torch.sin(arg)], dim=-1)


# ------------------------------------------------------------------ Philox4x32-10 (Salmon et al., SC'11) and the draws
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four, key: two words (scalars or broadcastable integer arrays) -> uint64 array [..., 4] of 32-bit words"""
    c = [np.asarray(v, dtype=np.uint64) & _LO for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(v, dtype=np.uint64) & _LO for v in key)
    for r in range(10):
        ka = (k0 + np.uint64((_W0 * r) & 0xFFFFFFFF)) & _LO
        kb = (k1 + np.uint64((_W1 * r) & 0xFFFFFFFF)) & _LO
        p0, p1 = _M0 * c[0], _M1 * c[2]               # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _S32) ^ c[1] ^ ka, p1 & _LO, (p0 >> _S32) ^ c[3] ^ kb, p0 & _LO]
    return np.stack(c, axis=-1)


def u01(bits):
    """(float32(bits >> 8) + 0.5f) * 2^-24 in float32: the sum rounds from 2^23 on, so 1.0 is reachable and 0.0 is not"""
    hi = (np.asarray(bits, dtype=np.uint64) >> np.uint64(8)).astype(np.float32)
    return (hi + np.float32(0.5)) * np.float32(2.0 ** -24)


def _box_muller(u, dt):
    u = u.astype(dt)
    two_pi = dt(6.283185307179586)
    r0, r1 = np.sqrt(dt(-2) * np.log(u[..., 0])), np.sqrt(dt(-2) * np.log(u[..., 2]))
    a0, a1 = two_pi * u[..., 1], two_pi * u[..., 3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)


def normals4(counter, key, dtype=np.float64):
    """Box-Muller of the four uniforms of one Philox block: r0 cos, r0 sin, r1 cos, r1 sin (r0 from word 0 with the angle of
    word 1, r1 from word 2 with the angle of word 3).  dtype=np.float32 evaluates the same formula in float32."""
    return _box_muller(u01(philox4x32_10(counter, key)), dtype)


def seed_key(seed):
    seed = int(seed)
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def init_noise_draws(seed, sample0, sigma0, B, A, dtype=np.float64):
    """[B, A, 3]: sigma0 * the first three normals of counter (atom, sample0 + b, 0xFFFFFFFF, 0)"""
    b, a = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(A, dtype=np.uint64), indexing="ij")
    n = normals4((a, b + np.uint64(sample0), 0xFFFFFFFF, 0), seed_key(seed), dtype)
    return n[..., :3] * dtype(sigma0)


def augment_rot_uniforms(seed, step, sample0, B):
    """[4, B] float32: u01 of the four words of counter (0, sample0 + b, step, 1)"""
    b = np.arange(B, dtype=np.uint64) + np.uint64(sample0)
    return u01(philox4x32_10((0, b, step, 1), seed_key(seed))).T.copy()


def augment_trans_draws(seed, step, sample0, B, dtype=np.float64):
    """[B, 3]: the first three normals of counter (1, sample0 + b, step, 1)"""
    b = np.arange(B, dtype=np.uint64) + np.uint64(sample0)
    return normals4((1, b, step, 1), seed_key(seed), dtype)[..., :3]


def augment_noise_draws(seed, step, sample0, B, A, dtype=np.float64):
    """[B, A, 3]: the first three normals of counter (atom, sample0 + b, step, 2)"""
    b, a = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(A, dtype=np.uint64), indexing="ij")
    return normals4((a, b + np.uint64(sample0), step, 2), seed_key(seed), dtype)[..., :3]


def moments(v):
    """(mean, variance, kurtosis) of a flat sample"""
    v = np.asarray(v, dtype=np.float64).ravel()
    m = v.mean()
    c = v - m
    var = (c ** 2).mean()
    return m, var, (c ** 4).mean() / var ** 2


def ulp32(x):
    """spacing of float32 at |x| (a python float)"""
    return float(np.spacing(np.float32(abs(float(x)))))
