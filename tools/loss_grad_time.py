"""Time of PhysDockLoss.grads() (the five terms and both gradients) against the forward "terms only" row of tools/loss_time.py,
at the cfg1 (T = 256 / A = 2048) and cfg2 (T = 512 / A = 4096) shapes, B = 48, in one process on one device; plus the
smooth-lDDT gradient launch alone and its issue-slot model.

    python tools/loss_grad_time.py [--reps 20] [--out profiles/loss_grad_time.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.loss_time import timed  # noqa: E402

#: issue cycles per pair term and lane of smooth_lddt_grad_kernel (estimated from the source, see NOTES.md):
#: 6 transcendental wave instructions (v_rsq, v_exp, 4 v_rcp) x 8 + 23 other VALU x 4, over 64 lanes
CYCLES_PER_TERM = (6 * 8 + 23 * 4) / 64


def active_strips(xg, ex, clamp, full):
    """64-row x 16-column strips with at least one pair inside the clamp (the strips the kernels compute)"""
    x = xg.double().cpu().numpy()
    e = ex.double().cpu().numpy()
    A = x.shape[0]
    nt = (A + 63) // 64
    pad = nt * 64
    xp = np.zeros((pad, 3)); xp[:A] = x
    ep = np.zeros(pad); ep[:A] = e
    n = 0
    for ti in range(nt):
        d = np.sqrt(((xp[ti * 64:(ti + 1) * 64, None] - xp[None]) ** 2).sum(-1))
        m = (d < clamp) * ep[ti * 64:(ti + 1) * 64, None] * ep[None]
        s = m.reshape(64, pad // 16, 16).any(axis=(0, 2))
        if not full:
            s[: ti * 4] = False
        n += int(s.sum())
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from physdock_amd import PhysDockConfig, PhysDockLoss, loss
    from physdock_amd.synthetic import loss_features, loss_outputs, make_batch
    cfg = PhysDockConfig()
    clamp = cfg.loss.smooth_lddt_loss.max_clamp_distance
    lines = []
    for tag, (n_prot, n_lig) in (("cfg1", (224, 32)), ("cfg2", (448, 64))):
        f = loss_features(make_batch(n_prot, 9, n_lig, 8, seed=0), seed=6)
        o = {k: v.cuda() for k, v in loss_outputs(f, 48, seed=7).items()}
        f = {k: v.cuda() for k, v in f.items()}
        B, A, T = o["x_denoised"].shape[0], o["x_denoised"].shape[1], f["is_ligand"].shape[0]
        L = PhysDockLoss(cfg)
        fwd = timed(lambda: L.terms(o, f), args.reps)
        bwd = timed(lambda: L.grads(o, f), args.reps)
        xd = o["x_denoised"].contiguous()
        xg, ex = f["x_gt"].float().contiguous(), f["x_exists"].float().contiguous()
        one = torch.ones(1, device="cuda")
        ws = loss._gws(B, A, T, xd.device)
        g = torch.empty_like(xd)
        sl = timed(lambda: loss._smooth_lddt_grad(xd, xg, ex, clamp, one, g, ws, 0), args.reps)
        lines.append(f"{tag}: B = {B}, A = {A}, T = {T}   (us per call: median / min / max of {args.reps} x 5 calls)")
        lines.append(f"  {'forward: terms only (no host read)':44s} {fwd[0]:9.1f} {fwd[1]:9.1f} {fwd[2]:9.1f}")
        lines.append(f"  {'grads(): 5 terms + g_x + g_p':44s} {bwd[0]:9.1f} {bwd[1]:9.1f} {bwd[2]:9.1f}")
        lines.append(f"  {'  of it: pd_loss_smooth_lddt_grad alone':44s} {sl[0]:9.1f} {sl[1]:9.1f} {sl[2]:9.1f}")
        lines.append(f"  grads() / forward = {bwd[0] / fwd[0]:.2f} (bar 3)")
        strips = active_strips(xg, ex, clamp, full=True)
        terms = strips * 64 * 16 * B
        model_us = terms * CYCLES_PER_TERM / 1024 / 2.4e3
        lines.append(f"  smooth lDDT gradient: {strips} active 64 x 16 strips of {((A + 63) // 64) * ((A + 63) // 64) * 4} (full rows), "
                     f"{terms:.3e} pair terms; issue model {model_us:.1f} us at 1024 SIMDs x 2.4 GHz (assumed) -> "
                     f"the launch reaches {100 * model_us / sl[0]:.0f} % of it")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
