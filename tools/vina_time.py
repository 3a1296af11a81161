"""Time VinaScore.score (csrc/vina.hip) with device events at P = 64 poses, L = 50 ligand atoms, A = 2048 pose atoms, next to the
same five terms, the score and the forces written as torch operations on the same GPU (cdist for the distances, the analytic
derivative for the forces).  Each timed window is `--calls` back-to-back calls between two events, after a warm-up; the line reports
the median and the spread of `--windows` windows per call.  The receptor is a jittered 3.8 A lattice with the ligand's atoms on
sites near its centre.

    python tools/vina_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physdock_amd import scoring  # noqa: E402
from physdock_amd.scoring import VinaScore  # noqa: E402


def per_call_us(fn, calls, windows, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / calls)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def torch_form(x, t, n_rot):
    """score [P], terms [P,5] and forces [P,L,3] of pd_vina_score as torch operations"""
    lig = x[:, t["lig_idx"]]                                             # [P,L,3]
    r = torch.cdist(lig, x)                                              # [P,L,A]
    ty, tl = t["types"], t["types"][t["lig_idx"]]
    d = r - (t["radius"][t["lig_idx"]][:, None] + t["radius"][None, :])
    count = (t["lig_active"][:, None] & t["rec_mask"][None, :]) & (r < scoring.CUTOFF)
    hyd = ((tl[:, None] & ty[None, :] & scoring.HYDROPHOBIC) > 0) & count
    don, acc = (ty & scoring.DONOR) > 0, (ty & scoring.ACCEPTOR) > 0
    hb = ((don[t["lig_idx"]][:, None] & acc[None, :]) | (acc[t["lig_idx"]][:, None] & don[None, :])) & count
    q1, q2 = d * 2.0, (d - 3.0) * 0.5
    g1, g2 = torch.exp(-q1 * q1), torch.exp(-q2 * q2)
    zero = torch.zeros((), device=x.device)
    hs, hbs = hyd & (d > 0.5) & (d < 1.5), hb & (d > -0.7) & (d < 0)
    per_pair = torch.stack([torch.where(count, g1, zero), torch.where(count, g2, zero), torch.where(count & (d < 0), d * d, zero),
                            torch.where(hyd & (d <= 0.5), 1.0, torch.where(hs, 1.5 - d, zero)),
                            torch.where(hb & (d <= -0.7), 1.0, torch.where(hbs, -d / 0.7, zero))], -1)
    w = t["weights"]
    terms = per_pair.sum((1, 2))
    inter = terms @ w
    de = w[0] * (-4.0 * q1 * g1) + w[1] * (-q2 * g2) + w[2] * torch.where(d < 0, 2.0 * d, zero) - w[3] * hs - w[4] / 0.7 * hbs
    de = torch.where(count & (r > 0), de / r.clamp_min(1e-30), zero)
    forces = -(de[..., None] * (lig[:, :, None, :] - x[:, None, :, :])).sum(2)
    return inter / (1.0 + scoring.ROT_WEIGHT * n_rot), terms, forces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    n, Lg, A = 64, 50, 2048
    rng = np.random.default_rng(50)
    side = 13
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    order = np.argsort(((grid - (side - 1) / 2.0) ** 2).sum(-1), kind="stable")[:A]
    sites = (grid[order] - (side - 1) / 2.0) * 3.8
    lig_idx = np.sort(rng.permutation(A)[:Lg])
    rec = np.setdiff1d(np.arange(A), lig_idx)
    x = np.empty((n, A, 3))
    x[:, lig_idx] = sites[:Lg] + rng.uniform(-0.9, 0.9, (n, Lg, 3))
    x[:, rec] = sites[Lg:] + rng.uniform(-0.6, 0.6, (n, A - Lg, 3))
    elements = rng.choice([6, 6, 6, 7, 8, 16], A)
    types = scoring.element_types(elements, acceptors=True)
    types[elements == 7] |= scoring.DONOR
    v = VinaScore.from_types(types, lig_idx, np.ones(A), 6, device="cuda")
    x = torch.from_numpy(x.astype(np.float32)).cuda()
    radius = np.asarray([scoring.RADII.get(int(z), scoring.DEFAULT_RADIUS) for z in elements], dtype=np.float32)
    t = dict(lig_idx=torch.from_numpy(lig_idx).cuda(), types=torch.from_numpy(types.astype(np.int64)).cuda(),
             radius=torch.from_numpy(radius).cuda(), rec_mask=torch.from_numpy(v.rec_mask).cuda().bool(),
             lig_active=torch.from_numpy(v.lig_active).cuda().bool(), weights=torch.tensor(scoring.WEIGHTS, device="cuda"))
    out = v.score(x, forces=True)
    score, terms, forces = torch_form(x, t, v.n_rot)
    err = max(float((out["score"] - score).abs().max()), float((out["forces"] - forces).abs().max()))
    rel = float(((out["terms"] - terms).abs() / terms.abs().clamp_min(1.0)).max())
    hip = per_call_us(lambda: v.score(x, forces=True), args.calls, args.windows)
    tor = per_call_us(lambda: torch_form(x, t, v.n_rot), max(args.calls // 10, 1), args.windows)
    line = (f"P={n} L={Lg} A={A}: VinaScore.score with forces {hip[0]:.1f} us per call (min {hip[1]:.1f}, max {hip[2]:.1f} over "
            f"{args.windows} windows of {args.calls} calls; two kernels plus six output allocations); torch cdist expression {tor[0]:.1f} us "
            f"(min {tor[1]:.1f}, max {tor[2]:.1f}; {tor[0] / hip[0]:.1f} x); max |difference| of score and forces {err:.1e}, of the terms "
            f"{rel:.1e} relative")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
