"""Time PoseValidity.check (csrc/validity.hip) with device events at P = 64 poses, L = 50 ligand atoms, A = 2048 pose atoms, next to
the same eight quantities written as a torch expression on the same GPU (cdist for the distances, a batched float64 eigh for the
planes).  Each timed window is `--calls` back-to-back calls between two events, after a warm-up; the line reports the median and
the spread of `--windows` windows per call.  The ligand is a chain with two aromatic-like rings (planar groups of 6) placed in a
box inside a random receptor.

    python tools/validity_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physdock_amd.validity import PoseValidity  # noqa: E402


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


def torch_form(x, t):
    """the eight columns of pd_pose_validity as torch operations: x [P,A,3] -> val [P,8]"""
    lig = x[:, t["lig_idx"]]                                             # [P,L,3]
    r = t["radius"]
    rl = r[t["lig_idx"]]
    dl = torch.cdist(lig, lig)                                           # [P,L,L]
    q12 = dl[:, t["pair12"][:, 0], t["pair12"][:, 1]] / t["d12_ref"]
    q13 = dl[:, t["pair13"][:, 0], t["pair13"][:, 1]] / t["d13_ref"]
    inf = torch.tensor(float("inf"), device=x.device)
    act = t["lig_active"]
    far = t["far"] & act[:, None] & act[None, :]
    clash = torch.where(far, dl / (rl[:, None] + rl[None, :]), inf).amin((1, 2))
    dr = torch.cdist(lig, x)                                             # [P,L,A]
    ok = act[:, None] & t["rec_mask"][None, :]
    rec = torch.where(ok, dr / (rl[:, None] + r[None, :]), inf).amin((1, 2))
    dist = torch.where(ok, dr, inf).amin((1, 2))
    g = lig[:, t["planar"]].double()                                     # [P,G,6,3]
    c = g - g.mean(2, keepdim=True)
    w, v = torch.linalg.eigh(c.transpose(2, 3) @ c / g.shape[2])
    plane = (c @ v[..., :1]).abs().amax((1, 2, 3)).float()
    return torch.stack([q12.amin(1), q12.amax(1), q13.amin(1), q13.amax(1), clash, rec, dist, plane], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    n, Lg, A = 64, 50, 2048
    rng = np.random.default_rng(50)
    bonds = [(i, i + 1) for i in range(Lg - 1)] + [(0, 5), (20, 25)]
    groups = [tuple(range(0, 6)), tuple(range(20, 26))]
    ref = np.cumsum(rng.standard_normal((Lg, 3)) * 0.9, 0)
    elements = rng.choice([1, 6, 6, 6, 7, 8], A)
    lig_idx = np.sort(rng.permutation(A)[:Lg])
    v = PoseValidity.from_bonds(Lg, bonds, ref, elements, lig_idx, planar_groups=groups, device="cuda")
    x = rng.uniform(-25, 25, (n, A, 3))
    x[:, lig_idx] = ref[None] - ref.mean(0) + rng.standard_normal((n, Lg, 3)) * 0.2
    x = torch.from_numpy(x.astype(np.float32)).cuda()
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(v, k))).cuda() for k in ("radius", "d12_ref", "d13_ref")}
    t.update({k: torch.from_numpy(np.ascontiguousarray(getattr(v, k))).cuda().bool() for k in ("rec_mask", "lig_active", "far")})
    t.update({k: torch.from_numpy(np.ascontiguousarray(getattr(v, k))).cuda().long() for k in ("pair12", "pair13")})
    t["lig_idx"] = torch.from_numpy(v.ligand_idx).cuda().long()
    t["planar"] = torch.from_numpy(v.planar[:, :6]).cuda().long()
    out = v.check(x)
    val = torch.cat([out["bond_ratio"], out["angle_ratio"], out["internal_clash"][:, None], out["receptor_clash"][:, None],
                     out["receptor_distance"][:, None], out["planarity"][:, None]], 1)
    err = float((val - torch_form(x, t)).abs().max())
    hip = per_call_us(lambda: v.check(x), args.calls, args.windows)
    tor = per_call_us(lambda: torch_form(x, t), max(args.calls // 10, 1), args.windows)
    line = (f"P={n} L={Lg} A={A} n12={len(v.pair12)} n13={len(v.pair13)} G={len(v.planar)}: PoseValidity.check {hip[0]:.1f} us per call "
            f"(min {hip[1]:.1f}, max {hip[2]:.1f} over {args.windows} windows of {args.calls} calls; two kernels plus four output "
            f"allocations); torch cdist expression {tor[0]:.1f} us (min {tor[1]:.1f}, max {tor[2]:.1f}; {tor[0] / hip[0]:.1f} x); "
            f"max |difference| {err:.1e}")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
