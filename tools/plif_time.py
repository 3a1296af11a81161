"""Time InteractionFingerprint.fingerprint and .pairwise (csrc/plif.hip) with device events at P = 64 poses, L = 50 ligand atoms,
A = 2048 pose atoms (residues of eight atoms), next to the same bits, distances, counts and Tanimoto matrix written as torch
operations on the same GPU (cdist for the distances, scatter-reductions over the residues).  The torch expression is the yardstick
printed beside the kernels, not a target they must beat by a fixed factor.  Each timed window is `--calls` back-to-back calls between
two events, after a warm-up; the line reports the median and the spread of `--windows` windows per call.  The receptor is a jittered
3.8 A lattice with the ligand's atoms on sites near its centre.

    python tools/plif_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physdock_amd import interactions, scoring  # noqa: E402
from physdock_amd.interactions import InteractionFingerprint  # noqa: E402


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


def torch_form(x, t, R):
    """bits [P,R], ligand_bits [P,L], min_dist [P,R] and counts [P,6] of pd_plif_fingerprint as torch operations"""
    r = torch.cdist(x[:, t["lig_idx"]], x)                                # [P,L,A]
    pair = t["lig_active"][:, None] & t["rec_mask"][None, :]
    byte = torch.zeros(r.shape, dtype=torch.int64, device=x.device)
    for k in range(6):
        byte |= ((r < t["thr"][k]) & (t["allow"][k] & pair)[None]).long() << k
    ligand_bits = torch.stack([((byte >> k) & 1).amax(2) << k for k in range(6)]).sum(0)
    per_atom = torch.stack([((byte >> k) & 1).amax(1) << k for k in range(6)]).sum(0)                      # [P,A]: OR over the ligand
    kinds = torch.stack([(per_atom >> k) & 1 for k in range(6)], -1)                                       # [P,A,6]
    idx = t["residue_of"][None, :, None].expand(x.shape[0], -1, 6)
    res_kinds = torch.zeros(x.shape[0], R, 6, dtype=torch.int64, device=x.device).scatter_reduce(1, idx, kinds, "amax")
    bits = (res_kinds << torch.arange(6, device=x.device)).sum(-1)
    near = torch.where(pair[None], r, torch.inf).amin(1)                                                   # [P,A]
    min_dist = torch.full((x.shape[0], R), torch.inf, device=x.device).scatter_reduce(1, t["residue_of"][None].expand(x.shape[0], -1), near, "amin")
    return bits, ligand_bits, min_dist, res_kinds.sum(1)


def torch_pairwise(bits):
    k = torch.stack([(bits.int() >> b) & 1 for b in range(6)], -1).flatten(1).float()                      # [P, 6 R]
    shared = k @ k.T
    n = k.sum(1)
    union = n[:, None] + n[None, :] - shared
    return torch.where(union == 0, 1.0, shared / union.clamp_min(1.0))


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
    charges = np.where(elements == 7, rng.integers(0, 2, A) * interactions.CATION, np.where(elements == 8, rng.integers(0, 2, A) * interactions.ANION, 0))
    residue_of = np.arange(A) // 8
    R = int(residue_of.max()) + 1
    f = InteractionFingerprint.from_types(types, charges, lig_idx, np.ones(A), residue_of, device="cuda")
    x = torch.from_numpy(x.astype(np.float32)).cuda()
    ty, q = torch.from_numpy(types.astype(np.int64)).cuda(), torch.from_numpy(charges.astype(np.int64)).cuda()
    li = torch.from_numpy(lig_idx).cuda()
    lt, lq = ty[li][:, None], q[li][:, None]
    H, D, Ac = scoring.HYDROPHOBIC, scoring.DONOR, scoring.ACCEPTOR
    allow = torch.stack([torch.ones(Lg, A, dtype=torch.bool, device="cuda"), ((lt & H) > 0) & ((ty & H) > 0)[None], ((lt & D) > 0) & ((ty & Ac) > 0)[None],
                         ((lt & Ac) > 0) & ((ty & D) > 0)[None], ((lq & 1) > 0) & ((q & 2) > 0)[None], ((lq & 2) > 0) & ((q & 1) > 0)[None]])
    tv = f.threshold_values
    t = dict(lig_idx=li, rec_mask=torch.from_numpy(f.rec_mask).cuda().bool(), lig_active=torch.from_numpy(f.lig_active).cuda().bool(),
             residue_of=torch.from_numpy(residue_of).cuda(), allow=allow, thr=[tv[0], tv[1], tv[2], tv[2], tv[3], tv[3]])
    out = f.fingerprint(x)
    bits, ligand_bits, min_dist, counts = torch_form(x, t, R)
    differ = int((out["bits"].int() != bits).sum()) + int((out["ligand_bits"].int() != ligand_bits).sum())
    err = float((out["min_dist"] - min_dist).abs().max())
    tan = f.pairwise(out["bits"])
    tan_err = float((tan - torch_pairwise(out["bits"])).abs().max())
    hip = per_call_us(lambda: f.fingerprint(x), args.calls, args.windows)
    tor = per_call_us(lambda: torch_form(x, t, R), max(args.calls // 10, 1), args.windows)
    hip_p = per_call_us(lambda: f.pairwise(out["bits"]), args.calls, args.windows)
    tor_p = per_call_us(lambda: torch_pairwise(out["bits"]), max(args.calls // 10, 1), args.windows)
    line = (f"P={n} L={Lg} A={A} R={R}: InteractionFingerprint.fingerprint {hip[0]:.1f} us per call (min {hip[1]:.1f}, max {hip[2]:.1f} over "
            f"{args.windows} windows of {args.calls} calls; three kernels plus six allocations); torch cdist expression {tor[0]:.1f} us "
            f"(min {tor[1]:.1f}, max {tor[2]:.1f}; {tor[0] / hip[0]:.1f} x); bytes that differ {differ} (a pair within rounding of a "
            f"threshold may), max |difference| of min_dist {err:.1e}; counts equal {bool((out['counts'] == counts).all())}.  "
            f"pairwise {hip_p[0]:.1f} us (min {hip_p[1]:.1f}, max {hip_p[2]:.1f}); torch expression {tor_p[0]:.1f} us (min {tor_p[1]:.1f}, "
            f"max {tor_p[2]:.1f}; {tor_p[0] / hip_p[0]:.1f} x); max |difference| {tan_err:.1e}")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
