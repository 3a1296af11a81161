"""Time the fused Monte-Carlo search (pd_vina_search, csrc/vina_refine.hip) next to the same work composed on the host from
`pd_vina_refine`: 64 poses x 8 chains x 20 steps on the largest case of tests/vina_refine_ref.py (P3_A300_L12_T3: 300 pose atoms, a
12-atom ligand with 3 torsions; its three poses repeated to 64, every pose under its own id so that every chain draws its own steps).

    fused        one pd_vina_search launch over 64 x 8 blocks and one pd_vina_search_select launch
    composed     21 pd_vina_refine launches on 512 poses (the 64 repeated 8 times): the start and the 20 steps of every chain, each a
                 grid-wide wait.  The proposal step between the launches (draw, move, Metropolis, copies) is LEFT OUT, and every launch
                 minimises the unperturbed poses, so this is a lower bound that favours the composition.

Both go straight to the C ABI with buffers allocated beforehand; `VinaRefine.search` (with its scoring and allocations) is timed too.
Each figure is the median of `--runs` runs between two device events after one warm-up run.

    python tools/search_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vina_refine_ref as ref  # noqa: E402
from physdock_amd import ops  # noqa: E402
from physdock_amd.refine import VinaRefine  # noqa: E402
from physdock_amd.scoring import VinaScore  # noqa: E402


def median_ms(fn, runs):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    n_pose, K, steps, max_iters, grad_tol, max_step = 64, 8, 20, 20, 1e-4, 1.0
    c = ref.make_case("P3_A300_L12_T3")
    v = VinaScore.from_types(c["types"], c["lig_idx"], c["rec_mask"], c["n_rot"], ligand_active=c["lig_active"], device="cuda")
    r = VinaRefine.from_vina(v, c["bonds"], device="cuda")
    x = torch.from_numpy(np.resize(c["x"], (n_pose,) + c["x"].shape[1:])).cuda()
    x8 = x.repeat(K, 1, 1).contiguous()
    L_ = ops._lib.init()
    A, Lg, T = x.shape[1], r.n_atoms, r.n_torsions
    f64 = lambda *s: torch.empty(*s, device="cuda", dtype=torch.float64)
    i32 = lambda *s: torch.empty(*s, device="cuda", dtype=torch.int32)
    P = ops.ptr
    rot_amp = r.default_rotate_amp(x)
    # fused
    _, head = r._poses(x, "search")
    numel = L_.pd_vina_search_workspace_numel(n_pose, K, Lg, T)
    ws = f64(numel)
    o = [torch.empty(n_pose, K, Lg, 3, device="cuda"), f64(n_pose, K), f64(n_pose, K), i32(n_pose, K), i32(n_pose, K), i32(n_pose, K)]
    sel = [i32(n_pose), f64(n_pose), torch.empty_like(x)]

    def fused():
        ops.check(L_.pd_vina_search(*head, max_iters, grad_tol, max_step, 0, 0, 0, steps, steps, 1.2, 2.0, rot_amp, P(ws), numel, *[P(t) for t in o],
                                    None, None, None, None, None, n_pose, K, A, Lg, T, ops.stream()), "pd_vina_search")
        ops.check(L_.pd_vina_search_select(head[0], head[1], P(o[0]), P(o[1]), P(sel[0]), P(sel[1]), P(sel[2]), n_pose, K, A, Lg, ops.stream()),
                  "pd_vina_search_select")

    # composed
    n8 = n_pose * K
    _, head8 = r._poses(x8, "refine")
    numel8 = L_.pd_vina_refine_workspace_numel(n8, Lg, T)
    ws8 = f64(numel8)
    o8 = [torch.empty_like(x8), f64(n8), f64(n8), i32(n8), i32(n8), i32(n8), f64(n8)]

    def composed():
        for _ in range(steps + 1):
            ops.check(L_.pd_vina_refine(*head8, max_iters, grad_tol, max_step, P(ws8), numel8, *[P(t) for t in o8], None, n8, A, Lg, T, ops.stream()),
                      "pd_vina_refine")

    tf, tc = median_ms(fused, args.runs), median_ms(composed, args.runs)
    tp = median_ms(lambda: r.search(x, chains=K, steps=steps, rotate_amp=rot_amp, max_iters=max_iters), args.runs)
    ev_f, ev_c = int(o[5].sum()), int(o8[4].sum()) * (steps + 1)
    res = r.search(x, chains=K, steps=steps, rotate_amp=rot_amp, max_iters=max_iters)
    line = (f"P={n_pose} K={K} steps={steps} max_iters={max_iters} A={A} L={Lg} T={T}: fused pd_vina_search + select {tf[0]:.2f} ms (min {tf[1]:.2f}, max "
            f"{tf[2]:.2f}; {ev_f} evaluations of E), composed {steps + 1} x pd_vina_refine on {n8} poses {tc[0]:.2f} ms (min {tc[1]:.2f}, max {tc[2]:.2f}; "
            f"{ev_c} evaluations, the proposal step left out), fused / composed = {tf[0] / tc[0]:.2f}; VinaRefine.search {tp[0]:.2f} ms (min {tp[1]:.2f}, "
            f"max {tp[2]:.2f}); median of {args.runs} runs after one warm-up; E {float(res['energy_start'][:, 0].mean()):.3f} -> "
            f"{float(res['energy'].mean()):.3f} kcal/mol mean over the poses, accepted {float(res['accepted'].double().mean()):.1f} of {steps} steps per "
            f"chain, moved {float(res['moved'].mean()):.2f} A mean")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
