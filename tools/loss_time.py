"""Time of PhysDockLoss and of each of its terms at the cfg1 (T = 256 / A = 2048) and cfg2 (T = 512 / A = 4096) shapes, B = 48:
median of repeated calls after warm-up, device time from events around a batch of calls.

    python tools/loss_time.py [--reps 20] [--out profiles/loss_time.txt]
"""
import argparse
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, inner=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from physdock_amd import PhysDockConfig, PhysDockLoss, loss
    from physdock_amd.synthetic import loss_features, loss_outputs, make_batch
    cfg = PhysDockConfig()
    lines = []
    for tag, (n_prot, n_lig) in (("cfg1", (224, 32)), ("cfg2", (448, 64))):
        f = loss_features(make_batch(n_prot, 9, n_lig, 8, seed=0), seed=6)
        o = {k: v.cuda() for k, v in loss_outputs(f, 48, seed=7).items()}
        f = {k: v.cuda() for k, v in f.items()}
        B, A, T = o["x_denoised"].shape[0], o["x_denoised"].shape[1], f["is_ligand"].shape[0]
        L = PhysDockLoss(cfg)
        both = {**o, **f}
        st = lambda t: {k: v for k, v in cfg.loss[t].items() if k != "weight"}
        runs = {"PhysDockLoss (5 terms + NaN check)": lambda: L(o, f), "terms only (no host read)": lambda: L.terms(o, f)}
        for t in ("weighted_mse_loss", "smooth_lddt_loss", "bond_loss", "distogram_loss"):
            runs[t + (" (+ key_res_loss, one pass)" if t == "bond_loss" else "")] = (lambda t=t: getattr(loss, t)(**both, **st(t)))
        lines.append(f"{tag}: B = {B}, A = {A}, T = {T}   (us per call: median / min / max of {args.reps} x 5 calls)")
        for name, fn in runs.items():
            med, lo, hi = timed(fn, args.reps)
            lines.append(f"  {name:42s} {med:9.1f} {lo:9.1f} {hi:9.1f}")
        m = (torch.cdist(f["x_gt"], f["x_gt"]) < 15.0).float().mean().item()
        lines.append(f"  smooth lDDT: {B * A * A:.3e} pair terms, {m:.3f} of the pairs inside the 15 A clamp")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
