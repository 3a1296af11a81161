"""Time the PAE / pTM pass of get_metrics (pd_metrics_pae_tm: table, one pass over the logits, combine) with device events: warm-up,
then the median of 20 launches, at T=256 P=1, T=512 P=1 and T=512 P=20, against a torch restatement (softmax + two weighted sums
+ the row reductions) on the same inputs.  Bytes = logits read + pae written.

    python tools/metrics_time.py [--out file]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physdock_amd import metrics  # noqa: E402

HBM_ACHIEVABLE = 6.0e12             # bytes / s, the project's streaming figure (NOTES.md: kernels on the HBM roof move 6 TB/s)


def median_ms(fn, n=20, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def torch_form(lg, w, asym, c):
    d0 = 1.24 * (torch.clamp(w.sum().long(), min=19) - 15).float() ** (1. / 3) - 1.8
    p = torch.softmax(lg, -1)
    pae = (p * c).sum(-1)
    tm = (p * (1. / (1 + c * c / (d0 * d0)))).sum(-1)
    out = [pae]
    for m in (torch.ones_like(tm[0]), (asym[:, None] != asym[None, :]).float()):
        pw = m * (w[None, :] * w[:, None])
        per = (tm * m * (pw / (1e-8 + pw.sum(-1, keepdim=True)))).sum(-1)
        out.append(torch.gather(per, 1, (per * w).argmax(-1, keepdim=True)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for T, P in ((256, 1), (512, 1), (512, 20)):
        g = torch.Generator(device="cuda").manual_seed(T + P)
        lg = torch.randn(P, T, T, 64, device="cuda", generator=g) * 2
        w = torch.ones(T, device="cuda")
        asym = (torch.arange(T, device="cuda") * 3 // T).int()
        c = metrics.bin_centres("cuda")
        t_hip = median_ms(lambda: metrics._pae_tm(lg, w, asym, 32.0))
        t_torch = median_ms(lambda: torch_form(lg, w, asym, c))
        nbytes = lg.numel() * 4 + P * T * T * 4
        lines.append(f"T={T} P={P}: pd_metrics_pae_tm {t_hip * 1e3:.1f} us = {nbytes / (t_hip * 1e-3) / 1e12:.2f} TB/s of {nbytes / 1e6:.1f} MB "
                     f"(achievable HBM {HBM_ACHIEVABLE / 1e12:.1f} TB/s); torch restatement {t_torch * 1e3:.1f} us ({t_torch / t_hip:.1f} x)")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
