"""Time PoseClusters.cluster (csrc/cluster.hip) at n = 64 and 4096 poses (and 8192, the limit) next to the host path it stands beside,
D.cpu() + ranking.get_representatives(5), at the same n on the same box.  Two inputs per n: seven planted modes at cutoff 2.0 (K = 7)
and the same matrix at cutoff 0 (K = n singletons - the longest leader chain, the kernel's worst case).  Three figures per input:

  call     `spec.cluster(...)` in windows of `--calls` back-to-back calls between two device events, after a warm-up: the three
           launches, ten `torch.empty` and the Python of one call, as a caller who does not synchronise pays them;
  kernels  `pd_pose_clusters` alone on preallocated buffers, the same windows: the three launches;
  wall     one `spec.cluster(...)` between two synchronisations on the host clock: what a caller who waits for the result pays.

Each line gives the median and the spread over `--windows` windows (`wall`: over 30 calls).  At n = 64 `call` and `wall` are launch
and allocation overhead, not kernel time.  The host path is timed on the host clock; which K-means ran (scikit-learn or the
fallback of ranking.py) is printed.

    python tools/cluster_time.py [--out file]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physdock_amd import PoseClusters, ops  # noqa: E402
from physdock_amd.ranking import get_representatives  # noqa: E402


def planted(n, modes, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(n, 3, dtype=torch.float64)
    x[:, 0] = 8.0 * (torch.arange(n) % modes)
    x += (torch.rand(n, 3, generator=g, dtype=torch.float64) - 0.5) * 0.6
    d = torch.cdist(x, x).float()
    d = torch.triu(d, 1)
    return (d + d.T).contiguous()


def per_call_us(fn, calls, windows, warm=5):
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
    return statistics.median(ts), min(ts), max(ts)


def wall_us(fn, reps, warm, sync=True):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts), min(ts), max(ts)


def kernels_only(D, order, score, cutoff):
    """a closure that launches pd_pose_clusters on buffers allocated once"""
    n, dev = D.shape[0], D.device
    L_ = ops._lib.init()
    numel = L_.pd_pose_clusters_workspace_numel(n)
    ws = torch.empty(numel, dtype=torch.float64, device=dev)
    i32 = lambda m: torch.empty(m, dtype=torch.int32, device=dev)
    f32 = lambda m: torch.empty(m, dtype=torch.float32, device=dev)
    bufs = [i32(n), f32(n), i32(n), i32(n), f32(n), i32(n), f32(n), f32(n), i32(1)]      # labels .. n_clusters, the header's order
    ptrs = [ops.ptr(b) for b in bufs]
    d, o, s, w = ops.ptr(D), ops.ptr(order), ops.ptr(score), ops.ptr(ws)

    def launch():
        ops.check(L_.pd_pose_clusters(d, o, cutoff, None, s, w, numel, *ptrs, n, ops.stream()), "pd_pose_clusters")
    launch.keep = (bufs, ws)
    return launch


def fmt(t):
    return f"{t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    try:
        import sklearn  # noqa: F401
        kmeans = "scikit-learn KMeans"
    except ImportError:
        kmeans = "the farthest-point fallback (no scikit-learn)"
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    for n in (64, 4096, 8192):
        D = planted(n, 7, n).cuda()
        order = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(torch.int32).cuda()
        score = torch.randn(n, generator=torch.Generator().manual_seed(2)).cuda()
        for label, cutoff in (("7 planted modes, cutoff 2.0", 2.0), ("singletons, cutoff 0", 0.0)):
            spec = PoseClusters(cutoff)
            K = int(spec.cluster(D, order=order, scores=score)["n_clusters"])
            calls = args.calls if n * K < 1 << 22 else 5                              # the long chains: fewer calls per window
            call = per_call_us(lambda: spec.cluster(D, order=order, scores=score), calls, args.windows)
            kern = per_call_us(kernels_only(D, order, score, cutoff), calls, args.windows)
            wall = wall_us(lambda: spec.cluster(D, order=order, scores=score), 30, 3)
            say(f"n={n} {label}, K={K}: call {fmt(call)}; kernels {fmt(kern)}; {args.windows} windows of {calls} calls; wall {fmt(wall)} over 30 calls")
        if n <= 4096:
            host = wall_us(lambda: get_representatives(D.cpu().numpy().astype(np.float64), 5), 5 if n > 1000 else 20, 1, sync=False)
            say(f"n={n} host D.cpu() + get_representatives(5), {kmeans}: {fmt(host)} over {5 if n > 1000 else 20} calls")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
