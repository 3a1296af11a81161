"""Time DistogramScore (csrc/distogram_score.hip) with device events at P = 64 poses of a system of T = 256 tokens - 224 receptor tokens
of eight atoms and 32 ligand tokens of one atom, K = 39 bins: the table kernel alone (pd_distogram_tables, once per system), `score`
(pd_distogram_score + pd_distogram_reduce and five allocations) and `potential(forces=True)` (two launches and four allocations).  Each
timed window is `--calls` back-to-back calls between two events, after a warm-up; a line reports the median and the spread of
`--windows` windows per call.  Nothing is tuned and no time is a pass criterion.

    python tools/distogram_score_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from physdock_amd import ops  # noqa: E402
from physdock_amd.distogram import DistogramScore  # noqa: E402
from sasa_time import per_call_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    n_pose, T_rec, T_lig, K = 64, 224, 32, 39
    T = T_rec + T_lig
    rng = np.random.default_rng(39)
    chunk = np.concatenate([np.full(T_rec, 8), np.ones(T_lig, np.int64)])
    start = np.cumsum(chunk) - chunk
    A = int(chunk.sum())
    side = 7
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    sites = (grid - (side - 1) / 2.0) * 3.8
    sites = sites[np.argsort((sites ** 2).sum(-1), kind="stable")][:T_rec]
    x = rng.normal(size=(n_pose, A, 3)) * 1.2
    for t in range(T):
        x[:, start[t]:start[t] + chunk[t]] += sites[t] if t < T_rec else rng.normal(size=3) * 2.0
    raw = rng.uniform(-2, 2, (T, T, K))
    batch = {"token_id_to_pseudo_beta_atom_id": torch.from_numpy(start + np.minimum(chunk - 1, 4)),
             "is_ligand": torch.from_numpy(np.concatenate([np.zeros(T_rec), np.ones(T_lig)]).astype(np.float32)),
             "x_gt": torch.from_numpy(x[0].astype(np.float32))}
    spec = DistogramScore.from_logits(torch.from_numpy((raw + raw.transpose(1, 0, 2)).astype(np.float32)).cuda(), batch)
    x = torch.from_numpy(x.astype(np.float32)).cuda()
    t = spec.tables("cuda")
    out = spec.score(x)
    assert bool((out["ok"] == 1).all()) and bool(torch.isfinite(out["nll_interface"]).all())
    tab = per_call_us(lambda: ops.distogram_tables(t["logits"], spec.centres, spec.contact_bin, t["lse"], t["expected"], t["p_contact"]),
                      args.calls, args.windows)
    sc = per_call_us(lambda: spec.score(x), args.calls, args.windows)
    po = per_call_us(lambda: spec.potential(x, forces=True), args.calls, args.windows)
    line = (f"P={n_pose} T={T} ligand tokens={T_lig} A={A} K={K}: tables {tab[0]:.1f} us per call (min {tab[1]:.1f}, max {tab[2]:.1f} over "
            f"{args.windows} windows of {args.calls} calls; once per system), score {sc[0]:.1f} us (min {sc[1]:.1f}, max {sc[2]:.1f}; two kernels "
            f"plus five allocations), potential(forces=True) {po[0]:.1f} us (min {po[1]:.1f}, max {po[2]:.1f}; two kernels plus four "
            f"allocations); untuned; mean nll_interface {float(out['nll_interface'].mean()):.3f}, contacts per pose "
            f"{float(out['n_contacts'].float().mean()):.1f}")
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
