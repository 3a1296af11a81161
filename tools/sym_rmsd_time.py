"""Time pd_sym_rmsd (symmetry-corrected pairwise ligand RMSD, csrc/sym_rmsd.hip) with device events: warm-up, then the median of
20 launches, at n = 100 poses, L = 44 and 64 ligand atoms and M = 1, 12, 288, 4096 table rows (random permutations, identity
first; the kernel's work does not depend on the table being a group).  M = 1 is timed against pd_pairwise_rmsd, the other sizes
against a torch restatement on the same inputs (gather by the table, squared differences, mean, amin), which is also used to
check the values.  Terms = n (n + 1) / 2 * M * L distance terms (upper triangle and the reference column).

    python tools/sym_rmsd_time.py [--out file]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physdock_amd.ranking import pairwise_ligand_rmsd  # noqa: E402
from physdock_amd.symmetry import LigandSymmetry  # noqa: E402


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


def torch_form(lig, ref, perms, chunk=8):
    """lig [n,L,3], ref [L,3], perms long [M,L] -> (D [n,n], r [n]); pose j permuted, `chunk` rows i at a time to bound the memory"""
    n = lig.shape[0]
    other = torch.cat([lig, ref[None]])[:, perms]                      # [n+1,M,L,3]
    out = []
    for i0 in range(0, n, chunk):
        d = lig[i0:i0 + chunk, None, None] - other[None]               # [c,n+1,M,L,3]
        out.append((d * d).sum(-1).mean(-1).amin(-1))
    c = torch.cat(out).sqrt()
    return c[:, :n], c[:, n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, lines = 100, []
    for Lg in (44, 64):
        for M in (1, 12, 288, 4096):
            rng = np.random.default_rng(Lg * 10000 + M)
            A = Lg + 300
            x = torch.from_numpy((rng.standard_normal((n, A, 3)) * 5).astype(np.float32)).cuda()
            x_gt = torch.from_numpy((rng.standard_normal((A, 3)) * 5).astype(np.float32)).cuda()
            idx = torch.arange(300, A, dtype=torch.int32, device="cuda")
            table = np.stack([np.arange(Lg)] + [rng.permutation(Lg) for _ in range(M - 1)])
            sym = LigandSymmetry.from_permutations(table, device="cuda")
            t_hip = median_ms(lambda: pairwise_ligand_rmsd(x, idx, x_gt, symmetry=sym))
            D, r = pairwise_ligand_rmsd(x, idx, x_gt, symmetry=sym)
            terms = n * (n + 1) / 2 * M * Lg
            head = f"n={n} L={Lg} M={M}: pd_sym_rmsd {t_hip * 1e3:.1f} us ({terms / (t_hip * 1e-3) / 1e9:.1f} G terms/s)"
            if M == 1:
                t_ref = median_ms(lambda: pairwise_ligand_rmsd(x, idx, x_gt))
                D0, r0 = pairwise_ligand_rmsd(x, idx, x_gt)
                tail = f"pd_pairwise_rmsd {t_ref * 1e3:.1f} us ({t_ref / t_hip:.2f} x)"
            else:
                lig, rl, pl = x[:, idx.long()], x_gt[idx.long()], torch.from_numpy(table).cuda()
                chunk = 8 if M <= 288 else 1
                t_ref = median_ms(lambda: torch_form(lig, rl, pl, chunk), n=20 if M <= 288 else 5, warm=5 if M <= 288 else 1)
                D0, r0 = torch_form(lig, rl, pl, chunk)
                D0 = torch.triu(D0, 1) + torch.triu(D0, 1).T         # the kernel mirrors the upper triangle
                tail = f"torch restatement {t_ref * 1e3:.1f} us ({t_ref / t_hip:.1f} x)"
            err = max(float((D - D0).abs().max()), float((r - r0).abs().max()))
            lines.append(f"{head}; {tail}; max |difference| {err:.1e}")
            print(lines[-1], flush=True)
            del sym
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
