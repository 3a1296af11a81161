"""Time FlexRefine.search (csrc/vina_flex.hip) with device events on the system of tools/flex_refine_time.py - P = 64 poses of a
32-atom ligand in a receptor of A = 2048 pose atoms - with 0, 4 and 10 flexible residues at the default `chains` and `steps`, next to
VinaRefine.search on the same poses in the same run.  The figure to read is the ratio to VinaRefine.search: per evaluation the kernel
does about (L + F) x A pair tests instead of L x A, so the ratio is expected near 1 with no flexible residue and at or below
(L + F) / L times the ratio of the evaluation counts otherwise.  Each timed window is `--calls` back-to-back calls between two events,
after a warm-up; a line reports the median and the spread of `--windows` windows.

    python tools/flex_search_time.py [--out file]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from flex_refine_time import system  # noqa: E402
from refine_time import per_call_us  # noqa: E402
from physdock_amd.flex import FlexRefine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    n_pose, Lg, A = 64, 32, 2048
    vina, r, xd, chains = system(n_pose, Lg, A)
    rot = r.default_rotate_amp(xd)                                                      # read back once, outside the timed windows
    kw = dict(seed=args.seed, rotate_amp=rot)
    lines = []
    base = per_call_us(lambda: r.search(xd, **kw), args.calls, args.windows)
    out = r.search(xd, **kw)
    ev0 = float(out["evaluations"].double().mean())
    K, steps = out["energy_chains"].shape[1], 20
    lines.append(f"VinaRefine.search P={n_pose} L={Lg} T={r.n_torsions} A={A} chains={K} steps={steps}: {base[0] / 1e3:.2f} ms per call (min "
                 f"{base[1] / 1e3:.2f}, max {base[2] / 1e3:.2f} over {args.windows} windows of {args.calls} calls), evaluations {ev0:.1f} per chain "
                 f"mean, E {float(out['energy_start'].mean()):.3f} -> {float(out['energy'].mean()):.3f} kcal/mol mean")
    for n_res in (0, 4, 10):
        use = chains[:n_res]
        rec_bonds = [b for ch in use for b in zip(ch[:-1], ch[1:])]
        tors = [[(ch[k], ch[k + 1]) for k in range(3)] for ch in use]
        f = FlexRefine.from_tables(vina.types, vina.ligand_idx, vina.rec_mask, vina.lig_active, vina.n_rot, r.rot, r.moving, r.intra, rec_bonds, tors,
                                   device="cuda")
        t = per_call_us(lambda: f.search(xd, **kw), args.calls, args.windows)
        o = f.search(xd, **kw)
        ev = float(o["evaluations"].double().mean())
        M = f.n_movable
        lines.append(f"FlexRefine.search residues={n_res} F={f.n_flex_atoms} S={f.n_flex_torsions} M={M}: {t[0] / 1e3:.2f} ms per call (min {t[1] / 1e3:.2f}, "
                     f"max {t[2] / 1e3:.2f}), ratio to VinaRefine.search {t[0] / base[0]:.2f} ((L+F)/L = {M / Lg:.2f}; x evaluations ratio "
                     f"{ev / ev0:.2f} = {M / Lg * ev / ev0:.2f}), evaluations {ev:.1f} per chain mean, accepted {float(o['accepted'].double().mean()):.1f} of "
                     f"{steps}, E {float(o['energy_start'].mean()):.3f} -> {float(o['energy'].mean()):.3f} kcal/mol mean, moved "
                     f"{float(o['moved'].mean()):.2f} A, moved_flex {float(o['moved_flex'].mean()):.2f} A mean")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
