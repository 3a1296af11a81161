"""Poses/s of PhysDock.sample_diffusion_many at the screening regime: G in {1, 2, 3, 4} systems x 20 samples per call, medium model,
cfg1-size systems of different real sizes, 40 steps with template projection, graphs warm.  The single-system 20-sample rate
(sample_diffusion) and parallel.StreamPool's two-stream rate are measured in the same process.  Each rate is the median of
`--reps` timed repetitions (n calls each); min / max give the spread.

    python tools/multi_system_time.py [--reps 3] [--calls 4]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from physdock_amd import PhysDock, PhysDockConfig, param_shapes, seeded_state_dict  # noqa: E402
from physdock_amd.synthetic import cfg1_batch, make_batch, reference_conformers  # noqa: E402


def rate(fn, poses, reps, calls):
    for _ in range(2):
        fn(0)                                   # warm: every unit graph captured
    out = []
    for r in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(calls):
            fn(1 + r * calls + i)
        torch.cuda.synchronize()
        out.append(poses * calls / (time.perf_counter() - t0))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--samples", type=int, default=20)
    args = ap.parse_args()
    cfg = PhysDockConfig(model_name="medium")
    model = PhysDock(cfg)
    model.load_state_dict(seeded_state_dict(param_shapes(cfg), seed=0))
    model = model.cuda().eval()
    raw = [cfg1_batch(0), make_batch(221, 8, 35, 64, 2), make_batch(210, 9, 30, 128, 3), make_batch(200, 9, 40, 128, 4)]
    systems = [({k: v.cuda() for k, v in b.items()}, reference_conformers(b, n_conf=8, seed=11 + i).cuda()) for i, b in enumerate(raw)]
    B = args.samples
    kw = dict(num_sample=B, steps=40, karras_noise_schedule_power=1000, align_ref_pos=True, mmff_gamma_0_factor=6.0)
    for i, (b, _) in enumerate(systems):
        print(f"system {i}: A = {b['ref_pos'].shape[0]}, T = {b['target_feat'].shape[0]}", flush=True)

    def single(seed):
        b, c = systems[0]
        model.sample_diffusion(b, seed=seed, ref_mol_poses=c, use_ref_mol_poses=True, **kw)
    r = rate(single, B, args.reps, args.calls)
    print(f"sample_diffusion, 1 system x {B}: {r[0]:.1f} poses/s (min {r[1]:.1f}, max {r[2]:.1f})", flush=True)

    from physdock_amd.parallel import StreamPool
    pool = StreamPool.for_model(model, n=2)

    def two_streams(seed):
        pool.map(lambda m, it: m.sample_diffusion(it[0], seed=seed, ref_mol_poses=it[1], use_ref_mol_poses=True, **kw), systems[:2])
    r = rate(two_streams, 2 * B, args.reps, args.calls)
    print(f"StreamPool, 2 streams x 1 system x {B}: {r[0]:.1f} poses/s (min {r[1]:.1f}, max {r[2]:.1f})", flush=True)
    model._stream_pool = None
    del pool
    torch.cuda.empty_cache()

    for G in (1, 2, 3, 4):
        grp = systems[:G]

        def many(seed):
            model.sample_diffusion_many([b for b, _ in grp], seeds=[seed * 8 + g for g in range(G)], ref_mol_poses=[c for _, c in grp], **kw)
        r = rate(many, G * B, args.reps, args.calls)
        print(f"sample_diffusion_many, G = {G} x {B}: {r[0]:.1f} poses/s (min {r[1]:.1f}, max {r[2]:.1f})  "
              f"workspace {model.engine(torch.device('cuda', 0)).ws.nbytes() / 2 ** 30:.1f} GiB", flush=True)


if __name__ == "__main__":
    main()
