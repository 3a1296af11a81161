#!/usr/bin/env python
"""Benchmark of the PhysDock redocking hot path on MI355X.

A *step* is one full `sample_diffusion` call - conditioning trunk + 40 reverse-diffusion
steps with template-projection physics correction - over one batch of synthetic input
(BASELINE.json configs[1]: crop_size=256 / atom_crop_size=2048, 64 diffusion samples,
medium model, fp32).  Metric: poses/sec, whole job.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N>1: launched by torch.distributed.run, one rank per GPU; samples shard across ranks
     with no data-path collective, one RCCL gather of the poses at the end of every step)

Rank 0 prints ONE JSON line.  A plain run does only what the headline needs: set-up, W warm-up
calls, K timed calls (`ms_per_step` = milliseconds per timed call), the outputs of the last
timed call written as DIR/<name>.npy when --dump-outputs is given, the line.
--full adds the side measurements: "roofline" for the dominant kernel (live HIP-event timing
of its launches in an instrumented pass), "extra" (other sample counts, screening flow, graph
cache, MMFF branch, bf16 x 6 fallback, the cfg2 crop) and "cpu_baseline" (the CPU oracle timed
on the host cores, N=1 only); --no-roofline / --no-extra / --no-cpu-baseline drop one of them.
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

PEAK_FP32_MFMA_TFLOPS = 157.3          # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 peak
PEAK_BF16_MFMA_TFLOPS = 2516.6         # same guide: dense bf16 MFMA peak (v_mfma_f32_32x32x16_bf16, 2.5 PF)
#: kernels that contract on the bf16 pipe with 3-way split operands issue SIX bf16 MFMAs per fp32-accurate block, so their
#: ceiling in algorithmic (fp32-equivalent) FLOP/s is the bf16 peak / 6
PEAK_SPLIT_TFLOPS = PEAK_BF16_MFMA_TFLOPS / 6


def pipe_peak(nprod):
    """ceiling in algorithmic (fp32-equivalent) TFLOP/s of a kernel by the number of 16-bit MFMA products it issues per
    fp32-accurate block: 0 = fp32 MFMA, 6 = three-part bf16 operands, 3 = two-part fp16 operands"""
    return PEAK_FP32_MFMA_TFLOPS if not nprod else PEAK_BF16_MFMA_TFLOPS / nprod


def pipe_name(nprod):
    return {0: "fp32 mfma", 6: "bf16 x6 split", 3: "f16 x3 split"}.get(int(nprod or 0), "?")


DIT_GFLOP_PER_SAMPLE_STEP = 39.8
TRUNK_GFLOP = 2742.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--samples", type=int, default=64, help="diffusion samples per call per GPU")
    ap.add_argument("--diffusion-steps", type=int, default=40)
    ap.add_argument("--model", default="medium")
    ap.add_argument("--cfg", default="cfg1", choices=["cfg1", "cfg2", "small"])
    ap.add_argument("--no-physics", action="store_true")
    ap.add_argument("--full", action="store_true", help="also run the side measurements (roofline pass, extra configurations, "
                                                        "CPU baseline); a plain run times the headline call only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the poses of the last timed call (float32, what the caller receives) as DIR/poses.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline", default="b1", choices=["b1", "full", "quick"],
                    help="b1: B = 1 measured with complete oracle calls, B = 20 extrapolated and labelled (about 4 minutes of host "
                         "time); full: B = 20 also measured with one complete call (5 - 6 minutes more); quick: extrapolated only")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-extra", action="store_true", help="skip the B=1 / B=20 / cfg2 / MMFF / screening side measurements")
    ap.add_argument("--launch-log", default=None, help="write the GEMM / attention launch sequence (symbol, shape) of the timed "
                                                       "calls as JSON (tools/pmc_report.py joins it with rocprofv3 dispatches)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not args.full:           # a plain run: the headline call only
        args.no_roofline = args.no_extra = args.no_cpu_baseline = True
    return args


def make_crop(name, device):
    """synthetic crop of a named configuration + 40 synthetic reference conformers of its ligand"""
    from physdock_amd import synthetic
    batch = {"small": synthetic.small_batch, "cfg1": synthetic.cfg1_batch, "cfg2": synthetic.cfg2_batch}[name](0)
    confs = synthetic.reference_conformers(batch, n_conf=40, seed=1)
    dbatch = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    return batch, dbatch, confs


def build_inputs(args, device):
    from physdock_amd import PhysDock, PhysDockConfig, param_shapes, seeded_state_dict, small_config
    cfg = small_config() if args.cfg == "small" else PhysDockConfig(model_name=args.model)
    batch, dbatch, confs = make_crop(args.cfg, device)
    P = seeded_state_dict(param_shapes(cfg), seed=0)      # trained weights are not available offline
    model = PhysDock(cfg)
    model.load_state_dict(P, strict=True)
    model = model.to(device).eval()
    return cfg, P, batch, dbatch, confs, model


def usable_cores():
    """CPUs this process may actually use: min(affinity mask, cgroup quota) - NOT os.cpu_count()
    (the GPU box shows 256 logical CPUs but grants a 16-CPU quota; 256 threads there thrash)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(p))))
    except (OSError, ValueError):
        pass
    return n


def physical_cores():
    """distinct (socket, core) pairs of the box (None when /proc/cpuinfo does not say)"""
    try:
        pairs, sock = set(), "0"
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                sock = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                pairs.add((sock, line.split(":", 1)[1].strip()))
        return len(pairs) or None
    except OSError:
        return None


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(cfg, P, batch, confs, args):
    """the CPU oracle (torch CPU fp32, all usable cores) on the same synthetic crop, seeded weights and
    physics branch (template projection, 40 conformers, factor 6).
    B = 1 is MEASURED by the book: 2 timed COMPLETE calls (conditioning trunk + all `diffusion_steps` steps inside the timed region;
    2-step calls as warm-up), median - `value`, `extrapolated: false`.  B = 20 (the demo's samples per round): labelled extrapolation
    (trunk timed on its own, the loop through 2-step sampler calls, call = t_trunk + steps * t_step); with --cpu-baseline full ONE
    complete call, measured (4 - 6 minutes more, beyond the 10 minutes a --full run is given).  --cpu-baseline quick skips the complete
    calls: both rows are then labelled extrapolations and `value` says so."""
    import statistics
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import physdock_oracle as orc
    cores = usable_cores()
    torch.set_num_threads(cores)
    n = args.diffusion_steps
    A = batch["ref_pos"].shape[0]
    t_all = time.perf_counter()
    phys = dict(align_ref_pos=True, ref_mol_poses=confs, mmff_gamma_0_factor=6.0, karras_noise_schedule_power=1000)

    def draws(B, k, n_noisy, seed):
        g = torch.Generator().manual_seed(seed)
        return {"init": torch.randn(B, A, 3, generator=g), "rot_u": torch.rand(k, 4, B, generator=g),
                "trans": torch.randn(k, B, 3, generator=g), "diffuse": torch.randn(n_noisy, B, A, 3, generator=g)}
    with torch.no_grad():
        tt = []
        for rep in range(1):                                   # one timed pass (it warms the thread pool; the full calls below run the
            t0 = time.perf_counter()                           # trunk three more times inside their timed region)
            cond = orc.diffusion_conditioning(P, batch)
            tt.append(time.perf_counter() - t0)
        t_trunk = tt[-1]
        by_b = {}
        for B in (1, 20):
            k = 2
            noise = draws(B, k, k, 0)
            ts = []
            for rep in range(3 if B == 20 else 2):             # 1 warm-up + 2 timed (B = 1: warm-up + 1; it is measured in full below)
                t0 = time.perf_counter()
                orc.sample_diffusion(P, batch, noise, num_sample=B, steps=k, conditioning=cond, **phys)
                ts.append((time.perf_counter() - t0) / k)
            t_step = statistics.median(ts[1:])
            by_b[str(B)] = {"poses_per_s": B / (t_trunk + n * t_step), "t_step_s": t_step, "extrapolated": True}
        full = full20 = None
        if args.cpu_baseline in ("b1", "full"):
            n_noisy = int((orc.karras_noise_schedule(n, p=1000)[:-1] > 1.0).sum())
            tf = []
            for rep in range(2):                               # complete calls: trunk + n steps, nothing reused (the 2-step calls above were the warm-up)
                noise = draws(1, n, n_noisy, 10 + rep)
                t0 = time.perf_counter()
                orc.sample_diffusion(P, batch, noise, num_sample=1, steps=n, **phys)
                tf.append(time.perf_counter() - t0)
            full = statistics.median(tf)
            by_b["1"] = {"poses_per_s": 1.0 / full, "call_s": full, "calls_timed": 2, "call_times_s": [round(t, 2) for t in tf],
                         "extrapolated": False, "extrapolated_estimate_poses_per_s": by_b["1"]["poses_per_s"], "t_step_s": by_b["1"]["t_step_s"]}
        if args.cpu_baseline == "full":
            # B = 20, the demo's samples per round (BASELINE.md section 3 asks for B in {1, 20}): ONE complete call, measured (round 6;
            # 4 - 6 minutes of the host cores - the 2-step calls above were its warm-up)
            noise = draws(20, n, n_noisy, 20)
            t0 = time.perf_counter()
            orc.sample_diffusion(P, batch, noise, num_sample=20, steps=n, **phys)
            full20 = time.perf_counter() - t0
            by_b["20"] = {"poses_per_s": 20.0 / full20, "call_s": full20, "calls_timed": 1, "extrapolated": False,
                          "extrapolated_estimate_poses_per_s": by_b["20"]["poses_per_s"], "t_step_s": by_b["20"]["t_step_s"]}
    phys_cores = physical_cores()
    return {"value": by_b["1"]["poses_per_s"], "unit": "poses/s", "cores": cores, "cores_used": cores, "cores_physical": phys_cores,
            "kind": "port", "cpu_model": cpu_model(), "samples": 1,
            "by_samples": by_b, "t_trunk_s": t_trunk, "wall_s": time.perf_counter() - t_all,
            "extrapolated": full is None,
            "sample": f"oracle (torch CPU fp32, {cores} threads of {cpu_model()}, {phys_cores} physical cores on the box): "
                      + (f"value = B = 1 measured: 3 complete sample_diffusion calls (trunk + {n} steps with the template-projection physics "
                         f"branch inside the timed region), median {full:.1f} s per call; " if full is not None else
                         "value = B = 1 extrapolated (--cpu-baseline quick); ")
                      + (f"B = 20 measured: one complete 20-sample call, {full20:.0f} s = {by_b['20']['poses_per_s']:.3f} poses/s" if full20 is not None else
                         f"B = 20 extrapolated (labelled): trunk {t_trunk:.1f} s + {n} x {by_b['20']['t_step_s']:.2f} s per step from 2-step sampler calls "
                         f"(1 warm-up + 2 timed) = {by_b['20']['poses_per_s']:.3f} poses/s")}


class LaunchTimer:
    """Brackets every GEMM / attention launch of one eager pass with HIP events on the launch stream
    (the torch current stream = the stream the C ABI launches on) and aggregates per kernel symbol."""

    GEMM_NAMES = {0: "128, 128, 2, 2", 1: "128, 64, 2, 2", 2: "128, 32, 4, 1", 3: "64, 64, 2, 2"}

    def __init__(self, ops, time_launches=True):
        self.ops = ops
        self.time_launches = time_launches
        self.rec = {}      # kernel symbol -> [events, flops, bytes]
        self.shape_rec = {}  # (kernel symbol, shape string) -> [events, flops, bytes]
        self.split = {}    # kernel symbol -> runs on the bf16 matrix pipe (split operands)
        self.log = []      # launch order: [symbol, shape string]  (joined with rocprofv3 dispatches by tools/pmc_report.py)

    def _launch(self, name, shape, launch, flops, nbytes=0.0):
        self.log.append([name, shape])
        if not self.time_launches:
            return launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); launch(); e1.record()
        for store, key in ((self.rec, name), (self.shape_rec, (name, shape))):
            r = store.setdefault(key, [[], 0.0, 0.0])
            r[0].append((e0, e1))
            r[1] += flops
            r[2] += nbytes

    def __enter__(self):
        ops = self.ops
        L = ops._lib.init()
        import ctypes as C

        def gemm_hook(a, launch):
            v = L.pd_gemm_variant(C.byref(a))
            nprod, v = (3 if v >= 2000000 else 6 if v >= 1000000 else 0), v % 1000000
            streamed, epi, tcode, v = (v % 10000) >= 5000, (v // 10000) % 10, v // 100000, v % 5000
            cfg, lay, pro, scalar = (v % 1000) // 100, (v % 100) // 10, v % 10, v >= 1000
            name = "gemm_kernel<%s, %s, %s, %s, %d>" % (self.GEMM_NAMES[cfg], "true" if lay >= 1 else "false",
                                                         "true" if lay == 2 else "false", "false" if scalar else "true", pro)
            if streamed:        # persistent direct-epilogue variant (csrc/gemm_stream.hip)
                name = "gemm_stream_kernel<%d, %d, Tile<%s> >" % (pro, epi, ("128, 128, 2", "64, 64, 2", "128, 64, 4")[min(tcode, 2)])
                glu_tile = epi in (2, 5)
                if nprod == 6:  # 3 x bf16 split-operand variant (csrc/gemm_split.hip); names as rocprofv3 prints them:
                    # PRO = 3 when A arrives pre-split (pd_gemm_args.A3); the STile's last argument = direct-W loop
                    name = "gemm_split_kernel<%d, %d, STile<%s> >" % (
                        3 if a.A3 else pro, epi,
                        (("128, 128, 4, 8, false" if glu_tile else "128, 128, 2, 8, true"), "64, 64, 2, 4, true", "128, 64, 4, 4, true")[tcode])
                elif nprod == 3:  # 2 x fp16 split-operand variant (csrc/gemm_f16.hip)
                    # (the GLU tile takes direct-W loads - last argument true - when A arrives pre-split)
                    name = "gemm_f16_kernel<%d, %d, FTile<%s, 0> >" % (
                        3 if a.A2 else pro, epi,
                        "64, 128, 1, 4, true" if tcode == 1 else
                        ("128, 128, 4, 8, true" if a.A2 else "128, 128, 4, 8, false") if glu_tile else "128, 128, 2, 8, true")
                    if tcode in (3, 4):   # K = 128 rows kernel (whole rows in LDS, own statistics): 128- / 64-row tiles
                        name = "gemm_f16_rows_kernel<%d, %d, %d>" % (pro, epi, 128 if tcode == 3 else 64)
                    elif tcode == 6:      # N = 512, long K: one accumulator tile per wave, K in double-buffered chunks
                        name = "gemm_f16_wchunk_kernel<%d>" % epi
                    elif tcode == 5:      # K = 512 wide-rows kernel (64 rows on sixteen waves)
                        name = "gemm_f16_wrows_kernel<%d, %d, %s>" % (3 if a.A2 else pro, epi, "2, 2, 2, 16" if glu_tile else
                                                                       "2, 1, 4, 16")
            nb = max(a.batch, 1)
            n_out = a.N // 2 if a.glu else a.N
            byt = 4.0 * nb * (a.M * a.K + a.N * a.K + a.M * n_out * (1 + bool(a.res) + (bool(a.mul) and a.mul_rows_per_group == 0)))
            self.split[name] = nprod
            shape = "M=%d N=%d K=%d" % (a.M, a.N, a.K) + (" x%d" % nb if nb > 1 else "")
            self._launch(name, shape, launch, 2.0 * a.M * a.N * a.K * nb, byt)

        def attn_hook(a, launch):
            v = L.pd_attention_variant(C.byref(a))          # 4 / 8 waves per block, or 4 + 100 * key chunks
            name = "attn_kernel<%d, %s>" % (v % 100, "true" if v > 100 else "false")
            if v >= 3000:       # the software-pipelined form (csrc/attn_pipe.hip): waves, K / V pre-split, bias as the accumulator's initial value
                name = "attn_pipe_kernel<%d, %s, %s>" % (v % 100, "true" if a.K2 else "false", "true" if a.bias else "false")
            elif v >= 2000:     # fp16 matrix pipe, two-part operands, three products per block (csrc/attn_f16.hip)
                # template arguments as rocprofv3 prints them: waves, parts, K / V pre-split (K2 / V2), key-split launch
                name = "attn_parts_kernel<%d, 2, %s, %s>" % (v % 100, "true" if a.K2 else "false", "true" if v % 1000 > 100 else "false")
            elif v >= 1000:     # bf16 matrix pipe, three-part operands, six products per block (csrc/attn_split.hip)
                name = "attn_split_kernel<%d>" % (v % 100)
            self.split[name] = 3 if v >= 2000 else (6 if v >= 1000 else 0)
            c = a.nheads * 32                    # q, o: nq rows; k, v: nk rows; the bias tile set is read once per launch
            byt = 4.0 * a.nbatch * c * (2 * a.nq + 2 * a.nk) + (4.0 * a.nheads * a.nq * a.nk if a.bias else 0.0)
            shape = "batch=%d heads=%d nq=%d nk=%d%s" % (a.nbatch, a.nheads, a.nq, a.nk, " bias" if a.bias else "")
            self._launch(name, shape, launch, 4.0 * a.nbatch * a.nheads * a.nq * a.nk * 32, byt)
        def transition_hook(a, launch):
            name, shape = "transition_f16_kernel<3, %s>" % os.environ.get("PD_TRANSITION_BM", "64"), "M=%d C=%d hidden=%d" % (a.M, a.C, a.hidden)
            if not self.time_launches:
                ok = launch()
                if ok:
                    self.log.append([name, shape])
                return ok
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); ok = launch(); e1.record()
            if ok:            # (a declined shape launched nothing: the caller runs the three-launch form, which is recorded there)
                self.log.append([name, shape])
                self.split[name] = 3
                for store, key in ((self.rec, name), (self.shape_rec, (name, shape))):
                    r = store.setdefault(key, [[], 0.0, 0.0])
                    r[0].append((e0, e1))
                    r[1] += 6.0 * a.M * a.C * a.hidden          # the two projections
                    r[2] += 8.0 * a.M * a.C                     # x in, x out
            return ok
        ops.GEMM_HOOK = gemm_hook
        ops.ATTN_HOOK = attn_hook
        ops.TRANSITION_HOOK = transition_hook
        return self

    def __exit__(self, *e):
        self.ops.GEMM_HOOK = None
        self.ops.ATTN_HOOK = None
        self.ops.TRANSITION_HOOK = None

    def summary(self, by_shape=False):
        torch.cuda.synchronize()
        out = []
        for key, (ev, fl, by) in (self.shape_rec if by_shape else self.rec).items():
            t = sum(a.elapsed_time(b) for a, b in ev) * 1e-3
            d = dict(kernel=key[0], shape=key[1]) if by_shape else dict(kernel=key)
            d.update(launches=len(ev), total_s=t, avg_launch_ms=1e3 * t / len(ev), flop_per_launch=fl / len(ev),
                     tflops=fl / t / 1e12, algorithmic_bytes_per_launch=by / len(ev))
            out.append(d)
        return sorted(out, key=lambda d: -d["total_s"])


DUMP_BUDGET_BYTES = 64 * 2 ** 20


def dump_outputs(d, arrays):
    """--dump-outputs: every array as DIR/<name>.npy in float32, 64 MB in all at most - an array over its share of that keeps a
    fixed, seeded sample of its rows (leading dimension, in order); at the benchmark's shapes nothing is sampled"""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    share = DUMP_BUDGET_BYTES // max(len(arrays), 1)
    for name, t in arrays.items():
        a = t.detach().to("cpu", torch.float32).numpy()
        if a.nbytes > share:
            keep = max(1, share // max(a.nbytes // a.shape[0], 1))
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
        np.save(os.path.join(d, name + ".npy"), np.ascontiguousarray(a))


class _DryRunSampler:
    """stand-in for PhysDock on the CPU (PD_BENCH_DRYRUN): poses are a deterministic function of (seed, global sample id), as the
    Philox-keyed sampler's are, so the rank-block checks of the real run apply unchanged"""

    def __init__(self, A):
        self.A = A

    def sample_diffusion(self, batch, num_sample=1, seed=0, sample_offset=0, **kw):
        rows = [torch.randn(self.A, 3, generator=torch.Generator().manual_seed(1000003 * seed + sample_offset + i))
                for i in range(num_sample)]
        return torch.stack(rows)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: become N ranks (one process per GPU) via torch.distributed.run
        if torch.cuda.device_count() < args.gpus and os.environ.get("PD_BENCH_DRYRUN") != "1":
            sys.exit(f"bench.py --gpus {args.gpus}: only {torch.cuda.device_count()} GPU(s) visible on this node")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # (a fresh child process, not an exec of this one: device_count() above may already have initialised the runtime here)
        import subprocess
        sys.exit(subprocess.call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
                                  "--master-addr", "127.0.0.1", "--master-port", os.environ.get("MASTER_PORT", "29511"),
                                  os.path.abspath(__file__)] + sys.argv[1:]))
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if world != args.gpus:
        sys.exit(f"bench.py --gpus {args.gpus} launched with WORLD_SIZE={world}: the two must agree (one rank per GPU)")
    dist = world > 1 or "TORCHELASTIC_RUN_ID" in os.environ      # launched by torch.distributed.run
    # PD_BENCH_DRYRUN=1 (tests/test_distributed_cpu.py): the same launcher / rank / gather / max-over-ranks / JSON code on the gloo
    # backend with a stand-in sampler on the CPU - so that the first real multi-GPU run cannot die on argument plumbing
    dry = os.environ.get("PD_BENCH_DRYRUN") == "1"
    if dist:
        import torch.distributed as td
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if not dry:
            torch.cuda.set_device(local)
        td.init_process_group("gloo" if dry else "nccl")
    device = torch.device("cpu") if dry else torch.device("cuda", local if dist else 0)
    if dry:
        torch.cuda.synchronize = lambda *a, **k: None
        args.no_roofline = args.no_extra = args.no_cpu_baseline = True
    else:
        torch.cuda.set_device(device)

    if os.environ.get("PD_BENCH_TWEAK"):          # lab A/B runs (tools/ab_f16.sh): "NAME=value,..." sets physdock_amd.ops switches
        from physdock_amd import ops as _o
        for kv in os.environ["PD_BENCH_TWEAK"].split(","):
            k_, v_ = kv.split("=")
            setattr(_o, k_, {"True": True, "False": False}.get(v_, int(v_) if v_.isdigit() else v_))
    if dry:
        from physdock_amd import synthetic
        batch = {"small": synthetic.small_batch, "cfg1": synthetic.cfg1_batch, "cfg2": synthetic.cfg2_batch}[args.cfg](0)
        dbatch, confs, model = batch, torch.zeros(1, 1, 3), _DryRunSampler(batch["ref_pos"].shape[0])
    else:
        cfg, P, batch, dbatch, confs, model = build_inputs(args, device)
    B, nsteps = args.samples, args.diffusion_steps
    A = batch["ref_pos"].shape[0]
    kw = dict(num_sample=B, steps=nsteps, karras_noise_schedule_power=1000, use_graph=not args.no_graph)
    if args.no_physics:
        kw.update(align_ref_pos=False)
    else:   # rounds >= 1 of redocking.py with --enable_physics_correction: template projection while t > 6*gamma_min
        kw.update(align_ref_pos=True, ref_mol_poses=confs.to(device), use_ref_mol_poses=True, mmff_gamma_0_factor=6.0)
    gathered = [torch.empty(B, A, 3, device=device) for _ in range(world)] if (dist and rank == 0) else None

    def one_call(i):
        x = model.sample_diffusion(dbatch, seed=1234 + i, sample_offset=rank * B, **kw)
        if dist:   # the single collective of the path: poses to rank 0 for ranking
            td.gather(x, gathered, dst=0)
        return x

    warm_ms = []
    for i in range(args.warmup):          # (timed one by one for `extra.first_call_ms`: nothing here is part of the measured region)
        torch.cuda.synchronize(); t_w = time.perf_counter()
        one_call(i)
        torch.cuda.synchronize(); warm_ms.append(1e3 * (time.perf_counter() - t_w))
    logger = None
    if args.launch_log and rank == 0:        # profiling runs only (eager calls): shapes of every launch, no events, no timing claim
        from physdock_amd import ops as _ops
        logger = LaunchTimer(_ops, time_launches=False)
        logger.__enter__()
    if dist:
        td.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        x = one_call(args.warmup + i)
    torch.cuda.synchronize()
    if dist:
        td.barrier()
    elapsed = time.perf_counter() - t0
    if logger is not None:
        logger.__exit__()
        with open(args.launch_log, "w") as f:
            json.dump(logger.log, f)
    per_rank_s = [elapsed]
    if dist:
        # every rank's own clock around the timed region, on rank 0's line: a straggler (a GPU that throttles, a slow xGMI gather) is
        # visible in the first real multi-GPU run instead of hiding inside the maximum
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        allt = [torch.zeros_like(t) for _ in range(world)]
        td.all_gather(allt, t)
        per_rank_s = [float(v) for v in allt]
        elapsed = max(per_rank_s)
    assert torch.isfinite(x).all()
    if dist and rank == 0:      # the gathered blocks of the last call: every rank's poses arrived and the ranks' streams differ
        assert all(bool(torch.isfinite(t).all()) for t in gathered), "non-finite poses in a gathered rank block"
        assert torch.equal(gathered[0], x), "rank 0's own block changed in the gather"
        assert all(not torch.equal(gathered[0], gathered[r]) for r in range(1, world)), \
            "rank blocks are identical: sample_offset did not separate the ranks' Philox streams"
    if args.dump_outputs and rank == 0:      # what the caller of the timed path receives from its last call (the whole node's poses)
        dump_outputs(args.dump_outputs, {"poses": torch.cat(gathered) if dist else x})
    poses = B * world * args.steps
    value = poses / elapsed

    out = {
        "metric": "poses/sec (whole node) at crop_size=256, atom_crop_size=2048",
        "value": value, "unit": "poses/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "per_rank_s": [round(v, 4) for v in per_rank_s],
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32 (fp16x2-split operands x3 MFMA / bf16x3-split x6 MFMA, fp32 accumulate)", "data": "synthetic",
        "arithmetic": "fp32 results; chip-filling contractions run on split operands with fp32 accumulation: where a rigorous "
                      "bound of |A| is known before the launch (the DiT blocks: LayerNorm + AdaLN table, pd_dit_bounds) as two "
                      "fp16 parts of the power-of-two scaled value / three MFMAs per block (22 significand bits), elsewhere as "
                      "three bf16 parts / six MFMAs (error free); both measured at least as accurate as the fp32 MFMA against "
                      "float64; everything else on the fp32 MFMA / fp32 VALU; MMFF94 relaxation in fp64",
        "config": {"workload": f"{args.cfg}: one sample_diffusion call = conditioning trunk + {nsteps} reverse-diffusion steps, "
                               f"{B} samples per call per GPU, "
                               + ("template-projection physics correction (40 synthetic conformers, factor 6)"
                                  if not args.no_physics else "no physics correction"),
                   "model": args.model, "tokens": int(batch["target_feat"].shape[0]), "atoms": int(A),
                   "msa_rows": int(batch["msa_feat"].shape[0]), "samples_per_gpu": B, "diffusion_steps": nsteps,
                   "karras_power": 1000, "weights": "seeded random (no trained weights offline)",
                   "hipgraph": not args.no_graph, "parallelism": f"sample-parallel x{world}"},
    }
    if rank == 0:
        flop_per_call = (DIT_GFLOP_PER_SAMPLE_STEP * B * nsteps + TRUNK_GFLOP) * 1e9 if args.cfg == "cfg1" else None
        if flop_per_call:
            out["path_tflops_per_gpu"] = flop_per_call * args.steps / elapsed / 1e12
            out["path_frac_of_fp32_mfma_peak"] = out["path_tflops_per_gpu"] / PEAK_FP32_MFMA_TFLOPS
            out["path_frac_of_split_bf16_peak"] = out["path_tflops_per_gpu"] / PEAK_SPLIT_TFLOPS

    # ---- roofline of the dominant kernel: instrumented eager pass of the SAME call, HIP events around
    #      every GEMM / attention launch; the kernel symbol with the largest total time is reported
    if rank == 0 and not args.no_roofline:
        from physdock_amd import ops
        kw2 = dict(kw); kw2["use_graph"] = False
        with LaunchTimer(ops) as lt:
            model.sample_diffusion(dbatch, seed=99, sample_offset=0, **kw2)
            summ = lt.summary()
        dom = summ[0]
        traffic, traffic_src = None, None
        for tag in ("r06", "r05", "r04", "r03", "r02"):   # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same call (tools/collect_profiles.sh)
            pmc = os.path.join(REPO, "profiles", f"{tag}_pmc_summary.json")
            if os.path.exists(pmc) and args.cfg == "cfg1" and B == 64:
                allrows = json.load(open(pmc))
                rows = [r for r in allrows if r["kernel"].replace("void ", "") == dom["kernel"]]
                if not rows:        # same kernel template, later template arguments renamed / added since the PMC passes
                    stem = dom["kernel"].split(",")[0]
                    rows = [r for r in allrows if r["kernel"].replace("void ", "").startswith(stem)]
                if rows:
                    n = sum(r["launches"] for r in rows)
                    traffic = sum((r["fetch_bytes_x2"] + r["write_bytes"]) * r["launches"] for r in rows) / n
                    traffic_src = (f"profiles/{tag}_pmc_summary.json: per-launch (FETCH_SIZE x2 [gfx950 wide-read correction] + "
                                   "WRITE_SIZE) x 1024 B averaged over ALL launches of the symbol (the same average as "
                                   "algorithmic_bytes_per_launch), separate --pmc passes of this same call; FETCH_SIZE counts L2 "
                                   "misses incl. Infinity-Cache hits; per-shape rows: profiles/" + tag + "_pmc_by_shape.txt")
                    break
        peak = pipe_peak(lt.split.get(dom["kernel"]))
        shapes = [d for d in lt.summary(by_shape=True) if d["kernel"] == dom["kernel"]]
        out["roofline"] = {"kernel": dom["kernel"], "bound": "mfma", "achieved": dom["tflops"],
                           "peak": peak, "unit": "TFLOP/s", "frac": dom["tflops"] / peak,
                           "peak_basis": ("dense bf16 / fp16 MFMA peak 2516.6 TF / %d partial products per fp32-accurate block"
                                          % lt.split[dom["kernel"]] if lt.split.get(dom["kernel"])
                                          else "fp32 MFMA peak (v_mfma_f32_32x32x2_f32)"),
                           "frac_of_fp32_mfma_peak": dom["tflops"] / PEAK_FP32_MFMA_TFLOPS,
                           "launches": dom["launches"], "avg_launch_ms": dom["avg_launch_ms"],
                           "flop_per_launch": dom["flop_per_launch"], "traffic": traffic,
                           "algorithmic_bytes_per_launch": dom.get("algorithmic_bytes_per_launch"), "traffic_source": traffic_src,
                           "by_shape": [dict(shape=d["shape"], launches=d["launches"], avg_launch_ms=round(d["avg_launch_ms"], 4),
                                             tflops=round(d["tflops"], 2), frac=round(d["tflops"] / peak, 4),
                                             algorithmic_bytes_per_launch=d["algorithmic_bytes_per_launch"]) for d in shapes],
                           "note": "algorithmic flops = 2*M*N*K per GEMM launch (4*B*H*Nq*Nk*32 per attention launch)"}
        out["kernels"] = [dict({k: (round(v, 4) if isinstance(v, float) else v) for k, v in d.items()},
                               pipe=pipe_name(lt.split.get(d["kernel"]))) for d in summ[:8]]
        out["kernels_by_shape"] = [dict({k: (round(v, 4) if isinstance(v, float) else v) for k, v in d.items()},
                                        pipe=pipe_name(lt.split.get(d["kernel"])),
                                        frac_of_pipe_peak=round(d["tflops"] / pipe_peak(lt.split.get(d["kernel"])), 4))
                                   for d in lt.summary(by_shape=True)[:14]]
    # ---- the regime of BASELINE configs #1 / #5 and of the demo (20 samples per round): same call at B = 1 and B = 20
    if rank == 0 and world == 1 and not args.no_extra and args.cfg == "cfg1":
        extra = {}
        for Bx in (1, 20):
            kwx = dict(kw, num_sample=Bx)
            model.sample_diffusion(dbatch, seed=6, **kwx)                 # unit capture
            model.sample_diffusion(dbatch, seed=7, **kwx)                 # whole-loop capture / warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(3):
                model.sample_diffusion(dbatch, seed=8 + i, **kwx)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / 3
            extra[f"samples_{Bx}"] = {"poses_per_s": Bx / dt, "ms_per_call": 1e3 * dt}
        # BASELINE config #5 (screening_demo.sh: 20 samples per round, 40 kept, ranking, PDB output) for ONE ligand through the
        # whole device-side flow: driver.redock = 2 rounds x (trunk + 40 steps at B=20) + template re-selection + alignment +
        # ranking + PDB text of the 40 kept poses; 10 k ligands are independent systems (parallel.map_systems shards them)
        from physdock_amd import driver
        from physdock_amd.synthetic import pdb_meta
        meta = pdb_meta({k: batch[k].numpy() for k in ("token_id_to_chunk_sizes", "asym_id", "is_ligand", "residue_index")})
        rk = dict(ref_mol_poses=confs.to(device), physics_correction=True, max_samples=40, max_rounds=2, num_samples_per_round=20,
                  steps=nsteps, karras_noise_schedule_power=1000, ranking=True, infer_meta_data=meta)
        # (every round runs its own trunk, as when the loader re-samples the MSA per round - `batch_msa_feat`, redocking.py:83;
        #  `shared_trunk_*`: rounds that see identical features take round 0's conditioning, driver.redock(reuse_conditioning=True))
        rk["reuse_conditioning"] = False
        for _w in range(2):                     # (unit capture, then whole-loop capture of each round's schedule)
            driver.redock(model, dbatch, seed=5, **rk)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(2):
            res = driver.redock(model, dbatch, seed=6 + i, **rk)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 2
        extra["screening_ligand"] = {"ligands_per_s": 1.0 / dt, "ms_per_ligand": 1e3 * dt, "rounds": len(res["rounds"]),
                                     "samples_per_round": 20, "poses_kept": int(res["poses"].shape[0]),
                                     "pdb_blocks": len(res["pdb_blocks"])}
        rks = dict(rk, reuse_conditioning=True)
        for _w in range(2):
            driver.redock(model, dbatch, seed=5, **rks)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(2):
            driver.redock(model, dbatch, seed=6 + i, **rks)
        torch.cuda.synchronize()
        dts = (time.perf_counter() - t0) / 2
        extra["screening_ligand"].update(shared_trunk_ligands_per_s=1.0 / dts, shared_trunk_ms_per_ligand=1e3 * dts)
        # graph cache behaviour of a screening stream (one receptor, ligands of different sizes): a NEW ligand size is a cache
        # miss = one eager pass (it is the call's result) + capture / instantiation of the step-loop graph; every later ligand
        # of that size replays.  Measured on a ragged system of another shape at the demo's 20 samples per round.
        from physdock_amd import synthetic as _syn
        rb = _syn.make_batch(221, 8, 35, 64, 2)
        rconf = _syn.reference_conformers(rb, n_conf=40, seed=1).to(device)
        rdb = {k_: (v_.to(device) if isinstance(v_, torch.Tensor) else v_) for k_, v_ in rb.items()}
        kwr = dict(kw, num_sample=20, ref_mol_poses=rconf) if not args.no_physics else dict(kw, num_sample=20)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        model.sample_diffusion(rdb, seed=70, **kwr)
        torch.cuda.synchronize(); t_miss = time.perf_counter() - t0
        cap_ms = model.last_capture_ms
        t0 = time.perf_counter()
        model.sample_diffusion(rdb, seed=71, **kwr)                         # second call of the schedule: unit replay + whole-loop capture
        torch.cuda.synchronize(); t_second = time.perf_counter() - t0
        t0 = time.perf_counter()
        for i in range(2):
            model.sample_diffusion(rdb, seed=72 + i, **kwr)
        torch.cuda.synchronize(); t_hit = (time.perf_counter() - t0) / 2
        extra["graph_cache"] = {"new_shape_call_ms": 1e3 * t_miss, "second_call_ms": 1e3 * t_second, "cached_shape_call_ms": 1e3 * t_hit, "capture_ms": cap_ms,
                                "unit_graphs_cached": len(model._units), "whole_loop_graphs_cached": sum(1 for g_ in model._graphs.values() if g_["exec"]),
                                "max_cached_graphs": model.max_cached_graphs,
                                "note": "new shape = ragged T 256 / A 1803 system at 20 samples, first call: workspace allocation + the first step unit of "
                                        "each kind eager, every other unit recorded and launched while the GPU works (one hipGraph per step head / "
                                        "tail; heads keyed by shape + schedule + step, tails by what the physics branch depends on); the second call "
                                        "of a schedule also records the whole loop as one graph, without a device synchronisation"}
        # the same ligands two at a time on two HIP streams of this GPU (parallel.StreamPool): their half-empty tail rounds overlap
        from physdock_amd.parallel import StreamPool
        pool = StreamPool(model, n=2)
        for _w in range(2):                     # (each replica: step units, then the whole-loop graphs of both rounds' schedules)
            pool.map(lambda m, sd_: driver.redock(m, dbatch, seed=sd_, **rk), [20 + 2 * _w, 21 + 2 * _w])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pool.map(lambda m, sd_: driver.redock(m, dbatch, seed=sd_, **rk), [30, 31, 32, 33])
        torch.cuda.synchronize()
        dt2 = (time.perf_counter() - t0) / 4
        extra["screening_ligand"].update(two_streams_ligands_per_s=1.0 / dt2, two_streams_ms_per_ligand=1e3 * dt2)
        del pool
        # ---- the same 64-pose call with the RELAXATION branch live (model.py:252-261): a 32-atom synthetic MMFF94 molecule
        #      (every term kind, mmff.synthetic_terms) relaxed on the device (pd_mmff_relax, 5 BFGS iterations, fp64) in each of
        #      the low-noise steps, inside the same hipGraph - what `--enable_physics_correction` runs when a ref_mol is given
        from physdock_amd import mmff
        lig = batch["is_ligand"][batch["atom_id_to_token_id"]].bool()
        terms, _ = mmff.synthetic_terms(int(lig.sum()), 5, coords=batch["x_gt"][lig].double().numpy())
        kwm = dict(kw, ref_mol=terms, mmff_iters=5)
        sig, plan = model._step_plan(nsteps, 0.8, 1.0, 1.5, 1.0, kw.get("mmff_gamma_0_factor", 1.0), kw.get("align_ref_pos", True), 1000)
        n_relax = sum(1 for p_ in plan if p_["mmff"] and not p_["align"])
        for _w in range(2):
            model.sample_diffusion(dbatch, seed=40, **kwm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(2):
            xm = model.sample_diffusion(dbatch, seed=41 + i, **kwm)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 2
        assert torch.isfinite(xm).all()
        extra["samples_64_mmff"] = {"poses_per_s": B / dt, "ms_per_call": 1e3 * dt, "relaxation_steps": n_relax,
                                    "ligand_atoms": int(lig.sum()), "mmff_iters": 5, "backend": "device (pd_mmff_relax, fp64)"}
        # ---- BASELINE config #3 in miniature: a STREAM of different systems (Posebusters: every system has its own token / atom counts, so
        #      every call is the first of its shape), 64 samples per system, one round, ranking, PDB text - through driver.redock, each
        #      system seen ONCE: workspace allocation for the shape, trunk, eager first unit of each kind, the other step units recorded
        #      and launched behind, alignment, ranking, PDB formatting all inside the clock
        shapes3 = [(200, 27), (180, 41), (224, 18), (210, 33), (190, 24), (216, 38)]
        systems3 = [_syn.system(npro, 9, nlig, 128, seed=40 + j, n_conf=8) for j, (npro, nlig) in enumerate(shapes3)]
        for s3 in systems3:
            s3["dbatch"] = {k_: v_.to(device) for k_, v_ in s3["batch"].items()}
        rk3 = dict(max_samples=64, max_rounds=1, num_samples_per_round=64, steps=nsteps, karras_noise_schedule_power=1000, ranking=True,
                   physics_correction=False)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for j, s3 in enumerate(systems3):
            r3 = driver.redock(model, s3["dbatch"], seed=80 + j, infer_meta_data=s3["infer_meta_data"], **rk3)
        torch.cuda.synchronize(); dt3 = time.perf_counter() - t0
        extra["stream_of_new_systems_64"] = {"systems": len(systems3), "poses_per_s": 64 * len(systems3) / dt3, "ms_per_system": 1e3 * dt3 / len(systems3),
                                             "tokens_atoms": [[int(s3["batch"]["target_feat"].shape[0]), int(s3["batch"]["ref_pos"].shape[0])] for s3 in systems3],
                                             "note": "every system a new shape (first call: no cached graph), ranking + PDB text included"}
        # ---- the headline's own worst cases
        # (a) first calls at B = 64: call 1 = workspace allocation + weight packing + trunk + first-call bound check (three eager denoiser
        #     passes) + the step units recorded and launched; call 2 = unit replay (the whole-loop graph is recorded meanwhile);
        #     call 3+ = one graph replay
        extra["first_calls_b64_ms"] = {"call_1": round(warm_ms[0], 1) if warm_ms else None,
                                       "call_2": round(warm_ms[1], 1) if len(warm_ms) > 1 else None,
                                       "steady_state": round(1e3 * elapsed / args.steps, 1)}
        # (b) a NEW physics threshold on a cached shape (redocking.py:318-322 changes mmff_gamma_0_factor every round): the 40 denoiser
        #     heads replay, only the tails whose branch changed run eagerly and are captured
        if not args.no_physics and not args.no_graph:
            kwf = dict(kw, mmff_gamma_0_factor=6.9)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            model.sample_diffusion(dbatch, seed=60, **kwf)
            torch.cuda.synchronize(); t_new = time.perf_counter() - t0
            extra["new_threshold_call_b64"] = {"ms": round(1e3 * t_new, 1), "unit_misses": model.last_unit_misses,
                                               "head_misses": model.last_head_misses, "capture_ms": round(model.last_capture_ms or 0.0, 2)}
        # (c) weights whose magnitude bounds turn out too loose for the two-part fp16 format run the DiT on bf16 x 6 (engine.check_dit_bounds
        #     switches a family off): the same 64-sample call with BOTH families forced off the fp16 format
        eng_ = model.engine(device)
        saved_off = set(eng_.f16_off)
        eng_.f16_off = {"atom", "token"}
        model._drop_graphs()
        try:
            for i in range(2):
                model.sample_diffusion(dbatch, seed=61 + i, **kw)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(2):
                xf = model.sample_diffusion(dbatch, seed=63 + i, **kw)
            torch.cuda.synchronize(); dtf = (time.perf_counter() - t0) / 2
            assert torch.isfinite(xf).all()
            extra["bf16x6_fallback"] = {"poses_per_s": B / dtf, "ms_per_call": 1e3 * dtf,
                                        "note": "DiT atom + token families off the fp16 x 3 format (bf16 x 6, no bounds needed); trunk unchanged"}
        finally:
            eng_.f16_off = saved_off
            model._drop_graphs()
        # ---- BASELINE config #4: synthetic crop at crop_size=512 / atom_crop_size=4096 (tiling stress), same model and call
        model.release_workspace()
        batch2, dbatch2, confs2 = make_crop("cfg2", device)
        kw2c = dict(kw, ref_mol_poses=confs2.to(device)) if not args.no_physics else dict(kw)
        for _w in range(2):
            model.sample_diffusion(dbatch2, seed=50, **kw2c)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(2):
            x2 = model.sample_diffusion(dbatch2, seed=51 + i, **kw2c)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 2
        assert torch.isfinite(x2).all()
        from physdock_amd import ops
        with LaunchTimer(ops) as lt2:
            model.sample_diffusion(dbatch2, seed=59, **dict(kw2c, use_graph=False))
            s2 = lt2.summary()
        d2 = s2[0]
        pk2 = pipe_peak(lt2.split.get(d2["kernel"]))
        extra["cfg2"] = {"workload": "cfg2: T=512 / A=4096 / S=128, %d samples, %d steps, template-projection physics" % (B, nsteps),
                         "poses_per_s": B / dt, "ms_per_call": 1e3 * dt, "workspace_gb": model.engine(device).ws.nbytes() / 2 ** 30,
                         "dominant_kernel": {"kernel": d2["kernel"], "launches": d2["launches"], "avg_launch_ms": d2["avg_launch_ms"],
                                             "tflops": d2["tflops"], "peak": pk2, "frac": d2["tflops"] / pk2},
                         "by_shape": [dict(kernel=d["kernel"], shape=d["shape"], launches=d["launches"],
                                           avg_launch_ms=round(d["avg_launch_ms"], 4), tflops=round(d["tflops"], 2))
                                      for d in lt2.summary(by_shape=True)[:6]]}
        model.release_workspace()
        out["extra"] = extra
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(cfg, P, batch, confs, args)
        best = max(v["poses_per_s"] for v in out["cpu_baseline"]["by_samples"].values())
        out["gpu_over_cpu"] = value / best        # against the CPU's BEST figure (B = 20), not the B = 1 value
        out["gpu_over_cpu_basis"] = "GPU value (B = %d) / max over the CPU rows (B = 1 and B = 20; measured or extrapolated as " \
                                    "by_samples labels them, --cpu-baseline %s)" % (B, args.cpu_baseline)
    if rank == 0:
        print(json.dumps(out))
    if dist:
        td.barrier()                  # rank 0 finishes its instrumented pass before anyone tears the group down
        td.destroy_process_group()


if __name__ == "__main__":
    main()
