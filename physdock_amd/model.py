"""`PhysDock` - drop-in for the reference model class on the sampling hot path.

Mirrors ``PhysDock.models.model.PhysDock`` (reference models/model.py:55-68): same
constructor (a config from ``PhysDockConfig``), same parameter names (strict
``load_state_dict`` of a reference checkpoint works, see params.py), same
``sample_diffusion(...)`` / ``forward(batch)`` signatures and return values.  Everything
between "feature tensors on the device" and "coordinates on the device" runs in the HIP
kernels of libphysdock_hip.so; there is no PyTorch compute fallback - on a machine
without the built library or without a GPU the calls raise.

Extensions (keyword-only, not in the reference): ``noise=`` injects pre-drawn random
numbers (parity mode; same draw order as the reference, see oracle), ``seed=`` /
``sample_offset=`` select the on-device Philox streams (perf / multi-GPU mode),
``use_graph=`` replays the step loop from a hipGraph, ``relax_fn=`` / ``mmff_backend=`` choose how the ``ref_mol``
relaxation branch runs (physics.py), ``conditioning=`` / ``return_conditioning=`` share one trunk run between calls.
"""
from __future__ import annotations

import math
import os
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import ops, sampling
from .engine import Engine
from .packing import PackedWeights
from .params import param_shapes


#: PD_CHECK_FINITE=1: EVERY sample_diffusion call checks its poses for inf / NaN (one tiny reduction + a host sync) and raises;
#: without it the check still runs on the first call of every (shape, schedule, weights version) and on every eager call
_CHECK_FINITE = os.environ.get("PD_CHECK_FINITE") == "1"
#: PD_BOUND_CHECK=0 switches the first-call check of the fp16-format operand bounds off (engine.check_dit_bounds)
_BOUND_CHECK = os.environ.get("PD_BOUND_CHECK", "1") != "0"
#: missing step units whose kind has already run on the shape are recorded first and launched like cached ones (sample_diffusion, "the
#: loop as UNITS"); 0: every missing unit runs eagerly and is recorded behind the loop (round 6's first form; A/B knob)
PIPELINED_CAPTURE = os.environ.get("PD_PIPELINED_CAPTURE", "1") != "0"


def _register(root: nn.Module, name: str, tensor: torch.Tensor):
    parts = name.split(".")
    mod = root
    for p in parts[:-1]:
        if p not in mod._modules:
            mod.add_module(p, nn.Module())
        mod = mod._modules[p]
    mod.register_parameter(parts[-1], nn.Parameter(tensor, requires_grad=False))


def karras_noise_schedule(num_steps=200, sigma_data=16, s_max=160, s_min=4 * 10e-4, p=7):
    """reference models/model.py:117-129; same fp32 torch op order (host side, p=1000 amplifies rounding)"""
    idx = torch.arange(num_steps, dtype=torch.float32)
    t = sigma_data * (s_max ** (1 / p) + idx / (num_steps - 1) * (s_min ** (1 / p) - s_max ** (1 / p))) ** p
    return torch.cat([t, torch.zeros_like(t[:1])])


class PhysDock(nn.Module):
    supports_conditioning_reuse = True      # sample_diffusion(conditioning=, return_conditioning=): driver.redock shares the trunk between rounds

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.num_augmentation_sample = config.model.num_augmentation_sample
        self.sigma_data = config.sigma_data
        for name, shape in param_shapes(config).items():
            # weights are expected to come from load_state_dict; start from zeros like an un-initialised buffer
            _register(self, name, torch.zeros(shape))
        self._packed: Optional[PackedWeights] = None
        self._engine: Optional[Engine] = None
        self._packed_versions = None
        self._graphs = {}                 # whole step-loop hipGraphs per (shape, schedule, physics plan), LRU-ordered (dict insertion order)
        self._units = {}                  # per-step head / tail hipGraphs (sample_diffusion: "the loop as UNITS"), LRU-ordered
        self.max_cached_graphs = 64       # a screening stream over one receptor needs one graph per ligand SIZE (18 - 44 atoms in the demo)
        self.max_cached_units = 64 * 96   # 40 heads + 40 tails (+ gathers) per shape
        self.unit_captures = self.whole_captures = 0     # counters (tests, bench.py): unit graphs / whole-loop graphs captured so far
        self.last_unit_misses = self.last_head_misses = 0
        self._warm_kinds = set()          # (shape key, unit kind) pairs whose workspace buffers exist: their units may be recorded before they run
        self._capture_stream = None
        self.last_capture_ms = None       # host time of the most recent graph capture + instantiation (bench.py reports it)
        #: workspace buffers are cached per shape (288 GB of HBM make re-allocation pointless for a stream of
        #: same-size crops); when systems of many different sizes pass through, the cache is dropped beyond this size
        self.workspace_limit_bytes = 160 * 2 ** 30
        self.register_load_state_dict_post_hook(lambda m, k: m._invalidate())

    # ------------------------------------------------------------------ plumbing
    def _invalidate(self):
        self._packed = None
        self._engine = None
        self._stream_pool = None          # parallel.StreamPool.for_model: replicas hold copies of the old weights
        self._drop_graphs()

    def _drop_graphs(self):
        for g in self._graphs.values():
            for ex in g["exec"] or ():
                ops._lib.lib().pd_graph_destroy(ex)
        for u in self._units.values():
            ops._lib.lib().pd_graph_destroy(u["exec"])
        self._graphs = {}
        self._units = {}
        self._warm_kinds = set()

    def release_workspace(self):
        """free every cached activation buffer and captured step-loop graph (they are rebuilt on the next call)"""
        self._drop_graphs()
        if self._engine is not None:
            torch.cuda.synchronize(self._engine.device)
            self._engine.ws.bufs.clear()

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._invalidate()
        return r

    def _param_versions(self):
        """sum of the parameters' in-place modification counters: the packed weights, their fp16 / bf16 splits and every static
        magnitude bound derive from the values at pack time, so an in-place update (optimizer step, `p.data.mul_`, ...) must
        rebuild them - a stale bound would let the fp16 operand format overflow silently.  (Writes through `p.data` bypass the
        counters by PyTorch's design: call `_invalidate()` after those, or run with PD_CHECK_FINITE=1.)"""
        return sum(p._version for p in self.parameters()) + sum(b._version for b in self.buffers())

    def engine(self, device) -> Engine:
        if self._engine is not None and self._packed_versions != self._param_versions():
            self._invalidate()               # a weight was modified in place since the engine was built
        if self._engine is None or self._engine.device != device:
            if device.type != "cuda":
                raise RuntimeError("physdock_amd.PhysDock runs its sampler on an MI355X (HIP) device only; "
                                   "there is no CPU path (the CPU oracle lives in oracle/ and is test-only)")
            params = {k: v for k, v in self.state_dict().items()}
            if any(v.device != device for v in params.values()):
                raise RuntimeError("model parameters and batch must be on the same device")
            self._packed = PackedWeights(params, self.config)
            self._engine = Engine(self._packed, self.config, device)
            self._packed_versions = self._param_versions()
        return self._engine

    @staticmethod
    def _pad_masked(b, pa, pt):
        """append `pa` MASKED atoms and `pt` MASKED tokens to the feature dict b (in place; `_prepare_batch` and `_pad_to_group`):
        padded atoms belong to no token segment and point at token 0, padded tokens own no atoms, every mask is 0 on them"""
        import torch.nn.functional as F
        dev = b["ref_pos"].device

        def pad(k, dims, value=0):
            v = b[k]
            spec = []
            for d in range(v.dim() - 1, -1, -1):
                spec += [0, dims.get(d, 0)]
            b[k] = F.pad(v, spec, value=value)
        for k in ("ref_feat", "ref_pos", "a_mask", "x_gt"):
            pad(k, {0: pa})
        if "x_exists" in b:
            pad("x_exists", {0: pa})
        pad("ap_mask", {0: pa, 1: pa})
        b["ref_space_uid"] = torch.cat([b["ref_space_uid"], b["ref_space_uid"].max() + 1 +
                                        torch.arange(pa, device=dev, dtype=b["ref_space_uid"].dtype)])
        b["atom_id_to_token_id"] = torch.cat([b["atom_id_to_token_id"],
                                              torch.zeros(pa, device=dev, dtype=b["atom_id_to_token_id"].dtype)])
        b["token_id_to_chunk_sizes"] = torch.cat([b["token_id_to_chunk_sizes"],
                                                  torch.zeros(pt, device=dev, dtype=b["token_id_to_chunk_sizes"].dtype)])
        for k in ("target_feat", "key_res_feat", "pocket_res_feat", "is_ligand"):
            pad(k, {0: pt})
        for k in ("token_bonds_feature", "rel_tok_feat", "templ_feat", "z_mask"):
            pad(k, {0: pt, 1: pt})
        pad("msa_feat", {1: pt})
        for k in ("asym_id", "sym_id", "entity_id"):
            b[k] = torch.cat([b[k], (b[k].max() + 1).expand(pt).to(b[k].dtype)])
        b["residue_index"] = torch.cat([b["residue_index"], torch.zeros(pt, device=dev, dtype=b["residue_index"].dtype)])

    @staticmethod
    def _prepare_batch(batch):
        """Boundary bookkeeping (layout only): int32 token start offsets for the pooling kernels, fp32
        contiguity, and - for un-padded real systems whose token / atom counts are not multiples of 4
        (reference feature_loader.py:982-983) - padding with MASKED tokens / atoms.  The reference's own
        masks (a_mask / ap_mask / z_mask, tensor_utils.py:642-646) make padded entries inert: masked keys
        get weight exp(-1e9) = 0, triangle operands are multiplied by the mask, pooling is per token."""
        if "_tok_start" in batch:
            return batch
        b = dict(batch)
        A, T = b["ref_pos"].shape[0], b["target_feat"].shape[0]
        b["_A_real"], b["_T_real"] = A, T
        # atoms: to a multiple of 64 for systems of DiT size - sample-major [B * A, C] activations then consist of whole 64-row tiles for
        # every sample count, which is what the fp16-format rows / tile kernels and the fused transition take (a ragged 1 803-atom system
        # at 20 samples ran 65 % slower than the LARGER 2 048-atom crop through row-remainder launches); <= 3 % more (masked) rows
        pa = (-A) % (64 if A >= 512 else 4)
        pt = (-T) % 4
        # (padded atoms belong to no token segment - token_id_to_chunk_sizes, hence _tok_start, covers the real atoms only, so the pooling
        #  kernels never see them - and point at token 0 where an index is needed; adding a padded TOKEN for them, as this did, turned a
        #  256-token system into 260 tokens: sample-major token rows with a remainder in every projection)
        if pa or pt:
            PhysDock._pad_masked(b, pa, pt)
        chunk = b["token_id_to_chunk_sizes"]
        ts = torch.zeros(chunk.shape[0] + 1, dtype=torch.int32, device=chunk.device)
        ts[1:] = torch.cumsum(chunk, 0).to(torch.int32)
        b["_tok_start"] = ts
        # tokens per block of the fused downscale + pool kernel (csrc/pool.hip): as many consecutive tokens as are sure to hold <= 64 atoms
        mc = int(chunk.max()) if chunk.numel() else 0
        b["_pool_tpb"] = min(32, 64 // mc) if 0 < mc <= 64 else 0
        for k in ("ref_feat", "ref_pos", "a_mask", "ap_mask", "target_feat", "key_res_feat", "pocket_res_feat",
                  "token_bonds_feature", "rel_tok_feat", "msa_feat", "templ_feat", "z_mask", "x_gt", "is_ligand", "t_mask"):
            v = b[k]
            if v.dtype != torch.float32 or not v.is_contiguous():
                b[k] = v.float().contiguous()
        for k, dt in (("ref_space_uid", torch.int64), ("atom_id_to_token_id", torch.int64), ("residue_index", torch.int64),
                      ("asym_id", torch.int32), ("sym_id", torch.int32), ("entity_id", torch.int32)):
            if b[k].dtype != dt or not b[k].is_contiguous():
                b[k] = b[k].to(dt).contiguous()
        return b

    # ------------------------------------------------------------------ reference API
    def karras_noise_schedule(self, num_steps=200, sigma_data=16, s_max=160, s_min=4 * 10e-4, p=7):
        return karras_noise_schedule(num_steps, sigma_data, s_max, s_min, p)

    def _step_plan(self, steps, gamma_0, gamma_min, step_scale_eta, ode_step_scale_eta, mmff_gamma_0_factor,
                   align_ref_pos, p, relaxes=True):
        """Host-side resolution of every per-step scalar and branch of reference model.py:211-281
        (all t-dependent branches depend only on the schedule, so none needs a device sync).
        relaxes: is there a molecule to relax (the elif of model.py:252 is only reachable with one)"""
        sig = karras_noise_schedule(steps, p=p)
        sd = float(self.sigma_data)
        plan = []
        for i in range(steps):
            t_cur, t_next = sig[i], sig[i + 1]
            noisy = bool(t_cur > gamma_min)
            t_hat = t_cur * (gamma_0 + 1) if noisy else t_cur
            sdev = torch.sqrt(t_hat ** 2 - t_cur ** 2) if noisy else torch.zeros(())
            c_in = 1 / torch.sqrt(t_hat ** 2 + sd ** 2)
            c_noise = torch.log(t_hat / sd) / 4.0
            align = bool(align_ref_pos and t_cur > gamma_min * mmff_gamma_0_factor)
            plan.append(dict(
                t_hat=float(t_hat), sdev=float(sdev), noisy=noisy, c_in=float(c_in), tau=float(t_hat * c_noise),
                c_skip=float(sd ** 2 / (sd ** 2 + t_hat ** 2)), c_out=float(sd * t_hat / torch.sqrt(sd ** 2 + t_hat ** 2)),
                dt=float(t_next - t_hat), eta=float(step_scale_eta if noisy else ode_step_scale_eta), align=align,
                mmff=bool(relaxes and not align and t_cur <= gamma_min * mmff_gamma_0_factor)))
        return sig, plan

    def _check_bounds_once(self, eng, sched, check):
        """First call of this engine (= these weights) on this schedule: check the fp16-format operand bounds against what the
        denoiser's launches really see (`check()` runs engine.check_dit_bounds) - a violated bound raises, on this and on EVERY later
        call of this engine + schedule; a uselessly loose one moves the family to bf16 x 6: returns True, and the caller prepares
        the denoiser again.  Once per (weights, schedule); replays and later systems pay nothing."""
        ck = sched[:5]
        if not (_BOUND_CHECK and ops.F16_GEMM and ops.SPLIT_GEMM) or ck in eng._bounds_checked:
            return False
        if ck in eng._bounds_failed:
            raise eng._bounds_failed[ck]
        try:
            switched = check()
        except FloatingPointError as e:
            eng._bounds_failed[ck] = e
            raise
        eng._bounds_checked.add(ck)          # only a check that RETURNED counts
        if switched:
            self._drop_graphs()
        return bool(switched)

    def _check_finite(self, outs, fresh, use_graph, who):
        """Finite check: ALWAYS on the first call of a (shape, schedule, weights version) - the eager pass that precedes a graph
        capture, and every eager call - and on every call with PD_CHECK_FINITE=1 (one tiny reduction + a host sync; replays stay
        sync-free).  A violated magnitude bound (weights changed behind the engine's back through `.data`, a caller-supplied bound
        that does not hold) overflows the fp16 operand format to inf / NaN: that must be an exception, not a pose."""
        if (_CHECK_FINITE or fresh) and not all(bool(torch.isfinite(o).all()) for o in outs):
            if use_graph:
                self._drop_graphs()          # the loop captured from this pass would replay the same overflow
            raise FloatingPointError(f"{who} produced non-finite coordinates: an fp16-format operand bound was violated "
                                     "(rebuild the engine after changing weights; ops.F16_GEMM / F16_ATTN = False to confirm)")

    @torch.no_grad()
    def sample_diffusion(
            self,
            batch: Dict[str, torch.Tensor],
            num_sample: int = 5,
            steps: int = 200,
            gamma_0: float = 0.8,
            gamma_min: float = 1.0,
            noise_scale_lambda: float = 1.003,
            step_scale_eta: float = 1.5,
            ode_step_scale_eta=1.0,
            ref_mol=None,
            ref_mol_poses=None,
            use_ref_mol_poses=False,
            mmff_gamma_0_factor=1.0,
            mmff_iters=5,
            align_ref_pos=True,
            karras_noise_schedule_power=7,
            *,
            noise=None,
            seed: int = 0,
            sample_offset: int = 0,
            use_graph: bool = True,
            conditioning=None,
            return_conditioning: bool = False,
            relax_fn=None,
            mmff_backend: str = "auto",
    ) -> torch.Tensor:
        """reference models/model.py:157-282.  Returns x_next [num_sample, A, 3] on the batch device.

        `ref_mol` switches on the relaxation branch (model.py:252-261) exactly as in the reference; how the relaxed
        ligand is produced is described in physics.py (device MMFF94 kernel, host RDKit, or an injected `relax_fn` with
        the signature of the reference's `get_next_step_pos`).  The step loop itself is sampling.py."""
        from . import physics
        device = batch["x_gt"].device
        eng = self.engine(device)
        if eng.ws.nbytes() > self.workspace_limit_bytes:
            self.release_workspace()
        batch = self._prepare_batch(batch)
        L = ops._lib.init()
        ws = eng.ws
        B = num_sample
        A = batch["ref_pos"].shape[0]            # padded atom count
        A_real = batch["_A_real"]
        if B <= 0:
            return torch.empty(0, A_real, 3, device=device)

        relaxer = physics.resolve_relaxer(ref_mol, relax_fn, mmff_backend)
        if ref_mol_poses is None and use_ref_mol_poses:      # model.py:188-203: ETKDG conformers of the reference molecule
            if not (ref_mol is not None and physics.have_rdkit() and physics._is_rdkit_mol(ref_mol)):
                raise RuntimeError("use_ref_mol_poses=True without ref_mol_poses needs an RDKit ref_mol (and RDKit) to embed "
                                   "conformers (reference model.py:188-203); pass ref_mol_poses [C,L,3]")
            n_lig_real = int((batch["is_ligand"][batch["atom_id_to_token_id"]][:A_real] > 0).sum())
            ref_mol_poses = physics.rdkit_ref_mol_poses(ref_mol, 512)[:, :n_lig_real]

        sig, plan = self._step_plan(steps, gamma_0, gamma_min, step_scale_eta, ode_step_scale_eta, mmff_gamma_0_factor,
                                    align_ref_pos, karras_noise_schedule_power, relaxes=relaxer.kind != "none")
        sched = sampling.sched_id(steps, sig, gamma_0, gamma_min, karras_noise_schedule_power)

        # ---- per-call setup: conditioning trunk, hoisted biases, AdaLN tables
        a, ap, s, z = conditioning if conditioning is not None else eng.conditioning(batch)
        tau = ws.get("tau", steps)
        tau.copy_(torch.tensor([p["tau"] for p in plan], dtype=torch.float32))
        prep = eng.prepare_dit(a, ap, s, z, batch, tau, B=B)
        if self._check_bounds_once(eng, sched, lambda: eng.check_dit_bounds(batch, a, s, prep, plan, B, float(self.sigma_data))):
            prep = eng.prepare_dit(a, ap, s, z, batch, tau, B=B)

        # the denoiser's inputs are staged like the loop's own (sampling.py; a / s included: a graph captured with the trunk's own
        # outputs must stay valid when a later call passes conditioning=, and vice versa)
        def staged(name, t):
            buf = ws.get("loop:" + name, *t.shape, dtype=t.dtype)
            buf.copy_(t)
            return buf
        cond_out = (a, ap, s, z)
        a, s = staged("a", a), staged("s", s)
        batch = dict(batch)
        for k in ("a_mask", "atom_id_to_token_id", "_tok_start", "ref_pos"):
            batch[k] = staged(k, batch[k])
        loop = sampling.StepLoop(eng, "loop:", [plan], B, A, sig[0], noise_scale_lambda, mmff_iters, noise is not None)
        slot = loop.add_slot("loop:", "the crop", batch, batch["a_mask"], batch["ref_pos"], plan, relaxer, ref_mol_poses,
                             noise, seed, sample_offset)

        def denoise(i):
            eng.af3_dit(batch, loop.x_hat, loop.x_den, a, s, prep, B, plan[i], row=i)
        common = (B, A, batch["target_feat"].shape[0], A_real, batch["_T_real"], sched, noise is not None,
                  float(noise_scale_lambda), sample_offset)
        units = loop.units(common, denoise)

        # A whole schedule seen twice is additionally captured as ONE graph (one per segment around a host relaxation)
        entry = None
        if use_graph:
            key = (common, tuple(u[0] for u in units))
            entry = self._graphs.get(key)
            if entry is not None:
                self._graphs[key] = self._graphs.pop(key)          # LRU order
        if entry is not None and entry["exec"] is not None:
            fresh = False
            breaks = [after for _, _, after, _ in units if after is not None]
            for k, g in enumerate(entry["exec"]):
                ops.check(L.pd_graph_launch(g, ops.stream()), "graph_launch")
                if k < len(breaks):
                    breaks[k]()
        else:
            fresh = sampling.run_units(self, units, use_graph, PIPELINED_CAPTURE)
        if use_graph and not (entry and entry["exec"]):
            terms = relaxer.terms if relaxer.kind == "device" else None    # (a graph keeps the tables it captured alive, as a unit)
            if entry is None:
                self._graphs[key] = {"exec": None, "terms": terms}
            else:
                # the second call of the same schedule on the same shape: the whole N-step loop as ONE graph from here on
                # (recorded without a device synchronisation while the GPU executes the units launched above: a synchronising capture
                #  stalled every stream of the device - the other replica of a StreamPool too: two systems at a time fell from 3.1 to 2.7
                #  ligands/s when the promotion landed in the measured region)
                segments = [[]]
                for _, fn, after, _ in units:
                    segments[-1].append(fn)
                    if after is not None:
                        segments.append([])
                entry["exec"] = sampling.record(self, segments, sync=not PIPELINED_CAPTURE)
                entry["terms"] = terms                                     # the tables THIS capture recorded
                self.whole_captures += 1
            while len(self._graphs) > self.max_cached_graphs:
                old = self._graphs.pop(next(iter(self._graphs)))
                for ex in old["exec"] or ():
                    L.pd_graph_destroy(ex)
        out = slot.x_a[:, :A_real].clone()
        self._check_finite([out], fresh, use_graph, "sample_diffusion")
        if return_conditioning:
            return out, tuple(t.clone() for t in cond_out)
        return out

    @staticmethod
    def _pad_to_group(batches):
        """Group padding for sample_diffusion_many: every (already `_prepare_batch`ed) system padded to the group's largest padded
        atom and token counts with MASKED atoms / tokens, as `_prepare_batch` pads (padded atoms belong to no token segment and
        point at token 0; padded tokens own no atoms).  The real counts are kept; a system that has the group shape is returned
        as it is."""
        A = max(b["ref_pos"].shape[0] for b in batches)
        T = max(b["target_feat"].shape[0] for b in batches)
        out = []
        for b in batches:
            pa, pt = A - b["ref_pos"].shape[0], T - b["target_feat"].shape[0]
            if not (pa or pt):
                out.append(b)
                continue
            b = dict(b)
            PhysDock._pad_masked(b, pa, pt)
            b["_tok_start"] = torch.cat([b["_tok_start"], b["_tok_start"][-1:].expand(pt)]).contiguous()
            out.append(b)
        return out

    @torch.no_grad()
    def sample_diffusion_many(self, batches, num_sample=5, steps=200, gamma_0=0.8, gamma_min=1.0, noise_scale_lambda=1.003,
                              step_scale_eta=1.5, align_ref_pos=True, karras_noise_schedule_power=7, *,
                              ode_step_scale_eta=1.0, mmff_gamma_0_factor=1.0, ref_mol_poses=None, ref_mol=None,
                              mmff_iters=5, seeds=None, sample_offsets=None, noises=None, conditionings=None,
                              return_conditioning=False, use_graph=True, mmff_backend="auto", relax_fn=None):
        """`sample_diffusion` for several systems in ONE step loop: G systems x num_sample samples run every denoiser launch
        together as G num_sample rows (the row-wise launches), through grouped launches (attention: one bias set and real key count
        per system; pooling, unpooling and the preconditioning: per-system tables), so that rounds of few samples fill the chip.
        Returns a list of [num_sample, A_real_g, 3] in input order (with return_conditioning: (that list, list of (a, ap, s, z))).

        Shared across the group: the schedule and its scalars, num_sample, align_ref_pos, noise_scale_lambda.  Per system (a scalar
        or a list): ode_step_scale_eta, mmff_gamma_0_factor; lists with None entries: ref_mol_poses, ref_mol, noises (dicts as
        sample_diffusion's noise=; all or none), conditionings (each (a, ap, s, z) at the GROUP's padded shape - as
        return_conditioning=True returns them - not at the shape sample_diffusion gives a smaller system alone); seeds /
        sample_offsets (ints).  Each system draws exactly the
        random numbers of its own sample_diffusion call and gets its own physics tail.  Systems are padded (masked atoms / tokens)
        to the group's largest padded shape.  Host-side relaxation (an RDKit molecule on the host backend, relax_fn=) would break
        the loop once per system and step: ValueError; the device MMFF relaxation (mmff.MMFFTerms) is supported."""
        from . import physics
        batches = list(batches)
        G = len(batches)
        if G == 0:
            return ([], []) if return_conditioning else []

        def per(v, name, lists_only=False):
            if isinstance(v, (list, tuple)):
                if len(v) != G:
                    raise ValueError(f"sample_diffusion_many: {name} has {len(v)} entries for {G} systems")
                return list(v)
            if lists_only and v is not None:
                raise ValueError(f"sample_diffusion_many: {name} must be a list with one entry per system (None entries allowed)")
            return [v] * G
        etas = [float(v) for v in per(ode_step_scale_eta, "ode_step_scale_eta")]
        facs = [float(v) for v in per(mmff_gamma_0_factor, "mmff_gamma_0_factor")]
        poses_in = per(ref_mol_poses, "ref_mol_poses", True)
        mols = per(ref_mol, "ref_mol", True)
        seeds_ = [int(v) for v in per(0 if seeds is None else seeds, "seeds")]
        offs = [int(v) for v in per(0 if sample_offsets is None else sample_offsets, "sample_offsets")]
        noises_ = per(noises, "noises", True)
        conds_in = per(conditionings, "conditionings", True)
        if any(n is None for n in noises_) and any(n is not None for n in noises_):
            raise ValueError("sample_diffusion_many: noises must be given for every system or for none")
        if relax_fn is not None:
            raise ValueError("sample_diffusion_many: relax_fn= relaxes on the host - one host break per system and step would "
                             "serialise the group; use sample_diffusion for it (or an mmff.MMFFTerms ref_mol: device relaxation)")
        relaxers = [physics.resolve_relaxer(m, None, mmff_backend) for m in mols]
        for r in relaxers:
            if r.kind == "host":
                raise ValueError("sample_diffusion_many: this ref_mol relaxes on the host (RDKit backend) - one host break per "
                                 "system and step would serialise the group; pass an mmff.MMFFTerms table (device relaxation) or "
                                 "use sample_diffusion")
        device = batches[0]["x_gt"].device
        eng = self.engine(device)
        if eng.ws.nbytes() > self.workspace_limit_bytes:
            self.release_workspace()
        bats = self._pad_to_group([self._prepare_batch(b) for b in batches])
        ws = eng.ws
        B = num_sample
        A, T = bats[0]["ref_pos"].shape[0], bats[0]["target_feat"].shape[0]
        Ars = [int(b["_A_real"]) for b in bats]
        Trs = [int(b["_T_real"]) for b in bats]
        if B <= 0:
            outs = [torch.empty(0, ar, 3, device=device) for ar in Ars]
            return (outs, [None] * G) if return_conditioning else outs
        noise_mode = noises_[0] is not None
        plans = []
        for g in range(G):
            sig, plan = self._step_plan(steps, gamma_0, gamma_min, step_scale_eta, etas[g], facs[g], align_ref_pos,
                                        karras_noise_schedule_power, relaxes=relaxers[g].kind != "none")
            plans.append(plan)
        sched = sampling.sched_id(steps, sig, gamma_0, gamma_min, karras_noise_schedule_power)

        # ---- conditioning per system (the trunk's outputs are shape-keyed workspace buffers: each is consumed before the next runs)
        tau = ws.get("tau", steps)
        tau.copy_(torch.tensor([p["tau"] for p in plans[0]], dtype=torch.float32))
        memo = {}
        cond_out = [None] * G

        for g, c in enumerate(conds_in):
            if c is not None and tuple(int(t.shape[0]) for t in c) != (A, A * A, T, T * T):
                raise ValueError(f"sample_diffusion_many: conditionings[{g}] has (a, ap, s, z) for another shape than the group's padded "
                                 f"{A} atoms / {T} tokens (a conditioning is only reusable by a group that pads the system the same "
                                 f"way: take it from sample_diffusion_many(return_conditioning=True) on the same group)")

        def cond_of(g):
            if g not in memo:
                c = conds_in[g] if conds_in[g] is not None else eng.conditioning(bats[g])
                memo.clear()
                memo[g] = c
                if return_conditioning:
                    cond_out[g] = tuple(t.clone() for t in c)
            return memo[g]

        def check_first():                        # the once-per-(weights, schedule) check of sample_diffusion, on the first system
            a0, ap0, s0, z0 = cond_of(0)
            prep0 = eng.prepare_dit(a0, ap0, s0, z0, bats[0], tau, B=B)
            return eng.check_dit_bounds(bats[0], a0, s0, prep0, plans[0], B, float(self.sigma_data))
        self._check_bounds_once(eng, sched, check_first)
        prep = eng.prepare_dit_many(cond_of, bats, tau, B)
        memo.clear()
        a_g, s_g = prep["a"], prep["s"]

        # ---- the group descriptor and the denoiser's per-system inputs, staged like the loop's own (sampling.py)
        def stacked(name, ts, dtype=None):
            buf = ws.get("grp:" + name, G, *ts[0].shape, dtype=dtype or ts[0].dtype)
            for g, t in enumerate(ts):
                buf[g].copy_(t)
            return buf
        tok_start = stacked("tok_start", [b["_tok_start"] for b in bats])
        a2t = stacked("a2t", [b["atom_id_to_token_id"] for b in bats])
        a_mask = stacked("a_mask", [b["a_mask"] for b in bats])
        ref_pos = stacked("ref_pos", [b["ref_pos"] for b in bats])
        nk_a = stacked("nk_atom", [torch.tensor(v, dtype=torch.int32) for v in Ars])
        nk_t = stacked("nk_token", [torch.tensor(v, dtype=torch.int32) for v in Trs])
        tpbs = [int(b["_pool_tpb"]) for b in bats]
        gbatch = {"_A_real": max(Ars), "_T_real": max(Trs), "_pool_tpb": 0 if min(tpbs) <= 0 else min(tpbs),
                  "_tok_start": tok_start, "atom_id_to_token_id": a2t}
        grp = {"G": G, "B": B, "nk_atom": nk_a, "nk_token": nk_t}
        loop = sampling.StepLoop(eng, "grp:", plans, B, A, sig[0], noise_scale_lambda, mmff_iters, noise_mode)
        for g in range(G):
            loop.add_slot(f"grp{g}:", f"system {g}'s crop", bats[g], a_mask[g], ref_pos[g], plans[g], relaxers[g], poses_in[g],
                          noises_[g], seeds_[g], offs[g])

        def denoise(i):
            eng.af3_dit(gbatch, loop.x_hat, loop.x_den, a_g, s_g, prep, G * B, plans[0][i], row=i, grp=grp)
        # one head per step for the whole group, one tail per step and slot; recorded behind the loop (not pipelined)
        common = ("many", G, B, A, T, tuple(Ars), tuple(Trs), gbatch["_pool_tpb"], sched, noise_mode, float(noise_scale_lambda),
                  tuple(offs))
        fresh = sampling.run_units(self, loop.units(common, denoise), use_graph, False)
        outs = [s.x_a[:, :Ars[s.g]].clone() for s in loop.slots]
        self._check_finite(outs, fresh, use_graph, "sample_diffusion_many")
        if return_conditioning:
            return outs, cond_out
        return outs

    @torch.no_grad()
    def forward(self, batch, return_loss=False):
        """reference models/model.py:99-115 (training-time forward; kept for API completeness):
        conditioning -> 48 noised copies (per-sample noise level) -> denoiser -> distogram logits.
        return_loss=True: returns (outputs, cum_loss, losses) with `cum_loss, losses = PhysDockLoss(config)(outputs, batch)`
        (physdock_amd.loss; `batch` then also carries the reference's loss features, in its real - un-padded - sizes)."""
        device = batch["x_gt"].device
        feats = batch
        eng = self.engine(device)
        if eng.ws.nbytes() > self.workspace_limit_bytes:
            self.release_workspace()
        batch = self._prepare_batch(batch)
        L = ops._lib.init()
        ws = eng.ws
        B = self.num_augmentation_sample
        A, T = batch["ref_pos"].shape[0], batch["target_feat"].shape[0]
        A_real, T_real = batch["_A_real"], batch["_T_real"]
        sd = float(self.sigma_data)
        a, ap, s, z = eng.conditioning(batch)
        # augmentation_diffuse (model.py:87-97): per-sample noise levels; RNG on the host generator
        t_hat = (torch.exp(torch.normal(0, 1, (B,)) * 1.5 - 1.2) * sd).to(device)
        x_noisy = ws.get("fw_xn", B, A, 3)
        x_noisy.copy_(batch["x_gt"][None] + torch.normal(0, 1, (B, A, 3)).to(device) * t_hat[:, None, None])
        x_hat = ws.get("fw_xhat", B, A, 3)
        rot = torch.rand(4, B).to(device).contiguous()
        tr = torch.normal(0, 1, (B, 3)).to(device).contiguous()
        ops.check(L.pd_augment(ops.ptr(x_noisy), 1.0, ops.ptr(batch.get("x_exists", batch["a_mask"])), ops.ptr(rot), ops.ptr(tr),
                               None, 1.0, 0.0, None, 0, 0, ops.ptr(x_hat), B, A, ops.stream()), "augment")
        th = t_hat.cpu()
        scal = {"c_in": (1 / torch.sqrt(th ** 2 + sd ** 2)).to(device), "c_skip": (sd ** 2 / (sd ** 2 + th ** 2)).to(device),
                "c_out": (sd * th / torch.sqrt(sd ** 2 + th ** 2)).to(device)}
        tau = (th * (torch.log(th / sd) / 4.0)).to(device)
        prep = eng.prepare_dit(a, ap, s, z, batch, tau, per_sample=True, B=B)
        x_den = ws.get("fw_xden", B, A, 3)
        eng.af3_dit(batch, x_hat, x_den, a, s, prep, B, scal, row=0, per_sample=True)
        pd = eng.lin(z, "linear_distogram", T * T).reshape(T, T, -1)[:T_real, :T_real]
        outputs = {"x_denoised": x_den[:, :A_real].clone(), "x_hat": x_hat[:, :A_real].clone(), "t_hat": t_hat,
                   "p_distogram": pd + pd.transpose(0, 1)}
        if not return_loss:
            return outputs
        from .loss import PhysDockLoss
        cum_loss, losses = PhysDockLoss(self.config)(outputs, feats)
        return outputs, cum_loss, losses

    @torch.no_grad()
    def predict_distogram(self, batch, conditioning=None):
        """The distance head at inference: p_distogram fp32 [T,T,no_bins] at the system's real token count - `linear_distogram` of the
        trunk's pair representation z, symmetrised, exactly as `forward` computes it (reference models/model.py:107-108), so that
        given the same z the logits are bit-equal to `forward(batch)["p_distogram"]`.  `conditioning`: None runs the trunk; else the
        (a, ap, s, z) tuple `sample_diffusion(return_conditioning=True)` returned, or its last two tensors (s, z) - only the head runs
        (z may be at a group's padded token count, as `sample_diffusion_many` returns it)."""
        eng = self.engine(batch["x_gt"].device)
        if conditioning is None and eng.ws.nbytes() > self.workspace_limit_bytes:
            self.release_workspace()
        batch = self._prepare_batch(batch)
        z = eng.conditioning(batch)[3] if conditioning is None else conditioning[-1]
        c_z = z.shape[-1]
        T = batch["target_feat"].shape[0] if conditioning is None else math.isqrt(z.numel() // c_z)
        if z.numel() != T * T * c_z or T < batch["_T_real"]:
            raise ValueError(f"predict_distogram: the conditioning's z has shape {tuple(z.shape)}, the batch holds {batch['_T_real']} tokens")
        pd = eng.lin(z.reshape(T * T, c_z), "linear_distogram", T * T).reshape(T, T, -1)[:batch["_T_real"], :batch["_T_real"]]
        return pd + pd.transpose(0, 1)


def weighted_rigid_align(x_pred, x_gt, weights):
    """reference utils/tensor_utils.py:724-778: returns x_gt moved onto x_pred (second argument moves)."""
    L = ops._lib.init()
    xp = x_pred.float().contiguous()
    B, A = xp.shape[0], xp.shape[1]
    xg = x_gt.float().contiguous()
    out = torch.empty_like(xp)
    ops.check(L.pd_kabsch_align(ops.ptr(xp), None, ops.ptr(xg), 0 if xg.dim() == 2 else A * 3,
                                ops.ptr(weights.float().contiguous()), ops.ptr(out), B, A, ops.stream()), "kabsch")
    return out
