"""The sampler's step loop, once: what `PhysDock.sample_diffusion` (one system) and `PhysDock.sample_diffusion_many` (a group) share.

A loop runs G systems x B samples as G * B rows of the buffers x_a / x_hat / x_den / x_proj.  Each system is a `Slot`: its plan, its
relaxer, its ligand tables, conformer pool and relaxation buffers, its random numbers and views of its B rows.  One step is

    head:  augment every slot (reference models/model.py:212-218), then ONE denoiser call for all rows - the entry point's own
           (`af3_dit(..., grp=None)` after `prepare_dit`, or `af3_dit(..., grp=grp)` after `prepare_dit_many`: other launchers)
    tail:  per slot, the physics correction and the Euler update (model.py:223-281)

The loop as UNITS: one unit = the launches of one step's head (~115 kernels, the expensive part) or of one slot's tail (1 - 4 kernels).
A head depends on the shape, the schedule and the step index only; what the drivers change between calls - the physics threshold
(`mmff_gamma_0_factor` x 1.15 / x 0.7 per round, redocking.py:318-322), the template pool size, the relaxation - lives in the tails.
Every unit is captured as its own hipGraph, keyed by exactly what its launches depend on, so a call with a new threshold or pool
replays all heads and the unchanged tails and runs (then captures) only the few tails that changed (`run_units`).

Everything a unit reads is staged in workspace buffers: a captured hipGraph replays raw addresses, so no caller-owned or per-call
temporary tensor may be referenced from inside the loop.  The buffers of a single-system loop are named "loop:*", those of a group
"grp:*" (rows) and "grp{g}:*" (slot g): a captured single-system graph and a captured group graph never share a buffer.
"""
from __future__ import annotations

import ctypes as C
import threading
import time
from functools import partial

import torch

from . import ops
from .engine import off


_CAPTURE_LOCK = threading.Lock()


class Slot:
    """one system's share of a step loop (attributes: StepLoop.add_slot, the only place that builds one)"""


def sched_id(steps, sig, gamma_0, gamma_min, power):
    """what identifies a schedule in unit keys; its first five fields key the once-per-(weights, schedule) bounds check"""
    return (steps, float(sig[0]), float(sig[-2]), float(gamma_0), float(gamma_min), float(power))


def tail_kind(p, slot, mmff_iters):
    """which branch the tail of plan entry p takes for this slot, with everything the branch's launches depend on beyond the
    step scalars: the pool's size (template matching), the relaxer and - on the device - its table's content hash"""
    if p["align"]:
        return ("align", slot.poses is not None and (slot.n_conf, slot.n_lig))
    if p["mmff"]:
        r = slot.relaxer
        return ("mmff", (r.kind, r.kind == "device" and r.terms.signature(), int(mmff_iters), slot.n_lig))
    return ("plain",)


def tail_key(common, slot, i, mmff_iters):
    """unit key of slot's tail of step i.  `common` carries the shape with the REAL atom / token counts (launch arguments -
    reduction bounds - of the captured kernels: two systems that pad to one shape must not share a graph); a group's starts
    with "many" and carries the group's fields"""
    p = slot.plan[i]
    return (common, "T", slot.g, i, p["t_hat"], p["eta"], p["dt"], tail_kind(p, slot, mmff_iters))


class StepLoop:
    """the row buffers of one loop over len(plans) systems x B samples, its slots and the step functions"""

    def __init__(self, eng, prefix, plans, B, A, sig0, noise_scale_lambda, mmff_iters, noise_mode):
        self.L = ops._lib.init()
        self.ws, self.device, self.B, self.A = eng.ws, eng.device, B, A
        self.sig0, self.lam, self.iters = float(sig0), float(noise_scale_lambda), int(mmff_iters)
        G, self.steps = len(plans), len(plans[0])
        R = G * B

        def buf(name, *shape, **kw):
            return eng.ws.get(prefix + name, *shape, **kw)
        self.x_a, self.x_hat, self.x_den, self.x_proj = (buf(n, R, A, 3) for n in ("x_a", "x_hat", "x_den", "x_proj"))
        self.bref = buf("bref", R, A, 3) if any(p["align"] for pl in plans for p in pl) else None
        self.x_ref = buf("x_ref", R, A, 3) if any(p["mmff"] for pl in plans for p in pl) else None
        self.lig_w = buf("lig_w", G, A)
        # random numbers: parity mode copies the callers' draws into fixed buffers (add_slot); the schedule - hence which steps
        # inject noise - is the same for every slot
        noisy = [p["noisy"] for p in plans[0]]
        self.n_noisy = sum(noisy)
        self.k_noisy = [sum(noisy[:i]) for i in range(self.steps)]
        if noise_mode:
            self.n_init = buf("n_init", R, A, 3, zero=True)
            self.n_rot = buf("n_rot", G, self.steps, 4, B)
            self.n_tr = buf("n_trans", G, self.steps, B, 3)
            self.n_dif = buf("n_diffuse", G, max(self.n_noisy, 1), B, A, 3, zero=True)
        else:
            self.seed = buf("seed", G, dtype=torch.int64)
        self.slots = []

    def add_slot(self, prefix, label, batch, a_mask, ref_pos, plan, relaxer, ref_mol_poses, noise, seed, sample_offset):
        """stage what system `batch` (prepared; `a_mask` / `ref_pos`: its staged copies) contributes, as the next slot"""
        ws, L, device, B, A = self.ws, self.L, self.device, self.B, self.A
        A_real = batch["_A_real"]
        s = Slot()
        s.g = g = len(self.slots)
        rows = slice(g * B, (g + 1) * B)
        s.plan, s.relaxer, s.sample_offset, s.a_mask, s.ref_pos = plan, relaxer, sample_offset, a_mask, ref_pos
        s.x_a, s.x_hat, s.x_den, s.x_proj = self.x_a[rows], self.x_hat[rows], self.x_den[rows], self.x_proj[rows]
        any_align = any(p["align"] for p in plan)
        any_mmff = any(p["mmff"] for p in plan)
        s.fill_bref = any_align
        s.bref = self.bref[rows] if any_align else None
        s.x_ref = self.x_ref[rows] if any_mmff else None

        def staged(name, t):
            b = ws.get(prefix + name, *t.shape, dtype=t.dtype)
            b.copy_(t)
            return b
        lig_flag = batch["is_ligand"][batch["atom_id_to_token_id"]]          # index gather on metadata, once per call
        lig_flag[A_real:] = 0                                                # padded atoms carry a placeholder token index
        s.lig_w = self.lig_w[g]
        s.lig_w.copy_(a_mask * lig_flag)
        s.lig_idx = s.poses = s.ref_dist = s.tm_eps = None
        s.n_lig = s.n_conf = 0
        if (any_align and ref_mol_poses is not None) or any_mmff:
            s.lig_idx = staged("lig_idx", torch.nonzero(lig_flag > 0).flatten().to(torch.int32))
            s.n_lig = int(s.lig_idx.numel())
        # (a pool for another atom count: the reference silently keeps ref_pos, model.py:229-243)
        if any_align and ref_mol_poses is not None and ref_mol_poses.shape[1] == s.n_lig:
            s.poses = staged("poses", ref_mol_poses.to(device).float())
            s.n_conf = s.poses.shape[0]
            s.ref_dist = ws.get(prefix + "ref_dist", s.n_conf, s.n_lig, s.n_lig)
            s.tm_eps = ws.get(prefix + "tm_eps", B, s.n_conf)      # eps[b, c] scratch: lets the matching run conformer-parallel
            ops.check(L.pd_pose_dist(ops.ptr(s.poses), ops.ptr(s.ref_dist), s.n_conf, s.n_lig, ops.stream()), "pose_dist")
        if any_mmff:
            if s.n_lig == 0:
                raise ValueError(f"ref_mol given but {label} has no ligand atoms")
            if relaxer.kind == "host":
                slot_of = torch.full((A,), -1, dtype=torch.int32, device=device)
                slot_of[s.lig_idx.long()] = torch.arange(s.n_lig, dtype=torch.int32, device=device)
                s.atom_slot = staged("atom_slot", slot_of)
                s.lig_in = ws.get(prefix + "lig_in", B, s.n_lig, 3)
                s.lig_out = ws.get(prefix + "lig_out", B, s.n_lig, 3)
            else:
                s.mm = relaxer.terms.device_tables(device, s.n_lig)
                s.mm_ws = ws.get(prefix + "mmff_ws", relaxer.terms.workspace_numel(B), dtype=torch.float64)
        if noise is not None:                      # (atoms beyond A_real stay zero)
            s.seed = None
            s.n_init, s.n_rot, s.n_tr, s.n_dif = self.n_init[rows], self.n_rot[g], self.n_tr[g], self.n_dif[g]
            s.n_init[:, :A_real].copy_(noise["init"])
            s.n_rot.copy_(noise["rot_u"])
            s.n_tr.copy_(noise["trans"])
            if self.n_noisy:
                s.n_dif[:self.n_noisy, :, :A_real].copy_(noise["diffuse"])
        else:
            s.seed = self.seed[g:g + 1]
            s.seed.fill_(int(seed))
        self.slots.append(s)
        return s

    # ------------------------------------------------------------------ step functions (recorded into graphs: launches only)
    def augment(self, s, i):
        """model.py:212-218: augmentation and noise injection of slot s (step 0: its initial noise and reference copy)"""
        L, B, A, p = self.L, self.B, self.A, s.plan[i]
        sp = ops.stream()
        if i == 0 and s.fill_bref:       # `batch_ref_pos = ref_pos[None].repeat(...)` (model.py:183): part of the replayed loop
            s.bref.copy_(s.ref_pos[None].expand(B, A, 3))
        if s.seed is None:
            ru, tr = off(s.n_rot, i * 4 * B), off(s.n_tr, i * B * 3)
            nz = off(s.n_dif, self.k_noisy[i] * B * A * 3) if p["noisy"] else None
            sd = None
            src, x_scale = (s.n_init, self.sig0) if i == 0 else (s.x_a, 1.0)
        else:
            ru = tr = nz = None
            sd = ops.ptr(s.seed)
            src, x_scale = s.x_a, 1.0
            if i == 0:
                ops.check(L.pd_init_noise(ops.ptr(s.x_a), sd, s.sample_offset, self.sig0, B, A, sp), "init_noise")
        ops.check(L.pd_augment(ops.ptr(src), x_scale, ops.ptr(s.a_mask), ru, tr, nz, self.lam, p["sdev"], sd, i, s.sample_offset,
                               ops.ptr(s.x_hat), B, A, sp), "augment")

    def head(self, i, denoise):
        """augment every slot, then the entry point's one denoiser call for all rows (model.py:219-221)"""
        for s in self.slots:
            self.augment(s, i)
        denoise(i)

    def gather(self, s):
        """the ligand read-out of a host relaxation"""
        ops.check(self.L.pd_ligand_gather(ops.ptr(s.x_den), ops.ptr(s.lig_idx), ops.ptr(s.lig_in), self.B, self.A, s.n_lig,
                                          ops.stream()), "ligand_gather")

    def host_relax(self, s):
        s.lig_out.copy_(s.relaxer(s.lig_in.clone(), self.iters).to(device=self.device, dtype=torch.float32))

    def tail(self, s, i):
        """model.py:223-281: physics correction and Euler update of slot s"""
        L, B, A, p = self.L, self.B, self.A, s.plan[i]
        sp = ops.stream()
        if p["align"]:
            if s.poses is not None:
                ops.check(L.pd_template_match(ops.ptr(s.x_den), ops.ptr(s.lig_idx), ops.ptr(s.ref_dist), ops.ptr(s.poses),
                                              ops.ptr(s.bref), ops.ptr(s.tm_eps), None, B, A, s.n_lig, s.n_conf, sp), "template_match")
            target = s.bref
        elif p["mmff"]:
            if s.relaxer.kind == "host":
                ops.check(L.pd_ligand_scatter(ops.ptr(s.x_ref), ops.ptr(s.x_den), ops.ptr(s.lig_out), ops.ptr(s.atom_slot),
                                              B, A, s.n_lig, sp), "ligand_scatter")
            else:
                s.relaxer.terms.launch_relax(s.mm, s.x_den, s.lig_idx, s.x_ref, s.mm_ws, B, A, self.iters, sp)
            target = s.x_ref
        else:
            target = None
        proj = lig_w = None
        if target is not None:
            proj, lig_w = ops.ptr(s.x_proj), ops.ptr(s.lig_w)
            ops.check(L.pd_kabsch_align(ops.ptr(s.x_den), ops.ptr(s.a_mask), ops.ptr(target), A * 3, lig_w, proj, B, A, sp), "kabsch")
        ops.check(L.pd_euler(ops.ptr(s.x_hat), ops.ptr(s.x_den), proj, lig_w, p["t_hat"], p["eta"], p["dt"], ops.ptr(s.x_a),
                             B, A, sp), "euler")

    def units(self, common, denoise):
        """the loop as a list of (key, fn, after, terms): fn() issues the unit's launches; `after` (or None) is host work that
        must run once the unit has been issued - a host relaxation reads the gathered ligand: the loop breaks there; `terms`
        (or None) is the MMFF table object whose device tables the unit's launches address"""
        units = []
        for i, p in enumerate(self.slots[0].plan):           # (noisy, sdev, t_hat: the schedule's, equal in every slot's plan)
            fill = tuple(i == 0 and s.fill_bref for s in self.slots)
            units.append(((common, "H", i, p["noisy"], p["sdev"], p["t_hat"], fill), partial(self.head, i, denoise), None, None))
            for s in self.slots:
                q = s.plan[i]
                if q["mmff"] and s.relaxer.kind == "host":
                    units.append(((common, "G", s.g, i, s.n_lig), partial(self.gather, s), partial(self.host_relax, s), None))
                units.append((tail_key(common, s, i, self.iters), partial(self.tail, s, i), None,
                              s.relaxer.terms if q["mmff"] else None))
        return units


def record(model, fn_lists, sync=True):
    """record (not run) each list of launch functions as one hipGraph; one capture at a time per process: objects driven from
    several host threads (parallel.StreamPool) replay concurrently, but two overlapping captures make unrelated launches of the
    other thread fail.  sync=False (units recorded in the middle of a call): no device synchronisation around the recording -
    nothing is enqueued on the recording stream, and the launch stream keeps executing the units issued before"""
    L = ops._lib.init()
    with _CAPTURE_LOCK:
        if sync:
            torch.cuda.synchronize()
        t_cap = time.perf_counter()
        execs = []
        if model._capture_stream is None:
            model._capture_stream = torch.cuda.Stream()
        with torch.cuda.stream(model._capture_stream):
            for fns in fn_lists:
                ops.check(L.pd_graph_begin(ops.stream()), "graph_begin")
                for fn in fns:
                    fn()
                ex = C.c_void_p()
                ops.check(L.pd_graph_end(ops.stream(), C.byref(ex)), "graph_end")
                execs.append(ex)
        if sync:
            torch.cuda.synchronize()
            model.last_capture_ms = 1e3 * (time.perf_counter() - t_cap)
        else:
            model.last_capture_ms = (model.last_capture_ms or 0.0) + 1e3 * (time.perf_counter() - t_cap)
    return execs


def run_units(model, units, use_graph, pipelined):
    """Issue the loop.  use_graph=False: every unit runs eagerly.  Otherwise the units that exist in `model._units` are replayed
    and the others run eagerly - they produce this call's result AND allocate their workspace buffers, so recording them behind
    the loop needs no launch of its own.
    pipelined: a missing unit whose KIND (head / gather / tail of one physics branch) has already run once on this shape - earlier
    in this call or in an earlier one - finds every workspace buffer it touches allocated: it is RECORDED first (no execution:
    ~12 us per launch on the host against ~35 us for an eager launch) and then launched like a cached one, while the GPU still
    works on the units issued before.  Only the first unit of a kind runs eagerly (it allocates).  First call of a new shape at
    20 samples: 225 -> 179 ms against 164 ms cached; at 64 samples 392 -> 334 ms against 333 ms (profiles/r06_new_shape_call.txt).
    Returns whether any launch of this call ran for the first time (= was not replayed from a checked capture)."""
    if not use_graph:
        for _, fn, after, _ in units:
            fn()
            if after is not None:
                after()
        return True
    L = ops._lib.init()
    sp = ops.stream()
    fresh = False
    missing, recorded = [], 0
    if pipelined:
        model.last_capture_ms = 0.0
    for ukey, fn, after, terms in units:
        u = model._units.get(ukey)
        kind = (ukey[0], ukey[1], ukey[-1][0] if ukey[1] == "T" else None)
        if u is None and pipelined and kind in model._warm_kinds:
            u = model._units[ukey] = {"exec": record(model, [[fn]], sync=False)[0], "terms": terms}
            model.unit_captures += 1
            recorded += 1
            fresh = True                                       # (its first execution: the caller's finite check applies)
        if u is not None:
            model._units[ukey] = model._units.pop(ukey)        # LRU order
            ops.check(L.pd_graph_launch(u["exec"], sp), "graph_launch")
        else:
            fresh = True
            fn()
            missing.append((ukey, fn, terms))
            model._warm_kinds.add(kind)
        if after is not None:
            after()
    model.last_unit_misses = len(missing) + recorded
    model.last_head_misses = sum(1 for k, _, _ in missing if k[1] == "H")
    if missing:
        # the captured launches hold raw device addresses: a unit keeps the MMFF table object whose tables it captured alive
        # (a later call with an EQUAL table - same signature, e.g. rebuilt from the same RDKit molecule - replays against
        # these tables, not against its own freshly built and soon freed ones)
        for (ukey, _, terms), ex in zip(missing, record(model, [[fn] for _, fn, _ in missing], sync=not pipelined)):
            model._units[ukey] = {"exec": ex, "terms": terms}
        model.unit_captures += len(missing)
    while len(model._units) > model.max_cached_units:
        L.pd_graph_destroy(model._units.pop(next(iter(model._units)))["exec"])
    return fresh
