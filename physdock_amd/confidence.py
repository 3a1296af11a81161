"""`ConfidenceModule` - the reference's confidence head (PhysDock/models/layers/confidence_module.py:13-88) on the HIP
kernels.

The reference keeps this module out of the released model (model.py:15,68 are commented out; the file's first line says
so), but its config block (`config.model.confidence_module`, configs.py:141-150) and the class are part of the package.
Same constructor signature, same parameter names (strict ``load_state_dict`` of a reference module's state dict works),
same ``forward(batch, s, z, x_pred) -> (p_pae, p_pde, p_plddt)``.  The Pairformer and AtomTransformer stacks inside it run
through the trunk's kernels (engine.Engine.pairformer / atom_transformer); three small element-wise kernels
(csrc/confidence.hip) cover the entry and exit.  No PyTorch compute fallback: on a machine without the built library or
without a GPU the call raises.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .configs import ConfigDict
from .engine import Engine
from .model import _register
from .packing import PackedWeights
from .params import confidence_param_shapes


class ConfidenceModule(nn.Module):
    def __init__(self, c_a: int, c_ap: int, c_s: int, c_z: int, inf: float, eps: float, no_blocks_heads: int,
                 no_blocks_atom: int = 3, c_pae: int = 64, c_pde: int = 64, c_plddt: int = 50):
        super().__init__()
        self.dims = dict(c_a=c_a, c_ap=c_ap, c_s=c_s, c_z=c_z, no_blocks_heads=no_blocks_heads, no_blocks_atom=no_blocks_atom,
                         c_pae=c_pae, c_pde=c_pde, c_plddt=c_plddt)
        for k in ("c_a", "c_s", "c_z"):
            assert self.dims[k] % 32 == 0, f"{k} must be a multiple of the head width 32"
        self.inf, self.eps = float(inf), float(eps)
        for name, shape in confidence_param_shapes(**self.dims).items():
            _register(self, name, torch.zeros(shape))
        self._engine: Optional[Engine] = None
        #: forward_poses / score_poses keep the logits and entry tensors of a chunk of poses in cached workspace buffers; the default
        #: chunk is what fits this budget, and a cache grown beyond it (systems of many sizes) is dropped at the next call
        self.workspace_limit_bytes = 8 * 2 ** 30
        self.register_load_state_dict_post_hook(lambda m, k: m._invalidate())

    def _invalidate(self):
        self._engine = None

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._invalidate()
        return r

    def engine(self, device) -> Engine:
        if self._engine is None or self._engine.device != device:
            if device.type != "cuda":
                raise RuntimeError("physdock_amd.ConfidenceModule runs on an MI355X (HIP) device only; there is no CPU path "
                                   "(the CPU oracle lives in oracle/ and is test-only)")
            params = {"confidence_module." + k: v for k, v in self.state_dict().items()}
            if any(v.device != device for v in params.values()):
                raise RuntimeError("module parameters and batch must be on the same device")
            cfg = ConfigDict({"model": {"diffusion_conditioning": {"inf": self.inf, "eps": self.eps}}})
            self._engine = Engine(PackedWeights(params, cfg), cfg, device)
        return self._engine

    @torch.no_grad()
    def forward(self, batch, s: torch.Tensor, z: torch.Tensor, x_pred: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """batch keys read: token_id_to_centre_atom_id [T], atom_id_to_token_id [A], ap_mask [A,A], z_mask [T,T]
        (confidence_module.py:62-65); s [T,c_s], z [T,T,c_z]; x_pred [B,A,3] of which only pose 0 is used (:66,80)."""
        eng = self.engine(x_pred.device)
        T, A = s.shape[0], x_pred.shape[-2]
        b, s_p, z_p, pa, pt = self._padded(batch, s, z, T, A)
        x0 = F.pad(x_pred[0].float(), (0, 0, 0, pa)).contiguous()
        p_pae, p_pde, p_plddt = eng.confidence(b, s_p, z_p, x0, self.dims)
        if pa or pt:
            p_pae, p_pde, p_plddt = p_pae[:T, :T].contiguous(), p_pde[:T, :T].contiguous(), p_plddt[:A].contiguous()
        return p_pae, p_pde, p_plddt

    @staticmethod
    def _padded(batch, s, z, T, A):
        """layout-only boundary work: dtypes, contiguity and - for token / atom counts that are not multiples of 4 - padding
        with masked tokens / atoms exactly like PhysDock._prepare_batch (padded entries are inert under the masks).
        Returns (engine batch, s [T', c_s], z [T' * T', c_z], padded atoms, padded tokens)."""
        device = s.device
        pa, pt = (-A) % 4, (-T) % 4
        if pa and not pt:
            pt = 4
        b = {"_A_real": A, "_T_real": T}
        b["ap_mask"] = F.pad(batch["ap_mask"].float(), (0, pa, 0, pa)).contiguous()
        b["z_mask"] = F.pad(batch["z_mask"].float(), (0, pt, 0, pt)).contiguous()
        a2t = batch["atom_id_to_token_id"].to(torch.int64)
        b["atom_id_to_token_id"] = torch.cat([a2t, torch.full((pa,), T, device=device, dtype=torch.int64)]).contiguous()
        ctr = batch["token_id_to_centre_atom_id"].to(torch.int64)
        b["token_id_to_centre_atom_id"] = torch.cat([ctr, torch.zeros(pt, device=device, dtype=torch.int64)]).contiguous()
        s_p = F.pad(s.float(), (0, 0, 0, pt)).contiguous()
        z_p = F.pad(z.float(), (0, 0, 0, pt, 0, pt)).contiguous().reshape((T + pt) * (T + pt), -1)
        return b, s_p, z_p, pa, pt

    def default_chunk(self, T, A, num_poses):
        """poses whose logits and entry tensors exist at a time: as many as fit half of `workspace_limit_bytes` (at least one; the
        other half is left to the stacks' own scratch, so that a call of the default chunk never trips the cache-drop rule)"""
        Tp, Ap = T + (-T) % 4, A + (-A) % 4
        per = Engine.confidence_pose_bytes(Tp, Ap, self.dims, self.dims["c_pae"], self.dims["c_pde"], self.dims["c_plddt"])
        return max(1, min(int(num_poses), int(self.workspace_limit_bytes) // 2 // per))

    def _poses_setup(self, batch, s, z, x_pred, chunk):
        if x_pred.dim() != 3 or x_pred.shape[-1] != 3:
            raise ValueError(f"x_pred must be [num_poses, num_atoms, 3], got {tuple(x_pred.shape)}")
        eng = self.engine(x_pred.device)
        T, A, NP = s.shape[0], x_pred.shape[1], x_pred.shape[0]
        if NP < 1:
            raise ValueError("x_pred holds no pose")
        if chunk is not None and int(chunk) < 1:
            raise ValueError(f"chunk={chunk}: expected a positive number of poses")
        b, s_p, z_p, pa, pt = self._padded(batch, s, z, T, A)
        x = F.pad(x_pred.float(), (0, 0, 0, pa)).contiguous()
        chunk = min(NP, int(chunk)) if chunk is not None else self.default_chunk(T, A, NP)
        if eng.ws.nbytes() > self.workspace_limit_bytes:       # systems of many sizes passed through: start from an empty cache
            torch.cuda.synchronize(x.device)
            eng.ws.bufs.clear()
        return eng, b, s_p, z_p, x, T, A, NP, pt, chunk

    @torch.no_grad()
    def forward_poses(self, batch, s: torch.Tensor, z: torch.Tensor, x_pred: torch.Tensor, poses=None):
        """`forward` for the rows `poses` (index tensor or list; default: all) of x_pred [B,A,3]: (p_pae [P,T,T,c_pae], p_pde
        [P,T,T,c_pde], p_plddt [P,A,c_plddt]), row p bit-equal to `forward(batch, s, z, x_pred[i:i+1])` for i = poses[p].  What does
        not depend on the pose runs once per call (Engine.confidence_poses); the stacked logits are fresh tensors - at T = 256 they
        are 33.5 MB per pose, so to rank many poses use `score_poses`, which never holds more than a chunk of them."""
        if poses is not None:
            idx = torch.as_tensor(poses, dtype=torch.int64, device=x_pred.device).reshape(-1)
            x_pred = x_pred.index_select(0, idx)
        eng, b, s_p, z_p, x, T, A, NP, pt, chunk = self._poses_setup(batch, s, z, x_pred, None)
        Tp, d = T + pt, self.dims
        out = (torch.empty(NP, T, T, d["c_pae"], device=x.device), torch.empty(NP, T, T, d["c_pde"], device=x.device),
               torch.empty(NP, A, d["c_plddt"], device=x.device))

        def sink(p0, n, pae, pde, plddt):
            out[0][p0:p0 + n].copy_(pae.view(n, Tp, Tp, -1)[:, :T, :T])
            out[1][p0:p0 + n].copy_(pde.view(n, Tp, Tp, -1)[:, :T, :T])
            out[2][p0:p0 + n].copy_(plddt[:, :A])
        eng.confidence_poses(b, s_p, z_p, x, d, chunk, sink)
        return out

    @torch.no_grad()
    def score_poses(self, batch, s: torch.Tensor, z: torch.Tensor, x_pred: torch.Tensor, *, chunk: Optional[int] = None,
                    skip_self_pairs: bool = False) -> Dict[str, torch.Tensor]:
        """The ground-truth-free scores of every pose of x_pred [P,A,3]: `get_metrics` of `forward_poses`, bit for bit, without the
        stacked logits ever existing.  Returns device tensors ranking_confidence, ptm, iptm, mean_plddt [P] (fp32), has_clash [P]
        (int64) and plddt [P,A] (also under get_metrics' name atom_plddts); `ranking.rank_by_confidence` orders poses by them.
        batch: the keys of `forward` and of `get_metrics` (s_mask, asym_id, is_ligand [T], a_mask, atom_id_to_token_id [A]).
        The logits live in workspace buffers of `chunk` poses (default: what fits `workspace_limit_bytes`) that are reused by every
        chunk and every later call; the result does not depend on `chunk`.  As `get_metrics`: no host synchronisation except on
        the first call for a batch dict (the chain index, cached under batch["_metrics_chain"]), so later calls can be captured
        in a graph.  `skip_self_pairs`: see get_metrics."""
        from . import metrics as M
        eng, b, s_p, z_p, x, T, A, NP, pt, chunk = self._poses_setup(batch, s, z, x_pred, chunk)
        s_mask, asym, a_mask, is_lig = (batch[k] for k in ("s_mask", "asym_id", "a_mask", "is_ligand"))
        M._dev("ConfidenceModule.score_poses", s_mask, asym, a_mask, is_lig)
        if tuple(a_mask.shape) != (A,) or tuple(is_lig.shape) != (T,) or tuple(s_mask.shape) != (T,):
            raise ValueError(f"inconsistent shapes: x_pred {tuple(x_pred.shape)}, s {tuple(s.shape)}, a_mask {tuple(a_mask.shape)}, "
                             f"is_ligand {tuple(is_lig.shape)}, s_mask {tuple(s_mask.shape)}")
        chain, poly, n_chain = M._chain_index(batch)
        w, asym32, am = M._f(s_mask), M._i32(asym), M._f(a_mask)
        xr = x[:, :A].contiguous() if x.shape[1] != A else x
        Tp, Ap, d, dev = T + pt, x.shape[1], self.dims, x.device
        crop = Tp != T or Ap != A
        if crop:       # get_metrics reads contiguous real-size logits: the chunk is cropped into a second reused buffer
            c_pae = eng.ws.get("confp_pae_crop", chunk, T, T, d["c_pae"])
            c_pl = eng.ws.get("confp_plddt_crop", chunk, A, d["c_plddt"])
        out = {k: torch.empty(NP, dtype=torch.float32, device=dev) for k in ("ranking_confidence", "ptm", "iptm", "mean_plddt")}
        out["has_clash"] = torch.empty(NP, dtype=torch.int64, device=dev)
        out["plddt"] = torch.empty(NP, A, dtype=torch.float32, device=dev)

        def sink(p0, n, pae, pde, plddt):
            if crop:
                c_pae[:n].copy_(pae.view(n, Tp, Tp, -1)[:, :T, :T])
                c_pl[:n].copy_(plddt[:, :A])
                la, lp = c_pae[:n], c_pl[:n]
            else:
                la, lp = pae.view(n, T, T, -1), plddt
            atom, mean = M._plddt(lp)
            r = M._pae_tm(la, w, asym32, 32.0, want_pae=False)
            has, rank = M._clash(xr[p0:p0 + n], am, chain, poly, n_chain, skip_self_pairs, r["ptm"], r["iptm"])
            for k, v in (("plddt", atom), ("mean_plddt", mean), ("ptm", r["ptm"]), ("iptm", r["iptm"]), ("has_clash", has),
                         ("ranking_confidence", rank)):
                out[k][p0:p0 + n].copy_(v)
        eng.confidence_poses(b, s_p, z_p, x, d, chunk, sink)
        out["atom_plddts"] = out["plddt"]
        return out

    @classmethod
    def from_config(cls, config):
        """`ConfidenceModule(**config.model.confidence_module)` as the reference would build it (model.py:68)"""
        return cls(**dict(config.model.confidence_module))

