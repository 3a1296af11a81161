"""Does a sampled pose agree with what the trunk itself predicted about distances - and which ligand atom sits where the trunk did not
expect it?  The released model carries a trained distance head (`linear_distogram`: 39-bin logits over the pseudo-beta distance of two
tokens, 3.25 .. 50.75 A) that the sampler never reads; `PhysDock.predict_distogram` makes the logits available at inference and
`DistogramScore` scores every pose against them on the device (kernels `pd_distogram_*`, csrc/distogram_score.hip;
tests/distogram_score_ref.py is the written definition).  No ground truth, no confidence weights, no borrowed force field.

One system: logits `l [T,T,K]` fp32, `pb [T]` (`token_id_to_pseudo_beta_atom_id`; -1 = the token has none), `is_ligand [T]`, `s_mask [T]`
(ones if absent).  A token is active when `s_mask != 0` and `pb >= 0`; L = the active ligand tokens, R = the other active tokens.  The
pair classes are `interface` (i in L, j in R, read at `l[i,j]`), `ligand` (i < j both in L) and - only with `receptor=True`, because in
redocking the receptor's template comes from `x_gt` and makes these pairs uninformative - `receptor` (i < j both in R).

    edges      e_k = linspace(min_bin, max_bin, K - 1) in float64; centres c_0 = e_0 - w / 2, c_b = (e_{b-1} + e_b) / 2,
               c_{K-1} = e_{K-2} + w / 2 with w = e_1 - e_0
    tables     lse = log sum_b exp l_b (float64), u_b = lse - l_b; expected = sum_b exp(-u_b) c_b and p_contact = sum_{b <= c*}
               exp(-u_b) in fp32, c* the last bin whose upper edge is <= contact_cutoff (`contact_edge` is that edge)
    pair       d2 in float64 from the fp32 coordinates, bin = #{k : d2 > e_k^2} (the convention of the distogram loss), nll = u[bin]

`score(x_pred [P,A,3], detail=False)` returns device tensors, nothing is read back: `nll_interface`, `nll_ligand`, `nll_receptor`, `nll`
fp32 [P] (the mean NLL of a class, of the enabled classes together; NaN where a class has no pair), `n_pairs` int32 [3], `token_nll` fp32
[P,T] (per token the mean interface NLL against the other side: a high value is a ligand atom where the trunk did not expect it; NaN
for a token without a partner), `expected_error` [P] (the mean |d - expected| over the interface pairs with expected <= max_expected),
`contact_recovery` [P] (of the interface pairs with p_contact >= 0.5, the share the pose has at bin <= c*), `contact_precision` [P] (the
mean p_contact over the interface pairs the pose has in contact), `n_contacts` int32 [P], `ok` uint8 [P] (0: a non-finite coordinate at
an active pseudo-beta atom; that pose's floats are NaN and its integers 0) and, with `detail=True`, `bins` uint8 [P,|L|,T] (the bin of
every pair of a ligand row, 255 in the column of an inactive token).

`potential(x_pred, forces=False)`: V_ij(d) interpolates u_ij linearly between the centres (constant below c_0 and from c_{K-1} on, the
right-hand slope at a centre, no gradient at d = 0); `potential` fp32 [P] is its mean over the interface and ligand pairs, `forces`
fp32 [P,|L|,3] minus its gradient on the pseudo-beta atom of each ligand token (the receptor is rigid, as in `VinaScore`) and
`abs_force` [P,|L|] the sum of the absolute values of the contributions.

Every sum is float64 in a fixed order: a pose's values are bit-identical whatever the batch.

**Caveats.**  The distogram sees ONE pseudo-beta atom per residue: side-chain placement is invisible to it.  The bins are 1.28 A wide.
In redocking the receptor template makes receptor - receptor pairs uninformative (hence `receptor=False`).  Agreement with the trunk is
self-consistency, not accuracy: a confidently wrong trunk rewards the wrong pose.  The defaults - contact_cutoff 8.0 A, max_expected
20.0 A, the choice of classes - are THIS PACKAGE'S OWN AND HAVE NOT BEEN VALIDATED on real complexes.  Limits: 2 <= K <= 64, T <= 4096,
P <= 65535.  Out of scope: minimising the potential or adding it to `VinaRefine`, feeding it into the sampler, atom-level distograms,
several systems in one launch.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .scoring import _host

__all__ = ["DistogramScore", "edges_centres", "DEFAULT_CONTACT_CUTOFF", "DEFAULT_MAX_EXPECTED", "DEFAULT_MIN_BIN", "DEFAULT_MAX_BIN",
           "MIN_BINS", "MAX_BINS", "MAX_TOKENS", "MAX_POSES", "VALUE_NAMES", "INACTIVE_BIN", "INACTIVE", "RECEPTOR", "LIGAND"]

#: the defaults (this package's own, not validated) and the bin range of config.loss.distogram_loss
DEFAULT_CONTACT_CUTOFF, DEFAULT_MAX_EXPECTED, DEFAULT_MIN_BIN, DEFAULT_MAX_BIN = 8.0, 20.0, 3.25, 50.75
#: limits of the kernels (csrc/distogram_score.hip)
MIN_BINS, MAX_BINS, MAX_TOKENS, MAX_POSES = 2, 64, 4096, 65535
#: the rows of the kernel's `values [7,P]`
VALUE_NAMES = ("nll_interface", "nll_ligand", "nll_receptor", "nll", "expected_error", "contact_recovery", "contact_precision")
#: the byte of `bins` in the column of an inactive token; values of a class byte
INACTIVE_BIN = 255
INACTIVE, RECEPTOR, LIGAND = 0, 1, 2


def edges_centres(min_bin: float = DEFAULT_MIN_BIN, max_bin: float = DEFAULT_MAX_BIN, no_bins: int = 39) -> Tuple[np.ndarray, np.ndarray]:
    """(edges float64 [K-1], centres float64 [K]) of the module docstring"""
    e = np.linspace(np.float64(min_bin), np.float64(max_bin), no_bins - 1)
    w = e[1] - e[0] if no_bins > 2 else np.float64(max_bin) - np.float64(min_bin)
    c = np.empty(no_bins, np.float64)
    c[0], c[-1] = e[0] - w / 2, e[-1] + w / 2
    c[1:-1] = (e[:-1] + e[1:]) / 2
    return e, c


class DistogramScore:
    """One system's spec, immutable, plus its device tables: host copies `token_class` uint8 [T], `pb_atom` int32 [T], `rows` int32 (the
    ligand tokens, then with `receptor` the receptor tokens), `ligand_tokens` / `receptor_tokens`, `edges`, `centres`, `contact_bin` (c*),
    `contact_edge`, `contact_cutoff`, `max_expected`, `receptor`, `n_pairs` int32 [3], `n_tokens` T, `no_bins` K, `n_pose_atoms` A; the
    logits stay where they were given and the tables (`lse`, `expected`, `p_contact`) are computed once per device, on first use."""

    def __init__(self, logits, pb, is_ligand, s_mask, n_pose_atoms, contact_cutoff, max_expected, receptor, min_bin, max_bin):
        if not isinstance(logits, torch.Tensor) or logits.dim() != 3 or logits.shape[0] != logits.shape[1]:
            raise ValueError(f"DistogramScore: the logits must be a tensor [T,T,no_bins], got {tuple(getattr(logits, 'shape', ()))}")
        if logits.dtype != torch.float32:
            raise ValueError(f"DistogramScore: the logits must be fp32 (PhysDock.predict_distogram), got {logits.dtype}")
        T, K = int(logits.shape[0]), int(logits.shape[2])
        if not (MIN_BINS <= K <= MAX_BINS and 1 <= T <= MAX_TOKENS):
            raise ValueError(f"DistogramScore: logits over {T} tokens and {K} bins; the kernels take up to {MAX_TOKENS} tokens and "
                             f"{MIN_BINS} .. {MAX_BINS} bins")
        pb = _host(pb, np.int64).reshape(-1)
        lig = _host(is_ligand, np.float64).reshape(-1) != 0
        sm = np.ones(T, bool) if s_mask is None else _host(s_mask, np.float64).reshape(-1) != 0
        if not (pb.shape[0] == lig.shape[0] == sm.shape[0] == T):
            raise ValueError(f"DistogramScore: the logits are over {T} tokens; pseudo-beta ids {pb.shape[0]}, is_ligand {lig.shape[0]}, "
                             f"s_mask {sm.shape[0]}")
        A = int(n_pose_atoms)
        if A < 1 or (pb >= A).any():
            raise ValueError(f"DistogramScore: a pseudo-beta atom id of {int(pb.max())} with poses of {A} atoms")
        for name, v in (("contact_cutoff", contact_cutoff), ("max_expected", max_expected), ("min_bin", min_bin), ("max_bin", max_bin)):
            if not np.isfinite(float(v)):
                raise ValueError(f"DistogramScore: {name} must be finite, got {v}")
        if not 0 <= float(min_bin) < float(max_bin):
            raise ValueError(f"DistogramScore: expected 0 <= min_bin < max_bin, got {min_bin}, {max_bin}")
        active = sm & (pb >= 0)
        cls = np.where(active, np.where(lig, LIGAND, RECEPTOR), INACTIVE).astype(np.uint8)
        edges, centres = edges_centres(min_bin, max_bin, K)
        near = np.nonzero(edges <= np.float64(contact_cutoff))[0]
        lt, rt = np.nonzero(cls == LIGAND)[0], np.nonzero(cls == RECEPTOR)[0]
        row_of = np.full(T, -1, np.int32)
        row_of[lt] = np.arange(lt.shape[0])
        nl, nr = int(lt.shape[0]), int(rt.shape[0])
        s = object.__setattr__
        s(self, "logits", logits.detach())
        s(self, "token_class", cls)
        s(self, "pb_atom", np.where(active, pb, 0).astype(np.int32))
        s(self, "ligand_tokens", lt.astype(np.int32))
        s(self, "receptor_tokens", rt.astype(np.int32))
        s(self, "rows", np.concatenate([lt, rt] if receptor else [lt]).astype(np.int32))
        s(self, "row_of", row_of)
        s(self, "edges", edges)
        s(self, "centres", centres)
        s(self, "contact_bin", int(near[-1]) if near.size else -1)
        s(self, "contact_edge", float(edges[near[-1]]) if near.size else float("nan"))
        s(self, "contact_cutoff", float(contact_cutoff))
        s(self, "max_expected", float(np.float32(max_expected)))
        s(self, "receptor", bool(receptor))
        s(self, "n_pairs", np.asarray([nl * nr, nl * (nl - 1) // 2, nr * (nr - 1) // 2 if receptor else 0], np.int32))
        s(self, "n_tokens", T)
        s(self, "no_bins", K)
        s(self, "n_pose_atoms", A)
        s(self, "_tables", {})

    def __setattr__(self, name, value):
        raise AttributeError("DistogramScore is immutable")

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_logits(p_distogram, batch, contact_cutoff: float = DEFAULT_CONTACT_CUTOFF, max_expected: float = DEFAULT_MAX_EXPECTED,
                    receptor: bool = False, min_bin: float = DEFAULT_MIN_BIN, max_bin: float = DEFAULT_MAX_BIN, pseudo_beta=None):
        """p_distogram fp32 [T,T,K] (`PhysDock.predict_distogram`, or `forward(batch)["p_distogram"]`); the batch gives
        `token_id_to_pseudo_beta_atom_id` (or `pseudo_beta=` [T]; a batch without it, like the sampler's own feature dict, falls back
        to the first atom of every token), `is_ligand`, `s_mask` (ones if absent) and the atom count of a pose.  contact_cutoff,
        max_expected (A), receptor: the module docstring - this package's own defaults, not validated; min_bin / max_bin: those of
        `config.loss.distogram_loss`."""
        if pseudo_beta is None:
            pseudo_beta = batch.get("token_id_to_pseudo_beta_atom_id")
        if pseudo_beta is None:
            chunk = batch["token_id_to_chunk_sizes"].long()
            pseudo_beta = torch.cumsum(chunk, 0) - chunk
        n_atoms = int((batch["x_gt"] if "x_gt" in batch else batch["atom_id_to_token_id"]).shape[0])
        return DistogramScore(p_distogram, pseudo_beta, batch["is_ligand"], batch.get("s_mask"), n_atoms, contact_cutoff, max_expected,
                              receptor, min_bin, max_bin)

    @staticmethod
    def from_conditioning(model, batch, conditioning, **kw):
        """through `model.predict_distogram(batch, conditioning=)`: `conditioning` is what `sample_diffusion(return_conditioning=True)`
        returned, or its last two tensors (s, z); the bin range comes from the model's `config.loss.distogram_loss`.  Other keywords
        as for `from_logits`."""
        cfg = getattr(getattr(getattr(model, "config", None), "loss", None), "distogram_loss", None)
        if cfg is not None:
            kw.setdefault("min_bin", cfg["min_bin"])
            kw.setdefault("max_bin", cfg["max_bin"])
        return DistogramScore.from_logits(model.predict_distogram(batch, conditioning=conditioning), batch, **kw)

    @staticmethod
    def from_batch(model, batch, **kw):
        """runs the trunk once (`model.predict_distogram(batch)`).  Other keywords as for `from_logits`."""
        return DistogramScore.from_conditioning(model, batch, None, **kw)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernels' tables on `device` (uploaded and computed once): pb_atom, token_class, rows, row_of, logits, lse, expected,
        p_contact, n_pairs"""
        device = ops.resolve_device(device)
        t = self._tables.get(device)
        if t is None:
            if device.type != "cuda":
                raise ValueError(f"DistogramScore: the kernels run on the GPU, got {device}")
            ops._lib.init()
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            T = self.n_tokens
            t = {k: up(getattr(self, k)) for k in ("pb_atom", "token_class", "rows", "row_of", "n_pairs")}
            t["logits"] = self.logits.to(device).contiguous()
            t["lse"] = torch.empty((T, T), dtype=torch.float64, device=device)
            t["expected"], t["p_contact"] = (torch.empty((T, T), dtype=torch.float32, device=device) for _ in range(2))
            with torch.cuda.device(device):
                ops.distogram_tables(t["logits"], self.centres, self.contact_bin, t["lse"], t["expected"], t["p_contact"])
            self._tables[device] = t
        return t

    def _poses(self, x_pred, who):
        if not isinstance(x_pred, torch.Tensor) or x_pred.dim() != 3 or x_pred.shape[1] != self.n_pose_atoms or x_pred.shape[2] != 3:
            raise ValueError(f"DistogramScore.{who}: the spec is over poses of {self.n_pose_atoms} atoms, x_pred has shape "
                             f"{tuple(getattr(x_pred, 'shape', ()))}")
        if not 1 <= x_pred.shape[0] <= MAX_POSES:
            raise ValueError(f"DistogramScore.{who}: {x_pred.shape[0]} poses; the kernels take 1 .. {MAX_POSES}")
        if not x_pred.is_cuda:
            raise ValueError(f"DistogramScore.{who}: x_pred must be on the GPU, got a tensor on {x_pred.device}")
        return x_pred.float().contiguous()

    def score(self, x_pred: torch.Tensor, detail: bool = False) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> the dict of device tensors of the module docstring.  Nothing is read back."""
        x = self._poses(x_pred, "score")
        t = self.tables(x.device)
        P, T = x.shape[0], self.n_tokens
        nL, nR, NR = int(self.ligand_tokens.shape[0]), int(self.receptor_tokens.shape[0]), int(self.rows.shape[0])
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=x.device)
        bins = new((P, nL, T), torch.uint8)
        ws = new((P * NR * 8,), torch.float64)
        out = dict(values=new((len(VALUE_NAMES), P), torch.float32), token_nll=new((P, T), torch.float32),
                   n_contacts=new((P,), torch.int32), ok=new((P,), torch.uint8))
        ops.distogram_score(x, t, self.edges * self.edges, self.contact_bin, self.max_expected, bins, ws, out, nL, nR, NR)
        values = out.pop("values")
        out.update({k: values[i] for i, k in enumerate(VALUE_NAMES)})
        out["n_pairs"] = t["n_pairs"]
        if detail:
            out["bins"] = bins
        return out

    def potential(self, x_pred: torch.Tensor, forces: bool = False) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> {"potential" fp32 [P]} and, with forces=True, "forces" fp32 [P,|L|,3] (minus the gradient on the
        pseudo-beta atom of every ligand token, `ligand_tokens` order) and "abs_force" fp32 [P,|L|].  Nothing is read back."""
        x = self._poses(x_pred, "potential")
        t = self.tables(x.device)
        P = x.shape[0]
        nL, nR = int(self.ligand_tokens.shape[0]), int(self.receptor_tokens.shape[0])
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=x.device)
        out = {"potential": new((P,), torch.float32)}
        if forces:
            out["forces"], out["abs_force"] = new((P, nL, 3), torch.float32), new((P, nL), torch.float32)
        ops.distogram_potential(x, t, self.centres, new((P * nL * 5,), torch.float64), out["potential"], out.get("forces"),
                                out.get("abs_force"), nL, nR)
        return out

    def describe(self, result, row: int) -> List[Tuple[int, float]]:
        """host helper (one read-back): [(ligand token id, token_nll)] of pose `row`, the worst (largest) first, token order among
        equal values; tokens without a value (NaN) come last"""
        v = result["token_nll"][row]
        v = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(-1)
        if v.shape[0] != self.n_tokens:
            raise ValueError(f"DistogramScore.describe: a row holds {self.n_tokens} values, got {v.shape[0]}")
        key = lambda t: (np.isnan(v[t]), -v[t] if not np.isnan(v[t]) else 0.0, t)
        return [(int(t), float(v[t])) for t in sorted((int(t) for t in self.ligand_tokens), key=key)]

    def __repr__(self):
        return (f"DistogramScore(tokens={self.n_tokens}, bins={self.no_bins}, ligand_tokens={self.ligand_tokens.shape[0]}, "
                f"receptor_tokens={self.receptor_tokens.shape[0]}, contact_cutoff={self.contact_cutoff:g} (edge {self.contact_edge:g}), "
                f"max_expected={self.max_expected:g}, receptor={self.receptor})")
