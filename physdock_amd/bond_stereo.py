"""Did the double bonds come out as the stated isomer?  Tetrahedral stereo has a device-side accept / reject (`chirality`); this is
PoseBusters' other stereo check, the double-bond one: for every pose of a batch and every stated double bond, is it cis or trans, and
how far is it twisted out of its plane (kernel `pd_bond_stereo`, csrc/bond_stereo.hip: one launch, one 64-lane wave per pose).  **The
package's own definition, not RDKit's**: tests/bond_stereo_ref.py is the written form in numpy float64.

    entry            (a, b, c, d, a2, d2) with its expected kind: b=c the double bond, a the LOWEST-index heavy substituent of b, d of c,
                     a2 / d2 the other substituent or -1 (`Ligand.bond_stereo`, `smiles.parse_smiles`)
    dihedral [P,n]   the IUPAC dihedral a-b-c-d in degrees, float64 from the fp32 coordinates, rounded once to fp32; NaN for a
                     coordinate that is not finite or three atoms on a line (|m|^2 or |n|^2 < 1e-12)
    state [P,n]      0 undefined, 1 cis (cos phi > 0), 2 trans (cos phi < 0), 3 perpendicular (cos phi == 0) - of a against d
    twist [P,n]      min(|phi|, 180 - |phi|), the largest over the substituent pairs (a | a2) x (d | d2), so a pyramidal end shows
    per pose         n_wrong (entries whose state is not the expected kind; an undefined entry counts), n_twisted (twist > max_twist,
                     or undefined), max_twist_seen (NaN if any entry is undefined), ok (n_wrong == 0)

`BondStereo.from_ligand(ligand, ligand_idx)` takes the entries of a `ligand.Ligand` at the ligand's atom indices in the pose,
`from_batch(batch, ligand)` finds those in a feature dict, `from_tables(quads, expect)` takes the tables as they are.  `check(x_pred)`
returns the device tensors above and reads nothing back, `accept(x_pred)` is the bool [P] mask `redock(bond_stereo_filter=True)` stacks
with the chirality and validity masks, `label(x)` is `state` without an expectation and `describe(result, row)` the one read-back.

**Caveats.**  cis / trans relative to the lowest-index substituents, not CIP E / Z (that needs CIP priorities).  `max_twist` defaults
to 30 degrees: the package's own default, unvalidated.  `ok` and `accept` test the isomer alone; the twist is reported, not judged.
A wrong isomer is reported, not repaired.  Limits: up to 1024 entries, up to 65535 poses per launch.  Out of scope: atropisomers,
allenes and cumulenes, double bonds in rings of 8 or more atoms beyond reading their marks, V2000 / V3000 stereo flags."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from . import ops

__all__ = ["BondStereo", "MAX_ENTRIES", "MAX_POSES", "DEFAULT_MAX_TWIST", "STATES", "check_redock_bond_stereo", "score_bond_stereo"]

#: limits of the kernel (csrc/bond_stereo.hip)
MAX_ENTRIES, MAX_POSES = 1024, 65535
#: degrees; the package's own default, unvalidated
DEFAULT_MAX_TWIST = 30.0
STATES = ("undefined", "cis", "trans", "perpendicular")


class BondStereo:
    """The stated double bonds of one ligand as the kernel's tables, immutable: `entries` int32 [n,7] rows (a, b, c, d, kind, a2, d2)
    with atom indices INTO THE POSE (kind 0 where nothing is expected), `n_entries`, `n_atoms` (the ligand's atom count the spec was
    built over, or None from plain tables) and `max_twist`."""

    def __init__(self, quads, expect, n_atoms: Optional[int] = None, max_twist: float = DEFAULT_MAX_TWIST):
        q = np.array([] if quads is None else quads, dtype=np.int64).reshape(-1, 6)
        n = int(q.shape[0])
        if n > MAX_ENTRIES:
            raise ValueError(f"BondStereo: {n} entries; the kernel takes up to {MAX_ENTRIES}")
        if n and (q[:, :4].min() < 0 or q[:, 4:].min() < -1):
            row = int(np.nonzero((q[:, :4] < 0).any(1) | (q[:, 4:] < -1).any(1))[0][0])
            raise ValueError(f"BondStereo: entry {row} {tuple(q[row].tolist())} holds a negative index (only a2 and d2 may be -1)")
        if n and q.max() >= 2 ** 31:
            raise ValueError("BondStereo: an index beyond int32")
        self.has_expect = expect is not None
        e = np.zeros(n, dtype=np.int64) if expect is None else np.array(expect, dtype=np.int64).reshape(-1)
        if e.shape[0] != n:
            raise ValueError(f"BondStereo: {n} entries but {e.shape[0]} expected kinds")
        if self.has_expect and n and not np.isin(e, (1, 2)).all():
            raise ValueError("BondStereo: an expected kind is 1 (cis) or 2 (trans)")
        self.max_twist = float(max_twist)
        if not 0.0 <= self.max_twist <= 90.0:
            raise ValueError(f"BondStereo: max_twist={max_twist}; degrees in 0 .. 90")
        self.quads = np.ascontiguousarray(q, dtype=np.int32)
        self.expect = np.ascontiguousarray(e, dtype=np.uint8)
        self.entries = np.concatenate([q[:, :4], e[:, None], q[:, 4:]], axis=1).astype(np.int32)
        for a in (self.quads, self.expect, self.entries):
            a.setflags(write=False)
        self.n_entries = n
        self.n_atoms = None if n_atoms is None else int(n_atoms)
        self.max_index = int(q.max()) if n else -1
        self._tables = {}

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_tables(quads, expect=None, max_twist: float = DEFAULT_MAX_TWIST) -> "BondStereo":
        """quads [n,6] = (a, b, c, d, a2, d2), atom indices into the pose, a2 / d2 = -1 for none; expect [n] (1 cis, 2 trans) or None:
        a spec that labels only"""
        return BondStereo(quads, expect, None, max_twist)

    @staticmethod
    def from_ligand(ligand, ligand_idx=None, max_twist: float = DEFAULT_MAX_TWIST) -> "BondStereo":
        """the rows of `ligand.bond_stereo`; ligand_idx [L]: the pose index of every ligand atom (None: the pose IS the ligand)"""
        rows = np.asarray(ligand.bond_stereo, dtype=np.int64).reshape(-1, 7)
        L = int(ligand.n_atoms)
        if ligand_idx is None:
            idx = np.arange(L, dtype=np.int64)
        else:
            idx = np.asarray(ligand_idx.detach().cpu() if isinstance(ligand_idx, torch.Tensor) else ligand_idx, dtype=np.int64).reshape(-1)
            if idx.shape[0] != L or (L and idx.min() < 0):
                raise ValueError(f"BondStereo.from_ligand: ligand_idx holds {idx.shape[0]} indices for the ligand's {L} atoms, or a "
                                 "negative one")
        q = rows[:, [0, 1, 2, 3, 5, 6]]
        q = np.where(q >= 0, idx[np.clip(q, 0, None)], -1)
        return BondStereo(q, rows[:, 4], L, max_twist)

    @staticmethod
    def from_batch(batch, ligand, max_twist: float = DEFAULT_MAX_TWIST) -> "BondStereo":
        """from a feature dict: the ligand's atoms are those of `driver.ligand_atom_mask`, in the ligand's order"""
        from .driver import ligand_atom_mask
        idx = torch.nonzero(ligand_atom_mask(batch)).flatten()
        if int(idx.numel()) != ligand.n_atoms:
            raise ValueError(f"BondStereo.from_batch: the batch's ligand has {int(idx.numel())} atoms, this ligand {ligand.n_atoms}")
        return BondStereo.from_ligand(ligand, idx, max_twist)

    # ------------------------------------------------------------------ device side
    def tables(self, device) -> Dict[str, torch.Tensor]:
        """the kernel's tables on `device` (uploaded once)"""
        return ops.cached_upload(self._tables, device, lambda up: {"quads": up(self.quads.copy()), "expect": up(self.expect.copy())})

    def _run(self, x: torch.Tensor, expect: bool, what: str) -> Dict[str, torch.Tensor]:
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[2] != 3 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"BondStereo.{what}: poses must be [P >= 1, A >= 1, 3], got {tuple(getattr(x, 'shape', ()))}")
        P, A, n = int(x.shape[0]), int(x.shape[1]), self.n_entries
        if P > MAX_POSES:
            raise ValueError(f"BondStereo.{what}: {P} poses; one launch takes up to {MAX_POSES}")
        if self.max_index >= A:
            raise ValueError(f"BondStereo.{what}: the entries reach atom {self.max_index}, the poses hold {A}")
        x = x.float().contiguous()
        new = lambda shape, dtype: torch.empty(*shape, device=x.device, dtype=dtype)
        out = {"dihedral": new((P, n), torch.float32), "twist": new((P, n), torch.float32), "state": new((P, n), torch.uint8),
               "n_wrong": new((P,), torch.int32), "n_twisted": new((P,), torch.int32), "max_twist_seen": new((P,), torch.float32),
               "ok": new((P,), torch.int32)}
        if n == 0:
            out["n_wrong"].zero_(); out["n_twisted"].zero_(); out["max_twist_seen"].zero_(); out["ok"].fill_(1)
            return out
        t = self.tables(x.device)
        with torch.cuda.device(x.device):
            ops.check(ops._lib.init().pd_bond_stereo(ops.ptr(x), ops.ptr(t["quads"]), ops.ptr(t["expect"]) if expect else None,
                                                     self.max_twist, ops.ptr(out["dihedral"]), ops.ptr(out["twist"]), ops.ptr(out["state"]),
                                                     ops.ptr(out["n_wrong"]), ops.ptr(out["n_twisted"]), ops.ptr(out["max_twist_seen"]),
                                                     ops.ptr(out["ok"]), P, A, n, ops.stream()), "pd_bond_stereo")
        return out

    def check(self, x_pred: torch.Tensor) -> Dict[str, torch.Tensor]:
        """x_pred [P,A,3] (device) -> device tensors `dihedral`, `twist` fp32 [P,n], `state` uint8 [P,n], `n_wrong`, `n_twisted` int32
        [P], `max_twist_seen` fp32 [P], `ok` int32 [P] (module docstring).  Nothing is read back.  A spec without expected kinds
        counts the undefined entries as wrong."""
        return self._run(x_pred, self.has_expect, "check")

    def accept(self, x_pred: torch.Tensor) -> torch.Tensor:
        """bool [P]: poses whose every stated double bond is the expected isomer (all True without entries)"""
        if self.n_entries == 0:
            return torch.ones(x_pred.shape[0], dtype=torch.bool, device=x_pred.device)
        return self.check(x_pred)["ok"].bool()

    def label(self, x: torch.Tensor) -> torch.Tensor:
        """`state` uint8 [P,n] of the poses x [P,A,3], whatever the spec expects"""
        return self._run(x, False, "label")["state"]

    def describe(self, result: Dict[str, torch.Tensor], row: int = 0) -> List[dict]:
        """pose `row` of a `check` result as a list of dicts, worst twist first (an undefined twist in front; ties in entry order):
        `entry`, `atoms` (a, b, c, d), `expected`, `found` (names of `STATES`), `dihedral`, `twist`, `twisted`.  The one read-back."""
        got = torch.stack([result["dihedral"][row].double(), result["twist"][row].double(), result["state"][row].double()]).cpu().numpy()
        items = []
        for k in range(self.n_entries):
            tw = float(got[1, k])
            items.append({"entry": k, "atoms": tuple(int(v) for v in self.quads[k, :4]), "expected": STATES[int(self.expect[k])],
                          "found": STATES[int(got[2, k])], "dihedral": float(got[0, k]), "twist": tw,
                          "twisted": not tw <= self.max_twist})
        return sorted(items, key=lambda it: (0 if it["twist"] != it["twist"] else 1, -it["twist"] if it["twist"] == it["twist"] else 0.0,
                                             it["entry"]))

    def __repr__(self):
        return f"BondStereo(n_entries={self.n_entries}, n_atoms={self.n_atoms}, max_twist={self.max_twist:g})"


def check_redock_bond_stereo(bond_stereo, bond_stereo_filter, batch) -> None:
    """redock(bond_stereo=): raise ValueError unless it is a `BondStereo` whose entries lie inside the batch's atoms and which, when
    built from a ligand, was built over the batch's ligand atom count; `bond_stereo_filter=True` needs one with expected kinds"""
    if bond_stereo is None:
        if bond_stereo_filter:
            raise ValueError("bond_stereo_filter=True needs bond_stereo=")
        return
    if not isinstance(bond_stereo, BondStereo):
        raise ValueError(f"bond_stereo= takes a bond_stereo.BondStereo of the ligand, got {type(bond_stereo).__name__}")
    from .driver import ligand_atom_mask
    n = int(ligand_atom_mask(batch).sum())
    if bond_stereo.n_atoms is not None and bond_stereo.n_atoms != n:
        raise ValueError(f"bond_stereo= was built over {bond_stereo.n_atoms} ligand atoms, the batch's ligand holds {n}")
    A = int(batch["x_gt"].shape[0])
    if bond_stereo.max_index >= A:
        raise ValueError(f"bond_stereo= reaches atom {bond_stereo.max_index}, the batch holds {A}")
    if bond_stereo_filter and not bond_stereo.has_expect:
        raise ValueError("bond_stereo_filter=True needs a BondStereo with expected kinds")


def score_bond_stereo(bond_stereo, aligned) -> dict:
    """redock(bond_stereo=): {"bond_stereo": state, dihedral, twist, n_wrong, n_twisted and ok of `BondStereo.check` of the kept poses}"""
    found = bond_stereo.check(aligned)
    return {"bond_stereo": {k: found[k] for k in ("state", "dihedral", "twist", "n_wrong", "n_twisted", "ok")}}
