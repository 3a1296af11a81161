"""Generate tests/golden/g18_metrics_*.npz from the UNMODIFIED reference (PhysDock/data/tools/get_metrics.py: get_metrics and, per
pose, get_has_clash), imported read-only.

    python tools/make_golden_metrics.py --ref /path/to/reference [--only small,mid]

Per fixture: the features (s_mask, asym_id, a_mask, atom_id_to_token_id, is_ligand as bool) and x_pred; the logits are rebuilt
from an integer hash (physdock_amd.synthetic.metrics_case) and pinned by checksums.  Per quantity q in atom_plddts, mean_plddt,
pae, ptm, iptm, ranking_confidence: `ref_q` (the reference; one call per logit set where the case stacks P of them), `f64_q` (a
float64 numpy evaluation of the same formulas on the fp32 logits, synthetic.metrics_eval) and `e32_q` = max |plain fp32 numpy
evaluation - f64_q|.  pae is stored on the rows `pae_rows` (all rows where they fit, else a stride) with `sum_f64_pae` = [sum,
sum of squares] over the full array.  Decisions: `f64_rows` [P,2] (the argmax rows of pTM / ipTM) with `f64_gaps` (top two of
per_alignment_i w_i), `ref_has_clash` [B] (the reference's get_has_clash per pose), `f64_has_clash_skip` [B] (the loop restated
over a < b), `n_clash` [B,n,n] / `n_atoms` [n] and `closest_clash`.  The clash case also stores `a_mask_pose` [B,A] with
`ref_has_clash_pose` / `f64_has_clash_pose_skip` (pose b under its own mask; see synthetic.metrics_case).

Conditions asserted here (not measurements): the argmax gaps are >= 1e-4; no eligible inter-chain distance lies within 1e-4 A of
1.1; a fractional sum of s_mask is >= 1e-3 from an integer; |ref - f64| <= max(4 e32, 8 ulp32(max |f64|)) for every quantity, so
that the tests' tolerance is not looser than the reference itself needs; the float64 decisions equal the reference's.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")
QUANTITIES = ("atom_plddts", "mean_plddt", "pae", "ptm", "iptm", "ranking_confidence")
MAX_BYTES = 288475                  # the largest g17_* fixture
MAX_PAE_ROWS = 32


def bound(e32, f64):
    return max(4 * e32, 8 * float(np.spacing(np.float32(np.abs(f64).max()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("PHYSDOCK_REFERENCE"), required="PHYSDOCK_REFERENCE" not in os.environ,
                    help="checkout of the reference (or set PHYSDOCK_REFERENCE)")
    from physdock_amd.synthetic import (CLASH_MARGIN, FRAC_MARGIN, METRICS_CASES, METRICS_FEAT_KEYS, METRICS_STACKED, TM_GAP, metrics_case,
                                        metrics_eval)
    ap.add_argument("--only", default=",".join(METRICS_CASES))
    args = ap.parse_args()
    import tools.make_golden as mg
    mg.REF = args.ref
    mg.install_shims()
    import PhysDock.data.tools.get_metrics as RM
    for name in args.only.split(","):
        o, f, info = metrics_case(name)
        on, fn = {k: v.numpy() for k, v in o.items()}, {k: v.numpy() for k, v in f.items()}
        P, B, T = METRICS_STACKED.get(name), on["x_pred"].shape[0], fn["s_mask"].shape[0]
        # ---- the reference: get_metrics per logit set (it scores pose 0 of the x_pred it is given), get_has_clash per pose
        unused = {k: torch.zeros(T) for k in ("is_protein", "is_dna", "is_rna")}          # read by the reference, never used
        sets = [(o["p_plddt"], o["p_pae"], o["x_pred"])] if P is None else [(o["p_plddt"][p], o["p_pae"][p], o["x_pred"][p:p + 1]) for p in range(P)]
        refs = [RM.get_metrics({"p_plddt": a, "p_pae": b, "x_pred": c}, {**f, **unused}) for a, b, c in sets]
        ref = {k: np.concatenate([r[k].numpy() for r in refs]) for k in refs[0]}
        a2t = fn["atom_id_to_token_id"]
        def ref_clash(b, mask):
            return int(RM.get_has_clash(on["x_pred"][b], mask, fn["asym_id"][a2t], ~fn["is_ligand"][a2t]))
        ref_has = np.asarray([ref_clash(b, fn["a_mask"]) for b in range(B)], np.int64)
        # ---- float64 and plain fp32 restatements
        e64, e64s, e32 = metrics_eval(on, fn, np.float64), metrics_eval(on, fn, np.float64, skip_self_pairs=True), metrics_eval(on, fn, np.float32)
        assert e64["gaps"].min() >= TM_GAP or name == "onechain", (name, e64["gaps"])
        if name == "onechain":
            assert e64["gaps"][:, 0].min() >= TM_GAP and (e64["iptm"] == 0).all() and (e64["rows"][:, 1] == 0).all()
        assert e64["closest"] > CLASH_MARGIN, (name, e64["closest"])     # by construction: pairs are 0.4 - 0.6 A or more than 1.8 A apart
        sw = float(fn["s_mask"].astype(np.float64).sum())
        if (fn["s_mask"] % 1 != 0).any():
            assert abs(sw - round(sw)) >= FRAC_MARGIN, sw
        assert (e32["rows"] == e64["rows"]).all() and (e32["has_clash"] == e64["has_clash"]).all()
        nposes = len(ref["has_clash"])
        assert (ref["has_clash"] == ref_has[:nposes]).all() and (e64["has_clash"] == ref_has).all(), (name, ref_has, e64["has_clash"])
        rows = np.arange(T) if T <= MAX_PAE_ROWS else np.arange(0, T, (T // 10) | 1)
        arrays = {"case": np.array(name), "x_pred": on["x_pred"], "pae_rows": rows, "sum_w": np.float64(sw),
                  "f64_rows": e64["rows"].astype(np.int64), "f64_gaps": e64["gaps"], "ref_has_clash": ref_has,
                  "f64_has_clash_skip": e64s["has_clash"], "n_clash": e64["n_clash"].astype(np.int64), "n_atoms": e64["n_atoms"].astype(np.int64),
                  "closest_clash": np.float64(e64["closest"]),
                  "sum_f64_pae": np.array([e64["pae"].sum(), (e64["pae"] ** 2).sum()])}
        for k in METRICS_FEAT_KEYS:
            arrays[k] = fn[k]
        for k in ("p_plddt", "p_pae"):
            v = on[k].astype(np.float64)
            arrays["checksum_" + k] = np.array([v.sum(), (v ** 2).sum()])
        print(f"g18_metrics_{name}: T {T} A {a2t.shape[0]} B {B} P {P}; sum w {sw:.6f}; rows {e64['rows'].tolist()} gaps {e64['gaps'].min():.2e}; "
              f"has_clash ref {ref_has.tolist()} a<b {e64s['has_clash'].tolist()}; closest approach to 1.1: {e64['closest']:.3f}")
        for q in QUANTITIES:
            r, v64, v32 = np.asarray(ref[q]), e64[q], e32[q]
            if q == "ranking_confidence":
                v64, v32 = v64[:len(r)], v32[:len(r)]
            assert r.shape == v64.shape, (q, r.shape, v64.shape)
            err32 = float(np.abs(v32.astype(np.float64) - v64).max())
            dref = float(np.abs(r.astype(np.float64) - v64).max())
            print(f"    {q:18s} dtype {r.dtype}  max|f64| {np.abs(v64).max():.6g}  e32 {err32:.3e}  |ref - f64| {dref:.3e}  bound {bound(err32, v64):.3e}")
            assert dref <= bound(err32, v64), (name, q, dref, bound(err32, v64))
            if q == "pae":
                r, v64 = r[:, rows], v64[:, rows]
            arrays["ref_" + q], arrays["f64_" + q], arrays["e32_" + q] = r, v64, np.float64(err32)
        if name == "chains3":
            assert ref_has.all() and not e64s["has_clash"].any()         # the self-pair quirk: well-separated chains, has_clash = 1
        if name == "clash":
            masks = info["a_mask_pose"]
            per = [metrics_eval(on, fn, np.float64, a_mask=masks[b]) for b in range(B)]
            pers = [metrics_eval(on, fn, np.float64, a_mask=masks[b], skip_self_pairs=True) for b in range(B)]
            arrays["a_mask_pose"] = masks
            arrays["ref_has_clash_pose"] = np.asarray([ref_clash(b, masks[b]) for b in range(B)], np.int64)
            arrays["f64_has_clash_pose_skip"] = np.asarray([pers[b]["has_clash"][b] for b in range(B)], np.int64)
            arrays["n_clash_pose"] = np.asarray([per[b]["n_clash"][b, 0, 1] for b in range(B)], np.int64)
            arrays["n_min_pose"] = np.asarray([per[b]["n_atoms"].min() for b in range(B)], np.int64)
            assert all(per[b]["closest"] > CLASH_MARGIN for b in range(B))
            assert arrays["n_clash_pose"].tolist() == [0, 80, 101, 100, 0] and arrays["n_min_pose"].tolist() == [202, 150, 202, 200, 202]
            assert arrays["ref_has_clash_pose"].tolist() == [0, 1, 1, 0, 0] == [int(per[b]["has_clash"][b]) for b in range(B)]
            assert ref_has.tolist() == [0, 0, 1, 0, 0]
            print(f"    per-pose masks: n_clash {arrays['n_clash_pose'].tolist()} min {arrays['n_min_pose'].tolist()} "
                  f"has_clash {arrays['ref_has_clash_pose'].tolist()}")
        path = os.path.join(OUT, f"g18_metrics_{name}.npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < MAX_BYTES, os.path.getsize(path)
        print(f"    wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
