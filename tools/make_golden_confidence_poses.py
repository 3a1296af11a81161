"""Generate tests/golden/g19_confidence_poses_{small,ragged}.npz from the UNMODIFIED reference, imported read-only: its
ConfidenceModule (PhysDock/models/layers/confidence_module.py) run once per pose on x_pred[p:p+1] - the module reads pose 0 only -
and its get_metrics (PhysDock/data/tools/get_metrics.py) on each result.

    python tools/make_golden_confidence_poses.py --ref /path/to/reference [--only small,ragged]

The system, s / z and the poses are rebuilt by physdock_amd.synthetic.confidence_poses_case (x_pred and the metrics' features are
stored as well); the weights are synthetic.confidence_poses_weights: G12's seeded ones with linear_d scaled up.  Per fixture:
* logits, as G12 stores them: p_plddt [P,A,50] in full, p_pae / p_pde on the rows and columns `rows` ([P,R,R,64]; all of them
  where they fit) with `pae_sum` / `pde_sum` [P] (float64 sums of the full tensors), `logit_max` (largest |logit| of p_pae), `bins`
  [P,T,T] (uint8: the centre-distance bin of every token pair, the reference's argmin);
* per quantity q in ptm, iptm, mean_plddt, atom_plddts, ranking_confidence: `ref_q` [P,..] (the reference), `f64_q` (the whole path
  in float64: the oracle's module on float64 weights and inputs, then synthetic.metrics_eval) and `e32_q` = max |ref_q - f64_q|,
  what the reference's own fp32 evaluation of the same inputs costs; `ref_has_clash` [P];
* `order`: the poses best first (descending ranking_confidence, then mean_plddt, then index) and `min_gap`, `gap_needed`.

Conditions asserted here: across the poses the centre distances hit all 13 bins; no centre distance lies within 1e-4 A of a bin
midpoint; no eligible inter-chain distance lies within 1e-4 A of 1.1; the reference's ranking_confidence values differ pairwise by
at least `gap_needed` = 10 x the largest change of the reference's ranking_confidence when every p_pae logit moves by d = 2e-4 max
|p_pae logit| in the direction that changes the score most - the TM term falls with the error bin, so an expectation of it moves
most under +d on the bins below a threshold and -d on the others; every threshold and both signs are tried, for every pose (the
rigorous bound exp(2 d) - 1 of a [0, 1] expectation is ten times looser than anything this finds); has_clash of the last pose is 1 and of the others 0; the float64 decisions equal the reference's.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
OUT = os.path.join(ROOT, "tests", "golden")
QUANTITIES = ("ptm", "iptm", "mean_plddt", "atom_plddts", "ranking_confidence")
MAX_BYTES = 900 * 1024
MAX_ROWS = 24
TOL = 2e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("PHYSDOCK_REFERENCE"), required="PHYSDOCK_REFERENCE" not in os.environ,
                    help="checkout of the reference (or set PHYSDOCK_REFERENCE)")
    from physdock_amd.synthetic import (CLASH_MARGIN, CONF_POSES_CASES, CONF_POSES_FEAT_KEYS, confidence_poses_case, confidence_poses_weights,
                                        metrics_eval)
    ap.add_argument("--only", default=",".join(CONF_POSES_CASES))
    args = ap.parse_args()
    import tools.make_golden as mg
    mg.REF = args.ref
    mg.install_shims()
    import PhysDock.data.tools.get_metrics as RM
    from PhysDock.models.layers.confidence_module import ConfidenceModule as RefConfidence
    import physdock_oracle as orc
    for name in args.only.split(","):
        cm, batch, inp = confidence_poses_case(name)
        sd = confidence_poses_weights(cm)
        mod = RefConfidence(**cm)
        mod.load_state_dict(sd, strict=True)
        mod.eval()
        x = inp["x_pred"]
        P, A, T = x.shape[0], x.shape[1], inp["s"].shape[0]
        feats = {k: batch[k] for k in CONF_POSES_FEAT_KEYS}
        fn = {k: v.numpy() for k, v in feats.items()}
        unused = {k: torch.zeros(T) for k in ("is_protein", "is_dna", "is_rna")}          # read by the reference, never used
        # ---- the reference, pose by pose; the same path in float64
        P64 = {"confidence_module." + k: v.double() for k, v in sd.items()}
        b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
        ref_l, refs, f64s = [], [], []
        for p in range(P):
            with torch.no_grad():
                pae, pde, plddt = mod(batch, inp["s"], inp["z"], x[p:p + 1])
                l64 = orc.confidence_module(P64, b64, inp["s"].double(), inp["z"].double(), x[p:p + 1].double(), cm["inf"], cm["eps"])
            for got, want in zip((pae, pde, plddt), l64):
                assert want.dtype == torch.float64 and float((got.double() - want).abs().max() / want.abs().max()) < 2e-5
            ref_l.append((pae, pde, plddt))
            refs.append(RM.get_metrics({"p_plddt": plddt, "p_pae": pae, "x_pred": x[p:p + 1]}, {**feats, **unused}))
            f64s.append(metrics_eval({"p_plddt": l64[2].numpy(), "p_pae": l64[0].numpy(), "x_pred": x[p:p + 1].numpy()}, fn, np.float64))
        ref = {k: np.concatenate([np.asarray(r[k]) for r in refs]) for k in refs[0]}
        f64 = {k: np.concatenate([np.asarray(r[k]) for r in f64s]) for k in QUANTITIES + ("has_clash",)}
        # ---- conditions
        ctr = inp["token_id_to_centre_atom_id"]
        v = torch.linspace(3.375, 24.375, 13)
        xc = x[:, ctr]
        d = torch.norm(xc[:, :, None] - xc[:, None], dim=-1)
        bins = (d[..., None] - v).abs().argmin(-1)
        assert len(torch.unique(bins)) == 13, torch.unique(bins).tolist()
        mid = float((d.double()[..., None] - (v[:-1] + 0.875).double()).abs().min())
        assert mid > 1e-4, mid
        closest = min(r["closest"] for r in f64s)
        assert closest > CLASH_MARGIN, closest
        assert ref["has_clash"].tolist() == [0] * (P - 1) + [1] == f64["has_clash"].tolist(), ref["has_clash"]
        logit_max = max(float(l[0].abs().max()) for l in ref_l)
        delta = TOL * logit_max
        k = torch.arange(64)
        worst = 0.0
        for p in range(P):
            base = float(refs[p]["ranking_confidence"][0])
            for kk in range(1, 64):
                for sign in (1.0, -1.0):
                    eps = sign * delta * torch.where(k < kk, 1.0, -1.0)
                    r = RM.get_metrics({"p_plddt": ref_l[p][2], "p_pae": ref_l[p][0] + eps, "x_pred": x[p:p + 1]}, {**feats, **unused})
                    worst = max(worst, abs(float(r["ranking_confidence"][0]) - base))
        gap_needed = 10 * worst
        rc = ref["ranking_confidence"].astype(np.float64)
        min_gap = min(abs(rc[i] - rc[j]) for i in range(P) for j in range(i))
        print(f"g19_confidence_poses_{name}: T {T} A {A} P {P}; max |pae logit| {logit_max:.3f}; ranking_confidence {rc.tolist()}; "
              f"min gap {min_gap:.3e} needed {gap_needed:.3e}; nearest bin midpoint {mid:.2e}; closest approach to 1.1: {closest:.3f}")
        assert min_gap >= gap_needed, (min_gap, gap_needed)
        order = sorted(range(P), key=lambda i: (-rc[i], -float(ref["mean_plddt"][i]), i))
        assert order == sorted(range(P), key=lambda i: (-f64["ranking_confidence"][i], -f64["mean_plddt"][i], i))
        rows = np.arange(T) if T <= MAX_ROWS else np.arange(0, T, -(-T // MAX_ROWS))
        sel = torch.from_numpy(rows)
        arrays = {"case": np.array(name), "x_pred": x.numpy(), "rows": rows, "bins": bins.numpy().astype(np.uint8),
                  "p_plddt": torch.stack([l[2] for l in ref_l]).numpy(),
                  "p_pae": torch.stack([l[0][sel][:, sel] for l in ref_l]).numpy(),
                  "p_pde": torch.stack([l[1][sel][:, sel] for l in ref_l]).numpy(),
                  "pae_sum": np.array([float(l[0].double().sum()) for l in ref_l]), "pde_sum": np.array([float(l[1].double().sum()) for l in ref_l]),
                  "logit_max": np.float64(logit_max), "ref_has_clash": ref["has_clash"].astype(np.int64), "order": np.asarray(order, np.int64),
                  "min_gap": np.float64(min_gap), "gap_needed": np.float64(gap_needed), "closest_clash": np.float64(closest)}
        for k in CONF_POSES_FEAT_KEYS:
            arrays[k] = fn[k]
        for q in QUANTITIES:
            r, v64 = np.asarray(ref[q]).astype(np.float64).reshape(f64[q].shape), f64[q]
            arrays["ref_" + q], arrays["f64_" + q], arrays["e32_" + q] = np.asarray(ref[q]).reshape(f64[q].shape), v64, np.float64(np.abs(r - v64).max())
            print(f"    {q:18s} max|f64| {np.abs(v64).max():.6g}  e32 = |ref - f64| {float(arrays['e32_' + q]):.3e}")
        path = os.path.join(OUT, f"g19_confidence_poses_{name}.npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < MAX_BYTES, os.path.getsize(path)
        print(f"    wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
