#!/usr/bin/env python
"""One SHA-256 per sampler call over a fixed list of calls on the small configuration (seeded weights, synthetic systems), as JSON:
run on two commits, the two outputs are equal exactly when no launch of the step loop changed.  The calls cover every tail branch
(align / device relaxation / host relaxation / plain), seeded and injected noise, eager, unit replay and the promoted whole-loop
graph, conditioning reuse, and a group of three systems (steps=6, p=1000: sigma = 2560, 310, 37.4, 4.50, 0.54, 0.064, so a
threshold factor 6.0 gives 3 align steps and 3 relax / plain steps).

    python tools/sampler_digest.py [--out digests.json]
"""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from physdock_amd import PhysDock, mmff  # noqa: E402
from physdock_amd.configs import small_config  # noqa: E402
from physdock_amd.model import karras_noise_schedule  # noqa: E402
from physdock_amd.params import param_shapes, seeded_state_dict  # noqa: E402
from physdock_amd.synthetic import make_batch, reference_conformers, small_batch  # noqa: E402


def to_dev(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def noise(B, steps, A, seed):
    g = torch.Generator().manual_seed(seed)
    n_noisy = int((karras_noise_schedule(steps, p=1000)[:-1] > 1.0).sum())
    return {"init": torch.randn(B, A, 3, generator=g), "rot_u": torch.rand(steps, 4, B, generator=g),
            "trans": torch.randn(steps, B, 3, generator=g), "diffuse": torch.randn(n_noisy, B, A, 3, generator=g)}


def device_terms(raw):
    lig = raw["is_ligand"][raw["atom_id_to_token_id"]].bool()
    return mmff.synthetic_terms(int(lig.sum()), 5, coords=raw["x_gt"][lig].double().numpy())[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = small_config()
    model = PhysDock(cfg)
    model.load_state_dict(seeded_state_dict(param_shapes(cfg), seed=0), strict=True)
    model = model.cuda().eval()
    digests = {}

    def put(name, xs):
        h = hashlib.sha256()
        for x in xs if isinstance(xs, (list, tuple)) else [xs]:
            assert torch.isfinite(x).all(), name
            h.update(x.detach().cpu().contiguous().numpy().tobytes())
        digests[name] = h.hexdigest()
        print(name, digests[name][:16], flush=True)

    raw = small_batch(0)
    b = to_dev(raw)
    A = b["ref_pos"].shape[0]
    kw = dict(num_sample=3, steps=6, karras_noise_schedule_power=1000)
    put("seeded eager", model.sample_diffusion(b, seed=5, sample_offset=2, use_graph=False, **kw))
    for call in ("first", "unit replay", "whole-loop graph"):
        put(f"seeded graph, {call}", model.sample_diffusion(b, seed=5, sample_offset=2, use_graph=True, **kw))
    nz = noise(3, 6, A, 11)
    for call in ("first", "replay"):
        put(f"noise graph, {call}", model.sample_diffusion(b, noise=nz, use_graph=True, **kw))
    pool = reference_conformers(raw, n_conf=4)
    tk = dict(kw, seed=5, align_ref_pos=True, ref_mol_poses=pool)
    put("align + plain, factor 6", model.sample_diffusion(b, mmff_gamma_0_factor=6.0, **tk))
    put("align + plain, factor 20 on the warm cache", model.sample_diffusion(b, mmff_gamma_0_factor=20.0, **tk))
    terms = device_terms(raw)
    put("align + device relax", model.sample_diffusion(b, mmff_gamma_0_factor=6.0, ref_mol=terms, **tk))
    put("align + host relax", model.sample_diffusion(b, mmff_gamma_0_factor=6.0, ref_mol=object(),
                                                     relax_fn=lambda mol, pos, iters: pos, **tk))
    x, cond = model.sample_diffusion(b, seed=7, return_conditioning=True, **kw)
    put("return_conditioning", x)
    put("conditioning=", model.sample_diffusion(b, seed=8, conditioning=cond, **kw))

    sizes = [(18, 5, 6), (14, 5, 4), (16, 5, 8)]
    raws = [make_batch(n, apr, nl, 8, seed=20 + i) for i, (n, apr, nl) in enumerate(sizes)]
    bs = [to_dev(r) for r in raws]
    gk = dict(num_sample=2, steps=6, karras_noise_schedule_power=1000, align_ref_pos=True)
    nzs = [noise(2, 6, r["ref_pos"].shape[0], 30 + i) for i, r in enumerate(raws)]
    put("group, noises=", model.sample_diffusion_many(bs, noises=nzs, **gk))
    pools = [reference_conformers(r, n_conf=4, seed=40 + i) for i, r in enumerate(raws)]
    pk = dict(gk, seeds=[1, 2, 3], ref_mol_poses=pools, mmff_gamma_0_factor=[6.0, 6.0, 3.0], ref_mol=[None, device_terms(raws[1]), None])
    for call in ("first", "replay"):
        put(f"group, seeded + pools + device relax, {call}", model.sample_diffusion_many(bs, **pk))

    text = json.dumps(digests, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
