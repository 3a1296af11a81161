"""Time of one LddtPli.score call at P = 64, A = 2048, L = 44, M = 4096 beside ranking.pairwise_ligand_rmsd with the same symmetry
table (NOTES.md, lDDT-PLI section): a synthetic crop of the cfg1 atom count with a 44-atom ligand, a table of twelve independent pair
swaps (2^12 rows), windows between device events after 20 warm-up calls, the two calls alternating.  Prints one JSON line."""
import itertools, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physdock_amd import LddtPli, LigandSymmetry
from physdock_amd.driver import ligand_atom_mask
from physdock_amd.ranking import pairwise_ligand_rmsd
from physdock_amd.synthetic import make_batch

batch = {k: v.cuda() for k, v in make_batch(334, 6, 44, 8, 0).items()}
A = batch["x_gt"].shape[0]
lig = torch.nonzero(ligand_atom_mask(batch)).flatten().to(torch.int32)
L = int(lig.numel())
assert (A, L) == (2048, 44), (A, L)
rows = []
for bits in itertools.product((0, 1), repeat=12):                 # twelve independent swaps of atom pairs: 2^12 rows, identity first
    p = list(range(L))
    for k, b in enumerate(bits):
        if b:
            p[2 * k], p[2 * k + 1] = p[2 * k + 1], p[2 * k]
    rows.append(p)
sym = LigandSymmetry.from_permutations(rows)
obj = LddtPli.from_batch(batch, sym)
g = torch.Generator().manual_seed(1)
x = (batch["x_gt"].float().cpu()[None] + 0.7 * torch.randn(64, A, 3, generator=g)).cuda()
x_gt = batch["x_gt"].float()

def timed(fn, reps):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return out

res = {"P": 64, "A": A, "L": L, "M": sym.n_perms, "n_contacts": obj.n_contacts, "n_candidates": obj.n_candidates}
a, b = [], []
for rnd in range(3):                                              # alternate the two, five windows each per round
    a += timed(lambda: obj.score(x), 2000)
    b += timed(lambda: pairwise_ligand_rmsd(x, lig, x_gt, symmetry=sym), 200)
res["score_us"] = [round(v, 2) for v in a]
res["sym_rmsd_us"] = [round(v, 2) for v in b]
res["score_us_median"], res["sym_rmsd_us_median"] = float(np.median(a)), float(np.median(b))
sc = obj.score(x)
res["lddt_mean"] = float(sc["lddt_pli"].mean())
print(json.dumps(res))
