"""pd_plif_fingerprint, pd_plif_compare and pd_plif_pairwise (csrc/plif.hip) straight on the C ABI, InteractionFingerprint, and the
interactions keyword of redock / redock_many.

The yardstick is the float64 restatement tests/plif_ref.py and its acceptance rule (its docstring): lo <= dev <= hi bit by bit for
`bits` and `ligand_bits`, where lo / hi are the fingerprints with every threshold lowered / raised by 1e-4 A; `counts` are the
popcounts of the device's own bits; `min_dist` lies within the derived rounding bound of the sqrtf / fmaf chain element by element,
with nothing multiplied on, and +inf matches exactly.  In every seeded case lo == hi (tests/test_plif_cpu.py asserts it on the CPU;
it is asserted again here), so the device must equal the restatement.  compare and pairwise are checked against integer numpy: the
int outputs exactly, the one fp32 division exactly or within 1 ulp.  Output buffers are one row longer than needed and pre-filled
with a sentinel (bytes 0xA5 - bit 7 is never set by the kernel -, NaN, -7777).

Case d has 66 poses: 66 = 4 * PAIR_TILE + 2 crosses the 16 x 16 tile of plif_pairwise_kernel, and the random rows of 257 and 300
bytes cross its 256-byte chunk."""
import ctypes

import numpy as np
import pytest
import torch

import plif_ref as ref

pytestmark = pytest.mark.gpu

PD_ERR_ARG, PD_ERR_UNSUPPORTED = -1, -3
NAN = float("nan")
BYTE, INT = 0xA5, -7777
CASE_A = "a_P3_A300_L5_R40"
OUT = ("bits", "ligand_bits", "min_dist", "counts")


# ------------------------------------------------------------------ sentinels, plumbing
def sentinel(shape, dtype):
    fill = {torch.uint8: BYTE, torch.int32: INT, torch.float32: NAN}[dtype]
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")


def untouched(buf):
    return bool(torch.isnan(buf).all()) if buf.dtype == torch.float32 else bool((buf == (BYTE if buf.dtype == torch.uint8 else INT)).all())


def body(buf):
    torch.cuda.synchronize()
    assert untouched(buf[-1]), "the row behind the output was written"
    head = buf[:-1]
    assert not (torch.isnan(head).any() if buf.dtype == torch.float32 else (head == (BYTE if buf.dtype == torch.uint8 else INT)).any()), \
        "an output element kept its sentinel"
    return head


@pytest.fixture(scope="module")
def L():
    from physdock_amd import ops
    return ops._lib.init()


def P(t):
    from physdock_amd import ops
    return ops.ptr(t)


def S():
    from physdock_amd import ops
    return ops.stream()


def thr(values):
    return (ctypes.c_float * 4)(*values)


def tables(c):
    """a case's tables on the device, every index the kernels would follow checked to be inside its array first"""
    A, R = c["x"].shape[1], int(c["n_residues"])
    start, atom = ref.csr(c)
    assert 0 <= c["lig_idx"].min() and c["lig_idx"].max() < A and len(c["types"]) == A == len(c["charges"]) == len(c["rec_mask"])
    assert len(c["lig_active"]) == len(c["lig_idx"]) <= 1024 and not c["rec_mask"][c["lig_idx"]].any() and 1 <= R <= A
    assert len(start) == R + 1 and start[0] == 0 and (np.diff(start) >= 0).all() and start[-1] == len(atom) <= A
    assert len(atom) == 0 or (0 <= atom.min() and atom.max() < A and len(set(atom.tolist())) == len(atom))
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()
    return dict(lig_idx=up(c["lig_idx"], np.int32), types=up(c["types"], np.uint8), charges=up(c["charges"], np.uint8),
                lig_active=up(c["lig_active"], np.uint8), res_start=up(start, np.int32), res_atom=up(atom, np.int32), N=len(atom))


def launch(L, x, c, d=None):
    """one pd_plif_fingerprint call into sentinel buffers -> dict of the bodies"""
    d = d or tables(c)
    x = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    n, A, Lg, R, N = x.shape[0], x.shape[1], len(c["lig_idx"]), int(c["n_residues"]), d["N"]
    assert A == len(c["types"])
    ws_bits, ws_min = sentinel((n, N), torch.uint8), sentinel((n, N), torch.float32)
    buf = dict(bits=sentinel((n, R), torch.uint8), ligand_bits=sentinel((n, Lg), torch.uint8), min_dist=sentinel((n, R), torch.float32),
               counts=sentinel((n, 6), torch.int32))
    rc = L.pd_plif_fingerprint(P(x), P(d["lig_idx"]), P(d["types"]), P(d["charges"]), P(d["lig_active"]), P(d["res_start"]), P(d["res_atom"]),
                               thr(c["thresholds"]), P(ws_bits), P(ws_min), P(buf["bits"]), P(buf["ligand_bits"]), P(buf["min_dist"]),
                               P(buf["counts"]), n, A, Lg, R, N, S())
    assert rc == 0, rc
    body(ws_bits), body(ws_min)                                        # the workspace: all of it written, nothing behind it
    return {k: body(v) for k, v in buf.items()}


def check(case, out, want):
    """the device against the restatement under the acceptance rule"""
    for k in ("bits", "ligand_bits"):
        dev, lo, hi = out[k].cpu().numpy(), want["lo"][k], want["hi"][k]
        assert dev.shape == lo.shape and dev.dtype == np.uint8, (case, k)
        assert not (lo & ~dev).any() and not (dev & ~hi).any(), (case, k, "lo <= dev <= hi fails in", int(((lo & ~dev) | (dev & ~hi) > 0).sum()), "bytes")
    bits = out["bits"].cpu().numpy()
    assert not (bits >> 6).any() and not (out["ligand_bits"].cpu().numpy() >> 6).any(), "bits 6 and 7 are always 0"
    assert np.array_equal(out["counts"].cpu().numpy(), ref.popcounts(bits)), (case, "counts are the popcounts of the device's own bits")
    dev, m, b = out["min_dist"].cpu().double().numpy(), want["min_dist"], want["bound"]
    assert np.array_equal(np.isinf(dev), np.isinf(m)) and (dev[np.isinf(dev)] > 0).all(), (case, "+inf must match exactly")
    fin = np.isfinite(m)
    err = np.abs(dev[fin] - m[fin])
    ratio = (err / b[fin]).max() if fin.any() else 0.0
    print(f"ENVELOPE | pd_plif_fingerprint | {case} min_dist | {m[fin].max():.2e} | {err.max():.2e} | {b[fin].max():.2e} | {ratio:.2f} |")
    assert (err <= b[fin]).all(), (case, "min_dist", err.max(), ratio)


def same(a, b, keys=None):
    return all(torch.equal(a[k], b[k]) for k in (keys or a))


# ------------------------------------------------------------------ cases a - d: the fingerprint
@pytest.mark.parametrize("name", list(ref.CASES))
def test_kernel_against_float64(L, name):
    c = ref.make_case(name)
    want = ref.restate(c)
    assert want["open_bytes"] == 0, "the case must leave no bit open"
    d = tables(c)
    out = launch(L, c["x"], c, d)
    check(name, out, want)
    assert np.array_equal(out["bits"].cpu().numpy(), want["lo"]["bits"]) and np.array_equal(out["ligand_bits"].cpu().numpy(), want["lo"]["ligand_bits"])
    n = c["x"].shape[0]
    # bit-identical from launch to launch
    assert same(launch(L, c["x"], c, d), out)
    # a pose fingerprinted alone is the pose inside the batch
    for p in sorted({0, 1, n // 2, n - 1}):
        one = launch(L, c["x"][p:p + 1], c, d)
        assert all(torch.equal(one[k][0], out[k][p]) for k in out), (name, p)
    # reversing the poses reverses the outputs
    rev = launch(L, c["x"][::-1], c, d)
    assert all(torch.equal(rev[k].flip(0), out[k]) for k in out), name
    # inactive ligand atoms report 0
    off = torch.from_numpy(c["lig_active"] == 0).cuda()
    assert not out["ligand_bits"][:, off].any()


def test_case_a_shows_and_misses_every_kind_and_has_empty_residues(L):
    c = ref.make_case(CASE_A)
    out = launch(L, c["x"], c)
    bits = out["bits"].cpu().numpy()
    for k in range(6):
        assert (bits >> k & 1).any() and not (bits >> k & 1).all(), ref.KIND_NAMES[k]
    start, _ = ref.csr(c)
    empty = np.diff(start) == 0
    assert empty.sum() >= 2 and np.isinf(out["min_dist"].cpu().numpy()[:, empty]).all() and not bits[:, empty].any()
    assert np.isfinite(out["min_dist"].cpu().numpy()[:, ~empty]).all()


def test_relabelling_two_equal_ligand_atoms_changes_nothing_on_the_residue_side(L):
    c = ref.make_case(CASE_A)
    i, k = 0, 4                                                        # both active; made equal in type and charge
    c["types"][c["lig_idx"][k]] = c["types"][c["lig_idx"][i]]
    c["charges"][c["lig_idx"][k]] = c["charges"][c["lig_idx"][i]]
    assert c["lig_active"][i] and c["lig_active"][k]
    out = launch(L, c["x"], c)
    swapped = dict(c, lig_idx=c["lig_idx"].copy())
    swapped["lig_idx"][[i, k]] = c["lig_idx"][[k, i]]
    new = launch(L, c["x"], swapped)
    assert same(new, out, ["bits", "min_dist", "counts"])
    perm = list(range(len(c["lig_idx"])))
    perm[i], perm[k] = k, i
    assert torch.equal(new["ligand_bits"], out["ligand_bits"][:, perm]) and out["ligand_bits"][:, [i, k]].any()
    check("relabelled", new, ref.restate(swapped))


def test_a_ligand_far_away_shows_nothing_and_keeps_finite_distances(L):
    c = ref.make_case(CASE_A)
    x = c["x"].copy()
    x[1, c["lig_idx"]] += np.float32([60.0, 0.0, 0.0])                # pose 1: the ligand 60 A away; poses 0 and 2 as they were
    want = ref.restate(c, x)
    assert want["open_bytes"] == 0 and not want["lo"]["bits"][1].any() and want["lo"]["bits"][0].any()
    out = launch(L, x, c)
    assert not out["bits"][1].any() and not out["ligand_bits"][1].any() and not out["counts"][1].any()
    start, _ = ref.csr(c)
    owned = torch.from_numpy(np.diff(start) > 0).cuda()
    assert torch.isfinite(out["min_dist"][1, owned]).all() and (out["min_dist"][1, owned] > 30).all()
    check("far ligand", out, want)
    base = launch(L, c["x"], c)
    assert same({k: v[[0, 2]] for k, v in out.items()}, {k: v[[0, 2]] for k, v in base.items()})


def test_thresholds_are_arguments(L):
    c = ref.make_case("b_P2_A65_L1_R3")
    for t in ((3.0, 5.0, 2.75, 6.0), (0.0, 0.0, 0.0, 0.0), (100.0, 100.0, 100.0, 100.0)):
        c2 = dict(c, thresholds=t)
        want = ref.restate(c2)
        assert want["open_bytes"] == 0
        check(f"thresholds {t}", launch(L, c["x"], c2), want)
    assert not launch(L, c["x"], dict(c, thresholds=(0.0,) * 4))["bits"].any()


# ------------------------------------------------------------------ compare, pairwise
def compare_dev(L, bits, ref_row, mask):
    n, R = bits.shape
    buf = dict(shared=sentinel((n,), torch.int32), n_pose=sentinel((n,), torch.int32), n_reference=sentinel((1,), torch.int32),
               recovery=sentinel((n,), torch.float32), tanimoto=sentinel((n,), torch.float32))
    rc = L.pd_plif_compare(P(bits), P(ref_row), mask, P(buf["shared"]), P(buf["n_pose"]), P(buf["n_reference"]), P(buf["recovery"]),
                           P(buf["tanimoto"]), n, R, S())
    assert rc == 0, rc
    return {k: body(v) for k, v in buf.items()}


def pairwise_dev(L, bits, mask):
    n, R = bits.shape
    buf = sentinel((n, n), torch.float32)
    assert L.pd_plif_pairwise(P(bits), mask, P(buf), n, R, S()) == 0
    return body(buf)


def within_one_ulp(dev, want):
    dev, want = np.asarray(dev, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return bool((np.abs(dev.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all())


def bit_rows(L):
    """the rows compare and pairwise are tested on: the device's bits of cases a and d, and random bytes whose rows cross the
    256-byte chunk of the pairwise kernel, with empty and full rows among them"""
    rows = {}
    for name in (CASE_A, "d_P66_A65_L2_R9"):
        c = ref.make_case(name)
        rows[name] = launch(L, c["x"], c)["bits"].contiguous()
    rng = np.random.default_rng(77)
    for n, R in ((33, 257), (66, 300)):
        b = (rng.integers(0, 64, (n, R)) & rng.integers(0, 64, (n, R))).astype(np.uint8)
        b[1], b[n - 1], b[5] = 0, 0, 63
        rows[f"random_P{n}_R{R}"] = torch.from_numpy(b).cuda()
    return rows


def test_compare_and_pairwise_against_integer_numpy(L):
    for name, bits in bit_rows(L).items():
        host = bits.cpu().numpy()
        n = host.shape[0]
        for mask in (63, 4 | 8 | 16 | 32, 1, 2):
            t = pairwise_dev(L, bits, mask)
            want_t = ref.pairwise(host, mask)
            assert torch.equal(t, t.T) and bool((t.diagonal() == 1.0).all()), (name, mask, "symmetric with a unit diagonal")
            assert within_one_ulp(t.cpu().numpy(), want_t), (name, mask)
            for p in sorted({0, 1, min(5, n - 1), n - 1}):
                out = compare_dev(L, bits, bits[p], mask)
                want = ref.compare(host, host[p], mask)
                for k in ("shared", "n_pose"):
                    assert np.array_equal(out[k].cpu().numpy(), want[k]), (name, mask, p, k)
                assert int(out["n_reference"][0]) == want["n_reference"]
                for k in ("recovery", "tanimoto"):
                    assert within_one_ulp(out[k].cpu().numpy(), want[k]), (name, mask, p, k)
                assert torch.equal(out["tanimoto"], t[p]), (name, mask, p, "compare against row p is row p of pairwise")
        zero = torch.zeros(host.shape[1], dtype=torch.uint8, device="cuda")
        out = compare_dev(L, bits, zero, 63)                           # an empty reference: recovery 1, tanimoto 1 only for an empty pose
        assert int(out["n_reference"][0]) == 0 and not out["shared"].any() and bool((out["recovery"] == 1.0).all())
        assert torch.equal(out["tanimoto"] == 1.0, out["n_pose"] == 0)


def test_pairwise_is_independent_of_the_batch(L):
    bits = bit_rows(L)["random_P66_R300"]
    full = pairwise_dev(L, bits, 63)
    assert torch.equal(pairwise_dev(L, bits, 63), full)
    sub = [3, 17, 40, 65]
    assert torch.equal(pairwise_dev(L, bits[sub].contiguous(), 63), full[sub][:, sub])
    assert torch.equal(pairwise_dev(L, bits.flip(0).contiguous(), 63), full.flip(0).flip(1))


# ------------------------------------------------------------------ argument handling
def test_fingerprint_argument_handling(L):
    c = ref.make_case("b_P2_A65_L1_R3")
    d = tables(c)
    x = torch.from_numpy(c["x"]).cuda()
    n, A, Lg, R, N = 2, 65, 1, 3, d["N"]
    bufs = [sentinel((n, N), torch.uint8), sentinel((n, N), torch.float32), sentinel((n, R), torch.uint8), sentinel((n, Lg), torch.uint8),
            sentinel((n, R), torch.float32), sentinel((n, 6), torch.int32)]
    names = ["x", "lig_idx", "type", "charge", "lig_active", "res_start", "res_atom", "thresholds", "ws_bits", "ws_min", "bits", "ligand_bits",
             "min_dist", "counts"]
    good = [P(x), P(d["lig_idx"]), P(d["types"]), P(d["charges"]), P(d["lig_active"]), P(d["res_start"]), P(d["res_atom"]), thr(c["thresholds"])] + \
           [P(b) for b in bufs]
    call = lambda args, sizes=(n, A, Lg, R, N): L.pd_plif_fingerprint(*args, *sizes, S())
    rcs = {}
    for k, name in enumerate(names):
        args = list(good)
        args[k] = None
        rcs["null " + name] = call(args)
    for k, name in enumerate(["P", "A", "L", "R", "N"]):
        for v in (0, -1):
            if name == "N" and v == 0:
                continue                                               # N = 0 is a receptor without atoms: valid
            sz = [n, A, Lg, R, N]
            sz[k] = v
            rcs[f"{name}={v}"] = call(good, sz)
    rcs["N>A"] = call(good, (n, A, Lg, R, A + 1))
    for k, name in enumerate(names):
        if name in ("x", "lig_idx", "res_start", "res_atom", "ws_min", "min_dist", "counts"):
            args = list(good)
            args[k] = good[k] + 2                                      # a float / int pointer off its 4-byte alignment
            rcs["misaligned " + name] = call(args)
    for k in range(4):
        for bad in (-1.0, NAN, float("inf"), -0.5e-30):
            t = list(c["thresholds"])
            t[k] = bad
            rcs[f"threshold {k} {bad}"] = call(good[:7] + [thr(t)] + good[8:])
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), rcs
    unsupported = {"L": call(good, (n, A, 1025, R, N)), "A": call(good, (n, (1 << 22) + 1, Lg, R, N)), "P": call(good, (65536, A, Lg, R, N)),
                   "R>A": call(good, (n, A, Lg, A + 1, N))}
    assert all(rc == PD_ERR_UNSUPPORTED for rc in unsupported.values()), unsupported
    torch.cuda.synchronize()
    assert all(untouched(b) for b in bufs), "a rejected call wrote"
    assert call(good) == 0
    for b in bufs:
        body(b)
    # a receptor without atoms: N = 0, the workspace and the list may be NULL; every residue is empty
    start0 = torch.zeros(R + 1, dtype=torch.int32, device="cuda")
    fresh = [sentinel((n, R), torch.uint8), sentinel((n, Lg), torch.uint8), sentinel((n, R), torch.float32), sentinel((n, 6), torch.int32)]
    assert L.pd_plif_fingerprint(*good[:5], P(start0), None, good[7], None, None, *[P(b) for b in fresh], n, A, Lg, R, 0, S()) == 0
    bits, lig_bits, md, counts = (body(b) for b in fresh)
    assert not bits.any() and not lig_bits.any() and not counts.any() and bool(torch.isinf(md).all())


def test_compare_and_pairwise_argument_handling(L):
    n, R = 3, 10
    bits = torch.zeros(n, R, dtype=torch.uint8, device="cuda")
    row = torch.zeros(R, dtype=torch.uint8, device="cuda")
    bufs = [sentinel((n,), torch.int32), sentinel((n,), torch.int32), sentinel((1,), torch.int32), sentinel((n,), torch.float32),
            sentinel((n,), torch.float32)]
    good = [P(bits), P(row), 63] + [P(b) for b in bufs]
    rcs = {}
    for k in range(len(good)):
        if k != 2:
            args = list(good)
            args[k] = None
            rcs[f"compare null {k}"] = L.pd_plif_compare(*args, n, R, S())
        if k > 2:
            args = list(good)
            args[k] = good[k] + 2
            rcs[f"compare misaligned {k}"] = L.pd_plif_compare(*args, n, R, S())
    for mask in (-1, 64):
        rcs[f"compare mask {mask}"] = L.pd_plif_compare(*good[:2], mask, *good[3:], n, R, S())
    for sz in ((0, R), (-1, R), (n, 0), (n, -1)):
        rcs[f"compare sizes {sz}"] = L.pd_plif_compare(*good, *sz, S())
    tan = sentinel((n, n), torch.float32)
    rcs["pairwise null bits"] = L.pd_plif_pairwise(None, 63, P(tan), n, R, S())
    rcs["pairwise null out"] = L.pd_plif_pairwise(P(bits), 63, None, n, R, S())
    rcs["pairwise misaligned"] = L.pd_plif_pairwise(P(bits), 63, P(tan) + 2, n, R, S())
    for mask in (-1, 64):
        rcs[f"pairwise mask {mask}"] = L.pd_plif_pairwise(P(bits), mask, P(tan), n, R, S())
    for sz in ((0, R), (-1, R), (n, 0), (n, -1)):
        rcs[f"pairwise sizes {sz}"] = L.pd_plif_pairwise(P(bits), 63, P(tan), *sz, S())
    assert all(rc == PD_ERR_ARG for rc in rcs.values()), rcs
    unsupported = {"compare P": L.pd_plif_compare(*good, 65536, R, S()), "compare R": L.pd_plif_compare(*good, n, (1 << 22) + 1, S()),
                   "pairwise P": L.pd_plif_pairwise(P(bits), 63, P(tan), 65536, R, S()),
                   "pairwise R": L.pd_plif_pairwise(P(bits), 63, P(tan), n, (1 << 22) + 1, S())}
    assert all(rc == PD_ERR_UNSUPPORTED for rc in unsupported.values()), unsupported
    torch.cuda.synchronize()
    assert all(untouched(b) for b in bufs + [tan]), "a rejected call wrote"
    assert L.pd_plif_compare(*good[:2], 0, *good[3:], n, R, S()) == 0 and L.pd_plif_pairwise(P(bits), 0, P(tan), n, R, S()) == 0
    assert bool((body(tan) == 1.0).all()) and bool((body(bufs[3]) == 1.0).all())          # no kind counts: everything agrees


# ------------------------------------------------------------------ InteractionFingerprint, graph capture
def fp_of(c, device="cuda"):
    from physdock_amd.interactions import InteractionFingerprint
    return InteractionFingerprint.from_types(c["types"], c["charges"], c["lig_idx"], c["rec_mask"], c["residue_of"], n_residues=c["n_residues"],
                                             ligand_active=c["lig_active"], thresholds=c["thresholds"], device=device)


def test_the_class_agrees_with_the_c_abi_and_captures_into_a_graph(L):
    c = ref.make_case(CASE_A)
    f = fp_of(c)
    x = torch.from_numpy(c["x"]).cuda()
    raw = launch(L, c["x"], c)
    out = f.fingerprint(x)
    assert set(out) == set(OUT) and all(t.is_cuda for t in out.values())
    assert out["bits"].dtype == out["ligand_bits"].dtype == torch.uint8 and out["min_dist"].dtype == torch.float32 and out["counts"].dtype == torch.int32
    assert out["bits"].shape == (3, 40) and out["ligand_bits"].shape == (3, 5) and out["min_dist"].shape == (3, 40) and out["counts"].shape == (3, 6)
    assert same(out, raw)
    # compare: a byte row, coordinates, kinds
    host = out["bits"].cpu().numpy()
    got = f.compare(out["bits"], out["bits"][1])
    want = ref.compare(host, host[1])
    assert set(got) == {"shared", "n_pose", "n_reference", "recovery", "tanimoto"} and got["n_reference"].shape == ()
    assert np.array_equal(got["shared"].cpu().numpy(), want["shared"]) and int(got["n_reference"]) == want["n_reference"]
    assert float(got["recovery"][1]) == 1.0 and float(got["tanimoto"][1]) == 1.0 and within_one_ulp(got["recovery"].cpu().numpy(), want["recovery"])
    by_x = f.compare(out["bits"], x[1])
    assert same(by_x, got) and same(f.compare(out["bits"], c["x"][1]), got) and same(f.compare(out["bits"], host[1]), got)
    specific = ("hbond_donor", "hbond_acceptor", "cationic", "anionic")
    sp = f.compare(out["bits"], x[1], kinds=specific)
    assert np.array_equal(sp["shared"].cpu().numpy(), ref.compare(host, host[1], 60)["shared"]) and int(sp["n_reference"]) < int(got["n_reference"])
    t = f.pairwise(out["bits"])
    assert t.shape == (3, 3) and torch.equal(t[1], got["tanimoto"]) and within_one_ulp(t.cpu().numpy(), ref.pairwise(host))
    assert within_one_ulp(f.pairwise(out["bits"], kinds=specific).cpu().numpy(), ref.pairwise(host, 60))
    # satisfies: what pose 0 shows is satisfied by pose 0; a kind a residue shows in no pose by none; nothing required by all
    shown = [(int(s), ref.KIND_NAMES[k]) for s in range(40) for k in range(6) if host[0, s] >> k & 1]
    ok = f.satisfies(out["bits"], shown)
    assert ok.dtype == torch.bool and ok.is_cuda and ok.shape == (3,) and bool(ok[0])
    assert ok.tolist() == [bool(((host[p] & host[0]) == host[0]).all()) for p in range(3)]
    s_free, k_free = next((s, k) for s in range(40) for k in range(6) if not (host[:, s] >> k & 1).any())
    assert f.satisfies(out["bits"], shown[:1] + [(s_free, ref.KIND_NAMES[k_free])]).tolist() == [False] * 3
    assert f.satisfies(out["bits"], []).tolist() == [True] * 3
    one = shown[0]
    assert f.satisfies(out["bits"], [one]).tolist() == [bool(host[p, one[0]] >> ref.KIND_NAMES.index(one[1]) & 1) for p in range(3)]
    assert f.describe(out["bits"][0]) == [(s, [ref.KIND_NAMES[k] for k in range(6) if host[0, s] >> k & 1]) for s in range(40) if host[0, s]]
    with pytest.raises(ValueError, match="pose atoms"):
        f.fingerprint(x[:, :-1])
    # capture, then replay on other coordinates
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    xs = x.clone()
    with torch.cuda.stream(s):
        f.fingerprint(xs)
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        captured = f.fingerprint(xs)
    xs.copy_(x.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(captured[k], out[k].flip(0)) for k in out)


# ------------------------------------------------------------------ redock, redock_many
@pytest.fixture(scope="module")
def small(small_model_inputs):
    from physdock_amd import PhysDock
    cfg, P_, batch = small_model_inputs
    model = PhysDock(cfg)
    model.load_state_dict(P_, strict=True)
    return model.cuda().eval(), {k: v.cuda() for k, v in batch.items()}, cfg


def same_result(a, b):
    """two redock results: the same keys, bit-equal tensors, equal everything else"""
    def eq(u, w):
        if isinstance(u, torch.Tensor):
            return isinstance(w, torch.Tensor) and torch.equal(u, w)
        if isinstance(u, dict):
            return isinstance(w, dict) and set(u) == set(w) and all(eq(u[k], w[k]) for k in u)
        return u == w
    return eq(a, b)


def test_redock_reports_the_fingerprint_and_changes_nothing_else(small):
    from physdock_amd import driver
    from physdock_amd.interactions import InteractionFingerprint
    from physdock_amd.validity import PoseValidity
    model, dbatch, _ = small
    bonds = [(i, i + 1) for i in range(int(driver.ligand_atom_mask(dbatch).sum()) - 1)]
    fp = InteractionFingerprint.from_batch(dbatch, bonds)
    validity = PoseValidity.from_batch(dbatch, bonds)
    kw = dict(num_samples_per_round=4, max_samples=4, steps=4, seed=3)
    plain = driver.redock(model, dbatch, **kw)
    assert same_result(plain, driver.redock(model, dbatch, **kw)), "the path without the keyword is deterministic"
    out = driver.redock(model, dbatch, interactions=fp, **kw)
    assert "x_gt" in dbatch and set(out) == set(plain) | {"interactions", "interaction_recovery"}
    assert same_result({k: out[k] for k in plain}, plain)
    assert set(out["interactions"]) == set(OUT) and out["interactions"]["bits"].shape == (4, fp.n_residues)
    assert same(out["interactions"], fp.fingerprint(out["poses"]))
    assert same(out["interaction_recovery"], fp.compare(out["interactions"]["bits"], dbatch["x_gt"].float()))
    assert set(out["interaction_recovery"]) == {"shared", "n_pose", "n_reference", "recovery", "tanimoto"}
    # the kept poses against the restatement
    host = dict(x=out["poses"].cpu().numpy(), lig_idx=fp.ligand_idx, types=fp.types, charges=fp.charges, lig_active=fp.lig_active,
                rec_mask=fp.rec_mask, residue_of=fp.residue_of, n_residues=fp.n_residues, thresholds=fp.threshold_values)
    check("redock poses", out["interactions"], ref.restate(host))
    both = driver.redock(model, dbatch, interactions=fp, validity=validity, **kw)
    assert set(both) == set(plain) | {"interactions", "interaction_recovery", "validity"}
    assert same(both["interactions"], out["interactions"]) and same(both["interaction_recovery"], out["interaction_recovery"])
    assert same_result(both["validity"], driver.redock(model, dbatch, validity=validity, **kw)["validity"])
    many = driver.redock_many(model, [(dbatch, {"interactions": fp})], **kw)         # one system: the sequential path
    assert same_result(many[0], out)
    grouped = driver.redock_many(model, [(dbatch, {"interactions": fp})], group=1, **kw)
    assert set(grouped[0]) == set(out) and same(grouped[0]["interactions"], fp.fingerprint(grouped[0]["poses"]))
    assert same(grouped[0]["interaction_recovery"], fp.compare(grouped[0]["interactions"]["bits"], dbatch["x_gt"].float()))
