"""Build libphysdock_hip.so (hipcc, gfx950 only) in-tree next to this file."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
LIB = os.path.join(HERE, "libphysdock_hip.so")


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = sources() + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    deps += [os.path.join(INCLUDE, f) for f in os.listdir(INCLUDE)]
    return any(os.path.getmtime(d) > t for d in deps)


#: No packed-fp32 VALU anywhere (v_pk_add / mul / fma_f32).  hipcc (ROCm 7.2) forms them both in the SLP vectoriser and when it
#: lowers explicit float2 / float4 arithmetic; on MI355X a packed op that reads a register pair a global_load has just returned
#: intermittently sees stale data in lanes 48-63 (the last pass of the wave) - whole output rows with (row % 8) in {6, 7} off
#: by O(1).  Timing decides: on an otherwise idle GPU the fp32 kernels never showed it (every parity test passed bit-
#: reproducibly), the first split GEMM did in multi-tile blocks (NOTES.md "staging hazard"), and with a second kernel stream on
#: the same CUs the generic GEMM with a norm prologue did in 1 of 2 launches (tools/concurrent_gemm_stress.py KIND=normproj:
#: 146 of 300 launches wrong; 0 of 300 with this flag set).  -fno-slp-vectorize alone leaves the ops that come from vector
#: types; disabling the target feature removes them all (the host pass prints "not a recognized feature", harmless).
#: Scalar f32 VALU is also what the CDNA guide recommends beside MFMAs.
#: tests/test_gemm_split_gpu.py::test_split_multi_tile_stress and tests/test_concurrent_streams_gpu.py guard it.
NO_PACKED_F32 = ["-fno-slp-vectorize", "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
#: attn_pipe.hip: fmaxf without the sNaN-quieting v_max_f32 x, x in front of every operand (no NaN can enter the running maximum:
#: scores are finite or -inf); infinities stay honoured (-inf masks, the initial maximum)
EXTRA_FLAGS = {"attn_pipe.hip": ["-fno-honor-nans"]}


def compile_cmd(src, out, mode=("-c",)):
    """the hipcc command line of one source file (shared by build() and the device-assembly check in
    tests/test_build_rules_cpu.py, which passes mode=("-S", "--cuda-device-only"))"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    base = os.path.basename(src)
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
           "-Wno-unused-result", "-I", INCLUDE, "-I", CSRC, *mode, src, "-o", out]
    if os.environ.get("PD_NO_EXTRA_FLAGS") != "1":
        cmd[1:1] = NO_PACKED_F32
    if os.environ.get("PD_LAB"):          # lab build: in-kernel phase traces (never shipped)
        cmd[1:1] = ["-DPD_LAB=1"]
    if os.environ.get("PD_NO_EXTRA_FLAGS") != "1":
        cmd[1:1] = EXTRA_FLAGS.get(base, [])
    return cmd


def build(force=False, verbose=True, only=None):
    """only: names of the sources to recompile (the other objects of the last full build are reused)"""
    if not force and not only and not needs_build():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    procs = []
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    for src in sources():
        obj = os.path.join(HERE, "build", os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        if only and os.path.basename(src) not in only and os.path.exists(obj):
            continue
        procs.append((src, subprocess.Popen(compile_cmd(src, obj), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, pr in procs:
        out, _ = pr.communicate()
        if pr.returncode != 0:
            sys.stderr.write(out.decode())
            raise RuntimeError(f"hipcc failed on {src}")
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    subprocess.check_call(cmd)
    if verbose:
        print(f"built {LIB}")
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, only=[a for a in sys.argv[1:] if a.endswith(".hip")] or None)
