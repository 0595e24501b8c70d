"""Build libg2vlm_hip.so (the C-ABI HIP library) in-tree with hipcc for gfx950.

hipcc cross-compiles without a GPU, so this runs in the CPU-only build container; the built
.so travels to the GPU box with the repo snapshot (it is git-ignored, not gpurun-ignored).

Each .hip source is compiled to its own object (in parallel, only when it or a header is newer
than the object) and the objects are linked into one shared library.
"""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "lib", "libg2vlm_hip.so")
OBJ = os.path.join(HERE, "lib", "obj")
SOURCES = ["gemm.hip", "gemm_big.hip", "gemm_8p.hip", "gemm_4w.hip", "gemm_skinny.hip", "attn.hip", "norm_rope.hip", "misc.hip", "decode.hip",
           "decode_layer.hip", "decode_batch.hip", "decode_shared.hip", "decode_fp8.hip", "decode_kv8.hip", "logprob.hip", "topk.hip", "cloud.hip",
           "voxel.hip", "consistency.hip", "render.hip", "mesh.hip", "nn.hip", "normals.hip"]


# per-source flags.  attn.hip: hipcc's SLP vectoriser packs neighbouring f32 adds / multiplies of the softmax into v_pk_*_f32,
# which cost an MFMA gap more than the two scalar instructions they replace (MI355X guide, cycle constants: 'packed f32 VALU')
FILE_FLAGS = {"attn.hip": ["-fno-slp-vectorize"]}


# kernels that OWN accumulation registers (asm statements name a-registers literally): their resource usage as hipcc reports it
# (-Rpass-analysis=kernel-resource-usage) is kept beside the object, for every instantiation of the shipped build;
# tests/test_build_cpu.py reads it (no scratch, the whole AGPR file allocated)
# decode_fp8.hip: the e4m3 GEMVs hold up to 12 rows of weights per lane; every instantiation must stay spill-free
# (tests/test_fp8_decode_cpu.py)
# decode_kv8.hip: the attention on an e4m3 cache holds a batch as codes AND as converted fragments; no scratch, <= 256 VGPRs
# (tests/test_kv8_cpu.py)
# logprob.hip: a lane holds 32 logits of a chunk between its max pass and its exp pass; no scratch (tests/test_score_cpu.py)
# topk.hip: a lane holds the 32 keys of a chunk through its selection rounds; no scratch (tests/test_score_questions_cpu.py)
RESOURCE_AUDIT = ("gemm_4w.hip", "attn.hip", "decode_fp8.hip", "decode_kv8.hip", "logprob.hip", "topk.hip")


def resources_path(src, objdir=None):
    return os.path.join(objdir or OBJ, src + ".resources.txt")


def _headers():
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(ROOT, "include", "g2vlm_hip.h")]


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(ROOT, "include", "g2vlm_hip.h")]
    return any(os.path.getmtime(d) > t for d in deps) or any(not os.path.exists(resources_path(f)) for f in RESOURCE_AUDIT)


COMM_SRC = os.path.join(HERE, "csrc_comm", "comm.cpp")
COMM_LIB = os.path.join(HERE, "lib", "libg2vlm_comm.so")


def build_comm(force=False, verbose=False):
    """libg2vlm_comm.so: the RCCL-backed collective entry points (include/g2vlm_comm.h).  Host code only."""
    hdr = os.path.join(ROOT, "include", "g2vlm_comm.h")
    if not force and os.path.exists(COMM_LIB) and os.path.getmtime(COMM_LIB) > max(os.path.getmtime(COMM_SRC), os.path.getmtime(hdr)):
        return COMM_LIB
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(os.path.dirname(COMM_LIB), exist_ok=True)
    cmd = [hipcc, "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), COMM_SRC, "-o", COMM_LIB + ".tmp",
           "-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath,/opt/rocm/lib"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    os.replace(COMM_LIB + ".tmp", COMM_LIB)
    return COMM_LIB


def build(force=False, verbose=False, extra_flags=(), out=None):
    """Compile every HIP source into one shared library.  Returns the library path.
    extra_flags / out: experiment builds (tools/attn_variants.sh), never the shipped library."""
    if out is not None:
        return _compile(list(extra_flags), out, verbose, force=True, objdir=out + ".obj")
    if not force and not _stale():
        return LIB
    return _compile([], LIB, verbose, force=force, objdir=OBJ)


def _compile(extra_flags, lib, verbose, force, objdir):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    os.makedirs(objdir, exist_ok=True)
    srcs = [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    hdr_t = max(os.path.getmtime(h) for h in _headers())
    # kernarg preload: the first 16 dwords of a kernel's arguments arrive in SGPRs with the wave instead of behind an s_load
    # round trip at its start (gfx940+; kernels keep a compatibility prologue).  -1.6 % on the ~170-launch decode step.
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-kernarg-preload-count=16", *extra_flags, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]

    def one(s):
        src, obj = os.path.join(CSRC, s), os.path.join(objdir, s + ".o")
        audit = s in RESOURCE_AUDIT
        if not force and os.path.exists(obj) and os.path.getmtime(obj) > max(os.path.getmtime(src), hdr_t) and \
                (not audit or os.path.exists(resources_path(s, objdir))):
            return obj
        cmd = base + FILE_FLAGS.get(s, []) + (["-Rpass-analysis=kernel-resource-usage"] if audit else []) + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        if audit:
            r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
            remarks = [ln for ln in r.stderr.splitlines() if "-Rpass-analysis=kernel-resource-usage" in ln]
            rest = [ln for ln in r.stderr.splitlines() if "-Rpass-analysis=kernel-resource-usage" not in ln]
            if r.returncode != 0:
                raise subprocess.CalledProcessError(r.returncode, cmd, stderr="\n".join(rest))
            with open(resources_path(s, objdir), "w") as f:
                f.write("\n".join(remarks) + "\n")
        else:
            subprocess.run(cmd, check=True)
        return obj

    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        objs = list(ex.map(one, srcs))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", lib + ".tmp"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    os.replace(lib + ".tmp", lib)
    return lib


if __name__ == "__main__":
    import sys
    print(build(force="--incremental" not in sys.argv, verbose=True))
    print(build_comm(force="--incremental" not in sys.argv, verbose=True))
