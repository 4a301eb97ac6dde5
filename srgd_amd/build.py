"""Build the engine ``libsrgd_hip.so`` (C ABI: include/srgd_hip.h) and the ten extension libraries beside it (``libsrgd_<name>.so``,
include/srgd_<name>.h) in-tree with hipcc for gfx950: one row of ``LIBRARIES`` per library.

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting
``srgd_amd/libsrgd_hip.so`` travels to the GPU box with the tree (git-ignored, not
gpurun-ignored).  ``python -m srgd_amd.build`` or ``__graft_entry__.build()``.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ_DIR = os.path.join(HERE, "build")
# resize.hip's host code reproduces Pillow's double-precision tables: no fused multiply-adds in it (its kernels are integer code);
# threshold.hip's definition is in separate fp32 multiplications and additions, on the host and in its kernels
EXTRA_FLAGS = {"resize.hip": ["-ffp-contract=off"], "threshold.hip": ["-ffp-contract=off"]}
SOURCES = ["conv_igemm.hip", "conv3x3_bf16.hip", "conv3x3_split.hip", "conv3x3_mx2.hip", "conv1x1_split.hip", "conv1x1_bf16.hip", "conv3x3_mxfp8.hip", "conv1x1_mxfp8.hip", "quant_mxfp8.hip", "norm_act.hip", "attention.hip", "linattn_fused.hip", "linattn_fused256.hip", "cond.hip", "sampler.hip", "imageio.hip", "engine.hip", "kernel_api.hip"]
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value",
         "-fno-gpu-rdc", "-DNDEBUG", "-fvisibility=hidden"]
# one row per library: (name, .so path, sources, export pattern of the version script) - the engine first, every source in one row
LIBRARIES = [(name, os.path.join(HERE, f"libsrgd_{name}.so"), sources, pattern) for name, sources, pattern in (
             ("hip", SOURCES, "srgd_*"),
             ("metrics", ["metrics.hip"], "srgd_image_metrics*"),
             ("ensemble", ["ensemble.hip"], "srgd_image_ensemble*"),
             ("consistency", ["consistency.hip"], "srgd_image_consistency*"),
             ("backproject", ["backproject.hip"], "srgd_image_backproject*"),
             ("guidance", ["guidance.hip"], "srgd_guidance*"),
             ("solver", ["solver.hip"], "srgd_solver*"),
             ("resize", ["resize.hip"], "srgd_resize*"),
             ("alpha", ["alpha.hip"], "srgd_alpha*"),
             ("threshold", ["threshold.hip"], "srgd_threshold*"),
             ("selfens", ["selfens.hip"], "srgd_selfens*"))]
LIB = LIBRARIES[0][1]


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the MI355X engine cannot be built (there is no CPU fallback)")


def _digest() -> str:
    h = hashlib.sha256()
    for root in (CSRC, os.path.join(os.path.dirname(HERE), "include")):
        for name in sorted(os.listdir(root)):
            with open(os.path.join(root, name), "rb") as f:
                h.update(name.encode())
                h.update(f.read())
    h.update(" ".join(FLAGS).encode())
    h.update(repr(sorted(EXTRA_FLAGS.items())).encode())
    h.update(b"version-script:srgd_*")
    return h.hexdigest()


def link(hipcc: str, out: str, objs: list, pattern: str, vers: str) -> None:
    """Link ``objs`` into the shared library ``out`` behind the version script ``vers``: the dynamic symbol table holds the C ABI
    (``pattern``) and nothing else - without it the weak template instantiations of libstdc++ types (default visibility by the
    standard library's own attribute) leak out as exports."""
    with open(vers, "w") as f:
        f.write(f"{{ global: {pattern}; local: *; }};\n")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={vers}", "-o", out, *objs],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link of {os.path.basename(out)} failed:\n{r.stdout}\n{r.stderr}")


def build(force: bool = False, verbose: bool = False) -> str:
    stamp = os.path.join(OBJ_DIR, "stamp")
    digest = _digest()
    if not force and all(os.path.exists(row[1]) for row in LIBRARIES) and os.path.exists(stamp) and open(stamp).read() == digest:
        return LIB
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = _hipcc()

    def compile_one(src):
        obj = os.path.join(OBJ_DIR, src.replace(".hip", ".o"))
        cmd = [hipcc, *FLAGS, *EXTRA_FLAGS.get(src, []), "-c", os.path.join(CSRC, src), "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stdout}\n{r.stderr}")
        if verbose and r.stderr.strip():
            print(r.stderr, file=sys.stderr)
        return obj

    every = [src for row in LIBRARIES for src in row[2]]
    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as ex:
        objs = dict(zip(every, ex.map(compile_one, every)))
    for name, lib, sources, pattern in LIBRARIES:
        link(hipcc, lib, [objs[src] for src in sources], pattern,
             os.path.join(OBJ_DIR, "exports.map" if name == "hip" else f"exports_{name}.map"))
    with open(stamp, "w") as f:
        f.write(digest)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
