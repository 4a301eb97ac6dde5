"""Build ``libsrgd_hip.so`` (the C-ABI engine, include/srgd_hip.h), ``libsrgd_metrics.so`` (include/srgd_metrics.h), ``libsrgd_ensemble.so`` (include/srgd_ensemble.h), ``libsrgd_consistency.so`` (include/srgd_consistency.h), ``libsrgd_backproject.so`` (include/srgd_backproject.h), ``libsrgd_guidance.so`` (include/srgd_guidance.h), ``libsrgd_solver.so`` (include/srgd_solver.h), ``libsrgd_resize.so`` (include/srgd_resize.h), ``libsrgd_alpha.so`` (include/srgd_alpha.h), ``libsrgd_threshold.so`` (include/srgd_threshold.h) and ``libsrgd_selfens.so`` (include/srgd_selfens.h) in-tree with hipcc for gfx950.

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
LIB = os.path.join(HERE, "libsrgd_hip.so")
METRICS_LIB = os.path.join(HERE, "libsrgd_metrics.so")      # include/srgd_metrics.h: a library of its own, from METRICS_SOURCES
OBJ_DIR = os.path.join(HERE, "build")
METRICS_SOURCES = ["metrics.hip"]
ENSEMBLE_LIB = os.path.join(HERE, "libsrgd_ensemble.so")    # include/srgd_ensemble.h: a library of its own, from ENSEMBLE_SOURCES
ENSEMBLE_SOURCES = ["ensemble.hip"]
CONSISTENCY_LIB = os.path.join(HERE, "libsrgd_consistency.so")    # include/srgd_consistency.h: a library of its own, from CONSISTENCY_SOURCES
CONSISTENCY_SOURCES = ["consistency.hip"]
BACKPROJECT_LIB = os.path.join(HERE, "libsrgd_backproject.so")    # include/srgd_backproject.h: a library of its own, from BACKPROJECT_SOURCES
BACKPROJECT_SOURCES = ["backproject.hip"]
GUIDANCE_LIB = os.path.join(HERE, "libsrgd_guidance.so")    # include/srgd_guidance.h: a library of its own, from GUIDANCE_SOURCES
GUIDANCE_SOURCES = ["guidance.hip"]
SOLVER_LIB = os.path.join(HERE, "libsrgd_solver.so")    # include/srgd_solver.h: a library of its own, from SOLVER_SOURCES
SOLVER_SOURCES = ["solver.hip"]
RESIZE_LIB = os.path.join(HERE, "libsrgd_resize.so")    # include/srgd_resize.h: a library of its own, from RESIZE_SOURCES
RESIZE_SOURCES = ["resize.hip"]
ALPHA_LIB = os.path.join(HERE, "libsrgd_alpha.so")    # include/srgd_alpha.h: a library of its own, from ALPHA_SOURCES
ALPHA_SOURCES = ["alpha.hip"]
THRESHOLD_LIB = os.path.join(HERE, "libsrgd_threshold.so")    # include/srgd_threshold.h: a library of its own, from THRESHOLD_SOURCES
THRESHOLD_SOURCES = ["threshold.hip"]
SELFENS_LIB = os.path.join(HERE, "libsrgd_selfens.so")    # include/srgd_selfens.h: a library of its own, from SELFENS_SOURCES
SELFENS_SOURCES = ["selfens.hip"]
# resize.hip's host code reproduces Pillow's double-precision tables: no fused multiply-adds in it (its kernels are integer code);
# threshold.hip's definition is in separate fp32 multiplications and additions, on the host and in its kernels
EXTRA_FLAGS = {"resize.hip": ["-ffp-contract=off"], "threshold.hip": ["-ffp-contract=off"]}
SOURCES = ["conv_igemm.hip", "conv3x3_bf16.hip", "conv3x3_split.hip", "conv3x3_mx2.hip", "conv1x1_split.hip", "conv1x1_bf16.hip", "conv3x3_mxfp8.hip", "conv1x1_mxfp8.hip", "quant_mxfp8.hip", "norm_act.hip", "attention.hip", "linattn_fused.hip", "linattn_fused256.hip", "cond.hip", "sampler.hip", "imageio.hip", "engine.hip", "kernel_api.hip"]
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value",
         "-fno-gpu-rdc", "-DNDEBUG", "-fvisibility=hidden"]


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


def build(force: bool = False, verbose: bool = False) -> str:
    stamp = os.path.join(OBJ_DIR, "stamp")
    digest = _digest()
    if not force and os.path.exists(LIB) and os.path.exists(METRICS_LIB) and os.path.exists(ENSEMBLE_LIB) and os.path.exists(CONSISTENCY_LIB) and os.path.exists(BACKPROJECT_LIB) and os.path.exists(GUIDANCE_LIB) and os.path.exists(SOLVER_LIB) and os.path.exists(RESIZE_LIB) and os.path.exists(ALPHA_LIB) and os.path.exists(THRESHOLD_LIB) and os.path.exists(SELFENS_LIB) and os.path.exists(stamp) and open(stamp).read() == digest:
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

    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_one, SOURCES + METRICS_SOURCES + ENSEMBLE_SOURCES + CONSISTENCY_SOURCES + BACKPROJECT_SOURCES + GUIDANCE_SOURCES + SOLVER_SOURCES + RESIZE_SOURCES + ALPHA_SOURCES + THRESHOLD_SOURCES + SELFENS_SOURCES))
    selfens_objs = objs[len(objs) - len(SELFENS_SOURCES):]
    objs = objs[:len(objs) - len(SELFENS_SOURCES)]
    threshold_objs = objs[len(objs) - len(THRESHOLD_SOURCES):]
    objs = objs[:len(objs) - len(THRESHOLD_SOURCES)]
    alpha_objs = objs[len(objs) - len(ALPHA_SOURCES):]
    objs = objs[:len(objs) - len(ALPHA_SOURCES)]
    resize_objs = objs[len(objs) - len(RESIZE_SOURCES):]
    objs = objs[:len(objs) - len(RESIZE_SOURCES)]
    solver_objs = objs[len(objs) - len(SOLVER_SOURCES):]
    objs = objs[:len(objs) - len(SOLVER_SOURCES)]
    guidance_objs = objs[len(objs) - len(GUIDANCE_SOURCES):]
    objs = objs[:len(objs) - len(GUIDANCE_SOURCES)]
    metrics_objs = objs[len(SOURCES):len(SOURCES) + len(METRICS_SOURCES)]
    ensemble_objs = objs[len(SOURCES) + len(METRICS_SOURCES):len(SOURCES) + len(METRICS_SOURCES) + len(ENSEMBLE_SOURCES)]
    consistency_objs = objs[len(SOURCES) + len(METRICS_SOURCES) + len(ENSEMBLE_SOURCES):len(objs) - len(BACKPROJECT_SOURCES)]
    backproject_objs = objs[len(objs) - len(BACKPROJECT_SOURCES):]
    objs = objs[:len(SOURCES)]
    # version script: the dynamic symbol table holds the C ABI (srgd_*) and nothing else - without it the weak template
    # instantiations of libstdc++ types (default visibility by the standard library's own attribute) leak out as exports
    vers = os.path.join(OBJ_DIR, "exports.map")
    with open(vers, "w") as f:
        f.write("{ global: srgd_*; local: *; };\n")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={vers}", "-o", LIB, *objs],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    mvers = os.path.join(OBJ_DIR, "exports_metrics.map")
    with open(mvers, "w") as f:
        f.write("{ global: srgd_image_metrics*; local: *; };\n")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={mvers}", "-o", METRICS_LIB,
                        *metrics_objs], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link of the metrics library failed:\n{r.stdout}\n{r.stderr}")
    evers = os.path.join(OBJ_DIR, "exports_ensemble.map")
    with open(evers, "w") as f:
        f.write("{ global: srgd_image_ensemble*; local: *; };\n")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={evers}", "-o", ENSEMBLE_LIB,
                        *ensemble_objs], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link of the ensemble library failed:\n{r.stdout}\n{r.stderr}")
    cvers = os.path.join(OBJ_DIR, "exports_consistency.map")
    with open(cvers, "w") as f:
        f.write("{ global: srgd_image_consistency*; local: *; };\n")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={cvers}", "-o", CONSISTENCY_LIB,
                        *consistency_objs], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link of the consistency library failed:\n{r.stdout}\n{r.stderr}")
    bvers = os.path.join(OBJ_DIR, "exports_backproject.map")
    with open(bvers, "w") as f:
        f.write("{ global: srgd_image_backproject*; local: *; };\n")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={bvers}", "-o", BACKPROJECT_LIB,
                        *backproject_objs], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link of the back-projection library failed:\n{r.stdout}\n{r.stderr}")
    gvers = os.path.join(OBJ_DIR, "exports_guidance.map")
    with open(gvers, "w") as f:
        f.write("{ global: srgd_guidance*; local: *; };\n")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={gvers}", "-o", GUIDANCE_LIB,
                        *guidance_objs], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link of the guidance library failed:\n{r.stdout}\n{r.stderr}")
    svers = os.path.join(OBJ_DIR, "exports_solver.map")
    with open(svers, "w") as f:
        f.write("{ global: srgd_solver*; local: *; };\n")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={svers}", "-o", SOLVER_LIB,
                        *solver_objs], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link of the solver library failed:\n{r.stdout}\n{r.stderr}")
    rvers = os.path.join(OBJ_DIR, "exports_resize.map")
    with open(rvers, "w") as f:
        f.write("{ global: srgd_resize*; local: *; };\n")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={rvers}", "-o", RESIZE_LIB,
                        *resize_objs], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link of the resize library failed:\n{r.stdout}\n{r.stderr}")
    avers = os.path.join(OBJ_DIR, "exports_alpha.map")
    with open(avers, "w") as f:
        f.write("{ global: srgd_alpha*; local: *; };\n")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={avers}", "-o", ALPHA_LIB,
                        *alpha_objs], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link of the alpha library failed:\n{r.stdout}\n{r.stderr}")
    tvers = os.path.join(OBJ_DIR, "exports_threshold.map")
    with open(tvers, "w") as f:
        f.write("{ global: srgd_threshold*; local: *; };\n")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={tvers}", "-o", THRESHOLD_LIB,
                        *threshold_objs], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link of the threshold library failed:\n{r.stdout}\n{r.stderr}")
    evers = os.path.join(OBJ_DIR, "exports_selfens.map")
    with open(evers, "w") as f:
        f.write("{ global: srgd_selfens*; local: *; };\n")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={evers}", "-o", SELFENS_LIB,
                        *selfens_objs], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link of the self-ensemble library failed:\n{r.stdout}\n{r.stderr}")
    with open(stamp, "w") as f:
        f.write(digest)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
