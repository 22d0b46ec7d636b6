"""Build libloftr_hip.so (the C-ABI of the HIP kernels), libloftr_global.so (the global reconstruction stages,
include/loftr_global.h) and libloftr_calib.so (view-graph calibration, include/loftr_calib.h) in-tree for gfx950.

    python -m loftr_amd.build [--force]

hipcc cross-compiles without a GPU.  The shared object lands next to this file so that it
travels with the repo snapshot to the GPU box (a JIT cache would not).
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ_DIR = os.path.join(CSRC, "build")
LIB_PATH = os.path.join(HERE, "libloftr_hip.so")
SOURCES = ["linear.hip", "coarse_plan.hip", "attention.hip", "transformer.hip", "coarse_match.hip", "fine.hip", "misc.hip",
           "sp_convert.hip", "conv.hip", "eval.hip", "input.hip", "comm.hip", "pose.hip", "train.hip", "train_bwd.hip", "encoder_fused.hip", "fine_fused.hip", "head_grads.hip", "encoder_bwd.hip", "fine_bwd.hip", "train_glue.hip", "bank.hip", "pose_gpu.hip", "window_head.hip", "window_head_first.hip", "geometry.hip", "geometry_gpu.hip", "absolute_pose.hip", "absolute_pose_gpu.hip", "scan.hip", "atlas.hip", "atlas_gpu.hip", "triangulate.hip", "triangulate_gpu.hip", "model_lookup.hip", "model_lookup_gpu.hip", "bundle.hip", "bundle_gpu.hip", "register.hip", "register_gpu.hip", "complete.hip", "complete_gpu.hip", "merge.hip", "merge_gpu.hip", "split.hip", "split_gpu.hip", "similarity.hip", "similarity_gpu.hip", "overlap.hip", "overlap_gpu.hip", "undistort.hip", "undistort_gpu.hip", "refine.hip", "refine_gpu.hip", "rotation.hip", "rotation_gpu.hip"]
# the second library: its own translation units, the same flags and version script; it links no object of the first
GLOBAL_LIB_PATH = os.path.join(HERE, "libloftr_global.so")
GLOBAL_SOURCES = ["position.hip", "position_gpu.hip"]
# what a library is stale against besides its translation units.  The first: every other file of csrc/ (as before the second existed)
# and its C ABI header.  The second: the headers its two units include, directly or through them, and both C ABI headers.
GLOBAL_ONLY = GLOBAL_SOURCES + ["position_core.h"]
GLOBAL_HEADERS = ["position_core.h", "bundle_core.h", "tracks_core.h", "stage_timer.h", "common.h"]
# the third library (view-graph calibration): as the second, with its own units, core header and C ABI header
CALIB_LIB_PATH = os.path.join(HERE, "libloftr_calib.so")
CALIB_SOURCES = ["calib.hip", "calib_gpu.hip"]
CALIB_ONLY = CALIB_SOURCES + ["calib_core.h"]
CALIB_HEADERS = ["calib_core.h", "bundle_core.h", "tracks_core.h", "stage_timer.h", "common.h"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-parameter"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _deps_mtime(sources):
    """the newest of the files a library is built from"""
    include = os.path.join(os.path.dirname(HERE), "include")
    if sources is GLOBAL_SOURCES:
        paths = [os.path.join(CSRC, f) for f in GLOBAL_SOURCES + GLOBAL_HEADERS] + [os.path.join(include, "loftr_global.h")]
    elif sources is CALIB_SOURCES:
        paths = [os.path.join(CSRC, f) for f in CALIB_SOURCES + CALIB_HEADERS] + [os.path.join(include, "loftr_calib.h")]
    else:
        paths = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip")) and f not in GLOBAL_ONLY + CALIB_ONLY]
    paths.append(os.path.join(include, "loftr_hip.h"))
    return max(os.path.getmtime(p) for p in paths)


def build(force=False, verbose=True, extra_flags=(), lib_path=None, obj_dir=None):
    """Compile every HIP source for gfx950 and link libloftr_hip.so, libloftr_global.so and libloftr_calib.so.  Returns the first
    one's path.
    extra_flags / lib_path / obj_dir build a variant of the first library next to the product (A/B experiments)."""
    global LIB_PATH, OBJ_DIR
    lib_default, obj_default = LIB_PATH, OBJ_DIR
    if lib_path:
        LIB_PATH, OBJ_DIR, force = lib_path, obj_dir or (OBJ_DIR + "_variant"), True
    try:
        path = _build(force, verbose, tuple(extra_flags), LIB_PATH, SOURCES)
        if not lib_path:
            _build(force, verbose, tuple(extra_flags), GLOBAL_LIB_PATH, GLOBAL_SOURCES)
            _build(force, verbose, tuple(extra_flags), CALIB_LIB_PATH, CALIB_SOURCES)
        return path
    finally:
        LIB_PATH, OBJ_DIR = lib_default, obj_default


def _build(force, verbose, extra_flags, lib, sources):
    if not force and os.path.exists(lib) and os.path.getmtime(lib) >= _deps_mtime(sources):
        return lib
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = _hipcc()

    def compile_one(src):
        obj = os.path.join(OBJ_DIR, src.replace(".hip", ".o"))
        cmd = [hipcc, *FLAGS, *extra_flags, "-c", os.path.join(CSRC, src), "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr}")
        if verbose and r.stderr.strip():
            sys.stderr.write(r.stderr)
        return obj

    with ThreadPoolExecutor(max_workers=min(8, len(sources))) as ex:
        objs = list(ex.map(compile_one, sources))
    # export the C ABI only (include/loftr_hip.h, include/loftr_global.h, include/loftr_calib.h: loftr_*); the C++ launch helpers shared between translation units stay internal
    vs = os.path.join(OBJ_DIR, "exports.map")
    with open(vs, "w") as fh:
        fh.write("{ global: loftr_*; local: *; };\n")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={vs}", "-o", lib, *objs, "-ldl"],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stderr}")
    if verbose:
        print(f"built {lib} ({os.path.getsize(lib) / 1e6:.2f} MB)")
    return lib


if __name__ == "__main__":
    # python -m loftr_amd.build [--force] [--variant NAME -DFLAG ...]  ->  libloftr_hip_NAME.so
    if "--variant" in sys.argv:
        i = sys.argv.index("--variant")
        name = sys.argv[i + 1]
        build(extra_flags=[a for a in sys.argv[i + 2:] if a.startswith("-")],
              lib_path=os.path.join(HERE, f"libloftr_hip_{name}.so"), obj_dir=os.path.join(CSRC, "build", f"variant_{name}"))
    else:
        build(force="--force" in sys.argv)
