"""Build the native libraries of the package in-tree (no JIT cache).

  lib/libsvslam_hip.so      HIP kernels + C ABI (include/svslam.h), gfx950
  lib/libsvslam_synth.so    CPU generator of the synthetic stereo stream
  lib/libsvslam_pipeline.so C++ host pipeline (Frontend/Backend/Map mirror of the
                            reference) bound to libsvslam_hip.so
  lib/lib<name>_host_emu.so a kernel header of csrc/ compiled for the host by tests/cpp/<name>_host_emu/emu.cpp, one per
                            entry of EMUS (lv, pg, lf, brief, lc, gd: k_loop_verify.h, k_pose_graph.h, k_local_fusion.h,
                            k_brief.h, k_loop_candidates.h, k_global_desc.h; bm, cf, colour, orb: k_stereo_bm.h,
                            k_cloud_filter.h, k_colour.h, k_orb.h; orb_desc: k_orb_desc.h with the two it shares code with).  The build fails here, not in a test, when a kernel file stops being plain
                            C++ between the HIP qualifiers; the tests load the same libraries through build_emu

hipcc cross-compiles gfx950 without a GPU, so this runs in the build container.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
HOST = os.path.join(HERE, "host")
LIB = os.path.join(HERE, "lib")
ROOT = os.path.dirname(HERE)

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
             "-Wno-unused-value"]
# development: extra compiler flags for an A/B variant (tools/ab.sh), output directory of the variant
HIP_FLAGS += os.environ.get("SVS_EXTRA_HIP_FLAGS", "").split()
if os.environ.get("SVS_LIB_DIR"):
    LIB = os.path.abspath(os.environ["SVS_LIB_DIR"])
if os.environ.get("SVS_IEEE_DIV"):      # parity-debugging build: IEEE division / sqrt instead of estimate + Newton in the LM kernels
    HIP_FLAGS.append("-DSVS_IEEE_DIV")


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _sources(d, exts):
    out = []
    for root, _, files in os.walk(d):
        for f in files:
            if f.endswith(exts):
                out.append(os.path.join(root, f))
    return out


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def source_hash():
    """sha256 (first 12 hex digits) over the sources and flags libsvslam_hip.so is compiled from: svslam_build_info() carries
    it, the PMC summaries under profiles/ are stamped with it and bench.py says whether the stamp is the loaded library's"""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(_sources(CSRC, (".hip", ".h")) + [os.path.join(ROOT, "include", "svslam.h")]):
        h.update(os.path.relpath(f, ROOT).encode())
        h.update(open(f, "rb").read())
    h.update(" ".join(HIP_FLAGS).encode())
    return h.hexdigest()[:12]


def build_hip(force=False, verbose=False):
    os.makedirs(LIB, exist_ok=True)
    out = os.path.join(LIB, "libsvslam_hip.so")
    srcs = _sources(CSRC, (".hip", ".h")) + [os.path.join(ROOT, "include", "svslam.h")]
    if force or _newer(out, srcs):
        _run([HIPCC] + HIP_FLAGS + ['-DSVS_SRC_HASH="%s"' % source_hash(),
                                     os.path.join(CSRC, "svslam_hip.hip"), os.path.join(CSRC, "synth.hip"),
                                     "-o", out], verbose)
    return out


def build_synth(force=False, verbose=False):
    os.makedirs(LIB, exist_ok=True)
    out = os.path.join(LIB, "libsvslam_synth.so")
    srcs = [os.path.join(CSRC, f) for f in ("synth_cpu.c", "synth_scene.h", "synth_traj.h")]
    if force or _newer(out, srcs):
        _run(["gcc", "-O2", "-fPIC", "-shared", "-std=gnu99", srcs[0], "-o", out, "-lm"], verbose)
    return out


def build_pipeline(force=False, verbose=False):
    os.makedirs(LIB, exist_ok=True)
    out = os.path.join(LIB, "libsvslam_pipeline.so")
    main = os.path.join(HOST, "pipeline_capi.cpp")
    if not os.path.exists(main):
        return None
    srcs = _sources(HOST, (".cpp", ".h")) + [os.path.join(ROOT, "include", "svslam.h")]
    hip_so = build_hip(force=False, verbose=verbose)
    if force or _newer(out, srcs + [hip_so]):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", os.path.join(ROOT, "include"),
              "-I", CSRC, main, "-o", out, "-L", LIB, "-lsvslam_hip", "-Wl,-rpath,$ORIGIN"], verbose)
    return out


# The host emulations: tests/cpp/<name>_host_emu/emu.cpp includes a kernel header of csrc/ and compiles it with g++.
# name -> (files besides emu.cpp it is made of, relative to the tree's root; flags besides EMU_FLAGS)
EMU_FLAGS = ["-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]
_C, _SHIM = "stereovision-slam_amd/csrc/", "tests/cpp/hip_on_host.h"
EMUS = {
    "lv": ([_C + "k_loop_verify.h", _C + "k_pose_graph.h"], []),
    "pg": ([_C + "k_pose_graph.h"], []),
    "lf": ([_C + "k_local_fusion.h", _C + "k_pose_graph.h"], []),
    "brief": ([_C + "k_brief.h"], []),
    "lc": ([_C + "k_loop_candidates.h"], []),
    "gd": ([_C + "k_global_desc.h"], []),
    "bm": ([_C + "k_stereo_bm.h", _C + "pyr_geom.h", _SHIM], ["-pthread"]),
    "cf": ([_C + "k_cloud_filter.h", _SHIM], ["-Wno-unknown-pragmas"]),
    "colour": ([_C + "k_colour.h", "include/svslam.h", _SHIM], ["-Wno-unknown-pragmas"]),
    "orb": ([_C + "k_orb.h"], ["-Wno-unknown-pragmas"]),
    "orb_desc": ([_C + "k_orb_desc.h", _C + "k_orb.h", _C + "k_brief.h"], ["-Wno-unknown-pragmas"]),
}


def build_emu(name, root=ROOT, out_dir=LIB, force=False, verbose=False, opt="-O2"):
    """lib<name>_host_emu.so in out_dir from the tree at root: this one, or a test's copy with an edited kernel (the mutant tests, which
    also lower opt: they compile once per mutant)"""
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "lib%s_host_emu.so" % name)
    main = os.path.join(str(root), "tests", "cpp", name + "_host_emu", "emu.cpp")
    deps, flags = EMUS[name]
    if force or _newer(out, [main] + [os.path.join(str(root), d) for d in deps]):
        _run(["g++", opt] + EMU_FLAGS + flags + [main, "-o", out], verbose)
    return out


def build_all(force=False, verbose=False):
    return [build_hip(force, verbose), build_synth(force, verbose), build_pipeline(force, verbose)] + \
           [build_emu(n, force=force, verbose=verbose) for n in EMUS]


if __name__ == "__main__":
    for p in build_all(force="--force" in sys.argv, verbose=True):
        print("built", p)
