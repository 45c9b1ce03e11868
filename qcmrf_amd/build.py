"""Build libqsv.so for gfx950 and the host-only modules (ingest reader, counts formatter) in-tree:  python -m qcmrf_amd.build [--force]"""
from __future__ import annotations

import os
import subprocess
import sys
import sysconfig

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(CSRC, "libqsv.so")
SOURCES = ["qsv_kmulti_m0_r5.hip", "qsv_kmulti_m0_r4.hip", "qsv_kmulti_m0_r3.hip", "qsv_kmulti_m0_low.hip", "qsv.hip",
           "qsv_kmulti_m1.hip", "qsv_kmulti_m2.hip", "qsv_noise.hip", "qsv_noise_hbm.hip", "qsv_noise_measure.hip", "qsv_noise_accept.hip", "qsv_noise_kraus2.hip", "qsv_noise_dynamic.hip", "qsv_density.hip", "qsv_branch.hip"]      # slowest first
DEPENDS = SOURCES + ["qsv_common.h", "qsv_kernels.h", "qsv_kmulti.h", "qsv_kmulti_inst.h", "qsv_gates.inc", "qsv_multi.inc", "qsv_layout.inc", "qsv_measure.inc", "qsv_marginals.inc", "qsv_top.inc",
                     "qsv_exec.inc", "qsv_density.inc", "qsv_noise.h", "qsv_noise_ops.h", "qsv_noise_kernel.h", "qsv_noise_hbm.h", "qsv_noise_hbm_kernel.h", "qsv_noise_hbm_shots.inc", "qsv_noise_lds_shots.inc", "qsv_density.h", "qsv_branch.h", "qsv_branch.inc", os.path.join("..", "..", "include", "qsv.h")]
CFLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
          "-Wno-unused-value", "-Wno-unused-result"]
OBJDIR = os.path.join(CSRC, "_obj")
# host-only CPython modules next to libqsv.so (host C++ against Python's own headers, no HIP in them):
# (module, sources, what Python does in its place where the module cannot be built)
EXT_MODULES = [("_ingest_native", ["ingest_native.cpp"], "ingest reads blocks in Python"),         # reader of clique-block signatures (qcmrf_amd.ingest) and the front end's walk (qcmrf_amd.frontend)
               ("_counts_native", ["counts_native.cpp"], "counts are sorted and formatted in Python")]   # sampled words -> count dict (qcmrf_amd.backend)
EXT_CFLAGS = ["-O2", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fno-exceptions", "-fno-rtti", "-Wall"]


def ext_out(name):
    return os.path.join(HERE, name + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))


def _newer(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(os.path.join(CSRC, d)) > t for d in deps)


def lib_stale():
    return _newer(OUT, DEPENDS)


def ext_stale():
    return any(_newer(ext_out(name), sources) for name, sources, _ in EXT_MODULES)


def stale():
    return lib_stale() or ext_stale()


def build_ext(verbose=True, force=True):
    """the host-only modules (EXT_MODULES): one host compile and link each.  Returns the paths of the ones that stand
    built; a module that cannot be built (no host C++ compiler, no Python headers) is left out and its work stays in
    Python, so that is not an error."""
    include = sysconfig.get_paths()["include"]
    have_headers = os.path.exists(os.path.join(include, "Python.h"))
    cxx = os.environ.get("CXX", "c++")
    built = []
    for name, sources, instead in EXT_MODULES:
        out = ext_out(name)
        if not force and not _newer(out, sources):
            built.append(out)
            continue
        if not have_headers:
            if verbose:
                print("[qcmrf_amd.build] no Python.h under %s: %s not built, %s" % (include, name, instead), flush=True)
            continue
        tmp = out + ".tmp%d" % os.getpid()
        cmd = [cxx] + EXT_CFLAGS + ["-I" + include, "-shared", "-o", tmp] + sources
        if verbose:
            print("[qcmrf_amd.build]", " ".join(cmd), flush=True)
        try:
            subprocess.check_call(cmd, cwd=CSRC)
            os.replace(tmp, out)
        except (OSError, subprocess.CalledProcessError) as e:
            if verbose:
                print("[qcmrf_amd.build] %s not built (%s): %s" % (name, e, instead), flush=True)
            if os.path.exists(tmp):
                os.remove(tmp)
            continue
        built.append(out)
    return built


def build(force=False, verbose=True):
    """one object per translation unit, compiled side by side (the k_multi instantiations are most of
    the work: qsv_kmulti_inst.h), then one link; next to it the host-only modules (build_ext)"""
    if force or ext_stale():
        build_ext(verbose, force)
    if not force and not lib_stale():
        return OUT
    from concurrent.futures import ThreadPoolExecutor
    hipcc = os.environ.get("HIPCC", "hipcc")
    os.makedirs(OBJDIR, exist_ok=True)

    def compile_one(src):
        import time
        obj = os.path.join(OBJDIR, src.replace(".hip", ".o"))
        cmd = [hipcc] + CFLAGS + ["-c", "-o", obj, src]
        if verbose:
            print("[qcmrf_amd.build]", " ".join(cmd), flush=True)
        t0 = time.time()
        subprocess.check_call(cmd, cwd=CSRC)
        if verbose:
            print("[qcmrf_amd.build] %s: %.0f s" % (src, time.time() - t0), flush=True)
        return obj

    with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 1)) as pool:
        objs = list(pool.map(compile_one, SOURCES))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs + ["-ldl"]
    if verbose:
        print("[qcmrf_amd.build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd, cwd=CSRC)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(OUT)
