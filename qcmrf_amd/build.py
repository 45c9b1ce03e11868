"""Build libqsv.so for gfx950 and the host-only ingest reader in-tree:  python -m qcmrf_amd.build [--force]"""
from __future__ import annotations

import os
import subprocess
import sys
import sysconfig

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(CSRC, "libqsv.so")
SOURCES = ["qsv_kmulti_m0_r5.hip", "qsv_kmulti_m0_r4.hip", "qsv_kmulti_m0_r3.hip", "qsv_kmulti_m0_low.hip", "qsv.hip",
           "qsv_kmulti_m1.hip", "qsv_kmulti_m2.hip", "qsv_noise.hip", "qsv_noise_hbm.hip", "qsv_noise_measure.hip", "qsv_noise_accept.hip", "qsv_noise_kraus2.hip", "qsv_density.hip", "qsv_branch.hip"]      # slowest first
DEPENDS = SOURCES + ["qsv_common.h", "qsv_kernels.h", "qsv_kmulti.h", "qsv_kmulti_inst.h", "qsv_gates.inc", "qsv_multi.inc", "qsv_layout.inc", "qsv_measure.inc",
                     "qsv_exec.inc", "qsv_density.inc", "qsv_noise.h", "qsv_noise_ops.h", "qsv_noise_kernel.h", "qsv_noise_hbm.h", "qsv_noise_hbm_kernel.h", "qsv_noise_hbm_shots.inc", "qsv_noise_lds_shots.inc", "qsv_density.h", "qsv_branch.h", "qsv_branch.inc", os.path.join("..", "..", "include", "qsv.h")]
CFLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
          "-Wno-unused-value", "-Wno-unused-result"]
OBJDIR = os.path.join(CSRC, "_obj")
# the native reader of clique-block signatures (qcmrf_amd.ingest): host C++ against Python's own headers, no HIP in it
EXT_SOURCES = ["ingest_native.cpp"]
EXT_OUT = os.path.join(HERE, "_ingest_native" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))
EXT_CFLAGS = ["-O2", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fno-exceptions", "-fno-rtti", "-Wall"]


def _newer(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(os.path.join(CSRC, d)) > t for d in deps)


def lib_stale():
    return _newer(OUT, DEPENDS)


def ext_stale():
    return _newer(EXT_OUT, EXT_SOURCES)


def stale():
    return lib_stale() or ext_stale()


def build_ext(verbose=True):
    """_ingest_native: one host compile and link.  Returns its path, or None where it cannot be built (no host C++
    compiler, no Python headers): ingest then reads the blocks in Python, so that is not an error."""
    include = sysconfig.get_paths()["include"]
    if not os.path.exists(os.path.join(include, "Python.h")):
        if verbose:
            print("[qcmrf_amd.build] no Python.h under %s: _ingest_native not built, ingest reads blocks in Python" % include, flush=True)
        return None
    cxx = os.environ.get("CXX", "c++")
    tmp = EXT_OUT + ".tmp%d" % os.getpid()
    cmd = [cxx] + EXT_CFLAGS + ["-I" + include, "-shared", "-o", tmp] + EXT_SOURCES
    if verbose:
        print("[qcmrf_amd.build]", " ".join(cmd), flush=True)
    try:
        subprocess.check_call(cmd, cwd=CSRC)
        os.replace(tmp, EXT_OUT)
    except (OSError, subprocess.CalledProcessError) as e:
        if verbose:
            print("[qcmrf_amd.build] _ingest_native not built (%s): ingest reads blocks in Python" % e, flush=True)
        if os.path.exists(tmp):
            os.remove(tmp)
        return None
    return EXT_OUT


def build(force=False, verbose=True):
    """one object per translation unit, compiled side by side (the k_multi instantiations are most of
    the work: qsv_kmulti_inst.h), then one link; next to it the ingest reader (build_ext)"""
    if force or ext_stale():
        build_ext(verbose)
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
