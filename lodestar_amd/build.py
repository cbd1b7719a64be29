"""In-tree build of the native pieces (run on the CPU container; the .so files travel to
the GPU box with the tree).  hipcc cross-compiles gfx950 without a GPU.

  * lodestar_amd/liblodestar_bls.so   the product: HIP kernels + C ABI (include/lodestar_bls.h)
  * build/lb_harness.so               test infrastructure: the same arithmetic headers
                                      compiled for x86, checked against oracle/ on CPU
  * build/lb_cpu_pool                 CPU baseline pool (oracle/cpu_pool.cpp)
"""
from __future__ import annotations

import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lodestar_amd", "csrc")
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "lodestar_amd", "liblodestar_bls.so")
HARNESS = os.path.join(ROOT, "build", "lb_harness.so")
CPU_POOL = os.path.join(ROOT, "build", "lb_cpu_pool.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _sources(*names):
    return [os.path.join(CSRC, n) for n in names]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _deps():
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    return hdrs + [os.path.join(INC, "lodestar_bls.h")]


def _jobs():
    """parallel compiles: the host's CPUs, at most 16 (the GPU box's share), at most one per group"""
    n = os.cpu_count() or 4
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        pass
    return max(1, min(16, n, int(os.environ.get("MAX_JOBS", "16") or 16)))


HOST_UNITS = [("lb_engine.hip", "engine.o"), ("lb_kzg_host.hip", "kzg_host.o")]
# every unit of the library compiles with these (tools/isa_compare.py compiles with them too)
LIB_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-value"]


def build_lib(force=False, verbose=True, extra_flags=(), out=None):
    """The split build (tools/gen_kdecls.py): lb_kgroup.hip once per kernel group (-DLB_KGROUP=g)
    and the host units (host code + launches, -DLB_KGROUP=99: lb_engine.hip, the BLS pipeline, and
    lb_kzg_host.hip, the KZG calls), compiled in parallel, linked into one shared library."""
    out = out or LIB
    if not force and not extra_flags and not _stale(out, _deps()):
        return out
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_kdecls
    cur = open(gen_kdecls.OUT).read() if os.path.exists(gen_kdecls.OUT) else ""
    if cur != gen_kdecls.render():
        with open(gen_kdecls.OUT, "w") as f:
            f.write(gen_kdecls.render())
    odir = os.path.join(ROOT, "build", "obj" + ("" if out == LIB else "_" + os.path.basename(out)))
    os.makedirs(odir, exist_ok=True)
    base = [HIPCC, *LIB_FLAGS, "-I" + INC, "-I" + CSRC, *extra_flags]
    units = [(os.path.join(CSRC, src), "99", os.path.join(odir, obj)) for src, obj in HOST_UNITS]
    units += [(os.path.join(CSRC, "lb_kgroup.hip"), str(g), os.path.join(odir, f"kgroup{g}.o"))
              for g in range(gen_kdecls.N_GROUPS)]
    # the slowest units first
    order = [u for u in units if u[1] in ("3", "6", "8", "9", "7")] + [u for u in units if u[1] not in ("3", "6", "8", "9", "7")]
    running, failed = [], []
    t0 = time.time()
    # per-unit staleness: every unit on the headers, lb_kgroup.hip and a host unit also on itself;
    # no unit includes a host unit, so the kernel groups outlive a change to the host code
    hdrs = [d for d in _deps() if os.path.basename(d) not in [src for src, _ in HOST_UNITS]]
    pend = [u for u in order if force or extra_flags or _stale(u[2], hdrs + [u[0]])]
    while pend or running:
        while pend and len(running) < _jobs():
            src, g, obj = pend.pop(0)
            cmd = base + ["-DLB_KGROUP=" + g, "-c", src, "-o", obj]
            if verbose:
                print("[build]", " ".join(cmd[-5:]), flush=True)
            running.append((subprocess.Popen(cmd), os.path.basename(obj), time.time()))
        time.sleep(0.2)
        for r in list(running):
            rc = r[0].poll()
            if rc is not None:
                running.remove(r)
                if verbose:
                    print(f"[build] {r[1]} done in {time.time() - r[2]:.0f} s (rc {rc})", flush=True)
                if rc != 0:
                    failed.append(r[1])
    if failed:
        raise subprocess.CalledProcessError(1, f"hipcc ({failed})")
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", *[u[2] for u in units], "-o", out + ".tmp"]
    subprocess.run(cmd, check=True)
    os.replace(out + ".tmp", out)
    if verbose:
        print(f"[build] {out} in {time.time() - t0:.0f} s", flush=True)
    return out


def _build_so(src, out, extra_deps=(), flags=("-O2",), force=False, verbose=True):
    """one g++ shared object from one source; stale on the source, the csrc headers and extra_deps"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not force and not _stale(out, _deps() + [src, *extra_deps]):
        return out
    cmd = ["g++", *flags, "-shared", "-fPIC", "-I" + INC, "-I" + CSRC, src, "-o", out + ".tmp"]
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(out + ".tmp", out)
    return out


HDIR = os.path.join(ROOT, "tests", "harness")
FR_VIEWS = os.path.join(HDIR, "fr_views.h")  # the pointer views the kzg_*_lanes.h headers share
COMB_HARNESS = os.path.join(ROOT, "build", "lb_comb_harness.so")
FR_HARNESS = os.path.join(ROOT, "build", "lb_fr_harness.so")
KZG_BATCH_HARNESS = os.path.join(ROOT, "build", "lb_kzg_batch_harness.so")
KZG_BLOB_HARNESS = os.path.join(ROOT, "build", "lb_kzg_blob_harness.so")
KZG_CELLS_HARNESS = os.path.join(ROOT, "build", "lb_kzg_cells_harness.so")
KZG_FK20_HARNESS = os.path.join(ROOT, "build", "lb_kzg_fk20_harness.so")
KZG_RECOVER_HARNESS = os.path.join(ROOT, "build", "lb_kzg_recover_harness.so")
SEARCH_HARNESS = os.path.join(ROOT, "build", "lb_search_harness.so")
PIPELINE_HARNESS = os.path.join(ROOT, "build", "lb_pipeline_harness.so")


def build_harness(force=False, verbose=True):
    return _build_so(os.path.join(HDIR, "lb_harness.cpp"), HARNESS, force=force, verbose=verbose)


def build_comb_harness(force=False, verbose=True):
    """the fixed-base comb of the resident pubkey table on the CPU (tests/test_pk_comb_cpu.py)"""
    return _build_so(os.path.join(HDIR, "lb_comb_harness.cpp"), COMB_HARNESS, force=force, verbose=verbose)


def build_fr_harness(force=False, verbose=True):
    """the scalar field, its transform and the evaluate-and-divide scan on the CPU (tests/test_fr_cpu.py)"""
    return _build_so(os.path.join(HDIR, "lb_fr_harness.cpp"), FR_HARNESS, force=force, verbose=verbose)


def build_kzg_batch_harness(force=False, verbose=True):
    """the segmented aggregation and the evaluation of the batched KZG verification on the CPU
    (tests/test_kzg_batch_cpu.py)"""
    return _build_so(os.path.join(HDIR, "lb_kzg_batch_harness.cpp"), KZG_BATCH_HARNESS, force=force, verbose=verbose)


def build_kzg_blob_harness(force=False, verbose=True):
    """the transcripts, the many-polynomial quotient scan, the status fold and the offsets validator of
    the per-blob KZG calls on the CPU (tests/test_kzg_blob_cpu.py)"""
    return _build_so(os.path.join(HDIR, "lb_kzg_blob_harness.cpp"), KZG_BLOB_HARNESS,
                     [os.path.join(HDIR, "kzg_blob_lanes.h"), FR_VIEWS], ("-O2", "-std=c++17", "-pthread"), force, verbose)


def build_kzg_cells_harness(force=False, verbose=True):
    """the combiner, the coset transform, the cell interpolation and quotient lanes and the status fold
    of the cell calls on the CPU (tests/test_kzg_cells_cpu.py)"""
    return _build_so(os.path.join(HDIR, "lb_kzg_cells_harness.cpp"), KZG_CELLS_HARNESS,
                     [os.path.join(HDIR, "kzg_cells_lanes.h"), FR_VIEWS], ("-O2", "-std=c++17", "-pthread"), force, verbose)


def build_kzg_fk20_harness(force=False, verbose=True):
    """the column transforms and the 128-point transform's schedule, over the scalar field and over G1
    points, of the FK20 call on the CPU (tests/test_kzg_fk20_cpu.py)"""
    return _build_so(os.path.join(HDIR, "lb_kzg_fk20_harness.cpp"), KZG_FK20_HARNESS,
                     [os.path.join(HDIR, "kzg_fk20_lanes.h"), FR_VIEWS], ("-O2", "-std=c++17"), force, verbose)


def build_kzg_recover_harness(force=False, verbose=True):
    """the slot map, the vanishing polynomial's values, the column decode and the blob's elements from
    its coefficients of the recovery call, and its argument check, on the CPU (tests/test_kzg_recover_cpu.py)"""
    return _build_so(os.path.join(HDIR, "lb_kzg_recover_harness.cpp"), KZG_RECOVER_HARNESS,
                     [os.path.join(HDIR, "kzg_recover_lanes.h"), os.path.join(HDIR, "kzg_fk20_lanes.h"), FR_VIEWS],
                     ("-O2", "-std=c++17"), force, verbose)


def build_search_harness(force=False, verbose=True):
    """the invalid-set search's planner and interpreter (csrc/lb_search_plan.h) against a model device on
    the CPU (tests/test_search_plan_cpu.py; tests/test_gpu_parity.py compares the device's trace with it)"""
    return _build_so(os.path.join(HDIR, "lb_search_harness.cpp"), SEARCH_HARNESS,
                     [os.path.join(HDIR, "search_model.h")], ("-O2", "-std=c++17"), force, verbose)


def build_pipeline_harness(force=False, verbose=True):
    """the batch pipeline's form selection (csrc/lb_pipeline_plan.h) on the CPU (tests/test_pipeline_plan_cpu.py)"""
    return _build_so(os.path.join(HDIR, "lb_pipeline_harness.cpp"), PIPELINE_HARNESS, flags=("-O2", "-std=c++17"),
                     force=force, verbose=verbose)


def build_cpu_pool(force=False, verbose=True):
    src = os.path.join(ROOT, "oracle", "cpu_pool.cpp")
    if not os.path.exists(src):
        return None
    return _build_so(src, CPU_POOL, flags=("-O3", "-pthread"), force=force, verbose=verbose)


# tools/ubench programs the GPU tests run (correctness of the asm Fp multiply; the row, wave and
# group engines' arithmetic at operand level)
UBENCH = ["fpmul_asm", "lanes_check"]


def build_ubench(force=False, verbose=True):
    out = []
    for name in UBENCH:
        src = os.path.join(ROOT, "tools", "ubench", name + ".hip")
        dst = os.path.join(ROOT, "tools", "ubench", name)
        if force or _stale(dst, _deps() + [src]):
            cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value",
                   "-I" + INC, "-I" + CSRC, src, "-o", dst]
            if verbose:
                print("[build]", " ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
        out.append(dst)
    return out


NAPI = os.path.join(ROOT, "lodestar_amd", "napi", "lodestar_bls.node")


def build_napi(force=False, verbose=True):
    """N-API addon (plain C against the system node_api.h) linked to liblodestar_bls.so."""
    src = os.path.join(ROOT, "lodestar_amd", "napi", "lb_napi.c")
    hdr = "/usr/include/node/node_api.h"
    if not os.path.exists(hdr):
        return None
    if not force and not _stale(NAPI, [src, LIB, os.path.join(INC, "lodestar_bls.h")]):
        return NAPI
    cmd = ["gcc", "-O2", "-shared", "-fPIC", "-pthread", "-I/usr/include/node", "-I" + INC, src, "-o", NAPI + ".tmp",
           "-L" + os.path.dirname(LIB), "-llodestar_bls", "-Wl,-rpath,$ORIGIN/.."]
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(NAPI + ".tmp", NAPI)
    return NAPI


def build_all(force=False):
    build_lib(force)
    build_napi(force)
    build_harness(force)
    build_comb_harness(force)
    build_fr_harness(force)
    build_kzg_batch_harness(force)
    build_kzg_blob_harness(force)
    build_kzg_cells_harness(force)
    build_kzg_fk20_harness(force)
    build_kzg_recover_harness(force)
    build_search_harness(force)
    build_pipeline_harness(force)
    build_cpu_pool(force)
    build_ubench(force)


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
