"""Build the native parts in-tree (gfx950 only).

  gmres_amd/lib/libgmres_hip.so     HIP kernels + C-ABI (include/gmres_hip.h), hipcc
  gmres_amd/lib/libgmres_fhost.so   Fortran host (restart loop, Givens), amdflang
  gmres_amd/lib/test_mfp_hip        Fortran driver mirroring tests/test_poisson_mf.f90
  gmres_amd/lib/sweep_hip           Fortran sweep drivers (utils.f90 table layout)

hipcc cross-compiles gfx950 code objects without a GPU, so this runs in the
build container; the .so files travel to the GPU box with the repo snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
LIB = os.path.join(PKG, "lib")
CSRC = os.path.join(PKG, "csrc")
FSRC = os.path.join(PKG, "fortran")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

HIP_SO = os.path.join(LIB, "libgmres_hip.so")
FHOST_SO = os.path.join(LIB, "libgmres_fhost.so")
DRIVER = os.path.join(LIB, "test_mfp_hip")

# Translation units compiled in parallel, one per subsystem: the C-ABI's context, tuning,
# profiling and stateless entries (gk_api), the Arnoldi launches with the streaming kernels
# and the MGS-R cycle (gk_step), the Householder cycle (gk_hh), the operator and
# preconditioner launches with the stencil kernels (gk_op), the Chebyshev pass split by
# level count, the blocked and the strict resident steps (gk_blk, gk_resident), the
# collectives (gk_comm), the short-recurrence solvers (gk_sr_api), the compressed-basis
# step (gk_cb) and the CGS2 step (gk_cgs).
# Seconds per unit, one compile at a time on an 8-core build machine: gk_api 7,
# gk_cheb0..3 26-31, gk_blk 15, gk_resident 42-48 (the unrolled resident kernels),
# gk_comm 4, gk_sr_api 8; the single gk_api unit they were split from took 47-60.
def _src(unit: str) -> str:
    return os.path.join(CSRC, unit + ".hip")


def _unit(unit: str) -> tuple[str, list[str], str]:
    return (_src(unit), [], unit + ".o")


# (source, extra defines, object name): the Chebyshev pass in GK_CF_PARTS parts
GK_CF_PARTS = 4
HIP_UNITS = ([_unit("gk_api"), _unit("gk_step"), _unit("gk_hh"), _unit("gk_op")]
             + [(_src("gk_cheb"), [f"GK_CF_PART={p}"], f"gk_cheb{p}.o") for p in range(GK_CF_PARTS)]
             + [_unit(u) for u in ("gk_blk", "gk_resident", "gk_comm", "gk_sr_api")])
# ... and the unit of the opt-in FP32-compressed basis: its resident step, scale and widening copy (its
# launch-path projection, x update and Gram are float instantiations in gk_step's unit); HIP_UNITS stays
# the FP64 solvers' list
HIP_UNITS_CB = [_unit("gk_cb")]
# ... and the unit of the opt-in CGS2 Arnoldi step (batched dots, reduce, j-column AXPY): fourteen in all
HIP_UNITS_CGS = [_unit("gk_cgs")]
# ... and the unit of the multigrid preconditioner's transfer and closing kernels: fifteen with it
HIP_UNITS_MG = [_unit("gk_mg")]
HIP_UNITS_ALL = HIP_UNITS + HIP_UNITS_CB + HIP_UNITS_CGS + HIP_UNITS_MG
HIP_SOURCES = sorted({u[0] for u in HIP_UNITS_ALL})
HIP_HEADERS = [os.path.join(CSRC, h) for h in ("gk_common.hpp", "gk_kernels.hpp", "gk_step_kernels.hpp",
                                                "gk_hh_kernels.hpp", "gk_march.hpp", "gk_stencil.hpp", "gk_cheb.hpp",
                                                "gk_res.hpp", "gk_blk.hpp", "gk_sr.hpp", "gk_host.hpp", "gk_resident.hpp",
                                                "gk_cb.hpp", "gk_cgs.hpp", "gk_mg.hpp")]
HIP_DEPS = HIP_SOURCES + HIP_HEADERS + [os.path.join(ROOT, "include", "gmres_hip.h")]
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall"]
F_SOURCES = [os.path.join(FSRC, "gmres_hip.f90")]


def _newer(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd: list[str], cwd: str | None = None) -> None:
    print("+", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, cwd=cwd)


def hipcc() -> str:
    for c in (os.path.join(ROCM, "bin", "hipcc"), shutil.which("hipcc") or ""):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def flang() -> str:
    for c in (os.path.join(ROCM, "lib", "llvm", "bin", "flang"), os.path.join(ROCM, "bin", "amdflang"),
              shutil.which("flang") or ""):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("amdflang not found")


def _scratch_kernels(remarks: str, name: str) -> list[str]:
    """Kernels named like `name` whose resource-usage remark reports scratch."""
    bad, fn = [], None
    for line in remarks.splitlines():
        if "Function Name:" in line:
            fn = line.split("Function Name:", 1)[1].split()[0]
        elif "ScratchSize [bytes/lane]:" in line and fn and name in fn:
            if int(line.split("ScratchSize [bytes/lane]:", 1)[1].split()[0]) > 0:
                bad.append(fn)
    return bad


def _compile_link(so: str, defines: list[str]) -> None:
    """Compile the HIP translation units in parallel into objects beside `so`,
    then link them into the shared library.  The Chebyshev pass, the resident
    step kernels, the two-level right-preconditioning march and the stencil marches
    (among them the accumulating cbpr2 sweep of the right-preconditioned update) must not spill
    registers to scratch (gk_cheb.hip refuses such a
    pass at run time; a spilled resident kernel holds w in scratch memory): the
    build fails here, naming them."""
    objs, procs = [], []
    for src, unit_defs, oname in HIP_UNITS_ALL:
        obj = os.path.join(os.path.dirname(so), oname)
        cmd = [hipcc(), *HIP_FLAGS, *[f"-D{x}" for x in defines + unit_defs], "-c", src, "-o", obj,
               "-Rpass-analysis=kernel-resource-usage"]
        print("+", " ".join(cmd), flush=True)
        procs.append(subprocess.Popen(cmd, stderr=subprocess.PIPE, text=True))
        objs.append(obj)
    bad = []
    for p in procs:
        err = p.communicate()[1]
        sys.stderr.write("".join(l + "\n" for l in err.splitlines() if "warning:" in l or "error" in l))
        for name in ("k_cheb_fused", "k_mgs_wpc", "k_mgs_wres", "k_mgs_res", "k_mgs_blk", "k_right_cbpr2",
                     "k_mgs_wcb", "k_stencil", "k_cgs_", "k_mg_"):
            bad += _scratch_kernels(err, name)
    if any(p.returncode for p in procs):
        raise subprocess.CalledProcessError(max(p.returncode for p in procs), "hipcc")
    if bad:
        raise RuntimeError(f"kernels built with a register spill to scratch (refused): {bad}")
    _run([hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared", *objs, "-o", so, "-lrccl"])
    for o in objs:
        os.remove(o)


def build_hip(force: bool = False) -> str:
    os.makedirs(LIB, exist_ok=True)
    if force or _newer(HIP_SO, HIP_DEPS):
        _compile_link(HIP_SO, [])
    return HIP_SO


def build_fortran(force: bool = False) -> str:
    os.makedirs(LIB, exist_ok=True)
    moddir = os.path.join(LIB, "mod")
    os.makedirs(moddir, exist_ok=True)
    common = ["-O2", "-ffp-contract=off", "-fPIC", f"-J{moddir}"]
    link = [f"-L{LIB}", "-lgmres_hip", "-Wl,-rpath,$ORIGIN"]
    if force or _newer(FHOST_SO, F_SOURCES + [HIP_SO]):
        _run([flang(), *common, "-shared", *F_SOURCES, "-o", FHOST_SO, *link])
    for name in ("test_mfp_hip", "sweep_hip"):
        src = os.path.join(FSRC, name + ".f90")
        exe = os.path.join(LIB, name)
        if force or _newer(exe, [src, FHOST_SO]):
            _run([flang(), *common, src, "-o", exe, f"-L{LIB}", "-lgmres_fhost", "-lgmres_hip", "-Wl,-rpath,$ORIGIN"])
    return FHOST_SO


def build_variant(name: str, defines: list[str]) -> str:
    """An A/B build: libgmres_hip.so compiled with extra -D macros (kernel
    geometry knobs such as GK_RES_RW / GK_RES_WB) plus a copy of the Fortran
    host beside it (its $ORIGIN rpath then binds that build); select it with
    GK_LIB_DIR=<returned dir>."""
    d = os.path.join(LIB, "variants", name)
    os.makedirs(d, exist_ok=True)
    so = os.path.join(d, "libgmres_hip.so")
    _compile_link(so, defines)
    build_fortran()
    shutil.copy2(FHOST_SO, os.path.join(d, "libgmres_fhost.so"))
    return d


def build_all(force: bool = False) -> None:
    build_hip(force)
    build_fortran(force)


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
