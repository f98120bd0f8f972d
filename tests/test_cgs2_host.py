"""Host-side checks of the CGS2 option that need no GPU: the header's lines, the ctypes
constants and signatures, the Fortran bindings and the driver's argument."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from gmres_amd import build

    build.build_all()
    from gmres_amd import _native

    return _native


def test_header_declares_the_scheme():
    txt = open(os.path.join(ROOT, "include", "gmres_hip.h")).read()
    assert re.search(r"^#define GK_ORTH_MGSR 0\b", txt, re.M)
    assert re.search(r"^#define GK_ORTH_CGS2 1\b", txt, re.M)
    assert re.search(r"^int gk_set_orthogonalization\(gk_ctx \*ctx, int scheme\);", txt, re.M)
    assert re.search(r"^int gk_get_orthogonalization\(gk_ctx \*ctx, int \*scheme\);", txt, re.M)
    assert re.search(r"^#define GK_NKID 26\b", txt, re.M)  # no new kernel id
    # the FP32 basis is out of scope, and the header says so
    assert "GK_ORTH_CGS2 on a" in txt and "GK_BASIS_F32" in txt and "GK_ERR_STATE" in txt


def test_native_constants_and_signatures(built):
    nat = built
    assert (nat.GK_ORTH_MGSR, nat.GK_ORTH_CGS2) == (0, 1)
    assert nat.GK_CGS_KB in (8, 16)
    assert nat._SIGS["gk_set_orthogonalization"] == (nat.c_int, [nat.c_vp, nat.c_int])
    assert nat._SIGS["gk_get_orthogonalization"] == (nat.c_int, [nat.c_vp, nat._ip])
    L = nat.hip()
    assert hasattr(L, "gk_set_orthogonalization") and hasattr(L, "gk_get_orthogonalization")
    assert L.gk_set_orthogonalization(None, nat.GK_ORTH_CGS2) == nat.GK_ERR_ARG  # null context
    # the kernels' default batch is the constant the tests size their shapes by
    txt = open(os.path.join(ROOT, "gmres_amd", "csrc", "gk_cgs.hpp")).read()
    assert re.search(rf"CGS_KB_DEFAULT = {nat.GK_CGS_KB};", txt)


def test_python_surface():
    import gmres_amd as ga
    from gmres_amd import solver

    assert solver.ORTH == {"mgsr": 0, "cgs2": 1}
    assert callable(ga.Context.set_orth) and isinstance(ga.Context.orth, property)


def test_fortran_bindings_and_driver_argument(built):
    src = open(os.path.join(ROOT, "gmres_amd", "fortran", "gmres_hip.f90")).read()
    assert "GK_ORTH_MGSR = 0, GK_ORTH_CGS2 = 1" in src
    assert re.search(r"public ::.*GK_ORTH_MGSR, GK_ORTH_CGS2", src)
    for name in ("gk_set_orthogonalization", "gk_get_orthogonalization"):
        assert f"bind(C, name='{name}')" in src
    assert re.search(r"side, basis, orth\)", src)  # the optional argument, after basis
    built.fhost()
    out = subprocess.run(["nm", "-D", "--undefined-only", built.FHOST_SO], capture_output=True, text=True).stdout
    assert "gk_set_orthogonalization" in out  # gmres_mgsr_hip(orth=...) calls it
    exe = os.path.join(ROOT, "gmres_amd", "lib", "test_mfp_hip")
    usage = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout
    assert "cgs2" in usage and "f32" in usage


def test_build_lists_the_unit():
    from gmres_amd import build as b

    assert [u[2] for u in b.HIP_UNITS_CGS] == ["gk_cgs.o"]
    assert len(b.HIP_UNITS + b.HIP_UNITS_CB + b.HIP_UNITS_CGS) == 14
    remarks = ("gk_cgs.hip:36:1: remark: Function Name: _ZN2gk10k_cgs_dotsILi16ELb1EEEvPKdS2_xixPd\n"
               "gk_cgs.hip:36:1: remark:     ScratchSize [bytes/lane]: 8 [-Rpass-analysis=kernel-resource-usage]\n")
    assert b._scratch_kernels(remarks, "k_cgs_") == ["_ZN2gk10k_cgs_dotsILi16ELb1EEEvPKdS2_xixPd"]
