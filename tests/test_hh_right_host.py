"""CPU checks of right-preconditioned Householder GMRES: the C-ABI's new names, gmres_hh's
argument handling, and the yardstick of the single-step GPU test (tests/hh_right_data.py);
no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import hh_data as hd
from tests import hh_right_data as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(text: str, name: str) -> int:
    m = re.search(r"^#define\s+%s\s+(-?\d+)\s*$" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def test_cabi_names_of_right_householder():
    from gmres_amd import _native as nat

    hdr = open(os.path.join(ROOT, "include", "gmres_hip.h")).read()
    assert nat.GK_HH_PREC_NONE == _define(hdr, "GK_HH_PREC_NONE") == 0
    assert nat.GK_HH_PREC_LEFT == _define(hdr, "GK_HH_PREC_LEFT") == 1
    assert nat.GK_HH_PREC_RIGHT == _define(hdr, "GK_HH_PREC_RIGHT") == 2
    # no new tuning key: the update's route is GK_TUNE_RIGHT_FUSED's
    assert nat.GK_TUNE_RIGHT_FUSED == _define(hdr, "GK_TUNE_RIGHT_FUSED") == 31
    assert max(int(v) for v in re.findall(r"^#define\s+GK_TUNE_\w+\s+(\d+)\s*$", hdr, re.M)) == 32
    # the precondition argument is a plain int in the header and in the bindings
    for name, args in (("gk_hh_cycle_start", [nat.c_vp, nat.c_int, nat._dp]),
                       ("gk_hh_step", [nat.c_vp, nat.c_int, nat.c_int, nat._dp]),
                       ("gk_hh_step_async", [nat.c_vp, nat.c_int, nat.c_int]),
                       ("gk_hh_update_x", [nat.c_vp, nat._dp, nat.c_int])):
        assert nat._SIGS[name] == (nat.c_int, args) and name in nat.header_symbols()
    assert re.search(r"int gk_hh_cycle_start\(gk_ctx \*ctx, int precondition, double \*g1\);", hdr)
    assert re.search(r"int gk_hh_step\(gk_ctx \*ctx, int j, int precondition, double \*hcol\);", hdr)
    assert re.search(r"int gk_hh_step_async\(gk_ctx \*ctx, int j, int precondition\);", hdr)
    # the Fortran host names the same values
    f90 = open(os.path.join(ROOT, "gmres_amd", "fortran", "gmres_hip.f90")).read()
    assert "GK_HH_PREC_NONE = 0, GK_HH_PREC_LEFT = 1, GK_HH_PREC_RIGHT = 2" in f90


@pytest.mark.parametrize("arg,mode", [(True, 1), (False, 0), ("right", 2), ("left", 1), ("none", 0),
                                      (np.bool_(True), 1)])
def test_hh_prec_mode(arg, mode):
    from gmres_amd import solver

    assert solver.hh_prec_mode(arg) == mode


def test_hh_prec_mode_rejects_other_words():
    from gmres_amd import solver

    with pytest.raises(ValueError, match="'right'"):
        solver.hh_prec_mode("both")


class _FakeHost:
    def __init__(self):
        self.calls = []

    def gmres_hh_hip_run(self, *args):
        self.calls.append(args)
        return 0


class _FakeCtx:
    handle, m, nloc = ctypes.c_void_p(0), 4, 16


@pytest.mark.parametrize("arg,mode,exit_", [(True, 1, 1), (False, 0, 0), ("right", 2, 1)])
def test_gmres_hh_passes_the_mode(monkeypatch, arg, mode, exit_):
    """gmres_hh hands the Fortran driver the GK_HH_PREC_* value, and the in-cycle exit of
    gmres_hh_prec_omp by default wherever it preconditions."""
    from gmres_amd import _native as nat
    from gmres_amd import solver

    fake = _FakeHost()
    monkeypatch.setattr(nat, "fhost", lambda: fake)
    solver.gmres_hh(_FakeCtx(), precondition=arg, max_cycles=2)
    (call,) = fake.calls
    assert call[3] == mode and call[4] == exit_
    fake.calls.clear()
    solver.gmres_hh(_FakeCtx(), precondition=arg, midcycle_exit=False, max_cycles=2)
    assert fake.calls[0][3] == mode and fake.calls[0][4] == 0


@pytest.mark.parametrize("N", hr.SHAPES + [hr.WONLY_SHAPE])
def test_right_step_pin(oracle, N):
    """The yardstick before anything is measured against it: a float64 step on the oracle's
    A M^-1 (what the device applies, bit for bit) with numpy's dots stays below a quarter of
    every bound of the long-double step, for every (N, j) the GPU test runs; and the same
    step without the preconditioner exceeds one.  (cbpr2 is a polynomial in A, so M^-1 A and
    A M^-1 agree to rounding: one step cannot tell the sides apart -- the cycle start and the
    update do, test_gpu_hh_right.py's residual tests.)"""
    P = hd.reflectors(N, hr.M)
    for j in hr.js():
        ref = hr.reference(oracle, N, j)
        h, p, *_ = hd.hh_step(P, j, lambda v: hr.right_op_f64(oracle, v, N), dtype=np.float64)
        r = hd.hh_ratios(h, p, ref, j)
        print(f"N={N} j={j}: float64 step over bound h {r[0]:.3e}, pivot {r[1]:.3e}, rest {r[2]:.3e}")
        assert max(r) < 0.25, (N, j, r)
        hw, pw, *_ = hd.hh_step(P, j, lambda v: oracle.stvec(np.ascontiguousarray(v, dtype=np.float64), N),
                                dtype=np.float64)
        assert max(hd.hh_ratios(hw, pw, ref, j)) > 1.0, (N, j)
