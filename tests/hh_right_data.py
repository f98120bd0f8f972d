"""The long-double step of right-preconditioned Householder GMRES on planted reflectors (test
infrastructure for tests/test_gpu_hh_right.py and tests/test_hh_right_host.py; a helper, no
tests).

tests/hh_data.py plants reflectors P_1..P_m and holds ONE step of gmres_hh.f90:255-321 to its
long-double evaluation.  Here the operator between the two reflection chains is A M^-1 with
cbpr2 (gk_hh_step with GK_HH_PREC_RIGHT), restated in np.longdouble: general_data.cbpr2_ld
(t / d, z + alpha (t - A z), the float64 coefficients the device uses) followed by the
long-double stencil.  The bounds are hh_data.hh_bounds unchanged -- 64 eps ||w0|| on the
Hessenberg column, 64 eps |pivot|, 64 eps max |rest| -- although the device forms w0 in
float64 from v rounded to float64: one cbpr2 and one stencil are about ten roundings per
element, each of a term no larger than a few |w0_i|-sized neighbours, far inside 64 eps ||w0||
once the reflections (which keep the norm) have spread them; test_hh_right_host.py pins that
a float64 step on the oracle's operator stays below a quarter of every bound.
"""
from __future__ import annotations

import numpy as np

from tests import hh_data as hd
from tests.general_data import EPS, MARGIN, cbpr2_ld, stencil_any

PARAMS = (8.2, 0.2)
M = 8
# N = 34 and 66: VEC 2, below and just above one wave of double2 lanes per line
SHAPES = [34, 66]
# beyond those: the smallest N <= 130 at which the w-only reflection chains can be forced
# (two workgroups), where GK_TUNE_HH_FUSE 1 / 0 are different launches
WONLY_SHAPE = 130

_refs: dict = {}


def js(m: int = M) -> list[int]:
    return [1, 3, m]


def right_op_ld(oracle, v: np.ndarray, N: int) -> np.ndarray:
    """A M^-1 v in long double."""
    return stencil_any(cbpr2_ld(oracle, v, N), N)


def reference(oracle, N: int, j: int, m: int = M):
    """hh_data.hh_step_ld of step j on hh_data.reflectors(N, m) with the operator A M^-1; the
    sign of h[j] is guarded as in hh_data.hh_reference.  Once per case."""
    key = (N, m, j)
    if key not in _refs:
        ref = hd.hh_step_ld(hd.reflectors(N, m), j, N, lambda v: right_op_ld(oracle, v, N))
        assert abs(ref[4]) > hd.SIGN_GUARD * MARGIN * EPS * ref[2], (N, j, ref[4], ref[2])  # change m, not the bound
        _refs[key] = ref
    return _refs[key]


def right_op_f64(oracle, v: np.ndarray, N: int) -> np.ndarray:
    """A M^-1 v on the oracle (bit-exact with both device routes, test_gpu_right_precond.py)."""
    v64 = np.ascontiguousarray(v, dtype=np.float64)
    return oracle.stvec(oracle.precond(oracle.PREC_CBPR2, v64, N, params=PARAMS), N)
