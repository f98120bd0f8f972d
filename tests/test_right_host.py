"""CPU checks of the right-preconditioning yardstick (tests/right_gmres_host.py)
and of the C-ABI's new names; no GPU.

The helper restates restarted MGS-R GMRES(m) on the oracle's stvec / precond /
dot / norm2.  In left mode it must BE the oracle's solver before anything is
measured against it in right mode; in right mode its stopping quantity must be
the true residual, and in left mode visibly not."""
import os

import numpy as np
import pytest

from tests.right_gmres_host import CASES, TOL, case_id, gmres_mgsr_host, host_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N,m,prec,degree", [(32, 10, "cbpr2", 8), (64, 30, "cheb", 8)])
def test_helper_left_reproduces_oracle(oracle, N, m, prec, degree):
    """Same vector primitives in the same order as or_gmres_mgsr (MGSR_MF, 1 thread):
    same cycles and n_out, histories bit for bit."""
    kind = {"cbpr2": oracle.PREC_CBPR2, "cheb": oracle.PREC_CHEB}[prec]
    ref = oracle.gmres_mgsr(oracle.rhs_ones(N), N, m, tol=TOL, prec=kind, params=(8.2, 0.2), degree=degree,
                            variant=oracle.MGSR_MF, threads=1)
    h = gmres_mgsr_host(oracle, N, m, prec=prec, degree=degree, side="left", tol=TOL)
    assert h.n_cycles == len(ref.hist_res)
    assert h.n_out == ref.n_out
    assert np.array_equal(h.hist_res, ref.hist_res)
    assert np.array_equal(h.final_err, ref.final_err)
    assert np.array_equal(h.hist_ferr, ref.hist_ferr)
    assert np.array_equal(h.x, ref.x)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_helper_right_estimate_is_the_true_residual(oracle, case):
    """Right side: |g(j+1)| / ||b|| at the end of every cycle is the true relative
    residual to rounding (measured on these cases: gap <= 2.1e-8)."""
    h = host_solve(oracle, case, "right")
    print(f"{case_id(case)}: right gap {h.gap():.3e}, cycles {h.n_cycles}, last n_out {h.n_out}")
    assert h.gap() < 1e-6


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_helper_left_estimate_is_not(oracle, case):
    """Control: on the left the same quantity is off by more than 10 % on every
    case (measured: >= 0.116), so the gap discriminates."""
    h = host_solve(oracle, case, "left")
    print(f"{case_id(case)}: left gap {h.gap():.3e}, last est / true {h.hist_ferr[-1, h.n_out - 1]:.3e} / "
          f"{h.hist_res[-1]:.3e}")
    assert h.gap() > 0.1


def test_cabi_names_of_right_preconditioning():
    from gmres_amd import _native as nat

    assert "gk_set_precond_side" in nat._SIGS
    assert nat.GK_TUNE_RIGHT_FUSED == 31 and (nat.GK_SIDE_LEFT, nat.GK_SIDE_RIGHT) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "gmres_hip.h")).read()
    for line in ("#define GK_TUNE_RIGHT_FUSED 31", "#define GK_SIDE_LEFT 0", "#define GK_SIDE_RIGHT 1"):
        assert line in hdr, line
