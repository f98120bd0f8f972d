"""The yardstick of the CGS2 step's GPU tests, pinned without a GPU (tests/cgs2_data.py).

On the planted columns of tests/general_data.py the strict step bound (64 eps ||w|| ||v|| per
Hessenberg entry, 64 eps max |v_ref| per element of the new column) against cgs2_step in long
double passes a correct float64 CGS2 step with another summation tree by a factor of 8 or more
and fails every planted fault on the column; CGS2 and the strict MGS-R step differ on planted
columns at second order in the Gram off-diagonals (printed, not asserted); restarted GMRES(m)
with the CGS2 step holds the residual-history contract of the blocked step against the
reference's own runs (tests/golden/reference_runs.json); and one CGS2 cycle loses at most 8 x
the orthogonality the same MGS-R cycle loses.

Figures these tests print (pytest -s): summation-order margin <= 0.06 (h) and 0.09 (column) of
the bound; smallest fault excess on the column 2.6e7 x the bound (faults planted in both sweeps,
as a kernel would have them); CGS2 against mgs_step_ld up to 7e8 x the bound; solves 670 / 670,
1354 / 1357 and 3590 / 3592 iterations with history deviations 5.5e-7, 2.3e-7 and 3.4e-7;
orthogonality ratio 0.9 - 1.2.
"""
import json
import os

import numpy as np
import pytest

from tests import cgs2_data as cd
from tests.general_data import mgs_step_ld, step_bounds

HERE = os.path.dirname(os.path.abspath(__file__))
REF = json.load(open(os.path.join(HERE, "golden", "reference_runs.json")))

# (N, m): the issue's shapes, and (33, 17): odd n, j = 8, 9 and 17 cross a batch of 8 columns
SHAPES = [(2, 3), (3, 5), (45, 12), (130, 6), (64, 16), (33, 17)]


def _js(N, m):
    return [8, 9, 17] if (N, m) == (33, 17) else [1, 2, m]


def _ratios(h, v, V, w0, ref):
    hb, vb = step_bounds(V, w0, ref[1])
    return float(np.max(np.abs(h - ref[0]) / hb)), float(np.max(np.abs(v - ref[1])) / vb)


def _case(oracle, N, m, j):
    return cd.step_ref(N, m, j, w0_of=lambda v: oracle.stvec(v, N), key="A")


@pytest.mark.parametrize("N,m", SHAPES)
def test_summation_order_margin(oracle, N, m):
    """A float64 step with 512-element chunked partials against the long-double step."""
    for j in _js(N, m):
        V, w0, ref = _case(oracle, N, m, j)
        rh, rv = _ratios(*cd.cgs2_step(V, w0, dtype=np.float64, chunk=512), V, w0, ref)
        print(f"N={N} m={m} j={j}: chunked float64 step, h dev/bound {rh:.4f}, column dev/bound {rv:.4f}")
        assert rh <= 1.0 / 8 and rv <= 1.0 / 8


@pytest.mark.parametrize("N,m", SHAPES)
def test_planted_faults_exceed_the_bound(oracle, N, m):
    for j in _js(N, m):
        V, w0, ref = _case(oracle, N, m, j)
        for fault in cd.FAULTS:
            fh, fv = _ratios(*cd.cgs2_step(V, w0, fault=fault), V, w0, ref)
            print(f"N={N} m={m} j={j}: {fault}: h dev/bound {fh:.3e}, column dev/bound {fv:.3e}")
            assert fv > 1.0, (fault, j)


@pytest.mark.parametrize("N,m", SHAPES)
def test_cgs2_against_the_strict_step_is_second_order(oracle, N, m):
    """Printed for the record: the two orders differ far outside the strict bound on planted
    columns (nothing on an orthonormal basis), so the device step is held to cgs2_step."""
    for j in _js(N, m):
        V, w0, ref = _case(oracle, N, m, j)
        rh, rv = _ratios(*mgs_step_ld(V, w0), V, w0, ref)
        print(f"N={N} m={m} j={j}: mgs_step_ld vs cgs2_step: h dev/bound {rh:.3e}, column dev/bound {rv:.3e}")
        assert np.isfinite(rh) and np.isfinite(rv)


def _contract(got, ref, rtol=1e-5, atol=1e-13):  # tests/test_gpu_blocked.py::_contract
    k = min(len(got), len(ref))
    assert k >= 1
    g, r = np.asarray(got[:k]), np.asarray(ref[:k])
    bad = np.abs(g - r) > rtol * np.abs(r) + atol
    assert not bad.any(), f"cycles {np.nonzero(bad)[0].tolist()} deviate: got={g} ref={r}"


@pytest.mark.parametrize("key", ["mgsr_mf_identity_32_m10", "mgsr_mf_identity_64_m20", "mgsr_omp_identity_128_m30"])
def test_cgs2_solve_holds_the_history_contract(key):
    g = REF[key]
    run = cd.cgs2_gmres(g["N"], g["m"], tol=1e-15)
    hi = [k for k, v in enumerate(g["hist_res"]) if v > 1e-10]
    ref = np.asarray(g["hist_res"][: len(hi)])
    k = min(len(ref), run.n_cycles)
    dev = float(np.max(np.abs(run.hist_res[:k] - ref[:k]) / ref[:k]))
    print(f"{key}: {run.iterations} iterations (reference {g['iterations']}), max history deviation {dev:.2e}, "
          f"max |x - 1| {np.max(np.abs(run.x - 1.0)):.2e}")
    assert run.n_cycles >= len(hi)
    _contract(run.hist_res[: len(hi)], ref)
    assert abs(run.iterations - g["iterations"]) <= 0.01 * g["iterations"]
    assert np.max(np.abs(run.x - 1.0)) < 1e-9


@pytest.mark.parametrize("N,m", [(45, 12), (64, 20), (128, 30), (256, 95)])
def test_loss_of_orthogonality_within_8x_of_mgsr(N, m):
    lc, lm = cd.ortho_loss(cd.arnoldi_cycle(N, m, "cgs2")), cd.ortho_loss(cd.arnoldi_cycle(N, m, "mgsr"))
    print(f"N={N} m={m}: ||V^T V - I||_F CGS2 {lc:.3e}, MGS-R {lm:.3e}, ratio {lc / lm:.2f}")
    assert lc <= 8.0 * lm
