"""The premises of the general-data GPU tests, pinned without a GPU (tests/general_data.py):
general_rhs has none of the square's symmetries while b = A*1 and its Krylov vectors have
all of them, and the single-step bound of test_gpu_step_known_answer.py -- 64 eps ||w|| ||v||
per Hessenberg entry, 64 eps max|v_ref| per element of the new column -- passes a correct
float64 step with another summation tree by a factor of 8 or more and fails each seeded fault
(with the multigrid cycle as the operator, which cancels w0 to a tenth: by a factor of 2).
"""
import numpy as np
import pytest

from tests import mg_data
from tests.general_data import (MG_DEGREE, MG_PARAMS, PREC_STEP_CASES, asymmetry, assert_asymmetric, blocked_step,
                                general_rhs, mgs_step_ld, planted_basis, step_bounds)


def test_general_rhs_is_asymmetric_and_rhs_ones_is_not(oracle):
    N = 64
    x_true, b = general_rhs(oracle, N, 7)
    assert min(asymmetry(b, N)) > 0.1 * np.max(np.abs(b))
    assert np.array_equal(b, oracle.stvec(x_true, N))
    # the blind spot itself: four cbpr2 Krylov vectors of b = A*1 carry every symmetry
    ones = oracle.rhs_ones(N)
    v = oracle.precond(oracle.PREC_CBPR2, ones, N)
    for _ in range(4):
        v = v / np.linalg.norm(v)
        assert max(asymmetry(v, N)) < 1e-14
        with pytest.raises(AssertionError):
            assert_asymmetric(v, N)
        v = oracle.precond(oracle.PREC_CBPR2, oracle.stvec(v, N), N)


def _dot_tree(a, b, skip_last=False):
    """Float64 dot with a summation tree of its own: 256-element partials, summed in
    reverse order."""
    p = a * b
    if skip_last:
        p = p[:-1]
    parts = [float(np.sum(p[s:s + 256])) for s in range(0, p.size, 256)]
    s = 0.0
    for x in reversed(parts):
        s += x
    return s


def _step_f64(V, w0, fault=None):
    """The step in float64 with _dot_tree; fault: None, "dot_tail" (the last element left out
    of one dot), "axpy1" / "axpy2" (one 512-element chunk left out of one AXPY of the first /
    second pass), "one_pass" (the second pass skipped)."""
    j = V.shape[0]
    w = w0.copy()
    h = np.zeros(j + 1)
    hit = j // 2
    for p in range(1 if fault == "one_pass" else 2):
        for i in range(j):
            d = _dot_tree(w, V[i], skip_last=(fault == "dot_tail" and p == 0 and i == hit))
            upd = w - d * V[i]
            if fault == f"axpy{p + 1}" and i == hit:
                c = (w.size // 512) // 2 * 512
                upd[c:c + 512] = w[c:c + 512]
            w = upd
            h[i] += d
    h[j] = np.sqrt(_dot_tree(w, w))
    return h, w / h[j]


def _ratios(h, v, V, w0, ref):
    hb, vb = step_bounds(V, w0, ref[1])
    return float(np.max(np.abs(h - ref[0]) / hb)), float(np.max(np.abs(v - ref[1])) / vb)


@pytest.mark.parametrize("N,j", [(45, 5), (130, 6), (256, 8)])
def test_step_bound_passes_reordering_and_fails_seeded_faults(oracle, N, j):
    V = planted_basis(N, j, seed=100 + N)
    for k in range(j):
        assert_asymmetric(V[k], N)
    gram = V @ V.T - np.eye(j)
    assert 1e-7 < np.max(np.abs(gram)) < 1e-2  # ~pert / N: signal for both passes, amplification near 1
    w0 = oracle.stvec(V[j - 1], N)
    ref = mgs_step_ld(V, w0)
    # the reference is a step: the new column has unit length and is orthogonal to V as far
    # as two passes over columns with Gram off-diagonals d ~ 1e-3 leave it (second order in d)
    assert np.max(np.abs(V @ ref[1])) < 1e-6 and abs(np.linalg.norm(ref[1]) - 1.0) < 1e-14
    rh, rv = _ratios(*_step_f64(V, w0), V, w0, ref)
    print(f"N={N} j={j}: reordered float64 step, h dev/bound {rh:.4f}, column dev/bound {rv:.4f}")
    assert rh <= 1.0 / 8 and rv <= 1.0 / 8
    for fault in ("dot_tail", "axpy1", "axpy2", "one_pass"):
        fh, fv = _ratios(*_step_f64(V, w0, fault), V, w0, ref)
        print(f"N={N} j={j}: {fault}: h dev/bound {fh:.3e}, column dev/bound {fv:.3e}")
        assert max(fh, fv) > 10.0, fault


MG_PIN_CASES = ([(c[1], c[5], c[6], j) for c in PREC_STEP_CASES if c[2] == "mg" for j in (1, 2, c[6])]
                + [("left", 1450, 2, j) for j in (1, 2)])


@pytest.mark.parametrize("side,N,m,j", MG_PIN_CASES, ids=[f"{s}-{N}-j{j}" for s, N, m, j in MG_PIN_CASES])
def test_step_bound_with_multigrid_operator(oracle, side, N, m, j):
    """The multigrid rows of PREC_STEP_CASES and the N = 1450 step of test_gpu_mg.py, on the
    columns the GPU tests plant (seed 5000 + 7 N + m): w0 = M^-1 A v (right: A M^-1 v) from the
    restated cycle.  M^-1 approximates A^-1, so the step cancels w0 = v_j + (a remainder of
    about a tenth of it) down to h(j+1) / ||w0|| ~ 0.1 and the new column's rounding error,
    eps ||w0|| / h(j+1) per element, uses more of its bound than on the identity: the reordered
    float64 step stays below 1/2 of both bounds (measured: h <= 0.004, column <= 0.19, the
    level the Chebyshev(8) rows reach), and every seeded fault still exceeds 10 (>= 2.9e3)."""
    V = planted_basis(N, m, seed=5000 + 7 * N + m)[:j]
    for k in range(j):
        assert_asymmetric(V[k], N)
    w0 = mg_data.op_mg(oracle, V[j - 1], N, side, MG_PARAMS, MG_DEGREE)
    ref = mgs_step_ld(V, w0)
    print(f"mg {side} N={N} j={j}: h(j+1) / ||w0|| {ref[0][j] / np.linalg.norm(w0):.3f}")
    rh, rv = _ratios(*_step_f64(V, w0), V, w0, ref)
    print(f"mg {side} N={N} j={j}: reordered float64 step, h dev/bound {rh:.4f}, column dev/bound {rv:.4f}")
    assert rh <= 0.5 and rv <= 0.5
    for fault in ("dot_tail", "axpy1", "axpy2", "one_pass"):
        fh, fv = _ratios(*_step_f64(V, w0, fault), V, w0, ref)
        print(f"mg {side} N={N} j={j}: {fault}: h dev/bound {fh:.3e}, column dev/bound {fv:.3e}")
        assert max(fh, fv) > 10.0, fault


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("N,j", [(45, 5), (130, 6), (256, 8)])
def test_blocked_step_emulation(oracle, N, j, S):
    """The blocked step (GK_TUNE_RES_BLOCK) runs its second sweep over the blocks in reverse
    order, so on the planted columns it differs from the strict step at second order in the
    Gram off-diagonals -- far outside the strict bound (measured here: h 4e3 .. 5e5 and the
    column 1.4e4 .. 1.3e6 times the bound).  Its float64 emulation with another summation tree
    stays within 1/8 of the strict bound of its own long-double evaluation, which is what
    test_gpu_step_known_answer.py holds k_mgs_blk to, next to the widened bound against the
    strict reference.  S = 1 of the emulation is the strict step."""
    V = planted_basis(N, j, seed=100 + N)
    w0 = oracle.stvec(V[j - 1], N)
    strict = mgs_step_ld(V, w0)
    one = blocked_step(V, w0, 1)
    assert np.array_equal(one[0], strict[0]) and np.array_equal(one[1], strict[1])
    ref = blocked_step(V, w0, S)
    emu = blocked_step(V, w0, S, dtype=np.float64, dot=_dot_tree)
    rh, rv = _ratios(*emu, V, w0, ref)
    sh, sv = _ratios(*emu, V, w0, strict)
    print(f"N={N} j={j} S={S}: float64 emulation vs long-double blocked step: h dev/bound {rh:.4f}, column "
          f"{rv:.4f}; vs the strict step: h {sh:.3e}, column {sv:.3e}")
    assert rh <= 1.0 / 8 and rv <= 1.0 / 8
    assert max(sh, sv) > 10.0  # the order of the second sweep shows on planted columns
