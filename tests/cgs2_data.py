"""The CGS2 Arnoldi step (gk_set_orthogonalization GK_ORTH_CGS2, include/gmres_hip.h) restated
in NumPy -- the yardstick of tests/test_cgs2_data.py, tests/test_gpu_cgs2_step_known_answer.py
and tests/test_gpu_cgs2.py (a helper, no tests).

The order the header states, per step j on the operator stage's w:

    for sweep = 1, 2:
        s_k = <w, V_k>  for k = 1..j, every dot on the SAME w
        w_e = ((w_e - s_1 V_1,e) - s_2 V_2,e) ... - s_j V_j,e     (element-wise, k ascending)
        H(k,j) = s_k (sweep 1)  /  H(k,j) + s_k (sweep 2)
    h = ||w||;  V(:,j+1) = w / h

cgs2_step evaluates it in any dtype (long double: the reference the device step is held to),
optionally with chunked dot partials (another summation tree) and with one planted fault of the
kind a kernel can have.  cgs2_gmres is restarted GMRES(m) on the identity-preconditioned
5-point operator with that step in float64, the Givens rotations and back substitution of
tests/right_gmres_host.py and the exit of gmres_mgsr_mf.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests.general_data import stencil_any
from tests.right_gmres_host import _back_solve, _givens

FAULTS = ("one_sweep", "dot_tail", "axpy_tail", "axpy_chunk", "dot_zero")


def _dot(a, b, chunk):
    """<a, b> in the operands' dtype: np.dot, or `chunk`-element partials summed last to first."""
    if chunk is None:
        return np.dot(a, b)
    p = a * b
    s = p.dtype.type(0)
    for c0 in reversed(range(0, p.size, chunk)):
        s = s + np.sum(p[c0:c0 + chunk])
    return s


def cgs2_step(V: np.ndarray, w0: np.ndarray, dtype=np.longdouble, chunk=None, fault=None):
    """One CGS2 step on the rows of V (row k = Krylov column k) in `dtype`; returns
    (h[0..j], v_new) rounded to float64.  chunk: the dots' partial length (None: np.dot).
    fault (in both sweeps, as a kernel would have it; column j // 2 where one column is meant):
      "one_sweep"   the second sweep skipped
      "dot_tail"    the last element left out of every dot
      "axpy_tail"   the last element of one column left out of the AXPY
      "axpy_chunk"  one 512-element chunk of one column left out of the AXPY
      "dot_zero"    one column's dot zeroed"""
    assert fault is None or fault in FAULTS, fault
    Vd = np.asarray(V, dtype=dtype)
    w = np.asarray(w0, dtype=dtype).copy()
    j, n = Vd.shape
    hit = j // 2
    h = np.zeros(j + 1, dtype=dtype)
    for sweep in range(1 if fault == "one_sweep" else 2):
        cut = n - 1 if fault == "dot_tail" else n
        s = [_dot(w[:cut], Vd[k, :cut], chunk) for k in range(j)]  # every dot on the same w
        if fault == "dot_zero":
            s[hit] = dtype(0)
        for k in range(j):
            upd = w - s[k] * Vd[k]
            if k == hit and fault == "axpy_tail":
                upd[n - 1] = w[n - 1]
            if k == hit and fault == "axpy_chunk":
                c0 = (n // 512) // 2 * 512
                upd[c0:c0 + 512] = w[c0:c0 + 512]
            w = upd
            h[k] = h[k] + s[k]
    h[j] = np.sqrt(_dot(w, w, chunk))
    return h.astype(np.float64), (w / h[j]).astype(np.float64)


def _orth_f64(V, w, j, orth):
    """The step's projections in float64 on rows 0..j-1 of V; returns (h[0..j-1], w)."""
    h = np.zeros(j)
    if orth == "cgs2":
        for _ in range(2):
            s = V[:j] @ w
            for k in range(j):
                w = w - s[k] * V[k]
            h += s
    else:  # the strict MGS-R step (gmres_mgsr.f90:341-360)
        for _ in range(2):
            for k in range(j):
                d = np.dot(w, V[k])
                h[k] += d
                w = w - d * V[k]
    return h, w


def arnoldi_cycle(N: int, m: int, orth: str, r0: np.ndarray | None = None) -> np.ndarray:
    """The m + 1 basis rows of one cycle on the 5-point operator from r0 (default b = A*1)."""
    n = N * N
    r = stencil_any(np.ones(n), N) if r0 is None else r0
    V = np.zeros((m + 1, n))
    V[0] = r / np.linalg.norm(r)
    for j in range(1, m + 1):
        _, w = _orth_f64(V, stencil_any(V[j - 1], N), j, orth)
        V[j] = w / np.linalg.norm(w)
    return V


def ortho_loss(V: np.ndarray) -> float:
    """||V V^T - I||_F over the rows of V."""
    return float(np.linalg.norm(V @ V.T - np.eye(V.shape[0])))


@dataclass
class Cgs2Run:
    x: np.ndarray
    iterations: int        # (cycles - 1) m + n_out
    n_cycles: int
    n_out: int
    hist_res: np.ndarray   # true relative residual after each cycle


def cgs2_gmres(N: int, m: int, tol: float = 1e-15, max_cycles: int = 1000, orth: str = "cgs2") -> Cgs2Run:
    """Restarted GMRES(m) from x0 = 0 on b = A*1, identity preconditioner, float64: the step of
    `orth`, the reference's Givens rotations, the exit of gmres_mgsr_mf inside the j loop."""
    n = N * N
    b = stencil_any(np.ones(n), N)
    beta0 = np.linalg.norm(b)
    x = np.zeros(n)
    hist = []
    h_val, n_out, ferr = 0.0, 0, 0.0
    for _ in range(max_cycles):
        H = np.zeros((m + 1, m))
        g = np.zeros(m + 1)
        cs = np.zeros(m)
        sn = np.zeros(m)
        V = np.zeros((m + 1, n))
        w = b - stencil_any(x, N)
        beta = np.linalg.norm(w)
        g[0] = beta
        V[0] = w / beta
        for j in range(m):
            n_out = j + 1
            hj, w = _orth_f64(V, stencil_any(V[j], N), j + 1, orth)
            H[: j + 1, j] = hj
            h_val = np.linalg.norm(w)
            H[j + 1, j] = h_val
            _givens(H, cs, sn, g, j)
            ferr = abs(g[j + 1]) / beta0
            if h_val < tol or ferr < tol:
                break
            V[j + 1] = w / h_val
        y = _back_solve(H, g, n_out, m)
        t = np.zeros(n)
        for k in range(n_out):
            t = t + V[k] * y[k]
        x = x + t
        hist.append(np.linalg.norm(b - stencil_any(x, N)) / beta0)
        if h_val < tol or ferr < tol:
            break
    return Cgs2Run(x=x, iterations=(len(hist) - 1) * m + n_out, n_cycles=len(hist), n_out=n_out,
                   hist_res=np.array(hist))


# The planted columns and the long-double references of the step tests, shared by
# tests/test_cgs2_data.py and tests/test_gpu_cgs2_step_known_answer.py; once per case, unchanged.
_basis: dict = {}
_refs: dict = {}


def planted(N: int, m: int) -> np.ndarray:
    from tests.general_data import planted_basis

    if (N, m) not in _basis:
        _basis[(N, m)] = planted_basis(N, m, seed=5000 + 7 * N + m)
    return _basis[(N, m)]


def step_ref(N: int, m: int, j: int, w0_of=None, key=None):
    """(V[:j], w0, cgs2_step(V[:j], w0) in long double) of step j on the planted columns of an
    (N, m) context; w0_of(v): the operator stage (default A v in float64), `key` naming it."""
    k = (N, m, j, key)
    if k not in _refs:
        V = planted(N, m)[:j]
        w0 = stencil_any(V[j - 1], N) if w0_of is None else w0_of(V[j - 1])
        _refs[k] = (V, w0, cgs2_step(V, w0))
    return _refs[k]
