"""Host restatement of restarted MGS-R GMRES(m) on an FP32-compressed Krylov basis
-- the yardstick of the compressed-basis tests (a helper, no tests).

The control flow is tests/right_gmres_host.py's (mgsr_drive with variant = MGSR_MF:
two MGS passes, the Givens rotations in the reference's order, the exit inside the j
loop); only the oracle's stvec / precond / dot / norm2 do vector arithmetic.  With
basis = "f32" every new basis column is rounded through float32
(v.astype(float32).astype(float64): one IEEE round-to-nearest-even conversion of the
FP64 quotient w / h) and everything else stays FP64, which is what
gk_set_basis_precision(GK_BASIS_F32) stores and computes.

guard (basis "f32" only): one cycle on such a basis resolves a residual reduction of
about 2^-24, so a cycle whose final_err(j) falls below floor = 2^-20 g(1) / ||b||
closes at n_out = j -- back-solve, update of x -- WITHOUT any convergence being
declared; the next cycle starts from the FP64 true residual.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import mg_data
from tests.right_gmres_host import PARAMS, _back_solve, _givens

# the issue's table: (N, m, preconditioner, degree, side, tol, max_cycles)
CASES = [
    (32, 10, "identity", 0, "left", 1e-8, 1000),
    (64, 30, "cbpr2", 0, "right", 1e-8, 1000),
    (65, 16, "cbpr2", 0, "left", 1e-8, 1000),
    (48, 20, "cheb", 4, "right", 1e-8, 1000),
    (130, 12, "cbpr2", 0, "right", 1e-8, 6),   # unconverged: six cycles of it
]
# one cycle reduces the residual past the basis's resolution: the exit guard's case
GUARD_CASE = (64, 30, "cheb", 8, "right", 1e-12, 1000)
GUARD = 2.0 ** -20


def case_id(case) -> str:
    N, m, prec, degree, side, tol, _ = case
    return f"N{N}-m{m}-{prec}{degree if prec == 'cheb' else ''}-{side}-{tol:g}"


def round32(v: np.ndarray) -> np.ndarray:
    return v.astype(np.float32).astype(np.float64)


@dataclass
class CbResult:
    x: np.ndarray
    n_cycles: int
    n_out: int                 # of the last cycle
    n_outs: list               # of every cycle
    hist_res: np.ndarray       # true relative residual after each cycle
    hist_ferr: np.ndarray      # (cycles, m): final_err(j) of every step
    final_err: np.ndarray      # (m,) as the driver leaves it after the last cycle
    H1: np.ndarray             # (m + 1, m): the raw Hessenberg columns of cycle 1 (before the rotations)
    guarded: list              # per cycle: closed by the guard

    @property
    def exit_estimate(self) -> float:
        return float(self.hist_ferr[-1, self.n_out - 1])


def gmres_cb_host(orc, N, m, prec="cbpr2", degree=8, side="left", tol=1e-8, params=PARAMS, max_cycles=1000,
                  basis="f32", guard=True, threads=1, b=None) -> CbResult:
    assert side in ("left", "right") and basis in ("f32", "f64")
    kind = "mg" if prec == "mg" else {"identity": orc.PREC_IDENTITY, "cbpr2": orc.PREC_CBPR2, "cheb": orc.PREC_CHEB}[prec]
    store = round32 if basis == "f32" else (lambda v: v)
    orc.set_threads(threads)
    try:
        n = N * N
        b = orc.rhs_ones(N) if b is None else np.ascontiguousarray(b, dtype=np.float64)
        if kind == "mg":  # the aggregation multigrid V-cycle's restatement (tests/mg_data.py)
            minv = lambda r: mg_data.mg(orc, r, N, params, degree)  # noqa: E731
        else:
            minv = lambda r: orc.precond(kind, r, N, params=params, degree=degree)  # noqa: E731
        beta0 = orc.norm2(b)
        x = np.zeros(n)
        final_err = np.zeros(m)
        hist_res, hist_ferr, n_outs, guarded = [], [], [], []
        H1 = np.zeros((m + 1, m))
        h_val, n_out = 0.0, 0
        for cyc in range(max_cycles):
            H = np.zeros((m + 1, m))
            g = np.zeros(m + 1)
            cs = np.zeros(m)
            sn = np.zeros(m)
            V = np.zeros((m + 1, n))
            r = b - orc.stvec(x, N)
            w = minv(r) if side == "left" else r
            beta = orc.norm2(w)
            g[0] = beta
            V[0] = store(w / beta)
            floor = GUARD * (g[0] / beta0)
            ferr = np.zeros(m)
            closed = False
            for j in range(m):
                n_out = j + 1
                w = minv(orc.stvec(V[j], N)) if side == "left" else orc.stvec(minv(V[j]), N)
                for k in range(2):
                    for i in range(j + 1):
                        h = orc.dot(w, V[i])
                        H[i, j] = H[i, j] + h
                        w = w - h * V[i]
                h_val = orc.norm2(w)
                H[j + 1, j] = h_val
                if cyc == 0:
                    H1[: j + 2, j] = H[: j + 2, j]
                _givens(H, cs, sn, g, j)
                final_err[j] = ferr[j] = abs(g[j + 1]) / beta0
                if basis == "f32" and guard and final_err[j] < floor:
                    closed = True
                    break
                if h_val < tol or final_err[j] < tol:
                    break
                V[j + 1] = store(w / h_val) if h_val != 0.0 else np.zeros(n)
            y = _back_solve(H, g, n_out, m)
            t = np.zeros(n)
            for k in range(n_out):
                t = t + V[k] * y[k]
            x = x + (t if side == "left" else minv(t))
            hist_res.append(orc.norm2(b - orc.stvec(x, N)) / beta0)
            hist_ferr.append(ferr)
            n_outs.append(n_out)
            guarded.append(closed)
            if not closed and (h_val < tol or final_err[n_out - 1] < tol):
                break
        return CbResult(x=x, n_cycles=len(hist_res), n_out=n_out, n_outs=n_outs, hist_res=np.array(hist_res),
                        hist_ferr=np.array(hist_ferr), final_err=final_err.copy(), H1=H1, guarded=guarded)
    finally:
        orc.set_threads(1)


_cache: dict = {}


def host_solve(orc, case, basis="f32", guard=True, threads=1, max_cycles=None) -> CbResult:
    """The helper's run of one case, computed once per process and shared; callers do
    not modify it."""
    N, m, prec, degree, side, tol, cap = case
    cap = cap if max_cycles is None else max_cycles
    key = (N, m, prec, degree, side, tol, cap, basis, guard, threads)
    if key not in _cache:
        _cache[key] = gmres_cb_host(orc, N, m, prec=prec, degree=degree or 8, side=side, tol=tol, max_cycles=cap,
                                    basis=basis, guard=guard, threads=threads)
    return _cache[key]


def band(orc, case) -> np.ndarray:
    """S_c: the running maximum over cycles of the relative difference in hist_res between
    the restatement at 1 and at 8 oracle threads (its own summation-order spread: the
    tests/sr_band.py idea).  Length = the shorter of the two runs."""
    r1 = host_solve(orc, case, threads=1)
    r8 = host_solve(orc, case, threads=8)
    k = min(r1.n_cycles, r8.n_cycles)
    return np.maximum.accumulate(np.abs(r8.hist_res[:k] - r1.hist_res[:k]) / r1.hist_res[:k])
