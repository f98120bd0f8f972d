"""The aggregation multigrid V-cycle of GK_PREC_MG restated on host arrays.

TEST SUPPORT: the contract of include/gmres_hip.h's GK_PREC_MG, written with the CPU
oracle's stencil (oracle.stvec) and Chebyshev sweeps (oracle.precond(PREC_CHEB, ...) at
each level's side) and numpy sums in the stated association order -- every element-wise
expression is a single IEEE operation, so the device cycle is compared with
np.array_equal.

Vectors are flat, i fastest: f(i, j) = f[j * N + i].

Levels: N_0 = N; while N_l is even and N_l / 2 >= 8, N_{l+1} = N_l / 2.  On l < L, with
Cheb = Chebyshev(degree) on `params` from a zero start:

    z  = Cheb(r)
    f  = r - A z
    rc(I, J) = ((f(2I, 2J) + f(2I+1, 2J)) + f(2I, 2J+1)) + f(2I+1, 2J+1)
    ec = MG_{l+1}(rc)
    z(i, j) = z(i, j) + ec(i // 2, j // 2)
    t  = r - A z ;  d = Cheb(t) ;  out = z + d

and MG_L(r) = Chebyshev(nu_c) on the exact spectrum interval of the N_L grid.
"""
import math

import numpy as np

NMIN = 8
DEFAULT_PARAMS = (8.0, 1.0)
DEFAULT_DEGREE = 2


def levels(N: int) -> list[int]:
    out = [N]
    while out[-1] % 2 == 0 and out[-1] // 2 >= NMIN:
        out.append(out[-1] // 2)
    return out


def coarse(NL: int) -> tuple[float, float, int]:
    """(lo, hi, nu_c) of the last level: the 5-point operator's extreme eigenvalues on an
    NL x NL Dirichlet grid and the smallest degree in 1..64 whose Chebyshev error bound
    1 / cosh((nu + 1) acosh sigma) is at most 0.1 (64 where none is)."""
    t = math.pi / (2.0 * (NL + 1))
    lo = 8.0 * math.sin(t) * math.sin(t)
    hi = 8.0 * math.cos(t) * math.cos(t)
    sigma = (hi + lo) / (hi - lo)
    ac = math.acosh(sigma)
    for nu in range(1, 65):
        if 1.0 / math.cosh((nu + 1) * ac) <= 0.1:
            return lo, hi, nu
    return lo, hi, 64


def restrict(f: np.ndarray, N: int) -> np.ndarray:
    """P^T f: the four members of each 2 x 2 block summed in the stated order."""
    F = np.asarray(f, dtype=np.float64).reshape(N, N)  # F[j, i]
    rc = ((F[0::2, 0::2] + F[0::2, 1::2]) + F[1::2, 0::2]) + F[1::2, 1::2]
    return np.ascontiguousarray(rc).reshape(-1)


def prolong_add(z: np.ndarray, ec: np.ndarray, N: int) -> np.ndarray:
    """z + P ec: every fine point takes its block's coarse value."""
    Z = np.asarray(z, dtype=np.float64).reshape(N, N)
    E = np.asarray(ec, dtype=np.float64).reshape(N // 2, N // 2)
    return np.ascontiguousarray(Z + np.repeat(np.repeat(E, 2, axis=0), 2, axis=1)).reshape(-1)


def resid(oracle, r: np.ndarray, z: np.ndarray, N: int) -> np.ndarray:
    return r - oracle.stvec(z, N)


def resid_restrict(oracle, r: np.ndarray, z: np.ndarray, N: int) -> np.ndarray:
    return restrict(resid(oracle, r, z, N), N)


def mg(oracle, r: np.ndarray, N: int, params=DEFAULT_PARAMS, degree: int = DEFAULT_DEGREE) -> np.ndarray:
    """out = MG_0(r) on the N x N grid."""
    sides = levels(N)
    assert len(sides) >= 2, f"no coarse level for N = {N}"
    return _cycle(oracle, np.ascontiguousarray(r, dtype=np.float64).reshape(-1), sides, 0, params, degree)


def _cycle(oracle, r, sides, l, params, degree):
    n = sides[l]
    if l == len(sides) - 1:
        lo, hi, nuc = coarse(n)
        return oracle.precond(oracle.PREC_CHEB, r, n, params=(lo, hi), degree=nuc)

    def cheb(v):
        return oracle.precond(oracle.PREC_CHEB, v, n, params=params, degree=degree)

    z = cheb(r)
    rc = resid_restrict(oracle, r, z, n)
    ec = _cycle(oracle, rc, sides, l + 1, params, degree)
    z = prolong_add(z, ec, n)
    t = resid(oracle, r, z, n)
    return z + cheb(t)


def op_mg(oracle, v: np.ndarray, N: int, side: str = "left", params=DEFAULT_PARAMS,
          degree: int = DEFAULT_DEGREE) -> np.ndarray:
    """The operator stage of an MG-preconditioned Arnoldi step: M^-1 A v on the left,
    A M^-1 v on the right."""
    if side == "right":
        return oracle.stvec(mg(oracle, v, N, params, degree), N)
    return mg(oracle, oracle.stvec(v, N), N, params, degree)


def pcg(oracle, N: int, params=DEFAULT_PARAMS, degree: int = DEFAULT_DEGREE, tol: float = 1e-8, max_iter: int = 200,
        b=None, full: bool = False):
    """Preconditioned CG with the restated cycle in the oracle's operation order for pcg_omp,
    x0 = 0, every reduction through oracle.dot / oracle.norm2 (oracle.set_threads changes their
    summation order).  b = None: b = A 1, stopped on ||r|| / ||b|| < tol, returns
    (iterations, final relative residual).  full = True: also the history of ||r|| (absolute,
    one entry per iteration run) and x -- (iterations, relative residual, history, x); with
    tol = 0 that is exactly max_iter iterations."""
    b = oracle.rhs_ones(N) if b is None else np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    x = np.zeros_like(b)
    r = b.copy()
    z = mg(oracle, r, N, params, degree)
    p = z.copy()
    rz = oracle.dot(r, z)
    bn = oracle.norm2(b)
    hist = []
    it, rel = 0, 1.0
    for it in range(1, max_iter + 1):
        ap = oracle.stvec(p, N)
        alpha = rz / oracle.dot(ap, p)
        x = x + alpha * p
        r = r - alpha * ap
        res = oracle.norm2(r)
        hist.append(res)
        rel = res / bn
        if rel < tol:
            break
        z = mg(oracle, r, N, params, degree)
        rz_new = oracle.dot(r, z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return (it, rel, np.array(hist), x) if full else (it, rel)


def pbicgstab(oracle, b: np.ndarray, N: int, max_iter: int, params=DEFAULT_PARAMS, degree: int = DEFAULT_DEGREE):
    """Preconditioned BiCGSTAB with M^-1 = mg in the oracle's operation order for pbicgstab_omp
    (x0 = 0, r0 = p = r = b; z1 = M^-1 p, alpha = <r, r0> / <A z1, r0>; s = r - alpha A z1;
    z2 = M^-1 s, omega = <A z2, s> / <A z2, A z2>; x = x + alpha z1 + omega z2; r = s - omega A z2;
    beta = (<r, r0> / <r_old, r0>) (alpha / omega); p = r + beta (p - omega A z1)), a fixed
    max_iter iterations: (history of ||r||, x).  A zero denominator ends the run at the last
    finite iteration."""
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    x = np.zeros_like(b)
    r = b.copy()
    r0 = r.copy()
    p = r.copy()
    hist = []
    for _ in range(max_iter):
        z1 = mg(oracle, p, N, params, degree)
        ap = oracle.stvec(z1, N)
        rr0 = oracle.dot(r, r0)
        ap_r0 = oracle.dot(ap, r0)
        if ap_r0 == 0.0 or rr0 == 0.0:
            break
        alpha = rr0 / ap_r0
        s = r - alpha * ap
        z2 = mg(oracle, s, N, params, degree)
        as_ = oracle.stvec(z2, N)
        as_as = oracle.dot(as_, as_)
        if as_as == 0.0:
            break
        omega = oracle.dot(as_, s) / as_as
        if omega == 0.0:
            break
        x = (x + alpha * z1) + omega * z2
        r = s - omega * as_
        hist.append(oracle.norm2(r))
        beta = (oracle.dot(r, r0) / rr0) * (alpha / omega)
        p = r + beta * (p - omega * ap)
    return np.array(hist), x
