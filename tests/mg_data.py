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


def pcg(oracle, N: int, params=DEFAULT_PARAMS, degree: int = DEFAULT_DEGREE, tol: float = 1e-8, max_iter: int = 200):
    """Preconditioned CG with the restated cycle, b = A 1, x0 = 0, to ||r|| / ||b|| < tol:
    (iterations, final relative residual)."""
    b = oracle.rhs_ones(N)
    x = np.zeros_like(b)
    r = b.copy()
    z = mg(oracle, r, N, params, degree)
    p = z.copy()
    rz = float(r @ z)
    bn = float(np.sqrt(b @ b))
    for it in range(1, max_iter + 1):
        ap = oracle.stvec(p, N)
        alpha = rz / float(p @ ap)
        x += alpha * p
        r -= alpha * ap
        rel = float(np.sqrt(r @ r)) / bn
        if rel < tol:
            return it, rel
        z = mg(oracle, r, N, params, degree)
        rz_new = float(r @ z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return max_iter, rel
