"""The shifted operator A_sigma = A_poisson + sigma I of gk_set_shift restated on host arrays.

TEST SUPPORT: the contract of include/gmres_hip.h's gk_set_shift.  The CPU oracle knows
sigma = 0 only, so the shifted operator gets a model of its own, pinned to the oracle bit for
bit at sigma = 0 (tests/test_shift_data.py) and compared with the device under np.array_equal
(tests/test_gpu_shift.py).

The rule.  With s = ((W + E) + N) + S (N: line j + 1, S: line j - 1, missing neighbours 0),

    y = fma(diag, c, -s),   diag = fl(4 + sigma)

ONE fused multiply-add, modelled exactly (fma): where diag is a power of two the product is
exact and diag * c - s is the same double; otherwise the correctly rounded value of the exact
diag c - s -- CPython's float(Fraction) per element (fma_fraction), or the same value by
error-free transformations on whole arrays with the Fraction as the fallback wherever their
result is not provably the correct rounding (fma; tests/test_shift_data.py holds the two
equal).  Everything on top -- cbpr2, the Chebyshev sweeps, the V-cycle, PCG -- is a single
IEEE operation per expression in the kernels' order.

Multigrid under a shift: level l runs sigma_l = 4^l sigma and smooths on the caller's interval
moved by sigma_l - sigma; the last level runs Chebyshev(nu_c) on its exact interval plus
sigma_L, nu_c recomputed from that interval.  `rule` and `fault` select the wrong rules and the
planted faults the CPU tests must tell apart from the right one.

Vectors are flat, i fastest: f(i, j) = f[j * N + i].
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from tests import mg_data

SPLIT = 134217729.0  # 2^27 + 1 (Veltkamp)


def diag_of(sigma: float) -> float:
    return 4.0 + float(sigma)


def is_pow2(x: float) -> bool:
    m, _ = math.frexp(x)
    return m == 0.5


def fma_fraction(a: float, c: np.ndarray, s: np.ndarray) -> np.ndarray:
    """round(a c - s) per element through exact rationals: the definition."""
    fa = Fraction(a)
    return np.array([float(fa * Fraction(float(x)) - Fraction(float(y))) for x, y in zip(c.ravel(), s.ravel())],
                    dtype=np.float64).reshape(c.shape)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma(a: float, c: np.ndarray, s: np.ndarray) -> np.ndarray:
    """round(a c - s), exactly one rounding per element."""
    c = np.ascontiguousarray(c, dtype=np.float64)
    s = np.ascontiguousarray(s, dtype=np.float64)
    if is_pow2(a):
        return a * c - s
    with np.errstate(all="ignore"):
        # a c = p + e exactly (Dekker), p - s = q + t exactly, t + e = w + w2 exactly,
        # q + w = r + err exactly: the exact value is r + err + w2
        p = a * c
        ah = a * SPLIT
        ah = ah - (ah - a)
        al = a - ah
        ch = c * SPLIT
        ch = ch - (ch - c)
        cl = c - ch
        e = ((ah * ch - p) + ah * cl + al * ch) + al * cl
        q, t = _two_sum(p, -s)
        w, w2 = _two_sum(t, e)
        r, err = _two_sum(q, w)
        # r = round(q + w) is round(q + w + w2) too when w2 cannot carry q + w across the
        # midpoint next to it; half the gap below a power of two is half the one above, so
        # those (and everything outside the range where the splittings are exact) go the slow way
        half = 0.5 * np.spacing(np.abs(r))
        mant = np.frexp(r)[0]
        in_range = (np.maximum(np.abs(p), np.abs(s)) < 1e290) & ((np.abs(c) > 1e-200) | (c == 0.0)) & (
            (np.abs(s) > 1e-200) | (s == 0.0))
        sure = in_range & ((w2 == 0.0) | ((np.abs(w2) < half - np.abs(err)) & (np.abs(mant) != 0.5)))
    out = r.copy()
    bad = ~sure
    if bad.any():
        out[bad] = fma_fraction(a, c[bad], s[bad])
    return out


def neighbour_sum(v: np.ndarray, N: int, lo=None, hi=None) -> np.ndarray:
    """((W + E) + N) + S on a slab of whole lines; lo / hi: the line below the first / above
    the last (None: the physical boundary)."""
    g = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, N)
    W = np.zeros_like(g)
    E = np.zeros_like(g)
    Np = np.zeros_like(g)
    Sm = np.zeros_like(g)
    W[:, 1:] = g[:, :-1]
    E[:, :-1] = g[:, 1:]
    Np[:-1, :] = g[1:, :]
    Sm[1:, :] = g[:-1, :]
    if hi is not None:
        Np[-1, :] = hi
    if lo is not None:
        Sm[0, :] = lo
    return ((W + E) + Np) + Sm


def stencil(v: np.ndarray, N: int, sigma: float, lo=None, hi=None, two_roundings: bool = False) -> np.ndarray:
    """A_sigma v.  two_roundings: the planted fault diag * c - s in two IEEE operations."""
    g = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, N)
    s = neighbour_sum(g, N, lo, hi)
    d = diag_of(sigma)
    y = (d * g - s) if two_roundings else fma(d, g, s)
    return y.reshape(-1)


def cbpr2_coeffs(params):
    em, eM = float(params[0]), float(params[1])
    cc = (eM - em) / 2.0
    d = (eM + em) / 2.0
    alpha = 1.0 / d
    beta = cc * alpha / 2.0
    beta = beta * beta
    return d, 1.0 / (d - beta)


def cbpr2(r: np.ndarray, N: int, sigma: float, params=(8.2, 0.2)) -> np.ndarray:
    """zp = r / d ; z = zp + alpha (r - A_sigma zp)   (chebyshev.f90:19-37)"""
    r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    d, alpha = cbpr2_coeffs(params)
    zp = r / d
    return zp + alpha * (r - stencil(zp, N, sigma))


def cheb(r: np.ndarray, N: int, sigma: float, params, degree: int, **kw) -> np.ndarray:
    """Chebyshev(degree) from a zero start, the per-sweep kernels' recurrence."""
    r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    theta = (float(params[0]) + float(params[1])) / 2.0
    delta = abs(float(params[1]) - float(params[0])) / 2.0
    sg = theta / delta
    rho0 = delta / theta
    res = r.copy()
    d = r / theta
    z = d.copy()
    for _ in range(degree):
        rho1 = 1.0 / (2.0 * sg - rho0)
        c1, c2 = rho1 * rho0, 2.0 * rho1 / delta
        res = res - stencil(d, N, sigma, **kw)
        d = c1 * d + c2 * res
        z = z + d
        rho0 = rho1
    return z


def coarse(NL: int, shift: float) -> tuple[float, float, int]:
    """mg_data.coarse with the level's shift: the interval moved by it, nu_c from the moved one."""
    t = math.pi / (2.0 * (NL + 1))
    lo = 8.0 * math.sin(t) * math.sin(t) + shift
    hi = 8.0 * math.cos(t) * math.cos(t) + shift
    sg = (hi + lo) / (hi - lo)
    ac = math.acosh(sg)
    for nu in range(1, 65):
        ch = math.cosh((nu + 1) * ac) if (nu + 1) * ac < 700.0 else math.inf
        if 1.0 / ch <= 0.1:
            return lo, hi, nu
    return lo, hi, 64


def level_shifts(sigma: float, nlev: int, rule: str = "4l") -> list[float]:
    f = {"4l": 4.0, "2l": 2.0, "4l-fixed-intervals": 4.0}[rule]
    out = [float(sigma)]
    for _ in range(1, nlev):
        out.append(out[-1] * f)
    return out


def nu_c(N: int, sigma: float) -> int:
    sides = mg_data.levels(N)
    return coarse(sides[-1], level_shifts(sigma, len(sides))[-1])[2]


def mg(r: np.ndarray, N: int, sigma: float, params=mg_data.DEFAULT_PARAMS, degree: int = mg_data.DEFAULT_DEGREE,
       rule: str = "4l", fault: str | None = None) -> np.ndarray:
    """out = MG_0(r) for A_sigma.  rule: "4l" (the contract), "2l" (sigma_l = 2^l sigma) or
    "4l-fixed-intervals" (the smoothers keep the caller's interval on every level).
    fault: None, "drop-level-1" (level 1 runs sigma_1 = 0), "two-roundings" (every stencil
    diag * c - s in two operations) or "stale-nuc" (the last level keeps sigma = 0's nu_c)."""
    sides = mg_data.levels(N)
    assert len(sides) >= 2, f"no coarse level for N = {N}"
    sh = level_shifts(sigma, len(sides), rule)
    if fault == "drop-level-1":
        sh[1] = 0.0
    return _cycle(np.ascontiguousarray(r, dtype=np.float64).reshape(-1), sides, sh, 0, params, degree, rule, fault)


def _cycle(r, sides, sh, l, params, degree, rule, fault):
    n, sl = sides[l], sh[l]
    kw = {"two_roundings": fault == "two-roundings"}
    if l == len(sides) - 1:
        lo, hi, nuc = coarse(n, sl)
        if fault == "stale-nuc":
            nuc = mg_data.coarse(n)[2]
        return cheb(r, n, sl, (lo, hi), nuc, **kw)
    mv = 0.0 if rule == "4l-fixed-intervals" else sl - sh[0]
    pl = (float(params[0]) + mv, float(params[1]) + mv)
    z = cheb(r, n, sl, pl, degree, **kw)
    rc = mg_data.restrict(r - stencil(z, n, sl, **kw), n)
    ec = _cycle(rc, sides, sh, l + 1, params, degree, rule, fault)
    z = mg_data.prolong_add(z, ec, n)
    t = r - stencil(z, n, sl, **kw)
    return z + cheb(t, n, sl, pl, degree, **kw)


def resid_restrict(r: np.ndarray, z: np.ndarray, N: int, sigma: float) -> np.ndarray:
    return mg_data.restrict(np.asarray(r, dtype=np.float64).reshape(-1) - stencil(z, N, sigma), N)


def rhs_ones(N: int, sigma: float) -> np.ndarray:
    return stencil(np.ones(N * N), N, sigma)


def pcg(oracle, N: int, sigma: float, params=None, degree: int = mg_data.DEFAULT_DEGREE, tol: float = 1e-8,
        max_iter: int = 200, rule: str = "4l", full: bool = False):
    """mg_data.pcg on A_sigma with b = A_sigma 1: the oracle's operation order for pcg_omp and
    its reductions.  params None: (8 + sigma, 1 + sigma).  Returns (iterations, relative
    residual), with full also x."""
    params = (8.0 + sigma, 1.0 + sigma) if params is None else params
    b = rhs_ones(N, sigma)
    x = np.zeros_like(b)
    r = b.copy()
    z = mg(r, N, sigma, params, degree, rule)
    p = z.copy()
    rz = oracle.dot(r, z)
    bn = oracle.norm2(b)
    it, rel = 0, 1.0
    for it in range(1, max_iter + 1):
        ap = stencil(p, N, sigma)
        alpha = rz / oracle.dot(ap, p)
        x = x + alpha * p
        r = r - alpha * ap
        rel = oracle.norm2(r) / bn
        if rel < tol:
            break
        z = mg(r, N, sigma, params, degree, rule)
        rz_new = oracle.dot(r, z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return (it, rel, x) if full else (it, rel)


def pbicgstab(oracle, N: int, sigma: float, iters: int, params=None, degree: int = mg_data.DEFAULT_DEGREE):
    """mg_data.pbicgstab on A_sigma with b = A_sigma 1, a fixed number of iterations: x."""
    params = (8.0 + sigma, 1.0 + sigma) if params is None else params
    b = rhs_ones(N, sigma)
    x = np.zeros_like(b)
    r = b.copy()
    r0 = r.copy()
    p = r.copy()
    for _ in range(iters):
        z1 = mg(p, N, sigma, params, degree)
        ap = stencil(z1, N, sigma)
        rr0 = oracle.dot(r, r0)
        alpha = rr0 / oracle.dot(ap, r0)
        s = r - alpha * ap
        z2 = mg(s, N, sigma, params, degree)
        as_ = stencil(z2, N, sigma)
        omega = oracle.dot(as_, s) / oracle.dot(as_, as_)
        x = (x + alpha * z1) + omega * z2
        r = s - omega * as_
        beta = (oracle.dot(r, r0) / rr0) * (alpha / omega)
        p = r + beta * (p - omega * ap)
    return x


def gmres(N: int, sigma: float, iters: int, side: str, params=None, degree: int = mg_data.DEFAULT_DEGREE):
    """One cycle of `iters` MGS Arnoldi steps of multigrid-preconditioned GMRES on A_sigma from
    x0 = 0 with b = A_sigma 1 (left: M^-1 A; right: A M^-1, x = M^-1 V y): x.  float64 numpy;
    it measures the error a solve has at that iteration count, not the device's bits."""
    params = (8.0 + sigma, 1.0 + sigma) if params is None else params
    b = rhs_ones(N, sigma)

    def minv(v):
        return mg(v, N, sigma, params, degree)

    r0 = minv(b) if side == "left" else b
    beta = float(np.linalg.norm(r0))
    V = [r0 / beta]
    H = np.zeros((iters + 1, iters))
    for j in range(iters):
        w = minv(stencil(V[j], N, sigma)) if side == "left" else stencil(minv(V[j]), N, sigma)
        for _ in range(2):
            for i in range(j + 1):
                d = float(np.dot(w, V[i]))
                w = w - d * V[i]
                H[i, j] += d
        H[j + 1, j] = float(np.linalg.norm(w))
        V.append(w / H[j + 1, j])
    g = np.zeros(iters + 1)
    g[0] = beta
    y = np.linalg.lstsq(H, g, rcond=None)[0]
    t = np.asarray(V[:iters]).T @ y
    return t if side == "left" else minv(t)


def asym(N: int, seed: int, nlines: int | None = None) -> np.ndarray:
    """A seeded Gaussian vector: invariant under none of the square's symmetries
    (general_data.assert_asymmetric holds it to that on whole grids)."""
    from tests import general_data

    nl = N if nlines is None else nlines
    v = np.random.default_rng(seed).standard_normal(N * nl)
    if nl == N:
        general_data.assert_asymmetric(v, N)
    return v
