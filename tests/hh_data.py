"""Planted Householder reflectors and the long-double Householder step they are checked
against (test infrastructure for tests/test_gpu_hh_step_known_answer.py and
tests/test_hh_data.py).

Every other Householder check is a residual history of a b = A*1 or general-b solve held to
relative tiers (1e-8 / 1e-3 / 5e-2): GMRES corrects a slightly wrong H at the next restart, so
such a history cannot see a step that is wrong in its last ten digits.  Here the reflector
columns P_1..P_m are planted and ONE step of gmres_hh.f90:255-321 is compared with its
long-double evaluation on the same float64 reflectors.

Indices: step j is 1-based (gk_hh_step); vectors are 0-based, so reflector P_i (row i - 1) is
zero below index i - 1, v_j = P_1..P_j e_j has its unit entry at index j - 1, the Hessenberg
column is h[0..j] with h[:j] = w[:j], and the new reflector P_{j+1} has its pivot at index j.
"""
from __future__ import annotations

import numpy as np

from tests.general_data import EPS, MARGIN, assert_asymmetric, asymmetry, locate

SIGN_GUARD = 2.0 ** 20  # |w_j| before the fix-up, in units of the h bound
# Seed base of reflectors().  The guards and the CPU pins (test_hh_data.py: a correct float64 step
# below 1/8 of every bound) decide on the seed, never on a bound -- but the pin on the REST bound
# is a statement about these seeds, not about every seed: that ratio is a maximum over n
# roundings, measured against the largest of n small entries, and it has a tail.  Of the bases
# 7000, 7100 .. 7900 only 7100 keeps all ~50 pinned evaluations below 1/8; each of the others
# leaves one to four of them between 0.126 and 0.30 of the rest bound (7000: N = 130, j = 1 at
# 0.135 .. 0.151; 7500 also one rebuilt column at 0.19), and three miss an asymmetry guard at
# N = 2.  The step's h and pivot ratios stayed below 1/8 at every base.  So a correct step can sit
# at 0.3 of the rest bound; a device deviation near that on other data is rounding, one near 1
# is not.
SEED0 = 7100

# (N, m) of the launch-path cases: (2, 3) with j = 3 puts the tail on the vector's last element,
# (3, 5) and (45, 12) are odd n
LAUNCH_SHAPES = [(2, 3), (3, 5), (45, 12), (130, 6)]
PREC_SHAPES = [(45, 12), (181, 16)]      # launch path; w-only fused chain
VEC_SHAPES = [(45, 12), (181, 16)]       # gk_hh_update_x / gk_hh_verr: launch path; w-only chains

_P: dict = {}
_refs: dict = {}


def launch_js(m: int) -> list[int]:
    return sorted({1, 2, m} | ({5} if m >= 5 else set()))


def resident_js(m: int) -> list[int]:
    return sorted({1, 2, 5, m})


# The reflection chains of the w-only variant keep 90 register + 38 LDS chunks of 256 double2 per
# workgroup, so none of test_gpu_resident.HCASES reaches their LDS part (N = 300 on 4 workgroups:
# 44 register chunks each).  Two workgroups (share 128) at these sizes hold 90 register chunks
# each, then LDS chunks, and stream the rest: N, m, r2 cap, share, w-only.
WONLY_LDS_CASES = [(512, 24, 12, 128, 1),   # 90 + 38 chunks per workgroup, half the vector streamed
                   (333, 16, 12, 128, 1)]   # odd n: 90 + 18, 148 double2 and the last element streamed


def resident_shapes() -> list[tuple[int, int]]:
    """(N, m) of the forcing tuples of test_gpu_resident.HCASES / HPCASES and WONLY_LDS_CASES."""
    from tests import test_gpu_resident as tr

    return sorted({(c[0], c[1]) for c in tr.HCASES + tr.HPCASES + WONLY_LDS_CASES})


def all_cases() -> list[tuple[int, int, int]]:
    """Every (N, m, j) the GPU tests run (three ranks: (130, 6), j in launch_js)."""
    out = {(N, m, j) for N, m in LAUNCH_SHAPES for j in launch_js(m)}
    out |= {(N, m, j) for N, m in resident_shapes() for j in resident_js(m)}
    return sorted(out)


def reflectors(N: int, m: int) -> np.ndarray:
    """The planted reflectors of an (N, m) context; once per shape."""
    if (N, m) not in _P:
        _P[(N, m)] = planted_reflectors(N, m, seed=SEED0 + 7 * N + m)
    return _P[(N, m)]


def reference(oracle, N: int, m: int, j: int, precondition: bool = False):
    """hh_reference of step j on reflectors(N, m); once per case."""
    key = (N, m, j, bool(precondition))
    if key not in _refs:
        _refs[key] = hh_reference(oracle, reflectors(N, m), j, N, precondition)
    return _refs[key]


def planted_reflectors(N: int, m: int, seed: int) -> np.ndarray:
    """m rows of length N^2; row k is reflector P_{k+1}: zeros at indices < k, a pivot entry
    at index k of magnitude sqrt(0.5 + 0.4 u) (u uniform in [0, 1), random sign: the pivot of
    a reflector built by gmres_hh.f90:306-318 is >= 1/sqrt(2) in magnitude), seeded Gaussian
    for the rest, scaled so that the row has unit norm in float64."""
    n = N * N
    assert 1 <= m < n
    rng = np.random.default_rng(seed)
    P = np.zeros((m, n))
    for k in range(m):
        piv = np.sqrt(0.5 + 0.4 * rng.random()) * (1.0 if rng.random() < 0.5 else -1.0)
        g = rng.standard_normal(n - k - 1)
        P[k, k] = piv
        P[k, k + 1:] = g * (np.sqrt(1.0 - piv * piv) / np.linalg.norm(g))
        P[k] /= np.linalg.norm(P[k])
    return P


def stencil(v: np.ndarray, N: int) -> np.ndarray:
    """y = A v, the 5-point operator of poisson.f90:33-77 (4 v - the neighbours, zeros outside
    the square; index = i + j N), in v's dtype."""
    g = np.asarray(v).reshape(N, N)
    s = np.zeros_like(g)
    s[:, 1:] += g[:, :-1]
    s[:, :-1] += g[:, 1:]
    s[1:, :] += g[:-1, :]
    s[:-1, :] += g[1:, :]
    return (4 * g - s).reshape(-1)


def hh_step(P: np.ndarray, j: int, apply, dtype=np.longdouble, dot=np.dot, norm2=None):
    """gmres_hh.f90:255-321 in `dtype` with `dot` (norms: `norm2`, default sqrt(dot(x, x))), on
    the rows P[0..j-1] as given:
    v = P_1..P_j e_j; w = apply(v); w = P_j..P_1 w; h[:j] = w[:j]; tmp = ||w[j:]||;
    h[j] = -tmp if w[j] > 0 else tmp; w[:j] = 0; w[j] -= h[j]; p = w / ||w||.
    Returns (h, p, ||w0||, v, w[j] before the fix-up) in `dtype`."""
    if norm2 is None:
        def norm2(x):
            return np.sqrt(dot(x, x))
    Pd = np.asarray(P[:j], dtype=dtype)
    n = Pd.shape[1]
    v = np.zeros(n, dtype=dtype)
    v[j - 1] = 1
    for i in range(j, 0, -1):
        v = v - (2 * dot(v, Pd[i - 1])) * Pd[i - 1]
    w = np.asarray(apply(v), dtype=dtype).copy()
    nw0 = norm2(w)
    for i in range(1, j + 1):
        w = w - (2 * dot(w, Pd[i - 1])) * Pd[i - 1]
    h = np.zeros(j + 1, dtype=dtype)
    h[:j] = w[:j]
    tmp = norm2(w[j:])
    wj = w[j]
    h[j] = -tmp if wj > 0 else tmp
    w[:j] = 0
    w[j] = w[j] - h[j]
    return h, w / norm2(w), nw0, v, wj


def hh_step_ld(P: np.ndarray, j: int, N: int, apply=None):
    """The long-double step; apply defaults to the long-double stencil.  Returns
    (h, p, ||w0||, v, w_j before the fix-up) rounded to float64."""
    ap = apply if apply is not None else (lambda v: stencil(v, N))
    h, p, nw0, v, wj = hh_step(P, j, ap)
    return h.astype(np.float64), p.astype(np.float64), float(nw0), v.astype(np.float64), float(wj)


def hh_bounds(ref, j: int):
    """(bound on |h_i - h_ref_i|, on |p[j] - p_ref[j]|, on max |p[j+1:] - p_ref[j+1:]|):
    64 eps ||w0|| (the reflections keep the norm), 64 eps |p_ref[j]| and
    64 eps max |p_ref[j+1:]| -- the column is spiky at its pivot (0.7 .. 1 against ~1/N)."""
    p = ref[1]
    rest = float(np.max(np.abs(p[j + 1:]))) if p.size > j + 1 else 0.0
    return MARGIN * EPS * ref[2], MARGIN * EPS * abs(float(p[j])), MARGIN * EPS * rest


def hh_ratios(h, p, ref, j: int):
    """(h, pivot, rest) deviation over bound of one evaluation against `ref`; the leading
    zeros of p are not part of it (check_hh_step asserts them)."""
    hb, pb, rb = hh_bounds(ref, j)
    rest = float(np.max(np.abs(p[j + 1:] - ref[1][j + 1:])) / rb) if p.size > j + 1 else 0.0
    return float(np.max(np.abs(np.asarray(h) - ref[0])) / hb), float(abs(p[j] - ref[1][j]) / pb), rest


def hh_reference(oracle, P: np.ndarray, j: int, N: int, precondition: bool = False):
    """hh_step_ld of step j with the guards of the construction: v and w0 carry none of the
    square's symmetries, and w_j before the fix-up is 2^20 h-bounds away from zero, so the
    device and the reference take the same sign for h[j].  precondition: w0 =
    cbpr2(A float64(v)) through the oracle (bit-exact with the device on equal input)."""
    ap = None
    if precondition:
        def ap(v):
            return oracle.precond(oracle.PREC_CBPR2, oracle.stvec(np.asarray(v, dtype=np.float64), N), N)
    ref = hh_step_ld(P, j, N, ap)
    v = ref[3]
    w0 = ap(v) if precondition else oracle.stvec(v, N)
    if not precondition:  # the long-double stencil is the oracle's operator: four roundings of terms <= 4 max|v|
        assert np.max(np.abs(stencil(v.astype(np.longdouble), N).astype(np.float64) - w0)) <= 16 * EPS * np.max(np.abs(v))
    e = np.zeros(N * N)
    e[j - 1] = 1.0
    foot = stencil(e, N) != 0.0
    assert_bulk_asymmetric(v, N, e != 0.0)
    assert_bulk_asymmetric(w0, N, foot)
    if j > 1:
        assert_asymmetric(v, N)
        assert_asymmetric(w0, N)
    assert abs(ref[4]) > SIGN_GUARD * MARGIN * EPS * ref[2], (N, j, ref[4], ref[2])  # change the seed, not the bound
    return ref


def assert_bulk_asymmetric(x: np.ndarray, N: int, spike: np.ndarray) -> None:
    """assert_asymmetric on the scale of the entries off `spike`.  v_j = P_1..P_j e_j keeps an
    entry 1 - 2 P_j(j)^2 (down to -0.8) at index j - 1 over a bulk of ~1/N, and A v_j carries
    it on the stencil's footprint.  At j = 1 that index is the corner, which the transposition
    maps to itself, so there the asymmetry under transposition is the bulk's alone and cannot
    reach a tenth of the spike once N is large (0.02 .. 0.08 of it at N = 181 .. 512): it is
    held to a tenth of the bulk's largest entry instead, for every j."""
    lim = 0.1 * float(np.max(np.abs(x[~spike])))
    a = asymmetry(x, N)
    assert min(a) > lim, (a, lim)


def check_hh_step(h, p, ref, j: int, what: str = "", plan=None):
    """Assert one device step against `ref` within hh_bounds, and p[:j] == 0 exactly; returns
    the (h, pivot, rest) ratios of deviation to bound.  On failure the message names the
    entries of h that are off, and the first and last bad index of the column with their chunk
    and workgroup under `plan`."""
    h, p = np.asarray(h), np.asarray(p)
    hb, pb, rb = hh_bounds(ref, j)
    r = hh_ratios(h, p, ref, j)
    print(f"{what}: h dev/bound {r[0]:.3e}, pivot dev/bound {r[1]:.3e}, rest dev/bound {r[2]:.3e}")
    dh = np.abs(h - ref[0])
    bad_h = np.nonzero(~(dh <= hb))[0]
    assert bad_h.size == 0, f"{what}: h entries {bad_h.tolist()} off: got {h[bad_h]} ref {ref[0][bad_h]} bound {hb:.3e}"
    nz = np.nonzero(p[:j] != 0.0)[0]
    assert nz.size == 0, f"{what}: column not zero at {nz.tolist()} (below the pivot {j}): {p[nz]}"
    dp = np.abs(p - ref[1])
    lim = np.full(p.size, rb)
    lim[:j] = 0.0
    lim[j] = pb
    bad = np.nonzero(~(dp <= lim))[0]
    assert bad.size == 0, (f"{what}: new reflector off at {bad.size} elements, first {bad[0]} ({locate(bad[0], plan)}), "
                           f"last {bad[-1]} ({locate(bad[-1], plan)}), pivot {j}: dev {dp[j]:.3e} bound {pb:.3e}, "
                           f"rest: max dev {dp[j + 1:].max() if p.size > j + 1 else 0.0:.3e} bound {rb:.3e}")
    return r


def chain_down_ld(P: np.ndarray, v: np.ndarray, k: int, dtype=np.longdouble, dot=np.dot) -> np.ndarray:
    """P_1 .. P_k v (reflections k..1; gmres_hh.f90:269-283, :361-373, :581-585) in `dtype`."""
    Pd = np.asarray(P[:k], dtype=dtype)
    v = np.asarray(v, dtype=dtype).copy()
    for i in range(k, 0, -1):
        v = v - (2 * dot(v, Pd[i - 1])) * Pd[i - 1]
    return v


def update_x_ld(P: np.ndarray, x: np.ndarray, y: np.ndarray, dtype=np.longdouble, dot=np.dot) -> np.ndarray:
    """x + P_1 .. P_m [y; 0] (gmres_hh.f90:356-375), m = len(y)."""
    w = np.zeros(P.shape[1], dtype=dtype)
    w[: y.size] = y
    return np.asarray(x, dtype=dtype) + chain_down_ld(P, w, y.size, dtype, dot)


def vec_data(N: int, m: int):
    """(x, y) of the gk_hh_update_x cases: a seeded Gaussian x without the symmetries and a
    seeded y of length n_out = m."""
    rng = np.random.default_rng(9000 + 7 * N + m)
    x = rng.standard_normal(N * N)
    assert_asymmetric(x, N)
    return x, rng.standard_normal(m)


def rebuilt_ld(P: np.ndarray, k: int) -> np.ndarray:
    """Column k (1-based) of the basis gk_hh_verr rebuilds, P_1 .. P_k e_k, rounded to float64."""
    e = np.zeros(P.shape[1])
    e[k - 1] = 1.0
    return chain_down_ld(P, e, k).astype(np.float64)


def rebuilt_ratios(v: np.ndarray, v_ref: np.ndarray, k: int):
    """Deviation over bound of a rebuilt column: (every element against 64 eps max |v_ref|,
    the elements off index k - 1 against 64 eps max |v_ref off k - 1|).  The column keeps
    1 - 2 P_k(k)^2 at index k - 1 over a bulk of ~1/N, so the first bound alone would let the
    bulk be off by N roundings wherever that entry is large."""
    d = np.abs(np.asarray(v) - v_ref)
    off = np.arange(v_ref.size) != k - 1
    return (float(np.max(d) / (MARGIN * EPS * np.max(np.abs(v_ref)))),
            float(np.max(d[off]) / (MARGIN * EPS * np.max(np.abs(v_ref[off])))))


def update_x_bound(x: np.ndarray, y: np.ndarray) -> float:
    """64 eps (max |x| + ||y||) per element: the chain keeps ||[y; 0]||."""
    return MARGIN * EPS * (float(np.max(np.abs(x))) + float(np.linalg.norm(y)))


# ------------------------------------------------------------- device planting --

def hh_start(c, P: np.ndarray, precondition: bool = False) -> None:
    """Open a Householder cycle on context c (cbpr2 on the left when preconditioned; collective
    on N ranks) and plant its slab P[k] of every reflector column k.  gk_set_x and
    gk_vec_lincomb do not close a Householder cycle (cycle_hh, gk_hh.hip), and every chain
    reads its reflectors from HBM."""
    import ctypes

    from gmres_amd import _native as nat
    from tests.general_data import plant

    c.set_precond("cbpr2" if precondition else "identity", (8.2, 0.2), side="left")
    c.set_rhs_ones()
    g1 = ctypes.c_double()
    nat.check(nat.hip().gk_hh_cycle_start(c.handle, int(precondition), ctypes.byref(g1)), "gk_hh_cycle_start")
    for k in range(P.shape[0]):
        plant(c, k, P[k])


def hh_open(N: int, m: int, tunes, precondition: bool = False):
    """A context with its tuning applied, a Householder cycle open and reflectors(N, m) planted."""
    import gmres_amd as ga

    c = ga.Context(N, m)
    try:
        for k, v in tunes:
            c.tune(k, v)
        hh_start(c, reflectors(N, m), precondition)
    except Exception:
        c.close()
        raise
    return c


def hh_dev_step(c, j: int, precondition: bool = False, split: bool = False):
    """gk_hh_step(j) (split: gk_hh_step_async then gk_hh_step_wait): (h[0..j], column j)."""
    from gmres_amd import _native as nat

    L = nat.hip()
    h = np.zeros(c.m + 2)
    hp = h.ctypes.data_as(nat._dp)
    if split:
        nat.check(L.gk_hh_step_async(c.handle, j, int(precondition)), "gk_hh_step_async")
        nat.check(L.gk_hh_step_wait(c.handle, j, hp), "gk_hh_step_wait")
    else:
        nat.check(L.gk_hh_step(c.handle, j, int(precondition), hp), "gk_hh_step")
    return h[: j + 1].copy(), c.get_basis(j, 0)
