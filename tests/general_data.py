"""Data without the square's symmetries, and the long-double Arnoldi step they are
checked against (test infrastructure for tests/test_gpu_step_known_answer.py,
tests/test_gpu_cb_step_known_answer.py and tests/test_gpu_general_rhs.py).

The Poisson 5-point operator, cbpr2 and Chebyshev(k) commute with the eight symmetries
of the square and b = A*1 is invariant under all of them, so every Krylov vector of a
set_rhs_ones() solve equals its own index reversal, its transposed grid and its grid
with the lines reversed.  A kernel that walks a vector from the wrong end reproduces
such a solve bit for bit.  The vectors built here are invariant under none of them.
"""
from __future__ import annotations

import numpy as np

from tests import mg_data

EPS = 2.0 ** -52
MARGIN = 64.0  # over the first-order rounding error of one dot, eps ||w|| ||v||


def asymmetry(v: np.ndarray, N: int) -> tuple[float, float, float]:
    """max |v - S v| for S = index reversal, transposition, line reversal."""
    g = np.asarray(v).reshape(N, N)
    return (float(np.max(np.abs(g - g[::-1, ::-1]))), float(np.max(np.abs(g - g.T))),
            float(np.max(np.abs(g - g[::-1, :]))))


def assert_asymmetric(v: np.ndarray, N: int) -> None:
    if N < 2:
        return
    lim = 0.1 * float(np.max(np.abs(v)))
    a = asymmetry(v, N)
    assert min(a) > lim, (a, lim)


def general_rhs(oracle, N: int, seed: int):
    """(x_true, b = A x_true) for a seeded Gaussian x_true; b has none of the symmetries."""
    x_true = np.random.default_rng(seed).standard_normal(N * N)
    b = oracle.stvec(x_true, N)
    assert_asymmetric(b, N)
    return x_true, b


def planted_basis(N: int, j: int, seed: int, pert: float = 1e-3) -> np.ndarray:
    """j rows of length N^2 (row k = Krylov column k): an orthonormal set plus a Gaussian
    perturbation of norm ~pert each.  The Gram matrix is off the identity by about pert / N
    (1e-5 .. 1e-6 at the test sizes, ten orders above rounding), so both MGS passes and the
    norm carry signal, and the step's error amplification stays near 1."""
    n = N * N
    assert 1 <= j <= n
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, j)))
    G = rng.standard_normal((n, j))
    return np.ascontiguousarray((Q + pert * G / np.sqrt(n)).T)


def mgs_step_ld(V: np.ndarray, w0: np.ndarray):
    """gmres_mgsr.f90:341-363 in long double: two sequential passes over the rows of V
    (d = <w, V_i>; w -= d V_i; h_i += d), h_{j+1} = ||w||, the new column w / h_{j+1}.
    Returns (h[0..j], v_new) rounded to float64."""
    ld = np.longdouble
    Vl = np.asarray(V, dtype=ld)
    w = np.asarray(w0, dtype=ld).copy()
    j = Vl.shape[0]
    h = np.zeros(j + 1, dtype=ld)
    for _ in range(2):
        for i in range(j):
            d = np.dot(w, Vl[i])
            w = w - d * Vl[i]
            h[i] += d
    h[j] = np.sqrt(np.dot(w, w))
    return h.astype(np.float64), (w / h[j]).astype(np.float64)


def blocked_step(V: np.ndarray, w0: np.ndarray, S: int, dtype=np.longdouble, dot=np.dot):
    """The blocked step k_mgs_blk takes (gmres_amd/csrc/gk_blk.hpp, gk_blk.hip), evaluated in
    `dtype` with `dot`: per sweep the blocks {V_1}, {V_2..V_{S+1}}, ...; a block's dots
    z_k = <w, V_k> all on the w before the block's AXPYs, h_k = z_k - sum_{l<k} h_l <V_l, V_k>
    in l order, then w = ((w - h_1 V_1) - h_2 V_2) - ...; h summed over the two sweeps.  The
    second sweep visits the blocks in REVERSE order (S > 1; its first block is the one still on
    chip): on exactly orthonormal columns its h are 0 in any order, on the planted columns the
    result differs from the strict step's at second order in the Gram off-diagonals.
    S = 1 is the strict step.  Returns (h[0..j], v_new) rounded to float64."""
    Vd = np.asarray(V, dtype=dtype)
    w = np.asarray(w0, dtype=dtype).copy()
    j = Vd.shape[0]
    blocks = [[0]] + [list(range(s, min(s + S, j))) for s in range(1, j, S)]
    h = np.zeros(j + 1, dtype=dtype)
    for sweep in range(2):
        for blk in (blocks if sweep == 0 or S == 1 else blocks[::-1]):
            hn = []
            for k, ck in enumerate(blk):
                hk = dot(w, Vd[ck])
                for l in range(k):
                    hk = hk - hn[l] * dot(Vd[blk[l]], Vd[ck])
                hn.append(hk)
            for hk, ck in zip(hn, blk):
                w = w - hk * Vd[ck]
                h[ck] += hk
    h[j] = np.sqrt(dot(w, w))
    return h.astype(np.float64), (w / h[j]).astype(np.float64)


def step_bounds(V: np.ndarray, w0: np.ndarray, v_ref: np.ndarray):
    """(bound on |h_i - h_ref_i| for i = 0..j, bound on max |v_new - v_ref|):
    64 eps ||w0|| ||V_i|| (||.|| = 1 for h_{j+1}) and 64 eps max |v_ref|."""
    nw = float(np.linalg.norm(w0))
    nv = np.append(np.linalg.norm(V, axis=1), 1.0)
    return MARGIN * EPS * nw * nv, MARGIN * EPS * float(np.max(np.abs(v_ref)))


def locate(e: int, plan) -> str:
    """Where element e of a slab lives under a resident plan (gk_res_info): its chunk, and the
    workgroup that holds the chunk in registers or LDS, or the streamed part."""
    if not plan or not plan.get("variant"):
        return f"512-element chunk {e // 512}"
    dt = plan["wt"] - 64 if plan["cw"] else plan["wt"]  # double2 per chunk (a control wave holds none)
    ch, G, r, l = (e // 2) // dt, plan["G"], plan["r2e"], plan["l2e"]
    if e // 2 >= plan["nres2"]:
        part = "streamed part"
    elif ch < G * r:
        part = f"registers of workgroup {ch // r}"
    else:
        part = f"LDS of workgroup {(ch - G * r) // l}" if l else "past the register chunks"
    return f"chunk {ch} of {dt} double2, {part}"


def check_step(h, v_new, V, w0, ref=None, what="", bounds=None, plan=None):
    """Assert one device step against mgs_step_ld (or `ref`) within step_bounds (or `bounds`);
    returns the largest (h, column) ratio of deviation to bound.  On failure the message names
    the entries of h that are off, and the first and last bad index of the new column with
    their chunk and workgroup under `plan`."""
    h_ref, v_ref = ref if ref is not None else mgs_step_ld(V, w0)
    hb, vb = bounds if bounds is not None else step_bounds(V, w0, v_ref)
    dh = np.abs(np.asarray(h) - h_ref)
    dv = np.abs(np.asarray(v_new) - v_ref)
    rh, rv = float(np.max(dh / hb)), float(np.max(dv) / vb)
    print(f"{what}: h dev/bound {rh:.3e}, column dev/bound {rv:.3e}")
    bad_h = np.nonzero(dh > hb)[0]
    assert bad_h.size == 0, f"{what}: h entries {bad_h.tolist()} off: got {np.asarray(h)[bad_h]} ref {h_ref[bad_h]} bound {hb[bad_h]}"
    bad_v = np.nonzero(dv > vb)[0]
    assert bad_v.size == 0, (f"{what}: new column off at {bad_v.size} elements, first {bad_v[0]} "
                             f"({locate(bad_v[0], plan)}), last {bad_v[-1]} ({locate(bad_v[-1], plan)}), "
                             f"max dev {dv.max():.3e} bound {vb:.3e}")
    return rh, rv


# ------------------------------------- preconditioned steps, both basis formats ---

PARAMS = (8.2, 0.2)
MG_PARAMS, MG_DEGREE = mg_data.DEFAULT_PARAMS, mg_data.DEFAULT_DEGREE  # (8.0, 1.0), 2
# (id, side, preconditioner, degree, tunes by name, N, m, params): the step's first dot comes
# from the operator launch's epilogue; steps j = 1, 2, m on the launch path and on one resident
# plan (test_gpu_step_known_answer.py on FP64 columns, test_gpu_cb_step_known_answer.py on FP32,
# test_gpu_cgs2_step_known_answer.py in front of the CGS2 chain).  The multigrid rows: on the
# left the cycle's closing add carries the dot (k_mg_add<ACC_DOT>); 48 has three levels,
# 130 a coarse side of 65 (odd, and a wave seam at fine column 128), 256 six levels.
PREC_STEP_CASES = (
    [(f"left-cbpr2-{N}", "left", "cbpr2", 1, (), N, 6, PARAMS) for N in (45, 130)]
    + [(f"left-cheb{d}-sten{s}-{N}", "left", "cheb", d, (("GK_TUNE_CHEB_STEN", s),), N, 6, PARAMS)
       for d, N in ((4, 130), (8, 130), (4, 256), (8, 256), (11, 130), (4, 45)) for s in (1, 0)]
    + [(f"right-cbpr2-fused{f}-{N}", "right", "cbpr2", 1, (("GK_TUNE_RIGHT_FUSED", f),), N, 6, PARAMS)
       for N in (65, 130) for f in (1, 0)]
    + [("right-cheb3-130", "right", "cheb", 3, (), 130, 6, PARAMS)]
    + [(f"left-mg-{N}", "left", "mg", MG_DEGREE, (), N, 6, MG_PARAMS) for N in (48, 130, 256)]
    + [(f"right-mg-{N}", "right", "mg", MG_DEGREE, (), N, 6, MG_PARAMS) for N in (48, 130)])


def op_w0(oracle, v: np.ndarray, N: int, side: str = "left", prec: str = "identity", degree: int = 1,
          params=PARAMS) -> np.ndarray:
    """The operator stage of a step on the oracle (bit-exact with the device operators,
    test_gpu_kernels.py / test_gpu_right_precond.py; "mg": the restated V-cycle, test_gpu_mg.py):
    M^-1 A v on the left, A M^-1 v on the right."""
    if prec == "identity":
        return oracle.stvec(v, N)
    if prec == "mg":
        return mg_data.op_mg(oracle, v, N, side, params, degree)
    kind = {"cbpr2": oracle.PREC_CBPR2, "cheb": oracle.PREC_CHEB}[prec]
    if side == "right":
        return oracle.stvec(oracle.precond(kind, v, N, params=params, degree=degree), N)
    return oracle.precond(kind, oracle.stvec(v, N), N, params=params, degree=degree)


def stencil_any(v: np.ndarray, N: int) -> np.ndarray:
    """A v for the 5-point operator (4 v - the neighbours, zeros outside the square; index
    i + j N) in v's dtype: long double in, long double out."""
    g = np.asarray(v).reshape(N, N)
    s = np.zeros_like(g)
    s[:, 1:] += g[:, :-1]
    s[:, :-1] += g[:, 1:]
    s[1:, :] += g[:-1, :]
    s[:-1, :] += g[1:, :]
    return (4 * g - s).reshape(-1)


def cbpr2_ld(oracle, t: np.ndarray, N: int) -> np.ndarray:
    """M^-1 t of cbpr2 (chebyshev.f90:19-38: z = t / d; z + alpha (t - A z)) in long double,
    with the float64 coefficients the device uses."""
    d, alpha = oracle.cbpr2_coeffs(PARAMS)
    tl = np.asarray(t, dtype=np.longdouble)
    z = tl / np.longdouble(d)
    return z + np.longdouble(alpha) * (tl - stencil_any(z, N))


def cbpr2_abs(oracle, u: np.ndarray, N: int) -> np.ndarray:
    """|M^-1| u for u >= 0, term by term as cbpr2 evaluates it: u / d + |alpha| (u + |A| (u / d)),
    |A| u = 8 u - A u (4 u + the neighbours).  The magnitude every rounding of one cbpr2
    application, and every error of its input, is measured against."""
    d, alpha = oracle.cbpr2_coeffs(PARAMS)
    z = np.asarray(u, dtype=np.float64) / abs(d)
    return z + abs(alpha) * (u + (8.0 * z - stencil_any(z, N)))


# ------------------------------------------- FP32-compressed basis (gk_cb.hip) ---

# The cases of tests/test_gpu_cb_step_known_answer.py, shared with the CPU pins of
# tests/test_cb_step_data.py so that every (N, m, j) run on the device is pinned here first.
CB_LAUNCH_SHAPES = [(2, 3), (3, 5), (45, 12), (130, 6)]  # steps j = 1, 2, m
CB_RES_M, CB_RES_JS = 8, (1, 2, 5, 8)
# (N, workgroups, plan of k_mgs_wcb on those workgroups: r2e, l2e, streamed double2, odd n)
CB_RES_PLANS = [(23, 1, 1, 0, 8, True), (45, 1, 3, 0, 244, True),
                (130, 1, 33, 0, 2, False), (130, 2, 17, 0, 2, False), (130, 4, 9, 0, 2, False),
                (130, 16, 3, 0, 2, False),
                (259, 1, 90, 39, 516, True), (309, 2, 90, 3, 124, True), (320, 2, 90, 10, 0, False),
                (512, 8, 64, 0, 0, False)]

_cb_basis: dict = {}


def planted_basis_f32(N: int, j: int, seed: int) -> np.ndarray:
    """planted_basis rounded once to float32 (dtype float32).  The rounding moves the Gram
    matrix by ~1e-8; immaterial, the reference consumes the same float values."""
    return planted_basis(N, j, seed).astype(np.float32)


def cb_planted(N: int, m: int) -> np.ndarray:
    """The float columns (widened to float64, rows 0..m-1) every FP32-basis test of an (N, m)
    context plants; once per shape."""
    if (N, m) not in _cb_basis:
        _cb_basis[(N, m)] = planted_basis_f32(N, m, seed=7000 + 7 * N + m).astype(np.float64)
    return _cb_basis[(N, m)]


def cb_step_ld(V32: np.ndarray, w0: np.ndarray):
    """mgs_step_ld on the widened float columns.  Returns (h[0..j] as float64, the new
    column w / h_{j+1} UNROUNDED, in long double): what the device must round once."""
    ld = np.longdouble
    Vl = np.asarray(V32).astype(ld)  # float32 / float64 -> long double is exact
    w = np.asarray(w0, dtype=ld).copy()
    j = Vl.shape[0]
    h = np.zeros(j + 1, dtype=ld)
    for _ in range(2):
        for i in range(j):
            d = np.dot(w, Vl[i])
            w = w - d * Vl[i]
            h[i] += d
    h[j] = np.sqrt(np.dot(w, w))
    return h.astype(np.float64), w / h[j]


def ulp32(x: np.ndarray) -> np.ndarray:
    """The spacing of float32 in the binade of |x| (x of any precision; 2^-149 at and below
    the subnormals): a correctly rounded float32(x) lies within half of it."""
    ax = np.abs(np.asarray(x, dtype=np.longdouble))
    _, e = np.frexp(ax)  # |x| = f 2^e, f in [0.5, 1) (e = 0 for x = 0)
    return np.ldexp(1.0, np.where(ax == 0, -149, np.maximum(e - 24, -149)))


def cb_column_excess(stored: np.ndarray, v_ref: np.ndarray):
    """(|stored - v_ref| - ulp32(v_ref) / 2) / vb per element, vb = 64 eps max |v_ref|: <= 1
    where the stored value is a round-to-nearest of some value within the FP64 step bound of
    the reference, <= 0 where it needs none of that allowance; and vb."""
    vb = MARGIN * EPS * float(np.max(np.abs(v_ref)))
    dev = np.abs(np.asarray(stored).astype(np.longdouble) - v_ref)
    return ((dev - 0.5 * ulp32(v_ref)) / vb).astype(np.float64), vb


def locate_cb(e: int, plan, n: int) -> str:
    """Where element e of an n-element slab lives in k_mgs_wcb under `plan` (gk_res_info of an
    FP32-basis context): its chunk of 256 double2, the workgroup, whether the chunk is held in
    registers or LDS and as half of a float4 pair or alone, and the lane; or the streamed
    part / the odd tail element."""
    if not plan or not plan.get("variant"):
        return f"512-element chunk {e // 512}"
    WT, G, r, l = plan["wt"], plan["G"], plan["r2e"], plan["l2e"]
    if (n & 1) and e == n - 1:
        return f"odd tail element (workgroup {G - 1}, lane 0)"
    d = e // 2
    if d >= plan["nres2"]:
        return f"streamed part, double2 {d - plan['nres2']} of {n // 2 - plan['nres2']}"
    nch, ch = plan["nres2"] // WT, d // WT
    if ch < G * r:
        wg, part, width = ch // r, "registers", plan["r2"]
        c0 = wg * r
        cend = min(c0 + r, nch)
    else:
        wg, part, width = (ch - G * r) // l, "LDS", plan["l2"]
        c0 = G * r + wg * l
        cend = min(c0 + l, nch)
    k = ch - c0
    if (k | 1) < width and c0 + (k | 1) < cend:  # a lane owns double2 2t and 2t + 1 of the pair's 512
        off = d - (c0 + (k & ~1)) * WT
        lane, how = off // 2, f"half {off & 1} of the float4 pair in slots {k & ~1} / {k | 1}"
    else:
        lane, how = d - ch * WT, f"unpaired slot {k}"
    return f"chunk {ch}, {part} of workgroup {wg} ({cend - c0} chunks), {how}, lane {lane}"


def check_cb_step(h, stored, V, w0, ref, what="", plan=None):
    """Assert one FP32-basis device step against cb_step_ld: h within step_bounds, every stored
    element its own float32 round trip and within ulp32(v_ref) / 2 + vb of the reference.
    Returns (largest h dev / bound, largest column excess, elements != float32(v_ref))."""
    h_ref, v_ref = ref
    hb, _ = step_bounds(V, w0, v_ref)
    dh = np.abs(np.asarray(h) - h_ref)
    exc, vb = cb_column_excess(stored, v_ref)
    n_off = int(np.count_nonzero(stored != v_ref.astype(np.float32).astype(np.float64)))
    rh, rv = float(np.max(dh / hb)), float(np.max(exc))
    print(f"{what}: h dev/bound {rh:.3e}, column (dev - ulp32/2)/vb {rv:.3e}, {n_off} elements off float32(v_ref)")
    bad_h = np.nonzero(dh > hb)[0]
    assert bad_h.size == 0, f"{what}: h entries {bad_h.tolist()} off: got {np.asarray(h)[bad_h]} ref {h_ref[bad_h]} bound {hb[bad_h]}"
    not32 = np.nonzero(stored != stored.astype(np.float32).astype(np.float64))[0]
    assert not32.size == 0, f"{what}: {not32.size} stored elements are no float32 values, first {not32[0]}"
    bad = np.nonzero(exc > 1.0)[0]
    n = stored.size
    assert bad.size == 0, (f"{what}: new column off at {bad.size} elements, first {bad[0]} ({locate_cb(bad[0], plan, n)}), "
                           f"last {bad[-1]} ({locate_cb(bad[-1], plan, n)}), max excess {rv:.3e} x vb {vb:.3e}")
    return rh, rv, n_off


# ------------------------------------------------------------- device planting --

def plant(ctx, k: int, v: np.ndarray) -> None:
    """v into Krylov column k (0-based) of an FP64-basis context: host -> x -> column.
    Neither call closes an open MGS-R cycle, and a step reads its columns from HBM."""
    from gmres_amd import _native as nat

    ctx.set_x(v)
    nat.check(nat.hip().gk_vec_lincomb(ctx.handle, 0, 2 + k, 0, 0, 0, 0.0, 0.0), "gk_vec_lincomb")  # GK_LC_COPY
    ctx.sync()


def read_col(ctx, k: int) -> np.ndarray:
    return ctx.get_basis(k)
