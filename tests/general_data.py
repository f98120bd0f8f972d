"""Data without the square's symmetries, and the long-double Arnoldi step they are
checked against (test infrastructure for tests/test_gpu_step_known_answer.py and
tests/test_gpu_general_rhs.py).

The Poisson 5-point operator, cbpr2 and Chebyshev(k) commute with the eight symmetries
of the square and b = A*1 is invariant under all of them, so every Krylov vector of a
set_rhs_ones() solve equals its own index reversal, its transposed grid and its grid
with the lines reversed.  A kernel that walks a vector from the wrong end reproduces
such a solve bit for bit.  The vectors built here are invariant under none of them.
"""
from __future__ import annotations

import numpy as np

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
