"""The premises of tests/test_gpu_hh_step_known_answer.py, pinned without a GPU
(tests/hh_data.py): for every (N, m, j) the GPU tests run, a correct float64 Householder step
with another summation tree stays below 1/8 of each of the three bounds against the
long-double step -- 64 eps ||w0|| per entry of h, 64 eps |p_ref[j]| at the new reflector's
pivot, 64 eps max |p_ref[j+1:]| on the rest -- and each seeded index fault exceeds one.

Summation trees, both written out so that no library chooses the order: a pairwise tree
(halves added until one term is left), and 512-element partials summed in reverse order.
numpy.dot is evaluated and printed next to them but held to the bound itself, not to 1/8 of
it: it is the host's BLAS ddot -- a few sequential accumulators of n / 8 or so terms each,
chosen per CPU, not a pairwise sum -- and like the fully sequential sum (0.90 of the h bound
at N = 300) it is no stand-in for a device reduction, whose serial runs are a few dozen terms.
It reached 0.18 of the h bound (N = 256, j = 1; 0.15 at N = 333 and 512) with these seeds.

Measured worst ratios to the bound (h / pivot / rest) over the 42 cases: pairwise
0.042 / 0.020 / 0.094, reversed 512-chunks 0.042 / 0.022 / 0.091 (numpy.dot 0.181 / 0.049 /
0.109); with cbpr2 0.019 / 0.022 / 0.103; with running-sum norms at (45, 12) 0.028 / 0.068 /
0.123.  The seeded faults exceed a bound by at least 3e7 (tail norm from j + 1), 6e10 (last
element of P_j), 2e12 and more (the others).  The ratios are maxima over n roundings and have
a tail: hh_data.SEED0 says how the seed was settled.
"""
import numpy as np
import pytest

from tests import hh_data as hd
from tests.general_data import EPS

PIN = 1.0 / 8


def dot_pairwise(a, b):
    """Float64 dot as a balanced tree: the products, zero-padded to a power of two, halves
    added until one term is left."""
    p = a * b
    if p.size == 0:
        return 0.0
    size = 1 << (p.size - 1).bit_length()
    q = np.zeros(size)
    q[: p.size] = p
    while q.size > 1:
        q = q[: q.size // 2] + q[q.size // 2:]
    return float(q[0])


def dot_chunks(a, b):
    """Float64 dot with 512-element partials, summed in reverse order."""
    p = a * b
    q = np.zeros((p.size + 511) // 512 * 512)
    q[: p.size] = p
    q = q.reshape(-1, 512)
    while q.shape[1] > 1:  # each partial a balanced tree, written out so that no library picks the order
        q = q[:, : q.shape[1] // 2] + q[:, q.shape[1] // 2:]
    s = 0.0
    for x in q[::-1, 0]:
        s += float(x)
    return s


def dot_seq(a, b):
    """One running sum, the reference's dot_product order."""
    return float(np.cumsum(a * b)[-1])


def norm2_seq(x):
    """A running sum over the whole vector, the order of GK_TUNE_HH_NORM_ORDER 1."""
    return float(np.sqrt(np.cumsum(x * x)[-1])) if x.size else 0.0


TREES = [("pairwise", dot_pairwise), ("chunks512-reversed", dot_chunks)]

FAULTS = ["pj_last", "tail_lo", "tail_hi", "fix_hi", "down_lead", "chunk_skip"]


def _step_f64(P, j, apply, dot, fault=None):
    """hh_data.hh_step in float64 with one seeded fault: "pj_last" (the last element of P_j
    not read), "tail_lo" / "tail_hi" (the tail norm from index j - 1 / j + 1), "fix_hi" (the
    fix-up at index j + 1), "down_lead" (the DOWN chain's leading dot <e_j, P_j> taken from
    P_j[j] instead of P_j[j - 1]), "chunk_skip" (one 512-element chunk of the UP chain's
    reflection with P_j left as it was).  Returns (h, p), or None where the fault has no room."""
    Pd = np.array(P[:j], dtype=np.float64)
    n = Pd.shape[1]
    if (fault == "fix_hi" and j + 1 >= n) or (fault == "down_lead" and j >= n):
        return None
    if fault == "pj_last":
        Pd[j - 1, -1] = 0.0
    v = np.zeros(n)
    v[j - 1] = 1.0
    for i in range(j, 0, -1):
        d = Pd[i - 1, j] if (fault == "down_lead" and i == j) else dot(v, Pd[i - 1])
        v = v - (2 * d) * Pd[i - 1]
    w = apply(v).copy()
    for i in range(1, j + 1):
        upd = w - (2 * dot(w, Pd[i - 1])) * Pd[i - 1]
        if fault == "chunk_skip" and i == j:
            c = (n // 512) // 2 * 512
            upd[c:c + 512] = w[c:c + 512]
        w = upd
    h = np.zeros(j + 1)
    h[:j] = w[:j]
    t0 = {"tail_lo": j - 1, "tail_hi": j + 1}.get(fault, j)
    tmp = np.sqrt(dot(w[t0:], w[t0:]))
    h[j] = -tmp if w[j] > 0 else tmp
    w[:j] = 0.0
    f = j + 1 if fault == "fix_hi" else j
    w[f] = w[f] - h[j]
    return h, w / np.sqrt(dot(w, w))


@pytest.mark.parametrize("N,m,j", hd.all_cases())
def test_hh_step_bound_passes_reordering_and_fails_seeded_faults(oracle, N, m, j):
    P = hd.reflectors(N, m)
    ref = hd.reference(oracle, N, m, j)  # asserts the asymmetry of v and A v and the sign guard
    assert np.all(P[:, :m] == np.triu(P[:, :m])) and np.all(np.abs(np.diagonal(P[:, :m])) >= np.sqrt(0.5) * (1 - EPS))
    Pl = P.astype(np.longdouble)
    assert np.max(np.abs(np.sqrt(np.sum(Pl * Pl, axis=1)) - 1)) <= 8 * EPS  # unit rows, to the float64 norm's rounding
    # the reference is a step: p has unit length, h carries ||w0||
    assert abs(np.linalg.norm(ref[1]) - 1.0) < 1e-14 and abs(np.linalg.norm(ref[0]) - ref[2]) < 1e-13 * ref[2]

    def ap(x):
        return oracle.stvec(x, N)

    for name, dot in TREES + [("numpy.dot", np.dot)]:
        h, p, *_ = hd.hh_step(P, j, ap, np.float64, dot)
        r = hd.hh_ratios(h, p, ref, j)
        print(f"N={N} m={m} j={j}: float64 step, {name}: dev/bound h {r[0]:.4f} pivot {r[1]:.4f} rest {r[2]:.4f}")
        assert np.all(p[:j] == 0.0)
        assert max(r) < (1.0 if dot is np.dot else PIN), (name, r)
    for fault in FAULTS:
        out = _step_f64(P, j, ap, dot_chunks, fault)
        if out is None:
            print(f"N={N} m={m} j={j}: {fault}: no room")
            continue
        r = hd.hh_ratios(*out, ref, j)
        print(f"N={N} m={m} j={j}: {fault}: dev/bound h {r[0]:.3e} pivot {r[1]:.3e} rest {r[2]:.3e}")
        assert max(r) > 1.0, (fault, r)
    clean = _step_f64(P, j, ap, dot_chunks)
    h, p, *_ = hd.hh_step(P, j, ap, np.float64, dot_chunks)
    assert np.array_equal(clean[0], h) and np.array_equal(clean[1], p)  # the faulted step is the step


@pytest.mark.parametrize("N,m", hd.PREC_SHAPES)
def test_hh_preconditioned_step_pin(oracle, N, m):
    """w0 = cbpr2(A v): the reference applies the oracle's float64 operator to ITS v rounded to
    float64, each emulation to its own float64 v, so this also measures what the rounding
    of v costs through cbpr2 o A."""
    P = hd.reflectors(N, m)

    def ap(x):
        return oracle.precond(oracle.PREC_CBPR2, oracle.stvec(x, N), N)

    for j in (hd.launch_js(m) if (N, m) in hd.LAUNCH_SHAPES else hd.resident_js(m)):
        ref = hd.reference(oracle, N, m, j, precondition=True)
        for name, dot in TREES:
            h, p, *_ = hd.hh_step(P, j, ap, np.float64, dot)
            r = hd.hh_ratios(h, p, ref, j)
            print(f"cbpr2 N={N} m={m} j={j}: float64 step, {name}: dev/bound h {r[0]:.4f} pivot {r[1]:.4f} rest {r[2]:.4f}")
            assert max(r) < PIN, (name, r)


def test_hh_sequential_norms_pin(oracle):
    """GK_TUNE_HH_NORM_ORDER 1 at (45, 12): running-sum norms with tree dots."""
    N, m = 45, 12
    P = hd.reflectors(N, m)
    for j in hd.launch_js(m):
        ref = hd.reference(oracle, N, m, j)
        for name, dot in TREES:
            h, p, *_ = hd.hh_step(P, j, lambda x: oracle.stvec(x, N), np.float64, dot, norm2=norm2_seq)
            r = hd.hh_ratios(h, p, ref, j)
            print(f"sequential norms N={N} j={j}, {name} dots: dev/bound h {r[0]:.4f} pivot {r[1]:.4f} rest {r[2]:.4f}")
            assert max(r) < PIN, (name, r)


@pytest.mark.parametrize("N,m", hd.VEC_SHAPES)
def test_hh_update_x_and_rebuilt_basis_pins(N, m):
    """x + P_1..P_m [y; 0] within 64 eps (max|x| + ||y||) per element, and the rebuilt column
    P_1..P_k e_k within 64 eps |v_ref[k-1]| at its spike and 64 eps max|v_ref off the spike|
    elsewhere: float64 evaluations stay below 1/8, a reflection with one 512-element chunk
    skipped does not."""
    P = hd.reflectors(N, m)
    x, y = hd.vec_data(N, m)
    ref = hd.update_x_ld(P, x, y).astype(np.float64)
    b = hd.update_x_bound(x, y)
    for name, dot in TREES:
        r = float(np.max(np.abs(hd.update_x_ld(P, x, y, np.float64, dot) - ref)) / b)
        print(f"update_x N={N} m={m}, {name}: dev/bound {r:.4f}")
        assert r < PIN
    w = np.zeros(N * N)
    w[:m] = y
    w1 = w - (2 * np.dot(w, P[m - 1])) * P[m - 1]
    w1[512:1024] = w[512:1024]  # the first reflection misses one chunk
    bad = float(np.max(np.abs(x + hd.chain_down_ld(P, w1, m - 1, np.float64) - ref)) / b)
    print(f"update_x N={N} m={m}, one chunk of one reflection skipped: dev/bound {bad:.3e}")
    assert bad > 1.0
    worst = {}
    for k in range(1, m + 1):
        vref = hd.rebuilt_ld(P, k)
        e = np.zeros(N * N)
        e[k - 1] = 1.0
        for name, dot in TREES + [("running sum", dot_seq)]:
            r = hd.rebuilt_ratios(hd.chain_down_ld(P, e, k, np.float64, dot), vref, k)
            worst[name] = tuple(max(a, b) for a, b in zip(worst.get(name, (0.0, 0.0)), r))
            # one running sum per dot (GK_TUNE_VERR_ORDER 1) meets the bound on max|v_ref| only
            assert r[0] < PIN and (dot is dot_seq or r[1] < PIN), (k, name, r)
    for name, r in worst.items():
        print(f"rebuilt columns N={N} m={m}, {name}: worst dev/bound {r[0]:.4f}, off the spike {r[1]:.4f}")
