"""The host model of the shifted operator (tests/shift_data.py) held to what the device is
already held to, and to the rule of gk_set_shift: CPU only.

1. At sigma = 0 the model IS the oracle, bit for bit: stencil, cbpr2, Chebyshev(1, 2, 8) and the
   V-cycle of tests/mg_data.py.
2. The multigrid rule sigma_l = 4^l sigma with the intervals moved by sigma_l - sigma never
   needs more PCG iterations than sigma = 0; sigma_l = 2^l sigma and unmoved intervals do.
3. Planted faults change the V-cycle's output.
"""
import numpy as np
import pytest

from tests import mg_data
from tests import shift_data as sd

SIZES = (16, 48, 130)
SIGMAS = (0.0, 1e-3, 1e-2, 0.1, 1.0, 10.0, 100.0)
# PCG to 1e-8 on b = A_sigma 1, degree 2, params (8 + sigma, 1 + sigma), N = 128: the NumPy
# restatement's counts the rule was chosen by
TABLE_128 = (9, 9, 8, 6, 4, 2, 1)


def vec(N, seed):
    return sd.asym(N, seed)


def test_fma_fast_path_is_the_fraction():
    rng = np.random.default_rng(5)
    c = rng.standard_normal(20000)
    s = rng.standard_normal(20000) * 4.0
    # cancellation, exact zeros and ties: s next to diag c, c = 0, and a product on a midpoint
    s[:5000] = 4.37 * c[:5000] * (1.0 + rng.integers(-3, 4, 5000) * 2.0 ** -52)
    c[5000:5100] = 0.0
    s[5100:5200] = 0.0
    for diag in (4.37, 4.01, 4.0 + 0.37 * 4, 4.001, 104.0, 4.0 + 2.0 ** -50):
        assert np.array_equal(sd.fma(diag, c, s), sd.fma_fraction(diag, c, s)), diag
    for diag in (4.0, 8.0, 16.0):
        assert np.array_equal(sd.fma(diag, c[:2000], s[:2000]), sd.fma_fraction(diag, c[:2000], s[:2000])), diag


def test_fma_is_one_rounding():
    """diag c - s where two roundings differ from one: c = 1 + 2^-52, diag = 4.37."""
    c = np.array([1.0 + 2.0 ** -52, 3.0, -7.0 / 3.0])
    s = np.array([4.37, 1.0 / 3.0, 0.1])
    one = sd.fma(4.37, c, s)
    assert np.array_equal(one, sd.fma_fraction(4.37, c, s))
    big = np.random.default_rng(1).standard_normal(4096)
    bs = np.random.default_rng(2).standard_normal(4096)
    assert not np.array_equal(sd.fma(4.37, big, bs), 4.37 * big - bs)


@pytest.mark.parametrize("N", SIZES)
def test_sigma0_is_the_oracle(oracle, N):
    v = vec(N, 100 + N)
    assert np.array_equal(sd.stencil(v, N, 0.0), oracle.stvec(v, N))
    assert np.array_equal(sd.cbpr2(v, N, 0.0), oracle.precond(oracle.PREC_CBPR2, v, N, params=(8.2, 0.2)))
    for deg in (1, 2, 8):
        assert np.array_equal(sd.cheb(v, N, 0.0, (8.2, 0.2), deg),
                              oracle.precond(oracle.PREC_CHEB, v, N, params=(8.2, 0.2), degree=deg)), deg
    assert np.array_equal(sd.mg(v, N, 0.0), mg_data.mg(oracle, v, N))
    assert sd.nu_c(N, 0.0) == mg_data.coarse(mg_data.levels(N)[-1])[2]
    assert np.array_equal(sd.rhs_ones(N, 0.0), oracle.rhs_ones(N))


def test_slab_halo_lines_are_the_whole_grid():
    N, sg = 20, 0.37
    v = vec(N, 3)
    full = sd.stencil(v, N, sg).reshape(N, N)
    g = v.reshape(N, N)
    part = sd.stencil(g[5:12], N, sg, lo=g[4], hi=g[12]).reshape(-1, N)
    assert np.array_equal(part, full[5:12])


@pytest.fixture(scope="module")
def counts_128(oracle):
    return [sd.pcg(oracle, 128, s)[0] for s in SIGMAS]


def test_rule_iteration_table(counts_128):
    print("sigma_l = 4^l sigma, moved intervals:", dict(zip(SIGMAS, counts_128)))
    assert tuple(counts_128) == TABLE_128
    assert all(c <= counts_128[0] for c in counts_128)


def test_wrong_rules_are_caught(oracle, counts_128):
    c0 = counts_128[0]
    it, rel = sd.pcg(oracle, 128, 0.1, rule="2l", max_iter=c0 + 1)
    print("sigma_l = 2^l sigma at 0.1:", it, rel)
    assert it > c0
    it, rel = sd.pcg(oracle, 128, 1.0, rule="4l-fixed-intervals", max_iter=c0 + 1)
    print("unmoved intervals at 1:", it, rel)
    assert it > c0


@pytest.mark.parametrize("fault", ["drop-level-1", "two-roundings", "stale-nuc"])
def test_planted_faults_change_the_cycle(fault):
    N, sg = 48, 0.37
    v = vec(N, 48)
    good = sd.mg(v, N, sg)
    bad = sd.mg(v, N, sg, fault=fault)
    n = int(np.count_nonzero(good != bad))
    print(fault, "elements changed:", n, "max", float(np.max(np.abs(good - bad))))
    assert n >= 1
