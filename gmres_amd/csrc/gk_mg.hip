// gk_mg.hip -- the aggregation multigrid V-cycle's transfer and closing kernels for gfx950
// (gk_mg.hpp).
//
// All three are HBM-bandwidth bound streaming kernels in the project's idiom: 16-byte
// accesses along the fast index, one partial per workgroup into a fixed slab that the next
// launch re-reduces in a fixed order, and -ffp-contract=off so that every element-wise
// expression is the stated one.  Bytes per FINE unknown: the fused residual-restriction
// reads z and r and writes a quarter vector, 18 (OP_RESID into a vector followed by the
// plain restriction: 24 + 10 = 34); the prolongation reads z and a quarter vector and
// writes z, 18; the closing add reads two vectors and writes one, 24 (+ 8 for a dot partner).
#include <cmath>

#include "gk_march.hpp"
#include "gk_mg.hpp"

namespace gk {

// ----------------------------------------------------------------- host ---
int mg_levels(int N, int *sides) {
    if (N < 2 * MG_NMIN || N % 2 != 0) return 0;
    int n = 0;
    sides[n++] = N;
    while (N % 2 == 0 && N / 2 >= MG_NMIN && n < MG_LMAX) {
        N /= 2;
        sides[n++] = N;
    }
    return n;
}

// The extreme eigenvalues of the 5-point operator plus `shift` (the coarsest level's, 4^L
// times the context's) on an NL x NL Dirichlet grid, and the smallest degree whose Chebyshev
// error bound 1 / cosh((nu + 1) acosh sigma) is at most 0.1.
int mg_coarse_degree(int NL, double shift, double *lo, double *hi) {
    const double pi = 3.14159265358979323846;
    const double t = pi / (2.0 * (NL + 1));
    const double sn = std::sin(t), cs = std::cos(t);
    *lo = 8.0 * sn * sn + shift;
    *hi = 8.0 * cs * cs + shift;
    const double sigma = (*hi + *lo) / (*hi - *lo);
    const double ac = std::acosh(sigma);
    for (int nu = 1; nu <= MG_CDEG_MAX; ++nu)
        if (1.0 / std::cosh((nu + 1) * ac) <= 0.1) return nu;
    return MG_CDEG_MAX;
}

// -------------------------------------------------------------- restrict ---
// The line march of gk_march.hpp on the fine grid, two points per lane (N even: a lane's
// pair is one coarse column I = i0 / 2), an even number of lines from an even j0 (a line
// pair is one coarse line J = j / 2).  RESID: the march on z (we_load) with f = r - A z in
// OP_RESID's expression, never stored.  Else f = x as stored.  One coarse double per lane
// and line pair: rc(I,J) = ((f(2I,2J) + f(2I+1,2J)) + f(2I,2J+1)) + f(2I+1,2J+1).  Levels
// narrower than the workgroup leave lanes past the line's end.
struct MgrArgs {
    const double *x;  // RESID: z ; else f
    const double *r;  // RESID: the right-hand side of the residual
    double *rc;       // coarse output, (N/2)^2
    double diag;      // RESID: the level's diagonal, fl(4 + shift_l)
    int N, JT;        // fine side (even), lines per workgroup (even)
};

template <bool RESID>
__global__ __launch_bounds__(TPB) void k_mg_restrict(MgrArgs a) {
    const int N = a.N, Nc = N >> 1;
    const March m = march_init<2>(N, N, a.JT);  // j1 even: N and JT are
    if (m.j0 >= N) return;

    auto load_line = [&](int jj, double (&t)[2]) {
        const bool ok = m.act && jj >= 0 && jj < N;  // lines outside the grid are zeros
        ld_vec<2>(ok ? a.x + (i64)jj * N + m.i0 : nullptr, ok, t);
    };

    if constexpr (!RESID) {
        for (int j = m.j0; j < m.j1; j += 2) {
            double f0[2], f1[2];
            load_line(j, f0);
            load_line(j + 1, f1);
            const double s = ((f0[0] + f0[1]) + f1[0]) + f1[1];
            if (m.act) a.rc[(i64)(j >> 1) * Nc + (m.i0 >> 1)] = s;
        }
    } else {
        double tm[2], tc[2], tp[2], tn[2] = {0.0, 0.0};
        load_line(m.j0 - 1, tm);
        load_line(m.j0, tc);
        load_line(m.j0 + 1, tp);
        double pend = 0.0;
        for (int j = m.j0; j < m.j1; ++j) {
            if (j + 2 <= m.j1) load_line(j + 2, tn);  // in flight while line j is computed
            const i64 row = (i64)j * N;
            double left, right;
            we_load<2, false>(m, N, tc, a.x, row, 1.0, left, right);
            double rv[2], f[2];
            ld_vec<2>(m.act ? a.r + row + m.i0 : nullptr, m.act, rv);
#pragma unroll
            for (int k = 0; k < 2; ++k) f[k] = rv[k] - ax5_at<2>(a.diag, k, tc, tp, tm, left, right);
            if ((j & 1) == 0) {
                pend = f[0] + f[1];
            } else {
                pend = (pend + f[0]) + f[1];
                if (m.act) a.rc[(i64)(j >> 1) * Nc + (m.i0 >> 1)] = pend;
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                tm[k] = tc[k];
                tc[k] = tp[k];
                tp[k] = tn[k];
            }
        }
    }
}

hipError_t mg_restrict(bool fused, int N, double diag, const double *x, const double *r, double *rc,
                       hipStream_t st) {
    if (N < 2 || (N & 1) || x == nullptr || rc == nullptr || (fused && r == nullptr)) return hipErrorInvalidValue;
    const int gx = (N + TPB * 2 - 1) / (TPB * 2);
    // ~2048 workgroups of at most 64 lines, as set_geometry sizes the stencil sweeps, but an even
    // number of lines each and no cap on the workgroup count (no partial slab)
    int JT = (int)(((i64)N * gx + 2047) / 2048);
    JT = (JT + 1) & ~1;
    JT = JT < 2 ? 2 : (JT > 64 ? 64 : JT);
    const dim3 g(gx, (N + JT - 1) / JT, 1);
    MgrArgs a{x, r, rc, diag, N, JT};
    if (fused)
        k_mg_restrict<true><<<g, TPB, 0, st>>>(a);
    else
        k_mg_restrict<false><<<g, TPB, 0, st>>>(a);
    return hipGetLastError();
}

// ---------------------------------------------------------------- prolong ---
// A thread takes one coarse value ec(I,J) and the two fine double2 under it, (2I..2I+1, 2J)
// and (2I..2I+1, 2J+1): out = z + ec there.  Each thread reads what it writes before it
// writes it and nothing else of z: out may be z.
__global__ __launch_bounds__(TPB) void k_mg_prolong_add(const double *z, const double *__restrict__ ec, double *out,
                                                        int Nc) {
    const double2 *Z2 = reinterpret_cast<const double2 *>(z);
    double2 *O2 = reinterpret_cast<double2 *>(out);
    const i64 nc = (i64)Nc * Nc, stride = (i64)gridDim.x * TPB;
    for (i64 q = (i64)blockIdx.x * TPB + threadIdx.x; q < nc; q += stride) {
        const i64 J = q / Nc, I = q - J * Nc;
        const i64 e0 = 2 * J * Nc + I, e1 = e0 + Nc;  // in double2: a fine line holds Nc of them
        const double c = ec[q];
        const double2 a = Z2[e0], b = Z2[e1];
        O2[e0] = double2{a.x + c, a.y + c};
        O2[e1] = double2{b.x + c, b.y + c};
    }
}

hipError_t mg_prolong_add(int N, const double *z, const double *ec, double *out, hipStream_t st) {
    if (N < 2 || (N & 1) || z == nullptr || ec == nullptr || out == nullptr) return hipErrorInvalidValue;
    const int Nc = N / 2;
    const i64 nb = ((i64)Nc * Nc + TPB - 1) / TPB;
    k_mg_prolong_add<<<(unsigned)(nb < 2048 ? nb : 2048), TPB, 0, st>>>(z, ec, out, Nc);
    return hipGetLastError();
}

// -------------------------------------------------------------------- add ---
// out = a + b, the launch that writes the cycle's result: it carries the reduction the
// preconditioner's caller asked for, one partial per workgroup in part[blockIdx.x].
template <int ACC>
__global__ __launch_bounds__(TPB) void k_mg_add(const double *a, const double *b, double *out, const double *vdot,
                                                double *__restrict__ part, i64 n) {
    __shared__ double sm[WAVES];
    const double2 *A2 = reinterpret_cast<const double2 *>(a);
    const double2 *B2 = reinterpret_cast<const double2 *>(b);
    const double2 *D2 = reinterpret_cast<const double2 *>(vdot);
    double2 *O2 = reinterpret_cast<double2 *>(out);
    const i64 n2 = n >> 1, stride = (i64)gridDim.x * TPB;
    double acc = 0.0;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n2; e += stride) {
        const double2 x = A2[e], y = B2[e];
        double2 d{0.0, 0.0};
        if (ACC == ACC_DOT) d = D2[e];
        const double2 o{x.x + y.x, x.y + y.y};
        O2[e] = o;
        if (ACC == ACC_DOT) {
            acc = acc + o.x * d.x;
            acc = acc + o.y * d.y;
        } else if (ACC == ACC_NORM) {
            acc = acc + o.x * o.x;
            acc = acc + o.y * o.y;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {  // odd-length tail element
        const double o = a[n - 1] + b[n - 1];
        out[n - 1] = o;
        if (ACC == ACC_DOT) acc = acc + o * vdot[n - 1];
        if (ACC == ACC_NORM) acc = acc + o * o;
    }
    if (ACC != ACC_NONE) {
        const double s = block_sum(acc, sm);
        if (threadIdx.x == 0) part[blockIdx.x] = s;
    }
}

hipError_t mg_add(int acc, int G, i64 n, const double *a, const double *b, double *out, const double *vdot,
                  double *part, hipStream_t st) {
    if (n < 1 || G < 1 || G > NPMAX || a == nullptr || b == nullptr || out == nullptr) return hipErrorInvalidValue;
    if ((acc == ACC_DOT && vdot == nullptr) || (acc != ACC_NONE && part == nullptr)) return hipErrorInvalidValue;
    if (acc == ACC_DOT)
        k_mg_add<ACC_DOT><<<G, TPB, 0, st>>>(a, b, out, vdot, part, n);
    else if (acc == ACC_NORM)
        k_mg_add<ACC_NORM><<<G, TPB, 0, st>>>(a, b, out, vdot, part, n);
    else
        k_mg_add<ACC_NONE><<<G, TPB, 0, st>>>(a, b, out, vdot, part, n);
    return hipGetLastError();
}

}  // namespace gk
