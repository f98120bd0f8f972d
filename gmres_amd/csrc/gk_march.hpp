// gk_march.hpp -- the 5-point line march, stated once for the kernels that run it:
// k_stencil and k_right_cbpr2 (gk_stencil.hpp), k_sr_march and k_sr_march2 (gk_sr.hpp),
// k_mg_restrict (gk_mg.hip).  __device__ __forceinline__ pieces only: each kernel keeps its
// own loop and statement order (in k_sr_march the order of load issue is the software
// pipeline) and calls these inside it.
//
// The scheme.  A workgroup owns TPB*VEC consecutive points of the fast index i, VEC per
// lane, and marches over JT grid lines j.  Lines j-1, j, j+1 of the stencil's argument are
// in registers and one more line is in flight while line j is computed: every element is
// read from HBM once (plus the seam lines of a line tile).  The N/S neighbours are the
// lane's own registers; the W/E neighbours of a lane's first / last point come from the
// adjacent lanes by __shfl (wave64).
//
// The seams.
//   * Wave windows: lane 0 has no lane to its left, lane 63 none to its right.  They take
//     the point next to the window either by a load through L1 (we_load) or from a value
//     the kernel formed ahead of time (we_edge).  Two-level marches (level 2 = A of a
//     level-1 line computed one line ahead) need the LEVEL-1 value there, which the edge
//     lanes compute themselves (ax5 at the point ea) from two columns outside the window
//     (Edge2: ea next to it, eb one further).
//   * The grid's edge: a missing neighbour is zero.  x + 0 is exact, so the sum
//     ((W + E) + N) + S is bit-identical to the reference's separate edge / corner
//     statements (poisson.f90:33-77).  Lines -1 and nlines are halo lines or zeros.
//   * Line tiles: a tile re-reads lines j0-1 and j1 (two-level: j0-2 .. j1+1).
//   * Lanes past the line's end (act false) load nothing or column 0 (il) and store nothing.
//
// The Chebyshev pass (gk_cheb.hip: cf_dc_minus and its DPP neighbours) states the same
// point formula, the same one fma: whoever changes the operator changes it there too.
#pragma once
#include "gk_common.hpp"

namespace gk {

// A t at one point: diag c - (((W + E) + N) + S) as ONE fused multiply-add, diag = fl(4 + shift)
// a kernel argument (gk_host.hpp: diag_of).  At diag = 4 the product is exact, so the one
// rounding gives the double of the reference's two, 4.0 * c - 1.0 * sum   (poisson.f90:42)
__device__ __forceinline__ double ax5(double diag, double c, double W, double E, double n, double s) {
    const double sum = ((W + E) + n) + s;
    return __builtin_fma(diag, c, -sum);
}

// ... at point k of a lane's line tc (tp: line j+1, tm: line j-1); left / right: the W / E
// neighbours of the lane's first / last point
template <int VEC>
__device__ __forceinline__ double ax5_at(double diag, int k, const double (&tc)[VEC], const double (&tp)[VEC],
                                         const double (&tm)[VEC], double left, double right) {
    const double W = (k == 0) ? left : tc[k - 1];
    const double E = (k == VEC - 1) ? right : tc[k + 1];
    return ax5(diag, tc[k], W, E, tp[k], tm[k]);
}

// A lane's window: its first point i0 (act: inside the line) and the workgroup's lines
// j0 .. j1-1.  il: the load column of unconditional loads (a lane past N loads column 0,
// then writes nothing).
struct March {
    int lane;
    i64 i0;
    bool act;
    int j0, j1;
    __device__ __forceinline__ i64 il() const { return act ? i0 : 0; }
};
template <int VEC>
__device__ __forceinline__ March march_init(int N, int nlines, int JT) {
    March m;
    m.lane = threadIdx.x & 63;
    m.i0 = (i64)blockIdx.x * (TPB * VEC) + (i64)VEC * threadIdx.x;
    m.act = m.i0 < N;
    m.j0 = blockIdx.y * JT;
    m.j1 = min(m.j0 + JT, nlines);
    return m;
}

// W/E neighbours of a lane's first / last point from the adjacent lanes ...
template <int VEC>
__device__ __forceinline__ void we_shfl(const double (&t)[VEC], double &left, double &right) {
    left = __shfl_up(t[VEC - 1], 1, 64);  // previous lane's last point
    right = __shfl_down(t[0], 1, 64);     // next lane's first point
}
// ... and zeros beyond the grid's edge
template <int VEC>
__device__ __forceinline__ void we_clip(const March &m, int N, double &left, double &right) {
    left = m.i0 == 0 ? 0.0 : left;
    right = m.i0 + VEC >= N ? 0.0 : right;
}
// Lanes 0 and 63 read their outer neighbour through L1, from line x + row (XF: divided by dv,
// the operand transform the lane's own points had at load).
template <int VEC, bool XF>
__device__ __forceinline__ void we_load(const March &m, int N, const double (&t)[VEC], const double *x, i64 row,
                                        double dv, double &left, double &right) {
    we_shfl<VEC>(t, left, right);
    if (m.lane == 0 && m.act) left = (m.i0 > 0) ? x[row + m.i0 - 1] : 0.0;
    if (m.lane == 63 && m.act) right = (m.i0 + VEC < N) ? x[row + m.i0 + VEC] : 0.0;
    if (XF && m.lane == 0) left = left / dv;
    if (XF && m.lane == 63) right = right / dv;
    we_clip<VEC>(m, N, left, right);
}
// Lanes 0 and 63 (e0, e63) take `edge`, the value they hold for the point next to the window
// (k_sr_march forms it between we_shfl and this, and tests the lane here; the two-level
// marches hold the two flags in Edge2: we_select).
template <int VEC>
__device__ __forceinline__ void we_edge(const March &m, int N, bool e0, bool e63, double edge, double &left,
                                        double &right) {
    left = e0 ? edge : left;
    right = e63 ? edge : right;
    we_clip<VEC>(m, N, left, right);
}

// Two-level marches: the columns next to the window (ea) and one further (eb) -- lane 0 to
// its left, lane 63 to its right -- clamped into the line; a clamped column is one whose
// value is never used (grid edge), eb_ok says eb is inside the line; on: an edge lane of
// a window inside the line, the only lanes whose values there are used.  GROUPED: lanes 1..31
// load lane 0's columns and lanes 32..62 lane 63's, so a wave's edge load touches two cache
// lines (k_sr_march2; A/B'd for the short-recurrence marches only); else every lane takes
// the columns next to its own points (k_right_cbpr2).
struct Edge2 {
    bool e0, e63;  // the window's first / last lane
    i64 ea, eb;
    bool eb_ok, on;
};
template <int VEC, bool GROUPED>
__device__ __forceinline__ Edge2 edge2_init(const March &m, int N) {
    Edge2 e;
    e.e0 = m.lane == 0;
    e.e63 = m.lane == 63;
    const bool lo = GROUPED ? m.lane < 32 : e.e0;
    const i64 first = GROUPED ? m.i0 - (i64)VEC * m.lane : m.i0;  // the wave's / the lane's first point
    constexpr int span = GROUPED ? 64 * VEC : VEC;
    e.ea = first + (lo ? -1 : span);
    e.eb = first + (lo ? -2 : span + 1);
    e.on = (e.e0 || e.e63) && m.act;
    e.eb_ok = e.e0 ? (m.i0 - 2 >= 0) : ((!GROUPED || e.e63) ? (m.i0 + VEC + 1 < N) : true);
    e.ea = e.ea < 0 ? 0 : (e.ea >= N ? N - 1 : e.ea);
    e.eb = e.eb < 0 ? 0 : (e.eb >= N ? N - 1 : e.eb);
    return e;
}
// W/E neighbours of a level of a two-level march: the edge lanes take their value at ea
template <int VEC>
__device__ __forceinline__ void we_select(const March &m, const Edge2 &e, int N, const double (&t)[VEC], double ta,
                                          double &left, double &right) {
    we_shfl<VEC>(t, left, right);
    we_edge<VEC>(m, N, e.e0, e.e63, ta, left, right);
}

// VEC doubles at p by one load of the given cache policy (NT: non-temporal)
template <int VEC, bool NT>
__device__ __forceinline__ void ld_pol(const double *p, double (&v)[VEC]) {
    if constexpr (VEC == 2) {
        const double2 t = ldv<NT>(reinterpret_cast<const double2 *>(p));
        v[0] = t.x;
        v[1] = t.y;
    } else if constexpr (NT) {
        v[0] = __builtin_nontemporal_load(p);
    } else {
        v[0] = p[0];
    }
}

// The workgroup's partial of a fused reduction into its slot of the slab
__device__ __forceinline__ void put_partial(double acc, double *sm, double *part) {
    const double s = block_sum(acc, sm);
    if (threadIdx.x == 0) part[(i64)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

}  // namespace gk
