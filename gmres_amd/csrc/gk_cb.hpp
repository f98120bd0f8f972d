// gk_cb.hpp -- interface of the compressed-basis MGS-R step (gk_set_basis_precision
// GK_BASIS_F32; kernels, planner and launchers in gk_cb.hip, its own translation
// unit): the Krylov columns are STORED as FP32, everything else stays FP64.
//
// Layout (no allocation of its own): FP32 column k lives at float offset k * ld inside
// the context's V allocation ((m + 1) * ld doubles; ld is padded to 32 doubles, so a
// float column starts on a 128-B line) -- the lower half of the allocation.  The two
// FP64 vectors the operator stage reads come from the free upper half: v1w (column 1
// widened, the first dot's partner) in double column m - 1 and vjw (the newest column
// widened, the operator's input) in double column m; (m + 1) / 2 <= m - 1 needs m >= 3.
#pragma once
#include <string>

#include "gk_common.hpp"

namespace gk {

struct ResArgs;

// Chunks of 256 double2 of w per thread of k_mgs_wcb: CB_RW in registers, CB_LW in LDS
// (the H column of WO_HMAX doubles and the exchange words take the rest of the CU's 160 KiB).
// 90 is the largest register part that builds without scratch beside the batch buffers of
// 16 chunks per column (k_mgs_wres holds 89): 89 / 90 -> 0 bytes of scratch per lane with
// 256 VGPRs + 256 AGPRs, 91 / 92 / 96 -> 28 / 36 / 96 bytes.
#ifndef GK_CB_RW
#define GK_CB_RW 90
#endif
constexpr int CB_RW = GK_CB_RW, CB_LW = 39;
constexpr int CB_WT = 256;  // threads per workgroup (one wave per SIMD)

struct CbPlan {
    int G = 0;             // workgroups: one per CU of this context's share of the device
    int r2e = 0, l2e = 0;  // chunks per workgroup held in registers / LDS (<= CB_RW / CB_LW)
    int lds = 0;           // dynamic LDS bytes (pins one workgroup per CU)
    i64 nres2 = 0;         // double2 of w held on chip
    i64 nstream2 = 0;      // double2 of w streamed from / to HBM every pass
    bool on = false;       // the resident launch applies (m + 1 <= WO_HMAX)
};

// The plan of a slab of nloc unknowns on cus / share compute units with Krylov dimension m
// (pure: no context, no device).
GK_HIDDEN void plan_cb(i64 nloc, int cus, int share, int m, CbPlan &p);
// gk_cb_plan_query layout
enum { CPI_G = 0, CPI_RW, CPI_LW, CPI_R2E, CPI_L2E, CPI_LDS, CPI_NRES2, CPI_STREAM2, CPI_ON, CPI_LDS_STATIC, CPI_LEN };
GK_HIDDEN void cb_plan_info(const CbPlan &p, long long *info);

// One resident launch of Arnoldi step a.j on float columns (k_mgs_wcb): F = the FP32
// basis (column stride a.ld floats), the new column to F + a.j * a.ld and widened to vjw.
// a.V / a.vout are not read.  Returns GK_OK, or a GK_ERR_* code with its text in msg.
GK_HIDDEN int cb_launch(const CbPlan &p, const ResArgs &a, float *F, double *vjw, int dev, hipStream_t st,
                        std::string &msg);

// The launch path's two kernels of float columns alone (each returns hipGetLastError() of
// its launch; projection, x update and Gram: k_proj / k_update_x / k_gram<float>, gk_step_kernels.hpp).
// out = float(w / h), h = sqrt(sum(pin)), the same values widened to vjw (and to v1w unless nullptr)
GK_HIDDEN hipError_t cb_scale(int blocks, float *out, double *vjw, double *v1w, const double *w, const double *pin,
                              int npin, double *hslot, i64 n, double *hcopy, const double *hsrc, int ncopy,
                              hipStream_t st);
// out = in widened
GK_HIDDEN hipError_t cb_widen(int blocks, double *out, const float *in, i64 n, hipStream_t st);

}  // namespace gk
