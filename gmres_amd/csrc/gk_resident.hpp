// gk_resident.hpp -- interface of the resident MGS-R / Householder step (kernels,
// planner and launchers in gk_resident.hip, its own translation unit): the pure
// planner (no context, no device) and one launch entry.
#pragma once
#include <string>

#include "gk_common.hpp"

namespace gk {

struct ResArgs;

constexpr int RES_R2_BIG = 12;          // two register arrays of 12 double2 fit 256 VGPRs without spills

struct ResPlan {
    int G = 0, r2 = 0, l2 = 0;
    int r2e = 0, l2e = 0;  // chunks per workgroup used: the resident prefix spread evenly over G
    bool pf = false, nt = false, cw = false, wo = false;
    bool pc = false;       // column-cache variant (k_mgs_wpc): w in registers, running column cached
    bool pcs = false;      // ... its 16-chunk instantiation (whole column in registers)
    int blk = 0;           // > 1: the blocked-projection MGS step k_mgs_blk with blocks of `blk` (gk_blk.hpp);
                           // 1 with bvar >= 0: the strict step on k_mgs_blk<S = 1> (GK_TUNE_RES_PF)
    int bvar = -1;         // ... its instantiation (gk::BLK_*)
    int wt = 0;            // threads per workgroup = double2 per chunk (set by plan_resident)
    bool pipe = false;     // w-only MGS step: the software-pipelined pass (full workgroups only)
    int carry = 0;         // ... chunks of its ring carried across each all-gather (single rank only)
    i64 nres2 = 0;
    int lds = 0;
};

// Modelled bytes per projection of a slab of n2 double2 on G workgroups under the
// column-cache, the pairs and the w-only variant (what plan_resident compares).
GK_HIDDEN i64 pc_bytes(i64 n2, int G, bool hh);
GK_HIDDEN i64 pairs_bytes(i64 n2, int G);
GK_HIDDEN i64 wonly_bytes(i64 n2, int G);

// The variant a slab of nloc local unknowns runs on, from the tuning values alone.
GK_HIDDEN void plan_resident(i64 nloc, int gmax, int cap, int tune_wonly, bool hh, bool nt, ResPlan &p,
                             int tune_pc = -1, int tune_blk = 1, int tune_pf = 0, int tune_pipe = -1,
                             int tune_carry = -1);
GK_HIDDEN bool nt_auto_for(i64 max_nloc);

// The even spread of a slab's whole chunks (n2 double2 in chunks of dt, one per thread)
// over G workgroups: every workgroup holds ceil(chunks / G) register chunks (at most
// rmax), then the same for LDS (at most lmax); nres2 = the double2 held on chip.  A
// contiguous fill would leave the last workgroups idle and make the first ones set the
// pace of every all-gather (2048^2: slowest pass 10.2 us vs 4.3 us median).
GK_HIDDEN void res_spread(i64 n2, i64 dt, int G, int rmax, int lmax, int &r2e, int &l2e, i64 &nres2);

// gk_res_plan_query / gk_res_info layout
enum { RPI_VARIANT = 0, RPI_G, RPI_R2, RPI_L2, RPI_PF, RPI_CW, RPI_WO, RPI_NT, RPI_R2E, RPI_L2E, RPI_LDS, RPI_NRES2, RPI_PIPE,
       RPI_CHEB_STEN, RPI_WT, RPI_BLK, RPI_CARRY };
GK_HIDDEN void plan_info(const ResPlan &p, bool on, long long *info);

// Launch plan p's kernel for a.mode on stream st of device dev.  Returns GK_OK, or a
// GK_ERR_* code with its text in msg (the caller's set_err).
GK_HIDDEN int res_launch(const ResPlan &p, const ResArgs &a, int dev, hipStream_t st, std::string &msg);

// What the launchers of the resident kernels (gk_resident.hip, gk_blk.hip, gk_cb.hip) share.
// msg = the formatted text; returns code.
GK_HIDDEN int fail(std::string &msg, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
// Allow `kernel` lds bytes of dynamic LDS on device dev (memo[ATTR_DEVS]: one per instantiation).
GK_HIDDEN int dyn_lds(const void *kernel, int dev, int lds, std::atomic<int> *memo, std::string &msg);
// GK_OK, or the launch error of the `what` just launched.
GK_HIDDEN int launched(const char *what, std::string &msg);

}  // namespace gk
