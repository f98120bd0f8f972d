// gk_comm.hip -- collectives of a context and their C-ABI entry points: RCCL, the
// in-process group (several contexts of one process) and the device exchange
// (xgmi: granules written straight into the peers' memory, k_xchg / k_xhalo).
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "gk_host.hpp"

namespace gk {

// All-reduce / broadcast of a short vector, one workgroup per rank.
//   XS_SLAB : buf[0..count) is a partial slab; each rank reduces its own slab in a
//             fixed order, the ranks' totals are summed in rank order, and the
//             slab becomes {total, 0, ..., 0} (its consumer re-reduces it).
//   XS_VEC  : element-wise sum over ranks in rank order, count <= XS_MAXV.
//   XS_BCAST: buf = root's buf, count <= XS_MAXV.
// The rank-order sum is the same instruction sequence on every rank, so the
// replicated host loops see bit-identical scalars.
// seqbase != nullptr (a launch replayed from a captured graph): the sequence
// number is *seqbase + seq, the host having set *seqbase on the stream before the
// replay -- a graph's kernel arguments are fixed, an exchange's number is not.
template <int MODE>
__global__ __launch_bounds__(TPB) void k_xchg(double *__restrict__ buf, int count, XsPeers peers, int nranks,
                                               int rank, unsigned seq_arg, const unsigned *seqbase, int root,
                                               int *err, u64 timeout) {
    const unsigned seq = seqbase != nullptr ? *seqbase + seq_arg : seq_arg;
    __shared__ double sm[WAVES];
    __shared__ double pay[XS_MAXV];
    __shared__ unsigned rv[XS_MAXR * XS_MAXV * 2];
    __shared__ int bad;
    const int plen = MODE == XS_SLAB ? 1 : count;
    if (threadIdx.x == 0) bad = xs_flag(err);
    if (MODE == XS_SLAB) {
        const double s = reduce_slab(buf, count, sm);  // synchronises the block
        if (threadIdx.x == 0) pay[0] = s;
    } else {
        for (int k = threadIdx.x; k < plen; k += TPB) pay[k] = buf[k];
    }
    __syncthreads();
    const unsigned par = seq & 1u;
    const int tot = nranks * plen * 2;
    if (!bad) {
        for (int t = threadIdx.x; t < tot; t += TPB) {
            const int half = t & 1, k = (t >> 1) % plen, dst = (t >> 1) / plen;
            const u64 bits = (u64)__double_as_longlong(pay[k]);
            xs_put(peers.p[dst] + (((i64)par * XS_MAXR + rank) * XS_MAXV + k) * 2 + half, seq,
                   half ? (unsigned)(bits >> 32) : (unsigned)bits);
        }
        const u64 deadline = wall_clock64() + timeout;
        const u64 *mine = peers.p[rank];
        bool ok = true;
        for (int t = threadIdx.x; t < tot && ok; t += TPB) {
            const int half = t & 1, k = (t >> 1) % plen, src = (t >> 1) / plen;
            unsigned d = 0;
            const int g = xs_get(mine + (((i64)par * XS_MAXR + src) * XS_MAXV + k) * 2 + half, seq, deadline, &d, err);
            ok = g == XG_OK;
            rv[(src * XS_MAXV + k) * 2 + half] = d;
            if (g == XG_LATE) xs_fail(err, MODE == XS_BCAST ? XSE_BCAST : XSE_XCHG, src);
        }
        if (!ok) bad = 1;
    }
    __syncthreads();
    if (bad) {
        for (int k = threadIdx.x; k < count; k += TPB) buf[k] = __builtin_nan("");
        return;
    }
    auto val = [&](int r, int k) {
        const u64 lo = rv[(r * XS_MAXV + k) * 2], hi = rv[(r * XS_MAXV + k) * 2 + 1];
        return __longlong_as_double((long long)((hi << 32) | lo));
    };
    for (int k = threadIdx.x; k < count; k += TPB) {
        if (MODE == XS_SLAB && k > 0) {
            buf[k] = 0.0;
            continue;
        }
        double s;
        if (MODE == XS_BCAST) {
            s = val(root, k);
        } else {
            s = val(0, k);
            for (int r = 1; r < nranks; ++r) s = s + val(r, k);
        }
        buf[k] = s;
    }
}

// Halo lines through the same regions: my first grid line goes to rank-1
// (its side 1), my last to rank+1 (its side 0); then wait for mine and decode
// them into hlo / hhi, the buffers the stencil reads.  One thread per point.
constexpr int XS_HALO_LINES = CF_HMAX;  // deepest halo (the temporal-blocked Chebyshev passes)

__global__ __launch_bounds__(TPB) void k_xhalo(const double *__restrict__ vec, int N, int nlines, int nl,
                                               XsPeers peers, int nranks, int rank, unsigned seq,
                                               double *__restrict__ hlo, double *__restrict__ hhi, int *err,
                                               u64 timeout) {
    // nl grid lines each way: my first nl lines go to rank-1, my last nl to rank+1
    const i64 e = (i64)blockIdx.x * TPB + threadIdx.x;
    if (e >= (i64)nl * N) return;
    const bool lo = rank > 0, hi = rank < nranks - 1;
    const unsigned par = seq & 1u;
    auto slot = [&](u64 *base, int side) {
        return base + gk::XS_RED_WORDS + (((i64)par * 2 + side) * ((i64)XS_HALO_LINES * N) + e) * 2;
    };
    if (xs_flag(err)) {
        if (lo) hlo[e] = __builtin_nan("");
        if (hi) hhi[e] = __builtin_nan("");
        return;
    }
    if (lo) {
        const u64 bits = (u64)__double_as_longlong(vec[e]);
        u64 *q = slot(peers.p[rank - 1], 1);
        xs_put(q, seq, (unsigned)bits);
        xs_put(q + 1, seq, (unsigned)(bits >> 32));
    }
    if (hi) {
        const u64 bits = (u64)__double_as_longlong(vec[(i64)(nlines - nl) * N + e]);
        u64 *q = slot(peers.p[rank + 1], 0);
        xs_put(q, seq, (unsigned)bits);
        xs_put(q + 1, seq, (unsigned)(bits >> 32));
    }
    const u64 deadline = wall_clock64() + timeout;
    u64 *mine = peers.p[rank];
    for (int side = 0; side < 2; ++side) {
        if (side == 0 ? !lo : !hi) continue;
        const u64 *q = slot(mine, side);
        unsigned a = 0, b = 0;
        double v = __builtin_nan("");
        int g = xs_get(q, seq, deadline, &a, err);
        if (g == XG_OK) g = xs_get(q + 1, seq, deadline, &b, err);
        if (g == XG_OK)
            v = __longlong_as_double((long long)(((u64)b << 32) | a));
        else if (g == XG_LATE)
            xs_fail(err, XSE_HALO, side == 0 ? rank - 1 : rank + 1);
        (side == 0 ? hlo : hhi)[e] = v;
    }
}

}  // namespace gk

using namespace gkh;

namespace {

// ----------------------------------------------------------------- comm ---
constexpr int LG_MAX = 16;
struct RankPtrs {
    const double *p[LG_MAX];
};

__global__ void k_sum_ranks(RankPtrs src, int nr, double *__restrict__ out, int count) {
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int r = 0; r < nr; ++r) s += src.p[r][k];
        out[k] = s;
    }
}

}  // namespace

namespace gkh __attribute__((visibility("hidden"))) {

// Collectives run whenever a communicator exists (also a 1-rank RCCL one); a bare grid has none.
bool collective(const gk_grid *g) {
    const gk_ctx *c = g->ctx;
    return c != nullptr && (c->xs_on || c->comm != nullptr || c->lg != nullptr);
}

// ------------------------------------------------ device exchange (xgmi) ---
void xs_set_timeout(gk_ctx *c, int ms) {
    c->xs_timeout_ms = ms;
    c->xs_timeout = (gk::u64)ms * (gk::u64)c->xs_tick_per_ms;
}

int xs_alloc(gk_ctx *c) {
    if (c->xs_buf != nullptr) return GK_OK;
    HIPCHK(hipSetDevice(c->dev));
    c->xs_words = gk::XS_RED_WORDS + 8LL * gk::XS_HALO_LINES * c->N;
    if (hipExtMallocWithFlags((void **)&c->xs_buf, sizeof(gk::u64) * c->xs_words, hipDeviceMallocUncached) !=
        hipSuccess)
        return set_err(GK_ERR_NOMEM, "cannot allocate the exchange region");
    HIPCHK(hipMemsetAsync(c->xs_buf, 0, sizeof(gk::u64) * c->xs_words, c->st));
    HIPCHK(hipMalloc((void **)&c->xs_seqdev, sizeof(unsigned)));
    HIPCHK(hipHostMalloc((void **)&c->xs_err, sizeof(int), hipHostMallocMapped));
    HIPCHK(hipHostGetDevicePointer((void **)&c->xs_err_dev, c->xs_err, 0));
    *c->xs_err = 0;
    int khz = 0;
    HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->dev));
    if (khz > 0) c->xs_tick_per_ms = khz;
    xs_set_timeout(c, c->xs_timeout_ms);
    HIPCHK(hipStreamSynchronize(c->st));  // zeroed before any peer can see the region
    return GK_OK;
}

// The straggler named by a device-side failure code (gk::xs_fail).
std::string xs_culprit(int code) {
    const int op = code >> 16, src = (code & 0xFFFF) - 1;
    char buf[160];
    switch (op) {
        case gk::XSE_XCHG: std::snprintf(buf, sizeof buf, "rank %d's all-reduce granule", src); break;
        case gk::XSE_BCAST: std::snprintf(buf, sizeof buf, "rank %d's broadcast granule", src); break;
        case gk::XSE_HALO: std::snprintf(buf, sizeof buf, "the halo line of rank %d", src); break;
        case gk::XSE_RES_WG:
            std::snprintf(buf, sizeof buf, "workgroup %d of this rank inside a resident step (not co-resident?)", src);
            break;
        case gk::XSE_RES_RANK:
            std::snprintf(buf, sizeof buf, "rank %d's total inside a resident step (rank straggling)", src);
            break;
        default: std::snprintf(buf, sizeof buf, "an unknown peer (code %d)", code); break;
    }
    return buf;
}

// After a host wait: did a device exchange miss its deadline?  The exchange is
// then retired for the life of the context: sequence numbers may differ
// between ranks after a failed solve (a pipelined step was already queued), so
// its granules cannot be trusted again (gk_xchg_enable(1) refuses from now on)
// and resident steps go to the launch path.  The exchange is NOT switched off
// here: its error flag stays set, so every later exchange of this rank fails at
// once (NaN results, GK_ERR_COMM).  To continue, the CALLER switches every rank
// to RCCL / the local group with gk_xchg_enable(0) -- all ranks together, as
// bench.py's fallback does; flipping only the rank that saw the miss would
// desynchronise the ranks' collectives.
int xs_check(gk_ctx *c) {
    const int code = c->xs_err != nullptr ? __atomic_load_n(c->xs_err, __ATOMIC_ACQUIRE) : 0;
    if (code != 0) {
        c->xs_broken = true;
        c->res_broken = true;
        return set_err(GK_ERR_COMM, "device exchange: rank %d of %d missed the %d ms deadline waiting for %s",
                       c->rank, c->nranks, c->xs_timeout_ms, xs_culprit(code).c_str());
    }
    return GK_OK;
}

// After a host wait: did a resident step miss an in-launch deadline?  Then the
// context falls back to one launch per projection for the rest of its life.
int res_check(gk_ctx *c) {
    const int code = c->res_err != nullptr ? __atomic_load_n(c->res_err, __ATOMIC_ACQUIRE) : 0;
    if (code != 0) {
        *c->res_err = 0;
        c->res_broken = true;
        return set_err(GK_ERR_COMM,
                       "resident MGS-R step: an in-launch exchange missed its %d ms deadline waiting for %s; the "
                       "launch-per-projection path is used from now on",
                       c->res_timeout_ms, xs_culprit(code).c_str());
    }
    return GK_OK;
}

// Host-side watchdog of every wait on this context's stream: the device waits
// all carry deadlines, but a kernel that is never SCHEDULED (its queue not mapped:
// more processes / streams on a device than its hardware queues) would keep the
// host waiting forever.  Past twice the longest device deadline plus a minute,
// the wait fails with GK_ERR_COMM instead.
// GK_TUNE_WATCHDOG_MS overrides the limit (tests; a deployment that knows its queue drains).
long long watchdog_ms(const gk_ctx *c) {
    return c->watchdog_ms > 0 ? (long long)c->watchdog_ms : 2LL * std::max(c->res_timeout_ms, c->xs_timeout_ms) + 60000;
}

int spin_until(gk_ctx *c, hipError_t (*query)(void *), void *obj, const char *what) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 1;; ++it) {
        const hipError_t r = query(obj);
        if (r == hipSuccess) return GK_OK;
        if (r != hipErrorNotReady) return set_err(GK_ERR_HIP, "%s: %s", what, hipGetErrorString(r));
        if ((it & 1023u) == 0) {
            const long long ms = std::chrono::duration_cast<std::chrono::milliseconds>(
                                     std::chrono::steady_clock::now() - t0).count();
            if (ms > watchdog_ms(c)) {
                // work is still queued on the stream: the context cannot be used (or its
                // buffers freed) safely any more -- every later call fails, gk_destroy
                // frees only once the stream has drained
                c->broken = true;
                return set_err(GK_ERR_COMM,
                               "%s: not complete after %lld ms (rank %d of %d): a kernel of this context was never "
                               "scheduled -- more streams on the device than hardware queues?  The context is broken.",
                               what, ms, c->rank, c->nranks);
            }
        }
    }
}

hipError_t query_stream(void *s) { return hipStreamQuery(static_cast<hipStream_t>(s)); }
hipError_t query_event(void *e) { return hipEventQuery(static_cast<hipEvent_t>(e)); }

int sync_st(gk_ctx *c) {
    CHK(spin_until(c, query_stream, c->st, "stream synchronize"));
    CHK(res_check(c));
    return xs_check(c);
}

int xs_exchange(gk_ctx *c, double *buf, int count, int mode, int root) {
    unsigned seq = ++c->xs_seq;
    const unsigned *base = nullptr;
    if (c->capturing) {  // a graph node: its number relative to the base set before each replay
        seq -= c->graph_seq0;
        base = c->xs_seqdev;
    }
    switch (mode) {
        case gk::XS_SLAB:
            gk::k_xchg<gk::XS_SLAB><<<1, gk::TPB, 0, c->st>>>(buf, count, c->xs_peers, c->nranks, c->rank, seq, base,
                                                            root, c->xs_err_dev, c->xs_timeout);
            break;
        case gk::XS_VEC:
            gk::k_xchg<gk::XS_VEC><<<1, gk::TPB, 0, c->st>>>(buf, count, c->xs_peers, c->nranks, c->rank, seq, base,
                                                           root, c->xs_err_dev, c->xs_timeout);
            break;
        default:
            gk::k_xchg<gk::XS_BCAST><<<1, gk::TPB, 0, c->st>>>(buf, count, c->xs_peers, c->nranks, c->rank, seq,
                                                             base, root, c->xs_err_dev, c->xs_timeout);
            break;
    }
    LAUNCHCHK();
    return GK_OK;
}

int lg_barrier(gk_ctx *c) {
    gk_group *g = c->lg;
    std::unique_lock<std::mutex> lk(g->mu);
    if (g->broken) return set_err(GK_ERR_STATE, "local group broken by an earlier timeout");
    const long my = g->gen;
    if (++g->arrived == g->n) {
        g->arrived = 0;
        ++g->gen;
        g->cv.notify_all();
        return GK_OK;
    }
    if (!g->cv.wait_for(lk, std::chrono::seconds(300), [&] { return g->gen != my || g->broken; }) || g->broken) {
        g->broken = true;
        g->cv.notify_all();
        return set_err(GK_ERR_STATE, "local group barrier timed out");
    }
    return GK_OK;
}

// Phase 1: publish `p` and an event after its producer; wait for everyone.
int lg_publish(gk_ctx *c, const double *p) {
    c->lg->ptrs[c->rank] = p;
    HIPCHK(hipEventRecord(c->lev_a, c->st));
    return lg_barrier(c);
}

int lg_wait(gk_ctx *c, int q, bool second) {
    gk_ctx *o = c->lg->members[q];
    HIPCHK(hipStreamWaitEvent(c->st, second ? o->lev_b : o->lev_a, 0));
    return GK_OK;
}

// `vec`: element-wise sum of a short vector; otherwise `buf` is a partial slab
// whose consumer re-reduces it (any split of the same total is equivalent).
int allreduce(gk_ctx *c, double *buf, int count, bool vec) {
    if (!collective(c)) return GK_OK;
    ProfScope ps(c, GK_KID_COMM);
    if (c->xs_on) {
        if (!vec) return xs_exchange(c, buf, count, gk::XS_SLAB, 0);
        for (int k0 = 0; k0 < count; k0 += gk::XS_MAXV)
            CHK(xs_exchange(c, buf + k0, std::min(gk::XS_MAXV, count - k0), gk::XS_VEC, 0));
        return GK_OK;
    }
    if (c->lg == nullptr) {
        NCCLCHK(ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, c->comm, c->st));
        return GK_OK;
    }
    if (count > gk::NPMAX * 4) return set_err(GK_ERR_ARG, "local allreduce too large");
    CHK(lg_publish(c, buf));
    RankPtrs rp{};
    for (int q = 0; q < c->nranks; ++q) {
        CHK(lg_wait(c, q, false));
        rp.p[q] = c->lg->ptrs[q];
    }
    k_sum_ranks<<<(count + 255) / 256, 256, 0, c->st>>>(rp, c->nranks, c->lscratch, count);
    LAUNCHCHK();
    HIPCHK(hipEventRecord(c->lev_b, c->st));
    CHK(lg_barrier(c));
    for (int q = 0; q < c->nranks; ++q) CHK(lg_wait(c, q, true));  // nobody reads buf any more
    HIPCHK(hipMemcpyAsync(buf, c->lscratch, sizeof(double) * count, hipMemcpyDeviceToDevice, c->st));
    return GK_OK;
}

int bcast(gk_ctx *c, double *buf, int count, int root) {
    if (!collective(c)) return GK_OK;
    ProfScope ps(c, GK_KID_COMM);
    if (c->xs_on) {
        for (int k0 = 0; k0 < count; k0 += gk::XS_MAXV)
            CHK(xs_exchange(c, buf + k0, std::min(gk::XS_MAXV, count - k0), gk::XS_BCAST, root));
        return GK_OK;
    }
    if (c->lg == nullptr) {
        NCCLCHK(ncclBroadcast(buf, buf, count, ncclDouble, root, c->comm, c->st));
        return GK_OK;
    }
    CHK(lg_publish(c, buf));
    if (c->rank != root) {
        CHK(lg_wait(c, root, false));
        HIPCHK(hipMemcpyAsync(buf, c->lg->ptrs[root], sizeof(double) * count, hipMemcpyDeviceToDevice, c->st));
    }
    HIPCHK(hipEventRecord(c->lev_b, c->st));
    CHK(lg_barrier(c));
    if (c->rank == root)
        for (int q = 0; q < c->nranks; ++q) CHK(lg_wait(c, q, true));
    return GK_OK;
}

// Exchange nl grid lines of vec with the slab neighbours: lo <- the last nl
// lines of rank-1 (our rows -nl..-1), hi <- the first nl lines of rank+1 (our
// rows nlines..nlines+nl-1).  nl = 1 for a stencil sweep; the temporal-blocked
// Chebyshev passes need nl = L (their recompute cone).
int halo_lines(gk_grid *g, const double *vec, int nl, double *lo, double *hi) {
    if (!collective(g)) return GK_OK;
    gk_ctx *c = g->ctx;
    // a slab thinner than the halo would send lines it does not own (and its
    // neighbours would need lines from two ranks away)
    if (c->nranks > 1 && (nl < 1 || nl > c->nlines))
        return set_err(GK_ERR_ARG, "halo of %d lines from a slab of %d lines (rank %d)", nl, c->nlines, c->rank);
    ProfScope ps(c, GK_KID_HALO);
    const int N = c->N;
    const i64 cnt = (i64)nl * N;
    if (c->xs_on) {
        if (c->nranks == 1) return GK_OK;
        const unsigned seq = ++c->xs_hseq;
        gk::k_xhalo<<<(unsigned)((cnt + gk::TPB - 1) / gk::TPB), gk::TPB, 0, c->st>>>(
            vec, N, c->nlines, nl, c->xs_peers, c->nranks, c->rank, seq, lo, hi, c->xs_err_dev, c->xs_timeout);
        LAUNCHCHK();
        return GK_OK;
    }
    if (c->lg == nullptr) {
        NCCLCHK(ncclGroupStart());
        if (c->rank > 0) {
            NCCLCHK(ncclSend(vec, cnt, ncclDouble, c->rank - 1, c->comm, c->st));
            NCCLCHK(ncclRecv(lo, cnt, ncclDouble, c->rank - 1, c->comm, c->st));
        }
        if (c->rank < c->nranks - 1) {
            NCCLCHK(ncclSend(vec + (i64)(c->nlines - nl) * N, cnt, ncclDouble, c->rank + 1, c->comm, c->st));
            NCCLCHK(ncclRecv(hi, cnt, ncclDouble, c->rank + 1, c->comm, c->st));
        }
        NCCLCHK(ncclGroupEnd());
        return GK_OK;
    }
    CHK(lg_publish(c, vec));
    if (c->rank > 0) {
        gk_ctx *o = c->lg->members[c->rank - 1];
        CHK(lg_wait(c, c->rank - 1, false));
        HIPCHK(hipMemcpyAsync(lo, c->lg->ptrs[c->rank - 1] + (i64)(o->nlines - nl) * N, sizeof(double) * cnt,
                              hipMemcpyDeviceToDevice, c->st));
    }
    if (c->rank < c->nranks - 1) {
        CHK(lg_wait(c, c->rank + 1, false));
        HIPCHK(hipMemcpyAsync(hi, c->lg->ptrs[c->rank + 1], sizeof(double) * cnt, hipMemcpyDeviceToDevice, c->st));
    }
    HIPCHK(hipEventRecord(c->lev_b, c->st));
    CHK(lg_barrier(c));
    if (c->rank > 0) CHK(lg_wait(c, c->rank - 1, true));
    if (c->rank < c->nranks - 1) CHK(lg_wait(c, c->rank + 1, true));
    return GK_OK;
}

int halo(gk_grid *g, const double *vec) {
    gk_ctx *c = g->ctx;
    return c != nullptr ? halo_lines(g, vec, 1, c->hlo, c->hhi) : GK_OK;
}

// The neighbours' lines halo() received, null at a physical boundary (a bare grid has two)
const double *halo_lo(const gk_grid *g) {
    const gk_ctx *c = g->ctx;
    return (c != nullptr && c->nranks > 1 && c->rank > 0) ? c->hlo : nullptr;
}
const double *halo_hi(const gk_grid *g) {
    const gk_ctx *c = g->ctx;
    return (c != nullptr && c->nranks > 1 && c->rank < c->nranks - 1) ? c->hhi : nullptr;
}

}  // namespace gkh

extern "C" {

int gk_comm_unique_id(unsigned char id[128]) {
    ncclUniqueId u;
    NCCLCHK(ncclGetUniqueId(&u));
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    std::memcpy(id, &u, 128);
    return GK_OK;
}

int gk_comm_init(gk_ctx *c, int nranks, int rank, int max_lines, const unsigned char id[128]) {
    if (c == nullptr || nranks < 1 || rank < 0 || rank >= nranks || max_lines < c->nlines)
        return set_err(GK_ERR_ARG, "bad comm args");
    if (cb_on(c)) return set_err(GK_ERR_STATE, "the FP32 basis needs a single-rank context (gk_set_basis_precision)");
    if (c->pkind == GK_PREC_MG) return set_err(GK_ERR_STATE, "the multigrid preconditioner needs a single-rank context");
    graph_reset(c);
    HIPCHK(hipSetDevice(c->dev));
    c->nranks = nranks;
    c->rank = rank;
    c->max_lines = max_lines;
    c->min_lines = 0;
    set_geometry(c);
    // A 1-rank RCCL communicator is only built on request (GK_FORCE_RCCL=1): it
    // routes every collective through RCCL on one GPU (used by the tests).
    const char *force = std::getenv("GK_FORCE_RCCL");
    if (nranks > 1 || (force != nullptr && force[0] == '1')) {
        ncclUniqueId u;
        std::memcpy(&u, id, 128);
        ncclComm_t cm = nullptr;  // c->comm stays null when the init fails (gk_destroy, a later
        NCCLCHK(ncclCommInitRank(&cm, nranks, u, rank));  // gk_comm_init_xgmi)
        c->comm = cm;
        c->comm_ok = true;
    }
    return GK_OK;
}

int gk_group_create(int nranks, gk_group **out) {
    if (out == nullptr || nranks < 1 || nranks > LG_MAX) return set_err(GK_ERR_ARG, "bad group size");
    gk_group *g = new gk_group();
    g->n = nranks;
    g->members.assign(nranks, nullptr);
    g->ptrs.assign(nranks, nullptr);
    *out = g;
    return GK_OK;
}

int gk_group_destroy(gk_group *g) {
    delete g;
    return GK_OK;
}

int gk_comm_init_local(gk_ctx *c, gk_group *g, int rank, int max_lines) {
    if (c == nullptr || g == nullptr || rank < 0 || rank >= g->n || max_lines < c->nlines)
        return set_err(GK_ERR_ARG, "bad local comm args");
    if (cb_on(c)) return set_err(GK_ERR_STATE, "the FP32 basis needs a single-rank context (gk_set_basis_precision)");
    if (c->pkind == GK_PREC_MG) return set_err(GK_ERR_STATE, "the multigrid preconditioner needs a single-rank context");
    graph_reset(c);
    HIPCHK(hipSetDevice(c->dev));
    c->nranks = g->n;
    c->rank = rank;
    c->max_lines = max_lines;
    c->min_lines = 0;
    set_geometry(c);
    c->lg = g;
    c->res_share = g->n;  // members may share one device: resident launches split its CUs
    HIPCHK(hipEventCreateWithFlags(&c->lev_a, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->lev_b, hipEventDisableTiming));
    if (hipMalloc(&c->lscratch, sizeof(double) * gk::NPMAX * 4) != hipSuccess)
        return set_err(GK_ERR_NOMEM, "local comm scratch");
    {
        std::lock_guard<std::mutex> lk(g->mu);
        g->members[rank] = c;
    }
    CHK(xs_alloc(c));
    c->comm_ok = true;
    return GK_OK;
}

int gk_comm_init_xgmi(gk_ctx *c, int nranks, int rank, int max_lines) {
    if (c == nullptr || nranks < 1 || nranks > gk::XS_MAXR || rank < 0 || rank >= nranks || max_lines < c->nlines)
        return set_err(GK_ERR_ARG, "bad xgmi comm args (nranks <= %d)", gk::XS_MAXR);
    if (cb_on(c)) return set_err(GK_ERR_STATE, "the FP32 basis needs a single-rank context (gk_set_basis_precision)");
    if (c->pkind == GK_PREC_MG) return set_err(GK_ERR_STATE, "the multigrid preconditioner needs a single-rank context");
    graph_reset(c);
    HIPCHK(hipSetDevice(c->dev));
    if (c->comm != nullptr) {  // an RCCL communicator of an abandoned gk_comm_init: the exchange replaces it
        // abort, not destroy: ncclCommDestroy finalises collectively and can wait on
        // peers whose init failed or that have moved on; ncclCommAbort is local
        ncclCommAbort(c->comm);
        c->comm = nullptr;
        c->comm_ok = false;
    }
    c->nranks = nranks;
    c->rank = rank;
    c->max_lines = max_lines;
    c->min_lines = 0;
    set_geometry(c);
    return xs_alloc(c);  // comm_ok once gk_xchg_open has mapped the peers
}

int gk_xchg_handle(gk_ctx *c, unsigned char handle[64]) {
    if (c == nullptr || handle == nullptr) return set_err(GK_ERR_ARG, "null argument");
    CHK(xs_alloc(c));
    hipIpcMemHandle_t h;
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t size");
    HIPCHK(hipIpcGetMemHandle(&h, c->xs_buf));
    std::memcpy(handle, &h, 64);
    return GK_OK;
}

int gk_xchg_open(gk_ctx *c, const unsigned char *handles) {
    if (c == nullptr || handles == nullptr) return set_err(GK_ERR_ARG, "null argument");
    if (c->nranks > gk::XS_MAXR) return set_err(GK_ERR_ARG, "device exchange supports <= %d ranks", gk::XS_MAXR);
    if (c->xs_ready) return set_err(GK_ERR_STATE, "exchange already open");
    CHK(xs_alloc(c));
    HIPCHK(hipSetDevice(c->dev));
    for (int r = 0; r < c->nranks; ++r) {
        if (r == c->rank) {
            c->xs_peers.p[r] = c->xs_buf;
            continue;
        }
        hipIpcMemHandle_t h;
        std::memcpy(&h, handles + 64 * (size_t)r, 64);
        void *p = nullptr;
        HIPCHK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
        c->xs_mapped.push_back(p);
        c->xs_peers.p[r] = static_cast<gk::u64 *>(p);
    }
    graph_reset(c);  // captured steps hold the collective they were captured with
    c->xs_ready = true;
    c->xs_on = true;
    c->comm_ok = true;
    return GK_OK;
}

// Hardware queues HIP gives this process per device: GPU_MAX_HW_QUEUES, else
// HIP's default of 4.
int hw_queues() {
    const char *e = std::getenv("GPU_MAX_HW_QUEUES");
    const int q = (e != nullptr && *e != '\0') ? std::atoi(e) : 4;
    return q > 0 ? q : 4;
}

int gk_xchg_local(gk_ctx *c) {
    if (c == nullptr || c->lg == nullptr) return set_err(GK_ERR_STATE, "gk_xchg_local needs gk_comm_init_local");
    if (c->nranks > gk::XS_MAXR) return set_err(GK_ERR_ARG, "device exchange supports <= %d ranks", gk::XS_MAXR);
    std::lock_guard<std::mutex> lk(c->lg->mu);
    int same_dev = 0;
    for (int r = 0; r < c->nranks; ++r) {
        gk_ctx *o = c->lg->members[r];
        if (o == nullptr || o->xs_buf == nullptr)
            return set_err(GK_ERR_STATE, "rank %d of the group has not joined yet", r);
        same_dev += o->dev == c->dev;
    }
    // Every in-process rank on this device spins on its peers' granules from its
    // own stream: the streams must not share a hardware queue, or a spinning
    // exchange kernel can sit in front of its peer's kernel until the deadline
    // (seen with 4 ranks under HIP's default of 4 queues).  One more stream (the
    // null stream) may hold a queue too.
    const int q = hw_queues();
    if (same_dev + 1 > q)
        return set_err(GK_ERR_STATE,
                       "%d in-process ranks on device %d (+1 stream) need more than the %d hardware queues of this "
                       "process (GPU_MAX_HW_QUEUES): their spinning exchange kernels would deadlock; set "
                       "GPU_MAX_HW_QUEUES >= %d before the HIP runtime starts",
                       same_dev, c->dev, q, same_dev + 1);
    for (int r = 0; r < c->nranks; ++r) c->xs_peers.p[r] = c->lg->members[r]->xs_buf;
    graph_reset(c);
    c->xs_ready = true;
    c->xs_on = true;
    return GK_OK;
}

int gk_xchg_enable(gk_ctx *c, int on) {
    if (c == nullptr) return set_err(GK_ERR_ARG, "null context");
    graph_reset(c);
    if (on && !c->xs_ready) return set_err(GK_ERR_STATE, "exchange not open");
    if (on && c->xs_broken)
        return set_err(GK_ERR_STATE, "device exchange retired after a missed deadline (sequence numbers may "
                                     "differ between ranks)");
    if (!on && c->comm == nullptr && c->lg == nullptr && c->nranks > 1)
        return set_err(GK_ERR_STATE, "no RCCL or local communicator to fall back to");
    c->xs_on = on != 0;
    if (!c->xs_on && c->xs_err != nullptr) *c->xs_err = 0;  // a missed deadline does not outlive the switch
    return GK_OK;
}

}  // extern "C"

namespace gkh __attribute__((visibility("hidden"))) {
double host_hash(long long g, unsigned long long seed) {  // = gk::k_fill_hash
    unsigned long long z = (unsigned long long)g + seed * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

int xs_selftest_body(gk_ctx *c, std::string &why) {
    const int R = c->nranks, me = c->rank;
    // element-wise sum of a short vector
    double hv[8];
    for (int k = 0; k < 8; ++k) hv[k] = (me + 1) * (k + 1) + 0.25 * k;
    double *d = slot(c, 3);
    HIPCHK(hipMemcpyAsync(d, hv, sizeof hv, hipMemcpyHostToDevice, c->st));
    CHK(allreduce(c, d, 8, true));
    // a partial slab: 5 partials of (rank+1) -> {5 * sum(rank+1), 0, 0, 0, 0}
    double hs[5];
    for (double &v : hs) v = me + 1.0;
    double *e = slot(c, 2);
    HIPCHK(hipMemcpyAsync(e, hs, sizeof hs, hipMemcpyHostToDevice, c->st));
    CHK(allreduce(c, e, 5));
    // broadcast from the last rank
    double hb[3] = {me + 0.5, -me - 0.5, 1e300 * (me + 1)};
    HIPCHK(hipMemcpyAsync(c->hb, hb, sizeof hb, hipMemcpyHostToDevice, c->st));
    CHK(bcast(c, c->hb, 3, R - 1));
    // halo lines of a globally indexed vector
    CHK(fill_hash(c, c->vj, 7));
    CHK(halo(c, c->vj));
    double rv[8], rs[5], rb[3];
    std::vector<double> lo(c->N), hi(c->N);
    HIPCHK(hipMemcpyAsync(rv, d, sizeof rv, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(rs, e, sizeof rs, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(rb, c->hb, sizeof rb, hipMemcpyDeviceToHost, c->st));
    if (me > 0) HIPCHK(hipMemcpyAsync(lo.data(), c->hlo, sizeof(double) * c->N, hipMemcpyDeviceToHost, c->st));
    if (me < R - 1) HIPCHK(hipMemcpyAsync(hi.data(), c->hhi, sizeof(double) * c->N, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    if (*c->xs_err) {
        why = "missed the deadline waiting for " + xs_culprit(*c->xs_err);
        return GK_ERR_COMM;
    }
    for (int k = 0; k < 8; ++k) {
        double ex = 0.0;
        for (int r = 0; r < R; ++r) ex = ex + ((r + 1) * (k + 1) + 0.25 * k);
        if (rv[k] != ex) why = "vector all-reduce mismatch";
    }
    if (rs[0] != 5.0 * (R * (R + 1) / 2) || rs[1] != 0.0 || rs[4] != 0.0) why = "slab all-reduce mismatch";
    const int rt = R - 1;
    if (rb[0] != rt + 0.5 || rb[1] != -rt - 0.5 || rb[2] != 1e300 * (rt + 1)) why = "broadcast mismatch";
    for (int i = 0; i < c->N; ++i) {
        if (me > 0 && lo[i] != host_hash(c->g0 - c->N + i, 7)) why = "lower halo mismatch";
        if (me < R - 1 && hi[i] != host_hash(c->g0 + c->nloc + i, 7)) why = "upper halo mismatch";
    }
    return why.empty() ? GK_OK : GK_ERR_COMM;
}
}  // namespace gkh

extern "C" {

int gk_peer_info(int device, int peer, int *can_access, int *link_type, int *hops) {
    if (can_access == nullptr || link_type == nullptr || hops == nullptr) return set_err(GK_ERR_ARG, "null out");
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || peer < 0 || device >= n || peer >= n)
        return set_err(GK_ERR_ARG, "devices %d, %d outside 0..%d", device, peer, n - 1);
    *can_access = 1;
    *link_type = 0;
    *hops = 0;
    if (device == peer) return GK_OK;
    HIPCHK(hipDeviceCanAccessPeer(can_access, device, peer));
    unsigned lt = 0, hc = 0;
    HIPCHK(hipExtGetLinkTypeAndHopCount(device, peer, &lt, &hc));
    *link_type = (int)lt;
    *hops = (int)hc;
    return GK_OK;
}

int gk_xchg_selftest(gk_ctx *c, int timeout_ms) {
    CHK(check_ctx(c));
    if (!c->xs_ready) return set_err(GK_ERR_STATE, "exchange not open");
    HIPCHK(hipSetDevice(c->dev));
    {  // tests: this rank fails at once without taking part (its peers then miss their deadline)
        const char *f = std::getenv("GK_DEBUG_SELFTEST_FAIL");
        if (f != nullptr && f[0] != '\0' && std::atoi(f) == c->rank) {
            c->xs_on = false;
            graph_reset(c);
            if (c->comm == nullptr && c->lg == nullptr) c->comm_ok = c->nranks == 1;
            return set_err(GK_ERR_COMM, "device exchange self-test failed on rank %d: forced (GK_DEBUG_SELFTEST_FAIL)",
                           c->rank);
        }
    }
    const bool was_on = c->xs_on;
    const int t_keep = c->xs_timeout_ms;
    if (!was_on) graph_reset(c);  // graphs captured on another collective must not replay over this one
    c->xs_on = true;
    xs_set_timeout(c, timeout_ms > 0 ? timeout_ms : t_keep);
    std::string why;
    int rc = xs_selftest_body(c, why);
    if (rc == GK_ERR_HIP || rc == GK_ERR_ARG) why = g_err;
    xs_set_timeout(c, t_keep);
    if (rc != GK_OK) {
        (void)hipStreamSynchronize(c->st);
        *c->xs_err = 0;
        c->xs_on = false;
        graph_reset(c);  //  graphs captured over the exchange would replay its k_xchg nodes
        if (c->comm == nullptr && c->lg == nullptr) c->comm_ok = c->nranks == 1;
        return set_err(GK_ERR_COMM, "device exchange self-test failed on rank %d: %s", c->rank, why.c_str());
    }
    (void)was_on;
    return GK_OK;
}

int gk_comm_latency(gk_ctx *c, int iters, double *allreduce_us, double *halo_us) {
    CHK(check_ctx(c));
    if (iters < 1 || allreduce_us == nullptr || halo_us == nullptr) return set_err(GK_ERR_ARG, "bad arguments");
    *allreduce_us = *halo_us = 0.0;
    if (!collective(c)) return GK_OK;
    HIPCHK(hipSetDevice(c->dev));
    hipEvent_t e[3];
    for (auto &x : e) HIPCHK(hipEventCreate(&x));
    double *buf = slot(c, 0);
    const int count = std::max(1, c->np_pj);  // one projection's partial slab, as the launch path sends it
    int rc = allreduce(c, buf, count);         // warm: first-call setup stays out of the timing
    if (rc == GK_OK) rc = halo(c, c->w);
    if (rc == GK_OK) rc = hipEventRecord(e[0], c->st) == hipSuccess ? GK_OK : GK_ERR_HIP;
    for (int i = 0; i < iters && rc == GK_OK; ++i) rc = allreduce(c, buf, count);
    if (rc == GK_OK) rc = hipEventRecord(e[1], c->st) == hipSuccess ? GK_OK : GK_ERR_HIP;
    for (int i = 0; i < iters && rc == GK_OK; ++i) rc = halo(c, c->w);
    if (rc == GK_OK) rc = hipEventRecord(e[2], c->st) == hipSuccess ? GK_OK : GK_ERR_HIP;
    if (rc == GK_OK) rc = sync_st(c);
    float a = 0.f, b = 0.f;
    if (rc == GK_OK && (hipEventElapsedTime(&a, e[0], e[1]) != hipSuccess ||
                        hipEventElapsedTime(&b, e[1], e[2]) != hipSuccess))
        rc = set_err(GK_ERR_HIP, "event timing failed");
    for (auto &x : e) (void)hipEventDestroy(x);
    if (rc != GK_OK) return rc;
    *allreduce_us = 1e3 * a / iters;
    *halo_us = 1e3 * b / iters;
    return GK_OK;
}

int gk_comm_info(gk_ctx *c, int *kind, int *nranks_seen) {
    if (c == nullptr || kind == nullptr || nranks_seen == nullptr) return set_err(GK_ERR_ARG, "null argument");
    *kind = GK_COMM_NONE;
    *nranks_seen = 1;
    if (c->xs_on) {
        *kind = GK_COMM_XGMI;
        int k = 0;
        for (int r = 0; r < c->nranks; ++r) k += c->xs_peers.p[r] != nullptr;
        *nranks_seen = k;
    } else if (c->lg != nullptr) {
        *kind = GK_COMM_LOCAL;
        *nranks_seen = c->lg->n;
    } else if (c->comm != nullptr) {
        *kind = GK_COMM_RCCL;
        NCCLCHK(ncclCommCount(c->comm, nranks_seen));
    }
    return GK_OK;
}

}  // extern "C"
