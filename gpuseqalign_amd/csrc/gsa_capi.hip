// gsa_capi.hip -- extern "C" boundary of libgsa.so (declared in include/gsa.h): the context, the
// fills, the checks and traces; the score-only and database entry points are in gsa_score.hip, the
// context's type and the helpers both share in gsa_ctx.h.
//
// Device-resident entry points enqueue the wavefront fills (nw_krow.hip sparse, nw_lane.hip full,
// nw_strip.hip for the GSA_SPARSE_KERNEL=strip fallback); host-buffer
// entry points reproduce what the reference's align functions do around their kernels
// (allocate, copy in, fill, copy out, Stopwatch laps):
//   NwAlign_Gpu3_Ml_DiagDiag        nwalign_gpu3_ml_diagdiag.cu:288-596     -> gsa_align_full
//   NwAlign_Gpu9_Mlsp_DiagDiagDiag  nwalign_gpu9_mlsp_diagdiagdiag.cu:368-722 -> gsa_align_sparse
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/gsa.h"
#include "gsa_ctx.h"
#include "nw_check.h"
#include "nw_lane.h"
#include "nw_expand.h"
#include "nw_krow.h"
#include "nw_strip.h"
#include "nw_trace_dev.h"

namespace gsa {
int fold_moves(const unsigned char* moves, int64_t n, char* edit, int64_t cap, int64_t* edit_len, uint32_t* trace_hash);
}

// The grow-only buffers more than one entry point reserves, each with its floor: the host-buffer
// entry points' I/O buffers, the hand-off granules (8-byte words) and the pair descriptors.
// (Declared in gsa_ctx.h: gsa_score.hip calls them too.)
int ensure_dev(gsa_ctx* ctx, int slot, size_t bytes) { return reserve_hard(ctx, ctx->buf[kBufIo0 + slot], bytes, 256); }

int ensure_gran(gsa_ctx* ctx, size_t elems, hipStream_t st)
{
    return reserve_zeroed(ctx, ctx->buf[kBufGran], elems * sizeof(unsigned long long), 0, st);
}

int ensure_desc(gsa_ctx* ctx, size_t n)
{
    return reserve_hard(ctx, ctx->buf[kBufDesc], n * sizeof(gsa::PairDesc), 64 * sizeof(gsa::PairDesc));
}

namespace {

// Knobs: measurement and test switches, named as environment variables.  A context reads them
// once, from the environment, when it is created (gsa_ctx_create); gsa_set_knob changes them per
// context.  Launches never read the environment.
constexpr const char* kKnobNames[] = {
    "GSA_SPARSE_KERNEL", "GSA_KROW_K",      "GSA_KROW_NS",      "GSA_KROW_Q8",       "GSA_LANE_NS",
    "GSA_LANE_FEED",     "GSA_LANE_PAIR",   "GSA_FULL_KERNEL",  "GSA_FULL_FUSED",    "GSA_FULL_SPLIT",
    "GSA_FUSED_STAGED",
    "GSA_EXPAND_RR",     "GSA_BATCH_ORDER", "GSA_SCORE_SCAN",   "GSA_SCORE_KERNEL",  "GSA_SCORE_K",
    "GSA_SCORE_BIDI",    "GSA_SCORE_BIDI_SW", "GSA_BIDI_GRAN",  "GSA_BIDI_SKEW",     "GSA_BIDI_SW_CONT",
    "GSA_BIDI_LOG",      "GSA_TRACE_BAND",  "GSA_TRACE_BAND_BUDGET", "GSA_STAMPS",     "GSA_DB_LANES",
    "GSA_DB_MAXC"};

bool knob_known(const char* name)
{
    for (const char* k : kKnobNames)
        if (std::strcmp(k, name) == 0) return true;
    return false;
}

// Sparse fills run on the K-rows-per-lane kernel (nw_krow.hip, K = 4): 5.9 vs 8.0 ms for the
// 100k pair and 5.7 vs 4.3 TCUPS for 512 pairs of 20k against the strip kernel (nw_strip.hip).
// mlsppt runs on the K-rows kernel too, in its (NS 4, K 4) geometry (one tile row per ticket,
// enqueue_batch).  GSA_SPARSE_KERNEL=strip forces the strip kernel (read per launch, tested);
// GSA_KROW_K (2, 4) and GSA_KROW_NS (2, 4, 8) pick the K-rows geometry.
enum SparseKern { kSpStrip, kSpKrow };
SparseKern sparse_kernel(const gsa_ctx* ctx)
{
    const char* e = knob(ctx, "GSA_SPARSE_KERNEL");
    return (e && std::strcmp(e, "strip") == 0) ? kSpStrip : kSpKrow;
}



// Full fills run on the one-row-per-lane kernel (nw_lane.hip); GSA_LANE_NS = lane strips per
// workgroup (1..4, 6, 8; read per launch, tested; 4 is the default and the fastest measured).
int lane_ns(const gsa_ctx* ctx)
{
    const char* e = knob(ctx, "GSA_LANE_NS");
    const int v = e ? std::atoi(e) : gsa::kLaneNSDefault;
    return ((v >= 1 && v <= 4) || v == 6 || v == 8) ? v : gsa::kLaneNSDefault;
}

// Verification launch (nw_check.hip): zero the result words, launch, read them back.
int run_check(gsa_ctx* ctx, gsa::CheckArgs& a, bool sparse, hipStream_t st, gsa_check_result* out)
{
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    int s = reserve_hard(ctx, ctx->buf[kBufChk], 64);
    if (s != GSA_SUCCESS) return s;
    unsigned long long* const chk = ctx->buf[kBufChk].as<unsigned long long>();
    const unsigned long long init[3] = {0ull, 0ull, ~0ull};
    unsigned long long res[3];
    if ((e = hipMemcpyAsync(chk, init, sizeof(init), hipMemcpyHostToDevice, st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    a.res = chk;
    e = sparse ? gsa::launch_check_sparse(a, ctx->cu_count, st) : gsa::launch_check_full(a, st);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    if ((e = hipMemcpyAsync(res, chk, sizeof(res), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    out->checked = (int64_t)res[0];
    out->mismatches = (int64_t)res[1];
    out->first = res[1] ? (int64_t)res[2] : -1;
    return GSA_SUCCESS;
}

// The fused two-pass full fill's launch (enqueue_full_twopass): the expansion's arguments, the
// pass-1 geometry (ns strips per ticket), the workgroup's waves and the workgroups that take pass-1
// tickets first
struct FusedLaunch
{
    const gsa::ExpandArgs* xa;
    int ns, waves, p1;
    bool staged;  // nw_full_fused_kernel's row-64m hand-off through a storer wave (PTF 3), else direct
};

}  // namespace

// (batch_schedule and stage_descs are declared in gsa_ctx.h: gsa_score.hip calls them too.)

// Batch schedule (more than one pair): round-robin over the pairs, longest first, so the resident
// workgroups run the first tickets of every pair side by side instead of one pair's chain of
// dependent tickets; ticket j of a pair stays behind its ticket j-1.  Two ints per ticket, {pair,
// ticket within the pair}; empty for one pair or with GSA_BATCH_ORDER=pair (pair-major, comparisons).
std::vector<int> batch_schedule(const gsa_ctx* ctx, const std::vector<gsa::PairDesc>& hd, long long tickets)
{
    std::vector<int> sched;
    const int npairs = (int)hd.size();
    const char* order = knob(ctx, "GSA_BATCH_ORDER");
    if (npairs > 1 && !(order && std::strcmp(order, "pair") == 0))
    {
        std::vector<int> ord((size_t)npairs);
        for (int p = 0; p < npairs; ++p) ord[(size_t)p] = p;
        std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return hd[(size_t)x].nTickets > hd[(size_t)y].nTickets; });
        sched.reserve(2 * (size_t)tickets);
        for (int j = 0; j < hd[(size_t)ord[0]].nTickets; ++j)
            for (int p : ord)
            {
                if (hd[(size_t)p].nTickets <= j) break;
                sched.push_back(p);
                sched.push_back(j);
            }
    }
    return sched;
}

// The descriptors, then the schedule, into one device buffer (ddesc, units of PairDesc): staged
// in a pinned slot and copied in stream order.
int stage_descs(gsa_ctx* ctx, const std::vector<gsa::PairDesc>& hd, const std::vector<int>& sched, hipStream_t st)
{
    const size_t npairs = hd.size();
    const size_t schedUnits = (sched.size() * sizeof(int) + sizeof(gsa::PairDesc) - 1) / sizeof(gsa::PairDesc);
    const size_t units = npairs + schedUnits;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    int s = ensure_desc(ctx, units);
    if (s != GSA_SUCCESS) return s;
    void* host = nullptr;
    if ((s = ctx->stage.acquire(units * sizeof(gsa::PairDesc), &host, &e)) != GSA_SUCCESS) return fail(ctx, e, s);
    gsa::PairDesc* const hdesc = (gsa::PairDesc*)host;
    std::memcpy(hdesc, hd.data(), npairs * sizeof(gsa::PairDesc));
    if (!sched.empty()) std::memcpy(hdesc + npairs, sched.data(), sched.size() * sizeof(int));
    e = hipMemcpyAsync(ctx->buf[kBufDesc].p, hdesc, units * sizeof(gsa::PairDesc), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = ctx->stage.commit(st);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    return GSA_SUCCESS;
}

namespace {

// GSA_STAMPS=1: n stamp words for the launch about to go onto st, cleared on every launch
// (gsa_debug_stamps reads them behind it)
int reserve_stamps(gsa_ctx* ctx, size_t n, hipStream_t st, unsigned long long** stamps)
{
    ctx->stamps_n = 0;
    Buf& b = ctx->buf[kBufStamps];
    const int s = reserve_hard(ctx, b, n * sizeof(unsigned long long));
    if (s != GSA_SUCCESS) return s;
    const hipError_t e = hipMemsetAsync(b.p, 0, n * sizeof(unsigned long long), st);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    *stamps = b.as<unsigned long long>();
    ctx->stamps_n = n;
    ctx->stamps_stream = st;
    return GSA_SUCCESS;
}

// One batched launch: headers of every pair, then the persistent strip kernel over the
// tickets of all pairs (pair-major).  `pairs` holds device pointers.
int enqueue_batch(gsa_ctx* ctx, int mode, int npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                  int32_t gapo, int32_t tileBx, hipStream_t st, unsigned long long* done = nullptr, int ptChunk = 0,
                  const int32_t* lds = nullptr, int* const* rows64 = nullptr, const FusedLaunch* fused = nullptr)
{
    if (npairs < 1 || !pairs || !subst) return GSA_ERROR_INVALID_VALUE;
    if (substsz < 1 || substsz > 32) return GSA_ERROR_INVALID_VALUE;  // LDS profile holds <= 32 letters
    gsa::StripArgs a;
    std::memset(&a, 0, sizeof(a));
    a.subst = subst;
    a.substsz = substsz;
    a.g = gapo;
    const bool lane = mode == gsa::kModeFull;
    // mlsppt publishes column chunks from the K-rows kernel only
    const bool krow = mode == gsa::kModeSparse && (sparse_kernel(ctx) == kSpKrow || done || rows64);
    // single pairs: 4 strips per workgroup (each on its own SIMD: the pair's critical path);
    // batches: 8 (two strips per SIMD share the issue slots a single strip leaves idle, 512 x 20k
    // 5.7 -> 7.3 TCUPS; a single 100k pair 5.9 -> 8.4 ms), unless the batch's 4-strip tickets
    // (one tile row each) all fit the chip at once: then every pair runs on its critical path
    long long tileRows = 0;
    for (int p = 0; p < npairs; ++p)
        tileRows += std::max<long long>(1, ((long long)pairs[p].adjrows - 1 + gsa::kSparseTileBy - 1) / gsa::kSparseTileBy);
    const bool fitsChip = tileRows <= (long long)std::max(1, ctx->cu_count);
    const int nsDefault = (npairs > 1 && !fitsChip) ? gsa::kKrowNSBatchDefault : gsa::kKrowNSDefault;
    int krowK = env_int(ctx, "GSA_KROW_K", gsa::kKrowKDefault), krowNS = env_int(ctx, "GSA_KROW_NS", nsDefault);
    if (rows64)  // pass 1 of the two-pass full fill: the XR instances, K = 4 on 4 or 8 strips
    {
        krowK = 4;
        krowNS = fused ? fused->ns : env_int(ctx, "GSA_KROW_NS", (npairs > 1 && !fitsChip) ? 8 : 4) == 8 ? 8 : 4;
    }
    // mlsppt flags one ticket per tile row: only the geometry whose ticket is one tile row
    if (!gsa::krow_ok(krowNS, krowK) || (done && gsa::krow_ticket_rows(krowNS, krowK) != gsa::kSparseTileBy))
    {
        krowK = gsa::kKrowKDefault;
        krowNS = gsa::kKrowNSDefault;
    }
    a.ns = lane ? lane_ns(ctx) : krow ? krowNS : gsa::kSparseNS;
    // the K-rows fill's int8 column profile (its instance declines a table outside int8 and the int16
    // one runs instead) wherever its LDS fits; GSA_KROW_Q8=0 keeps the int16 profile
    if (krow && env_int(ctx, "GSA_KROW_Q8", 1) != 0)
    {
        const size_t lds8 = fused ? gsa::full_fused_lds_bytes(krowNS, substsz, true, fused->staged)
                                  : gsa::krow_lds_bytes(krowNS, krowNS == 2 ? 512 : 1024, substsz, true);
        a.q8 = lds8 <= (size_t)ctx->lds_max ? 1 : 0;
    }
    a.q8flag = ctx->ctl + 2;
    const int fullRows = gsa::kLaneRows * a.ns;  // rows per ticket of a full fill
    if (mode == gsa::kModeSparse)
    {
        if (tileBx < 64 || tileBx % 16 != 0) return GSA_ERROR_INVALID_VALUE;
        a.tBx = tileBx;
        a.tBy = gsa::kSparseTileBy;
    }
    std::vector<gsa::PairDesc> hd((size_t)npairs);
    long long tickets = 0, gran = 0, maxWork = 1, span = 1;
    for (int p = 0; p < npairs; ++p)
    {
        const gsa_pair_dev& in = pairs[p];
        if (in.adjrows < 1 || in.adjcols < 1 || !in.seqY || !in.seqX) return GSA_ERROR_INVALID_VALUE;
        gsa::PairDesc& d = hd[(size_t)p];
        std::memset(&d, 0, sizeof(d));
        d.seqY = in.seqY;
        d.seqX = in.seqX;
        d.R = in.adjrows - 1;
        d.C = in.adjcols - 1;
        if (mode == gsa::kModeFull)
        {
            if (!in.score) return GSA_ERROR_INVALID_VALUE;
            d.score = in.score;
            // row pitch: unpadded, or the caller's (gsa_full_pitch gives the one whose anti-diagonals
            // share their 128-byte line offset, so the strips' row segments are whole lines)
            d.ld = lds ? lds[p] : in.adjcols;
            if (d.ld < in.adjcols) return GSA_ERROR_INVALID_VALUE;
            d.Cp = d.C;
            // an empty row or column leaves nothing but headers to compute
            d.nTickets = (d.C == 0) ? 0 : (d.R + fullRows - 1) / fullRows;
            maxWork = std::max<long long>(maxWork, (long long)std::max(d.R, d.C) + 1);
        }
        else
        {
            if (!in.tileHrowMat || !in.tileHcolMat) return GSA_ERROR_INVALID_VALUE;
            gsa_sparse_geom geom;
            int s = gsa_sparse_geometry(in.adjrows, in.adjcols, tileBx, &geom);
            if (s != GSA_SUCCESS) return s;
            d.hrow = in.tileHrowMat;
            d.hcol = in.tileHcolMat;
            d.trows = geom.tileHdrMatRows;
            d.tcols = geom.tileHdrMatCols;
            d.Cp = d.tcols * tileBx;
            d.nTickets = krow ? gsa::krow_tickets(d.trows, krowNS, krowK) : d.trows;
            if (rows64)
            {
                d.rows64 = rows64[p];
                d.rpitch = gsa::rows64_pitch(d.Cp);
            }
            maxWork = std::max<long long>(maxWork, std::max((long long)d.tcols * (tileBx + 1),
                                                            (long long)d.trows * (gsa::kSparseTileBy + 1)));
            // the largest min(i, j) over the cells an output word depends on (StripArgs::qcap): header rows
            // end at row (trows - 1) tBy and run to column Cp, header columns end at column (tcols - 1) tBx
            // and run to row trows tBy; pass 1 of a full fill is read inside the matrix only.  Cells past
            // both may wrap: nothing reads them.
            const long long tBy = gsa::kSparseTileBy;
            span = std::max(span, rows64 ? (long long)std::min(d.R, d.C)
                                         : std::max(std::min<long long>((d.trows - 1) * tBy, d.Cp),
                                                    std::min<long long>(d.trows * tBy, (long long)(d.tcols - 1) * tileBx)));
        }
        d.ticketBase = (int)tickets;
        d.granOff = gran;
        tickets += d.nTickets;
        gran += (long long)d.nTickets * gsa::gran_stride(d.Cp);
        if (tickets > (1ll << 30)) return GSA_ERROR_INVALID_VALUE;
    }
    const std::vector<int> sched = batch_schedule(ctx, hd, tickets);
    hipError_t e;
    int s = stage_descs(ctx, hd, sched, st);
    if (s != GSA_SUCCESS) return s;

    gsa::PairDesc* const ddesc = ctx->buf[kBufDesc].as<gsa::PairDesc>();
    a.pairs = ddesc;
    a.nPairs = npairs;
    a.nTicketsTotal = (int)tickets;
    a.sched = sched.empty() ? nullptr : (const int*)(ddesc + npairs);
    a.qcap = (int)(0x7fffffffll / span);
    e = gsa::launch_headers(a, mode, maxWork, st);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    // gsa_last_launch: the instance decided above (a two-pass full fill's caller then names the kind)
    auto record = [&](unsigned epoch) {
        gsa_launch_info& li = new_launch_info(
            ctx, lane ? GSA_LAUNCH_FULL_LANE : krow ? GSA_LAUNCH_SPARSE_KROW : GSA_LAUNCH_SPARSE_STRIP, st, epoch);
        li.ns = a.ns;
        li.k = krow ? krowK : 1;
        li.q8 = a.q8;
        li.mlsppt = done ? 1 : 0;
        li.npairs = npairs;
        li.pair_major = (npairs > 1 && sched.empty()) ? 1 : 0;
        li.tickets = tickets;
    };
    if (tickets == 0)
    {
        record(0);  // headers only
        return GSA_SUCCESS;
    }

    // granule stride (Cp+1) and base are per pair: the kernel takes them from the descriptor
    if ((s = ensure_gran(ctx, (size_t)gran, st)) != GSA_SUCCESS) return s;
    a.gran = ctx->buf[kBufGran].as<unsigned long long>();
    a.ticket = ctx->ctl;
    a.err = ctx->ctl + 1;
    a.spin = ctx->spin_ticks;
    a.done = done;
    a.ptChunk = std::max(1, ptChunk);
    a.epoch = ++ctx->epoch;
    if (a.epoch == 0) a.epoch = ++ctx->epoch;  // 0 is the cleared-tag value
    if (fused)
    {
        if (!rows64) return GSA_ERROR_INVALID_VALUE;
        const size_t words = (size_t)tickets * (size_t)krowNS;
        if ((s = reserve_zeroed(ctx, ctx->buf[kBufXdone], words * sizeof(unsigned long long),
                                1024 * sizeof(unsigned long long), st)) != GSA_SUCCESS)
            return s;
        {
            a.xpair = fused->xa->pairs;
            a.xsched = fused->xa->sched;
            a.xTasks = fused->xa->nTasks;
            a.xrun = fused->xa->run;
            a.xP = fused->p1;
            a.xrole = ctx->ctl + 4;
            a.xcounter = ctx->ctl + 5;
            if ((e = hipMemsetAsync(a.xrole, 0, 8, st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
            ctx->stamps_n = 0;
            if (env_int(ctx, "GSA_STAMPS", 0) &&
                (s = reserve_stamps(ctx, 4 * words + 3 * (size_t)a.xTasks, st, &a.stamps)) != GSA_SUCCESS)
                return s;
        }
        a.xdone = ctx->buf[kBufXdone].as<unsigned long long>();
    }
    if (!fused && krow && !lane && env_int(ctx, "GSA_STAMPS", 0))
    {
        // the K-rows fill's ledger (nw_krow_kernel): 10 words per strip
        if ((s = reserve_stamps(ctx, 10 * (size_t)tickets * (size_t)krowNS, st, &a.stamps)) != GSA_SUCCESS) return s;
    }
    e = hipMemsetAsync(ctx->ctl, 0, 4, st);  // the ticket; the error word stays sticky
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    // one pair: one workgroup per CU (its tickets are a chain); a batch: all resident slots
    int grid = (npairs == 1) ? std::max(1, std::min((int)tickets, ctx->cu_count)) : 0;
    a.laneFeed = knob(ctx, "GSA_LANE_FEED") ? env_int(ctx, "GSA_LANE_FEED", 0) : -1;
    a.lanePair = knob(ctx, "GSA_LANE_PAIR") ? env_int(ctx, "GSA_LANE_PAIR", 0) : -1;
    e = lane     ? gsa::launch_lane_fill(a, a.ns, grid, st)
        : fused  ? gsa::launch_full_fused(a, fused->ns, fused->waves, fused->staged, 0, st)
        : rows64 ? gsa::launch_krow_fill_xr(a, krowNS, grid, st)
        : krow   ? gsa::launch_krow_fill(a, krowNS, krowK, 0, grid, st)
                 : gsa::launch_strip_fill(a, mode, grid, st);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    note_launch(ctx);
    record(a.epoch);
    return GSA_SUCCESS;
}

int enqueue_fill(gsa_ctx* ctx, int mode, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                 const int32_t* subst, int32_t substsz, int32_t gapo, int32_t* score, int32_t tileBx, int32_t* hrow,
                 int32_t* hcol, hipStream_t st, unsigned long long* done = nullptr, int ptChunk = 0,
                 const int32_t* ld = nullptr)
{
    gsa_pair_dev p {seqY, adjrows, seqX, adjcols, score, hrow, hcol};
    return enqueue_batch(ctx, mode, 1, &p, subst, substsz, gapo, tileBx, st, done, ptChunk, ld);
}

// enqueue_full_twopass's answer when its pass-1 scratch (header rows and columns plus every 64th
// row, ~2 % of the matrix) does not fit next to the caller's matrix: enqueue_full then runs the
// one-pass lane fill, which needs no scratch
constexpr int kNoScratch = -1000;

// Full fills in two passes (nw_expand.h): pass 1 = the K-rows sparse fill of every pair with tile
// width kExpTW, which also keeps rows 64m (XR instance), into the context's scratch; pass 2 =
// every 64-row x kExpTW tile of every matrix recomputed from its top row and left column at once.
// lds: row pitches (null: unpadded).
// (enqueue_full_split: slot 1 = the tail group's scratch; afterP1 recorded behind pass 1, beforeP1
// awaited before it; split: the caller records the timing events and no clock stamps are taken;
// rr >= 0: that expansion order, untuned; startEv: recorded on st just before pass 1)
struct TwoPassOpts
{
    int slot = 0;
    hipEvent_t afterP1 = nullptr, beforeP1 = nullptr, timeP1 = nullptr, startEv = nullptr;
    bool split = false;
    int rr = -1;
};
int enqueue_full_twopass(gsa_ctx* ctx, int npairs, const gsa_pair_dev* pairs, const int32_t* lds, const int32_t* subst,
                         int32_t substsz, int32_t gapo, hipStream_t st, const TwoPassOpts& opt = TwoPassOpts())
{
    Buf& exbuf = ctx->buf[kBufExp0 + opt.slot];
    Buf& exdesc = ctx->buf[kBufExpDesc0 + opt.slot];
    gsa_ctx::XTune& xt = ctx->xt[opt.slot];
    if (npairs < 1 || !pairs || !subst) return GSA_ERROR_INVALID_VALUE;
    if (substsz < 1 || substsz > 32) return GSA_ERROR_INVALID_VALUE;
    // pass-1 geometry as enqueue_batch derives it for the XR instances
    long long tileRows = 0;
    for (int p = 0; p < npairs; ++p)
        tileRows += std::max<long long>(1, ((long long)pairs[p].adjrows - 1 + gsa::kSparseTileBy - 1) / gsa::kSparseTileBy);
    const bool fitsChip = tileRows <= (long long)std::max(1, ctx->cu_count);
    // both passes in one launch (nw_full_fused_kernel) for single pairs; GSA_FULL_FUSED=0: two launches.
    // (A matrix without interior cells has no pass-1 tickets: the expansion alone writes its headers.)
    const int fusedMode = env_int(ctx, "GSA_FULL_FUSED", 1);
    bool interior = true;
    for (int p = 0; p < npairs; ++p) interior = interior && pairs[p].adjrows > 1 && pairs[p].adjcols > 1;
    // (never inside a split batch: a group of one pair would take the fused branch, which records
    // neither afterP1 nor timeP1, and group B would then start against an unrecorded event)
    const bool fused = interior && !opt.split && npairs == 1 && fusedMode >= 1;
    // (as enqueue_batch; the fused launch has its 4-strip instance only: launch_full_fused)
    const int ns = fused ? 4 : env_int(ctx, "GSA_KROW_NS", (npairs > 1 && !fitsChip) ? 8 : 4) == 8 ? 8 : 4;
    // pass 2 (fused or its own launch): the streamed expansion, kExpStreamWaves - 1 tile waves per
    // workgroup, tasks of that many 64-row tiles
    const int xWaves = gsa::kExpStreamWaves - 1;
    const int xmt = 1;
    std::vector<gsa_pair_dev> p1((size_t)npairs);
    std::vector<gsa::ExpandPair> ex((size_t)npairs);
    std::vector<size_t> off((size_t)npairs * 3);
    size_t bytes = 0;
    auto take = [&](size_t b) {
        const size_t o = bytes;
        bytes += (b + 255) & ~(size_t)255;
        return o;
    };
    long long tasks = 0, strips = 0;
    for (int p = 0; p < npairs; ++p)
    {
        const gsa_pair_dev& in = pairs[p];
        if (in.adjrows < 1 || in.adjcols < 1 || !in.seqY || !in.seqX || !in.score) return GSA_ERROR_INVALID_VALUE;
        const long long ld = lds ? lds[p] : in.adjcols;
        if (ld < in.adjcols) return GSA_ERROR_INVALID_VALUE;
        gsa_sparse_geom geom;
        int s = gsa_sparse_geometry(in.adjrows, in.adjcols, gsa::kExpHB, &geom);
        if (s != GSA_SUCCESS) return s;
        const int Cp = geom.tileHdrMatCols * gsa::kExpHB;
        const long long tickets = gsa::krow_tickets(geom.tileHdrMatRows, ns, 4);
        const long long nrows = tickets * ns * 4;  // rows 64m written by pass 1, m = 1 .. nrows
        off[3 * p] = take((size_t)geom.hrowElems * 4);
        off[3 * p + 1] = take((size_t)geom.hcolElems * 4);
        off[3 * p + 2] = take((size_t)(nrows * gsa::rows64_pitch(Cp)) * 4);
        gsa::ExpandPair& e = ex[(size_t)p];
        std::memset(&e, 0, sizeof(e));
        e.seqY = in.seqY;
        e.seqX = in.seqX;
        e.R = in.adjrows - 1;
        e.C = in.adjcols - 1;
        e.score = in.score;
        e.ld = ld;
        e.rpitch = gsa::rows64_pitch(Cp);
        e.tcols = geom.tileHdrMatCols;
        // (an empty sequence still has its header row or column: at least one task per dimension)
        e.colTiles = std::max(1, (e.C + gsa::kExpTW - 1) / gsa::kExpTW);
        // a last tile column wider than one pass-1 tile is split at its boundary: the pair's last
        // tiles, which wait for the end of pass 1 in a fused fill, are then at most kExpHB wide
        e.lastSplit = e.C - (e.colTiles - 1) * gsa::kExpTW > gsa::kExpHB ? 1 : 0;
        e.colTiles += e.lastSplit;
        e.rowChunks = std::max(1, (e.R + xWaves * gsa::kExpRows * xmt - 1) / (xWaves * gsa::kExpRows * xmt));
        e.taskBase = (int)tasks;
        tasks += (long long)e.colTiles * e.rowChunks;
        e.p1Strip0 = (int)strips;  // (enqueue_batch's ticketBase x ns: pair-major)
        e.p1Strips = (int)(tickets * ns);
        strips += tickets * ns;
        if (tasks > (1ll << 30) || strips > (1ll << 30)) return GSA_ERROR_INVALID_VALUE;
    }
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    if (reserve(exbuf, bytes, 256) != hipSuccess)
    {
        (void)hipGetLastError();  // the caller falls back to the one-pass lane fill
        return kNoScratch;
    }
    char* base = exbuf.as<char>();
    std::vector<int*> rows((size_t)npairs);
    for (int p = 0; p < npairs; ++p)
    {
        p1[(size_t)p] = pairs[p];
        p1[(size_t)p].score = nullptr;
        p1[(size_t)p].tileHrowMat = (int32_t*)(base + off[3 * p]);
        p1[(size_t)p].tileHcolMat = (int32_t*)(base + off[3 * p + 1]);
        rows[(size_t)p] = (int*)(base + off[3 * p + 2]);
        ex[(size_t)p].rows64 = rows[(size_t)p];
        ex[(size_t)p].hcol = p1[(size_t)p].tileHcolMat;
    }
    // the expansion's descriptors and (batches) its round-robin schedule, staged in a pinned slot and
    // copied in stream order
    // Task order of a batch's expansion.  Round-robin over the pairs (one task of every pair in turn)
    // keeps the tasks in flight spread over all matrices, and its pass 2 runs at one of two speeds on
    // a given output buffer: the same order on another allocation of the same size, or the same
    // buffer with every pair's tasks rotated by k/npairs of its range (order 2), takes the other
    // (64 x 20k: 18.5-20.2 vs 21.2-25.4 ms; which one is fast flips between the two orders;
    // profiles/r05_outbuf_probe.txt).  So the first two launches on an output buffer run orders 1
    // and 2 and time their pass 2 (HIP events; the second launch waits for the first's), and later
    // launches on that buffer take the faster.  GSA_EXPAND_RR fixes the order: 0 pair-major, 1, 2,
    // 3 shuffled, 4-6 probe variants.
    const int rrEnv = opt.rr >= 0 ? opt.rr : env_int(ctx, "GSA_EXPAND_RR", -1);
    int rr = rrEnv >= 0 ? rrEnv : 1;
    const bool tune = rrEnv < 0 && npairs > 1 && !fused;
    bool tuneRecord = false;
    if (tune)
    {
        if (xt.key != (const void*)pairs[0].score || xt.pairs != npairs || xt.tasks != tasks)
        {
            xt.key = (const void*)pairs[0].score;
            xt.pairs = npairs;
            xt.tasks = tasks;
            xt.ms[0] = xt.ms[1] = -1.f;
            xt.pending = false;
            xt.cold = true;
        }
        // (the tuning is best effort: an event that cannot be created or read ends it on order 1)
        bool evOk = true;
        for (int k = 0; k < 2; ++k)
            if (!xt.ev[k] && hipEventCreate(&xt.ev[k]) != hipSuccess)
            {
                xt.ev[k] = nullptr;
                evOk = false;
            }
        // the previous candidate's time, if its launch has ended: the host never waits for it (a
        // launch still running keeps the measurement pending and this one runs untimed)
        bool busy = false;
        if (xt.pending && evOk)
        {
            const hipError_t q = hipEventQuery(xt.ev[1]);
            float ms = -1.f;
            if (q == hipErrorNotReady)
            {
                (void)hipGetLastError();
                busy = true;
            }
            else if (q != hipSuccess || hipEventElapsedTime(&ms, xt.ev[0], xt.ev[1]) != hipSuccess || !(ms >= 0.f))
            {
                (void)hipGetLastError();
                evOk = false;
            }
            else
                xt.ms[xt.last] = ms;
            if (!busy) xt.pending = false;
        }
        if (!evOk)
        {
            xt.ms[0] = xt.ms[1] = 0.f;  // both "measured": order 1 from now on
            xt.pending = false;
        }
        const int next = xt.ms[0] < 0 ? 0 : xt.ms[1] < 0 ? 1 : (xt.ms[1] < xt.ms[0] ? 1 : 0);
        tuneRecord = !busy && !xt.cold && xt.ms[next] < 0;
        xt.cold = false;
        if (tuneRecord) xt.last = next;
        rr = next + 1;
    }
    // The schedule: runs of xRun tasks of one tile column of one pair, consecutive row chunks (a
    // workgroup claims a run; its tile waves rebuild the column profile only when the tile column
    // changes: the rebuild and its two barriers stop the workgroup's store stream, ~10 % of the
    // expansion at 100k one task at a time, profiles/r06_expand_probes.txt), padded with (-1, 0)
    // entries to whole runs.  Runs in order: a single pair by when their pass-1 rows arrive (the
    // fused fill; it helps two launches too), a batch round-robin over the pairs (rr 1; rr 2
    // rotated, 0 pair-major, 3 shuffled).
    // runs of 4 (8 and 16 measured equal at 100k, r06), shorter when the runs would not cover the
    // CUs twice: a 10k pair's 483 tasks were 121 runs of 4, one per workgroup, four tasks in a row
    // on half the CUs, and its last run alone set the fill's tail (48 us after the last strip)
    long long allTasks = 0;
    for (int p = 0; p < npairs; ++p) allTasks += (long long)ex[(size_t)p].rowChunks * ex[(size_t)p].colTiles;
    const long long cus = std::max(1, ctx->cu_count);
    const int xRun = allTasks >= 8 * cus ? 4 : allTasks >= 4 * cus ? 2 : 1;
    std::vector<int> xs;
    {
        struct Run { int p, g, jT; };
        auto runs_of = [&](int p) { return ((ex[(size_t)p].rowChunks + xRun - 1) / xRun) * ex[(size_t)p].colTiles; };
        auto run_at = [&](int p, long long r) { const int ct = ex[(size_t)p].colTiles; return Run {p, (int)(r / ct), (int)(r % ct)}; };
        std::vector<Run> order;
        if (npairs == 1)
        {
            // Task (rc, jT) can start once strip s1 = the last of its rows' strips has passed column
            // cb + cols + 64; strip s starts ~s lag steps after strip 0 and sweeps a column per
            // step, so it is ready at about s1 lag + cb + cols.  Row-chunk-major order made the first
            // workgroups wait for whole rows: at 100k they claimed row chunk 0's tiles to the far end
            // of the matrix, ready only ~4 ms later (profiles/r06_fused100k.txt).  lag = columns per
            // 256-row strip (192: the 100k pair's strip-to-strip spacing).
            const gsa::ExpandPair& d = ex[0];
            constexpr long long lag = 192;
            const int cm = xWaves * xmt;
            std::vector<std::pair<long long, long long>> key;
            for (long long r = 0; r < runs_of(0); ++r)
            {
                const Run u = run_at(0, r);
                const long long s1 = std::min<long long>((cm * (u.g * xRun + 1) - 1) / 4, d.p1Strips - 1);
                key.push_back({s1 * lag + gsa::ex_cb(d, u.jT) + gsa::ex_cols(d, u.jT), r});
            }
            std::stable_sort(key.begin(), key.end());
            for (const auto& k : key) order.push_back(run_at(0, k.second));
        }
        else if (rr == 0)
        {
            for (int p = 0; p < npairs; ++p)
                for (long long r = 0; r < runs_of(p); ++r) order.push_back(run_at(p, r));
        }
        else
        {
            std::vector<int> ord((size_t)npairs);
            for (int p = 0; p < npairs; ++p) ord[(size_t)p] = p;
            std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return runs_of(x) > runs_of(y); });
            // rr 2: pair k of the order starts k / npairs of the way into its runs
            std::vector<long long> rot((size_t)npairs, 0);
            if (rr == 2)
                for (int k = 0; k < npairs; ++k)
                    rot[(size_t)ord[(size_t)k]] = runs_of(ord[(size_t)k]) * k / npairs;
            for (long long j = 0; j < runs_of(ord[0]); ++j)
                for (int k = 0; k < npairs; ++k)
                {
                    const int p = ord[(size_t)k];
                    if (runs_of(p) <= j) break;
                    order.push_back(run_at(p, (j + rot[(size_t)p]) % runs_of(p)));
                }
            if (rr == 3)
            {
                // the whole schedule shuffled (fixed seed)
                uint64_t z = 0x9e3779b97f4a7c15ull;
                for (size_t i = order.size(); i > 1; --i)
                {
                    z += 0x9e3779b97f4a7c15ull;
                    uint64_t q = z;
                    q = (q ^ (q >> 30)) * 0xbf58476d1ce4e5b9ull;
                    q = (q ^ (q >> 27)) * 0x94d049bb133111ebull;
                    q ^= q >> 31;
                    std::swap(order[i - 1], order[(size_t)(q % i)]);
                }
            }
        }
        xs.reserve(2 * order.size() * (size_t)xRun);
        for (const Run& u : order)
        {
            const gsa::ExpandPair& d = ex[(size_t)u.p];
            for (int i = 0; i < xRun; ++i)
            {
                const int rc = u.g * xRun + i;
                xs.push_back(rc < d.rowChunks ? u.p : -1);
                xs.push_back(rc < d.rowChunks ? rc * d.colTiles + u.jT : 0);
            }
        }
    }
    const long long nEntries = (long long)(xs.size() / 2);
    const size_t descBytes = ((size_t)npairs * sizeof(gsa::ExpandPair) + 15) & ~(size_t)15;
    const size_t exBytes = descBytes + xs.size() * sizeof(int);
    int s = reserve_hard(ctx, exdesc, exBytes, 4096);
    if (s != GSA_SUCCESS) return s;
    void* host = nullptr;
    if ((s = ctx->expin.acquire(exBytes, &host, &e)) != GSA_SUCCESS) return fail(ctx, e, s);
    std::memcpy(host, ex.data(), (size_t)npairs * sizeof(gsa::ExpandPair));
    if (!xs.empty()) std::memcpy((char*)host + descBytes, xs.data(), xs.size() * sizeof(int));
    e = hipMemcpyAsync(exdesc.p, host, exBytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = ctx->expin.commit(st);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    gsa::ExpandArgs xa {};
    xa.subst = subst;
    xa.substsz = substsz;
    xa.g = gapo;
    xa.pairs = exdesc.as<const gsa::ExpandPair>();
    xa.nPairs = npairs;
    xa.nTasks = (int)nEntries;
    xa.run = xRun;
    xa.sched = (const int*)(exdesc.as<char>() + descBytes);
    xa.spin = ctx->spin_ticks;
    xa.err = ctx->ctl + 1;
    // (a group of a split batch has a claim counter of its own: the two groups' expansions overlap)
    xa.counter = ctx->ctl + 8 + opt.slot;
    // the fused single pair: every workgroup takes pass-1 tickets first.  A large pair's expansion
    // fills HBM, and its strips hand row 64m to a storer wave (their own write-through stores stalled
    // them); a small one's keeps HBM idle enough for the strips to store it directly, without the
    // staging's ~5 % per step (nw_krow.hip nw_full_fused_kernel): 10k direct, 100k staged
    const int stagedKnob = env_int(ctx, "GSA_FUSED_STAGED", -1);  // (tests: both instances at every size)
    // (the staging's 32 KiB beside pass 1's profile: a table of more than 26 letters leaves no room for
    // it in LDS, and the strips store directly at every size)
    const bool staged = (stagedKnob >= 0 ? stagedKnob != 0
                                         : (long long)(pairs[0].adjrows - 1) * (long long)(pairs[0].adjcols - 1) > (1ll << 30)) &&
                        gsa::full_fused_lds_bytes(ns, substsz, false, true) <= (size_t)ctx->lds_max;
    const FusedLaunch fl {&xa, ns, gsa::kExpStreamWaves, 1 << 30, staged};
    const int xGrid = (int)std::max<long long>(1, std::min<long long>(ctx->cu_count, (nEntries + xRun - 1) / xRun));
    // gsa_set_full_timing: events before pass 1, between the passes and after pass 2, and the
    // expansion's clock stamps (one per workgroup)
    const bool timed = ctx->timing && !opt.split;
    if (!opt.split) ctx->timing_state = 0;
    if (timed && !fused)
    {
        if ((s = reserve_hard(ctx, ctx->buf[kBufClk], (size_t)xGrid * 8, 1024 * 8)) != GSA_SUCCESS) return s;
        xa.clk = ctx->buf[kBufClk].as<unsigned long long>();
        ctx->clk_n = (size_t)xGrid;
    }
    if (timed && (e = hipEventRecord(ctx->pev[0], st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    if (opt.startEv && (e = hipEventRecord(opt.startEv, st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    if (opt.beforeP1 && (e = hipStreamWaitEvent(st, opt.beforeP1, 0)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    s = enqueue_batch(ctx, gsa::kModeSparse, npairs, p1.data(), subst, substsz, gapo, gsa::kExpHB, st, nullptr, 0,
                      nullptr, rows.data(), fused ? &fl : nullptr);
    if (s != GSA_SUCCESS) return s;
    if (fused)
    {
        ctx->ll.kind = GSA_LAUNCH_FULL_FUSED;
        ctx->ll.staged = staged ? 1 : 0;
        if (timed && (e = hipEventRecord(ctx->pev[2], st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
        ctx->timing_state = timed ? 2 : 0;
        return s;
    }
    if (timed && (e = hipEventRecord(ctx->pev[1], st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    if (opt.afterP1 && (e = hipEventRecord(opt.afterP1, st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    if (opt.timeP1 && (e = hipEventRecord(opt.timeP1, st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    if ((e = hipMemsetAsync(xa.counter, 0, 4, st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    if (tuneRecord && (e = hipEventRecord(xt.ev[0], st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    if ((e = gsa::launch_expand_stream(xa, st, xGrid)) != hipSuccess) return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    note_launch(ctx);
    ctx->ll.kind = GSA_LAUNCH_FULL_TWO_LAUNCH;  // (pass 1's record, enqueue_batch: the whole call's)
    if (tuneRecord)
    {
        if ((e = hipEventRecord(xt.ev[1], st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
        xt.pending = true;
    }
    if (timed)
    {
        if ((e = hipEventRecord(ctx->pev[2], st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
        ctx->timing_state = 1;
    }
    return GSA_SUCCESS;
}

// full fills: the two-pass fill (same box: 10k 100 -> 141 GCUPS, 64 x 20k batch 1084 -> 1093-1102
// GCUPS, profiles/r04_twopass.txt); GSA_FULL_KERNEL=lane: the one-pass lane fill (nw_lane.hip)
bool full_twopass(const gsa_ctx* ctx)
{
    const char* e = knob(ctx, "GSA_FULL_KERNEL");
    return !(e && std::strcmp(e, "lane") == 0);
}

// A batch whose pass-1 tickets are k full rounds and a short last one, split in two groups: group A
// (k rounds of tickets) on the caller's stream, group B (the rest) on a high-priority stream behind
// A's pass 1.  B's pass 1 then runs on the CUs A's pass 1 leaves, while A's expansion takes the
// others, instead of the last round's idle CUs waiting for every pair's pass 1.  Whether that pays
// depends on the box: 64 x 20k pairs, 0.434 -> 0.49-0.52 of HBM peak on four boxes, 0.508 -> 0.475
// on another (profiles/r05_split_ab.txt), so enqueue_full times both on the batch's first launches.
struct SplitPlan
{
    std::vector<gsa_pair_dev> pa, pb;
    std::vector<int32_t> la, lb;
};
bool split_plan(gsa_ctx* ctx, int npairs, const gsa_pair_dev* pairs, const int32_t* lds, SplitPlan& sp)
{
    if (npairs < 2 || env_int(ctx, "GSA_FULL_FUSED", 1) >= 2) return false;
    long long tileRows = 0;
    for (int p = 0; p < npairs; ++p)
    {
        if (pairs[p].adjrows < 2 || pairs[p].adjcols < 2) return false;
        tileRows += std::max<long long>(1, ((long long)pairs[p].adjrows - 1 + gsa::kSparseTileBy - 1) / gsa::kSparseTileBy);
    }
    if (tileRows <= (long long)std::max(1, ctx->cu_count)) return false;  // 4-strip single round
    const int ns = env_int(ctx, "GSA_KROW_NS", 8) == 8 ? 8 : 4;
    std::vector<long long> t((size_t)npairs);
    long long T = 0;
    for (int p = 0; p < npairs; ++p)
    {
        gsa_sparse_geom geom;
        if (gsa_sparse_geometry(pairs[p].adjrows, pairs[p].adjcols, gsa::kExpHB, &geom) != GSA_SUCCESS) return false;
        t[(size_t)p] = gsa::krow_tickets(geom.tileHdrMatRows, ns, 4);
        T += t[(size_t)p];
    }
    const long long S = std::max(1, ctx->cu_count);  // (8, 4) XR workgroups: one per CU
    const long long k = T / S, tail = T - k * S;
    if (k < 1 || tail < 16 || tail > S - 16) return false;
    // group A: pairs by tickets, largest first, while they fit k rounds; B: the rest
    std::vector<int> ord((size_t)npairs);
    for (int p = 0; p < npairs; ++p) ord[(size_t)p] = p;
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return t[(size_t)x] > t[(size_t)y]; });
    long long ta = 0;
    for (int p : ord)
    {
        const bool toA = ta + t[(size_t)p] <= k * S;
        if (toA) ta += t[(size_t)p];
        (toA ? sp.pa : sp.pb).push_back(pairs[p]);
        if (lds) (toA ? sp.la : sp.lb).push_back(lds[p]);
    }
    return !sp.pa.empty() && !sp.pb.empty();
}

// The two groups of a split plan; rr: both groups' expansion order (-1: each tuned on its own
// scratch slot); startEv: recorded on st before group A's pass 1.  Returns kNoScratch when nothing
// was enqueued (no room for group A's scratch).
int enqueue_full_split(gsa_ctx* ctx, const SplitPlan& sp, bool hasLds, const int32_t* subst, int32_t substsz,
                       int32_t gapo, hipStream_t st, int rr, hipEvent_t startEv)
{
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    if (!ctx->splitstream)
    {
        int lo = 0, hi = 0;
        if ((e = hipDeviceGetStreamPriorityRange(&lo, &hi)) != hipSuccess ||
            (e = hipStreamCreateWithPriority(&ctx->splitstream, hipStreamNonBlocking, hi)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    }
    for (int q = 0; q < 2; ++q)
        if (!ctx->split_ev[q] && (e = hipEventCreateWithFlags(&ctx->split_ev[q], hipEventDisableTiming)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    const bool timed = ctx->timing;
    if (timed && (e = hipEventRecord(ctx->pev[0], st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    // B's stream waits for everything before this call on the caller's stream too
    if ((e = hipEventRecord(ctx->split_ev[1], st)) != hipSuccess ||
        (e = hipStreamWaitEvent(ctx->splitstream, ctx->split_ev[1], 0)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    TwoPassOpts oa, ob;
    oa.slot = 0;
    oa.afterP1 = ctx->split_ev[0];
    oa.timeP1 = timed ? ctx->pev[1] : nullptr;  // pass1_ms: group A's pass 1
    oa.startEv = startEv;
    oa.split = true;
    oa.rr = rr;
    ob.slot = 1;
    ob.beforeP1 = ctx->split_ev[0];
    ob.split = true;
    ob.rr = rr;
    int r = enqueue_full_twopass(ctx, (int)sp.pa.size(), sp.pa.data(), hasLds ? sp.la.data() : nullptr, subst, substsz,
                                 gapo, st, oa);
    if (r != GSA_SUCCESS) return r;  // (kNoScratch: nothing enqueued yet; the caller's fallback)
    const gsa_launch_info groupA = ctx->ll;
    const unsigned epochA = ctx->ll_epoch0;
    r = enqueue_full_twopass(ctx, (int)sp.pb.size(), sp.pb.data(), hasLds ? sp.lb.data() : nullptr, subst, substsz,
                             gapo, ctx->splitstream, ob);
    if (r == kNoScratch)  // no room for a second scratch: group B on the one-pass lane fill
    {
        if ((e = hipStreamWaitEvent(ctx->splitstream, ctx->split_ev[0], 0)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
        r = enqueue_batch(ctx, gsa::kModeFull, (int)sp.pb.size(), sp.pb.data(), subst, substsz, gapo, 0,
                          ctx->splitstream, nullptr, 0, hasLds ? sp.lb.data() : nullptr);
    }
    if (r != GSA_SUCCESS) return r;
    // the caller's stream waits for group B
    if ((e = hipEventRecord(ctx->split_ev[1], ctx->splitstream)) != hipSuccess ||
        (e = hipStreamWaitEvent(st, ctx->split_ev[1], 0)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    // gsa_last_launch: both groups' pairs and tickets, group A's geometry, the caller's stream (which
    // waits for group B); the int8 word holds either group's epoch (both see the same table)
    ctx->ll.npairs += groupA.npairs;
    ctx->ll.tickets += groupA.tickets;
    ctx->ll.kind = groupA.kind;
    ctx->ll.ns = groupA.ns;
    ctx->ll_stream = st;
    ctx->ll_epoch0 = epochA;
    if (timed)
    {
        if ((e = hipEventRecord(ctx->pev[2], st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
        ctx->timing_state = 3;
        ctx->timing_groups = 2;
        ctx->clk_n = 0;
    }
    return GSA_SUCCESS;
}

uint64_t batch_key(int npairs, const gsa_pair_dev* pairs, const int32_t* lds)
{
    uint64_t h = 0x9e3779b97f4a7c15ull ^ (uint64_t)npairs;
    auto mix = [&](uint64_t v) {
        h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
        h *= 0xbf58476d1ce4e5b9ull;
        h ^= h >> 31;
    };
    for (int p = 0; p < npairs; ++p)
    {
        mix((uint64_t)(uintptr_t)pairs[p].score);
        mix(((uint64_t)(uint32_t)pairs[p].adjrows << 32) | (uint32_t)pairs[p].adjcols);
        mix(lds ? (uint64_t)(uint32_t)lds[p] : 0);
    }
    return h;
}

// Every full fill: the two-pass fill, or the lane fill (GSA_FULL_KERNEL=lane, or no room for the
// two-pass scratch); lds: row pitches (null: unpadded).
// A batch that splits (split_plan) runs, unless GSA_FULL_SPLIT or GSA_EXPAND_RR fix it, four
// candidates on its first four launches: one group with expansion order 1 and 2, two groups with
// order 1 and 2, each timed from just before pass 1 to the end on the caller's stream (HIP events;
// a launch waits on the host for the previous one's end event), and later launches of the same
// batch (pairs, shapes, output pointers) take the fastest.  Best effort like the order tuning: an
// event that cannot be created or read ends it on candidate 0.
int enqueue_full(gsa_ctx* ctx, int npairs, const gsa_pair_dev* pairs, const int32_t* lds, const int32_t* subst,
                 int32_t substsz, int32_t gapo, hipStream_t st)
{
    if (full_twopass(ctx))
    {
        const int spEnv = env_int(ctx, "GSA_FULL_SPLIT", -1), rrEnv = env_int(ctx, "GSA_EXPAND_RR", -1);
        SplitPlan sp;
        const bool can = spEnv != 0 && !(spEnv < 0 && rrEnv >= 0) && split_plan(ctx, npairs, pairs, lds, sp);
        if (can && spEnv > 0)
        {
            const int r = enqueue_full_split(ctx, sp, lds != nullptr, subst, substsz, gapo, st, -1, nullptr);
            if (r != kNoScratch) return r;
        }
        else if (can)
        {
            gsa_ctx::FTune& ft = ctx->ft;
            const uint64_t key = batch_key(npairs, pairs, lds);
            if (ft.key != key)
            {
                ft.key = key;
                ft.last = -1;
                for (float& m : ft.ms) m = -1.f;
                ft.pending = false;
                ft.cold = true;
            }
            bool evOk = true;
            for (int k = 0; k < 2; ++k)
                if (!ft.ev[k] && hipEventCreate(&ft.ev[k]) != hipSuccess)
                {
                    (void)hipGetLastError();
                    ft.ev[k] = nullptr;
                    evOk = false;
                }
            // the previous candidate's time if its launch has ended (never a host wait: a launch
            // still running keeps it pending, and this one runs untimed)
            bool busy = false;
            if (ft.pending && evOk)
            {
                const hipError_t q = hipEventQuery(ft.ev[1]);
                float ms = -1.f;
                if (q == hipErrorNotReady)
                {
                    (void)hipGetLastError();
                    busy = true;
                }
                else if (q != hipSuccess || hipEventElapsedTime(&ms, ft.ev[0], ft.ev[1]) != hipSuccess || !(ms >= 0.f))
                {
                    (void)hipGetLastError();
                    evOk = false;
                }
                else
                    ft.ms[ft.last] = ms;
                if (!busy) ft.pending = false;
            }
            if (!evOk)
            {
                for (float& m : ft.ms) m = 0.f;  // all "measured": candidate 0 from now on
                ft.pending = false;
            }
            int next = 0;
            while (next < 4 && ft.ms[next] >= 0.f) ++next;
            if (busy || ft.cold)
                next = 0;  // (untimed: the first launch on fresh buffers, or a measurement pending)
            else if (next == 4)
            {
                next = 0;
                for (int k = 1; k < 4; ++k)
                    if (ft.ms[k] < ft.ms[next]) next = k;
                ft.last = -1;
            }
            const bool rec = !busy && !ft.cold && ft.ms[next] < 0.f;
            ft.cold = false;
            const int rr = (next & 1) + 1;
            int r;
            if (next >= 2)
                r = enqueue_full_split(ctx, sp, lds != nullptr, subst, substsz, gapo, st, rr, rec ? ft.ev[0] : nullptr);
            else
            {
                TwoPassOpts o;
                o.rr = rr;
                o.startEv = rec ? ft.ev[0] : nullptr;
                r = enqueue_full_twopass(ctx, npairs, pairs, lds, subst, substsz, gapo, st, o);
            }
            if (r == GSA_SUCCESS && rec)
            {
                hipError_t e = hipEventRecord(ft.ev[1], st);
                if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
                ft.last = next;
                ft.pending = true;
            }
            if (r != kNoScratch) return r;
        }
        const int s = enqueue_full_twopass(ctx, npairs, pairs, lds, subst, substsz, gapo, st);
        if (s != kNoScratch) return s;
    }
    return enqueue_batch(ctx, gsa::kModeFull, npairs, pairs, subst, substsz, gapo, 0, st, nullptr, 0, lds);
}

}  // namespace

extern "C" {

const char* gsa_version(void) { return "gpuseqalign_amd 0.3 (gfx950 wavefront: K-rows sparse, two-pass full)"; }

int32_t gsa_sparse_tile_by(void) { return gsa::kSparseTileBy; }

int gsa_debug_stamps(gsa_ctx* ctx, uint64_t* out, int64_t cap, int64_t* n)
{
    if (!ctx || !n) return GSA_ERROR_INVALID_VALUE;
    *n = (int64_t)ctx->stamps_n;
    if (ctx->stamps_n == 0 || !out) return GSA_SUCCESS;
    if (cap < (int64_t)ctx->stamps_n) return GSA_ERROR_INVALID_VALUE;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stamps_stream);  // the launch's stream only
    if (e == hipSuccess) e = hipMemcpy(out, ctx->buf[kBufStamps].p, ctx->stamps_n * sizeof(uint64_t), hipMemcpyDeviceToHost);
    return e == hipSuccess ? GSA_SUCCESS : fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
}

int gsa_set_full_timing(gsa_ctx* ctx, int32_t on)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    if (on && !ctx->pev[0])
    {
        hipError_t e = hipSetDevice(ctx->device);
        for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipEventCreate(&ctx->pev[k]);
        if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    }
    ctx->timing = on != 0;
    ctx->timing_state = 0;
    return GSA_SUCCESS;
}

int gsa_last_full_timing(gsa_ctx* ctx, gsa_full_timing* out)
{
    if (!ctx || !out) return GSA_ERROR_INVALID_VALUE;
    std::memset(out, 0, sizeof(*out));
    out->pass1_ms = out->pass2_ms = -1.f;
    out->clock_ghz_median = out->clock_ghz_mean = -1.f;
    if (ctx->timing_state == 0) return GSA_ERROR_INVALID_VALUE;  // no timed full fill since timing was set
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipEventSynchronize(ctx->pev[2]);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    out->fused = ctx->timing_state == 2;
    out->groups = ctx->timing_state == 3 ? ctx->timing_groups : 0;
    if (out->fused) return hipEventElapsedTime(&out->pass2_ms, ctx->pev[0], ctx->pev[2]) == hipSuccess
                               ? GSA_SUCCESS : GSA_ERROR_CUDA_GENERAL;
    if (hipEventElapsedTime(&out->pass1_ms, ctx->pev[0], ctx->pev[1]) != hipSuccess ||
        hipEventElapsedTime(&out->pass2_ms, ctx->pev[1], ctx->pev[2]) != hipSuccess)
        return GSA_ERROR_CUDA_GENERAL;
    if (ctx->clk_n == 0) return GSA_SUCCESS;
    std::vector<unsigned long long> v(ctx->clk_n);
    if ((e = hipMemcpy(v.data(), ctx->buf[kBufClk].p, v.size() * 8, hipMemcpyDeviceToHost)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    std::vector<float> ghz;
    ghz.reserve(v.size());
    double cyc = 0, ticks = 0;
    for (unsigned long long w : v)
    {
        const double c = (double)(uint32_t)w, t = (double)(uint32_t)(w >> 32);
        if (t < 100) continue;  // under 1 us: too short to resolve
        ghz.push_back((float)(c / t * 0.1));
        cyc += c;
        ticks += t;
    }
    out->workgroups = (int64_t)ghz.size();
    if (ghz.empty()) return GSA_SUCCESS;
    std::nth_element(ghz.begin(), ghz.begin() + ghz.size() / 2, ghz.end());
    out->clock_ghz_median = ghz[ghz.size() / 2];
    out->clock_ghz_mean = (float)(cyc / ticks * 0.1);
    return GSA_SUCCESS;
}

int gsa_last_launch(gsa_ctx* ctx, gsa_launch_info* out)
{
    if (!ctx || !out) return GSA_ERROR_INVALID_VALUE;
    std::memset(out, 0, sizeof(*out));
    if (ctx->ll.kind == GSA_LAUNCH_NONE) return GSA_ERROR_INVALID_VALUE;  // nothing launched yet
    *out = ctx->ll;
    // the int8 instance's decline: its launch's epoch in ctl[2] (nw_krow.hip), read behind the launch
    if (ctx->ll.q8 != 0 && ctx->ll_epoch != 0)
    {
        unsigned word = 0;
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->ll_stream);  // the launch's stream only
        if (e == hipSuccess) e = hipMemcpy(&word, ctx->ctl + 2, sizeof(word), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        out->q8_declined = (word - ctx->ll_epoch0 <= ctx->ll_epoch - ctx->ll_epoch0) ? 1 : 0;
    }
    return GSA_SUCCESS;
}

int gsa_ctx_create(int device, gsa_ctx** out)
{
    if (!out) return GSA_ERROR_INVALID_VALUE;
    *out = nullptr;
    gsa_ctx* ctx = new (std::nothrow) gsa_ctx();
    if (!ctx) return GSA_ERROR_MEMORY_ALLOCATION;
    ctx->device = device;
    for (const char* k : kKnobNames)
        if (const char* v = std::getenv(k)) ctx->knobs[k] = v;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&ctx->cu_count, hipDeviceAttributeMultiprocessorCount, device);
    if (e == hipSuccess)
    {
        int lm = 0;
        if (hipDeviceGetAttribute(&lm, hipDeviceAttributeSharedMemPerBlockOptin, device) == hipSuccess && lm > 0)
            ctx->lds_max = lm;
        else if (hipDeviceGetAttribute(&lm, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && lm > 0)
            ctx->lds_max = lm;
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    // mlsppt's copy-back stream, created next so that it gets a hardware queue of its own
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->ptstream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&ctx->ctl, 256);
    if (e == hipSuccess) e = hipMemset(ctx->ctl, 0, 256);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev0);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev1);
    for (int k = 0; k < gsa_ctx::kStage && e == hipSuccess; ++k)
        e = hipEventCreateWithFlags(&ctx->stage.ev[k], hipEventDisableTiming);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&ctx->ptev[k], hipEventDisableTiming);
    for (int k = 0; k < gsa_ctx::kStage && e == hipSuccess; ++k)
        e = hipEventCreateWithFlags(&ctx->expin.ev[k], hipEventDisableTiming);
    if (e != hipSuccess)
    {
        int code = (int)e;
        gsa_ctx_destroy(ctx);
        (void)code;
        return GSA_ERROR_CUDA_GENERAL;
    }
    *out = ctx;
    return GSA_SUCCESS;
}

void gsa_ctx_destroy(gsa_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (Buf& b : ctx->buf) release(b);
    for (StageRing* r : {&ctx->stage, &ctx->expin})
        for (int k = 0; k < StageRing::kStage; ++k)
        {
            release(r->slot[k]);
            if (r->ev[k]) (void)hipEventDestroy(r->ev[k]);
        }
    for (hipEvent_t ev : ctx->pev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& t : ctx->xt)
        for (hipEvent_t ev : t.ev)
            if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : ctx->split_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : ctx->ft.ev)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->splitstream)
    {
        (void)hipStreamSynchronize(ctx->splitstream);
        (void)hipStreamDestroy(ctx->splitstream);
    }
    for (hipEvent_t ev : ctx->adbev)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : ctx->dbmev)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : ctx->ptev)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->ptstream) (void)hipStreamDestroy(ctx->ptstream);
    for (int k = 0; k < gsa_ctx::kCopyThreads; ++k)
    {
        if (ctx->xstream[k]) (void)hipStreamDestroy(ctx->xstream[k]);
        for (int j = 0; j < 2; ++j)
        {
            release(ctx->xstage[k][j]);
            if (ctx->xev[k][j]) (void)hipEventDestroy(ctx->xev[k][j]);
        }
    }
    if (ctx->ctl) (void)hipFree(ctx->ctl);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int gsa_last_hip_error(const gsa_ctx* ctx) { return ctx ? ctx->last_hip_error : 0; }


int gsa_device_cu_count(const gsa_ctx* ctx) { return ctx ? ctx->cu_count : 0; }

int gsa_sparse_geometry(int32_t adjrows, int32_t adjcols, int32_t tileBx, gsa_sparse_geom* geom)
{
    if (!geom || adjrows < 1 || adjcols < 1) return GSA_ERROR_INVALID_VALUE;
    if (tileBx < 64 || tileBx % 16 != 0) return GSA_ERROR_INVALID_VALUE;
    const int64_t tBy = gsa::kSparseTileBy;
    // padded dims as nwalign_gpu9_mlsp_diagdiagdiag.cu:416-431 (empty sequences -> one tile)
    int64_t trows = ((int64_t)adjrows - 1 + tBy - 1) / tBy;
    int64_t tcols = ((int64_t)adjcols - 1 + tileBx - 1) / tileBx;
    trows = std::max<int64_t>(trows, 1);
    tcols = std::max<int64_t>(tcols, 1);
    geom->tileBx = tileBx;
    geom->tileBy = (int32_t)tBy;
    geom->tileHdrMatRows = (int32_t)trows;
    geom->tileHdrMatCols = (int32_t)tcols;
    geom->tileHrowLen = tileBx + 1;
    geom->tileHcolLen = (int32_t)tBy + 1;
    geom->hrowElems = trows * tcols * (tileBx + 1);
    geom->hcolElems = trows * tcols * (tBy + 1);
    return GSA_SUCCESS;
}

int gsa_fill_full_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                      const int32_t* subst, int32_t substsz, int32_t gapo, int32_t* score, void* stream)
{
    if (!ctx || !score) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    gsa_pair_dev p {seqY, adjrows, seqX, adjcols, score, nullptr, nullptr};
    return enqueue_full(ctx, 1, &p, nullptr, subst, substsz, gapo, pick_stream(ctx, stream));
}

int32_t gsa_full_pitch(int32_t adjcols)
{
    if (adjcols < 1) return 0;
    const int64_t ld = 32 * (((int64_t)adjcols - 1 + 31) / 32) + 1;
    return ld > INT32_MAX ? 0 : (int32_t)ld;  // no pitch fits int32 past 2^31 - 32 columns
}

int32_t gsa_full_base_offset(void) { return 31; }

int gsa_fill_full_pitched_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                              const int32_t* subst, int32_t substsz, int32_t gapo, int32_t* score, int32_t ld,
                              void* stream)
{
    if (!ctx || !score) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    if (ld < adjcols) return GSA_ERROR_INVALID_VALUE;
    gsa_pair_dev p {seqY, adjrows, seqX, adjcols, score, nullptr, nullptr};
    return enqueue_full(ctx, 1, &p, &ld, subst, substsz, gapo, pick_stream(ctx, stream));
}

int gsa_fill_sparse_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                        const int32_t* subst, int32_t substsz, int32_t gapo, int32_t tileBx, int32_t* hrow,
                        int32_t* hcol, void* stream)
{
    if (!ctx || !hrow || !hcol) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    return enqueue_fill(ctx, gsa::kModeSparse, seqY, adjrows, seqX, adjcols, subst, substsz, gapo, nullptr, tileBx,
                        hrow, hcol, pick_stream(ctx, stream));
}

int gsa_fill_full_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst,
                            int32_t substsz, int32_t gapo, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return enqueue_full(ctx, npairs, pairs, nullptr, subst, substsz, gapo, pick_stream(ctx, stream));
}

int gsa_fill_full_batch_pitched_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* lds,
                                    const int32_t* subst, int32_t substsz, int32_t gapo, void* stream)
{
    if (!ctx || !lds) return GSA_ERROR_INVALID_VALUE;
    return enqueue_full(ctx, npairs, pairs, lds, subst, substsz, gapo, pick_stream(ctx, stream));
}

int gsa_fill_sparse_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst,
                              int32_t substsz, int32_t gapo, int32_t tileBx, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return enqueue_batch(ctx, gsa::kModeSparse, npairs, pairs, subst, substsz, gapo, tileBx,
                         pick_stream(ctx, stream));
}

int gsa_sync(gsa_ctx* ctx, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    const hipStream_t st = pick_stream(ctx, stream);
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    unsigned err = 0;
    if ((e = take_err(ctx, st, &err)) != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    // a hand-off spin of ANY launch since the last sync gave up (the word is sticky)
    if (err != 0) return GSA_ERROR_KERNEL_FAILURE;
    return GSA_SUCCESS;
}

int gsa_mem_stats_get(const gsa_ctx* ctx, gsa_mem_stats* out)
{
    if (!ctx || !out) return GSA_ERROR_INVALID_VALUE;
    *out = ctx->mem;
    return GSA_SUCCESS;
}

int gsa_mem_stats_reset(gsa_ctx* ctx)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    ctx->mem = gsa_mem_stats {};
    return GSA_SUCCESS;
}

int gsa_set_lap_callback(gsa_ctx* ctx, gsa_lap_fn fn, void* user)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    ctx->lap_fn = fn;
    ctx->lap_user = fn ? user : nullptr;
    return GSA_SUCCESS;
}

int gsa_set_knob(gsa_ctx* ctx, const char* name, const char* value)
{
    if (!ctx || !name || !knob_known(name)) return GSA_ERROR_INVALID_VALUE;
    if (value)
        ctx->knobs[name] = value;
    else
        ctx->knobs.erase(name);
    return GSA_SUCCESS;
}

int gsa_set_watchdog(gsa_ctx* ctx, int64_t microseconds)
{
    if (!ctx || microseconds < 0 || microseconds > 3600ll * 1000000ll) return GSA_ERROR_INVALID_VALUE;
    ctx->spin_ticks = (unsigned long long)microseconds * 100ull;  // s_memrealtime: 100 MHz
    return GSA_SUCCESS;
}

namespace {

// Device -> pageable host copy of a finished result (the caller's buffers of gsa_align_*).  A
// plain hipMemcpy into pageable memory runs at ~16 GB/s here (one staged stream); this splits
// the range over kCopyThreads threads, each streaming kCopyChunk pieces through two pinned
// buffers on its own stream, so the DMA and the host copies of different pieces overlap.
hipError_t copy_d2h(gsa_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    constexpr int T = gsa_ctx::kCopyThreads;
    constexpr size_t kC = gsa_ctx::kCopyChunk;
    hipError_t e = hipSuccess;
    // non-blocking streams: mlsppt copies finished tile rows while the fill still runs
    for (int k = 0; k < T && e == hipSuccess; ++k)
        if (!ctx->xstream[k]) e = hipStreamCreateWithFlags(&ctx->xstream[k], hipStreamNonBlocking);
    if (e != hipSuccess) return e;
    if (bytes < 2 * kC)
    {
        e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->xstream[0]);
        return e == hipSuccess ? hipStreamSynchronize(ctx->xstream[0]) : e;
    }
    for (int k = 0; k < T && e == hipSuccess; ++k)
    {
        for (int j = 0; j < 2 && e == hipSuccess; ++j)
        {
            e = reserve(ctx->xstage[k][j], kC, 0);
            if (e == hipSuccess && !ctx->xev[k][j]) e = hipEventCreateWithFlags(&ctx->xev[k][j], hipEventDisableTiming);
        }
    }
    if (e != hipSuccess) return e;
    // thread k: bytes [lo, hi), chunk aligned
    const size_t nChunks = (bytes + kC - 1) / kC, perT = (nChunks + T - 1) / T;
    hipError_t errs[T];
    auto work = [&](int k) {
        hipError_t r = hipSetDevice(ctx->device);
        const size_t lo = std::min(bytes, (size_t)k * perT * kC), hi = std::min(bytes, (size_t)(k + 1) * perT * kC);
        const size_t n = (hi - lo + kC - 1) / kC;
        auto issue = [&](size_t i) {
            const size_t off = lo + i * kC, len = std::min(kC, hi - off);
            hipError_t q = hipMemcpyAsync(ctx->xstage[k][i & 1].p, (const char*)src + off, len, hipMemcpyDeviceToHost,
                                          ctx->xstream[k]);
            return q == hipSuccess ? hipEventRecord(ctx->xev[k][i & 1], ctx->xstream[k]) : q;
        };
        if (r == hipSuccess && n > 0) r = issue(0);
        for (size_t i = 0; r == hipSuccess && i < n; ++i)
        {
            // chunk i+1 goes into the other buffer, whose host copy (chunk i-1) is done
            if (i + 1 < n && (r = issue(i + 1)) != hipSuccess) break;
            if ((r = hipEventSynchronize(ctx->xev[k][i & 1])) != hipSuccess) break;
            const size_t off = lo + i * kC;
            std::memcpy((char*)dst + off, ctx->xstage[k][i & 1].p, std::min(kC, hi - off));
        }
        if (r != hipSuccess) (void)hipStreamSynchronize(ctx->xstream[k]);
        errs[k] = r;
    };
    std::vector<std::thread> th;
    th.reserve(T - 1);
    for (int k = 1; k < T; ++k) th.emplace_back(work, k);
    work(0);
    for (auto& x : th) x.join();
    for (int k = 0; k < T; ++k)
        if (errs[k] != hipSuccess) return errs[k];
    return hipSuccess;
}

}  // namespace

int gsa_align_full(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                   const int32_t* subst, int32_t substsz, int32_t gapo, int32_t* score_out, int32_t* align_cost,
                   gsa_laps* laps)
{
    if (!ctx || !seqY || !seqX || !subst || !score_out) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    gsa_laps L {};
    auto t = Clock::now();
    const size_t cells = (size_t)adjrows * (size_t)adjcols;
    if ((s = ensure_dev(ctx, 0, (size_t)adjrows * 4)) || (s = ensure_dev(ctx, 1, (size_t)adjcols * 4)) ||
        (s = ensure_dev(ctx, 2, (size_t)substsz * substsz * 4)) || (s = ensure_dev(ctx, 3, cells * 4)))
        return s;
    L.alloc = ms_since(t);
    lap(ctx, "align.alloc");
    hipError_t e;
    if ((e = hipMemcpyAsync(ctx->buf[kBufIo0].p, seqY, (size_t)adjrows * 4, hipMemcpyHostToDevice, ctx->stream)) ||
        (e = hipMemcpyAsync(ctx->buf[kBufIo1].p, seqX, (size_t)adjcols * 4, hipMemcpyHostToDevice, ctx->stream)) ||
        (e = hipMemcpyAsync(ctx->buf[kBufIo2].p, subst, (size_t)substsz * substsz * 4, hipMemcpyHostToDevice, ctx->stream)) ||
        (e = hipStreamSynchronize(ctx->stream)))
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    L.cpy_dev = ms_since(t);
    lap(ctx, "align.cpy_dev");
    L.init_hdr = 0.f;  // headers are written by the fill launch itself
    lap(ctx, "align.init_hdr");
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    s = gsa_fill_full_dev(ctx, ctx->buf[kBufIo0].as<const int32_t>(), adjrows, ctx->buf[kBufIo1].as<const int32_t>(), adjcols,
                          ctx->buf[kBufIo2].as<const int32_t>(), substsz, gapo, ctx->buf[kBufIo3].as<int32_t>(), ctx->stream);
    if (s != GSA_SUCCESS) return s;
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    if ((s = gsa_sync(ctx, ctx->stream)) != GSA_SUCCESS) return s;
    L.calc = ms_since(t);
    lap(ctx, "align.calc");
    (void)hipEventElapsedTime(&L.calc_kernel_ms, ctx->ev0, ctx->ev1);
    if ((e = copy_d2h(ctx, score_out, ctx->buf[kBufIo3].p, cells * 4)))
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    L.cpy_host = ms_since(t);
    lap(ctx, "align.cpy_host");
    if (align_cost) *align_cost = score_out[cells - 1];
    if (laps) *laps = L;
    return GSA_SUCCESS;
}

int gsa_align_sparse(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                     const int32_t* subst, int32_t substsz, int32_t gapo, int32_t tileBx, int32_t* hrow_out,
                     int32_t* hcol_out, gsa_sparse_geom* geom_out, int32_t* align_cost, gsa_laps* laps)
{
    if (!ctx || !seqY || !seqX || !subst || !hrow_out || !hcol_out) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    gsa_sparse_geom geom;
    if ((s = gsa_sparse_geometry(adjrows, adjcols, tileBx, &geom)) != GSA_SUCCESS) return s;
    gsa_laps L {};
    auto t = Clock::now();
    if ((s = ensure_dev(ctx, 0, (size_t)adjrows * 4)) || (s = ensure_dev(ctx, 1, (size_t)adjcols * 4)) ||
        (s = ensure_dev(ctx, 2, (size_t)substsz * substsz * 4)) || (s = ensure_dev(ctx, 3, (size_t)geom.hrowElems * 4)) ||
        (s = ensure_dev(ctx, 4, (size_t)geom.hcolElems * 4)))
        return s;
    L.alloc = ms_since(t);
    lap(ctx, "align.alloc");
    hipError_t e;
    if ((e = hipMemcpyAsync(ctx->buf[kBufIo0].p, seqY, (size_t)adjrows * 4, hipMemcpyHostToDevice, ctx->stream)) ||
        (e = hipMemcpyAsync(ctx->buf[kBufIo1].p, seqX, (size_t)adjcols * 4, hipMemcpyHostToDevice, ctx->stream)) ||
        (e = hipMemcpyAsync(ctx->buf[kBufIo2].p, subst, (size_t)substsz * substsz * 4, hipMemcpyHostToDevice, ctx->stream)) ||
        (e = hipStreamSynchronize(ctx->stream)))
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    L.cpy_dev = ms_since(t);
    lap(ctx, "align.cpy_dev");
    lap(ctx, "align.init_hdr");  // headers are written by the fill launch itself
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    s = gsa_fill_sparse_dev(ctx, ctx->buf[kBufIo0].as<const int32_t>(), adjrows, ctx->buf[kBufIo1].as<const int32_t>(), adjcols,
                            ctx->buf[kBufIo2].as<const int32_t>(), substsz, gapo, tileBx, ctx->buf[kBufIo3].as<int32_t>(),
                            ctx->buf[kBufIo4].as<int32_t>(), ctx->stream);
    if (s != GSA_SUCCESS) return s;
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    if ((s = gsa_sync(ctx, ctx->stream)) != GSA_SUCCESS) return s;
    L.calc = ms_since(t);
    lap(ctx, "align.calc");
    (void)hipEventElapsedTime(&L.calc_kernel_ms, ctx->ev0, ctx->ev1);
    if ((e = copy_d2h(ctx, hrow_out, ctx->buf[kBufIo3].p, (size_t)geom.hrowElems * 4)) ||
        (e = copy_d2h(ctx, hcol_out, ctx->buf[kBufIo4].p, (size_t)geom.hcolElems * 4)))
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    L.cpy_host = ms_since(t);
    lap(ctx, "align.cpy_host");
    // align_cost from the last tile, as the reference does after its copy-back (:713-716);
    // the reference adds this to the align.calc lap.
    int32_t cost = gsa_sparse_align_cost(hrow_out, hcol_out, &geom, seqY, adjrows, seqX, adjcols, subst, substsz, gapo);
    L.calc += ms_since(t);
    lap(ctx, "align.calc");
    if (align_cost) *align_cost = cost;
    if (geom_out) *geom_out = geom;
    if (laps) *laps = L;
    return GSA_SUCCESS;
}

int gsa_check_sparse_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                         const int32_t* subst, int32_t substsz, int32_t gapo, const gsa_sparse_geom* geom,
                         const int32_t* hrow, const int32_t* hcol, gsa_check_result* out, void* stream)
{
    if (!ctx || !seqY || !seqX || !subst || !geom || !hrow || !hcol || !out) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    gsa_sparse_geom g;
    if ((s = gsa_sparse_geometry(adjrows, adjcols, geom->tileBx, &g)) != GSA_SUCCESS) return s;
    if (std::memcmp(&g, geom, sizeof(g)) != 0) return GSA_ERROR_INVALID_VALUE;  // not this pair's geometry
    gsa::CheckArgs a {};
    a.seqY = seqY;
    a.seqX = seqX;
    a.subst = subst;
    a.substsz = substsz;
    a.g = gapo;
    a.adjrows = adjrows;
    a.adjcols = adjcols;
    a.tBx = g.tileBx;
    a.tBy = g.tileBy;
    a.trows = g.tileHdrMatRows;
    a.tcols = g.tileHdrMatCols;
    a.hrowElems = g.hrowElems;
    a.hrow = hrow;
    a.hcol = hcol;
    return run_check(ctx, a, true, pick_stream(ctx, stream), out);
}

int gsa_check_full_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                       const int32_t* subst, int32_t substsz, int32_t gapo, const int32_t* score,
                       gsa_check_result* out, void* stream)
{
    if (!ctx || !seqY || !seqX || !subst || !score || !out) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    gsa::CheckArgs a {};
    a.seqY = seqY;
    a.seqX = seqX;
    a.subst = subst;
    a.substsz = substsz;
    a.g = gapo;
    a.adjrows = adjrows;
    a.adjcols = adjcols;
    a.score = score;
    a.ld = adjcols;
    return run_check(ctx, a, false, pick_stream(ctx, stream), out);
}

int gsa_check_full_pitched_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX,
                               int32_t adjcols, const int32_t* subst, int32_t substsz, int32_t gapo,
                               const int32_t* score, int32_t ld, gsa_check_result* out, void* stream)
{
    if (!ctx || !seqY || !seqX || !subst || !score || !out) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    if (ld < adjcols) return GSA_ERROR_INVALID_VALUE;
    gsa::CheckArgs a {};
    a.seqY = seqY;
    a.seqX = seqX;
    a.subst = subst;
    a.substsz = substsz;
    a.g = gapo;
    a.adjrows = adjrows;
    a.adjcols = adjcols;
    a.score = score;
    a.ld = ld;
    return run_check(ctx, a, false, pick_stream(ctx, stream), out);
}

// NwHash1_Plain (nwtrace1_plain.cpp:133-154) over a matrix that stays in HBM.  djb2-xor is one serial
// chain over every cell in row-major order, so the host folds it while the DMA brings the next rows:
// row chunks (~64 MB, unpadded) alternate between two pinned buffers on the context's copy stream.
int gsa_hash_full_dev(gsa_ctx* ctx, const int32_t* score, int32_t adjrows, int32_t adjcols, int32_t ld,
                      uint32_t* hash, void* stream)
{
    if (!ctx || !score || !hash || adjrows < 1 || adjcols < 1 || ld < adjcols) return GSA_ERROR_INVALID_VALUE;
    hipError_t e = hipSetDevice(ctx->device);
    const hipStream_t st = pick_stream(ctx, stream);
    // (the caller's work on `stream` first: the matrix may still be being filled)
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    const int64_t rowsPer = std::max<int64_t>(1, ((int64_t)16 << 20) / adjcols);
    const int64_t nChunks = (adjrows + rowsPer - 1) / rowsPer;
    const size_t bufBytes = (size_t)std::min<int64_t>(rowsPer, adjrows) * (size_t)adjcols * 4;
    void* buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    int rc = GSA_SUCCESS;
    for (int k = 0; k < 2 && e == hipSuccess; ++k)
    {
        e = hipHostMalloc(&buf[k], bufBytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
    }
    auto issue = [&](int64_t c) {
        const int64_t r0 = c * rowsPer, n = std::min<int64_t>(rowsPer, adjrows - r0);
        hipError_t q = hipMemcpy2DAsync(buf[c & 1], (size_t)adjcols * 4, score + r0 * (int64_t)ld, (size_t)ld * 4,
                                        (size_t)adjcols * 4, (size_t)n, hipMemcpyDeviceToHost, st);
        return q == hipSuccess ? hipEventRecord(ev[c & 1], st) : q;
    };
    uint32_t h = 5381;
    if (e == hipSuccess) e = issue(0);
    for (int64_t c = 0; e == hipSuccess && c < nChunks; ++c)
    {
        if (c + 1 < nChunks && (e = issue(c + 1)) != hipSuccess) break;
        if ((e = hipEventSynchronize(ev[c & 1])) != hipSuccess) break;
        const uint32_t* v = (const uint32_t*)buf[c & 1];
        const int64_t n = std::min<int64_t>(rowsPer, adjrows - c * rowsPer) * adjcols;
        for (int64_t k = 0; k < n; ++k) h = ((h << 5) + h) ^ v[k];
    }
    if (e != hipSuccess)
    {
        (void)hipStreamSynchronize(st);
        rc = fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    }
    for (int k = 0; k < 2; ++k)
    {
        if (buf[k]) (void)hipHostFree(buf[k]);
        if (ev[k]) (void)hipEventDestroy(ev[k]);
    }
    if (rc == GSA_SUCCESS) *hash = h;
    return rc;
}

// NwTrace1_Plain (nwtrace1_plain.cpp:6-131) over a matrix that stays in HBM.  The walk reads three
// stored neighbours per move; it runs on the host over blocks of the matrix copied on demand
// (kTB rows x kTC columns ending at the walk's position, so a walk up and to the left stays inside
// a block for up to kTB / kTC moves), and its moves are folded as the device Trace2's are.
int gsa_trace_full_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                       const int32_t* score, int32_t ld, char* edit, int64_t cap, int64_t* edit_len,
                       uint32_t* trace_hash, int32_t* align_cost, void* stream)
{
    if (!ctx || !seqY || !seqX || !score || !edit || !edit_len || !trace_hash || adjrows < 1 || adjcols < 1 ||
        ld < adjcols)
        return GSA_ERROR_INVALID_VALUE;
    constexpr int64_t kTB = 1024, kTC = 2048;
    hipError_t e = hipSetDevice(ctx->device);
    const hipStream_t st = pick_stream(ctx, stream);
    std::vector<int32_t> Y((size_t)adjrows), X((size_t)adjcols);
    if (e == hipSuccess) e = hipMemcpyAsync(Y.data(), seqY, (size_t)adjrows * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(X.data(), seqX, (size_t)adjcols * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    int32_t* blk = nullptr;
    if ((e = hipHostMalloc((void**)&blk, (size_t)(kTB * kTC) * 4, hipHostMallocDefault)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_ALLOCATION);
    int64_t bi0 = -1, bj0 = 0, bh = 0, bw = 0;  // the block held: rows [bi0, bi0 + bh), columns [bj0, bj0 + bw)
    // make rows i-1..i and columns j-1..j resident (a block ending at (i, j))
    auto fetch = [&](int64_t i, int64_t j) {
        const int64_t i0 = std::max<int64_t>(0, i - kTB + 1), j0 = std::max<int64_t>(0, j - kTC + 1);
        const int64_t h = std::min<int64_t>(kTB, adjrows - i0), w = std::min<int64_t>(kTC, adjcols - j0);
        hipError_t q = hipMemcpy2DAsync(blk, (size_t)w * 4, score + i0 * (int64_t)ld + j0, (size_t)ld * 4,
                                        (size_t)w * 4, (size_t)h, hipMemcpyDeviceToHost, st);
        if (q == hipSuccess) q = hipStreamSynchronize(st);
        bi0 = i0;
        bj0 = j0;
        bh = h;
        bw = w;
        return q;
    };
    auto held = [&](int64_t i, int64_t j) {
        const int64_t ilo = i > 0 ? i - 1 : 0, jlo = j > 0 ? j - 1 : 0;
        return bi0 >= 0 && ilo >= bi0 && i < bi0 + bh && jlo >= bj0 && j < bj0 + bw;
    };
    auto at = [&](int64_t i, int64_t j) { return blk[(i - bi0) * bw + (j - bj0)]; };
    std::vector<unsigned char> moves;
    moves.reserve((size_t)(adjrows + adjcols));
    int64_t i = adjrows - 1, j = adjcols - 1;
    int32_t cost = 0;
    for (bool first = true; e == hipSuccess; first = false)
    {
        if (!held(i, j) && (e = fetch(i, j)) != hipSuccess) break;
        if (first) cost = at(i, j);
        // the reference's order: diagonal, then up if strictly greater, then left if strictly greater
        int64_t best = INT64_MIN;
        int di = 0, dj = 0;
        unsigned char m = 0;
        if (i > 0 && j > 0)
        {
            best = at(i - 1, j - 1);
            di = dj = -1;
            m = X[(size_t)j] == Y[(size_t)i] ? '=' : 'X';
        }
        if (i > 0 && best < at(i - 1, j))
        {
            best = at(i - 1, j);
            di = -1;
            dj = 0;
            m = 'I';
        }
        if (j > 0 && best < at(i, j - 1))
        {
            best = at(i, j - 1);
            di = 0;
            dj = -1;
            m = 'D';
        }
        if (di == 0 && dj == 0) break;
        moves.push_back(m);
        i += di;
        j += dj;
    }
    (void)hipHostFree(blk);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    if (align_cost) *align_cost = cost;
    return gsa::fold_moves(moves.data(), (int64_t)moves.size(), edit, cap, edit_len, trace_hash);
}

int gsa_trace_sparse_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                         const int32_t* subst, int32_t substsz, int32_t gapo, const gsa_sparse_geom* geom,
                         const int32_t* hrow, const int32_t* hcol, char* edit, int64_t cap, int64_t* edit_len,
                         uint32_t* trace_hash, int32_t* align_cost, void* stream)
{
    if (!ctx || !seqY || !seqX || !subst || !geom || !hrow || !hcol || !edit || !edit_len || !trace_hash)
        return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    gsa_sparse_geom g;
    if ((s = gsa_sparse_geometry(adjrows, adjcols, geom->tileBx, &g)) != GSA_SUCCESS) return s;
    if (std::memcmp(&g, geom, sizeof(g)) != 0) return GSA_ERROR_INVALID_VALUE;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    hipStream_t st = pick_stream(ctx, stream);
    // start: NwTrace2_GetTileAndElemIJ(adjrows-1, adjcols-1) with its saturation (nwtrace2_sparse.cpp:8-38)
    const int64_t i0 = adjrows - 1, j0 = adjcols - 1;
    int64_t iT = i0 / g.tileBy, jT = j0 / g.tileBx, iE = i0 % g.tileBy, jE = j0 % g.tileBx;
    if (iT == g.tileHdrMatRows) { iT -= 1; iE += g.tileBy; }
    if (jT == g.tileHdrMatCols) { jT -= 1; jE += g.tileBx; }
    const size_t nmax = (size_t)i0 + (size_t)j0 + 1;
    if ((s = reserve_hard(ctx, ctx->buf[kBufTmoves], nmax)) != GSA_SUCCESS ||
        (s = reserve_hard(ctx, ctx->buf[kBufTres], 64)) != GSA_SUCCESS)
        return s;
    const bool dirs_lds = gsa::trace_lds_bytes(g.tileBy, g.tileBx, substsz, true) <= 160 * 1024;
    if (!dirs_lds &&
        (s = reserve_hard(ctx, ctx->buf[kBufTdirs], gsa::trace_dir_words(g.tileBy, g.tileBx) * 4)) != GSA_SUCCESS)
        return s;
    unsigned char* const tmoves = ctx->buf[kBufTmoves].as<unsigned char>();
    long long* const tres = ctx->buf[kBufTres].as<long long>();
    gsa::TraceArgs a {};
    a.seqY = seqY;
    a.seqX = seqX;
    a.subst = subst;
    a.substsz = substsz;
    a.g = gapo;
    a.adjrows = adjrows;
    a.adjcols = adjcols;
    a.tBx = g.tileBx;
    a.tBy = g.tileBy;
    a.tcols = g.tileHdrMatCols;
    a.hrow = hrow;
    a.hcol = hcol;
    a.iT0 = (int)iT;
    a.jT0 = (int)jT;
    a.iE0 = (int)iE;
    a.jE0 = (int)jE;
    a.edits = tmoves;
    a.cap = (long long)nmax;
    a.res = tres;
    a.dirs_scratch = dirs_lds ? nullptr : ctx->buf[kBufTdirs].as<unsigned>();
    // The walk enters tiles one after another, and recomputing one (a row scan over its rows) takes
    // ~160 us at 1024 x 256.  The tiles are independent given their headers, so the ones within
    // GSA_TRACE_BAND columns (default 1024) of the diagonal are recomputed first by many workgroups
    // at once; the walk copies their codes (or reads them in place when a tile is too wide for
    // LDS) and recomputes only the tiles it finds outside the band.
    a.tmap = nullptr;
    a.tcodes = nullptr;
    // The band is only a speed-up: its codes take at most 512 MB and half the free device memory
    // (GSA_TRACE_BAND_BUDGET, bytes, lowers the cap), and if its buffers cannot be had the walk
    // runs alone and recomputes every tile it enters.
    {
        const int band = env_int(ctx, "GSA_TRACE_BAND", 1024);
        const int trows = g.tileHdrMatRows, tcols = g.tileHdrMatCols;
        const size_t words = gsa::trace_dir_words(g.tileBy, g.tileBx);
        size_t budget = (size_t)512 << 20;
        {
            size_t freeB = 0, totalB = 0;
            if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) budget = std::min(budget, freeB / 2);
            const char* eb = knob(ctx, "GSA_TRACE_BAND_BUDGET");
            if (eb) budget = std::min(budget, (size_t)std::strtoull(eb, nullptr, 10));
        }
        const size_t maxSlots = budget / (words * 4);
        std::vector<int> list, map((size_t)trows * (size_t)tcols, -1);
        const double slope = (double)std::max<int64_t>(1, adjcols - 1) / (double)std::max<int64_t>(1, adjrows - 1);
        for (int r = 0; band > 0 && r < trows && list.size() / 2 < maxSlots; ++r)
        {
            const double c0 = (double)r * g.tileBy * slope - band, c1 = (double)(r + 1) * g.tileBy * slope + band;
            const int j0 = std::max(0, (int)(c0 / g.tileBx)), j1 = std::min(tcols - 1, (int)(c1 / g.tileBx));
            for (int c = j0; c <= j1 && list.size() / 2 < maxSlots; ++c)
            {
                if (r == iT && c == jT) continue;  // the start tile: recomputed by the walk (align cost)
                map[(size_t)r * tcols + c] = (int)(list.size() / 2);
                list.push_back(r);
                list.push_back(c);
            }
        }
        const int n = (int)(list.size() / 2);
        bool have = n > 0;
        const size_t ints = list.size() + map.size(), cbytes = (size_t)n * words * 4;
        have = have && reserve(ctx->buf[kBufTlist], ints * 4, 0) == hipSuccess;
        have = have && reserve(ctx->buf[kBufTband], cbytes, 0) == hipSuccess;
        if (!have) (void)hipGetLastError();  // a failed band allocation: the walk runs alone
        if (have)
        {
            int* const tlist = ctx->buf[kBufTlist].as<int>();
            // pageable sources: the copies are complete when the calls return
            if ((e = hipMemcpyAsync(tlist, list.data(), list.size() * 4, hipMemcpyHostToDevice, st)) != hipSuccess ||
                (e = hipMemcpyAsync(tlist + list.size(), map.data(), map.size() * 4, hipMemcpyHostToDevice, st)) != hipSuccess)
                return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
            a.tmap = tlist + list.size();
            a.tcodes = ctx->buf[kBufTband].as<unsigned>();
            if ((e = gsa::launch_trace_band(a, tlist, n, 4 * ctx->cu_count, st)) != hipSuccess)
                return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        }
        gsa_launch_info& li = new_launch_info(ctx, GSA_LAUNCH_TRACE_SPARSE, st, 0);
        li.npairs = 1;
        li.trace_band = band;
        li.band_tiles = have ? n : 0;
    }
    if ((e = gsa::launch_trace_sparse(a, st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    long long res[2] = {0, 0};
    if ((e = hipMemcpyAsync(res, tres, sizeof(res), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    if (res[0] < 0 || (size_t)res[0] > nmax) return GSA_ERROR_INVALID_RESULT;
    std::vector<unsigned char> moves((size_t)res[0]);
    if (res[0] > 0 && (e = hipMemcpy(moves.data(), tmoves, (size_t)res[0], hipMemcpyDeviceToHost)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    if (align_cost) *align_cost = (int32_t)res[1];
    return gsa::fold_moves(moves.data(), (int64_t)res[0], edit, cap, edit_len, trace_hash);
}

int gsa_align_sparse_pt(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                        const int32_t* subst, int32_t substsz, int32_t gapo, int32_t tileBx, int32_t* hrow_out,
                        int32_t* hcol_out, gsa_sparse_geom* geom_out, int32_t* align_cost, gsa_laps* laps)
{
    if (!ctx || !seqY || !seqX || !subst || !hrow_out || !hcol_out) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    gsa_sparse_geom geom;
    if ((s = gsa_sparse_geometry(adjrows, adjcols, tileBx, &geom)) != GSA_SUCCESS) return s;
    gsa_laps L {};
    auto t = Clock::now();
    const size_t trows = (size_t)geom.tileHdrMatRows;
    if ((s = ensure_dev(ctx, 0, (size_t)adjrows * 4)) || (s = ensure_dev(ctx, 1, (size_t)adjcols * 4)) ||
        (s = ensure_dev(ctx, 2, (size_t)substsz * substsz * 4)) || (s = ensure_dev(ctx, 3, (size_t)geom.hrowElems * 4)) ||
        (s = ensure_dev(ctx, 4, (size_t)geom.hcolElems * 4)))
        return s;
    hipError_t e;
    Buf& ptfl = ctx->buf[kBufPtFlags];
    bool fresh = false;
    if ((s = reserve_hard(ctx, ptfl, trows * sizeof(unsigned long long), 0, &fresh)) != GSA_SUCCESS) return s;
    if (fresh) std::memset(ptfl.p, 0, ptfl.cap);
    unsigned long long* const ptflags = ptfl.as<unsigned long long>();
    unsigned long long* dflags = nullptr;
    if ((e = hipHostGetDevicePointer((void**)&dflags, ptflags, 0)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    L.alloc = ms_since(t);
    lap(ctx, "align.alloc");
    if ((e = hipMemcpyAsync(ctx->buf[kBufIo0].p, seqY, (size_t)adjrows * 4, hipMemcpyHostToDevice, ctx->stream)) ||
        (e = hipMemcpyAsync(ctx->buf[kBufIo1].p, seqX, (size_t)adjcols * 4, hipMemcpyHostToDevice, ctx->stream)) ||
        (e = hipMemcpyAsync(ctx->buf[kBufIo2].p, subst, (size_t)substsz * substsz * 4, hipMemcpyHostToDevice, ctx->stream)) ||
        (e = hipStreamSynchronize(ctx->stream)))
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    L.cpy_dev = ms_since(t);
    lap(ctx, "align.cpy_dev");
    lap(ctx, "align.init_hdr");  // headers are written by the fill launch itself
    int32_t* dhr = ctx->buf[kBufIo3].as<int32_t>();
    int32_t* dhc = ctx->buf[kBufIo4].as<int32_t>();
    // Column chunks of ptChunk tile columns: a chunk's headers (header rows and columns of every
    // tile row) are final once every tile row's word counts it; the fill reaches a column in every
    // super-strip within the wavefront's fill-in, so chunks complete left to right while the fill
    // runs, and each is copied back (one strided copy per matrix) as soon as it is complete.
    const int tcols = geom.tileHdrMatCols;
    // ~4096 columns per chunk, fewer (down to one tile column) while two chunks of every tile row
    // overfill the kPtPin staging slots: the pinned buffer stays 64 MB up to ~7.8M rows at tBx 64
    const size_t chunkCol = trows * (size_t)(geom.tileHrowLen + geom.tileHcolLen) * 4;  // one tile column
    int cw = std::max(1, std::min(tcols, (4096 + tileBx - 1) / tileBx));
    while (cw > 1 && 2 * chunkCol * (size_t)cw > gsa_ctx::kPtPin) cw = (cw + 1) / 2;
    const int nCh = (tcols + cw - 1) / cw;
    {
        // room for a batch of at least one chunk
        const size_t need = std::max(gsa_ctx::kPtPin, 2 * chunkCol * (size_t)cw);
        if ((s = reserve_hard(ctx, ctx->buf[kBufPtPin], need)) != GSA_SUCCESS) return s;
    }
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    s = enqueue_fill(ctx, gsa::kModeSparse, ctx->buf[kBufIo0].as<const int32_t>(), adjrows, ctx->buf[kBufIo1].as<const int32_t>(),
                     adjcols, ctx->buf[kBufIo2].as<const int32_t>(), substsz, gapo, nullptr, tileBx, dhr, dhc, ctx->stream,
                     dflags, cw);
    if (s != GSA_SUCCESS) return s;
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    const unsigned long long epoch = ctx->epoch;
    const size_t rowW = (size_t)geom.tileHrowLen * 4, rowH = (size_t)geom.tileHcolLen * 4;  // bytes per tile
    // The caller's result buffers are usually fresh pages: fault them in (the kernel zero-fills each
    // page on first touch) on the copy threads while the fill runs, before the first chunk arrives,
    // instead of inside the first chunk's scatter (measured: 2-4.6 ms for an 8 MB chunk at 100k)
    std::vector<std::thread> prefault;
    {
        constexpr int T = gsa_ctx::kCopyThreads;
        const size_t nb[2] = {(size_t)geom.hrowElems * 4, (size_t)geom.hcolElems * 4};
        char* base[2] = {(char*)hrow_out, (char*)hcol_out};
        for (int k = 0; k < T; ++k)
            prefault.emplace_back([=]() {
                for (int m = 0; m < 2; ++m)
                {
                    const size_t lo = nb[m] * k / T, hi = nb[m] * (k + 1) / T;
                    for (size_t o = lo & ~(size_t)4095; o < hi; o += 4096)
                        if (o >= lo) ((volatile char*)base[m])[o] = 0;
                }
            });
    }
    auto join_prefault = [&]() {
        for (auto& x : prefault) x.join();
        prefault.clear();
    };
    struct JoinAtExit  // every return path joins the prefault threads
    {
        std::vector<std::thread>& v;
        ~JoinAtExit()
        {
            for (auto& x : v)
                if (x.joinable()) x.join();
        }
    } joinAtExit {prefault};
    int copied = 0;  // chunks copied back
    // Two pinned slots: the strided DMA of one batch of chunks (ptstream) runs while the copy
    // threads scatter the previous batch into the tile-major host matrices.
    const size_t chunkBytes = trows * (size_t)cw * (rowW + rowH);
    const size_t slotBytes = ctx->buf[kBufPtPin].cap / 2;
    const int perBatch = (int)std::max<size_t>(1, slotBytes / chunkBytes);
    struct Batch
    {
        int c0, c1, slot;
    };
    Batch inflight[2];
    int nInflight = 0, issued = 0, nextSlot = 0;
    struct DrainAtExit  // an error return waits for DMAs still writing the pinned slots
    {
        gsa_ctx* c;
        const int& n;
        ~DrainAtExit()
        {
            if (n > 0) (void)hipStreamSynchronize(c->ptstream);
        }
    } drainAtExit {ctx, nInflight};
    auto batch_geom = [&](const Batch& bt, size_t& j0, size_t& wr, size_t& wc, char*& hh, char*& hc) {
        j0 = (size_t)bt.c0 * cw;
        const size_t j1 = std::min((size_t)tcols, (size_t)bt.c1 * cw);
        wr = (j1 - j0) * rowW;  // bytes per tile row
        wc = (j1 - j0) * rowH;
        hh = ctx->buf[kBufPtPin].as<char>() + (size_t)bt.slot * slotBytes;
        hc = hh + trows * wr;
    };
    // the DMA engine reads HBM (the fill's header stores are system-scope and acknowledged before
    // their chunk is published); ptstream is the context's second stream, created right after the
    // fill's, so it has a hardware queue of its own and its copies run beside the fill (copies on
    // streams that share the fill's queue wait for it: measured)
    auto issue = [&](int upTo) -> hipError_t {
        Batch bt {issued, std::min(upTo, issued + perBatch), nextSlot};
        size_t j0, wr, wc;
        char *hh, *hc;
        batch_geom(bt, j0, wr, wc, hh, hc);
        hipError_t err = hipMemcpy2DAsync(hh, wr, (const char*)dhr + j0 * rowW, tcols * rowW, wr, trows,
                                          hipMemcpyDeviceToHost, ctx->ptstream);
        if (err == hipSuccess)
            err = hipMemcpy2DAsync(hc, wc, (const char*)dhc + j0 * rowH, tcols * rowH, wc, trows, hipMemcpyDeviceToHost,
                                   ctx->ptstream);
        if (err == hipSuccess) err = hipEventRecord(ctx->ptev[bt.slot], ctx->ptstream);
        if (err != hipSuccess) return err;
        inflight[nInflight++] = bt;
        issued = bt.c1;
        nextSlot ^= 1;
        return hipSuccess;
    };
    // scatter the oldest batch once its DMA is done (wait: block until it is)
    auto scatter = [&](bool wait) -> hipError_t {
        const Batch bt = inflight[0];
        hipError_t err = wait ? hipEventSynchronize(ctx->ptev[bt.slot]) : hipEventQuery(ctx->ptev[bt.slot]);
        if (err == hipErrorNotReady) return hipSuccess;
        if (err != hipSuccess) return err;
        join_prefault();
        size_t j0, wr, wc;
        char *hh, *hc;
        batch_geom(bt, j0, wr, wc, hh, hc);
        constexpr int T = gsa_ctx::kCopyThreads;
        auto work = [&](int k) {
            for (size_t r = (size_t)k; r < trows; r += T)
            {
                std::memcpy((char*)hrow_out + r * tcols * rowW + j0 * rowW, hh + r * wr, wr);
                std::memcpy((char*)hcol_out + r * tcols * rowH + j0 * rowH, hc + r * wc, wc);
            }
        };
        std::vector<std::thread> th;
        for (int k = 1; k < T; ++k) th.emplace_back(work, k);
        work(0);
        for (auto& x : th) x.join();
        copied = bt.c1;
        inflight[0] = inflight[1];
        --nInflight;
        return hipSuccess;
    };
    // one pipeline step: issue a DMA for ready chunks if a slot is free, scatter a finished batch
    auto pump = [&](int ready, bool wait) -> hipError_t {
        hipError_t err = hipSuccess;
        if (ready > issued && nInflight < 2) err = issue(ready);
        if (err == hipSuccess && nInflight > 0) err = scatter(wait || nInflight == 2);
        return err;
    };
    for (;;)
    {
        const hipError_t q = hipStreamQuery(ctx->stream);  // the fill (and its headers kernel) finished?
        if (q != hipSuccess && q != hipErrorNotReady) return fail(ctx, q, GSA_ERROR_KERNEL_FAILURE);
        if (q == hipSuccess) break;
        int ready = nCh;
        for (size_t r = 0; r < trows && ready > issued; ++r)
        {
            const unsigned long long v = __atomic_load_n(ptflags + r, __ATOMIC_ACQUIRE);
            ready = std::min(ready, (v >> 32) == epoch ? (int)(v & 0xffffffffu) : 0);
        }
        if (ready > issued || nInflight > 0)
        {
            if ((e = pump(ready, false)) != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        }
        else
            std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    if ((s = gsa_sync(ctx, ctx->stream)) != GSA_SUCCESS) return s;
    L.calc = ms_since(t);
    lap(ctx, "align.calc");
    (void)hipEventElapsedTime(&L.calc_kernel_ms, ctx->ev0, ctx->ev1);
    while (copied < nCh)
        if ((e = pump(nCh, true)) != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    L.cpy_host = ms_since(t);
    lap(ctx, "align.cpy_host");
    int32_t cost = gsa_sparse_align_cost(hrow_out, hcol_out, &geom, seqY, adjrows, seqX, adjcols, subst, substsz, gapo);
    L.calc += ms_since(t);
    lap(ctx, "align.calc");
    if (align_cost) *align_cost = cost;
    if (geom_out) *geom_out = geom;
    if (laps) *laps = L;
    return GSA_SUCCESS;
}

}  // extern "C"
