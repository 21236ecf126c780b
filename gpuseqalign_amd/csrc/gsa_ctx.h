// gsa_ctx.h -- the context behind the C API (include/gsa.h) and the helpers its translation units
// share: gsa_capi.hip (fills, traces, host-buffer entry points) and gsa_score.hip (score-only and
// database entry points).  Internal: not installed, included by those two only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../../include/gsa.h"
#include "nw_strip.h"

// One grow-only buffer of the context: device memory, pinned host memory or mapped host memory.
// The capacity is in bytes, whatever the buffer holds.
enum BufKind { kBufDevice, kBufPinned, kBufMapped };
struct Buf
{
    void* p = nullptr;
    size_t cap = 0;  // bytes
    BufKind kind = kBufDevice;
    template <class T>
    T* as() const
    {
        return (T*)p;
    }
};

inline void release(Buf& b)
{
    if (b.p) (void)(b.kind == kBufDevice ? hipFree(b.p) : hipHostFree(b.p));
    b.p = nullptr;
    b.cap = 0;
}

// Make `b` hold at least `bytes`: nothing to do when it exists and is large enough; otherwise it is
// freed and allocated anew at max(bytes, floor) (growth is to the requested size, never a shrink),
// and left empty when that fails.  A buffer may be regrown while an earlier launch on some stream
// still reads it: that is safe only because hipFree / hipHostFree wait for the device, so this must
// stay on the synchronous allocator (no hipFreeAsync, hipMallocAsync or memory pools).  The caller
// maps the error to its own policy (reserve_hard; the soft failures of the expansion scratch and the
// trace band).  *fresh is set when the buffer was allocated anew (its contents are undefined).
inline hipError_t reserve(Buf& b, size_t bytes, size_t floor, bool* fresh = nullptr)
{
    if (b.p && b.cap >= bytes) return hipSuccess;
    release(b);
    const size_t want = std::max(bytes, floor);
    const hipError_t e = b.kind == kBufDevice   ? hipMalloc(&b.p, want)
                         : b.kind == kBufPinned ? hipHostMalloc(&b.p, want, hipHostMallocDefault)
                                                : hipHostMalloc(&b.p, want, hipHostMallocMapped);
    if (e != hipSuccess)
    {
        b.p = nullptr;
        return e;
    }
    b.cap = want;
    if (fresh) *fresh = true;
    return hipSuccess;
}

// Pinned staging slots for small host-to-device copies enqueued in stream order (pair descriptors,
// schedules): a slot is written by the host, copied from on a stream, and reused only after the
// event recorded behind its copy has completed.  The events are the context's (gsa_ctx_create /
// gsa_ctx_destroy).
struct StageRing
{
    static constexpr int kStage = 4;
    Buf slot[kStage];
    hipEvent_t ev[kStage] = {nullptr, nullptr, nullptr, nullptr};
    bool used[kStage] = {false, false, false, false};
    int next = 0, cur = 0;
    StageRing()
    {
        for (Buf& b : slot) b.kind = kBufPinned;
    }
    // The next slot, free of its previous copy and at least `bytes` large.  Returns a gsa status, the
    // HIP error behind a failure in *e.
    int acquire(size_t bytes, void** host, hipError_t* e)
    {
        cur = next;
        next = (cur + 1) % kStage;
        if (used[cur] && (*e = hipEventSynchronize(ev[cur])) != hipSuccess) return GSA_ERROR_CUDA_GENERAL;
        if ((*e = reserve(slot[cur], bytes, 0)) != hipSuccess) return GSA_ERROR_MEMORY_ALLOCATION;
        *host = slot[cur].p;
        return GSA_SUCCESS;
    }
    // Behind the copy from the acquired slot, on the copy's stream.
    hipError_t commit(hipStream_t st)
    {
        const hipError_t e = hipEventRecord(ev[cur], st);
        if (e == hipSuccess) used[cur] = true;
        return e;
    }
};

// The context's buffers (gsa_ctx::buf), all grow-only.  Device memory unless noted.
enum BufId
{
    kBufGran,  // hand-off granules of the last launch (epoch-tagged, cleared once per allocation)
    // pair descriptors of the last launches, then the batch schedule (units of gsa::PairDesc); staged
    // through gsa_ctx::stage
    kBufDesc,
    // two-pass full fill (nw_expand.h): pass-1 outputs (header rows / columns, rows 64m) of the last
    // launch, and the expansion's pair descriptors and schedule (staged through gsa_ctx::expin).
    // Slot 1 of each: the tail group of a split batch (enqueue_full_split)
    kBufExp0,
    kBufExp1,
    kBufExpDesc0,
    kBufExpDesc1,
    // scratch of the host-buffer entry points (like DeviceArray::init): the sequences, the table, the outputs
    kBufIo0,
    kBufIo1,
    kBufIo2,
    kBufIo3,
    kBufIo4,
    kBufXdone,   // fused single-pair fill: one progress word per pass-1 strip (epoch-tagged, cleared once per allocation)
    kBufStamps,  // GSA_STAMPS=1: the fill's stamps of the last launch (gsa_debug_stamps)
    kBufClk,     // gsa_set_full_timing: the expansion's per-workgroup clock stamps
    // score-only NW from both ends (score_bidi): tap rows of both halves, the reversed sequences, the
    // combine's result, the transposed table (ints)
    kBufBidi,
    kBufChk,  // verification results (nw_check.hip), 64 bytes
    // device traceback (nw_trace_dev.hip): move bytes, [moves, cost] (64 bytes), global move codes
    kBufTmoves,
    kBufTres,
    kBufTdirs,
    // tiles precomputed around the diagonal (trace_band): codes, and [list | map] ints
    kBufTband,
    kBufTlist,
    kBufSbnd,  // score-only row scan (nw_scan.hip): boundary rows H/F, progress words (ints)
    // score-only control words (64 bytes): row scan [0] ticket|err, [1] best key, [2] result; AG/SW strip
    // [0] result, [1] best key, [3] its own error word (the fills' sticky word is not touched)
    kBufSctl,
    // score batch (gsa_score_batch_dev): two result words per pair, then the decoded answers
    // (gsa::ScoreOut per pair and one for the error word)
    kBufSbatch,
    // database search (gsa_score_db_dev): task counter, the lane subjects' offsets, lengths and results;
    // the boundary rows of the resident waves (queries of more than one sweep)
    kBufDbl,
    kBufDbbnd,
    // alignments of database hits (gsa_align_db_dev): the move codes of one chunk, its task counter and
    // per-hit offsets, lengths and fill results, the walk's results and move bytes
    kBufAdbCodes,
    kBufAdbMeta,
    kBufAdbRes,
    // many queries against a database (gsa_score_db_multi_dev): counters, the lane subjects' offsets,
    // lengths and indices and a launch's queries; the result matrix of one chunk; the patches from the
    // other paths, then the chunk's hits and compacted scores; the ranking's keys and sort storage
    kBufDbmMeta,
    kBufDbmOut,
    kBufDbmRes,
    kBufDbmSel,
    // the alignment of one long pair (gsa_align_pair_dev): the move codes of one chunk of strips; the
    // fill's task counter and the walk's record; the move bytes
    kBufPairCodes,
    kBufPairMeta,
    kBufPairMoves,
    // the alignments of a batch of long pairs (gsa_align_batch_dev; codes and moves in the two slots
    // above): a round's task counter, task, pair and walk tables; the pairs' walk records
    kBufPairBatchTab,
    kBufPairBatchRec,
    // overlap score of one long pair (gsa_score_overlap_dev): column C of every row of every ticket (ints)
    kBufOvCol,
    // mlsppt: host-mapped per-tile-row words (epoch << 32 | column chunks in memory); a pinned host
    // buffer (>= kPtPin) the strided column chunks are packed into by copies on ptstream
    kBufPtFlags,  // mapped host memory
    kBufPtPin,    // pinned host memory
    kBufCount
};

struct gsa_ctx
{
    int device = 0;
    int cu_count = 0;
    long long lds_max = 65536;  // dynamic LDS a workgroup may opt into (bytes)
    hipStream_t stream = nullptr;
    // 256 bytes: [0] ticket (zeroed per launch), [1] error flags: sticky across launches, read and
    // cleared by gsa_sync (or by the synchronous call that reports them)
    unsigned* ctl = nullptr;
    unsigned long long spin_ticks = 100000000ull;  // watchdog: 1 s of s_memrealtime (100 MHz)
    Buf buf[kBufCount];
    unsigned epoch = 0;
    int last_hip_error = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // pinned staging of kBufDesc and of kBufExpDesc0 / 1
    static constexpr int kStage = StageRing::kStage;
    StageRing stage, expin;
    // the split batch (enqueue_full_split): its high-priority stream and the events between the groups
    hipStream_t splitstream = nullptr;
    hipEvent_t split_ev[2] = {nullptr, nullptr};
    // GSA_STAMPS=1: words of kBufStamps the last launch wrote, and its stream
    size_t stamps_n = 0;
    hipStream_t stamps_stream = nullptr;
    // gsa_set_full_timing: events around the passes of the last two-pass full fill and the
    // expansion's per-workgroup clock stamps (clk_n words of kBufClk)
    bool timing = false;
    hipEvent_t pev[3] = {nullptr, nullptr, nullptr};
    size_t clk_n = 0;
    int timing_state = 0;  // 0 none, 1 two launches (events + stamps), 2 fused (one launch), 3 pipelined
    int timing_groups = 0;
    // the batch expansion's task order, tuned per output buffer (enqueue_full_twopass): key, the
    // order each candidate took (ms, < 0: not measured), the order of the last launch and its events
    struct XTune
    {
        const void* key = nullptr;
        int pairs = 0;
        long long tasks = 0;
        float ms[2] = {-1.f, -1.f};
        int last = -1;
        bool pending = false;
        bool cold = true;  // the first launch on a key runs untimed (fresh pages, first-touch costs)
        hipEvent_t ev[2] = {nullptr, nullptr};
    } xt[2];  // per scratch slot
    // a batch that can run as two pair groups (enqueue_full_split): whole-job times of the four
    // candidates (one group or two, expansion order 1 or 2), keyed by the batch (enqueue_full)
    struct FTune
    {
        uint64_t key = 0;
        float ms[4] = {-1.f, -1.f, -1.f, -1.f};
        int last = -1;
        bool pending = false;
        bool cold = true;  // the first launch on a key runs untimed (fresh pages, first-touch costs)
        hipEvent_t ev[2] = {nullptr, nullptr};
    } ft;
    // mlsppt: the events behind the two halves of kBufPtPin and the copies' stream
    hipEvent_t ptev[2] = {nullptr, nullptr};
    static constexpr size_t kPtPin = 64u << 20;  // two slots
    hipStream_t ptstream = nullptr;
    hipEvent_t adbev[3] = {nullptr, nullptr, nullptr};  // gsa_align_db_dev, gsa_align_pair_dev: around the fill and the walk
    hipEvent_t dbmev[4] = {nullptr, nullptr, nullptr, nullptr};  // gsa_score_db_multi_dev: the lane launches, the ranking
    // copy-back of the host-buffer entry points into pageable caller memory: per copy thread a
    // stream and two pinned chunks (DMA of chunk k+1 overlaps the host copy of chunk k)
    static constexpr int kCopyThreads = 8;
    static constexpr size_t kCopyChunk = 4u << 20;
    hipStream_t xstream[kCopyThreads] = {};
    Buf xstage[kCopyThreads][2];
    hipEvent_t xev[kCopyThreads][2] = {};
    gsa_mem_stats mem {};  // peak resource use of the fills since creation / gsa_mem_stats_reset
    // phase-boundary callback of the host-buffer entry points (gsa_set_lap_callback)
    gsa_lap_fn lap_fn = nullptr;
    void* lap_user = nullptr;
    // the knobs (kKnobNames): the environment when the context was created, then gsa_set_knob
    std::map<std::string, std::string> knobs;
    // gsa_last_launch: the instance the last call ran (kind 0: nothing launched yet), the stream it
    // ran on and the epoch its int8 instance writes to ctl[2] when it declines the table
    gsa_launch_info ll {};
    hipStream_t ll_stream = nullptr;
    unsigned ll_epoch0 = 0, ll_epoch = 0;  // first and last epoch of the call (a split batch has two)

    gsa_ctx()
    {
        buf[kBufPtFlags].kind = kBufMapped;
        buf[kBufPtPin].kind = kBufPinned;
        for (auto& pair : xstage)
            for (Buf& b : pair) b.kind = kBufPinned;
    }
};

// Defined in gsa_capi.hip, called from gsa_score.hip too (internal to the library)
#define GSA_INTERNAL __attribute__((visibility("hidden")))
GSA_INTERNAL int ensure_dev(gsa_ctx* ctx, int slot, size_t bytes);
GSA_INTERNAL int ensure_gran(gsa_ctx* ctx, size_t elems, hipStream_t st);
GSA_INTERNAL int ensure_desc(gsa_ctx* ctx, size_t n);
GSA_INTERNAL std::vector<int> batch_schedule(const gsa_ctx* ctx, const std::vector<gsa::PairDesc>& hd, long long tickets);
GSA_INTERNAL int stage_descs(gsa_ctx* ctx, const std::vector<gsa::PairDesc>& hd, const std::vector<int>& sched, hipStream_t st);

using Clock = std::chrono::steady_clock;

inline float ms_since(Clock::time_point& t)
{
    auto now = Clock::now();
    float ms = std::chrono::duration<float, std::milli>(now - t).count();
    t = now;
    return ms;
}

// Phase boundary of a host-buffer entry point: the caller's Stopwatch::lap(name)
// (stopwatch.cpp:43-50) through the registered callback, at the points the reference's align
// functions lap (nwalign_gpu9_mlsp_diagdiagdiag.cu:459-719)
inline void lap(gsa_ctx* ctx, const char* name)
{
    if (ctx->lap_fn) ctx->lap_fn(ctx->lap_user, name);
}

inline int fail(gsa_ctx* ctx, hipError_t e, int stat)
{
    ctx->last_hip_error = (int)e;
    // the runtime keeps its own last error until it is read: left there, the next call's launch check
    // (hipGetLastError behind its first kernel) would report this call's failure
    (void)hipGetLastError();
    return stat;
}

// reserve() under the hard-failure policy: the HIP error recorded, GSA_ERROR_MEMORY_ALLOCATION
inline int reserve_hard(gsa_ctx* ctx, Buf& b, size_t bytes, size_t floor = 0, bool* fresh = nullptr)
{
    const hipError_t e = reserve(b, bytes, floor, fresh);
    return e == hipSuccess ? GSA_SUCCESS : fail(ctx, e, GSA_ERROR_MEMORY_ALLOCATION);
}

// reserve_hard() for words whose tags must never match a live epoch by accident: the whole buffer is
// cleared once per allocation, in stream order before the launch that uses it (a non-blocking stream
// is not ordered behind the null stream).  A failed clear leaves the buffer to be allocated again.
inline int reserve_zeroed(gsa_ctx* ctx, Buf& b, size_t bytes, size_t floor, hipStream_t st)
{
    bool fresh = false;
    const int s = reserve_hard(ctx, b, bytes, floor, &fresh);
    if (s != GSA_SUCCESS || !fresh) return s;
    const hipError_t e = hipMemsetAsync(b.p, 0, b.cap, st);
    if (e == hipSuccess) return GSA_SUCCESS;
    b.cap = 0;
    return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
}

inline int check_inputs(int32_t adjrows, int32_t adjcols, int32_t substsz)
{
    if (adjrows < 1 || adjcols < 1) return GSA_ERROR_INVALID_VALUE;
    if (substsz < 1 || substsz > 32) return GSA_ERROR_INVALID_VALUE;  // LDS profile holds <= 32 letters
    return GSA_SUCCESS;
}

// the knob's value in this context, or null (unset)
inline const char* knob(const gsa_ctx* ctx, const char* name)
{
    auto it = ctx->knobs.find(name);
    return it == ctx->knobs.end() ? nullptr : it->second.c_str();
}

inline int env_int(const gsa_ctx* ctx, const char* name, int dflt)
{
    const char* e = knob(ctx, name);
    return e ? std::atoi(e) : dflt;
}

// NULL is the HIP null stream, as everywhere in HIP; the host-buffer entry points use the
// context's own stream explicitly.
inline hipStream_t pick_stream(gsa_ctx*, void* stream) { return (hipStream_t)stream; }

// Device bytes this context holds: the control words and every device buffer (scratch, hand-off
// granules, the host entry points' I/O buffers).  Pinned and mapped host memory is not counted.
inline long long held_bytes(const gsa_ctx* c)
{
    long long b = 256;
    for (const Buf& k : c->buf)
        if (k.kind == kBufDevice) b += (long long)k.cap;
    return b;
}

// Fold the footprint of the fill just launched (gsa::g_last_foot) into the context's peaks, as
// updateNwAlgPeakMemUsage does per launch (nwalign_shared.cpp:5-25).
inline void note_launch(gsa_ctx* c)
{
    const gsa::LaunchFoot& f = gsa::g_last_foot;
    c->mem.glmem_peak_allocs = std::max<int64_t>(c->mem.glmem_peak_allocs, held_bytes(c));
    c->mem.shmem_peak_allocs = std::max<int64_t>(c->mem.shmem_peak_allocs, f.lds_per_wg * f.active_wgs);
    c->mem.locmem_peak_allocs =
        std::max<int64_t>(c->mem.locmem_peak_allocs, f.scratch_per_lane * f.threads_per_wg * f.active_wgs);
    c->mem.regmem_peak_allocs =
        std::max<int64_t>(c->mem.regmem_peak_allocs, f.regs_per_lane * 4 * f.threads_per_wg * f.active_wgs);
}

// gsa_last_launch's record: a fresh one for the launch just decided (the caller fills the rest)
inline gsa_launch_info& new_launch_info(gsa_ctx* c, int kind, hipStream_t st, unsigned epoch)
{
    c->ll = gsa_launch_info {};
    c->ll.kind = kind;
    c->ll_stream = st;
    c->ll_epoch0 = c->ll_epoch = epoch;
    return c->ll;
}

// Read the sticky error word (after the caller's stream sync) and clear it if set.
inline hipError_t take_err(gsa_ctx* ctx, hipStream_t st, unsigned* err)
{
    hipError_t e = hipMemcpyAsync(err, ctx->ctl + 1, sizeof(unsigned), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && *err != 0)
    {
        e = hipMemsetAsync(ctx->ctl + 1, 0, sizeof(unsigned), st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    return e;
}
