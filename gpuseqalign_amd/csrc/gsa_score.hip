// gsa_score.hip -- the score-only and database entry points of libgsa.so (declared in include/gsa.h):
// gsa_score, gsa_score_dev, gsa_score_batch_dev, gsa_score_db_dev, gsa_score_db_multi_dev,
// gsa_align_db_dev, gsa_align_db_multi_dev, gsa_align_pair_dev and gsa_align_batch_dev, on the K-rows and strip score kernels (nw_krow.hip, nw_strip.hip), the row scan
// (nw_scan.hip), NW / SW from both ends (nw_bidi.hip) and the database lane kernels (nw_lanes.hip,
// nw_lanes_multi.hip, nw_lanes_trace.hip, nw_lanes_trace_multi.hip); the banded calls
// gsa_score_band_dev and gsa_align_pair_band_dev on nw_band.hip, their batch forms on nw_band_batch.hip,
// the banded extension calls (gsa_*_band_ext_*) on nw_band_ext.hip and nw_band_ext_batch.hip.  The context
// and the helpers shared with gsa_capi.hip are in gsa_ctx.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gsa.h"
#include "gsa_ctx.h"
#include "nw_band.h"
#include "nw_band_batch.h"
#include "nw_band_ext.h"
#include "nw_band_ext_batch.h"
#include "nw_bidi.h"
#include "nw_krow.h"
#include "nw_lanes.h"
#include "nw_lanes_multi.h"
#include "nw_lanes_semi.h"
#include "nw_lanes_semi_trace.h"
#include "nw_lanes_overlap.h"
#include "nw_lanes_overlap_trace.h"
#include "nw_lanes_trace.h"
#include "nw_lanes_trace_multi.h"
#include "nw_pair_semi_plan.h"
#include "nw_pair_semi_trace.h"
#include "nw_pair_semi_trace_batch.h"
#include "nw_pair_semi_trace_batch_plan.h"
#include "nw_pair_overlap_plan.h"
#include "nw_pair_overlap_trace.h"
#include "nw_pair_overlap_trace_batch.h"
#include "nw_pair_overlap_trace_batch_plan.h"
#include "nw_pair_trace.h"
#include "nw_pair_trace_batch.h"
#include "nw_pair_trace_batch_plan.h"
#include "nw_pair_trace_plan.h"
#include "nw_scan.h"
#include "nw_strip.h"

namespace {

// Score-only kernels: global alignments run on the strip kernel in its affine mode (shifted
// Gotoh, nw_strip.hip kModeScoreAG); local ones on the row scan (nw_scan.hip).  GSA_SCORE_SCAN=1
// sends global ones to the row scan as well (tests compare the two).
bool score_scan_forced(const gsa_ctx* ctx)
{
    const char* e = knob(ctx, "GSA_SCORE_SCAN");
    return e && std::atoi(e) == 1;
}

constexpr int kScoreTooLarge = 1000;  // internal: score_ag_strip -> row scan

// score-only fills on the K-rows layout (default) or, with GSA_SCORE_KERNEL=strip, the strip kernel
bool score_kernel_krow(const gsa_ctx* ctx)
{
    const char* e = knob(ctx, "GSA_SCORE_KERNEL");
    return !(e && std::strcmp(e, "strip") == 0);
}

// SW end-cell keys: score << bits | (2^bits-1 - row-major index), bits = ceil(log2((R+1)(C+1)));
// scores (< 2^31) keep 63 - bits >= 29 bits up to (R+1)(C+1) = 2^34
int sw_idx_bits(int64_t R, int64_t C) { return gsa::sw_idx_bits(R, C); }

// Score-only NW from both ends (nw_bidi.h): a single pair's wavefront time is (C + strips x hop)
// steps, and at 50k the strips' fill-in is ~30 % of it; the top half (rows 1..m) forward and the
// bottom half reversed (rows R..m+1 of the reversed pair) run at the same time, each with half the
// strips, as two pairs of one launch with their tickets interleaved, and a combine kernel takes the
// best crossing of the rows where they meet.  m = K floor(R/2K), so that row m of the top and row
// R - m of the reversed bottom are both a lane's last row (the strips' tap); R % K != 0 takes the
// one-direction path.
// Local modes (SW) run three pairs: the top half forward, the bottom half reversed, and the bottom
// half forward from a fresh (zero) border, whose end-cell keys (offset by m rows) share the top's
// swBest.  The keys then hold the best cell of every alignment that does not cross row m, first in
// row-major order, and the combine the best score through row m (M_cross).  If M_cross is below
// that score, or equal to it with the key's cell in the top half (before every crossing end), the
// key is the answer; otherwise an alignment through row m may end earlier or score more: when the top
// half ended on a ticket boundary, a second launch continues the pair from its ticket there, its row
// above the top's last-ticket granules (restamped), and the answer is the better of the top's keys
// and that run's (GSA_BIDI_SW_CONT=0: not); else the caller runs the one-direction kernel
// (kBidiFallback).
constexpr int kScoreTooLargeB = -1001;
constexpr int kBidiFallback = -1002;
int score_bidi(gsa_ctx* ctx, const int32_t* seqY, int64_t R, const int32_t* seqX, int64_t C, const int32_t* subst,
               int32_t substsz, int32_t gapo, int32_t gape, int K, bool transposed, gsa_score_result* out,
               hipStream_t st, bool local = false)
{
    const int64_t TR = (int64_t)(64 * K) * gsa::kSparseNS;
    const bool affine = gapo != gape;
    // The split.  A half whose rows end on a ticket boundary needs no lane tap: its last ticket's
    // drain writes that row to the granules like any other ticket's, and the combine reads it there.
    // A lane tap costs its strip 8 global stores per block, and as the half's last strip it sets the
    // half's end (50k NW-AG 2.94 ms with no tap, 3.19 with two lane taps).  So the top half ends on a
    // ticket boundary and takes the rows that make both halves end together: skew = p C 64K / (2 hop)
    // rows past R/2, p the lane tap's share of the C steps (0.117 affine, 0.05 linear: 8 / 4 stores
    // per block) and hop ~96 steps between strips; the bottom, when R is a multiple of the ticket too,
    // is free as well and the split even.  Short pairs keep two lane taps (m = K floor(R/2K)).
    int64_t m = (int64_t)K * (R / (2 * K));
    bool topFree = false, botFree = false;
    if (R >= 4 * TR && env_int(ctx, "GSA_BIDI_GRAN", 1))
    {
        const int skewEnv = env_int(ctx, "GSA_BIDI_SKEW", -1);
        // (local linear: 0.075, the third pair's share of the chip moves the balance; 50k SW-LG
        // 2.78 -> 2.76 ms, profiles/r05_sw_skew.txt)
        const double p = affine ? 0.117 : local ? 0.075 : 0.05;
        const bool both = R % TR == 0;
        const int64_t skew = both ? 0 : skewEnv >= 0 ? skewEnv : (int64_t)(p * (double)C * 64.0 * K / (2.0 * 96.0));
        int64_t mt = TR * (int64_t)llround((double)(R / 2 + skew) / (double)TR);
        mt = std::min(std::max(mt, TR), (R - 2 * K) / TR * TR);
        if (mt >= TR && R - mt >= 2 * K && (R - mt) % K == 0)
        {
            m = mt;
            topFree = true;
            botFree = both;
        }
    }
    const int64_t mb = R - m;
    const int64_t tkTop = (m + TR - 1) / TR, tkBot = (mb + TR - 1) / TR;
    const int nP = local ? 3 : 2;
    const size_t tapLen = ((size_t)gsa::kTapPad + (size_t)C + 160 + 63) & ~(size_t)63;
    // layout (ints): tap rows H, F of the top, then of the bottom; reversed Y (mb + 1), reversed X
    // (C + 1), the combine's result
    const size_t oRY = 4 * tapLen, oRX = oRY + (size_t)mb + 1, oRes = (oRX + (size_t)C + 1 + 63) & ~(size_t)63;
    const size_t oSub = oRes + 64;  // transposed: the table transposed
    const size_t need = oSub + (size_t)substsz * (size_t)substsz;
    hipError_t e;
    int s;
    if ((s = reserve_hard(ctx, ctx->buf[kBufBidi], need * sizeof(int))) != GSA_SUCCESS ||
        (s = reserve_hard(ctx, ctx->buf[kBufSctl], 64)) != GSA_SUCCESS)
        return s;
    int* const bidi = ctx->buf[kBufBidi].as<int>();
    unsigned long long* const sctl = ctx->buf[kBufSctl].as<unsigned long long>();
    int* tapH = bidi;
    int* tapF = tapH + tapLen;  // half 1: + 2 tapLen
    int* ry = bidi + oRY;
    int* rx = bidi + oRX;
    int* res = bidi + oRes;
    int* substT = transposed ? bidi + oSub : nullptr;
    if ((s = ensure_desc(ctx, local ? 4 : 2)) != GSA_SUCCESS) return s;
    const size_t stride = (size_t)gsa::gran_stride((int)C);
    const size_t granAll = (size_t)(tkTop + (nP - 1) * tkBot) * stride;
    const int64_t tkAll = (R + TR - 1) / TR;  // local, the way back: the whole pair's tickets
    if ((s = ensure_gran(ctx, 2 * granAll + (local ? 2 * (size_t)tkAll * stride : 0), st)) != GSA_SUCCESS) return s;
    gsa::PairDesc* const ddesc = ctx->buf[kBufDesc].as<gsa::PairDesc>();
    unsigned long long* const dgran = ctx->buf[kBufGran].as<unsigned long long>();
    gsa::PairDesc d[3];
    std::memset(d, 0, sizeof(d));
    d[0].seqY = seqY;
    d[0].seqX = seqX;
    d[0].R = (int)m;
    d[0].nTickets = (int)tkTop;
    d[0].granOff = 0;
    d[1].seqY = ry;
    d[1].seqX = rx;
    d[1].R = (int)mb;
    d[1].nTickets = (int)tkBot;
    d[1].granOff = (long long)((size_t)tkTop * stride);
    // local: the bottom half forward, rows m+1 .. R (seqY + m: its element 0 is row m's letter,
    // unused), from a fresh border
    d[2].seqY = seqY + m;
    d[2].seqX = seqX;
    d[2].R = (int)mb;
    d[2].nTickets = (int)tkBot;
    d[2].granOff = (long long)((size_t)(tkTop + tkBot) * stride);
    d[2].rowOff = (int)m;
    // local: keys of the top (StripArgs::swBest, word 1), of the reversed bottom (word 4, unused) and
    // of the fresh bottom (word 5)
    if (local)
    {
        d[1].swBest = sctl + 4;
        d[2].swBest = sctl + 5;
    }
    for (int h = 0; h < 3; ++h) d[h].C = d[h].Cp = (int)C;
    const int mode = local ? (affine ? gsa::kModeScoreSW : gsa::kModeScoreSWL) : affine ? gsa::kModeScoreAG : gsa::kModeScoreAGL;
    const int q8env = env_int(ctx, "GSA_KROW_Q8", 1);
    const int q8 =
        (q8env != 0 && (q8env == 2 || K == 4) && gsa::krow_score_lds_bytes(substsz, true) <= (size_t)ctx->lds_max) ? 1 : 0;
    gsa::StripArgs a;
    std::memset(&a, 0, sizeof(a));
    a.subst = transposed ? substT : subst;
    a.substsz = substsz;
    a.g = gapo;
    a.go = gapo;
    a.ge = gape;
    a.ns = gsa::kSparseNS;
    a.pairs = ddesc;
    a.nPairs = nP;
    a.nTicketsTotal = (int)(tkTop + (nP - 1) * tkBot);
    a.bidiTop = (int)tkTop;
    a.bidiMid = local ? (int)tkBot : 0;
    a.gran = dgran;
    a.gran2 = dgran + granAll;
    a.ticket = ctx->ctl;
    a.q8flag = ctx->ctl + 2;
    a.err = (unsigned*)(sctl + 3);
    a.agResult = (int*)sctl;
    a.swBest = sctl + 1;
    a.spin = ctx->spin_ticks;
    a.idxBits = sw_idx_bits(R, C);
    a.epoch = ++ctx->epoch;
    if (a.epoch == 0) a.epoch = ++ctx->epoch;
    a.q8 = q8;
    a.tapRow = topFree ? 0 : (int)m;
    a.tapRowB = botFree ? 0 : (int)mb;
    a.tapGran = (topFree ? 1 : 0) | (botFree ? 2 : 0);
    a.tapH = tapH;
    a.tapF = tapF;
    a.tapStride = (int)(2 * tapLen);
    (void)hipEventRecord(ctx->ev0, st);
    if ((e = gsa::launch_bidi_prep(d[0], d[1], ddesc, seqY, (int)m, (int)R, seqX, (int)C, ry, rx, ctx->ctl, sctl,
                                   res, subst, substsz, substT, st, local ? &d[2] : nullptr)) != hipSuccess ||
        (e = gsa::launch_krow_score(a, mode, K, std::max(1, std::min(a.nTicketsTotal, ctx->cu_count)), st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    note_launch(ctx);
    {
        gsa_launch_info& li = new_launch_info(ctx, GSA_LAUNCH_SCORE_KROW, st, a.epoch);
        li.ns = a.ns;
        li.k = K;
        li.q8 = q8;
        li.both_ends = 1;
        li.npairs = nP;
        li.tickets = a.nTicketsTotal;
    }
    // the rows where the halves meet: a lane tap (tap rows, one int per column from kTapPad), or the
    // half's last-ticket granules (the low word of each 64-bit granule)
    const int* gTop = (const int*)(dgran + (size_t)(tkTop - 1) * stride);
    const int* gBot = (const int*)(dgran + (size_t)(tkTop + tkBot - 1) * stride);
    const int* tH = topFree ? gTop : tapH + gsa::kTapPad;
    const int* tF = topFree ? gTop + 2 * granAll : tapF + gsa::kTapPad;
    const int* bH = botFree ? gBot : tapH + 2 * tapLen + gsa::kTapPad;
    const int* bF = botFree ? gBot + 2 * granAll : tapF + 2 * tapLen + gsa::kTapPad;
    if ((e = gsa::launch_bidi_combine(tH, tF, topFree ? 2 : 1, bH, bF, botFree ? 2 : 1, (int)m, (int)mb, (int)C, gapo,
                                      gape, affine, res, st, local)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    (void)hipEventRecord(ctx->ev1, st);
    unsigned long long rw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int score = 0;
    if ((e = hipMemcpyAsync(rw, sctl, sizeof(rw), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipMemcpyAsync(&score, res, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    (void)hipEventElapsedTime(&out->calc_kernel_ms, ctx->ev0, ctx->ev1);
    const unsigned err = (unsigned)rw[3];
    if (err == 2u) return kScoreTooLargeB;  // a value outside int16: the row scan
    if (err != 0) return GSA_ERROR_KERNEL_FAILURE;
    if (local)
    {
        if (rw[0] & 1u) return kScoreTooLargeB;  // a score >= 2^26: the row scan
        const int bits = sw_idx_bits(R, C);
        const unsigned long long mask = (1ull << bits) - 1;
        unsigned long long key = std::max(rw[1], rw[5]);  // top, fresh bottom
        unsigned long long idx = key ? mask - (key & mask) : 0;
        long long best = key ? (long long)(key >> bits) : 0;
        const long long ie = (long long)(idx / (unsigned long long)(C + 1));
        const bool fallback = !((long long)score < best || ((long long)score == best && ie <= m));
        const bool cont = fallback && topFree && env_int(ctx, "GSA_BIDI_SW_CONT", 1) != 0;
        if (env_int(ctx, "GSA_BIDI_LOG", 0))  // (tests: which way the pair went)
            std::fprintf(stderr, "gsa local both ends: m %lld, through m %d, best off it %lld at row %lld -> %s\n",
                         (long long)m, score, best, ie,
                         !fallback ? "answer" : cont ? "bottom again from row m" : "one direction");
        if (fallback && !cont) return kBidiFallback;
        if (cont)
        {
            // the pair from ticket tkTop on, its row above the top's last-ticket granules, in a granule
            // area of its own (its later tickets must not meet another half's granules)
            unsigned long long* seedH = dgran + 2 * granAll;
            unsigned long long* seedF = seedH + (size_t)tkAll * stride;
            unsigned ep2 = ++ctx->epoch;
            if (ep2 == 0) ep2 = ++ctx->epoch;
            const size_t last = (size_t)(tkTop - 1) * stride;
            gsa::PairDesc dc;
            std::memset(&dc, 0, sizeof(dc));
            dc.seqY = seqY;
            dc.seqX = seqX;
            dc.R = (int)R;
            dc.C = dc.Cp = (int)C;
            dc.nTickets = (int)tkAll;
            dc.swBest = sctl + 6;
            gsa::StripArgs b = a;
            b.pairs = ddesc + 3;
            b.nPairs = 1;
            b.bidiTop = b.bidiMid = 0;
            b.nTicketsTotal = (int)(tkAll - tkTop);
            b.tkFirst = (int)tkTop;
            b.gran = seedH;
            b.gran2 = seedF;
            b.epoch = ep2;
            b.tapRow = b.tapRowB = b.tapGran = 0;
            if ((e = hipMemcpyAsync(ddesc + 3, &dc, sizeof(dc), hipMemcpyHostToDevice, st)) != hipSuccess ||
                (e = hipMemsetAsync(ctx->ctl, 0, 4, st)) != hipSuccess ||
                (e = hipMemsetAsync(sctl, 0, 8, st)) != hipSuccess ||
                (e = hipMemsetAsync(sctl + 6, 0, 8, st)) != hipSuccess)
                return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
            if ((e = gsa::launch_bidi_seed(dgran + last, affine ? dgran + granAll + last : nullptr, seedH + last,
                                           affine ? seedF + last : nullptr, (long long)stride, ep2, st)) != hipSuccess ||
                (e = gsa::launch_krow_score(b, mode, K, std::max(1, std::min(b.nTicketsTotal, ctx->cu_count)), st)) !=
                    hipSuccess)
                return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
            note_launch(ctx);
            ctx->ll_epoch = ep2;  // (the record stays the both-ends call's; the word is this launch's)
            (void)hipEventRecord(ctx->ev1, st);
            if ((e = hipMemcpyAsync(rw, sctl, sizeof(rw), hipMemcpyDeviceToHost, st)) != hipSuccess ||
                (e = hipStreamSynchronize(st)) != hipSuccess)
                return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
            (void)hipEventElapsedTime(&out->calc_kernel_ms, ctx->ev0, ctx->ev1);
            const unsigned err2 = (unsigned)rw[3];
            if (err2 == 2u) return kScoreTooLargeB;
            if (err2 != 0) return GSA_ERROR_KERNEL_FAILURE;
            if (rw[0] & 1u) return kScoreTooLargeB;
            key = std::max(rw[1], rw[6]);  // the top's keys (word 1 is not touched again), the rest's
            idx = key ? mask - (key & mask) : 0;
            best = key ? (long long)(key >> bits) : 0;
        }
        out->score = (int32_t)best;
        out->i_end = (int64_t)(idx / (unsigned long long)(C + 1));
        out->j_end = (int64_t)(idx % (unsigned long long)(C + 1));
        return GSA_SUCCESS;
    }
    out->score = score;
    out->i_end = transposed ? C : R;
    out->j_end = transposed ? R : C;
    return GSA_SUCCESS;
}

// What a one-direction launch of score_ag_strip ran (gsa_align_pair_dev reads the checkpoint rows
// the K-rows kernel left in kBufGran: row t at t gran_stride(C), the affine second array `tickets`
// rows behind).
struct ScoreRoute
{
    bool krow = false;  // the K-rows score kernel (else the strip kernel)
    int K = 0;          // its rows per lane
    int64_t tickets = 0;
};

// route (may be null): no split from both ends for this call, and what ran instead
int score_ag_strip(gsa_ctx* ctx, const int32_t* seqY, int64_t R, const int32_t* seqX, int64_t C, const int32_t* subst,
                   int32_t substsz, int32_t gapo, int32_t gape, int32_t local, gsa_score_result* out, hipStream_t st,
                   ScoreRoute* route = nullptr)
{
    // the K-rows score kernel's rows per lane, tickets of 64 K NS rows: 2 in the modes with the
    // longer step (SW tracking, affine gaps: the block's fixed part is a smaller share there, and
    // twice the strips shorten it), 4 for NW-LG; same box, 5k-100k pairs: NW-AG -5..-7 %, SW-AG
    // -9..-11 %, SW-LG -2..-5 % with 2, NW-LG +12..18 % (profiles/r04_score_k.txt).  GSA_SCORE_K
    // = 2 / 4 forces one
    const int kenv = env_int(ctx, "GSA_SCORE_K", 0);
    const int scoreK = kenv == 2 || kenv == 4 ? kenv : (!local && gapo == gape) ? 4 : 2;
    // the K-rows score kernel unless GSA_SCORE_KERNEL=strip, or its LDS (a profile of substsz rows)
    // does not fit, or SW with ge > 0 (its per-row key offsets assume z grows along j); the strip
    // kernel's score modes otherwise, on its own 1024-row tickets
    const bool krow = score_kernel_krow(ctx) && (!local || gape <= 0) && gsa::krow_score_lds_bytes(substsz) <= ctx->lds_max;
    const int64_t TR = krow ? (int64_t)(64 * scoreK) * gsa::kSparseNS : (int64_t)gsa::kWaveRows * gsa::kSparseNS;
    const int64_t tickets = (R + TR - 1) / TR;
    if (tickets > (1ll << 30) || C > (1ll << 30)) return GSA_ERROR_INVALID_VALUE;
    // NW from both ends (score_bidi) when each half keeps >= 4 tickets, at 2 rows per lane in both
    // NW modes (its halves have half the strips, so the shorter block wins for NW-LG too: 50k 2.25 ->
    // 2.11 ms, profiles/r05_bidi_ab.txt).  GSA_SCORE_BIDI: 0 never, 2 at any size (tests)
    // A pair whose R is not a multiple of K but whose C is runs transposed (X down the rows, Y along
    // them, the table transposed: the same global score, and gaps cost the same either way).
    const int bidi = route ? 0 : env_int(ctx, "GSA_SCORE_BIDI", 1);
    const int kb = kenv == 2 || kenv == 4 ? kenv : 2;
    const int64_t TRb = (int64_t)(64 * kb) * gsa::kSparseNS;
    auto splits = [&](int64_t rows) { return rows % kb == 0 && rows >= 2 * kb && (bidi == 2 || rows >= 8 * TRb); };
    if (krow && !local && bidi != 0 && (splits(R) || splits(C)))
    {
        const bool tr = !splits(R);
        const int sb = tr ? score_bidi(ctx, seqX, C, seqY, R, subst, substsz, gapo, gape, kb, true, out, st)
                          : score_bidi(ctx, seqY, R, seqX, C, subst, substsz, gapo, gape, kb, false, out, st);
        return sb == kScoreTooLargeB ? kScoreTooLarge : sb;
    }
    // local: from both ends only by rows (the end cell's row-major tie rule does not survive a
    // transpose), and back to one direction when an alignment through the split may decide it
    if (route)
    {
        route->krow = krow;
        route->K = scoreK;
        route->tickets = tickets;
    }
    float bidiMs = 0.f;
    if (krow && local && bidi != 0 && env_int(ctx, "GSA_SCORE_BIDI_SW", 1) && splits(R))
    {
        const int sb = score_bidi(ctx, seqY, R, seqX, C, subst, substsz, gapo, gape, kb, false, out, st, true);
        if (sb == kScoreTooLargeB) return kScoreTooLarge;
        if (sb != kBidiFallback) return sb;
        bidiMs = out->calc_kernel_ms;
    }
    gsa::StripArgs a;
    std::memset(&a, 0, sizeof(a));
    a.subst = subst;
    a.substsz = substsz;
    a.g = gapo;
    a.go = gapo;
    a.ge = gape;
    a.ns = gsa::kSparseNS;
    gsa::PairDesc d;
    std::memset(&d, 0, sizeof(d));
    d.seqY = seqY;
    d.seqX = seqX;
    d.R = (int)R;
    d.C = (int)C;
    d.Cp = (int)C;
    d.nTickets = (int)tickets;
    int s = ensure_desc(ctx, 1);
    if (s != GSA_SUCCESS) return s;
    gsa::PairDesc* const ddesc = ctx->buf[kBufDesc].as<gsa::PairDesc>();
    hipError_t e = hipMemcpyAsync(ddesc, &d, sizeof(d), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    const size_t gran = (size_t)tickets * (size_t)gsa::gran_stride((int)C);
    if ((s = ensure_gran(ctx, 2 * gran, st)) != GSA_SUCCESS) return s;
    if ((s = reserve_hard(ctx, ctx->buf[kBufSctl], 64)) != GSA_SUCCESS) return s;
    unsigned long long* const dgran = ctx->buf[kBufGran].as<unsigned long long>();
    unsigned long long* const sctl = ctx->buf[kBufSctl].as<unsigned long long>();
    a.pairs = ddesc;
    a.nPairs = 1;
    a.nTicketsTotal = (int)tickets;
    a.gran = dgran;
    a.gran2 = dgran + gran;
    a.ticket = ctx->ctl;
    // an error word of its own: a fill enqueued earlier on this stream keeps its sticky error for
    // the caller's gsa_sync, and its error does not read as this launch's
    a.err = (unsigned*)(sctl + 3);
    a.spin = ctx->spin_ticks;
    a.agResult = (int*)sctl;
    a.swBest = sctl + 1;
    a.idxBits = sw_idx_bits(R, C);
    a.epoch = ++ctx->epoch;
    if (a.epoch == 0) a.epoch = ++ctx->epoch;
    if ((e = hipMemsetAsync(ctx->ctl, 0, 4, st)) != hipSuccess || (e = hipMemsetAsync(sctl, 0, 32, st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    (void)hipEventRecord(ctx->ev0, st);
    const int grid = std::max(1, std::min((int)tickets, ctx->cu_count));
    // a linear gap (gapo == gape) runs the step without E' and F' (d = 0)
    const int mode = local ? (gapo == gape ? gsa::kModeScoreSWL : gsa::kModeScoreSW)
                           : (gapo == gape ? gsa::kModeScoreAGL : gsa::kModeScoreAG);
    // the int8 column profile where its LDS fits (the instance declines a table outside int8 and the
    // int16 instance behind it runs) for the 4-rows-per-lane geometry (NW-LG): 50k 2.52 -> 2.46 ms;
    // at 2 rows per lane the int16 profile is faster (SW-LG 3.71 -> 3.42 ms, NW-AG 4.16 -> 3.87;
    // profiles/r04_score_k.txt).  GSA_KROW_Q8=0 / 2: int16 / int8 always
    const int q8env = env_int(ctx, "GSA_KROW_Q8", 1);
    a.q8 = (q8env != 0 && (q8env == 2 || scoreK == 4) && gsa::krow_score_lds_bytes(substsz, true) <= (size_t)ctx->lds_max) ? 1 : 0;
    a.q8flag = ctx->ctl + 2;
    if ((e = krow ? gsa::launch_krow_score(a, mode, scoreK, grid, st) : gsa::launch_strip_fill(a, mode, grid, st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    note_launch(ctx);
    {
        gsa_launch_info& li = new_launch_info(ctx, krow ? GSA_LAUNCH_SCORE_KROW : GSA_LAUNCH_SCORE_STRIP, st, a.epoch);
        li.ns = a.ns;
        li.k = krow ? scoreK : 1;
        li.q8 = krow ? a.q8 : 0;
        li.npairs = 1;
        li.tickets = tickets;
    }
    (void)hipEventRecord(ctx->ev1, st);
    unsigned long long res[4] = {0, 0, 0, 0};
    if ((e = hipMemcpyAsync(res, sctl, sizeof(res), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    const unsigned err = (unsigned)res[3];
    (void)hipEventElapsedTime(&out->calc_kernel_ms, ctx->ev0, ctx->ev1);
    out->calc_kernel_ms += bidiMs;  // (a local pair back from both ends: both launches)
    // a substitution value outside int16 after the shift: the int32 row scan computes it.  Bit 2 alone
    // from the K-rows kernel (every workgroup checks the whole table and claims no ticket); the strip
    // kernel's waves check the table rows of their own letters, and a wave that meets the raised flag
    // in a wait gives up with bit 1 as well: with bit 2 set that is no failure of its own
    if (err & 2u) return kScoreTooLarge;
    if (err != 0) return GSA_ERROR_KERNEL_FAILURE;
    if (local)
    {
        if (res[0] & 1u) return kScoreTooLarge;  // a score >= 2^26: the caller takes the row scan
        // max key: score << idxBits | (2^idxBits-1 - row-major index); 0 = no positive cell -> (0, 0, 0)
        const int bits = sw_idx_bits(R, C);
        const unsigned long long mask = (1ull << bits) - 1;
        const unsigned long long idx = res[1] ? mask - (res[1] & mask) : 0;
        out->score = (int32_t)(res[1] >> bits);
        out->i_end = (int64_t)(idx / (unsigned long long)(C + 1));
        out->j_end = (int64_t)(idx % (unsigned long long)(C + 1));
        return GSA_SUCCESS;
    }
    out->score = (int32_t)(uint32_t)res[0];
    out->i_end = R;
    out->j_end = C;
    return GSA_SUCCESS;
}

}  // namespace

namespace {

// Largest |substitution value| (>= 1) of a host table.
long long subst_absmax(const int32_t* sub, int32_t substsz)
{
    long long smax = 1;
    for (size_t k = 0; k < (size_t)substsz * (size_t)substsz; ++k)
        smax = std::max<long long>(smax, sub[k] < 0 ? -(long long)sub[k] : (long long)sub[k]);
    return smax;
}

// Value ranges of one pair (R, C >= 1), smax the largest |substitution value|, which bounds every
// score and shifted value: errorInvalidValue when no kernel holds the pair; *stripOk: the strip /
// K-rows score kernels do (else the row scan).
int score_ranges(int64_t R, int64_t C, long long smax, int32_t gapo, int32_t gape, int32_t local, bool* stripOk)
{
    const long long span = (R + C) * (long long)(-gape) + (long long)(gape - gapo) + smax;
    // unshifted int32 (row scan, lane kernels): |H| <= B = smax*min(R,C) + |go| + (R+C)|ge|, by the path
    // of min(i,j) diagonal steps and one gap; every sum of two values then stays inside int32
    const long long B = smax * std::min(R, C) + (long long)(-gapo) + (R + C) * (long long)(-gape);
    if (B >= (1ll << 30)) return GSA_ERROR_INVALID_VALUE;
    // Global modes: the kernels stand in for minus infinity with NEG = -2^29 (E left of column 1, F
    // above row 1, the cells before the matrix), and E = max(E_left + ge, H_left + go) is right only
    // while the true term wins: a value that comes from NEG is at most NEG + ge, a true H + go at
    // least -B + go, so -B - |go| >= -2^29 - |ge| is needed.  Once the first E of a row (F of a column)
    // is the true one, every later one is a maximum over true terms and one term <= NEG + ge, by
    // induction.  Shipped without the |ge| of slack: B + |go| < 2^29.  It holds for the shifted kernels
    // as well (their H' = H - (i+j) ge >= H >= -B, their NEG is the same).  Past it no kernel runs: at
    // -2000010 / -2000000 the same recurrence on the CPU scores a 300 x 10 pair -538870873 where
    // -579999935 is right (tests/test_exact_reference.py).
    // Local modes are left at B < 2^30: H >= 0 there, a value from NEG is negative wherever it stands
    // (NEG + (R+C) ge > -2^31), so it can only replace a true E or F that is negative too, and both
    // lose against the clamp (tests/test_gpu_value_ranges.py runs them at the same gap costs).
    if (!local && B + (long long)(-gapo) >= (1ll << 29)) return GSA_ERROR_INVALID_VALUE;
    const int bits = sw_idx_bits(R, C);
    const long long scoreBound = std::min<long long>((1ll << 31) - 1, smax * std::min(R, C));
    const int scoreBits = scoreBound > 0 ? 64 - __builtin_clzll((unsigned long long)scoreBound) : 1;
    // SW end-cell keys (score << bits | ~index) must fit 64 bits: the row scan packs full scores
    if (local && bits + scoreBits > 63) return GSA_ERROR_INVALID_VALUE;
    // the strip kernel's SW mode needs go < 0 (cells past C then never tie the maximum) and scores
    // below 2^26 packed with bits index bits (it reports larger ones); both modes keep shifted
    // values (i+j)*ge apart within int32 with margin; otherwise the row scan
    // (and scores below 2^26 by construction, so that no shifted key can wrap before the kernel flags it)
    *stripOk = (!local || (gapo < 0 && bits + 27 <= 63 && smax * std::min(R, C) < (1ll << 26))) && span < (1ll << 28);
    return GSA_SUCCESS;
}

// gsa_score_dev; smax < 0: read the table back from the device (in stream order, so the caller's
// writes to it are seen) to find the largest |value|; gsa_score passes it from its host copy.
int score_dev_impl(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                   const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int32_t local,
                   gsa_score_result* out, hipStream_t st, long long smax)
{
    if (!ctx || !seqY || !seqX || !subst || !out) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0 (nw_scan.hip)
    const int64_t R = adjrows - 1, C = adjcols - 1;
    out->calc_kernel_ms = 0.f;
    if (R == 0 || C == 0)
    {
        // one boundary: nothing to fill (score_oracle.c semantics)
        const int64_t k = R + C;
        out->score = (local || k == 0) ? 0 : (int32_t)(gapo + (k - 1) * gape);
        out->i_end = local ? 0 : R;
        out->j_end = local ? 0 : C;
        return GSA_SUCCESS;
    }
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    // value ranges: the largest |substitution value| bounds every score and shifted value
    if (smax < 0)
    {
        std::vector<int32_t> sub((size_t)substsz * (size_t)substsz);
        if ((e = hipMemcpyAsync(sub.data(), subst, sub.size() * 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        smax = subst_absmax(sub.data(), substsz);
    }
    bool stripOk = false;
    if ((s = score_ranges(R, C, smax, gapo, gape, local, &stripOk)) != GSA_SUCCESS) return s;
    if (!score_scan_forced(ctx) && stripOk)
    {
        s = score_ag_strip(ctx, seqY, R, seqX, C, subst, substsz, gapo, gape, local, out, st);
        if (s != kScoreTooLarge) return s;
    }
    const int64_t nTR = (R + 63) / 64;
    const size_t bnd = (size_t)(nTR + 1) * (size_t)(C + 1);
    const size_t need = 2 * bnd + (size_t)(nTR + 1);  // bh, bf, prog
    if ((s = reserve_hard(ctx, ctx->buf[kBufSbnd], need * sizeof(int))) != GSA_SUCCESS ||
        (s = reserve_hard(ctx, ctx->buf[kBufSctl], 64)) != GSA_SUCCESS)
        return s;
    int* const sbnd = ctx->buf[kBufSbnd].as<int>();
    unsigned long long* const sctl = ctx->buf[kBufSctl].as<unsigned long long>();
    gsa::ScoreArgs a {};
    a.seqY = seqY;
    a.seqX = seqX;
    a.subst = subst;
    a.substsz = substsz;
    a.go = gapo;
    a.ge = gape;
    a.R = R;
    a.C = C;
    a.nTR = (int)nTR;
    a.bh = sbnd;
    a.bf = sbnd + bnd;
    a.prog = sbnd + 2 * bnd;
    a.ticket = (unsigned*)sctl;
    a.err = (unsigned*)sctl + 1;
    a.spin = ctx->spin_ticks;
    a.best = sctl + 1;
    a.idxBits = sw_idx_bits(R, C);
    a.result = (int*)(sctl + 2);
    if ((e = hipMemsetAsync(a.prog, 0, (size_t)(nTR + 1) * sizeof(int), st)) != hipSuccess ||
        (e = hipMemsetAsync(sctl, 0, 64, st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    (void)hipEventRecord(ctx->ev0, st);
    if ((e = gsa::launch_score_scan(a, local, ctx->cu_count, st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    {
        gsa_launch_info& li = new_launch_info(ctx, GSA_LAUNCH_SCORE_SCAN, st, 0);
        li.k = 1;
        li.npairs = 1;
    }
    (void)hipEventRecord(ctx->ev1, st);
    unsigned long long ctl[3];
    if ((e = hipMemcpyAsync(ctl, sctl, sizeof(ctl), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    (void)hipEventElapsedTime(&out->calc_kernel_ms, ctx->ev0, ctx->ev1);
    if ((unsigned)(ctl[0] >> 32) != 0) return GSA_ERROR_KERNEL_FAILURE;  // a wait gave up
    if (local)
    {
        const int bits = sw_idx_bits(R, C);
        const unsigned long long mask = (1ull << bits) - 1;
        const unsigned long long idx = mask - (ctl[1] & mask);
        out->score = (int32_t)(ctl[1] >> bits);
        out->i_end = (int64_t)(idx / (unsigned long long)(C + 1));
        out->j_end = (int64_t)(idx % (unsigned long long)(C + 1));
    }
    else
    {
        out->score = (int32_t)(uint32_t)ctl[2];
        out->i_end = R;
        out->j_end = C;
    }
    return GSA_SUCCESS;
}

// gsa_score_batch_dev: the pairs the K-rows score kernel holds in one persistent launch (their
// tickets in one ticket space, two result words per pair, decoded on the device), the others -- and
// those the kernel flags -- one by one through score_dev_impl.
// What score_batch_impl's launch ran (gsa_align_batch_dev reads the checkpoint rows it left in
// kBufGran: pair p's row t at granOff[p] + t gran_stride(C), the affine second array granTotal words
// behind).
struct BatchScoreRoute
{
    int K = 0;                       // rows per lane of the K-rows launch; 0: nothing was launched
    long long granTotal = 0;         // words of the first array, over all pairs
    std::vector<char> inBatch;       // per pair of the call: it ran in that launch and came back unflagged
    std::vector<int> tickets;        // its tickets there
    std::vector<long long> granOff;  // its first row, in words
};

// route (may be null): what the launch ran; the pairs that did not run in it or came back flagged are
// then left unscored (inBatch 0), so that nothing overwrites kBufGran before the caller has read it
int score_batch_impl(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                     int32_t gapo, int32_t gape, int32_t local, gsa_score_result* out, float* batch_ms, hipStream_t st,
                     BatchScoreRoute* route = nullptr)
{
    if (!ctx || !pairs || !subst || !out || npairs < 1) return GSA_ERROR_INVALID_VALUE;
    if (substsz < 1 || substsz > 32) return GSA_ERROR_INVALID_VALUE;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    for (int p = 0; p < npairs; ++p)
        if (pairs[p].adjrows < 1 || pairs[p].adjcols < 1 || !pairs[p].seqY || !pairs[p].seqX) return GSA_ERROR_INVALID_VALUE;
    if (batch_ms) *batch_ms = 0.f;
    if (route)
    {
        *route = BatchScoreRoute {};
        route->inBatch.assign((size_t)npairs, 0);
        route->tickets.assign((size_t)npairs, 0);
        route->granOff.assign((size_t)npairs, 0);
    }
    // empty pairs: one boundary, nothing to fill (score_dev_impl)
    std::vector<int> work;
    for (int p = 0; p < npairs; ++p)
    {
        const int64_t R = pairs[p].adjrows - 1, C = pairs[p].adjcols - 1;
        out[p].calc_kernel_ms = 0.f;
        if (R == 0 || C == 0)
        {
            const int64_t k = R + C;
            out[p].score = (local || k == 0) ? 0 : (int32_t)(gapo + (k - 1) * gape);
            out[p].i_end = local ? 0 : R;
            out[p].j_end = local ? 0 : C;
        }
        else
            work.push_back(p);
    }
    // the K-rows score kernel, under score_ag_strip's conditions for it (else every pair alone)
    const bool krow = !score_scan_forced(ctx) && score_kernel_krow(ctx) && gsa::krow_score_lds_bytes(substsz) <= ctx->lds_max;
    const int kenv = env_int(ctx, "GSA_SCORE_K", 0);
    // rows per lane: 4 in every mode.  A single pair's rule (score_ag_strip: 2 for SW and affine gaps)
    // shortens its critical path; a batch fills the chip either way, and the longer strip's smaller
    // share of hand-off wins: 512 pairs of 18-22k, SW-LG 62.5 -> 47.6 ms, NW-AG 68.4 -> 49.7 ms,
    // NW-LG 54.1 -> 29.3 ms (profiles/score_batch_ab.txt).  GSA_SCORE_K = 2 / 4 forces one
    const int scoreK = kenv == 2 ? 2 : 4;
    if (work.empty())
    {
        if (krow)
        {
            gsa_launch_info& li = new_launch_info(ctx, GSA_LAUNCH_SCORE_KROW, st, 0);  // nothing to launch
            li.ns = gsa::kSparseNS;
            li.k = scoreK;
            li.npairs = npairs;
        }
        return GSA_SUCCESS;
    }
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    long long smax;
    {
        std::vector<int32_t> sub((size_t)substsz * (size_t)substsz);
        if ((e = hipMemcpyAsync(sub.data(), subst, sub.size() * 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        smax = subst_absmax(sub.data(), substsz);
    }
    // the batch's pairs (bp: indices into pairs) and those that run alone
    const int64_t TR = (int64_t)(64 * scoreK) * gsa::kSparseNS;
    std::vector<int> bp, alone;
    std::vector<gsa::PairDesc> hd;
    long long tickets = 0, gran = 0;
    for (int p : work)
    {
        const int64_t R = pairs[p].adjrows - 1, C = pairs[p].adjcols - 1;
        bool stripOk = false;
        int s = score_ranges(R, C, smax, gapo, gape, local, &stripOk);
        if (s != GSA_SUCCESS) return s;
        if (!krow || !stripOk)
        {
            alone.push_back(p);
            continue;
        }
        gsa::PairDesc d;
        std::memset(&d, 0, sizeof(d));
        d.seqY = pairs[p].seqY;
        d.seqX = pairs[p].seqX;
        d.R = (int)R;
        d.C = (int)C;
        d.Cp = (int)C;
        d.nTickets = (int)((R + TR - 1) / TR);
        d.ticketBase = (int)tickets;
        d.granOff = gran;
        tickets += d.nTickets;
        gran += (long long)d.nTickets * gsa::gran_stride(d.Cp);
        if (tickets > (1ll << 30) || C > (1ll << 30)) return GSA_ERROR_INVALID_VALUE;
        bp.push_back(p);
        hd.push_back(d);
    }
    float ms = 0.f;
    if (!bp.empty())
    {
        const int nb = (int)bp.size();
        const std::vector<int> sched = batch_schedule(ctx, hd, tickets);
        int s = stage_descs(ctx, hd, sched, st);
        if (s != GSA_SUCCESS) return s;
        if ((s = ensure_gran(ctx, 2 * (size_t)gran, st)) != GSA_SUCCESS) return s;
        if ((s = reserve_hard(ctx, ctx->buf[kBufSctl], 64)) != GSA_SUCCESS) return s;
        // two result words per pair, then the decoded answers and the error word's
        const size_t resBytes = (size_t)nb * 2 * sizeof(unsigned long long);
        const size_t outBytes = ((size_t)nb + 1) * sizeof(gsa::ScoreOut);
        if ((s = reserve_hard(ctx, ctx->buf[kBufSbatch], resBytes + outBytes, 4096)) != GSA_SUCCESS) return s;
        gsa::PairDesc* const ddesc = ctx->buf[kBufDesc].as<gsa::PairDesc>();
        unsigned long long* const dgran = ctx->buf[kBufGran].as<unsigned long long>();
        unsigned long long* const sctl = ctx->buf[kBufSctl].as<unsigned long long>();
        unsigned long long* const res = ctx->buf[kBufSbatch].as<unsigned long long>();
        gsa::ScoreOut* const dout = (gsa::ScoreOut*)(ctx->buf[kBufSbatch].as<char>() + resBytes);
        gsa::StripArgs a;
        std::memset(&a, 0, sizeof(a));
        a.subst = subst;
        a.substsz = substsz;
        a.g = gapo;
        a.go = gapo;
        a.ge = gape;
        a.ns = gsa::kSparseNS;
        a.pairs = ddesc;
        a.nPairs = nb;
        a.nTicketsTotal = (int)tickets;
        a.sched = sched.empty() ? nullptr : (const int*)(ddesc + nb);
        a.gran = dgran;
        a.gran2 = dgran + gran;
        a.ticket = ctx->ctl;
        a.err = (unsigned*)(sctl + 3);  // the score kernels' own error word (score_ag_strip)
        a.spin = ctx->spin_ticks;
        a.swBest = res;  // a batch: the base of the pairs' result words
        if (nb == 1)
        {
            // one pair left: the kernel's single-pair form, its words laid out as a batch's pair 0
            a.agResult = (int*)res;
            a.swBest = res + 1;
            a.idxBits = sw_idx_bits(hd[0].R, hd[0].C);
        }
        a.epoch = ++ctx->epoch;
        if (a.epoch == 0) a.epoch = ++ctx->epoch;
        if ((e = hipMemsetAsync(ctx->ctl, 0, 4, st)) != hipSuccess || (e = hipMemsetAsync(sctl, 0, 32, st)) != hipSuccess ||
            (e = hipMemsetAsync(res, 0, resBytes, st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        (void)hipEventRecord(ctx->ev0, st);
        const int mode = local ? (gapo == gape ? gsa::kModeScoreSWL : gsa::kModeScoreSW)
                               : (gapo == gape ? gsa::kModeScoreAGL : gsa::kModeScoreAG);
        // the int8 column profile for NW-LG only: at 4 rows per lane it gains there (512 pairs: 31.5 ->
        // 29.1 ms), costs NW-AG (49.5 -> 54.3 ms) and leaves SW-LG where it is (47.3 / 47.2;
        // profiles/score_batch_ab.txt).  GSA_KROW_Q8=0 / 2: int16 / int8 always
        const int q8env = env_int(ctx, "GSA_KROW_Q8", 1);
        a.q8 = (q8env != 0 && (q8env == 2 || mode == gsa::kModeScoreAGL) &&
                gsa::krow_score_lds_bytes(substsz, true) <= (size_t)ctx->lds_max) ? 1 : 0;
        a.q8flag = ctx->ctl + 2;
        // one pair: one workgroup per CU (its tickets are a chain); a batch: all resident slots
        const int grid = nb == 1 ? std::max(1, std::min((int)tickets, ctx->cu_count)) : 0;
        if ((e = gsa::launch_krow_score(a, mode, scoreK, grid, st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        note_launch(ctx);
        if ((e = gsa::launch_score_finalize(ddesc, nb, res, a.err, local != 0, dout, st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        {
            gsa_launch_info& li = new_launch_info(ctx, GSA_LAUNCH_SCORE_KROW, st, a.epoch);
            li.ns = a.ns;
            li.k = scoreK;
            li.q8 = a.q8;
            li.npairs = npairs;
            li.pair_major = (nb > 1 && sched.empty()) ? 1 : 0;
            li.tickets = tickets;
        }
        (void)hipEventRecord(ctx->ev1, st);
        std::vector<gsa::ScoreOut> ho((size_t)nb + 1);
        if ((e = hipMemcpyAsync(ho.data(), dout, outBytes, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
        const unsigned err = (unsigned)ho[(size_t)nb].score;
        if (err != 0 && err != 2u) return GSA_ERROR_KERNEL_FAILURE;
        for (int i = 0; i < nb; ++i)
        {
            const gsa::ScoreOut& o = ho[(size_t)i];
            // a table outside int16 after the shift (every pair), or a pair's score >= 2^26: alone
            if (err == 2u || o.status != 0)
            {
                alone.push_back(bp[(size_t)i]);
                continue;
            }
            gsa_score_result& r = out[bp[(size_t)i]];
            r.score = o.score;
            r.i_end = o.i_end;
            r.j_end = o.j_end;
            if (route)
            {
                route->inBatch[(size_t)bp[(size_t)i]] = 1;
                route->tickets[(size_t)bp[(size_t)i]] = hd[(size_t)i].nTickets;
                route->granOff[(size_t)bp[(size_t)i]] = hd[(size_t)i].granOff;
            }
        }
        if (route)
        {
            route->K = scoreK;
            route->granTotal = gran;
        }
    }
    if (route) alone.clear();
    for (int p : alone)
    {
        int s = score_dev_impl(ctx, pairs[p].seqY, pairs[p].adjrows, pairs[p].seqX, pairs[p].adjcols, subst, substsz, gapo,
                               gape, local, &out[p], st, smax);
        if (s != GSA_SUCCESS) return s;
        ms += out[p].calc_kernel_ms;
        out[p].calc_kernel_ms = 0.f;
    }
    if (batch_ms) *batch_ms = ms;
    return GSA_SUCCESS;
}

// Longest subject the database search sends to the lane kernel (GSA_DB_MAXC overrides it): the largest
// length of the sweep of tools/score_db_bench.py at which that kernel still beat the batched K-rows
// path in all three modes (profiles/score_db_ab.txt).  Measured: it won at every swept
// length, 64 ... 4096 (1.4-1.9x), so this is the sweep's upper end, not a crossover.
constexpr int kDbLanesLmax = 4096;

// gsa_score_db_dev: empty pairs on the host, the subjects the lane kernel does not take through
// score_batch_impl (first, so that gsa_last_launch reports the lane launch), the others, longest
// first, four to a wave task in one launch of nw_lanes.hip.
int score_db_impl(gsa_ctx* ctx, const int32_t* query, int32_t adjq, const int32_t* db, const int64_t* db_off,
                  int32_t nsubj, const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int32_t local,
                  gsa_score_result* out, float* kernel_ms, hipStream_t st)
{
    if (!ctx || !query || !db || !db_off || !subst || !out) return GSA_ERROR_INVALID_VALUE;
    if (nsubj < 1 || adjq < 1) return GSA_ERROR_INVALID_VALUE;
    if (substsz < 1 || substsz > 32) return GSA_ERROR_INVALID_VALUE;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    if (db_off[0] < 0) return GSA_ERROR_INVALID_VALUE;
    for (int s = 0; s < nsubj; ++s)
        if (db_off[s + 1] <= db_off[s] || db_off[s + 1] - db_off[s] > (int64_t)INT32_MAX) return GSA_ERROR_INVALID_VALUE;
    if (kernel_ms) *kernel_ms = 0.f;
    auto pair_of = [&](int s) {
        gsa_pair_dev p;
        std::memset(&p, 0, sizeof(p));
        p.seqY = query;
        p.adjrows = adjq;
        p.seqX = db + db_off[s];
        p.adjcols = (int32_t)(db_off[s + 1] - db_off[s]);
        return p;
    };
    if (env_int(ctx, "GSA_DB_LANES", 1) == 0)
    {
        std::vector<gsa_pair_dev> pairs((size_t)nsubj);
        for (int s = 0; s < nsubj; ++s) pairs[(size_t)s] = pair_of(s);
        return score_batch_impl(ctx, nsubj, pairs.data(), subst, substsz, gapo, gape, local, out, kernel_ms, st);
    }
    const int64_t R = adjq - 1;
    // empty pairs: one boundary, nothing to fill (score_batch_impl's rule)
    std::vector<int> work;
    for (int s = 0; s < nsubj; ++s)
    {
        const int64_t C = db_off[s + 1] - db_off[s] - 1;
        out[s].calc_kernel_ms = 0.f;
        if (R == 0 || C == 0)
        {
            const int64_t k = R + C;
            out[s].score = (local || k == 0) ? 0 : (int32_t)(gapo + (k - 1) * gape);
            out[s].i_end = local ? 0 : R;
            out[s].j_end = local ? 0 : C;
        }
        else
            work.push_back(s);
    }
    if (work.empty()) return GSA_SUCCESS;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    long long smax;
    {
        std::vector<int32_t> sub((size_t)substsz * (size_t)substsz);
        if ((e = hipMemcpyAsync(sub.data(), subst, sub.size() * 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        smax = subst_absmax(sub.data(), substsz);
    }
    const int lmax = std::max(0, std::min(env_int(ctx, "GSA_DB_MAXC", kDbLanesLmax), gsa::kDbLanesMaxC));
    // the query's profile must fit LDS (else every subject takes the other path)
    const bool fits = R < (1 << 20) && gsa::dblanes_lds_bytes((int)R, substsz) <= (size_t)ctx->lds_max;
    std::vector<int> lanes, other;
    for (int s : work)
    {
        const int64_t C = db_off[s + 1] - db_off[s] - 1;
        bool stripOk = false;
        int st2 = score_ranges(R, C, smax, gapo, gape, local, &stripOk);
        if (st2 != GSA_SUCCESS) return st2;
        // local: a row's best key packs the score above 13 column bits
        const bool keyOk = !local || smax * std::min(R, C) < gsa::kDbLanesMaxScore;
        (fits && C <= lmax && keyOk ? lanes : other).push_back(s);
    }
    float ms = 0.f;
    if (!other.empty())
    {
        std::vector<gsa_pair_dev> pairs(other.size());
        std::vector<gsa_score_result> res(other.size());
        for (size_t k = 0; k < other.size(); ++k) pairs[k] = pair_of(other[k]);
        int s = score_batch_impl(ctx, (int32_t)other.size(), pairs.data(), subst, substsz, gapo, gape, local, res.data(),
                                 &ms, st);
        if (s != GSA_SUCCESS) return s;
        for (size_t k = 0; k < other.size(); ++k) out[other[k]] = res[k];
    }
    if (!lanes.empty())
    {
        // longest first: a task's four subjects are of like length, and the long tasks start first
        std::stable_sort(lanes.begin(), lanes.end(), [&](int x, int y) {
            return db_off[x + 1] - db_off[x] > db_off[y + 1] - db_off[y];
        });
        const size_t n = lanes.size();
        const int ntasks = (int)((n + gsa::kDbLanesSubj - 1) / gsa::kDbLanesSubj);
        const int cmax = (int)(db_off[lanes[0] + 1] - db_off[lanes[0]] - 1);
        const int passes = (int)((R + gsa::kDbLanesPassRows - 1) / gsa::kDbLanesPassRows);
        std::vector<long long> hoff(n);
        std::vector<int> hlen(n);
        for (size_t k = 0; k < n; ++k)
        {
            hoff[k] = (long long)db_off[lanes[k]];
            hlen[k] = (int)(db_off[lanes[k] + 1] - db_off[lanes[k]] - 1);
        }
        // [counter, 64 B][offsets][lengths][results]
        const size_t offAt = 64, lenAt = offAt + n * 8, outAt = (lenAt + n * 4 + 15) / 16 * 16;
        const size_t bytes = outAt + n * sizeof(gsa::DbLanesOut);
        int s = reserve_hard(ctx, ctx->buf[kBufDbl], bytes, 4096);
        if (s != GSA_SUCCESS) return s;
        int wgs = 1;
        if ((e = gsa::dblanes_resident((int)R, substsz, local, gapo != gape, &wgs)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        const int grid = std::max(1, std::min(wgs, (ntasks + gsa::kDbLanesWaves - 1) / gsa::kDbLanesWaves));
        const int bndStride = cmax + 1;
        if (passes > 1)
        {
            // per resident wave and subject slot, (H, F) by column: bounded by the waves, not the database
            const size_t bb = (size_t)grid * gsa::kDbLanesWaves * gsa::kDbLanesSubj * (size_t)bndStride * sizeof(int2);
            if ((s = reserve_hard(ctx, ctx->buf[kBufDbbnd], bb, 4096)) != GSA_SUCCESS) return s;
        }
        char* const base = ctx->buf[kBufDbl].as<char>();
        gsa::DbLanesArgs a;
        std::memset(&a, 0, sizeof(a));
        a.query = query;
        a.db = db;
        a.subst = subst;
        a.substsz = substsz;
        a.go = gapo;
        a.ge = gape;
        a.R = (int)R;
        a.passes = passes;
        a.nsubj = (int)n;
        a.ntasks = ntasks;
        a.off = (const long long*)(base + offAt);
        a.len = (const int*)(base + lenAt);
        a.out = (gsa::DbLanesOut*)(base + outAt);
        a.counter = (unsigned*)base;
        a.bnd = passes > 1 ? ctx->buf[kBufDbbnd].as<int2>() : nullptr;
        a.bndStride = bndStride;
        if ((e = hipMemsetAsync(base, 0, 64, st)) != hipSuccess ||
            (e = hipMemcpyAsync(base + offAt, hoff.data(), n * 8, hipMemcpyHostToDevice, st)) != hipSuccess ||
            (e = hipMemcpyAsync(base + lenAt, hlen.data(), n * 4, hipMemcpyHostToDevice, st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        (void)hipEventRecord(ctx->ev0, st);
        if ((e = gsa::launch_dblanes(a, local, grid, nullptr, st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        (void)hipEventRecord(ctx->ev1, st);
        note_launch(ctx);
        {
            gsa_launch_info& li = new_launch_info(ctx, GSA_LAUNCH_SCORE_LANES, st, 0);
            li.ns = gsa::kDbLanesWaves;
            li.k = gsa::kDbLanesKQ;
            li.npairs = (int32_t)n;
            li.tickets = ntasks;
        }
        std::vector<gsa::DbLanesOut> ho(n);
        if ((e = hipMemcpyAsync(ho.data(), a.out, n * sizeof(gsa::DbLanesOut), hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        float lms = 0.f;
        (void)hipEventElapsedTime(&lms, ctx->ev0, ctx->ev1);
        ms += lms;
        for (size_t k = 0; k < n; ++k)
        {
            gsa_score_result& r = out[lanes[k]];
            r.score = ho[k].score;
            r.i_end = ho[k].i_end;
            r.j_end = ho[k].j_end;
            r.calc_kernel_ms = 0.f;
        }
    }
    if (kernel_ms) *kernel_ms = ms;
    return GSA_SUCCESS;
}

// gsa_last_launch's record, put back when the scope ends: the calls that report through an info
// struct of their own leave it as it was, also when they run other entry points' paths.
struct KeepLaunchRecord
{
    gsa_ctx* ctx;
    gsa_launch_info ll;
    hipStream_t st;
    unsigned e0, e1;
    explicit KeepLaunchRecord(gsa_ctx* c) : ctx(c), ll(c->ll), st(c->ll_stream), e0(c->ll_epoch0), e1(c->ll_epoch) {}
    ~KeepLaunchRecord()
    {
        ctx->ll = ll;
        ctx->ll_stream = st;
        ctx->ll_epoch0 = e0;
        ctx->ll_epoch = e1;
    }
};

// Default of gsa_align_db_dev's scratch_limit: bytes of move codes a call holds at once.
constexpr int64_t kAlignDbScratch = 256ll << 20;

// The move bytes of a walk (last move first) as a CIGAR: forward order, run-length encoded.
std::string fold_cigar(const unsigned char* mv, int64_t n)
{
    std::string s;
    for (int64_t k = n - 1; k >= 0;)
    {
        const unsigned char op = mv[k];
        int64_t run = 0;
        while (k >= 0 && mv[k] == op)
        {
            ++run;
            --k;
        }
        char dig[24];
        int nd = 0;
        for (int64_t v = run; v > 0; v /= 10) dig[nd++] = (char)('0' + v % 10);
        while (nd > 0) s += dig[--nd];
        s += (char)op;
    }
    return s;
}

// The CIGARs of the n results with status 0 into the caller's buffer, back to back in order, each with
// its terminator; one that does not fit gets status 2.  A string's offset does not depend on the
// buffer's size.  Returns the bytes all of them take (*cigar_need).
int64_t pack_cigars(gsa_align_db_result* res, const std::string* cig, int64_t n, char* cigar, int64_t cigar_cap)
{
    int64_t at = 0;
    for (int64_t k = 0; k < n; ++k)
    {
        gsa_align_db_result& r = res[k];
        if (r.status != 0) continue;
        const int64_t len = (int64_t)cig[k].size();
        if (at + len + 1 <= cigar_cap)
        {
            std::memcpy(cigar + at, cig[k].c_str(), (size_t)len + 1);
            r.cigar_off = at;
            r.cigar_len = len;
        }
        else
            r.status = 2;
        at += len + 1;
    }
    return at;
}

// The three events a fill launch and a walk launch are timed with (the launchers record them), made on
// first use.
int ensure_trace_events(gsa_ctx* ctx)
{
    for (hipEvent_t& ev : ctx->adbev)
    {
        const hipError_t e = ev ? hipSuccess : hipEventCreate(&ev);
        if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    }
    return GSA_SUCCESS;
}

// Adds the times of the fill and of the walk those events were last recorded around.
void add_trace_ms(const gsa_ctx* ctx, float* fill_ms, float* walk_ms)
{
    float m0 = 0.f, m1 = 0.f;
    (void)hipEventElapsedTime(&m0, ctx->adbev[0], ctx->adbev[1]);
    (void)hipEventElapsedTime(&m1, ctx->adbev[1], ctx->adbev[2]);
    *fill_ms += m0;
    *walk_ms += m1;
}

// log2 of the rows a lane's codes hold (KR = 8 or 16): the walks' krShift
int kr_shift(int KR) { return KR == 8 ? 3 : 4; }

// gsa_align_db_dev: hits with an empty side on the host; the hits the trace kernels take, longest
// first, in chunks whose move codes fit scratch_limit, a fill and a walk launch per chunk and one copy
// of the results and move bytes back (nw_lanes_trace.hip); the others (status 1) through
// score_batch_impl for their score and end cell.  gsa_last_launch's record is left as it was.
int align_db_impl(gsa_ctx* ctx, const int32_t* query, int32_t adjq, const int32_t* db, const int64_t* db_off,
                  int32_t nsubj, const int32_t* hits, int32_t nhits, const int32_t* subst, int32_t substsz,
                  int32_t gapo, int32_t gape, int32_t local, int64_t scratch_limit, gsa_align_db_result* out,
                  char* cigar, int64_t cigar_cap, int64_t* cigar_need, gsa_align_db_info* info, float* kernel_ms,
                  hipStream_t st)
{
    if (!ctx || !query || !db || !db_off || !subst || !out) return GSA_ERROR_INVALID_VALUE;
    if (nsubj < 1 || adjq < 1) return GSA_ERROR_INVALID_VALUE;
    if (substsz < 1 || substsz > 32) return GSA_ERROR_INVALID_VALUE;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    if (nhits < 0 || scratch_limit < 0 || cigar_cap < 0) return GSA_ERROR_INVALID_VALUE;
    if ((nhits > 0 && !hits) || (cigar_cap > 0 && !cigar)) return GSA_ERROR_INVALID_VALUE;
    if (db_off[0] < 0) return GSA_ERROR_INVALID_VALUE;
    for (int s = 0; s < nsubj; ++s)
        if (db_off[s + 1] <= db_off[s] || db_off[s + 1] - db_off[s] > (int64_t)INT32_MAX) return GSA_ERROR_INVALID_VALUE;
    for (int h = 0; h < nhits; ++h)
        if (hits[h] < 0 || hits[h] >= nsubj) return GSA_ERROR_INVALID_VALUE;
    if (kernel_ms) *kernel_ms = 0.f;
    if (cigar_need) *cigar_need = 0;
    gsa_align_db_info inf;
    std::memset(&inf, 0, sizeof(inf));
    if (info) *info = inf;
    const int64_t R = adjq - 1;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    long long smax = 1;
    if (R > 0)
    {
        // gsa_score_db_dev's range test, over the whole database: the same calls are rejected
        std::vector<int32_t> sub((size_t)substsz * (size_t)substsz);
        if ((e = hipMemcpyAsync(sub.data(), subst, sub.size() * 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        smax = subst_absmax(sub.data(), substsz);
        for (int s = 0; s < nsubj; ++s)
        {
            const int64_t C = db_off[s + 1] - db_off[s] - 1;
            bool stripOk = false;
            if (C > 0 && score_ranges(R, C, smax, gapo, gape, local, &stripOk) != GSA_SUCCESS)
                return GSA_ERROR_INVALID_VALUE;
        }
    }
    if (nhits == 0) return GSA_SUCCESS;

    const int64_t limit = scratch_limit > 0 ? scratch_limit : kAlignDbScratch;
    const bool fits = R < (1 << 20) && gsa::dblanes_lds_bytes((int)R, substsz) <= (size_t)ctx->lds_max;
    std::vector<std::string> cig((size_t)nhits);
    std::vector<int> lanes, other;
    for (int h = 0; h < nhits; ++h)
    {
        const int64_t C = db_off[hits[h] + 1] - db_off[hits[h]] - 1;
        gsa_align_db_result& r = out[h];
        std::memset(&r, 0, sizeof(r));
        if (R == 0 || C == 0)
        {
            const int64_t k = R + C;
            if (!local && k > 0)
            {
                r.score = (int32_t)(gapo + (k - 1) * gape);
                r.i_end = R;
                r.j_end = C;
                cig[(size_t)h] = std::to_string(k) + (R > 0 ? 'I' : 'D');
            }
            continue;
        }
        const bool keyOk = !local || smax * std::min(R, C) < gsa::kDbLanesMaxScore;
        // the fill keeps 4 x value + source: |H| <= smax min(R, C) + |go| + (R + C) |ge| (score_ranges' bound)
        const bool valOk = smax * std::min(R, C) + (long long)(-gapo) + (R + C) * (long long)(-gape) < gsa::kDbTraceMaxValue;
        const bool take = fits && C <= gsa::kDbLanesMaxC && keyOk && valOk && gsa::dbtrace_code_bytes(R, C) <= limit;
        (take ? lanes : other).push_back(h);
    }
    auto len_of = [&](int h) { return db_off[hits[h] + 1] - db_off[hits[h]] - 1; };
    float fill_ms = 0.f, walk_ms = 0.f, other_ms = 0.f;
    if (!lanes.empty())
    {
        // longest first: a task's four hits are of like length, and the long tasks start first
        std::stable_sort(lanes.begin(), lanes.end(), [&](int x, int y) { return len_of(x) > len_of(y); });
        // chunks [first, last) whose codes fit the limit; the largest of every buffer over the chunks
        std::vector<std::pair<size_t, size_t>> chunks;
        size_t maxN = 0;
        int64_t maxCodes = 0, maxMoves = 0;
        for (size_t b = 0; b < lanes.size();)
        {
            size_t k = b;
            int64_t cb = 0, mb = 0;
            while (k < lanes.size() && cb + gsa::dbtrace_code_bytes(R, len_of(lanes[k])) <= limit)
            {
                cb += gsa::dbtrace_code_bytes(R, len_of(lanes[k]));
                mb += R + len_of(lanes[k]);
                ++k;
            }
            chunks.emplace_back(b, k);
            maxN = std::max(maxN, k - b);
            maxCodes = std::max(maxCodes, cb);
            maxMoves = std::max(maxMoves, mb);
            b = k;
        }
        const int passes = (int)((R + gsa::kDbLanesPassRows - 1) / gsa::kDbLanesPassRows);
        const int cmax = (int)len_of(lanes[0]);
        int wgs = 1;
        if ((e = gsa::dbtrace_resident((int)R, substsz, local, gapo != gape, &wgs)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        const int maxTasks = (int)((maxN + gsa::kDbLanesSubj - 1) / gsa::kDbLanesSubj);
        const int maxGrid = std::max(1, std::min(wgs, (maxTasks + gsa::kDbLanesWaves - 1) / gsa::kDbLanesWaves));
        // meta: [counter, 64 B][offsets][code offsets][move offsets][lengths][fill results]
        const size_t offAt = 64, coffAt = offAt + maxN * 8, moffAt = coffAt + maxN * 8, lenAt = moffAt + maxN * 8;
        const size_t foutAt = (lenAt + maxN * 4 + 15) / 16 * 16;
        const size_t metaBytes = foutAt + maxN * sizeof(gsa::DbLanesOut);
        // results: [walk results][move bytes]
        const size_t movAt = maxN * sizeof(gsa::DbTraceOut);
        const size_t resBytes = movAt + (size_t)maxMoves;
        int s;
        if ((s = reserve_hard(ctx, ctx->buf[kBufAdbMeta], metaBytes, 4096)) != GSA_SUCCESS ||
            (s = reserve_hard(ctx, ctx->buf[kBufAdbRes], resBytes, 4096)) != GSA_SUCCESS ||
            (s = reserve_hard(ctx, ctx->buf[kBufAdbCodes], (size_t)maxCodes, 4096)) != GSA_SUCCESS)
            return s;
        if (passes > 1)
        {
            const size_t bb = (size_t)maxGrid * gsa::kDbLanesWaves * gsa::kDbLanesSubj * (size_t)(cmax + 1) * sizeof(int2);
            if ((s = reserve_hard(ctx, ctx->buf[kBufDbbnd], bb, 4096)) != GSA_SUCCESS) return s;
        }
        if (const int es = ensure_trace_events(ctx); es != GSA_SUCCESS) return es;
        char* const meta = ctx->buf[kBufAdbMeta].as<char>();
        unsigned char* const adbres = ctx->buf[kBufAdbRes].as<unsigned char>();
        std::vector<char> hmeta(lenAt + maxN * 4), hres(resBytes);
        for (const auto& ch : chunks)
        {
            const size_t n = ch.second - ch.first;
            const int ntasks = (int)((n + gsa::kDbLanesSubj - 1) / gsa::kDbLanesSubj);
            const int grid = std::max(1, std::min(wgs, (ntasks + gsa::kDbLanesWaves - 1) / gsa::kDbLanesWaves));
            std::memset(hmeta.data(), 0, 64);
            long long* const hoff = (long long*)(hmeta.data() + offAt);
            long long* const hcoff = (long long*)(hmeta.data() + coffAt);
            long long* const hmoff = (long long*)(hmeta.data() + moffAt);
            int* const hlen = (int*)(hmeta.data() + lenAt);
            int64_t cb = 0, mb = 0;
            for (size_t k = 0; k < n; ++k)
            {
                const int h = lanes[ch.first + k];
                hoff[k] = (long long)db_off[hits[h]];
                hlen[k] = (int)len_of(h);
                hcoff[k] = cb;
                hmoff[k] = mb;
                cb += gsa::dbtrace_code_bytes(R, hlen[k]);
                mb += R + hlen[k];
            }
            gsa::DbTraceArgs a;
            std::memset(&a, 0, sizeof(a));
            a.fill.query = query;
            a.fill.db = db;
            a.fill.subst = subst;
            a.fill.substsz = substsz;
            a.fill.go = gapo;
            a.fill.ge = gape;
            a.fill.R = (int)R;
            a.fill.passes = passes;
            a.fill.nsubj = (int)n;
            a.fill.ntasks = ntasks;
            a.fill.off = (const long long*)(meta + offAt);
            a.fill.len = (const int*)(meta + lenAt);
            a.fill.out = (gsa::DbLanesOut*)(meta + foutAt);
            a.fill.counter = (unsigned*)meta;
            a.fill.bnd = passes > 1 ? ctx->buf[kBufDbbnd].as<int2>() : nullptr;
            a.fill.bndStride = cmax + 1;
            a.codes = ctx->buf[kBufAdbCodes].as<unsigned char>();
            a.codeOff = (const long long*)(meta + coffAt);
            a.moveOff = (const long long*)(meta + moffAt);
            a.res = (gsa::DbTraceOut*)adbres;
            a.moves = adbres + movAt;
            a.local = local;
            if ((e = hipMemcpyAsync(meta, hmeta.data(), hmeta.size(), hipMemcpyHostToDevice, st)) != hipSuccess)
                return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
            if ((e = gsa::launch_dbtrace(a, grid, ctx->adbev, st)) != hipSuccess)
                return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
            note_launch(ctx);
            if ((e = hipMemcpyAsync(hres.data(), adbres, movAt + (size_t)mb, hipMemcpyDeviceToHost, st)) != hipSuccess ||
                (e = hipStreamSynchronize(st)) != hipSuccess)
                return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
            add_trace_ms(ctx, &fill_ms, &walk_ms);
            const gsa::DbTraceOut* const ho = (const gsa::DbTraceOut*)hres.data();
            for (size_t k = 0; k < n; ++k)
            {
                const int h = lanes[ch.first + k];
                gsa_align_db_result& r = out[h];
                r.score = ho[k].score;
                r.i_start = ho[k].i_start;
                r.j_start = ho[k].j_start;
                r.i_end = ho[k].i_end;
                r.j_end = ho[k].j_end;
                if (ho[k].moves < 0 || ho[k].moves > R + hlen[k]) return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);
                cig[(size_t)h] = fold_cigar((const unsigned char*)hres.data() + movAt + hmoff[k], ho[k].moves);
            }
            inf.chunks += 1;
            inf.tasks += ntasks;
            inf.code_bytes = std::max<int64_t>(inf.code_bytes, cb);
        }
        inf.lane_hits = (int32_t)lanes.size();
    }
    if (!other.empty())
    {
        // score and end cell from the score path; its launch record is not this call's to leave
        const KeepLaunchRecord keep(ctx);
        std::vector<gsa_pair_dev> pairs(other.size());
        std::vector<gsa_score_result> res(other.size());
        for (size_t k = 0; k < other.size(); ++k)
        {
            gsa_pair_dev& p = pairs[k];
            std::memset(&p, 0, sizeof(p));
            p.seqY = query;
            p.adjrows = adjq;
            p.seqX = db + db_off[hits[other[k]]];
            p.adjcols = (int32_t)(len_of(other[k]) + 1);
        }
        const int s = score_batch_impl(ctx, (int32_t)other.size(), pairs.data(), subst, substsz, gapo, gape, local,
                                       res.data(), &other_ms, st);
        if (s != GSA_SUCCESS) return s;
        for (size_t k = 0; k < other.size(); ++k)
        {
            gsa_align_db_result& r = out[other[k]];
            r.score = res[k].score;
            r.i_end = res[k].i_end;
            r.j_end = res[k].j_end;
            r.status = 1;
        }
        inf.unsupported = (int32_t)other.size();
    }
    // the strings back to back in hit order
    const int64_t at = pack_cigars(out, cig.data(), nhits, cigar, cigar_cap);
    if (cigar_need) *cigar_need = at;
    inf.fill_ms = fill_ms;
    inf.walk_ms = walk_ms;
    if (info) *info = inf;
    if (kernel_ms) *kernel_ms = fill_ms + walk_ms + other_ms;
    return GSA_SUCCESS;
}

// The semi-global calls have the lane kernels and no second path: a pair of R query
// and C subject letters (both >= 1) is taken iff the subject is within the kernels' column range, the
// query's profile fits the LDS a workgroup may have, and the value bound B stays below 2^18, which
// covers the signed result key and the trace fill's 4 v + tag.  All three grow with R and with C, so
// the longest query against the longest subject fails them iff any pair does.
int semi_ranges(const gsa_ctx* ctx, int64_t R, int64_t C, long long smax, int32_t substsz, int32_t gapo, int32_t gape)
{
    if (C > gsa::kDbLanesMaxC) return GSA_ERROR_INVALID_VALUE;
    if (R >= (1 << 20) || gsa::dblanes_lds_bytes((int)R, substsz) > (size_t)ctx->lds_max) return GSA_ERROR_INVALID_VALUE;
    const long long B = smax * std::min(R, C) - (long long)gapo - (R + C) * (long long)gape;
    if (B >= gsa::kDbSemiMaxValue) return GSA_ERROR_INVALID_VALUE;
    return GSA_SUCCESS;
}

// The alignment shape of a database call: the two old modes (global or local, by `local`), semi-global
//  or overlap (2.2o).  The last two have the lane kernels and no second path.
enum class DbShape
{
    plain,
    semi,
    overlap
};

// The overlap calls: semi_ranges' three tests, and a query of at most 8191 letters,
// because the end cell's row travels in a key beside the value as its column does (with a small table
// the LDS test alone lets longer queries through).  All grow with R and with C.
int overlap_ranges(const gsa_ctx* ctx, int64_t R, int64_t C, long long smax, int32_t substsz, int32_t gapo, int32_t gape)
{
    if (R > gsa::kDbOverlapMaxR) return GSA_ERROR_INVALID_VALUE;
    return semi_ranges(ctx, R, C, smax, substsz, gapo, gape);
}

int lane_only_ranges(DbShape shape, const gsa_ctx* ctx, int64_t R, int64_t C, long long smax, int32_t substsz, int32_t gapo,
                     int32_t gape)
{
    return shape == DbShape::overlap ? overlap_ranges(ctx, R, C, smax, substsz, gapo, gape)
                                     : semi_ranges(ctx, R, C, smax, substsz, gapo, gape);
}

// Default of gsa_score_db_multi_dev's scratch_limit: bytes of result matrix a call holds at once.
constexpr int64_t kDbMultiScratch = 256ll << 20;

bool offsets_ok(const int64_t* off, int32_t n)
{
    if (off[0] < 0) return false;
    for (int s = 0; s < n; ++s)
        if (off[s + 1] <= off[s] || off[s + 1] - off[s] > (int64_t)INT32_MAX) return false;
    return true;
}

// gsa_score_db_multi_dev: the queries in chunks of consecutive rows whose result matrix fits
// scratch_limit.  Per chunk: the pairs of other paths first (empty sides on the host, subjects past
// Lmax through score_batch_impl per query, whole queries through score_db_impl), then one launch of
// nw_lanes_multi.hip per sweep class over the lane subjects (sorted longest first once, for all
// queries), the other paths' results scattered into the matrix, the ranking, and one copy back.
// semi (gsa_score_db_multi_semi_dev, local = 0): the semi-global shape of nw_lanes_semi.hip.  There is
// no other path for it: every pair with letters on both sides runs on the lane kernel or the call is
// refused before anything is enqueued, and GSA_DB_LANES / GSA_DB_MAXC are not read.
// overlap (gsa_score_db_multi_overlap_dev, local = 0): the overlap shape of nw_lanes_overlap.hip, routed
// as the semi-global one is, with overlap_ranges' tests.
int score_db_multi_impl(gsa_ctx* ctx, const int32_t* queries, const int64_t* q_off, int32_t nq, const int32_t* db,
                        const int64_t* db_off, int32_t nsubj, const int32_t* subst, int32_t substsz, int32_t gapo,
                        int32_t gape, int32_t local, DbShape shape, int32_t top, int32_t max_workgroups, int64_t scratch_limit,
                        int32_t* scores, gsa_db_hit* hits, gsa_score_db_multi_info* info, float* kernel_ms,
                        hipStream_t st)
{
    static_assert(sizeof(gsa_db_hit) == sizeof(gsa::DbMultiHit), "gsa_db_hit is the ranking's record");
    const bool overlap = shape == DbShape::overlap;
    const bool semi = shape != DbShape::plain;  // the lane kernels alone, no second path
    if (!ctx || !queries || !q_off || !db || !db_off || !subst) return GSA_ERROR_INVALID_VALUE;
    if (nq < 1 || nsubj < 1) return GSA_ERROR_INVALID_VALUE;
    if (substsz < 1 || substsz > 32) return GSA_ERROR_INVALID_VALUE;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    if (top < 0 || max_workgroups < 0 || scratch_limit < 0) return GSA_ERROR_INVALID_VALUE;
    if (!scores && !hits) return GSA_ERROR_INVALID_VALUE;
    if (!offsets_ok(q_off, nq) || !offsets_ok(db_off, nsubj)) return GSA_ERROR_INVALID_VALUE;
    const int64_t limit = scratch_limit > 0 ? scratch_limit : kDbMultiScratch;
    const int64_t rowBytes = (int64_t)nsubj * (int64_t)sizeof(gsa::DbLanesOut);
    // rows of a chunk: within the limit, and few enough for 32-bit segment offsets in the ranking
    const int64_t rowsMax = std::min<int64_t>(std::min<int64_t>(limit / rowBytes, (1ll << 30) / nsubj), nq);
    if (rowsMax < 1) return GSA_ERROR_INVALID_VALUE;
    if (kernel_ms) *kernel_ms = 0.f;
    gsa_score_db_multi_info inf;
    std::memset(&inf, 0, sizeof(inf));
    if (info) *info = inf;
    const int ntop = std::min(top, nsubj);
    const bool rank = hits && ntop > 0;

    auto rows_of = [&](int q) { return q_off[q + 1] - q_off[q] - 1; };
    auto cols_of = [&](int s) { return db_off[s + 1] - db_off[s] - 1; };
    int64_t Rmax = 0, Cmax = 0;
    for (int q = 0; q < nq; ++q) Rmax = std::max(Rmax, rows_of(q));
    for (int s = 0; s < nsubj; ++s) Cmax = std::max(Cmax, cols_of(s));
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    long long smax = 1;
    if (Rmax > 0 && Cmax > 0)
    {
        std::vector<int32_t> sub((size_t)substsz * (size_t)substsz);
        if ((e = hipMemcpyAsync(sub.data(), subst, sub.size() * 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        smax = subst_absmax(sub.data(), substsz);
        // score_ranges' bounds grow with R and with C: the longest query against the longest subject
        // is outside every kernel's range iff any pair is
        bool stripOk = false;
        const int s = semi ? lane_only_ranges(shape, ctx, Rmax, Cmax, smax, substsz, gapo, gape)
                           : score_ranges(Rmax, Cmax, smax, gapo, gape, local, &stripOk);
        if (s != GSA_SUCCESS) return s;
    }
    const KeepLaunchRecord keep(ctx);

    // the subjects: the lane kernel's, longest first; those with no letters; those past Lmax
    const bool lanesOn = semi || env_int(ctx, "GSA_DB_LANES", 1) != 0;
    const int lmax = semi ? gsa::kDbLanesMaxC
                          : std::max(0, std::min(env_int(ctx, "GSA_DB_MAXC", kDbLanesLmax), gsa::kDbLanesMaxC));
    std::vector<int> laneS, emptyS, longS;
    for (int s = 0; s < nsubj; ++s)
    {
        const int64_t C = cols_of(s);
        (C == 0 ? emptyS : C <= lmax ? laneS : longS).push_back(s);
    }
    std::stable_sort(laneS.begin(), laneS.end(), [&](int x, int y) { return cols_of(x) > cols_of(y); });
    const size_t nl = laneS.size();
    const int cmax = nl ? (int)cols_of(laneS[0]) : 0;
    const int ntasks = (int)((nl + gsa::kDbLanesSubj - 1) / gsa::kDbLanesSubj);
    const int unitsPerQuery = (ntasks + gsa::kDbMultiUnit - 1) / gsa::kDbMultiUnit;
    // a query on the lane kernel: its profile fits LDS, and no lane subject is past the local key's bound
    auto on_lanes = [&](int64_t R) {
        if (!lanesOn || nl == 0 || R < 1 || R >= (1 << 20)) return false;
        if (gsa::dblanes_lds_bytes((int)R, substsz) > (size_t)ctx->lds_max) return false;
        return !local || smax * std::min<int64_t>(R, cmax) < gsa::kDbLanesMaxScore;
    };
    auto empty_pair = [&](int64_t R, int64_t C) {
        const int64_t k = R + C;
        // semi-global: no query letters, score 0 at (0, 0); no subject letters, R inserts ending in (R, 0)
        // overlap: an empty side, score 0 at (R, 0)
        if (overlap) return gsa::DbLanesOut {0, (int)R, 0, 0};
        if (semi) return gsa::DbLanesOut {R == 0 ? 0 : (int)(gapo + (R - 1) * gape), (int)R, 0, 0};
        return gsa::DbLanesOut {(local || k == 0) ? 0 : (int)(gapo + (k - 1) * gape), local ? 0 : (int)R, local ? 0 : (int)C, 0};
    };

    // meta: [unit counter, profile builds; 64 B][offsets][lengths][indices][a chunk's queries]
    const size_t offAt = 64, lenAt = offAt + nl * 8, idxAt = lenAt + nl * 4, qAt = (idxAt + nl * 4 + 15) / 16 * 16;
    const size_t metaBytes = qAt + (size_t)rowsMax * sizeof(gsa::DbMultiQuery);
    int s = reserve_hard(ctx, ctx->buf[kBufDbmMeta], metaBytes, 4096);
    if (s != GSA_SUCCESS) return s;
    if ((s = reserve_hard(ctx, ctx->buf[kBufDbmOut], (size_t)(rowsMax * rowBytes), 4096)) != GSA_SUCCESS) return s;
    size_t selBytes = 0, selTemp = 0;
    if (rank)
    {
        if ((e = gsa::dbmulti_select_bytes((int)rowsMax, nsubj, &selBytes, &selTemp)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        if ((s = reserve_hard(ctx, ctx->buf[kBufDbmSel], selBytes, 4096)) != GSA_SUCCESS) return s;
    }
    for (hipEvent_t& ev : ctx->dbmev)
        if (!ev && (e = hipEventCreate(&ev)) != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    char* const meta = ctx->buf[kBufDbmMeta].as<char>();
    gsa::DbLanesOut* const dout = ctx->buf[kBufDbmOut].as<gsa::DbLanesOut>();
    {
        std::vector<long long> hoff(nl);
        std::vector<int> hlen(nl);
        for (size_t k = 0; k < nl; ++k)
        {
            hoff[k] = (long long)db_off[laneS[k]];
            hlen[k] = (int)cols_of(laneS[k]);
        }
        // (pageable sources: the copies have left the vectors when the calls return)
        if ((e = hipMemsetAsync(meta, 0, 64, st)) != hipSuccess ||
            (nl && ((e = hipMemcpyAsync(meta + offAt, hoff.data(), nl * 8, hipMemcpyHostToDevice, st)) != hipSuccess ||
                    (e = hipMemcpyAsync(meta + lenAt, hlen.data(), nl * 4, hipMemcpyHostToDevice, st)) != hipSuccess ||
                    (e = hipMemcpyAsync(meta + idxAt, laneS.data(), nl * 4, hipMemcpyHostToDevice, st)) != hipSuccess)) ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    }

    float lanes_ms = 0.f, all_ms = 0.f, select_ms = 0.f, other_ms = 0.f;
    std::vector<gsa::DbMultiPatch> patches;
    std::vector<gsa::DbMultiQuery> hq;
    std::vector<gsa_pair_dev> pairs;
    std::vector<gsa_score_result> res;
    for (int64_t q0 = 0; q0 < nq; q0 += rowsMax)
    {
        const int64_t rows = std::min<int64_t>(rowsMax, nq - q0);
        const int64_t npair = rows * nsubj;
        patches.clear();
        hq.clear();
        auto patch = [&](int64_t row, int sidx, const gsa::DbLanesOut& v) {
            patches.push_back(gsa::DbMultiPatch {row * nsubj + sidx, v});
        };
        for (int64_t row = 0; row < rows; ++row)
        {
            const int q = (int)(q0 + row);
            const int64_t R = rows_of(q);
            const int32_t* const query = queries + q_off[q];
            if (R == 0)
            {
                for (int sj = 0; sj < nsubj; ++sj) patch(row, sj, empty_pair(0, cols_of(sj)));
                continue;
            }
            if (semi && nl == 0)
            {
                for (int sj = 0; sj < nsubj; ++sj) patch(row, sj, empty_pair(R, 0));
                continue;
            }
            if (!on_lanes(R))
            {
                if (semi) return GSA_ERROR_INVALID_VALUE;  // semi_ranges has let it through: not reached
                res.resize((size_t)nsubj);
                float ms = 0.f;
                if ((s = score_db_impl(ctx, query, (int32_t)(R + 1), db, db_off, nsubj, subst, substsz, gapo, gape, local,
                                       res.data(), &ms, st)) != GSA_SUCCESS)
                    return s;
                other_ms += ms;
                for (int sj = 0; sj < nsubj; ++sj)
                    patch(row, sj, gsa::DbLanesOut {res[(size_t)sj].score, (int)res[(size_t)sj].i_end, (int)res[(size_t)sj].j_end, 0});
                inf.other_queries += 1;
                continue;
            }
            hq.push_back(gsa::DbMultiQuery {(long long)q_off[q], (int)R, (int)row});
            for (int sj : emptyS) patch(row, sj, empty_pair(R, 0));
            if (!longS.empty())
            {
                pairs.resize(longS.size());
                res.resize(longS.size());
                for (size_t k = 0; k < longS.size(); ++k)
                {
                    gsa_pair_dev& p = pairs[k];
                    std::memset(&p, 0, sizeof(p));
                    p.seqY = query;
                    p.adjrows = (int32_t)(R + 1);
                    p.seqX = db + db_off[longS[k]];
                    p.adjcols = (int32_t)(cols_of(longS[k]) + 1);
                }
                float ms = 0.f;
                if ((s = score_batch_impl(ctx, (int32_t)longS.size(), pairs.data(), subst, substsz, gapo, gape, local,
                                          res.data(), &ms, st)) != GSA_SUCCESS)
                    return s;
                other_ms += ms;
                for (size_t k = 0; k < longS.size(); ++k)
                    patch(row, longS[k], gsa::DbLanesOut {res[k].score, (int)res[k].i_end, (int)res[k].j_end, 0});
            }
        }
        // results: [hits][scores][patches]
        const size_t scoAt = ((rank ? (size_t)rows * ntop * sizeof(gsa_db_hit) : 0) + 255) & ~(size_t)255;
        const size_t patAt = (scoAt + (scores ? (size_t)npair * 4 : 0) + 255) & ~(size_t)255;
        if ((s = reserve_hard(ctx, ctx->buf[kBufDbmRes], patAt + patches.size() * sizeof(gsa::DbMultiPatch), 4096)) != GSA_SUCCESS)
            return s;
        char* const dres = ctx->buf[kBufDbmRes].as<char>();
        // the lane queries, longest first: the sweep classes are runs of this order
        std::stable_sort(hq.begin(), hq.end(), [](const gsa::DbMultiQuery& x, const gsa::DbMultiQuery& y) { return x.R > y.R; });
        auto passes_of = [](int R) { return (R + gsa::kDbLanesPassRows - 1) / gsa::kDbLanesPassRows; };
        if (!hq.empty() &&
            (e = hipMemcpyAsync(meta + qAt, hq.data(), hq.size() * sizeof(gsa::DbMultiQuery), hipMemcpyHostToDevice, st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        // the boundary rows of every class, sized before the first launch: the buffer must not move between them
        std::vector<std::pair<size_t, size_t>> classes;  // [first, last) of hq
        size_t bndBytes = 0;
        std::vector<int> grids;
        for (size_t b = 0; b < hq.size();)
        {
            size_t k = b;
            const int passes = passes_of(hq[b].R);
            while (k < hq.size() && passes_of(hq[k].R) == passes) ++k;
            int wgs = 1;
            if ((e = overlap ? gsa::dboverlap_resident(passes, substsz, gapo != gape, &wgs)
                     : semi  ? gsa::dbsemi_resident(passes, substsz, gapo != gape, &wgs)
                             : gsa::dbmulti_resident(passes, substsz, local, gapo != gape, &wgs)) != hipSuccess)
                return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
            const long long nunits = (long long)(k - b) * unitsPerQuery;
            int grid = (int)std::max<long long>(1, std::min<long long>(wgs, nunits));
            if (max_workgroups > 0) grid = std::min(grid, max_workgroups);
            if (passes > 1)
                bndBytes = std::max(bndBytes, (size_t)grid * gsa::kDbLanesWaves * gsa::kDbLanesSubj * (size_t)(cmax + 1) * sizeof(int2));
            classes.emplace_back(b, k);
            grids.push_back(grid);
            b = k;
        }
        if (bndBytes && (s = reserve_hard(ctx, ctx->buf[kBufDbbnd], bndBytes, 4096)) != GSA_SUCCESS) return s;
        (void)hipEventRecord(ctx->dbmev[0], st);
        for (size_t c = 0; c < classes.size(); ++c)
        {
            const size_t b = classes[c].first, n = classes[c].second - b;
            gsa::DbMultiArgs a;
            std::memset(&a, 0, sizeof(a));
            a.queries = queries;
            a.q = (const gsa::DbMultiQuery*)(meta + qAt) + b;
            a.nq = (int)n;
            a.db = db;
            a.subst = subst;
            a.substsz = substsz;
            a.go = gapo;
            a.ge = gape;
            a.passes = passes_of(hq[b].R);
            a.nsubj = (int)nl;
            a.ntasks = ntasks;
            a.unitsPerQuery = unitsPerQuery;
            a.nunits = (int)(n * (size_t)unitsPerQuery);
            a.off = (const long long*)(meta + offAt);
            a.len = (const int*)(meta + lenAt);
            a.sidx = (const int*)(meta + idxAt);
            a.out = dout;
            a.ld = nsubj;
            a.counter = (unsigned*)meta;
            a.builds = (unsigned*)meta + 1;
            a.bnd = a.passes > 1 ? ctx->buf[kBufDbbnd].as<int2>() : nullptr;
            a.bndStride = cmax + 1;
            if ((e = hipMemsetAsync(meta, 0, 4, st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
            if ((e = overlap ? gsa::launch_dboverlap(a, grids[c], st)
                     : semi  ? gsa::launch_dbsemi(a, grids[c], st)
                             : gsa::launch_dbmulti(a, local, grids[c], st)) != hipSuccess)
                return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
            note_launch(ctx);
            inf.launches += 1;
            inf.workgroups = grids[c];
            inf.units += a.nunits;
            inf.lane_pairs += (int64_t)n * (int64_t)nl;
        }
        inf.lane_queries += (int32_t)hq.size();
        (void)hipEventRecord(ctx->dbmev[1], st);
        if (!patches.empty())
        {
            if ((e = hipMemcpyAsync(dres + patAt, patches.data(), patches.size() * sizeof(gsa::DbMultiPatch),
                                    hipMemcpyHostToDevice, st)) != hipSuccess)
                return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
            if ((e = gsa::launch_dbmulti_scatter((const gsa::DbMultiPatch*)(dres + patAt), (long long)patches.size(), dout, st)) != hipSuccess)
                return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        }
        if (scores && (e = gsa::launch_dbmulti_scores(dout, npair, (int*)(dres + scoAt), st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        (void)hipEventRecord(ctx->dbmev[2], st);
        if (rank && (e = gsa::launch_dbmulti_select(dout, (int)rows, nsubj, ntop, ctx->buf[kBufDbmSel].p, selTemp,
                                                    (gsa::DbMultiHit*)dres, st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        (void)hipEventRecord(ctx->dbmev[3], st);
        ctx->mem.glmem_peak_allocs = std::max<int64_t>(ctx->mem.glmem_peak_allocs, held_bytes(ctx));
        if (scores && (e = hipMemcpyAsync(scores + q0 * nsubj, dres + scoAt, (size_t)npair * 4, hipMemcpyDeviceToHost, st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        if (rank && (e = hipMemcpyAsync(hits + q0 * ntop, dres, (size_t)rows * ntop * sizeof(gsa_db_hit), hipMemcpyDeviceToHost, st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        float m0 = 0.f, m1 = 0.f, m2 = 0.f;
        (void)hipEventElapsedTime(&m0, ctx->dbmev[0], ctx->dbmev[1]);
        (void)hipEventElapsedTime(&m1, ctx->dbmev[2], ctx->dbmev[3]);
        (void)hipEventElapsedTime(&m2, ctx->dbmev[0], ctx->dbmev[3]);
        lanes_ms += m0;
        select_ms += m1;
        all_ms += m2;
        inf.result_bytes = std::max<int64_t>(inf.result_bytes, rows * rowBytes);
    }
    unsigned builds = 0;
    if ((e = hipMemcpyAsync(&builds, meta + 4, 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    inf.profile_builds = builds;
    inf.lanes_ms = lanes_ms;
    inf.select_ms = select_ms;
    if (info) *info = inf;
    if (kernel_ms) *kernel_ms = all_ms + other_ms;
    return GSA_SUCCESS;
}


// gsa_align_db_multi_dev: the hits of many queries in one call.  Every pair is routed as
// align_db_impl routes it for that query (empty sides on the host, status 1 through one
// score_batch_impl call for all queries); the traced hits follow the plan of
// nw_lanes_trace_multi_plan.h: per chunk one upload of its records, one fill launch per sweep class
// (nw_lanes_trace_multi.hip), one walk launch over all its hits and one copy back.  The code, meta and
// result buffers are gsa_align_db_dev's.  gsa_last_launch's record is left as it was.
// semi (gsa_align_db_multi_semi_dev, local = 0): the semi-global shape of nw_lanes_semi_trace.hip on
// the same plan and buffers.  No hit is status 1: a hit outside semi_ranges, or a scratch_limit below
// the largest hit's move codes, refuses the call before anything is enqueued.
// overlap (gsa_align_db_multi_overlap_dev, local = 0): the overlap shape of nw_lanes_overlap_trace.hip,
// routed as the semi-global one is, with overlap_ranges' tests over the hits.
int align_db_multi_impl(gsa_ctx* ctx, const int32_t* queries, const int64_t* q_off, int32_t nq, const int32_t* db,
                        const int64_t* db_off, int32_t nsubj, const int32_t* hit_query, const int32_t* hit_subject,
                        int32_t nhits, const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int32_t local,
                        DbShape shape, int32_t max_workgroups, int64_t scratch_limit, gsa_align_db_result* out, char* cigar,
                        int64_t cigar_cap, int64_t* cigar_need, gsa_align_db_multi_info* info, float* kernel_ms,
                        hipStream_t st)
{
    if (!ctx || !queries || !q_off || !db || !db_off || !subst || !out) return GSA_ERROR_INVALID_VALUE;
    const bool overlap = shape == DbShape::overlap;
    const bool semi = shape != DbShape::plain;  // the lane kernels alone, no second path
    if (nq < 1 || nsubj < 1) return GSA_ERROR_INVALID_VALUE;
    if (substsz < 1 || substsz > 32) return GSA_ERROR_INVALID_VALUE;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    if (nhits < 0 || max_workgroups < 0 || scratch_limit < 0 || cigar_cap < 0) return GSA_ERROR_INVALID_VALUE;
    if ((nhits > 0 && (!hit_query || !hit_subject)) || (cigar_cap > 0 && !cigar)) return GSA_ERROR_INVALID_VALUE;
    if (!offsets_ok(q_off, nq) || !offsets_ok(db_off, nsubj)) return GSA_ERROR_INVALID_VALUE;
    for (int h = 0; h < nhits; ++h)
        if (hit_query[h] < 0 || hit_query[h] >= nq || hit_subject[h] < 0 || hit_subject[h] >= nsubj)
            return GSA_ERROR_INVALID_VALUE;
    if (kernel_ms) *kernel_ms = 0.f;
    if (cigar_need) *cigar_need = 0;
    gsa_align_db_multi_info inf;
    std::memset(&inf, 0, sizeof(inf));
    if (info) *info = inf;
    auto rows_of = [&](int q) { return q_off[q + 1] - q_off[q] - 1; };
    auto cols_of = [&](int s) { return db_off[s + 1] - db_off[s] - 1; };
    int64_t Rmax = 0, Cmax = 0;
    for (int q = 0; q < nq; ++q) Rmax = std::max(Rmax, rows_of(q));
    for (int s = 0; s < nsubj; ++s) Cmax = std::max(Cmax, cols_of(s));
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    long long smax = 1;
    if (Rmax > 0 && Cmax > 0)
    {
        std::vector<int32_t> sub((size_t)substsz * (size_t)substsz);
        if ((e = hipMemcpyAsync(sub.data(), subst, sub.size() * 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        smax = subst_absmax(sub.data(), substsz);
        // score_ranges' bounds grow with R and with C: the longest query against the longest subject
        // is outside every kernel's range iff any pair is
        bool stripOk = false;
        // (semi-global and overlap: the hits alone are tested, below)
        const int s = semi ? GSA_SUCCESS : score_ranges(Rmax, Cmax, smax, gapo, gape, local, &stripOk);
        if (s != GSA_SUCCESS) return s;
    }
    if (nhits == 0) return GSA_SUCCESS;
    const KeepLaunchRecord keep(ctx);

    // the route of every pair, with that hit's query: align_db_impl's conditions
    const int64_t limit = scratch_limit > 0 ? scratch_limit : kAlignDbScratch;
    std::vector<std::string> cig((size_t)nhits);
    std::vector<unsigned char> lane((size_t)nhits, 0);
    std::vector<int> other;
    for (int h = 0; h < nhits; ++h)
    {
        const int64_t R = rows_of(hit_query[h]), C = cols_of(hit_subject[h]);
        gsa_align_db_result& r = out[h];
        std::memset(&r, 0, sizeof(r));
        if (overlap && (R == 0 || C == 0))
        {
            // an empty side: score 0, all cells (R, 0), nothing to say
            r.i_start = r.i_end = R;
            continue;
        }
        if (semi && (R == 0 || C == 0))
        {
            // no query letters: score 0 at (0, 0), nothing to say; no subject letters: R inserts
            if (R > 0)
            {
                r.score = (int32_t)(gapo + (R - 1) * gape);
                r.i_end = R;
                cig[(size_t)h] = std::to_string(R) + 'I';
            }
            continue;
        }
        if (semi)
        {
            if (lane_only_ranges(shape, ctx, R, C, smax, substsz, gapo, gape) != GSA_SUCCESS || gsa::dbtrace_code_bytes(R, C) > limit)
                return GSA_ERROR_INVALID_VALUE;
            lane[(size_t)h] = 1;
            continue;
        }
        if (R == 0 || C == 0)
        {
            const int64_t k = R + C;
            if (!local && k > 0)
            {
                r.score = (int32_t)(gapo + (k - 1) * gape);
                r.i_end = R;
                r.j_end = C;
                cig[(size_t)h] = std::to_string(k) + (R > 0 ? 'I' : 'D');
            }
            continue;
        }
        const bool fits = R < (1 << 20) && gsa::dblanes_lds_bytes((int)R, substsz) <= (size_t)ctx->lds_max;
        const bool keyOk = !local || smax * std::min(R, C) < gsa::kDbLanesMaxScore;
        const bool valOk = smax * std::min(R, C) + (long long)(-gapo) + (R + C) * (long long)(-gape) < gsa::kDbTraceMaxValue;
        const bool take = fits && C <= gsa::kDbLanesMaxC && keyOk && valOk && gsa::dbtrace_code_bytes(R, C) <= limit;
        if (take)
            lane[(size_t)h] = 1;
        else
            other.push_back(h);
    }
    float fill_ms = 0.f, walk_ms = 0.f, other_ms = 0.f;
    const std::vector<gsa::DbaChunk> plan =
        gsa::dba_plan(nhits, hit_query, hit_subject, q_off, db_off, lane.data(), limit, gsa::kDbAlignMultiUnit);
    if (!plan.empty())
    {
        static_assert(sizeof(gsa::DbaQuery) == 16 && sizeof(gsa::DbaTask) == 8 && sizeof(gsa::DbaUnit) == 16, "device records");
        // the largest of every buffer over the chunks, and every launch's grid
        size_t maxN = 0, maxQ = 0, maxT = 0, maxU = 0, bndBytes = 0;
        int64_t maxCodes = 0, maxMoves = 0;
        std::vector<std::vector<int>> grids(plan.size());
        for (size_t c = 0; c < plan.size(); ++c)
        {
            const gsa::DbaChunk& ch = plan[c];
            maxN = std::max(maxN, ch.hits.size());
            maxQ = std::max(maxQ, ch.queries.size());
            maxT = std::max(maxT, ch.tasks.size());
            maxU = std::max(maxU, ch.units.size());
            maxCodes = std::max<int64_t>(maxCodes, ch.codeBytes);
            maxMoves = std::max<int64_t>(maxMoves, ch.moveBytes);
            for (const gsa::DbaLaunch& L : ch.launches)
            {
                int wgs = 1;
                if ((e = overlap ? gsa::dboverlap_trace_resident(L.passes, substsz, gapo != gape, &wgs)
                         : semi  ? gsa::dbsemi_trace_resident(L.passes, substsz, gapo != gape, &wgs)
                                 : gsa::dbtrace_multi_resident(L.passes, substsz, local, gapo != gape, &wgs)) != hipSuccess)
                    return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
                int grid = std::max(1, std::min(wgs, L.nunits));
                if (max_workgroups > 0) grid = std::min(grid, max_workgroups);
                grids[c].push_back(grid);
                if (L.passes > 1)
                    bndBytes = std::max(bndBytes, (size_t)grid * gsa::kDbLanesWaves * gsa::kDbLanesSubj * (size_t)(ch.cmax + 1) * sizeof(int2));
            }
        }
        // meta: [unit counter, profile builds; 64 B][offsets][query offsets][code offsets][move offsets]
        //       [lengths][queries][tasks][units][fill results]
        auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
        const size_t offAt = 64, qoffAt = offAt + maxN * 8, coffAt = qoffAt + maxN * 8, moffAt = coffAt + maxN * 8;
        const size_t lenAt = moffAt + maxN * 8, qAt = up16(lenAt + maxN * 4), taskAt = qAt + maxQ * sizeof(gsa::DbaQuery);
        const size_t unitAt = up16(taskAt + maxT * sizeof(gsa::DbaTask)), foutAt = unitAt + maxU * sizeof(gsa::DbaUnit);
        const size_t metaBytes = foutAt + maxN * sizeof(gsa::DbLanesOut);
        // results: [walk results][move bytes]
        const size_t movAt = maxN * sizeof(gsa::DbTraceOut);
        const size_t resBytes = movAt + (size_t)maxMoves;
        int s;
        if ((s = reserve_hard(ctx, ctx->buf[kBufAdbMeta], metaBytes, 4096)) != GSA_SUCCESS ||
            (s = reserve_hard(ctx, ctx->buf[kBufAdbRes], resBytes, 4096)) != GSA_SUCCESS ||
            (s = reserve_hard(ctx, ctx->buf[kBufAdbCodes], (size_t)maxCodes, 4096)) != GSA_SUCCESS)
            return s;
        if (bndBytes && (s = reserve_hard(ctx, ctx->buf[kBufDbbnd], bndBytes, 4096)) != GSA_SUCCESS) return s;
        if (const int es = ensure_trace_events(ctx); es != GSA_SUCCESS) return es;
        char* const meta = ctx->buf[kBufAdbMeta].as<char>();
        unsigned char* const adbres = ctx->buf[kBufAdbRes].as<unsigned char>();
        if ((e = hipMemsetAsync(meta, 0, 64, st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        std::vector<char> hmeta(foutAt), hres(resBytes);
        for (size_t c = 0; c < plan.size(); ++c)
        {
            const gsa::DbaChunk& ch = plan[c];
            const size_t n = ch.hits.size();
            long long* const hoff = (long long*)(hmeta.data() + offAt);
            long long* const hqoff = (long long*)(hmeta.data() + qoffAt);
            long long* const hcoff = (long long*)(hmeta.data() + coffAt);
            long long* const hmoff = (long long*)(hmeta.data() + moffAt);
            int* const hlen = (int*)(hmeta.data() + lenAt);
            for (size_t k = 0; k < n; ++k)
            {
                hoff[k] = ch.hits[k].dbOff;
                hqoff[k] = ch.hits[k].qOff;
                hcoff[k] = ch.hits[k].codeOff;
                hmoff[k] = ch.hits[k].moveOff;
                hlen[k] = ch.hits[k].C;
            }
            std::memcpy(hmeta.data() + qAt, ch.queries.data(), ch.queries.size() * sizeof(gsa::DbaQuery));
            std::memcpy(hmeta.data() + taskAt, ch.tasks.data(), ch.tasks.size() * sizeof(gsa::DbaTask));
            std::memcpy(hmeta.data() + unitAt, ch.units.data(), ch.units.size() * sizeof(gsa::DbaUnit));
            if ((e = hipMemcpyAsync(meta + offAt, hmeta.data() + offAt, foutAt - offAt, hipMemcpyHostToDevice, st)) != hipSuccess)
                return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
            (void)hipEventRecord(ctx->adbev[0], st);
            for (size_t l = 0; l < ch.launches.size(); ++l)
            {
                const gsa::DbaLaunch& L = ch.launches[l];
                gsa::DbTraceMultiArgs a;
                std::memset(&a, 0, sizeof(a));
                a.queries = queries;
                a.db = db;
                a.subst = subst;
                a.substsz = substsz;
                a.go = gapo;
                a.ge = gape;
                a.passes = L.passes;
                a.q = (const gsa::DbaQuery*)(meta + qAt);
                a.units = (const gsa::DbaUnit*)(meta + unitAt) + L.firstUnit;
                a.nunits = L.nunits;
                a.tasks = (const gsa::DbaTask*)(meta + taskAt);
                a.off = (const long long*)(meta + offAt);
                a.len = (const int*)(meta + lenAt);
                a.codeOff = (const long long*)(meta + coffAt);
                a.out = (gsa::DbLanesOut*)(meta + foutAt);
                a.codes = ctx->buf[kBufAdbCodes].as<unsigned char>();
                a.counter = (unsigned*)meta;
                a.builds = (unsigned*)meta + 1;
                a.bnd = L.passes > 1 ? ctx->buf[kBufDbbnd].as<int2>() : nullptr;
                a.bndStride = ch.cmax + 1;
                if ((e = hipMemsetAsync(meta, 0, 4, st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
                if ((e = overlap ? gsa::launch_dboverlap_trace_fill(a, grids[c][l], st)
                         : semi  ? gsa::launch_dbsemi_trace_fill(a, grids[c][l], st)
                                 : gsa::launch_dbtrace_multi_fill(a, local, grids[c][l], st)) != hipSuccess)
                    return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
                note_launch(ctx);
                inf.launches += 1;
                inf.workgroups = grids[c][l];
            }
            (void)hipEventRecord(ctx->adbev[1], st);
            gsa::DbTraceMultiWalkArgs w;
            std::memset(&w, 0, sizeof(w));
            w.queries = queries;
            w.db = db;
            w.nhits = (int)n;
            w.local = local;
            w.qoff = (const long long*)(meta + qoffAt);
            w.off = (const long long*)(meta + offAt);
            w.len = (const int*)(meta + lenAt);
            w.out = (const gsa::DbLanesOut*)(meta + foutAt);
            w.codes = ctx->buf[kBufAdbCodes].as<unsigned char>();
            w.codeOff = (const long long*)(meta + coffAt);
            w.moveOff = (const long long*)(meta + moffAt);
            w.res = (gsa::DbTraceOut*)adbres;
            w.moves = adbres + movAt;
            if ((e = overlap ? gsa::launch_dboverlap_trace_walk(w, st)
                     : semi  ? gsa::launch_dbsemi_trace_walk(w, st)
                             : gsa::launch_dbtrace_multi_walk(w, st)) != hipSuccess)
                return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
            (void)hipEventRecord(ctx->adbev[2], st);
            if ((e = hipMemcpyAsync(hres.data(), adbres, movAt + (size_t)ch.moveBytes, hipMemcpyDeviceToHost, st)) != hipSuccess ||
                (e = hipStreamSynchronize(st)) != hipSuccess)
                return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
            add_trace_ms(ctx, &fill_ms, &walk_ms);
            const gsa::DbTraceOut* const ho = (const gsa::DbTraceOut*)hres.data();
            for (size_t k = 0; k < n; ++k)
            {
                const gsa::DbaHit& H = ch.hits[k];
                gsa_align_db_result& r = out[H.hit];
                r.score = ho[k].score;
                r.i_start = ho[k].i_start;
                r.j_start = ho[k].j_start;
                r.i_end = ho[k].i_end;
                r.j_end = ho[k].j_end;
                if (ho[k].moves < 0 || ho[k].moves > H.moveLen) return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);
                cig[(size_t)H.hit] = fold_cigar((const unsigned char*)hres.data() + movAt + H.moveOff, ho[k].moves);
            }
            inf.chunks += 1;
            inf.lane_hits += (int32_t)n;
            inf.lane_queries += (int32_t)ch.queries.size();
            inf.tasks += (int64_t)ch.tasks.size();
            inf.units += (int64_t)ch.units.size();
            inf.code_bytes = std::max<int64_t>(inf.code_bytes, ch.codeBytes);
        }
        unsigned builds = 0;
        if ((e = hipMemcpyAsync(&builds, meta + 4, 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        inf.profile_builds = builds;
    }
    if (!other.empty())
    {
        // score and end cell from the score path, all queries' pairs in one batch
        std::vector<gsa_pair_dev> pairs(other.size());
        std::vector<gsa_score_result> res(other.size());
        for (size_t k = 0; k < other.size(); ++k)
        {
            const int h = other[k];
            gsa_pair_dev& p = pairs[k];
            std::memset(&p, 0, sizeof(p));
            p.seqY = queries + q_off[hit_query[h]];
            p.adjrows = (int32_t)(rows_of(hit_query[h]) + 1);
            p.seqX = db + db_off[hit_subject[h]];
            p.adjcols = (int32_t)(cols_of(hit_subject[h]) + 1);
        }
        const int s = score_batch_impl(ctx, (int32_t)other.size(), pairs.data(), subst, substsz, gapo, gape, local,
                                       res.data(), &other_ms, st);
        if (s != GSA_SUCCESS) return s;
        for (size_t k = 0; k < other.size(); ++k)
        {
            gsa_align_db_result& r = out[other[k]];
            r.score = res[k].score;
            r.i_end = res[k].i_end;
            r.j_end = res[k].j_end;
            r.status = 1;
        }
        inf.unsupported = (int32_t)other.size();
    }
    // the strings back to back in hit order
    const int64_t at = pack_cigars(out, cig.data(), nhits, cigar, cigar_cap);
    if (cigar_need) *cigar_need = at;
    inf.fill_ms = fill_ms;
    inf.walk_ms = walk_ms;
    if (info) *info = inf;
    if (kernel_ms) *kernel_ms = fill_ms + walk_ms + other_ms;
    return GSA_SUCCESS;
}

// ---- One long pair traced from its score launch's checkpoint rows: the chunk loop ----
//
// trace_pair is the host loop of gsa_align_pair_dev, gsa_align_pair_semi_dev and
// gsa_align_pair_overlap_dev.  The score launch left the bottom row of each of its strips in kBufGran.
// The walk starts on (iEnd, jEnd) in state H; its record lives at kBufPairMeta + 64, the fill's task
// counter at kBufPairMeta + 0, the moves in kBufPairMoves (at most iEnd + jEnd - jW of them).  The caller
// planned the first chunk (only it knows what a limit below one strip means for its mode).  Per chunk:
// kBufPairCodes for its codes, the counter zeroed, one fill and one walk launch (the mode's launcher),
// the record copied back; a finished walk ends the loop, any other must stand on the chunk's upper
// boundary (the mode's go-on test), and the next chunk is semi_plan_chunk's for the columns
// jW + 1 ... rec.j.  At the end the moves are copied back and folded into the CIGAR.
//
// A mode is a struct of types and static functions: FillArgs, WalkArgs and WalkRec of its trace unit;
// mode_args, which sets the fields of the two argument structs only that unit has; launch (its
// *_fill_grid and launch_*_trace); rec_ok, go_on and end_ok, its checks of a returned record.

// What the loop needs of the call and of its score launch.
struct PairTrace
{
    const int32_t *seqY, *seqX, *subst;
    int32_t substsz, gapo, gape, local;
    int64_t R, C;        // letters of seqY and of seqX
    int64_t iEnd, jEnd;  // the cell the walk starts on
    int64_t jW;          // codes are kept for the columns jW + 1 ... jEnd; 0 in the modes without a window
    int KR;              // rows of a lane in the codes; a strip has 64 KR rows
    int64_t tickets;     // strips of the score launch: its second array lies that many rows behind the first
    int64_t limit;       // bytes of codes held at once
};

template <class Mode, class Info>
int trace_pair(gsa_ctx* ctx, const PairTrace& t, gsa::PairChunk ch, Info* inf, gsa_align_db_result* r, std::string* cig,
               hipStream_t st)
{
    using Rec = typename Mode::WalkRec;
    const int64_t TR = 64 * (int64_t)t.KR;
    const int64_t maxMoves = t.iEnd + t.jEnd - t.jW;
    int s;
    hipError_t e;
    if ((s = reserve_hard(ctx, ctx->buf[kBufPairMeta], 4096)) != GSA_SUCCESS ||
        (s = reserve_hard(ctx, ctx->buf[kBufPairMoves], (size_t)maxMoves, 4096)) != GSA_SUCCESS ||
        (s = ensure_trace_events(ctx)) != GSA_SUCCESS)
        return s;
    char* const meta = ctx->buf[kBufPairMeta].as<char>();
    Rec* const drec = (Rec*)(meta + 64);
    const size_t stride = (size_t)gsa::gran_stride((int)t.C);
    Rec rec;
    std::memset(&rec, 0, sizeof(rec));
    rec.i = (int)t.iEnd;
    rec.j = (int)t.jEnd;
    rec.state = 4u;
    if ((e = hipMemcpyAsync(drec, &rec, sizeof(rec), hipMemcpyHostToDevice, st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    for (;;)
    {
        const int nstrips = (int)(ch.tHi - ch.tLo + 1);
        if ((s = reserve_hard(ctx, ctx->buf[kBufPairCodes], (size_t)ch.codeBytes, 4096)) != GSA_SUCCESS) return s;
        if ((e = hipMemsetAsync(meta, 0, 4, st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        typename Mode::FillArgs f;
        std::memset(&f, 0, sizeof(f));
        f.seqY = t.seqY;
        f.seqX = t.seqX;
        f.subst = t.subst;
        f.substsz = t.substsz;
        f.go = t.gapo;
        f.ge = t.gape;
        f.J = (int)(t.jW + ch.J);  // the chunk's last column
        f.tLo = (int)ch.tLo;
        f.nstrips = nstrips;
        f.gran = ctx->buf[kBufGran].as<unsigned long long>();
        f.gran2 = f.gran + (size_t)t.tickets * stride;
        f.granStride = (long long)stride;
        f.codes = ctx->buf[kBufPairCodes].as<unsigned char>();
        f.stripBytes = ch.stripBytes;
        f.counter = (unsigned*)meta;
        typename Mode::WalkArgs w;
        std::memset(&w, 0, sizeof(w));
        w.seqY = t.seqY;
        w.seqX = t.seqX;
        w.codes = f.codes;
        w.stripBytes = ch.stripBytes;
        w.krShift = kr_shift(t.KR);
        w.tLo = (int)ch.tLo;
        w.iStop = (int)gsa::pair_chunk_stop_row(TR, ch);
        w.rec = drec;
        w.moves = ctx->buf[kBufPairMoves].as<unsigned char>();
        Mode::mode_args(t, f, w);
        if ((e = Mode::launch(t, f, w, ctx->adbev, st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        note_launch(ctx);
        if ((e = hipMemcpyAsync(&rec, drec, sizeof(rec), hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        add_trace_ms(ctx, &inf->fill_ms, &inf->walk_ms);
        inf->chunks += 1;
        inf->strips_filled += nstrips;
        inf->code_bytes = std::max<int64_t>(inf->code_bytes, ch.codeBytes);
        // moves written past their buffer, or a record the mode does not take
        if (rec.n < 0 || rec.n > maxMoves || !Mode::rec_ok(t, ch, rec)) return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);
        if (rec.done) break;
        // on the chunk's upper boundary: the next chunk, for the columns up to here
        if (!Mode::go_on(t, TR, ch, rec) || !gsa::semi_plan_chunk(TR, ch.tLo - 1, rec.j, t.jW, t.limit, &ch))
            return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);
    }
    if (!Mode::end_ok(rec)) return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);
    std::vector<unsigned char> mv((size_t)rec.n + 1);
    if (rec.n > 0 &&
        ((e = hipMemcpyAsync(mv.data(), ctx->buf[kBufPairMoves].p, (size_t)rec.n, hipMemcpyDeviceToHost, st)) != hipSuccess ||
         (e = hipStreamSynchronize(st)) != hipSuccess))
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    *cig = fold_cigar(mv.data(), rec.n);
    r->i_start = rec.i;
    r->j_start = rec.j;
    r->status = 0;
    return GSA_SUCCESS;
}

// The single-pair calls' shared end: the CIGAR into the caller's buffer (status 2 when it does not
// fit), the bytes it needs, the info and the kernel time.
template <class Info>
int finish_pair(gsa_align_db_result r, const std::string& cig, const Info& inf, gsa_align_db_result* out, char* cigar,
                int64_t cigar_cap, int64_t* cigar_need, Info* info, float* kernel_ms)
{
    const int64_t need = pack_cigars(&r, &cig, 1, cigar, cigar_cap);
    if (cigar_need) *cigar_need = need;
    *out = r;
    if (info) *info = inf;
    if (kernel_ms) *kernel_ms = inf.score_ms + inf.fill_ms + inf.walk_ms;
    return GSA_SUCCESS;
}

// gsa_align_pair_dev's unit (nw_pair_trace.hip): rows 1 ... iEnd of a pair of R rows, global or local.  A
// local path may end anywhere, so a finished record is taken as it stands.
struct GlobalTrace
{
    using FillArgs = gsa::PairFillArgs;
    using WalkArgs = gsa::PairWalkArgs;
    using WalkRec = gsa::PairWalkRec;
    static void mode_args(const PairTrace& t, FillArgs& f, WalkArgs& w)
    {
        f.local = w.local = t.local ? 1 : 0;
        f.R = (int)t.R;
        f.iEnd = (int)t.iEnd;
    }
    static hipError_t launch(const PairTrace& t, const FillArgs& f, const WalkArgs& w, hipEvent_t* ev, hipStream_t st)
    {
        int grid = 1;
        const hipError_t e = gsa::pair_fill_grid(f.local, t.gapo != t.gape, t.KR, f.nstrips, &grid);
        return e != hipSuccess ? e : gsa::launch_pair_trace(f, w, t.KR, grid, ev, st);
    }
    static bool rec_ok(const PairTrace&, const gsa::PairChunk&, const WalkRec&) { return true; }
    static bool go_on(const PairTrace&, int64_t TR, const gsa::PairChunk& ch, const WalkRec& r)
    {
        return ch.tLo >= 1 && r.i == gsa::pair_chunk_stop_row(TR, ch) && r.j >= 1 && r.j <= ch.J;
    }
    static bool end_ok(const WalkRec&) { return true; }
};

// gsa_align_pair_dev: the score from the K-rows score kernel in one direction (score_ag_strip with a
// route), whose checkpoint rows stay in kBufGran; then trace_pair from the end cell.  A pair the K-rows
// kernel or the 4 v + tag form does not take, or whose single strip exceeds the limit, gets its score
// and end cell and status 1.  gsa_last_launch's record is left as it was.
int align_pair_impl(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                    const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int32_t local,
                    int64_t scratch_limit, gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                    gsa_align_pair_info* info, float* kernel_ms, hipStream_t st)
{
    if (!ctx || !seqY || !seqX || !subst || !out) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    if (scratch_limit < 0 || cigar_cap < 0 || (cigar_cap > 0 && !cigar)) return GSA_ERROR_INVALID_VALUE;
    if (kernel_ms) *kernel_ms = 0.f;
    if (cigar_need) *cigar_need = 0;
    gsa_align_pair_info inf;
    std::memset(&inf, 0, sizeof(inf));
    if (info) *info = inf;
    const int64_t R = adjrows - 1, C = adjcols - 1;
    const int64_t limit = scratch_limit > 0 ? scratch_limit : (int64_t)gsa::kPairTraceScratch;
    gsa_align_db_result r;
    std::memset(&r, 0, sizeof(r));
    std::string cig;
    if (R == 0 || C == 0)
    {
        // one boundary, answered on the host as align_db_impl answers it
        const int64_t k = R + C;
        if (!local && k > 0)
        {
            r.score = (int32_t)(gapo + (k - 1) * gape);
            r.i_end = R;
            r.j_end = C;
            cig = std::to_string(k) + (R > 0 ? 'I' : 'D');
        }
    }
    else
    {
        hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
        std::vector<int32_t> sub((size_t)substsz * (size_t)substsz);
        if ((e = hipMemcpyAsync(sub.data(), subst, sub.size() * 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        const long long smax = subst_absmax(sub.data(), substsz);
        bool stripOk = false;
        if ((s = score_ranges(R, C, smax, gapo, gape, local, &stripOk)) != GSA_SUCCESS) return s;
        const KeepLaunchRecord keep(ctx);
        // the fill keeps 4 x value + source: |H| <= smax min(R, C) + |go| + (R + C) |ge| (score_ranges' bound)
        const bool valOk = smax * std::min(R, C) + (long long)(-gapo) + (R + C) * (long long)(-gape) < gsa::kDbTraceMaxValue;
        gsa_score_result sr {};
        ScoreRoute route;
        bool have = false;
        if (valOk && stripOk && !score_scan_forced(ctx))
        {
            s = score_ag_strip(ctx, seqY, R, seqX, C, subst, substsz, gapo, gape, local, &sr, st, &route);
            if (s == GSA_SUCCESS)
                have = true;
            else if (s != kScoreTooLarge)
                return s;
        }
        if (!have)
        {
            // the ordinary score path, whatever it takes for this pair
            route = ScoreRoute {};
            if ((s = score_dev_impl(ctx, seqY, adjrows, seqX, adjcols, subst, substsz, gapo, gape, local, &sr, st, smax)) !=
                GSA_SUCCESS)
                return s;
        }
        inf.score_ms = sr.calc_kernel_ms;
        r.score = sr.score;
        r.i_end = sr.i_end;
        r.j_end = sr.j_end;
        r.status = 1;
        const int K = route.K;
        if (have && route.krow && (K == 2 || K == 4))
        {
            const int KR = K * gsa::kSparseNS;
            const int64_t TR = 64 * (int64_t)KR;
            inf.strip_rows = (int32_t)TR;
            if (local && sr.score == 0)
                r.status = 0;  // no positive cell: (0, 0), an empty CIGAR
            else
            {
                const int64_t iEnd = sr.i_end, jEnd = sr.j_end;
                const int64_t strips = gsa::pair_strips(TR, iEnd);
                inf.strips = (int32_t)strips;
                gsa::PairChunk ch;
                if (iEnd >= 1 && jEnd >= 1 && gsa::pair_plan_chunk(TR, strips - 1, jEnd, limit, &ch))
                {
                    const PairTrace t {seqY, seqX, subst, substsz, gapo, gape, local, R, C, iEnd, jEnd, 0, KR, route.tickets, limit};
                    if ((s = trace_pair<GlobalTrace>(ctx, t, ch, &inf, &r, &cig, st)) != GSA_SUCCESS) return s;
                }
            }
        }
    }
    return finish_pair(r, cig, inf, out, cigar, cigar_cap, cigar_need, info, kernel_ms);
}

// ---- A batch of long pairs traced from their score launch's checkpoint rows: the round loop (2.2j) ----
//
// trace_batch is the host loop of gsa_align_batch_dev, gsa_align_batch_semi_dev and
// gsa_align_batch_overlap_dev, over the pairs the caller chose to trace.  The batched score launch left
// every pair's checkpoint rows in kBufGran, at its own granOff.  Every walk starts on its pair's
// (iEnd, jEnd) in state H; the records live in kBufPairBatchRec, all moves in kBufPairMoves (pair b's at
// the sum of its predecessors' iEnd + jEnd - jW).  Per round (nw_pair_trace_batch_plan.h):
// kBufPairCodes for the round's codes; a descriptor and a walk per chunk and a task per strip, the
// tasks by width descending (the longest chains first); one upload into kBufPairBatchTab of the task
// counter (64 bytes, zero), the tasks, the descriptors and the walks; one fill and one walk launch (the
// mode's launcher); the records copied back; each checked and its pair moved on by the mode's advance
// rule.  At the end one copy of all moves, folded into the CIGARs.
//
// A mode is a struct of types and static functions: Desc, Walk, FillArgs, WalkArgs and WalkRec of its
// trace unit; base, the PairBatchDesc inside a Desc; window, which sets the fields only that unit has;
// launch (its *_batch_fill_grid and launch_*_batch_trace); rec_ok and advance.

// What the loop needs of the call and of its score launch.
struct BatchTrace
{
    const gsa_pair_dev* pairs;
    const int32_t* subst;
    int32_t substsz, gapo, gape, local, max_workgroups;
    int KR;               // rows of a lane in the codes; a strip has 64 KR rows
    long long granTotal;  // words of the score launch's first array: the second lies that far behind
    int64_t limit;        // bytes of codes held at once
};

// A pair the loop traces.
struct BatchTracePair
{
    int p;               // index into the call's pairs
    int64_t iEnd, jEnd;  // the cell its walk starts on
    int64_t jW;          // its column window; 0 in the modes without one
    long long granOff;   // its first checkpoint row within kBufGran, in words
};

template <class Mode, class Info>
int trace_batch(gsa_ctx* ctx, const BatchTrace& t, const std::vector<BatchTracePair>& bp, Info* inf, gsa_align_db_result* res,
                std::string* cig, hipStream_t st)
{
    using Rec = typename Mode::WalkRec;
    using Desc = typename Mode::Desc;
    using Walk = typename Mode::Walk;
    const int64_t TR = 64 * (int64_t)t.KR;
    const size_t nb = bp.size();
    inf->batch_pairs = (int32_t)nb;
    std::vector<int64_t> movOff(nb);
    int64_t movTotal = 0;
    for (size_t b = 0; b < nb; ++b)
    {
        movOff[b] = movTotal;
        movTotal += bp[b].iEnd + bp[b].jEnd - bp[b].jW;
    }
    int s;
    hipError_t e;
    if ((s = reserve_hard(ctx, ctx->buf[kBufPairMoves], (size_t)movTotal, 4096)) != GSA_SUCCESS ||
        (s = reserve_hard(ctx, ctx->buf[kBufPairBatchRec], nb * sizeof(Rec), 4096)) != GSA_SUCCESS ||
        (s = ensure_trace_events(ctx)) != GSA_SUCCESS)
        return s;
    Rec* const drec = ctx->buf[kBufPairBatchRec].as<Rec>();
    unsigned char* const dmoves = ctx->buf[kBufPairMoves].as<unsigned char>();
    const unsigned long long* const dgran = ctx->buf[kBufGran].as<unsigned long long>();
    std::vector<Rec> rec(nb);
    std::memset(rec.data(), 0, nb * sizeof(Rec));
    std::vector<gsa::BatchPairState> state(nb);
    for (size_t b = 0; b < nb; ++b)
    {
        rec[b].i = (int)bp[b].iEnd;
        rec[b].j = (int)bp[b].jEnd;
        rec[b].state = 4u;
        state[b].tHi = gsa::pair_strips(TR, bp[b].iEnd) - 1;
        state[b].J = bp[b].jEnd;
        state[b].jW = bp[b].jW;
        inf->strips += (int32_t)(state[b].tHi + 1);
    }
    if ((e = hipMemcpyAsync(drec, rec.data(), nb * sizeof(Rec), hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    std::vector<gsa::BatchChunk> chunks;
    std::vector<gsa::PairBatchTask> tasks;
    std::vector<Desc> descs;
    std::vector<Walk> walks;
    std::vector<char> blob;
    for (;;)
    {
        const long long used = gsa::batch_plan_round(TR, t.limit, state, &chunks);
        if (chunks.empty())
        {
            for (const gsa::BatchPairState& S : state)
                if (S.tHi >= 0) return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);  // (no progress)
            break;
        }
        if ((s = reserve_hard(ctx, ctx->buf[kBufPairCodes], (size_t)used, 4096)) != GSA_SUCCESS) return s;
        unsigned char* const dcodes = ctx->buf[kBufPairCodes].as<unsigned char>();
        tasks.clear();
        descs.clear();
        walks.clear();
        for (size_t c = 0; c < chunks.size(); ++c)
        {
            const gsa::BatchChunk& ch = chunks[c];
            const BatchTracePair& B = bp[(size_t)ch.pair];
            const gsa_pair_dev& P = t.pairs[B.p];
            Desc d;
            std::memset(&d, 0, sizeof(d));
            gsa::PairBatchDesc& pd = Mode::base(d);
            pd.seqY = P.seqY;
            pd.seqX = P.seqX;
            pd.R = P.adjrows - 1;
            pd.iEnd = (int)B.iEnd;
            pd.J = (int)(B.jW + ch.c.J);  // the chunk's last column
            pd.granBase = B.granOff;
            pd.granStride = (long long)gsa::gran_stride(P.adjcols - 1);
            pd.stripBytes = ch.c.stripBytes;
            for (long long strip = ch.c.tLo; strip <= ch.c.tHi; ++strip)
            {
                gsa::PairBatchTask k;
                k.pair = (int)c;
                k.strip = (int)strip;
                k.codeOff = ch.codeOff + gsa::pair_code_off(ch.c, strip);
                tasks.push_back(k);
            }
            Walk w;
            std::memset(&w, 0, sizeof(w));
            w.seqY = P.seqY;
            w.seqX = P.seqX;
            w.codes = dcodes + ch.codeOff;
            w.stripBytes = ch.c.stripBytes;
            w.tLo = (int)ch.c.tLo;
            w.iStop = (int)gsa::pair_chunk_stop_row(TR, ch.c);
            w.rec = ch.pair;
            w.moves = dmoves + movOff[(size_t)ch.pair];
            Mode::window(B, d, w);
            descs.push_back(d);
            walks.push_back(w);
        }
        // the longest chains first
        std::stable_sort(tasks.begin(), tasks.end(), [&](const gsa::PairBatchTask& a, const gsa::PairBatchTask& b) {
            return chunks[(size_t)a.pair].c.J > chunks[(size_t)b.pair].c.J;
        });
        // one upload: the task counter (64 bytes, zero), the tasks, the pairs, the walks
        const size_t oTask = 64, oDesc = oTask + tasks.size() * sizeof(gsa::PairBatchTask),
                     oWalk = oDesc + descs.size() * sizeof(Desc), tabBytes = oWalk + walks.size() * sizeof(Walk);
        if ((s = reserve_hard(ctx, ctx->buf[kBufPairBatchTab], tabBytes, 4096)) != GSA_SUCCESS) return s;
        char* const dtab = ctx->buf[kBufPairBatchTab].as<char>();
        blob.assign(tabBytes, 0);
        std::memcpy(blob.data() + oTask, tasks.data(), tasks.size() * sizeof(gsa::PairBatchTask));
        std::memcpy(blob.data() + oDesc, descs.data(), descs.size() * sizeof(Desc));
        std::memcpy(blob.data() + oWalk, walks.data(), walks.size() * sizeof(Walk));
        if ((e = hipMemcpyAsync(dtab, blob.data(), tabBytes, hipMemcpyHostToDevice, st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        typename Mode::FillArgs f;
        std::memset(&f, 0, sizeof(f));
        f.pairs = (const Desc*)(dtab + oDesc);
        f.tasks = (const gsa::PairBatchTask*)(dtab + oTask);
        f.ntasks = (int)tasks.size();
        f.subst = t.subst;
        f.substsz = t.substsz;
        f.go = t.gapo;
        f.ge = t.gape;
        f.gran = dgran;
        f.gran2 = dgran + t.granTotal;
        f.codes = dcodes;
        f.counter = (unsigned*)dtab;
        typename Mode::WalkArgs w;
        std::memset(&w, 0, sizeof(w));
        w.walks = (const Walk*)(dtab + oWalk);
        w.nwalks = (int)walks.size();
        w.krShift = kr_shift(t.KR);
        w.recs = drec;
        const int walkGrid = t.max_workgroups > 0 ? std::min(w.nwalks, (int)t.max_workgroups) : w.nwalks;
        if ((e = Mode::launch(t, f, w, walkGrid, ctx->adbev, st)) != hipSuccess) return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        note_launch(ctx);
        if ((e = hipMemcpyAsync(rec.data(), drec, nb * sizeof(Rec), hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        add_trace_ms(ctx, &inf->fill_ms, &inf->walk_ms);
        inf->rounds += 1;
        inf->strips_filled += (int32_t)tasks.size();
        inf->code_bytes = std::max<int64_t>(inf->code_bytes, used);
        // every record that came back: in range, and finished or on its chunk's upper boundary as its mode has it
        for (const gsa::BatchChunk& ch : chunks)
        {
            const BatchTracePair& B = bp[(size_t)ch.pair];
            const Rec& r = rec[(size_t)ch.pair];
            if (r.n < 0 || r.n > B.iEnd + B.jEnd - B.jW || r.i < 0 || r.i > B.iEnd || r.j < 0 || r.j > B.jW + ch.c.J ||
                !Mode::rec_ok(r) || !Mode::advance(TR, ch.c, r.i, r.j, r.done != 0, &state[(size_t)ch.pair]))
                return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);
        }
    }
    std::vector<unsigned char> mv((size_t)movTotal + 1);
    if ((e = hipMemcpyAsync(mv.data(), dmoves, (size_t)movTotal, hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    for (size_t b = 0; b < nb; ++b)
    {
        gsa_align_db_result& r = res[(size_t)bp[b].p];
        cig[(size_t)bp[b].p] = fold_cigar(mv.data() + movOff[b], rec[b].n);
        r.i_start = rec[b].i;
        r.j_start = rec[b].j;
        r.status = 0;
    }
    return GSA_SUCCESS;
}

// The batch calls' shared end: the strings back to back in pair order, the results, the bytes the
// strings need and the info.
template <class Info>
void finish_batch(std::vector<gsa_align_db_result>& res, const std::vector<std::string>& cig, const Info& inf,
                  gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need, Info* info)
{
    const int64_t need = pack_cigars(res.data(), cig.data(), (int64_t)res.size(), cigar, cigar_cap);
    std::copy(res.begin(), res.end(), out);
    if (cigar_need) *cigar_need = need;
    if (info) *info = inf;
}

// gsa_align_batch_dev's unit (nw_pair_trace_batch.hip)
struct GlobalBatchTrace
{
    using Desc = gsa::PairBatchDesc;
    using Walk = gsa::PairBatchWalk;
    using FillArgs = gsa::PairBatchFillArgs;
    using WalkArgs = gsa::PairBatchWalkArgs;
    using WalkRec = gsa::PairWalkRec;
    static gsa::PairBatchDesc& base(Desc& d) { return d; }
    static void window(const BatchTracePair&, Desc&, Walk&) {}
    static hipError_t launch(const BatchTrace& t, const FillArgs& f, WalkArgs w, int walkGrid, hipEvent_t* ev, hipStream_t st)
    {
        w.local = t.local ? 1 : 0;
        int grid = 1;
        const hipError_t e = gsa::pair_batch_fill_grid(w.local, t.gapo != t.gape, t.KR, f.ntasks, t.max_workgroups, &grid);
        return e != hipSuccess ? e : gsa::launch_pair_batch_trace(f, w.local, w, t.KR, grid, walkGrid, ev, st);
    }
    static bool rec_ok(const WalkRec&) { return true; }
    static bool advance(long long TR, const gsa::PairChunk& c, long long i, long long j, bool done, gsa::BatchPairState* s)
    {
        return gsa::pair_batch_advance(TR, c, i, j, done, s);
    }
};

// gsa_align_batch_dev: the pairs' scores from score_batch_impl's launch (with a route), whose
// checkpoint rows stay in kBufGran, every pair's at its own granOff; then trace_batch over the pairs
// that launch scored, while those rows are still there.  The pairs that launch did not run or flagged
// go through align_pair_impl afterwards, one by one: that call overwrites kBufGran and reuses the
// kBufPair* slots.  gsa_last_launch's record is left as it was.
int align_batch_impl(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                     int32_t gapo, int32_t gape, int32_t local, int32_t max_workgroups, int64_t scratch_limit,
                     gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                     gsa_align_batch_info* info, float* kernel_ms, hipStream_t st)
{
    if (!ctx || !pairs || !subst || !out || npairs < 1) return GSA_ERROR_INVALID_VALUE;
    if (substsz < 1 || substsz > 32) return GSA_ERROR_INVALID_VALUE;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    for (int p = 0; p < npairs; ++p)
        if (pairs[p].adjrows < 1 || pairs[p].adjcols < 1 || !pairs[p].seqY || !pairs[p].seqX) return GSA_ERROR_INVALID_VALUE;
    if (scratch_limit < 0 || cigar_cap < 0 || max_workgroups < 0 || (cigar_cap > 0 && !cigar)) return GSA_ERROR_INVALID_VALUE;
    if (kernel_ms) *kernel_ms = 0.f;
    if (cigar_need) *cigar_need = 0;
    gsa_align_batch_info inf;
    std::memset(&inf, 0, sizeof(inf));
    if (info) *info = inf;
    const int64_t limit = scratch_limit > 0 ? scratch_limit : (int64_t)gsa::kPairBatchScratch;
    std::vector<gsa_align_db_result> res((size_t)npairs);
    std::memset(res.data(), 0, res.size() * sizeof(gsa_align_db_result));
    std::vector<std::string> cig((size_t)npairs);
    float other_ms = 0.f;
    // pairs with an empty side: one boundary, answered on the host as align_db_impl answers it
    std::vector<int> work;
    for (int p = 0; p < npairs; ++p)
    {
        const int64_t R = pairs[p].adjrows - 1, C = pairs[p].adjcols - 1;
        if (R > 0 && C > 0)
        {
            work.push_back(p);
            continue;
        }
        const int64_t k = R + C;
        if (!local && k > 0)
        {
            res[(size_t)p].score = (int32_t)(gapo + (k - 1) * gape);
            res[(size_t)p].i_end = R;
            res[(size_t)p].j_end = C;
            cig[(size_t)p] = std::to_string(k) + (R > 0 ? 'I' : 'D');
        }
        inf.host_pairs += 1;
    }
    if (!work.empty())
    {
        hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
        std::vector<int32_t> sub((size_t)substsz * (size_t)substsz);
        if ((e = hipMemcpyAsync(sub.data(), subst, sub.size() * 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        const long long smax = subst_absmax(sub.data(), substsz);
        // the pairs the 4 v + tag form holds (align_pair_impl's bound) are scored together; the others alone
        std::vector<int> sel, alone;
        std::vector<gsa_pair_dev> selPairs;
        for (int p : work)
        {
            const int64_t R = pairs[p].adjrows - 1, C = pairs[p].adjcols - 1;
            bool stripOk = false;
            const int s = score_ranges(R, C, smax, gapo, gape, local, &stripOk);
            if (s != GSA_SUCCESS) return s;
            const bool valOk = smax * std::min(R, C) + (long long)(-gapo) + (R + C) * (long long)(-gape) < gsa::kDbTraceMaxValue;
            if (valOk && stripOk)
            {
                sel.push_back(p);
                selPairs.push_back(pairs[p]);
            }
            else
                alone.push_back(p);
        }
        const KeepLaunchRecord keep(ctx);
        BatchScoreRoute route;
        std::vector<gsa_score_result> sres(sel.size());
        if (!sel.empty())
        {
            const int s = score_batch_impl(ctx, (int32_t)sel.size(), selPairs.data(), subst, substsz, gapo, gape, local,
                                           sres.data(), &inf.score_ms, st, &route);
            if (s != GSA_SUCCESS) return s;
        }
        const int K = route.K;
        const int KR = K * gsa::kSparseNS;
        const int64_t TR = 64 * (int64_t)KR;
        // the batch pairs: scored by the launch, a positive score, and one strip within the limit
        std::vector<BatchTracePair> bp;
        for (size_t k = 0; k < sel.size(); ++k)
        {
            const int p = sel[k];
            if (!route.inBatch[k] || !(K == 2 || K == 4))
            {
                alone.push_back(p);
                continue;
            }
            inf.strip_rows = (int32_t)TR;
            gsa_align_db_result& r = res[(size_t)p];
            r.score = sres[k].score;
            r.i_end = sres[k].i_end;
            r.j_end = sres[k].j_end;
            r.status = 1;
            if (local && r.score == 0)
            {
                r.status = 0;  // no positive cell: (0, 0), an empty CIGAR
                inf.host_pairs += 1;
                continue;
            }
            if (r.i_end < 1 || r.j_end < 1 || gsa::pair_strip_bytes(TR, r.j_end) > limit) continue;
            bp.push_back(BatchTracePair {p, r.i_end, r.j_end, 0, route.granOff[k]});
        }
        if (!bp.empty())
        {
            const BatchTrace t {pairs, subst, substsz, gapo, gape, local, max_workgroups, KR, route.granTotal, limit};
            const int s = trace_batch<GlobalBatchTrace>(ctx, t, bp, &inf, res.data(), cig.data(), st);
            if (s != GSA_SUCCESS) return s;
        }
        // the pairs that went alone, after the rounds: this overwrites kBufGran and the kBufPair* slots
        std::sort(alone.begin(), alone.end());
        inf.alone_pairs = (int32_t)alone.size();
        for (int p : alone)
        {
            const int64_t cap = 2 * ((int64_t)pairs[p].adjrows + (int64_t)pairs[p].adjcols) + 1;
            std::vector<char> buf((size_t)cap);
            float ms = 0.f;
            const int s = align_pair_impl(ctx, pairs[p].seqY, pairs[p].adjrows, pairs[p].seqX, pairs[p].adjcols, subst, substsz,
                                          gapo, gape, local, scratch_limit, &res[(size_t)p], buf.data(), cap, nullptr, nullptr,
                                          &ms, st);
            if (s != GSA_SUCCESS) return s;
            other_ms += ms;
            if (res[(size_t)p].status == 0) cig[(size_t)p].assign(buf.data(), (size_t)res[(size_t)p].cigar_len);
            res[(size_t)p].cigar_off = res[(size_t)p].cigar_len = 0;
        }
    }
    finish_batch(res, cig, inf, out, cigar, cigar_cap, cigar_need, info);
    if (kernel_ms) *kernel_ms = inf.score_ms + inf.fill_ms + inf.walk_ms + other_ms;
    return GSA_SUCCESS;
}


// What semi_pair_score's launch ran: the K-rows geometry whose checkpoint rows stay in kBufGran (row t
// at t gran_stride(C), the affine second array `tickets` rows behind).
struct SemiRoute
{
    int K = 0;
    int64_t tickets = 0;
    long long pmax = 0;  // max(0, largest table value): the window's bound (nw_pair_semi_plan.h)
};

// gsa_score_semi_dev for a pair with letters on both sides: the range tests of a mode without a
// second path, then the K-rows score kernel's semi-global instance in one direction (row R into
// kBufBidi) and the kernel that takes that row's first maximum; one copy brings score and end column
// back.  gsa_last_launch's record and the fills' sticky error word are left alone.
// overlap (gsa_score_overlap_dev): the same tests and geometry on the overlap instances, which store
// column C of every row into kBufOvCol as well; the kernel behind them takes the maximum over row R and
// column C and brings the end cell's row back too.
int semi_pair_score(gsa_ctx* ctx, const int32_t* seqY, int64_t R, const int32_t* seqX, int64_t C, const int32_t* subst,
                    int32_t substsz, int32_t gapo, int32_t gape, bool forAlign, gsa_score_result* out, hipStream_t st,
                    SemiRoute* route, bool overlap = false)
{
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    std::vector<int32_t> sub((size_t)substsz * (size_t)substsz);
    if ((e = hipMemcpyAsync(sub.data(), subst, sub.size() * 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    const long long smax = subst_absmax(sub.data(), substsz);
    bool stripOk = false;
    int s = score_ranges(R, C, smax, gapo, gape, 0, &stripOk);
    if (s != GSA_SUCCESS) return s;
    if (!stripOk) return GSA_ERROR_INVALID_VALUE;  // span < 2^28: the shifted values' room in int32
    if (gsa::krow_score_lds_bytes(substsz) > (size_t)ctx->lds_max) return GSA_ERROR_INVALID_VALUE;
    // the kernel's own test of the shifted table (nw_kscore_kernel: error bit 2)
    for (const int32_t v0 : sub)
    {
        const long long v = (long long)v0 - gapo - gape;
        if (v <= -32768 || v > 32767) return GSA_ERROR_INVALID_VALUE;
    }
    // the fill keeps 4 x value + source (align_pair_impl's bound)
    if (forAlign && smax * std::min(R, C) + (long long)(-gapo) + (R + C) * (long long)(-gape) >= gsa::kDbTraceMaxValue)
        return GSA_ERROR_INVALID_VALUE;
    // rows per lane as score_ag_strip picks them for a global pair
    const int kenv = env_int(ctx, "GSA_SCORE_K", 0);
    const int scoreK = kenv == 2 || kenv == 4 ? kenv : (gapo == gape) ? 4 : 2;
    const int64_t TR = (int64_t)(64 * scoreK) * gsa::kSparseNS;
    const int64_t tickets = (R + TR - 1) / TR;
    if (tickets > (1ll << 30) || C > (1ll << 30)) return GSA_ERROR_INVALID_VALUE;
    if (route)
    {
        route->K = scoreK;
        route->tickets = tickets;
        route->pmax = std::max<long long>(0, *std::max_element(sub.begin(), sub.end()));
    }
    const KeepLaunchRecord keep(ctx);
    gsa::StripArgs a;
    std::memset(&a, 0, sizeof(a));
    a.subst = subst;
    a.substsz = substsz;
    a.g = gapo;
    a.go = gapo;
    a.ge = gape;
    a.ns = gsa::kSparseNS;
    gsa::PairDesc d;
    std::memset(&d, 0, sizeof(d));
    d.seqY = seqY;
    d.seqX = seqX;
    d.R = (int)R;
    d.C = (int)C;
    d.Cp = (int)C;
    d.nTickets = (int)tickets;
    if ((s = ensure_desc(ctx, 1)) != GSA_SUCCESS) return s;
    gsa::PairDesc* const ddesc = ctx->buf[kBufDesc].as<gsa::PairDesc>();
    if ((e = hipMemcpyAsync(ddesc, &d, sizeof(d), hipMemcpyHostToDevice, st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    const size_t gran = (size_t)tickets * (size_t)gsa::gran_stride((int)C);
    if ((s = ensure_gran(ctx, 2 * gran, st)) != GSA_SUCCESS) return s;
    if ((s = reserve_hard(ctx, ctx->buf[kBufSctl], 64)) != GSA_SUCCESS) return s;
    // row R: columns -kTapPad .. C + 79, as the tap rows
    if ((s = reserve_hard(ctx, ctx->buf[kBufBidi], (size_t)(gsa::kTapPad + C + 80) * sizeof(int))) != GSA_SUCCESS) return s;
    // overlap: column C of the rows 0 ... tickets TR (every strip stores its rows, those past R too)
    if (overlap && (s = reserve_hard(ctx, ctx->buf[kBufOvCol], (size_t)(tickets * TR + 1) * sizeof(int))) != GSA_SUCCESS) return s;
    unsigned long long* const dgran = ctx->buf[kBufGran].as<unsigned long long>();
    unsigned long long* const sctl = ctx->buf[kBufSctl].as<unsigned long long>();
    a.pairs = ddesc;
    a.nPairs = 1;
    a.nTicketsTotal = (int)tickets;
    a.gran = dgran;
    a.gran2 = dgran + gran;
    a.ticket = ctx->ctl;
    a.err = (unsigned*)(sctl + 3);  // the score kernels' own error word (score_ag_strip)
    a.spin = ctx->spin_ticks;
    a.agResult = (int*)sctl;
    a.swBest = sctl + 1;
    a.idxBits = sw_idx_bits(R, C);
    a.rowR = ctx->buf[kBufBidi].as<int>();
    if (overlap) a.tapH = ctx->buf[kBufOvCol].as<int>();  // (no tap: tapRow stays 0)
    a.epoch = ++ctx->epoch;
    if (a.epoch == 0) a.epoch = ++ctx->epoch;
    if ((e = hipMemsetAsync(ctx->ctl, 0, 4, st)) != hipSuccess || (e = hipMemsetAsync(sctl, 0, 32, st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    (void)hipEventRecord(ctx->ev0, st);
    const int grid = std::max(1, std::min((int)tickets, ctx->cu_count));
    const int mode = overlap ? (gapo == gape ? gsa::kModeScoreOVL : gsa::kModeScoreOV)
                             : (gapo == gape ? gsa::kModeScoreSGL : gsa::kModeScoreSG);
    // the int8 profile as score_ag_strip picks it (GSA_KROW_Q8)
    const int q8env = env_int(ctx, "GSA_KROW_Q8", 1);
    a.q8 = (q8env != 0 && (q8env == 2 || scoreK == 4) && gsa::krow_score_lds_bytes(substsz, true) <= (size_t)ctx->lds_max) ? 1 : 0;
    a.q8flag = ctx->ctl + 2;
    // (overlap: score, i_end, j_end in the three ints at sctl; the error word at sctl + 3 stays clear of them)
    if (overlap ? ((e = gsa::launch_krow_score_overlap(a, mode, scoreK, grid, st)) != hipSuccess ||
                   (e = gsa::launch_overlap_max(a.rowR, a.tapH, (int)R, (int)C, gapo, gape, (int*)sctl, st)) != hipSuccess)
                : ((e = gsa::launch_krow_score_semi(a, mode, scoreK, grid, st)) != hipSuccess ||
                   (e = gsa::launch_semi_rowmax(a.rowR, (int)R, (int)C, gapo, gape, (int*)sctl, (int*)(sctl + 1), st)) != hipSuccess))
        return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    note_launch(ctx);
    (void)hipEventRecord(ctx->ev1, st);
    unsigned long long res[4] = {0, 0, 0, 0};
    if ((e = hipMemcpyAsync(res, sctl, sizeof(res), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    (void)hipEventElapsedTime(&out->calc_kernel_ms, ctx->ev0, ctx->ev1);
    if ((unsigned)res[3] != 0) return GSA_ERROR_KERNEL_FAILURE;
    out->score = (int32_t)(uint32_t)res[0];
    if (overlap)
    {
        out->i_end = (int64_t)(int32_t)(uint32_t)(res[0] >> 32);
        out->j_end = (int64_t)(int32_t)(uint32_t)res[1];
        // a cell of row R or of column C, and never a negative score
        if (out->score < 0 || out->i_end < 0 || out->i_end > R || out->j_end < 0 || out->j_end > C ||
            (out->i_end != R && out->j_end != C))
            return GSA_ERROR_KERNEL_FAILURE;
        return GSA_SUCCESS;
    }
    out->i_end = R;
    out->j_end = (int64_t)(int32_t)(uint32_t)res[1];
    if (out->j_end < 0 || out->j_end > C) return GSA_ERROR_KERNEL_FAILURE;
    return GSA_SUCCESS;
}

int score_semi_impl(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                    const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, gsa_score_result* out, hipStream_t st)
{
    if (!ctx || !seqY || !seqX || !subst || !out) return GSA_ERROR_INVALID_VALUE;
    const int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    const int64_t R = adjrows - 1, C = adjcols - 1;
    out->calc_kernel_ms = 0.f;
    if (R == 0 || C == 0)
    {
        // an empty side, answered on the host as the database calls answer it
        out->score = R == 0 ? 0 : (int32_t)(gapo + (R - 1) * gape);
        out->i_end = R;
        out->j_end = 0;
        return GSA_SUCCESS;
    }
    return semi_pair_score(ctx, seqY, R, seqX, C, subst, substsz, gapo, gape, false, out, st, nullptr);
}


// gsa_align_pair_semi_dev's unit (nw_pair_semi_trace.hip): rows 1 ... R over the columns of the window.
// The walk never leaves the window (the bound excludes it) and ends in row 0.
struct SemiTrace
{
    using FillArgs = gsa::SemiFillArgs;
    using WalkArgs = gsa::SemiWalkArgs;
    using WalkRec = gsa::SemiWalkRec;
    static void mode_args(const PairTrace& t, FillArgs& f, WalkArgs& w)
    {
        f.R = (int)t.R;
        f.jW = w.jW = (int)t.jW;
    }
    static hipError_t launch(const PairTrace& t, const FillArgs& f, const WalkArgs& w, hipEvent_t* ev, hipStream_t st)
    {
        int grid = 1;
        const hipError_t e = gsa::semi_fill_grid(t.gapo != t.gape, t.KR, f.nstrips, &grid);
        return e != hipSuccess ? e : gsa::launch_semi_trace(f, w, t.KR, grid, ev, st);
    }
    static bool rec_ok(const PairTrace&, const gsa::PairChunk&, const WalkRec& r) { return !r.left; }
    static bool go_on(const PairTrace& t, int64_t TR, const gsa::PairChunk& ch, const WalkRec& r)
    {
        return ch.tLo >= 1 && r.i == gsa::pair_chunk_stop_row(TR, ch) && r.j > t.jW && r.j <= t.jW + ch.J;
    }
    static bool end_ok(const WalkRec& r) { return r.i == 0; }
};

// gsa_align_pair_semi_dev: score and end column from semi_pair_score, whose checkpoint rows stay in
// kBufGran; the column window from the score (nw_pair_semi_plan.h); then trace_pair from (R, j_end) over
// the window, up to row 0.  gsa_last_launch's record is left as it was.
int align_pair_semi_impl(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                         const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int64_t scratch_limit,
                         gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                         gsa_align_pair_semi_info* info, float* kernel_ms, hipStream_t st)
{
    if (!ctx || !seqY || !seqX || !subst || !out) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    if (scratch_limit < 0 || cigar_cap < 0 || (cigar_cap > 0 && !cigar)) return GSA_ERROR_INVALID_VALUE;
    if (kernel_ms) *kernel_ms = 0.f;
    if (cigar_need) *cigar_need = 0;
    gsa_align_pair_semi_info inf;
    std::memset(&inf, 0, sizeof(inf));
    if (info) *info = inf;
    const int64_t R = adjrows - 1, C = adjcols - 1;
    const int64_t limit = scratch_limit > 0 ? scratch_limit : (int64_t)gsa::kPairTraceScratch;
    gsa_align_db_result r;
    std::memset(&r, 0, sizeof(r));
    std::string cig;
    if (R == 0 || C == 0)
    {
        // an empty side, answered on the host as the database calls answer it
        if (R > 0)
        {
            r.score = (int32_t)(gapo + (R - 1) * gape);
            r.i_end = R;
            cig = std::to_string(R) + 'I';
        }
    }
    else
    {
        gsa_score_result sr {};
        SemiRoute route;
        if ((s = semi_pair_score(ctx, seqY, R, seqX, C, subst, substsz, gapo, gape, true, &sr, st, &route)) != GSA_SUCCESS)
            return s;
        const KeepLaunchRecord keep(ctx);
        inf.score_ms = sr.calc_kernel_ms;
        r.score = sr.score;
        r.i_end = R;
        r.j_end = sr.j_end;
        const int KR = route.K * gsa::kSparseNS;
        const int64_t TR = 64 * (int64_t)KR;
        const int64_t jEnd = sr.j_end;
        const int64_t strips = gsa::pair_strips(TR, R);
        inf.strip_rows = (int32_t)TR;
        inf.strips = (int32_t)strips;
        if (jEnd == 0)
            cig = std::to_string(R) + 'I';  // the all-insert alignment on column 0: no codes
        else
        {
            const int64_t jW = gsa::semi_window(R, jEnd, sr.score, route.pmax, gape);
            inf.j_window = jW;
            gsa::PairChunk ch;
            // (a limit below one strip's windowed codes: known only once the score is)
            if (!gsa::semi_plan_chunk(TR, strips - 1, jEnd, jW, limit, &ch)) return GSA_ERROR_INVALID_VALUE;
            const PairTrace t {seqY, seqX, subst, substsz, gapo, gape, 0, R, C, R, jEnd, jW, KR, route.tickets, limit};
            if ((s = trace_pair<SemiTrace>(ctx, t, ch, &inf, &r, &cig, st)) != GSA_SUCCESS) return s;
        }
    }
    return finish_pair(r, cig, inf, out, cigar, cigar_cap, cigar_need, info, kernel_ms);
}


// gsa_score_overlap_dev: an empty side on the host (score 0 at (R, 0)), otherwise semi_pair_score on the
// overlap instances.
int score_overlap_impl(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                       const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, gsa_score_result* out, hipStream_t st)
{
    if (!ctx || !seqY || !seqX || !subst || !out) return GSA_ERROR_INVALID_VALUE;
    const int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    const int64_t R = adjrows - 1, C = adjcols - 1;
    out->calc_kernel_ms = 0.f;
    if (R == 0 || C == 0)
    {
        // an empty side: every candidate is 0, and row R's first cell wins
        out->score = 0;
        out->i_end = R;
        out->j_end = 0;
        return GSA_SUCCESS;
    }
    return semi_pair_score(ctx, seqY, R, seqX, C, subst, substsz, gapo, gape, false, out, st, nullptr, true);
}

// gsa_align_pair_overlap_dev's unit (nw_pair_overlap_trace.hip): rows 1 ... iEnd from column 1.  The walk
// ends as soon as it stands on row 0 or on column 0, whatever strips lie above.
struct OverlapTrace
{
    using FillArgs = gsa::OverlapFillArgs;
    using WalkArgs = gsa::OverlapWalkArgs;
    using WalkRec = gsa::OverlapWalkRec;
    static void mode_args(const PairTrace& t, FillArgs& f, WalkArgs&) { f.iEnd = (int)t.iEnd; }
    static hipError_t launch(const PairTrace& t, const FillArgs& f, const WalkArgs& w, hipEvent_t* ev, hipStream_t st)
    {
        int grid = 1;
        const hipError_t e = gsa::overlap_fill_grid(t.gapo != t.gape, t.KR, f.nstrips, &grid);
        return e != hipSuccess ? e : gsa::launch_overlap_trace(f, w, t.KR, grid, ev, st);
    }
    static bool rec_ok(const PairTrace& t, const gsa::PairChunk& ch, const WalkRec& r)
    {
        return r.i >= 0 && r.i <= t.iEnd && r.j >= 0 && r.j <= ch.J;
    }
    static bool go_on(const PairTrace&, int64_t TR, const gsa::PairChunk& ch, const WalkRec& r)
    {
        return gsa::overlap_walk_goes_on(TR, ch, r.i, r.j);
    }
    static bool end_ok(const WalkRec& r) { return r.i == 0 || r.j == 0; }
};

// gsa_align_pair_overlap_dev: score and end cell from semi_pair_score's overlap launch, whose checkpoint
// rows stay in kBufGran; then trace_pair from the end cell, bottom-up from i_end's strip, until the walk
// stands on row 0 or on column 0.  gsa_last_launch's record is left as it was.
int align_pair_overlap_impl(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                            const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int64_t scratch_limit,
                            gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                            gsa_align_pair_overlap_info* info, float* kernel_ms, hipStream_t st)
{
    if (!ctx || !seqY || !seqX || !subst || !out) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    if (scratch_limit < 0 || cigar_cap < 0 || (cigar_cap > 0 && !cigar)) return GSA_ERROR_INVALID_VALUE;
    if (kernel_ms) *kernel_ms = 0.f;
    if (cigar_need) *cigar_need = 0;
    gsa_align_pair_overlap_info inf;
    std::memset(&inf, 0, sizeof(inf));
    if (info) *info = inf;
    const int64_t R = adjrows - 1, C = adjcols - 1;
    const int64_t limit = scratch_limit > 0 ? scratch_limit : (int64_t)gsa::kPairTraceScratch;
    gsa_align_db_result r;
    std::memset(&r, 0, sizeof(r));
    // (an empty side, or score 0: the cells (R, 0)-(R, 0) and an empty CIGAR)
    r.i_start = r.i_end = R;
    std::string cig;
    if (R > 0 && C > 0)
    {
        gsa_score_result sr {};
        SemiRoute route;
        if ((s = semi_pair_score(ctx, seqY, R, seqX, C, subst, substsz, gapo, gape, true, &sr, st, &route, true)) != GSA_SUCCESS)
            return s;
        const KeepLaunchRecord keep(ctx);
        inf.score_ms = sr.calc_kernel_ms;
        r.score = sr.score;
        r.i_end = r.i_start = sr.i_end;
        r.j_end = r.j_start = sr.j_end;
        const int KR = route.K * gsa::kSparseNS;
        const int64_t TR = 64 * (int64_t)KR;
        const int64_t iEnd = sr.i_end, jEnd = sr.j_end;
        inf.strip_rows = (int32_t)TR;
        inf.strips = (int32_t)gsa::pair_strips(TR, iEnd);
        // an end cell on a free border (score 0 at (R, 0), by the tie rule): no path, no codes
        if (iEnd > 0 && jEnd > 0)
        {
            gsa::PairChunk ch;
            // (a limit below one strip's codes: known only once j_end is)
            if (!gsa::overlap_plan_chunk(TR, gsa::overlap_end_strip(TR, iEnd), jEnd, limit, &ch)) return GSA_ERROR_INVALID_VALUE;
            const PairTrace t {seqY, seqX, subst, substsz, gapo, gape, 0, R, C, iEnd, jEnd, 0, KR, route.tickets, limit};
            if ((s = trace_pair<OverlapTrace>(ctx, t, ch, &inf, &r, &cig, st)) != GSA_SUCCESS) return s;
        }
    }
    return finish_pair(r, cig, inf, out, cigar, cigar_cap, cigar_need, info, kernel_ms);
}


// What score_semi_batch_impl's launch ran (gsa_align_batch_semi_dev and gsa_align_batch_overlap_dev read
// the checkpoint rows it left in kBufGran: pair p's row t at granOff[p] + t gran_stride(C), the affine
// second array granTotal words behind).
struct SemiBatchRoute
{
    int K = 0;                       // rows per lane of the K-rows launch; 0: nothing was launched
    long long granTotal = 0;         // words of the first array, over all pairs
    long long pmax = 0;              // max(0, largest table value): the windows' bound (nw_pair_semi_plan.h); overlap: unused
    std::vector<int> tickets;        // per pair of the call: its tickets (0: an empty side)
    std::vector<long long> granOff;  // its first row, in words
};

// gsa_score_semi_batch_dev: score_batch_impl and semi_pair_score side by side.  Pairs with an empty side
// on the host; for the others the range tests of a mode without a second path, per pair, then the
// batched semi-global instances of the K-rows score kernel in one launch (every pair's row R into its
// own part of kBufBidi, PairDesc::score) and one workgroup per pair that takes the row's first maximum;
// one copy brings every score and end column back.  The answers, the host's included, are written once
// nothing can refuse the call any more: a refusal leaves out as it was.  gsa_last_launch's record and
// the fills' sticky error word are left alone.
// overlap (gsa_score_overlap_batch_dev): the same tests and geometry on the batched overlap instances,
// which store column C of every row of every one of a pair's tickets into its own part of kBufOvCol
// (PairDesc::hcol) as well; the workgroup behind them takes the first maximum over row R and column C
// and brings the end cell's row back too.  An empty side scores 0 at (R, 0).
int score_semi_batch_impl(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                          int32_t gapo, int32_t gape, bool forAlign, gsa_score_result* out, float* batch_ms, hipStream_t st,
                          SemiBatchRoute* route = nullptr, bool overlap = false)
{
    if (!ctx || !pairs || !subst || !out || npairs < 1) return GSA_ERROR_INVALID_VALUE;
    if (substsz < 1 || substsz > 32) return GSA_ERROR_INVALID_VALUE;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    for (int p = 0; p < npairs; ++p)
        if (pairs[p].adjrows < 1 || pairs[p].adjcols < 1 || !pairs[p].seqY || !pairs[p].seqX) return GSA_ERROR_INVALID_VALUE;
    if (batch_ms) *batch_ms = 0.f;
    if (route)
    {
        *route = SemiBatchRoute {};
        route->tickets.assign((size_t)npairs, 0);
        route->granOff.assign((size_t)npairs, 0);
    }
    std::vector<int> bp;
    for (int p = 0; p < npairs; ++p)
        if (pairs[p].adjrows > 1 && pairs[p].adjcols > 1) bp.push_back(p);
    // an empty side, answered on the host as score_semi_impl and score_overlap_impl answer it
    auto host_pairs = [&]() {
        for (int p = 0; p < npairs; ++p)
        {
            const int64_t R = pairs[p].adjrows - 1, C = pairs[p].adjcols - 1;
            out[p].calc_kernel_ms = 0.f;
            if (R == 0 || C == 0)
            {
                out[p].score = (overlap || R == 0) ? 0 : (int32_t)(gapo + (R - 1) * gape);
                out[p].i_end = R;
                out[p].j_end = 0;
            }
        }
    };
    if (bp.empty())
    {
        host_pairs();
        return GSA_SUCCESS;
    }
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
    std::vector<int32_t> sub((size_t)substsz * (size_t)substsz);
    if ((e = hipMemcpyAsync(sub.data(), subst, sub.size() * 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    const long long smax = subst_absmax(sub.data(), substsz);
    if (gsa::krow_score_lds_bytes(substsz) > (size_t)ctx->lds_max) return GSA_ERROR_INVALID_VALUE;
    // the kernel's own test of the shifted table (nw_kscore_kernel: error bit 2)
    for (const int32_t v0 : sub)
    {
        const long long v = (long long)v0 - gapo - gape;
        if (v <= -32768 || v > 32767) return GSA_ERROR_INVALID_VALUE;
    }
    // rows per lane as score_batch_impl picks them: 4 in both gap models
    const int kenv = env_int(ctx, "GSA_SCORE_K", 0);
    const int scoreK = kenv == 2 ? 2 : 4;
    const int64_t TR = (int64_t)(64 * scoreK) * gsa::kSparseNS;
    const int nb = (int)bp.size();
    std::vector<gsa::PairDesc> hd;
    std::vector<long long> rowOff, colOff;  // ints: the pair's row within kBufBidi (a multiple of 16), its column within kBufOvCol
    long long tickets = 0, gran = 0, rowInts = 0, colInts = 0;
    for (int p : bp)
    {
        const int64_t R = pairs[p].adjrows - 1, C = pairs[p].adjcols - 1;
        // semi_pair_score's tests, per pair
        bool stripOk = false;
        const int s = score_ranges(R, C, smax, gapo, gape, 0, &stripOk);
        if (s != GSA_SUCCESS) return s;
        if (!stripOk) return GSA_ERROR_INVALID_VALUE;  // span < 2^28: the shifted values' room in int32
        // the fill keeps 4 x value + source (align_pair_impl's bound)
        if (forAlign && smax * std::min(R, C) + (long long)(-gapo) + (R + C) * (long long)(-gape) >= gsa::kDbTraceMaxValue)
            return GSA_ERROR_INVALID_VALUE;
        gsa::PairDesc d;
        std::memset(&d, 0, sizeof(d));
        d.seqY = pairs[p].seqY;
        d.seqX = pairs[p].seqX;
        d.R = (int)R;
        d.C = (int)C;
        d.Cp = (int)C;
        d.nTickets = (int)((R + TR - 1) / TR);
        d.ticketBase = (int)tickets;
        d.granOff = gran;
        tickets += d.nTickets;
        gran += (long long)d.nTickets * gsa::gran_stride(d.Cp);
        if (tickets > (1ll << 30) || C > (1ll << 30)) return GSA_ERROR_INVALID_VALUE;
        // row R: columns -kTapPad .. C + 79, as the tap rows
        rowOff.push_back(rowInts);
        rowInts += ((long long)gsa::kTapPad + C + 80 + 15) & ~15ll;
        // overlap, column C: the rows 0 ... nTickets TR -- every strip of every ticket stores its K words per
        // lane, rows past R included, so the pair's last ticket counts whole; a column starts at a multiple
        // of 16 ints, which keeps every store the alignment it has in the single call
        colOff.push_back(colInts);
        colInts += (1 + (long long)d.nTickets * TR + 15) & ~15ll;
        hd.push_back(d);
    }
    // every buffer before anything is launched
    int s;
    if ((s = reserve_hard(ctx, ctx->buf[kBufBidi], (size_t)rowInts * sizeof(int))) != GSA_SUCCESS) return s;
    if (overlap && (s = reserve_hard(ctx, ctx->buf[kBufOvCol], (size_t)colInts * sizeof(int))) != GSA_SUCCESS) return s;
    int* const rows = ctx->buf[kBufBidi].as<int>();
    int* const cols = overlap ? ctx->buf[kBufOvCol].as<int>() : nullptr;
    for (int i = 0; i < nb; ++i)
    {
        hd[(size_t)i].score = rows + rowOff[(size_t)i];
        if (overlap) hd[(size_t)i].hcol = cols + colOff[(size_t)i];
    }
    if ((s = ensure_gran(ctx, 2 * (size_t)gran, st)) != GSA_SUCCESS) return s;
    if ((s = reserve_hard(ctx, ctx->buf[kBufSctl], 64)) != GSA_SUCCESS) return s;
    // two result words per pair (unused by these modes), then the answers and the error word's
    const size_t resBytes = (size_t)nb * 2 * sizeof(unsigned long long);
    const size_t outBytes = ((size_t)nb + 1) * sizeof(gsa::ScoreOut);
    if ((s = reserve_hard(ctx, ctx->buf[kBufSbatch], resBytes + outBytes, 4096)) != GSA_SUCCESS) return s;
    const std::vector<int> sched = batch_schedule(ctx, hd, tickets);
    if ((s = stage_descs(ctx, hd, sched, st)) != GSA_SUCCESS) return s;
    if (route)
    {
        route->K = scoreK;
        route->granTotal = gran;
        route->pmax = std::max<long long>(0, *std::max_element(sub.begin(), sub.end()));
        for (int i = 0; i < nb; ++i)
        {
            route->tickets[(size_t)bp[(size_t)i]] = hd[(size_t)i].nTickets;
            route->granOff[(size_t)bp[(size_t)i]] = hd[(size_t)i].granOff;
        }
    }
    const KeepLaunchRecord keep(ctx);
    gsa::PairDesc* const ddesc = ctx->buf[kBufDesc].as<gsa::PairDesc>();
    unsigned long long* const dgran = ctx->buf[kBufGran].as<unsigned long long>();
    unsigned long long* const sctl = ctx->buf[kBufSctl].as<unsigned long long>();
    unsigned long long* const res = ctx->buf[kBufSbatch].as<unsigned long long>();
    gsa::ScoreOut* const dout = (gsa::ScoreOut*)(ctx->buf[kBufSbatch].as<char>() + resBytes);
    gsa::StripArgs a;
    std::memset(&a, 0, sizeof(a));
    a.subst = subst;
    a.substsz = substsz;
    a.g = gapo;
    a.go = gapo;
    a.ge = gape;
    a.ns = gsa::kSparseNS;
    a.pairs = ddesc;
    a.nPairs = nb;
    a.nTicketsTotal = (int)tickets;
    a.sched = sched.empty() ? nullptr : (const int*)(ddesc + nb);
    a.gran = dgran;
    a.gran2 = dgran + gran;
    a.ticket = ctx->ctl;
    a.err = (unsigned*)(sctl + 3);  // the score kernels' own error word (score_ag_strip)
    a.spin = ctx->spin_ticks;
    a.swBest = res;
    a.rowR = rows;  // (every pair's own row and column come from its descriptor)
    a.tapH = cols;  // (overlap; no tap: tapRow stays 0)
    a.epoch = ++ctx->epoch;
    if (a.epoch == 0) a.epoch = ++ctx->epoch;
    if ((e = hipMemsetAsync(ctx->ctl, 0, 4, st)) != hipSuccess || (e = hipMemsetAsync(sctl, 0, 32, st)) != hipSuccess ||
        (e = hipMemsetAsync(res, 0, resBytes, st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
    (void)hipEventRecord(ctx->ev0, st);
    const bool linear = gapo == gape;
    const int mode = overlap ? (linear ? gsa::kModeScoreOVL : gsa::kModeScoreOV) : (linear ? gsa::kModeScoreSGL : gsa::kModeScoreSG);
    // the int8 profile for linear gaps only, as score_batch_impl picks it.  GSA_KROW_Q8=0 / 2: int16 / int8 always
    const int q8env = env_int(ctx, "GSA_KROW_Q8", 1);
    a.q8 = (q8env != 0 && (q8env == 2 || linear) && gsa::krow_score_lds_bytes(substsz, true) <= (size_t)ctx->lds_max) ? 1 : 0;
    a.q8flag = ctx->ctl + 2;
    // one pair: one workgroup per CU (its tickets are a chain); a batch: all resident slots
    const int grid = nb == 1 ? std::max(1, std::min((int)tickets, ctx->cu_count)) : 0;
    if (overlap ? ((e = gsa::launch_krow_score_overlap_batch(a, mode, scoreK, grid, st)) != hipSuccess ||
                   (e = gsa::launch_overlap_max_batch(ddesc, nb, gapo, gape, a.err, dout, st)) != hipSuccess)
                : ((e = gsa::launch_krow_score_semi_batch(a, mode, scoreK, grid, st)) != hipSuccess ||
                   (e = gsa::launch_semi_rowmax_batch(ddesc, nb, gapo, gape, a.err, dout, st)) != hipSuccess))
        return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    note_launch(ctx);
    (void)hipEventRecord(ctx->ev1, st);
    std::vector<gsa::ScoreOut> ho((size_t)nb + 1);
    if ((e = hipMemcpyAsync(ho.data(), dout, outBytes, hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    if (batch_ms) *batch_ms = ms;
    if ((unsigned)ho[(size_t)nb].score != 0) return GSA_ERROR_KERNEL_FAILURE;
    // semi-global: a column of row R; overlap: a cell of row R or of column C, and never a negative score
    for (int i = 0; i < nb; ++i)
    {
        const gsa::ScoreOut& o = ho[(size_t)i];
        const int R = hd[(size_t)i].R, C = hd[(size_t)i].C;
        if (o.j_end < 0 || o.j_end > C) return GSA_ERROR_KERNEL_FAILURE;
        if (overlap && (o.score < 0 || o.i_end < 0 || o.i_end > R || (o.i_end != R && o.j_end != C))) return GSA_ERROR_KERNEL_FAILURE;
    }
    host_pairs();
    for (int i = 0; i < nb; ++i)
    {
        const gsa::ScoreOut& o = ho[(size_t)i];
        gsa_score_result& r = out[bp[(size_t)i]];
        r.score = o.score;
        r.i_end = overlap ? o.i_end : hd[(size_t)i].R;
        r.j_end = o.j_end;
    }
    return GSA_SUCCESS;
}

// gsa_align_batch_semi_dev's unit (nw_pair_semi_trace_batch.hip): every pair over its own window; a
// finished walk stands in row 0
struct SemiBatchTrace
{
    using Desc = gsa::SemiBatchDesc;
    using Walk = gsa::SemiBatchWalk;
    using FillArgs = gsa::SemiBatchFillArgs;
    using WalkArgs = gsa::SemiBatchWalkArgs;
    using WalkRec = gsa::SemiWalkRec;
    static gsa::PairBatchDesc& base(Desc& d) { return d.p; }
    static void window(const BatchTracePair& B, Desc& d, Walk& w) { d.jW = w.jW = (int)B.jW; }
    static hipError_t launch(const BatchTrace& t, const FillArgs& f, const WalkArgs& w, int walkGrid, hipEvent_t* ev, hipStream_t st)
    {
        int grid = 1;
        const hipError_t e = gsa::semi_batch_fill_grid(t.gapo != t.gape, t.KR, f.ntasks, t.max_workgroups, &grid);
        return e != hipSuccess ? e : gsa::launch_semi_batch_trace(f, w, t.KR, grid, walkGrid, ev, st);
    }
    static bool rec_ok(const WalkRec& r) { return !r.left; }
    static bool advance(long long TR, const gsa::PairChunk& c, long long i, long long j, bool done, gsa::BatchPairState* s)
    {
        return gsa::semi_batch_advance(TR, c, i, j, done, s);
    }
};

// gsa_align_batch_semi_dev: every pair's score and end column from score_semi_batch_impl, whose
// checkpoint rows stay in kBufGran, every pair in its own granules; each pair's column window from its
// own score (nw_pair_semi_plan.h); then trace_batch over the pairs with a path right of column 0 whose
// one strip fits the limit (the others: the host's answer, or status 1).  gsa_last_launch's record is
// left as it was.
int align_batch_semi_impl(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                          int32_t gapo, int32_t gape, int32_t max_workgroups, int64_t scratch_limit,
                          gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                          gsa_align_batch_semi_info* info, float* kernel_ms, hipStream_t st)
{
    if (!ctx || !pairs || !subst || !out || npairs < 1) return GSA_ERROR_INVALID_VALUE;
    if (substsz < 1 || substsz > 32) return GSA_ERROR_INVALID_VALUE;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    for (int p = 0; p < npairs; ++p)
        if (pairs[p].adjrows < 1 || pairs[p].adjcols < 1 || !pairs[p].seqY || !pairs[p].seqX) return GSA_ERROR_INVALID_VALUE;
    if (scratch_limit < 0 || cigar_cap < 0 || max_workgroups < 0 || (cigar_cap > 0 && !cigar)) return GSA_ERROR_INVALID_VALUE;
    if (kernel_ms) *kernel_ms = 0.f;
    if (cigar_need) *cigar_need = 0;
    gsa_align_batch_semi_info inf;
    std::memset(&inf, 0, sizeof(inf));
    if (info) *info = inf;
    const int64_t limit = scratch_limit > 0 ? scratch_limit : (int64_t)gsa::kPairBatchScratch;
    std::vector<gsa_align_db_result> res((size_t)npairs);
    std::memset(res.data(), 0, res.size() * sizeof(gsa_align_db_result));
    std::vector<std::string> cig((size_t)npairs);
    const KeepLaunchRecord keep(ctx);
    SemiBatchRoute route;
    std::vector<gsa_score_result> sres((size_t)npairs);
    int s = score_semi_batch_impl(ctx, npairs, pairs, subst, substsz, gapo, gape, true, sres.data(), &inf.score_ms, st, &route);
    if (s != GSA_SUCCESS) return s;
    const int K = route.K;
    const int KR = K * gsa::kSparseNS;
    const int64_t TR = 64 * (int64_t)KR;
    inf.strip_rows = (int32_t)TR;                   // (0: every pair has an empty side)
    inf.gran_bytes = 16 * (int64_t)route.granTotal;  // both arrays, 8-byte words
    // the traced pairs: letters on both sides, an end cell right of column 0, one strip within the limit
    std::vector<BatchTracePair> bp;
    for (int p = 0; p < npairs; ++p)
    {
        const int64_t R = pairs[p].adjrows - 1, C = pairs[p].adjcols - 1;
        gsa_align_db_result& r = res[(size_t)p];
        r.score = sres[(size_t)p].score;
        r.i_end = sres[(size_t)p].i_end;
        r.j_end = sres[(size_t)p].j_end;
        if (R == 0 || C == 0 || r.j_end == 0)
        {
            // an empty side, or the all-insert alignment on column 0: no codes
            if (R > 0) cig[(size_t)p] = std::to_string(R) + 'I';
            inf.host_pairs += 1;
            continue;
        }
        if (!(K == 2 || K == 4)) return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);
        const int64_t jW = gsa::semi_window(R, r.j_end, r.score, route.pmax, gape);
        if (gsa::pair_strip_bytes(TR, r.j_end - jW) > limit)
        {
            r.status = 1;  // one strip's windowed codes exceed the limit: score and end cell only
            continue;
        }
        bp.push_back(BatchTracePair {p, R, r.j_end, jW, route.granOff[(size_t)p]});
        inf.window_cols += r.j_end - jW;
    }
    if (!bp.empty())
    {
        const BatchTrace t {pairs, subst, substsz, gapo, gape, 0, max_workgroups, KR, route.granTotal, limit};
        if ((s = trace_batch<SemiBatchTrace>(ctx, t, bp, &inf, res.data(), cig.data(), st)) != GSA_SUCCESS) return s;
    }
    finish_batch(res, cig, inf, out, cigar, cigar_cap, cigar_need, info);
    if (kernel_ms) *kernel_ms = inf.score_ms + inf.fill_ms + inf.walk_ms;
    return GSA_SUCCESS;
}


// gsa_align_batch_overlap_dev's unit (nw_pair_overlap_trace_batch.hip): gsa_align_batch_dev's descriptors;
// a finished walk stands on row 0 or on column 0
struct OverlapBatchTrace
{
    using Desc = gsa::PairBatchDesc;
    using Walk = gsa::OverlapBatchWalk;
    using FillArgs = gsa::OverlapBatchFillArgs;
    using WalkArgs = gsa::OverlapBatchWalkArgs;
    using WalkRec = gsa::OverlapWalkRec;
    static gsa::PairBatchDesc& base(Desc& d) { return d; }
    static void window(const BatchTracePair&, Desc&, Walk&) {}
    static hipError_t launch(const BatchTrace& t, const FillArgs& f, const WalkArgs& w, int walkGrid, hipEvent_t* ev, hipStream_t st)
    {
        int grid = 1;
        const hipError_t e = gsa::overlap_batch_fill_grid(t.gapo != t.gape, t.KR, f.ntasks, t.max_workgroups, &grid);
        return e != hipSuccess ? e : gsa::launch_overlap_batch_trace(f, w, t.KR, grid, walkGrid, ev, st);
    }
    static bool rec_ok(const WalkRec&) { return true; }
    static bool advance(long long TR, const gsa::PairChunk& c, long long i, long long j, bool done, gsa::BatchPairState* s)
    {
        return gsa::overlap_batch_advance(TR, c, i, j, done, s);
    }
};

// gsa_align_batch_overlap_dev: every pair's score and end cell from score_semi_batch_impl's overlap
// launch, whose checkpoint rows stay in kBufGran, every pair in its own granules; then trace_batch,
// bottom-up from each pair's end row's strip, over the pairs whose end cell lies off both free borders
// and whose one strip fits the limit (the others: the host's answer, or status 1).  gsa_last_launch's
// record is left as it was.
int align_batch_overlap_impl(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                             int32_t gapo, int32_t gape, int32_t max_workgroups, int64_t scratch_limit,
                             gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                             gsa_align_batch_overlap_info* info, float* kernel_ms, hipStream_t st)
{
    if (!ctx || !pairs || !subst || !out || npairs < 1) return GSA_ERROR_INVALID_VALUE;
    if (substsz < 1 || substsz > 32) return GSA_ERROR_INVALID_VALUE;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    for (int p = 0; p < npairs; ++p)
        if (pairs[p].adjrows < 1 || pairs[p].adjcols < 1 || !pairs[p].seqY || !pairs[p].seqX) return GSA_ERROR_INVALID_VALUE;
    if (scratch_limit < 0 || cigar_cap < 0 || max_workgroups < 0 || (cigar_cap > 0 && !cigar)) return GSA_ERROR_INVALID_VALUE;
    if (kernel_ms) *kernel_ms = 0.f;
    if (cigar_need) *cigar_need = 0;
    gsa_align_batch_overlap_info inf;
    std::memset(&inf, 0, sizeof(inf));
    if (info) *info = inf;
    const int64_t limit = scratch_limit > 0 ? scratch_limit : (int64_t)gsa::kPairBatchScratch;
    std::vector<gsa_align_db_result> res((size_t)npairs);
    std::memset(res.data(), 0, res.size() * sizeof(gsa_align_db_result));
    std::vector<std::string> cig((size_t)npairs);
    const KeepLaunchRecord keep(ctx);
    SemiBatchRoute route;
    std::vector<gsa_score_result> sres((size_t)npairs);
    int s = score_semi_batch_impl(ctx, npairs, pairs, subst, substsz, gapo, gape, true, sres.data(), &inf.score_ms, st, &route,
                                  true);
    if (s != GSA_SUCCESS) return s;
    const int K = route.K;
    const int KR = K * gsa::kSparseNS;
    const int64_t TR = 64 * (int64_t)KR;
    inf.strip_rows = (int32_t)TR;                    // (0: every pair has an empty side)
    inf.gran_bytes = 16 * (int64_t)route.granTotal;  // both arrays, 8-byte words
    // the traced pairs: an end cell off both free borders, one strip within the limit
    std::vector<BatchTracePair> bp;
    for (int p = 0; p < npairs; ++p)
    {
        gsa_align_db_result& r = res[(size_t)p];
        r.score = sres[(size_t)p].score;
        r.i_end = r.i_start = sres[(size_t)p].i_end;
        r.j_end = r.j_start = sres[(size_t)p].j_end;
        if (r.i_end == 0 || r.j_end == 0)
        {
            // an empty side, or score 0 at (R, 0) by the tie rule: no path, no codes
            inf.host_pairs += 1;
            continue;
        }
        if (!(K == 2 || K == 4)) return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);
        if (gsa::pair_strip_bytes(TR, r.j_end) > limit)
        {
            r.status = 1;  // one strip's codes exceed the limit: score and end cell only
            r.i_start = r.j_start = 0;
            continue;
        }
        bp.push_back(BatchTracePair {p, r.i_end, r.j_end, 0, route.granOff[(size_t)p]});
    }
    if (!bp.empty())
    {
        const BatchTrace t {pairs, subst, substsz, gapo, gape, 0, max_workgroups, KR, route.granTotal, limit};
        if ((s = trace_batch<OverlapBatchTrace>(ctx, t, bp, &inf, res.data(), cig.data(), st)) != GSA_SUCCESS) return s;
    }
    finish_batch(res, cig, inf, out, cigar, cigar_cap, cigar_need, info);
    if (kernel_ms) *kernel_ms = inf.score_ms + inf.fill_ms + inf.walk_ms;
    return GSA_SUCCESS;
}

// The info structs of the banded calls (EXT false) and of the banded extension calls (EXT true).
template <bool EXT>
struct BandInfoOf
{
    using pair = gsa_align_pair_band_info;
    using batch_pair = gsa_align_batch_band_pair;
    using batch = gsa_align_batch_band_info;
};
template <>
struct BandInfoOf<true>
{
    using pair = gsa_align_pair_band_ext_info;
    using batch_pair = gsa_align_batch_band_ext_pair;
    using batch = gsa_align_batch_band_ext_info;
};

// An end cell the extension fill reported: inside the (trimmed) matrix and inside the band.
inline bool band_ext_end_ok(int64_t i, int64_t j, int64_t R, int64_t C, int64_t lo, int64_t hi)
{
    return i >= 0 && i <= R && j >= 0 && j <= C && j - i >= lo && j - i <= hi;
}

// gsa_score_band_dev and gsa_align_pair_band_dev (align: the latter): the checks, the plan
// (nw_band_plan.h), one fill launch of one workgroup -- with move codes when the alignment is wanted
// and the 4 v + tag form and scratch_limit take them -- and, with codes, the walk; one copy brings the
// score and the walk's record back, a second the move bytes.  The certificate is computed here.
// Scratch: kBufPairMeta ([0] the result words, [64] the walk's record, [128] the pair's descriptor),
// kBufPairCodes, kBufPairMoves.  gsa_last_launch's record is not touched.
//
// EXT: gsa_score_band_ext_dev and gsa_align_pair_band_ext_dev, the same steps on the
// part of the pair the band reaches (nw_band_ext_plan.h: R, C below are R', C'; R0, C0 the whole pair),
// with the fill that keeps the band's best cell (nw_band_ext.hip) and the walk from that cell.
template <bool EXT>
int band_impl(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols, const int32_t* subst,
              int32_t substsz, int32_t gapo, int32_t gape, int64_t band_lo, int64_t band_hi, bool align, int64_t scratch_limit,
              gsa_score_result* sout, gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
              typename BandInfoOf<EXT>::pair* info, float* kernel_ms, hipStream_t st)
{
    if (!ctx || !seqY || !seqX || !subst || (align ? !out : !sout)) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    if (align && (scratch_limit < 0 || cigar_cap < 0 || (cigar_cap > 0 && !cigar))) return GSA_ERROR_INVALID_VALUE;
    const int64_t R0 = adjrows - 1, C0 = adjcols - 1;
    if (R0 >= (1ll << 30) || C0 >= (1ll << 30)) return GSA_ERROR_INVALID_VALUE;  // the kernel's int32 cell indices
    if (!(EXT ? gsa::band_ext_valid(band_lo, band_hi) : gsa::band_valid(R0, C0, band_lo, band_hi))) return GSA_ERROR_INVALID_VALUE;
    gsa::band_clamp(R0, C0, &band_lo, &band_hi);
    int64_t R = R0, C = C0;
    if (EXT) gsa::band_ext_trim(R0, C0, band_lo, band_hi, &R, &C);
    if (kernel_ms) *kernel_ms = 0.f;
    if (cigar_need) *cigar_need = 0;
    typename BandInfoOf<EXT>::pair inf;
    std::memset(&inf, 0, sizeof(inf));
    inf.band_lo = band_lo;
    inf.band_hi = band_hi;
    if constexpr (EXT)
    {
        inf.rows_used = R;
        inf.cols_used = C;
    }
    gsa_align_db_result r;
    std::memset(&r, 0, sizeof(r));
    r.i_end = EXT ? 0 : R;
    r.j_end = EXT ? 0 : C;
    std::string cig;
    if (EXT && (R == 0 || C == 0))
        inf.proved_optimal = 1;  // an empty side: score 0 at (0, 0), an empty CIGAR
    else if (R == 0 || C == 0)
    {
        // one boundary, answered on the host: row 0 is E only, column 0 F only; no path leaves the band.  The
        // one gap run is held to gsa_score_dev's value range (no table value takes part: smax = 1)
        const int64_t k = R + C;
        bool stripOk = false;
        if (k > 0 && (s = score_ranges(R, C, 1, gapo, gape, 0, &stripOk)) != GSA_SUCCESS) return s;
        if (k > 0)
        {
            r.score = (int32_t)(gapo + (k - 1) * gape);
            cig = std::to_string(k) + (R > 0 ? 'I' : 'D');
        }
        inf.proved_optimal = 1;
    }
    else
    {
        gsa::BandPlan plan;
        if (!gsa::band_plan(R, C, band_lo, band_hi, &plan)) return GSA_ERROR_INVALID_VALUE;  // wider than the limit
        hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
        std::vector<int32_t> sub((size_t)substsz * (size_t)substsz);
        if ((e = hipMemcpyAsync(sub.data(), subst, sub.size() * 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        const long long smax = subst_absmax(sub.data(), substsz);
        const long long pmax = std::max<long long>(0, *std::max_element(sub.begin(), sub.end()));
        bool stripOk = false;
        if ((s = score_ranges(R, C, smax, gapo, gape, 0, &stripOk)) != GSA_SUCCESS) return s;
        // the fill with codes keeps 4 x value + source: |H| <= B (score_ranges' bound, which holds in the band)
        const bool valOk = smax * std::min(R, C) + (long long)(-gapo) + (R + C) * (long long)(-gape) < gsa::kDbTraceMaxValue;
        const int64_t limit = scratch_limit > 0 ? scratch_limit : gsa::kBandScratch;
        const bool codes = align && valOk && plan.codeBytes <= limit;
        inf.strip_rows = gsa::kBandTR;
        inf.strips = (int32_t)plan.strips;
        inf.waves = plan.waves;
        inf.supersteps = (int32_t)plan.T;
        inf.code_bytes = plan.codeBytes;
        if ((s = reserve_hard(ctx, ctx->buf[kBufPairMeta], 4096)) != GSA_SUCCESS) return s;
        if (codes && ((s = reserve_hard(ctx, ctx->buf[kBufPairCodes], (size_t)plan.codeBytes, 4096)) != GSA_SUCCESS ||
                      (s = reserve_hard(ctx, ctx->buf[kBufPairMoves], (size_t)(R + C), 4096)) != GSA_SUCCESS))
            return s;
        if (const int es = ensure_trace_events(ctx); es != GSA_SUCCESS) return es;
        char* const meta = ctx->buf[kBufPairMeta].as<char>();
        gsa::BandWalkRec* const drec = (gsa::BandWalkRec*)(meta + 64);
        gsa::BandDesc* const ddesc = (gsa::BandDesc*)(meta + 128);
        static_assert(sizeof(gsa::BandWalkRec) <= 64 && sizeof(gsa::BandDesc) <= 128, "the slots of kBufPairMeta");
        gsa::BandDesc d;
        std::memset(&d, 0, sizeof(d));
        d.seqY = seqY;
        d.seqX = seqX;
        d.codes = codes ? ctx->buf[kBufPairCodes].as<unsigned char>() : nullptr;
        d.result = (int*)meta;
        d.stripBytes = plan.stripBytes;
        d.R = (int)R;
        d.C = (int)C;
        d.lo = (int)plan.lo;
        d.hi = (int)plan.hi;
        d.strips = (int)plan.strips;
        d.nq = (int)plan.nq;
        d.T = (int)plan.T;
        d.Wc = (int)plan.Wc;
        gsa::BandWalkArgs w;
        std::memset(&w, 0, sizeof(w));
        w.seqY = seqY;
        w.seqX = seqX;
        w.codes = d.codes;
        w.stripBytes = plan.stripBytes;
        w.R = d.R;
        w.C = d.C;
        w.lo = d.lo;
        w.hi = d.hi;
        w.rec = drec;
        w.moves = ctx->buf[kBufPairMoves].as<unsigned char>();
        w.start = EXT ? (const int*)meta : nullptr;
        // the result words and the walk's record start from zero: a kernel that wrote nothing is seen
        if ((e = hipMemsetAsync(meta, 0, 128, st)) != hipSuccess ||
            (e = hipMemcpyAsync(ddesc, &d, sizeof(d), hipMemcpyHostToDevice, st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        if ((e = (EXT ? gsa::launch_band_ext : gsa::launch_band)(ddesc, 1, plan.waves, subst, substsz, gapo, gape, codes,
                                                                 codes ? &w : nullptr, ctx->adbev, st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        note_launch(ctx);
        struct
        {
            int res[16];
            gsa::BandWalkRec rec;
        } back;
        static_assert(sizeof(back) == 64 + sizeof(gsa::BandWalkRec), "the first two slots of kBufPairMeta");
        if ((e = hipMemcpyAsync(&back, meta, sizeof(back), hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        (void)hipEventElapsedTime(&inf.score_ms, ctx->adbev[0], ctx->adbev[1]);
        if (codes) (void)hipEventElapsedTime(&inf.walk_ms, ctx->adbev[1], ctx->adbev[2]);
        if (back.res[1] != 1) return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);
        r.score = back.res[0];
        r.status = codes ? 0 : 1;
        if (EXT)
        {
            r.i_end = back.res[2];
            r.j_end = back.res[3];
            if (!band_ext_end_ok(r.i_end, r.j_end, R, C, plan.lo, plan.hi) || r.score < 0)
                return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);
        }
        if (codes)
        {
            const gsa::BandWalkRec& rec = back.rec;
            // a step off the band, a record out of range, or a walk that did not end at (0, 0)
            if (rec.offband || !rec.done || rec.n < 0 || rec.n > r.i_end + r.j_end || rec.i != 0 || rec.j != 0)
                return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);
            std::vector<unsigned char> mv((size_t)rec.n + 1);
            if (rec.n > 0 &&
                ((e = hipMemcpyAsync(mv.data(), ctx->buf[kBufPairMoves].p, (size_t)rec.n, hipMemcpyDeviceToHost, st)) != hipSuccess ||
                 (e = hipStreamSynchronize(st)) != hipSuccess))
                return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
            cig = fold_cigar(mv.data(), rec.n);
        }
        inf.proved_optimal = EXT ? gsa::band_ext_certificate(R0, C0, plan.lo, plan.hi, pmax, gapo, gape, r.score)
                                 : gsa::band_certificate(R, C, plan.lo, plan.hi, pmax, gapo, gape, r.score);
    }
    if (!align)
    {
        sout->score = r.score;
        sout->i_end = r.i_end;
        sout->j_end = r.j_end;
        sout->calc_kernel_ms = inf.score_ms;
        return GSA_SUCCESS;
    }
    const int64_t need = pack_cigars(&r, &cig, 1, cigar, cigar_cap);
    if (cigar_need) *cigar_need = need;
    *out = r;
    if (info) *info = inf;
    if (kernel_ms) *kernel_ms = inf.score_ms + inf.walk_ms;
    return GSA_SUCCESS;
}

// gsa_score_band_batch_dev and gsa_align_batch_band_dev (align: the latter): every pair is
// checked and planned as band_impl does (nothing is enqueued before all passed), the pairs with an empty
// side are answered here, the others run on nw_band_batch.hip: one launch without codes for the pairs
// that get none (all pairs of the score call), then the rounds of nw_band_batch_plan.h, each one upload,
// one fill launch, one walk launch and one copy back.  Scratch: kBufPairBatchTab ([0] the claim counter,
// [64] the round's descriptors, then its walk arguments), kBufPairBatchRec (the round's result words,
// walk records and move bytes, copied back as one), kBufPairCodes.  gsa_last_launch's record is not
// touched.
//
// EXT: gsa_score_band_ext_batch_dev and gsa_align_batch_band_ext_dev, as band_impl<true>
// does it per pair: the trimmed pair (b.R, b.C; b.R0, b.C0 the whole one), four result words per pair,
// nw_band_ext_batch.hip's launches, the walks from the end cells.
template <bool EXT>
int band_batch_impl(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                    int32_t gapo, int32_t gape, const int64_t* band_lo, const int64_t* band_hi, int32_t waves,
                    int32_t max_workgroups, bool align, int64_t scratch_limit, gsa_score_result* sout, gsa_align_db_result* out,
                    char* cigar, int64_t cigar_cap, int64_t* cigar_need, typename BandInfoOf<EXT>::batch_pair* pair_info,
                    typename BandInfoOf<EXT>::batch* info, float* kernel_ms, hipStream_t st)
{
    if (!ctx || npairs < 0 || !pairs || !subst || !band_lo || !band_hi || (align ? !out : !sout)) return GSA_ERROR_INVALID_VALUE;
    if (substsz < 1 || substsz > 32) return GSA_ERROR_INVALID_VALUE;
    if (gapo > gape || gape > 0) return GSA_ERROR_INVALID_VALUE;  // go <= ge <= 0
    if (max_workgroups < 0 || (waves != 0 && waves != 4 && waves != 8 && waves != 16)) return GSA_ERROR_INVALID_VALUE;
    if (align && (scratch_limit < 0 || cigar_cap < 0 || (cigar_cap > 0 && !cigar))) return GSA_ERROR_INVALID_VALUE;
    struct Bp
    {
        int64_t R, C, R0, C0;
        gsa::BandPlan plan;  // (lo, hi: also of a pair with an empty side)
        bool host, codes;
    };
    std::vector<Bp> bp((size_t)npairs);
    bool anyDev = false;
    for (int p = 0; p < npairs; ++p)
    {
        if (pairs[p].adjrows < 1 || pairs[p].adjcols < 1 || !pairs[p].seqY || !pairs[p].seqX) return GSA_ERROR_INVALID_VALUE;
        Bp& b = bp[(size_t)p];
        b.R = pairs[p].adjrows - 1;
        b.C = pairs[p].adjcols - 1;
        if (b.R >= (1ll << 30) || b.C >= (1ll << 30)) return GSA_ERROR_INVALID_VALUE;  // the kernel's int32 cell indices
        int64_t lo = band_lo[p], hi = band_hi[p];
        if (!(EXT ? gsa::band_ext_valid(lo, hi) : gsa::band_valid(b.R, b.C, lo, hi))) return GSA_ERROR_INVALID_VALUE;
        gsa::band_clamp(b.R, b.C, &lo, &hi);
        b.R0 = b.R;
        b.C0 = b.C;
        if (EXT) gsa::band_ext_trim(b.R0, b.C0, lo, hi, &b.R, &b.C);
        b.host = b.R == 0 || b.C == 0;
        b.codes = false;
        if (b.host)
        {
            b.plan.lo = lo;
            b.plan.hi = hi;
            bool stripOk = false;
            if (!EXT && b.R + b.C > 0 && score_ranges(b.R, b.C, 1, gapo, gape, 0, &stripOk) != GSA_SUCCESS) return GSA_ERROR_INVALID_VALUE;
        }
        else
        {
            if (!gsa::band_plan(b.R, b.C, lo, hi, &b.plan)) return GSA_ERROR_INVALID_VALUE;  // wider than the limit
            if (waves != 0 && !gsa::band_waves_ok(waves, b.plan.strips, b.plan.nq)) return GSA_ERROR_INVALID_VALUE;
            anyDev = true;
        }
    }
    const int64_t limit = scratch_limit > 0 ? scratch_limit : gsa::kBandBatchScratch;
    hipError_t e = hipSuccess;
    long long pmax = 0;
    if (anyDev)
    {
        if ((e = hipSetDevice(ctx->device)) != hipSuccess) return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
        std::vector<int32_t> sub((size_t)substsz * (size_t)substsz);
        if ((e = hipMemcpyAsync(sub.data(), subst, sub.size() * 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        const long long smax = subst_absmax(sub.data(), substsz);
        pmax = std::max<long long>(0, *std::max_element(sub.begin(), sub.end()));
        for (Bp& b : bp)
        {
            if (b.host) continue;
            bool stripOk = false;
            const int s = score_ranges(b.R, b.C, smax, gapo, gape, 0, &stripOk);
            if (s != GSA_SUCCESS) return s;
            // the fill with codes keeps 4 x value + source: |H| <= B (score_ranges' bound, which holds in the band)
            const bool valOk =
                smax * std::min(b.R, b.C) + (long long)(-gapo) + (b.R + b.C) * (long long)(-gape) < gsa::kDbTraceMaxValue;
            b.codes = align && valOk && b.plan.codeBytes <= limit;
        }
    }
    // every pair passed: from here on the call answers
    if (kernel_ms) *kernel_ms = 0.f;
    if (cigar_need) *cigar_need = 0;
    typename BandInfoOf<EXT>::batch inf;
    std::memset(&inf, 0, sizeof(inf));
    std::vector<gsa_align_db_result> res((size_t)npairs);
    if (npairs > 0) std::memset(res.data(), 0, res.size() * sizeof(gsa_align_db_result));
    std::vector<std::string> cig((size_t)npairs);
    std::vector<int> roundOf((size_t)npairs, -1);
    std::vector<int64_t> codeBytes((size_t)npairs, -1);
    std::vector<int> nocode;
    for (int p = 0; p < npairs; ++p)
    {
        const Bp& b = bp[(size_t)p];
        gsa_align_db_result& r = res[(size_t)p];
        r.i_end = EXT ? 0 : b.R;
        r.j_end = EXT ? 0 : b.C;
        if constexpr (EXT)
        {
            inf.rows_used += b.host ? 0 : b.R;
            inf.cols_used += b.host ? 0 : b.C;
        }
        if (b.host)
        {
            // one boundary, answered on the host as band_impl does: row 0 is E only, column 0 F only
            const int64_t k = b.R + b.C;
            if (!EXT && k > 0)
            {
                r.score = (int32_t)(gapo + (k - 1) * gape);
                cig[(size_t)p] = std::to_string(k) + (b.R > 0 ? 'I' : 'D');
            }
            inf.host_pairs += 1;
        }
        else if (b.codes)
            codeBytes[(size_t)p] = b.plan.codeBytes;
        else
        {
            nocode.push_back(p);
            roundOf[(size_t)p] = -2;
            r.status = 1;
        }
    }
    const gsa::BandBatchRounds rounds = gsa::band_batch_rounds(codeBytes, limit);
    if (!rounds.nocode.empty()) return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);  // (b.codes holds the limit)
    inf.nocode_pairs = align ? (int32_t)nocode.size() : 0;
    inf.rounds = (int32_t)rounds.rounds.size();
    inf.code_bytes = rounds.peakBytes;
    if (anyDev)
    {
        inf.strip_rows = gsa::kBandTR;
        if (const int es = ensure_trace_events(ctx); es != GSA_SUCCESS) return es;
    }
    // launch 0: the pairs without codes; then the rounds
    std::vector<char> blob, back;
    for (size_t l = 0; l < 1 + rounds.rounds.size(); ++l)
    {
        const bool codes = l > 0;
        const std::vector<int>& members = codes ? rounds.rounds[l - 1] : nocode;
        if (members.empty()) continue;
        const size_t n = members.size();
        // the order the workgroups claim the pairs in, and the waves all of them can run on
        std::vector<int64_t> T(n), strips(n), nq(n);
        for (size_t k = 0; k < n; ++k)
        {
            const gsa::BandPlan& pl = bp[(size_t)members[k]].plan;
            T[k] = pl.T;
            strips[k] = pl.strips;
            nq[k] = pl.nq;
        }
        const std::vector<int> order = gsa::band_batch_order(T);
        const int nwv = gsa::band_batch_pick_waves(waves, strips.data(), nq.data(), n);
        if (nwv == 0) return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);  // (checked per pair above)
        inf.waves = std::max(inf.waves, nwv);
        // the device tables: [counter | descriptors | walk arguments] and [result words | records | moves]
        const size_t descOff = 64, walkOff = descOff + ((n * sizeof(gsa::BandDesc) + 63) & ~(size_t)63);
        const size_t tabBytes = walkOff + (codes ? n * sizeof(gsa::BandWalkArgs) : 0);
        constexpr size_t kWords = EXT ? 4 : 2;  // result words of a pair
        const size_t recOff = (n * kWords * 4 + 63) & ~(size_t)63, movOff = recOff + (codes ? n * sizeof(gsa::BandWalkRec) : 0);
        std::vector<int64_t> mvAt(n, 0), cdAt(n, 0);
        int64_t movTotal = 0, codeTotal = 0;
        if (codes)
            for (size_t k = 0; k < n; ++k)
            {
                const Bp& b = bp[(size_t)members[(size_t)order[k]]];
                mvAt[k] = movTotal;
                cdAt[k] = codeTotal;
                movTotal += b.R + b.C;
                codeTotal += b.plan.codeBytes;
            }
        int s;
        if ((s = reserve_hard(ctx, ctx->buf[kBufPairBatchTab], tabBytes, 4096)) != GSA_SUCCESS ||
            (s = reserve_hard(ctx, ctx->buf[kBufPairBatchRec], movOff + (size_t)movTotal, 4096)) != GSA_SUCCESS ||
            (codes && (s = reserve_hard(ctx, ctx->buf[kBufPairCodes], (size_t)codeTotal, 4096)) != GSA_SUCCESS))
            return s;
        char* const dtab = ctx->buf[kBufPairBatchTab].as<char>();
        char* const drec = ctx->buf[kBufPairBatchRec].as<char>();
        unsigned char* const dcodes = ctx->buf[kBufPairCodes].as<unsigned char>();
        blob.assign(tabBytes, 0);
        for (size_t k = 0; k < n; ++k)
        {
            const int p = members[(size_t)order[k]];
            const Bp& b = bp[(size_t)p];
            gsa::BandDesc d;
            std::memset(&d, 0, sizeof(d));
            d.seqY = pairs[p].seqY;
            d.seqX = pairs[p].seqX;
            d.codes = codes ? dcodes + cdAt[k] : nullptr;
            d.result = (int*)drec + kWords * k;
            d.stripBytes = b.plan.stripBytes;
            d.R = (int)b.R;
            d.C = (int)b.C;
            d.lo = (int)b.plan.lo;
            d.hi = (int)b.plan.hi;
            d.strips = (int)b.plan.strips;
            d.nq = (int)b.plan.nq;
            d.T = (int)b.plan.T;
            d.Wc = (int)b.plan.Wc;
            std::memcpy(blob.data() + descOff + k * sizeof(d), &d, sizeof(d));
            if (!codes) continue;
            gsa::BandWalkArgs w;
            std::memset(&w, 0, sizeof(w));
            w.seqY = d.seqY;
            w.seqX = d.seqX;
            w.codes = d.codes;
            w.stripBytes = d.stripBytes;
            w.R = d.R;
            w.C = d.C;
            w.lo = d.lo;
            w.hi = d.hi;
            w.rec = (gsa::BandWalkRec*)(drec + recOff) + k;
            w.moves = (unsigned char*)drec + movOff + mvAt[k];
            w.start = EXT ? d.result : nullptr;
            std::memcpy(blob.data() + walkOff + k * sizeof(w), &w, sizeof(w));
        }
        int grid = 0, walkGrid = (int)std::min<size_t>(n, 65535);
        if (max_workgroups > 0) walkGrid = std::min(walkGrid, (int)max_workgroups);
        if ((e = (EXT ? gsa::band_ext_batch_fill_grid : gsa::band_batch_fill_grid)(gapo != gape, codes, nwv, (int)n, max_workgroups, &grid)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_CUDA_GENERAL);
        // the result words and the walks' records start from zero: a kernel that wrote nothing is seen
        if ((e = hipMemsetAsync(drec, 0, movOff, st)) != hipSuccess ||
            (e = hipMemcpyAsync(dtab, blob.data(), tabBytes, hipMemcpyHostToDevice, st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_MEMORY_TRANSFER);
        if ((e = (EXT ? gsa::launch_band_ext_batch : gsa::launch_band_batch)(
                 (const gsa::BandDesc*)(dtab + descOff), (int)n, (unsigned*)dtab, nwv, grid, subst, substsz, gapo, gape, codes,
                 codes ? (const gsa::BandWalkArgs*)(dtab + walkOff) : nullptr, walkGrid, ctx->adbev, st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        note_launch(ctx);
        back.resize(movOff + (size_t)movTotal);
        if ((e = hipMemcpyAsync(back.data(), drec, back.size(), hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(ctx, e, GSA_ERROR_KERNEL_FAILURE);
        float fill = 0.f, walk = 0.f;
        (void)hipEventElapsedTime(&fill, ctx->adbev[0], ctx->adbev[1]);
        if (codes) (void)hipEventElapsedTime(&walk, ctx->adbev[1], ctx->adbev[2]);
        (codes ? inf.fill_ms : inf.nocode_ms) += fill;
        inf.walk_ms += walk;
        const int* const words = (const int*)back.data();
        for (size_t k = 0; k < n; ++k)
        {
            const int p = members[(size_t)order[k]];
            const Bp& b = bp[(size_t)p];
            if (words[kWords * k + 1] != 1) return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);
            gsa_align_db_result& r = res[(size_t)p];
            r.score = words[kWords * k];
            if (EXT)
            {
                r.i_end = words[kWords * k + 2];
                r.j_end = words[kWords * k + 3];
                if (!band_ext_end_ok(r.i_end, r.j_end, b.R, b.C, b.plan.lo, b.plan.hi) || r.score < 0)
                    return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);
            }
            if (!codes) continue;
            roundOf[(size_t)p] = (int)l - 1;
            gsa::BandWalkRec rec;
            std::memcpy(&rec, back.data() + recOff + k * sizeof(rec), sizeof(rec));
            // a step off the band, a record out of range, or a walk that did not end at (0, 0)
            if (rec.offband || !rec.done || rec.n < 0 || rec.n > r.i_end + r.j_end || rec.i != 0 || rec.j != 0)
                return fail(ctx, hipErrorUnknown, GSA_ERROR_KERNEL_FAILURE);
            cig[(size_t)p] = fold_cigar((const unsigned char*)back.data() + movOff + mvAt[k], rec.n);
        }
        if (codes) inf.batch_pairs += (int32_t)n;
    }
    if (!align)
    {
        for (int p = 0; p < npairs; ++p)
        {
            sout[p].score = res[(size_t)p].score;
            sout[p].i_end = res[(size_t)p].i_end;
            sout[p].j_end = res[(size_t)p].j_end;
            sout[p].calc_kernel_ms = 0.f;
        }
        if (kernel_ms) *kernel_ms = inf.nocode_ms;
        return GSA_SUCCESS;
    }
    const int64_t at = pack_cigars(res.data(), cig.data(), npairs, cigar, cigar_cap);
    for (int p = 0; p < npairs; ++p)
    {
        const gsa_align_db_result& r = res[(size_t)p];
        const Bp& b = bp[(size_t)p];
        out[p] = r;
        if (pair_info)
        {
            typename BandInfoOf<EXT>::batch_pair& pi = pair_info[p];
            std::memset(&pi, 0, sizeof(pi));
            pi.band_lo = b.plan.lo;
            pi.band_hi = b.plan.hi;
            pi.round = roundOf[(size_t)p];
            pi.proved_optimal = 1;
            if constexpr (EXT)
            {
                pi.rows_used = b.R;
                pi.cols_used = b.C;
            }
            if (!b.host)
            {
                pi.code_bytes = b.plan.codeBytes;
                pi.strips = (int32_t)b.plan.strips;
                pi.supersteps = (int32_t)b.plan.T;
                pi.proved_optimal = EXT ? gsa::band_ext_certificate(b.R0, b.C0, b.plan.lo, b.plan.hi, pmax, gapo, gape, r.score)
                                        : gsa::band_certificate(b.R, b.C, b.plan.lo, b.plan.hi, pmax, gapo, gape, r.score);
            }
        }
    }
    if (cigar_need) *cigar_need = at;
    if (info) *info = inf;
    if (kernel_ms) *kernel_ms = inf.nocode_ms + inf.fill_ms + inf.walk_ms;
    return GSA_SUCCESS;
}

}  // namespace

extern "C" {

int64_t gsa_band_max_width(void) { return gsa::kBandMaxWidth; }

int gsa_score_band_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                       const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int64_t band_lo, int64_t band_hi,
                       gsa_score_result* out, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return band_impl<false>(ctx, seqY, adjrows, seqX, adjcols, subst, substsz, gapo, gape, band_lo, band_hi, false, 0, out, nullptr,
                     nullptr, 0, nullptr, nullptr, nullptr, pick_stream(ctx, stream));
}

int gsa_align_pair_band_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                            const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int64_t band_lo, int64_t band_hi,
                            int64_t scratch_limit, gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                            gsa_align_pair_band_info* info, float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return band_impl<false>(ctx, seqY, adjrows, seqX, adjcols, subst, substsz, gapo, gape, band_lo, band_hi, true, scratch_limit,
                     nullptr, out, cigar, cigar_cap, cigar_need, info, kernel_ms, pick_stream(ctx, stream));
}

int gsa_score_band_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                             int32_t gapo, int32_t gape, const int64_t* band_lo, const int64_t* band_hi, int32_t waves,
                             int32_t max_workgroups, gsa_score_result* out, float* batch_kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return band_batch_impl<false>(ctx, npairs, pairs, subst, substsz, gapo, gape, band_lo, band_hi, waves, max_workgroups, false, 0, out,
                           nullptr, nullptr, 0, nullptr, nullptr, nullptr, batch_kernel_ms, pick_stream(ctx, stream));
}

int gsa_align_batch_band_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                             int32_t gapo, int32_t gape, const int64_t* band_lo, const int64_t* band_hi, int32_t waves,
                             int32_t max_workgroups, int64_t scratch_limit, gsa_align_db_result* out, char* cigar,
                             int64_t cigar_cap, int64_t* cigar_need, gsa_align_batch_band_pair* pair_info,
                             gsa_align_batch_band_info* info, float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return band_batch_impl<false>(ctx, npairs, pairs, subst, substsz, gapo, gape, band_lo, band_hi, waves, max_workgroups, true,
                           scratch_limit, nullptr, out, cigar, cigar_cap, cigar_need, pair_info, info, kernel_ms,
                           pick_stream(ctx, stream));
}

int gsa_score_band_ext_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                           const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int64_t band_lo, int64_t band_hi,
                           gsa_score_result* out, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return band_impl<true>(ctx, seqY, adjrows, seqX, adjcols, subst, substsz, gapo, gape, band_lo, band_hi, false, 0, out, nullptr,
                           nullptr, 0, nullptr, nullptr, nullptr, pick_stream(ctx, stream));
}

int gsa_align_pair_band_ext_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                                const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int64_t band_lo,
                                int64_t band_hi, int64_t scratch_limit, gsa_align_db_result* out, char* cigar, int64_t cigar_cap,
                                int64_t* cigar_need, gsa_align_pair_band_ext_info* info, float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return band_impl<true>(ctx, seqY, adjrows, seqX, adjcols, subst, substsz, gapo, gape, band_lo, band_hi, true, scratch_limit,
                           nullptr, out, cigar, cigar_cap, cigar_need, info, kernel_ms, pick_stream(ctx, stream));
}

int gsa_score_band_ext_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                                 int32_t gapo, int32_t gape, const int64_t* band_lo, const int64_t* band_hi, int32_t waves,
                                 int32_t max_workgroups, gsa_score_result* out, float* batch_kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return band_batch_impl<true>(ctx, npairs, pairs, subst, substsz, gapo, gape, band_lo, band_hi, waves, max_workgroups, false, 0,
                                 out, nullptr, nullptr, 0, nullptr, nullptr, nullptr, batch_kernel_ms, pick_stream(ctx, stream));
}

int gsa_align_batch_band_ext_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                                 int32_t gapo, int32_t gape, const int64_t* band_lo, const int64_t* band_hi, int32_t waves,
                                 int32_t max_workgroups, int64_t scratch_limit, gsa_align_db_result* out, char* cigar,
                                 int64_t cigar_cap, int64_t* cigar_need, gsa_align_batch_band_ext_pair* pair_info,
                                 gsa_align_batch_band_ext_info* info, float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return band_batch_impl<true>(ctx, npairs, pairs, subst, substsz, gapo, gape, band_lo, band_hi, waves, max_workgroups, true,
                                 scratch_limit, nullptr, out, cigar, cigar_cap, cigar_need, pair_info, info, kernel_ms,
                                 pick_stream(ctx, stream));
}

int gsa_align_batch_overlap_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                                int32_t gapo, int32_t gape, int32_t max_workgroups, int64_t scratch_limit,
                                gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                                gsa_align_batch_overlap_info* info, float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return align_batch_overlap_impl(ctx, npairs, pairs, subst, substsz, gapo, gape, max_workgroups, scratch_limit, out, cigar,
                                    cigar_cap, cigar_need, info, kernel_ms, pick_stream(ctx, stream));
}

int gsa_score_overlap_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                                int32_t gapo, int32_t gape, gsa_score_result* out, float* batch_kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return score_semi_batch_impl(ctx, npairs, pairs, subst, substsz, gapo, gape, false, out, batch_kernel_ms,
                                 pick_stream(ctx, stream), nullptr, true);
}

int gsa_align_batch_semi_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                             int32_t gapo, int32_t gape, int32_t max_workgroups, int64_t scratch_limit,
                             gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                             gsa_align_batch_semi_info* info, float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return align_batch_semi_impl(ctx, npairs, pairs, subst, substsz, gapo, gape, max_workgroups, scratch_limit, out, cigar,
                                 cigar_cap, cigar_need, info, kernel_ms, pick_stream(ctx, stream));
}

int gsa_score_semi_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                             int32_t gapo, int32_t gape, gsa_score_result* out, float* batch_kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return score_semi_batch_impl(ctx, npairs, pairs, subst, substsz, gapo, gape, false, out, batch_kernel_ms,
                                 pick_stream(ctx, stream));
}

int gsa_align_pair_semi_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                            const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int64_t scratch_limit,
                            gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                            gsa_align_pair_semi_info* info, float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return align_pair_semi_impl(ctx, seqY, adjrows, seqX, adjcols, subst, substsz, gapo, gape, scratch_limit, out, cigar,
                                cigar_cap, cigar_need, info, kernel_ms, pick_stream(ctx, stream));
}

int gsa_align_pair_overlap_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                               const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int64_t scratch_limit,
                               gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                               gsa_align_pair_overlap_info* info, float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return align_pair_overlap_impl(ctx, seqY, adjrows, seqX, adjcols, subst, substsz, gapo, gape, scratch_limit, out, cigar,
                                   cigar_cap, cigar_need, info, kernel_ms, pick_stream(ctx, stream));
}

int gsa_score_overlap_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                          const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, gsa_score_result* out,
                          void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return score_overlap_impl(ctx, seqY, adjrows, seqX, adjcols, subst, substsz, gapo, gape, out, pick_stream(ctx, stream));
}

int gsa_score_semi_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                       const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, gsa_score_result* out,
                       void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return score_semi_impl(ctx, seqY, adjrows, seqX, adjcols, subst, substsz, gapo, gape, out, pick_stream(ctx, stream));
}

int gsa_align_pair_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                       const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int32_t local,
                       int64_t scratch_limit, gsa_align_db_result* out, char* cigar, int64_t cigar_cap,
                       int64_t* cigar_need, gsa_align_pair_info* info, float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return align_pair_impl(ctx, seqY, adjrows, seqX, adjcols, subst, substsz, gapo, gape, local, scratch_limit, out, cigar,
                           cigar_cap, cigar_need, info, kernel_ms, pick_stream(ctx, stream));
}

int gsa_align_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                        int32_t gapo, int32_t gape, int32_t local, int32_t max_workgroups, int64_t scratch_limit,
                        gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                        gsa_align_batch_info* info, float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return align_batch_impl(ctx, npairs, pairs, subst, substsz, gapo, gape, local, max_workgroups, scratch_limit, out, cigar,
                            cigar_cap, cigar_need, info, kernel_ms, pick_stream(ctx, stream));
}

int gsa_align_db_multi_dev(gsa_ctx* ctx, const int32_t* queries, const int64_t* q_off, int32_t nq, const int32_t* db,
                           const int64_t* db_off, int32_t nsubj, const int32_t* hit_query, const int32_t* hit_subject,
                           int32_t nhits, const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape,
                           int32_t local, int32_t max_workgroups, int64_t scratch_limit, gsa_align_db_result* out,
                           char* cigar, int64_t cigar_cap, int64_t* cigar_need, gsa_align_db_multi_info* info,
                           float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return align_db_multi_impl(ctx, queries, q_off, nq, db, db_off, nsubj, hit_query, hit_subject, nhits, subst, substsz,
                               gapo, gape, local, DbShape::plain, max_workgroups, scratch_limit, out, cigar, cigar_cap,
                               cigar_need, info, kernel_ms, pick_stream(ctx, stream));
}

int gsa_align_db_multi_semi_dev(gsa_ctx* ctx, const int32_t* queries, const int64_t* q_off, int32_t nq,
                                const int32_t* db, const int64_t* db_off, int32_t nsubj, const int32_t* hit_query,
                                const int32_t* hit_subject, int32_t nhits, const int32_t* subst, int32_t substsz,
                                int32_t gapo, int32_t gape, int32_t max_workgroups, int64_t scratch_limit,
                                gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                                gsa_align_db_multi_info* info, float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return align_db_multi_impl(ctx, queries, q_off, nq, db, db_off, nsubj, hit_query, hit_subject, nhits, subst, substsz,
                               gapo, gape, 0, DbShape::semi, max_workgroups, scratch_limit, out, cigar, cigar_cap, cigar_need,
                               info, kernel_ms, pick_stream(ctx, stream));
}

int gsa_align_db_multi_overlap_dev(gsa_ctx* ctx, const int32_t* queries, const int64_t* q_off, int32_t nq,
                                   const int32_t* db, const int64_t* db_off, int32_t nsubj, const int32_t* hit_query,
                                   const int32_t* hit_subject, int32_t nhits, const int32_t* subst, int32_t substsz,
                                   int32_t gapo, int32_t gape, int32_t max_workgroups, int64_t scratch_limit,
                                   gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                                   gsa_align_db_multi_info* info, float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return align_db_multi_impl(ctx, queries, q_off, nq, db, db_off, nsubj, hit_query, hit_subject, nhits, subst, substsz,
                               gapo, gape, 0, DbShape::overlap, max_workgroups, scratch_limit, out, cigar, cigar_cap,
                               cigar_need, info, kernel_ms, pick_stream(ctx, stream));
}

int32_t gsa_align_db_multi_unit(void) { return gsa::kDbAlignMultiUnit; }

int gsa_score_db_multi_dev(gsa_ctx* ctx, const int32_t* queries, const int64_t* q_off, int32_t nq, const int32_t* db,
                           const int64_t* db_off, int32_t nsubj, const int32_t* subst, int32_t substsz, int32_t gapo,
                           int32_t gape, int32_t local, int32_t top, int32_t max_workgroups, int64_t scratch_limit,
                           int32_t* scores, gsa_db_hit* hits, gsa_score_db_multi_info* info, float* kernel_ms,
                           void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return score_db_multi_impl(ctx, queries, q_off, nq, db, db_off, nsubj, subst, substsz, gapo, gape, local, DbShape::plain,
                               top, max_workgroups, scratch_limit, scores, hits, info, kernel_ms, pick_stream(ctx, stream));
}

int gsa_score_db_multi_semi_dev(gsa_ctx* ctx, const int32_t* queries, const int64_t* q_off, int32_t nq,
                                const int32_t* db, const int64_t* db_off, int32_t nsubj, const int32_t* subst,
                                int32_t substsz, int32_t gapo, int32_t gape, int32_t top, int32_t max_workgroups,
                                int64_t scratch_limit, int32_t* scores, gsa_db_hit* hits, gsa_score_db_multi_info* info,
                                float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return score_db_multi_impl(ctx, queries, q_off, nq, db, db_off, nsubj, subst, substsz, gapo, gape, 0, DbShape::semi, top,
                               max_workgroups, scratch_limit, scores, hits, info, kernel_ms, pick_stream(ctx, stream));
}

int gsa_score_db_multi_overlap_dev(gsa_ctx* ctx, const int32_t* queries, const int64_t* q_off, int32_t nq,
                                   const int32_t* db, const int64_t* db_off, int32_t nsubj, const int32_t* subst,
                                   int32_t substsz, int32_t gapo, int32_t gape, int32_t top, int32_t max_workgroups,
                                   int64_t scratch_limit, int32_t* scores, gsa_db_hit* hits,
                                   gsa_score_db_multi_info* info, float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return score_db_multi_impl(ctx, queries, q_off, nq, db, db_off, nsubj, subst, substsz, gapo, gape, 0, DbShape::overlap,
                               top, max_workgroups, scratch_limit, scores, hits, info, kernel_ms, pick_stream(ctx, stream));
}

int32_t gsa_score_db_multi_unit(void) { return gsa::kDbMultiUnit; }

int gsa_align_db_dev(gsa_ctx* ctx, const int32_t* query, int32_t adjq, const int32_t* db, const int64_t* db_off,
                     int32_t nsubj, const int32_t* hits, int32_t nhits, const int32_t* subst, int32_t substsz,
                     int32_t gapo, int32_t gape, int32_t local, int64_t scratch_limit, gsa_align_db_result* out,
                     char* cigar, int64_t cigar_cap, int64_t* cigar_need, gsa_align_db_info* info, float* kernel_ms,
                     void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return align_db_impl(ctx, query, adjq, db, db_off, nsubj, hits, nhits, subst, substsz, gapo, gape, local,
                         scratch_limit, out, cigar, cigar_cap, cigar_need, info, kernel_ms, pick_stream(ctx, stream));
}

int gsa_score_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst, int32_t substsz,
                        int32_t gapo, int32_t gape, int32_t local, gsa_score_result* out, float* batch_kernel_ms,
                        void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return score_batch_impl(ctx, npairs, pairs, subst, substsz, gapo, gape, local, out, batch_kernel_ms,
                            pick_stream(ctx, stream));
}

int gsa_score_db_dev(gsa_ctx* ctx, const int32_t* query, int32_t adjq, const int32_t* db, const int64_t* db_off,
                     int32_t nsubj, const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int32_t local,
                     gsa_score_result* out, float* kernel_ms, void* stream)
{
    if (!ctx) return GSA_ERROR_INVALID_VALUE;
    return score_db_impl(ctx, query, adjq, db, db_off, nsubj, subst, substsz, gapo, gape, local, out, kernel_ms,
                         pick_stream(ctx, stream));
}

int gsa_score_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                  const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int32_t local,
                  gsa_score_result* out, void* stream)
{
    return score_dev_impl(ctx, seqY, adjrows, seqX, adjcols, subst, substsz, gapo, gape, local, out,
                          pick_stream(ctx, stream), -1);
}

int gsa_score(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
              const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int32_t local,
              gsa_score_result* out, gsa_laps* laps)
{
    if (!ctx || !seqY || !seqX || !subst || !out) return GSA_ERROR_INVALID_VALUE;
    int s = check_inputs(adjrows, adjcols, substsz);
    if (s != GSA_SUCCESS) return s;
    gsa_laps L {};
    auto t = Clock::now();
    if ((s = ensure_dev(ctx, 0, (size_t)adjrows * 4)) || (s = ensure_dev(ctx, 1, (size_t)adjcols * 4)) ||
        (s = ensure_dev(ctx, 2, (size_t)substsz * substsz * 4)))
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
    s = score_dev_impl(ctx, ctx->buf[kBufIo0].as<const int32_t>(), adjrows, ctx->buf[kBufIo1].as<const int32_t>(), adjcols,
                       ctx->buf[kBufIo2].as<const int32_t>(), substsz, gapo, gape, local, out, ctx->stream,
                       subst_absmax(subst, substsz));
    if (s != GSA_SUCCESS) return s;
    L.calc = ms_since(t);
    lap(ctx, "align.calc");
    L.calc_kernel_ms = out->calc_kernel_ms;
    if (laps) *laps = L;
    return GSA_SUCCESS;
}

}  // extern "C"
