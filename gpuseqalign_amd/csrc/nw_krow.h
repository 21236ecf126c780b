// nw_krow.h -- launch interface of the K-rows-per-lane sparse (mlsp) fill (nw_krow.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "nw_strip.h"

namespace gsa {

constexpr int kKrowKDefault = 4;        // rows per lane
constexpr int kKrowNSDefault = 4;       // strip waves per workgroup, single pairs
constexpr int kKrowNSBatchDefault = 8;  // strip waves per workgroup, batches of pairs

// (ns, k) pairs the library instantiates: a ticket = ns * 64 * k rows, which divides the sparse
// tile height kSparseTileBy (1024) or, for (8, 4), spans two tile rows (the drain wave then also
// writes the header row between strips 3 and 4).
__host__ __device__ constexpr bool krow_ok(int ns, int k)
{
    return ((k == 2 || k == 4) && (ns == 2 || ns == 4)) || (k == 4 && ns == 8);
}
__host__ __device__ constexpr int krow_ticket_rows(int ns, int k) { return ns * 64 * k; }
// tickets of a pair with trows tile rows (the last ticket of a two-row geometry may cover one)
__host__ __device__ constexpr int krow_tickets(int trows, int ns, int k)
{
    return (trows * kSparseTileBy + krow_ticket_rows(ns, k) - 1) / krow_ticket_rows(ns, k);
}
// q8: the int8-profile instance's layout (nw_krow.hip)
size_t krow_lds_bytes(int ns, int lw, int substsz, bool q8 = false);
// StripArgs / PairDesc / granule contract as launch_strip_fill (sparse mode, a.tBx, a.tBy,
// per-pair hrow/hcol/trows/tcols/Cp); tickets of a pair = krow_tickets(trows, ns, k).
// Every s - 2g must lie in [-32768, 32767] and be at most a.qcap (the kernel sets error bit 2 otherwise).
// grid <= 0: every resident slot.
// The profile ring holds 512 columns for ns = 2, 1024 otherwise (lw is reserved).
hipError_t launch_krow_fill(const StripArgs& a, int ns, int k, int lw, int grid, hipStream_t stream);
// Pass 1 of the two-pass full fill (nw_expand.h): the sparse fill (K = 4, ns = 4 or 8, a.tBx =
// kExpHB) that also stores rows 64m into each pair's rows64 / rpitch (PairDesc).
hipError_t launch_krow_fill_xr(const StripArgs& a, int ns, int grid, hipStream_t stream);
// Both passes of the two-pass full fill in one launch: the first a.xP workgroups take pass-1
// tickets (the XR fill on (ns, 4) tickets) until none is left, then, like the rest, expansion
// tasks of `waves` x 64 rows (a.xpair, a.xsched, a.xTasks), each task waiting for the progress
// words a.xdone of the strips whose rows and header column it reads.  (ns, waves): (4, 8) or
// (8, 12).  grid <= 0: every resident slot.
// staged: the strips hand row 64m to a storer wave (large pairs); else they store it themselves
// full_fused_lds_bytes: the workgroup's dynamic LDS (pass 1's K-rows layout plus the staging, or the
// expansion's if larger); the caller picks q8 and staged so that it fits the device
size_t full_fused_lds_bytes(int ns, int substsz, bool q8, bool staged);
hipError_t launch_full_fused(const StripArgs& a, int ns, int waves, bool staged, int grid, hipStream_t stream);

// Score-only NW / SW (modes kModeScoreAG/AGL/SW/SWL of nw_strip.h, same StripArgs contract as
// launch_strip_fill for one pair: go, ge, gran + gran2, agResult, swBest, idxBits) on the K-rows
// layout (nw_kscore.hip): 1024-row tickets, grid > 0 workgroups.  Every s - go - ge must lie in
// (-32768, 32767] (error bit 2 otherwise); SW needs go < 0 and ge <= 0.  a.q8 as launch_kr: the
// int8-profile instance (values in [-127, 127]) with the int16 one behind it.
// A batch of independent pairs (a.sched set, or a.nPairs > 1 without a.bidiTop; the BATCH instances):
// tickets 64 k 4 rows per pair in one ticket space (PairDesc::ticketBase / nTickets / granOff; a.sched:
// {pair, ticket} per global ticket, ticket j of a pair behind its ticket j-1), a.swBest the base of
// two result words per pair (nw_strip.h), zeroed by the caller; agResult and idxBits unused; no taps,
// no bidi fields; grid <= 0: every resident slot.  launch_score_finalize (nw_bidi.h) decodes the words.
size_t krow_score_lds_bytes(int substsz, bool q8 = false);
hipError_t launch_krow_score(const StripArgs& a, int mode, int k, int grid, hipStream_t stream);
// (the affine modes' instances, in nw_kscore_ag.hip; called by launch_krow_score)
hipError_t launch_krow_score_affine(const StripArgs& a, int mode, int k, int grid, hipStream_t stream);
// Semi-global score of one pair (modes kModeScoreSG / SGL, nw_kscore_semi.hip): launch_krow_score's
// contract for one pair in a global mode (no taps, no batch, no bidi fields, grid > 0), except that no
// result cell is written: the strip that holds row R stores that row's shifted Hgo' at
// a.rowR[kTapPad + column], a buffer of kTapPad + a.Cp + 80 ints.  launch_semi_rowmax, enqueued
// behind it, unshifts the row and writes the maximum over the columns 0 .. C (column 0 analytic:
// go + (R - 1) ge) to *score and the smallest column that attains it to *jend.
hipError_t launch_krow_score_semi(const StripArgs& a, int mode, int k, int grid, hipStream_t stream);
hipError_t launch_semi_rowmax(const int* rowR, int R, int C, int go, int ge, int* score, int* jend, hipStream_t stream);
// Overlap (dovetail) score of one pair (modes kModeScoreOV / OVL, nw_kscore_overlap.hip):
// launch_krow_score_semi's contract with a free column 0 as well (H(i, 0) = 0), and besides row R at
// a.rowR every strip of every ticket stores column C of its rows, shifted as row R is, at a.tapH[row]:
// a buffer of 1 + nTickets x (256 k) ints (a.tapRow stays 0: no tap is taken).  launch_overlap_max,
// enqueued behind it, unshifts both, adds H(R, 0) = H(0, C) = 0 and writes to res[0 .. 2] the largest
// value and its cell (i_end, j_end): the smallest j of row R that attains it, or else the smallest i of
// column C.
hipError_t launch_krow_score_overlap(const StripArgs& a, int mode, int k, int grid, hipStream_t stream);
hipError_t launch_overlap_max(const int* rowR, const int* colC, int R, int C, int go, int ge, int* res, hipStream_t stream);
// Semi-global scores of a batch of independent pairs (nw_kscore_semi_batch.hip): launch_krow_score's
// contract for a batch (ticketBase / nTickets / granOff, a.sched, a.swBest two zeroed words per pair,
// grid <= 0: every resident slot) in the modes kModeScoreSG / SGL; pair p's row R goes to its own buffer
// PairDesc::score of kTapPad + Cp + 80 ints, at a multiple of 16 ints.  launch_semi_rowmax_batch,
// enqueued behind it, takes every pair's maximum as launch_semi_rowmax does, one workgroup per pair:
// out[p] = {score, R, j_end, 0}, out[nPairs].score the error word *err (launch_score_finalize's layout).
hipError_t launch_krow_score_semi_batch(const StripArgs& a, int mode, int k, int grid, hipStream_t stream);
hipError_t launch_semi_rowmax_batch(const PairDesc* pairs, int nPairs, int go, int ge, const unsigned* err, ScoreOut* out,
                                    hipStream_t stream);
// Overlap scores of a batch of independent pairs (nw_kscore_overlap_batch.hip): launch_krow_score_semi_batch's
// contract in the modes kModeScoreOV / OVL; pair p's row R goes to PairDesc::score as there, and column C
// of every row of every one of its tickets to PairDesc::hcol[row], its own buffer of 1 + nTickets x
// (256 k) ints at a multiple of 16 ints (rows past R are stored too, so a buffer sized by R alone would
// be overwritten by its neighbour's last ticket).  launch_overlap_max_batch, enqueued behind it, takes
// every pair's maximum as launch_overlap_max does, one workgroup per pair: out[p] = {score, i_end,
// j_end, 0}, out[nPairs].score the error word *err (launch_score_finalize's layout).
hipError_t launch_krow_score_overlap_batch(const StripArgs& a, int mode, int k, int grid, hipStream_t stream);
hipError_t launch_overlap_max_batch(const PairDesc* pairs, int nPairs, int go, int ge, const unsigned* err, ScoreOut* out,
                                    hipStream_t stream);

}  // namespace gsa
