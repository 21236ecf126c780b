// nw_pair_semi_plan.h -- the semi-global alignment of one long pair (gsa_align_pair_semi_dev; DESIGN.md
// 2.2k): the column window the move codes are kept for, and the chunks of strips over it.  No HIP
// here: tests/align_pair_semi_plan_driver.cpp checks it on the CPU.
//
// The window.  The end cell (R, j_end) may lie anywhere along a long subject, but the path spans about
// R columns.  With pmax = max(0, largest table value), m <= R diagonal moves and d letters of 'D' on a
// path of score S:  S <= pmax m + d gape <= pmax R + d gape, because the 'D' gaps cost at most d gape
// in all (gapo <= gape) and the 'I' gaps at most 0.  For gape < 0 this bounds d by
//   dmax = floor((pmax R - S) / |gape|),
// and the columns the path spans by j_end - j_start = m + d <= R + dmax.  So with
//   jW = max(0, j_end - R - dmax - 1)          (gape = 0: jW = 0)
// no optimal path to the end cell touches column jW below row 0 when jW > 0, and the fill may treat
// that column as minus infinity for the rows >= 1 and keep codes for the columns jW + 1 ... J only:
// lowering cells only lowers values; every optimal path to a cell and state on an optimal whole path,
// joined with the rest of it, is an optimal whole path and so stays right of jW; hence every cell and
// state the walk visits keeps its true value, every predecessor that attains the maximum there keeps
// its own, and every loser stays a loser -- tags and extend bits along the walk are unchanged, ties
// included.  A strip's codes then take (J - jW) TR / 2 bytes.
//
// The chunks are nw_pair_trace_plan.h's, bottom-up, with the width J - jW in place of J.
#pragma once
#include <stdint.h>

#include "nw_pair_trace_plan.h"

namespace gsa {

// jW of a pair whose query has R letters, for the end column jEnd and the score S; pmax = max(0,
// largest table value), gape <= 0
inline long long semi_window(long long R, long long jEnd, long long S, long long pmax, long long gape)
{
    if (gape >= 0) return 0;
    const long long room = pmax * R - S;  // >= 0 for every score an alignment attains
    const long long dmax = room > 0 ? room / -gape : 0;
    const long long jW = jEnd - R - dmax - 1;
    return jW > 0 ? jW : 0;
}

// The chunk whose lowest strip is tHi, for the columns jW + 1 ... J (J > jW): PairChunk::J is the
// width J - jW, stripBytes and codeBytes those of the window.  False when one strip does not fit.
inline bool semi_plan_chunk(long long TR, long long tHi, long long J, long long jW, long long limit, PairChunk* c)
{
    return J > jW && pair_plan_chunk(TR, tHi, J - jW, limit, c);
}

}  // namespace gsa
