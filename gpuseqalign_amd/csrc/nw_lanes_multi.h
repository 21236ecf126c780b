// nw_lanes_multi.h -- database search, score-only: many queries against one database in one persistent
// launch of the lane kernel, the best subjects of every query ranked on the device
// (nw_lanes_multi.hip); used by gsa_score.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_lanes.h"

namespace gsa {

// Wave tasks of one query a workgroup claims at once (a unit); -DGSA_DBM_UNIT=n builds another size
// for tools/score_db_multi_bench.py (DESIGN.md 2.2f "Measured").
#ifndef GSA_DBM_UNIT
#define GSA_DBM_UNIT 8
#endif
constexpr int kDbMultiUnit = GSA_DBM_UNIT;

struct DbMultiQuery
{
    long long off;  // of the query's header element in `queries`
    int R;          // letters (>= 1)
    int row;        // the query's row of the chunk's result matrix
};

struct DbMultiArgs
{
    const int* queries;         // the queries back to back, each with its header
    const DbMultiQuery* q;      // the launch's queries, longest first: all of `passes` sweeps
    int nq;
    const int* db;              // the subjects back to back, each with its header
    const int* subst;
    int substsz;
    int go, ge;
    int passes;                 // sweeps of every query of this launch: ceil(R / kDbLanesPassRows)
    int nsubj;                  // lane subjects, longest first (all with 1 <= C <= kDbLanesMaxC)
    int ntasks;                 // ceil(nsubj / kDbLanesSubj), per query
    int unitsPerQuery;          // ceil(ntasks / kDbMultiUnit)
    int nunits;                 // nq * unitsPerQuery
    const long long* off;       // nsubj offsets into db (of the header element)
    const int* len;             // nsubj letter counts C
    const int* sidx;            // nsubj subject indices: the column of the result matrix
    DbLanesOut* out;            // result matrix, out[row * ld + subject]
    long long ld;               // subjects of the database (a row of the matrix)
    unsigned* counter;          // unit counter, zero at launch
    unsigned* builds;           // profile builds, one per workgroup and query it switched to
    int2* bnd;                  // passes > 1: per wave slot and group, (H, F) of the sweep's last row by column
    int bndStride;              // entries per group: longest subject + 1
};

// dynamic LDS of a workgroup: the profile tab[d][i] of a query of `passes` sweeps, int32
size_t dbmulti_lds_bytes(int passes, int substsz);
// workgroups resident at once for this sweep class
hipError_t dbmulti_resident(int passes, int substsz, int local, bool affine, int* wgs);
hipError_t launch_dbmulti(const DbMultiArgs& a, int local, int grid, hipStream_t st);

// Results computed on other paths, written into the matrix before the ranking.
struct DbMultiPatch
{
    long long index;  // row * ld + subject
    DbLanesOut v;
};
hipError_t launch_dbmulti_scatter(const DbMultiPatch* list, long long n, DbLanesOut* out, hipStream_t st);
// scores[k] = out[k].score, k < n
hipError_t launch_dbmulti_scores(const DbLanesOut* out, long long n, int* scores, hipStream_t st);

struct DbMultiHit
{
    int subject, score, i_end, j_end;  // gsa_db_hit
};
// Bytes of ranking scratch for nq rows of nsubj results (keys, sorted keys, segment offsets, the
// sort's own storage); *tempBytes: the sort's share.
hipError_t dbmulti_select_bytes(int nq, int nsubj, size_t* bytes, size_t* tempBytes);
// The ntop best of every row by (score descending, subject ascending) into hits[nq][ntop].
hipError_t launch_dbmulti_select(const DbLanesOut* out, int nq, int nsubj, int ntop, void* scratch, size_t tempBytes,
                                 DbMultiHit* hits, hipStream_t st);

}  // namespace gsa
