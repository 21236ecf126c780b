// nw_lanes_trace_multi.h -- database search, the alignments of many queries' hits in one call: the
// fill with move codes over a task space of (query, hits) units and the walk with a query per hit
// (nw_lanes_trace_multi.hip); used by gsa_score.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_lanes_trace.h"
#include "nw_lanes_trace_multi_plan.h"

namespace gsa {

// Wave tasks of one query a workgroup claims at once (a unit); -DGSA_DBA_UNIT=n builds another size
// for tools/align_db_multi_bench.py (DESIGN.md 2.2g "Measured").
#ifndef GSA_DBA_UNIT
#define GSA_DBA_UNIT 4
#endif
constexpr int kDbAlignMultiUnit = GSA_DBA_UNIT;

static_assert(kDbaPassRows == kDbLanesPassRows && kDbaTaskHits == kDbLanesSubj && kDbaColBytes == kDbTraceColBytes,
              "the plan's constants are the kernels'");

struct DbTraceMultiArgs
{
    const int* queries;        // the queries back to back, each with its header
    const int* db;             // the subjects back to back, each with its header
    const int* subst;
    int substsz;
    int go, ge;
    int passes;                // sweeps of every query of this launch
    const DbaQuery* q;         // the chunk's queries
    const DbaUnit* units;      // the launch's units
    int nunits;
    const DbaTask* tasks;      // the chunk's tasks
    const long long* off;      // per hit of the chunk: offset into db (of the header element)
    const int* len;            // per hit: letter count C of the subject (1 <= C <= kDbLanesMaxC)
    const long long* codeOff;  // per hit: byte offset into codes, passes x (C + 1) x 192 bytes each
    DbLanesOut* out;           // per hit: score and end cell
    unsigned char* codes;      // the chunk's move codes
    unsigned* counter;         // unit counter, zero at launch
    unsigned* builds;          // profile builds, one per workgroup and query it switched to
    int2* bnd;                 // passes > 1: per wave slot and group, (H, F) of the sweep's last row by column
    int bndStride;             // entries per group: the chunk's longest subject + 1
};

struct DbTraceMultiWalkArgs
{
    const int* queries;
    const int* db;
    int nhits;                  // hits of the chunk, of every sweep class
    int local;
    const long long* qoff;      // per hit: offset into queries (of the header element)
    const long long* off;
    const int* len;
    const DbLanesOut* out;
    const unsigned char* codes;
    const long long* codeOff;
    const long long* moveOff;   // per hit: byte offset into moves, R + C bytes each
    DbTraceOut* res;            // per hit
    unsigned char* moves;       // one byte per move ('=', 'X', 'I', 'D'), last move first
};

// workgroups of the fill resident at once for this sweep class
hipError_t dbtrace_multi_resident(int passes, int substsz, int local, bool affine, int* wgs);
hipError_t launch_dbtrace_multi_fill(const DbTraceMultiArgs& a, int local, int grid, hipStream_t st);
hipError_t launch_dbtrace_multi_walk(const DbTraceMultiWalkArgs& a, hipStream_t st);

}  // namespace gsa
