// nw_lanes.h -- database search, score-only: one query against many short subjects, every subject on
// a group of lanes of one wave (nw_lanes.hip); used by gsa_score.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsa {

constexpr int kDbLanesG = 16;   // lanes per subject: one DPP row, the hand-off is row_shr:1
constexpr int kDbLanesKQ = 24;  // query rows a lane holds in registers
constexpr int kDbLanesWaves = 4;                            // waves per workgroup
constexpr int kDbLanesSubj = 64 / kDbLanesG;                // subjects per wave task
constexpr int kDbLanesPassRows = kDbLanesG * kDbLanesKQ;    // query rows one sweep of a task covers
constexpr int kDbLanesJBits = 13;                           // local: column bits of a row's best key
constexpr int kDbLanesMaxC = (1 << kDbLanesJBits) - 1;      // longest subject the kernel takes
constexpr long long kDbLanesMaxScore = 1ll << (31 - kDbLanesJBits);  // local: scores stay below this

struct DbLanesOut
{
    int score, i_end, j_end, pad;
};

struct DbLanesArgs
{
    const int* query;       // adjq ints, header in front
    const int* db;          // the subjects back to back, each with its header
    const int* subst;
    int substsz;
    int go, ge;
    int R;                  // query letters (>= 1)
    int passes;             // ceil(R / kDbLanesPassRows)
    int nsubj;              // subjects of this launch, longest first (all with 1 <= C <= kDbLanesMaxC)
    int ntasks;             // ceil(nsubj / kDbLanesSubj)
    const long long* off;   // nsubj offsets into db (of the header element)
    const int* len;         // nsubj letter counts C
    DbLanesOut* out;        // nsubj results, in the launch's order
    unsigned* counter;      // task counter, zero at launch
    int2* bnd;              // passes > 1: per wave slot and group, (H, F) of the sweep's last row by column
    int bndStride;          // entries per group: longest subject + 1
};

// dynamic LDS of a workgroup: the query profile tab[d][i], int32
size_t dblanes_lds_bytes(int R, int substsz);
// `grid` workgroups (0: as many as are resident, at most one per kDbLanesWaves tasks); *gridOut = the grid
hipError_t launch_dblanes(const DbLanesArgs& a, int local, int grid, int* gridOut, hipStream_t st);
// workgroups resident at once for this query (the size of the boundary scratch)
hipError_t dblanes_resident(int R, int substsz, int local, bool affine, int* wgs);

}  // namespace gsa
