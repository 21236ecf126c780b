// nw_lanes_trace_multi_plan.h -- database search, the alignments of many queries' hits in one call
// (gsa_align_db_multi_dev): the host's plan of chunks, launches, units and tasks.
// Plain C++ with no HIP in it, so that the plan is checked on a CPU (tests/test_align_db_multi_plan.py);
// used by gsa_score.hip, and its records are what nw_lanes_trace_multi.hip reads on the device.
//
// The hits the trace kernels take are ordered by query length (longest first, so the sweep classes are
// runs of the order), then query index, then subject length (longest first), then position in the
// caller's list.  That order is cut greedily into chunks whose move codes fit the limit.  In a chunk
// the hits of one query are cut into tasks of up to four (one wave: a hit per DPP row), the tasks of
// one query into units of up to `unit` consecutive tasks, and the units of one sweep class are one
// launch.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace gsa {

constexpr int kDbaPassRows = 384;  // query rows of one sweep (kDbLanesPassRows)
constexpr int kDbaTaskHits = 4;    // hits of a wave task (kDbLanesSubj)
constexpr int kDbaColBytes = 192;  // move codes of one column of one sweep (kDbTraceColBytes)

inline int dba_passes(long long R) { return (int)((R + kDbaPassRows - 1) / kDbaPassRows); }
// bytes of move codes of one hit: dbtrace_code_bytes
inline long long dba_code_bytes(long long R, long long C) { return (long long)dba_passes(R) * (C + 1) * kDbaColBytes; }

struct DbaQuery  // a query with hits in the chunk
{
    long long off;  // of the query's header element in `queries`
    int R;          // letters (>= 1)
    int index;      // the caller's query index
};

struct DbaTask  // hits [first, first + n) of the chunk, all of one query, 1 <= n <= kDbaTaskHits
{
    int first, n;
};

struct DbaUnit  // tasks [firstTask, firstTask + ntasks) of the chunk, all of chunk query `query`
{
    int query, firstTask, ntasks, pad;
};

struct DbaHit
{
    int hit;      // position in the caller's list
    int query;    // index into the chunk's queries
    int R, C;
    long long qOff, dbOff;      // of the header elements, into `queries` and `db`
    long long codeOff, codeLen; // bytes, into the chunk's codes
    long long moveOff, moveLen; // bytes, into the chunk's moves: R + C
};

struct DbaLaunch  // one sweep class of a chunk
{
    int passes;
    int firstUnit, nunits;
    int firstQuery, nqueries;
    int firstTask, ntasks;
};

struct DbaChunk
{
    std::vector<DbaHit> hits;
    std::vector<DbaQuery> queries;
    std::vector<DbaTask> tasks;
    std::vector<DbaUnit> units;
    std::vector<DbaLaunch> launches;
    long long codeBytes = 0, moveBytes = 0;
    int cmax = 0;  // the longest subject of the chunk
};

// hit_query / hit_subject: nhits indices into the offset tables; lane[h] != 0: hit h takes the trace
// kernels (both sides have letters and its codes alone fit `limit`); unit >= 1.
inline std::vector<DbaChunk> dba_plan(int nhits, const int32_t* hit_query, const int32_t* hit_subject, const int64_t* q_off,
                                      const int64_t* db_off, const unsigned char* lane, long long limit, int unit)
{
    auto rows_of = [&](int h) { return (long long)(q_off[hit_query[h] + 1] - q_off[hit_query[h]] - 1); };
    auto cols_of = [&](int h) { return (long long)(db_off[hit_subject[h] + 1] - db_off[hit_subject[h]] - 1); };
    std::vector<int> order;
    for (int h = 0; h < nhits; ++h)
        if (lane[h]) order.push_back(h);
    std::sort(order.begin(), order.end(), [&](int x, int y) {
        if (rows_of(x) != rows_of(y)) return rows_of(x) > rows_of(y);
        if (hit_query[x] != hit_query[y]) return hit_query[x] < hit_query[y];
        if (cols_of(x) != cols_of(y)) return cols_of(x) > cols_of(y);
        return x < y;
    });
    std::vector<DbaChunk> chunks;
    for (size_t b = 0; b < order.size();)
    {
        DbaChunk ch;
        size_t k = b;
        while (k < order.size())
        {
            const int h = order[k];
            const long long R = rows_of(h), C = cols_of(h), cb = dba_code_bytes(R, C);
            if (ch.codeBytes + cb > limit) break;
            if (ch.queries.empty() || ch.queries.back().index != hit_query[h])
                ch.queries.push_back(DbaQuery {(long long)q_off[hit_query[h]], (int)R, (int)hit_query[h]});
            ch.hits.push_back(DbaHit {h, (int)ch.queries.size() - 1, (int)R, (int)C, (long long)q_off[hit_query[h]],
                                      (long long)db_off[hit_subject[h]], ch.codeBytes, cb, ch.moveBytes, R + C});
            ch.codeBytes += cb;
            ch.moveBytes += R + C;
            ch.cmax = std::max(ch.cmax, (int)C);
            ++k;
        }
        if (k == b) break;  // a hit that fits no chunk: the caller's flags are wrong; plan nothing more
        // tasks and units per query, launches per sweep class
        for (size_t i = 0; i < ch.hits.size();)
        {
            size_t j = i;
            while (j < ch.hits.size() && ch.hits[j].query == ch.hits[i].query) ++j;
            const int q = ch.hits[i].query, passes = dba_passes(ch.hits[i].R);
            if (ch.launches.empty() || ch.launches.back().passes != passes)
                ch.launches.push_back(DbaLaunch {passes, (int)ch.units.size(), 0, q, 0, (int)ch.tasks.size(), 0});
            DbaLaunch& L = ch.launches.back();
            const int t0 = (int)ch.tasks.size();
            for (size_t f = i; f < j; f += kDbaTaskHits)
                ch.tasks.push_back(DbaTask {(int)f, (int)std::min<size_t>(kDbaTaskHits, j - f)});
            const int t1 = (int)ch.tasks.size();
            for (int t = t0; t < t1; t += unit) ch.units.push_back(DbaUnit {q, t, std::min(unit, t1 - t), 0});
            L.nunits = (int)ch.units.size() - L.firstUnit;
            L.nqueries = q + 1 - L.firstQuery;
            L.ntasks = t1 - L.firstTask;
            i = j;
        }
        chunks.push_back(std::move(ch));
        b = k;
    }
    return chunks;
}

}  // namespace gsa
