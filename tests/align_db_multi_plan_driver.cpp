// Stand-alone driver of gpuseqalign_amd/csrc/nw_lanes_trace_multi_plan.h for
// tests/test_align_db_multi_plan.py: reads cases from standard input, prints every plan as text.
//   case:  nq nsubj nhits unit limit
//          nq query lengths, nsubj subject lengths
//          nhits lines: query subject lane
// Output per case: "plan <chunks>", then per chunk "chunk codeBytes moveBytes cmax" and its records,
// one per line, tagged H (hit), Q (query), T (task), U (unit), L (launch); "end" closes a case.
#include <cstdio>
#include <vector>

#include "nw_lanes_trace_multi_plan.h"

int main()
{
    int nq, nsubj, nhits, unit;
    long long limit;
    while (std::scanf("%d %d %d %d %lld", &nq, &nsubj, &nhits, &unit, &limit) == 5)
    {
        std::vector<int64_t> qoff((size_t)nq + 1, 0), off((size_t)nsubj + 1, 0);
        for (int q = 0; q < nq; ++q)
        {
            long long len;
            if (std::scanf("%lld", &len) != 1) return 2;
            qoff[(size_t)q + 1] = qoff[(size_t)q] + len + 1;
        }
        for (int s = 0; s < nsubj; ++s)
        {
            long long len;
            if (std::scanf("%lld", &len) != 1) return 2;
            off[(size_t)s + 1] = off[(size_t)s] + len + 1;
        }
        std::vector<int32_t> hq((size_t)nhits), hs((size_t)nhits);
        std::vector<unsigned char> lane((size_t)nhits);
        for (int h = 0; h < nhits; ++h)
        {
            int q, s, l;
            if (std::scanf("%d %d %d", &q, &s, &l) != 3) return 2;
            hq[(size_t)h] = q;
            hs[(size_t)h] = s;
            lane[(size_t)h] = (unsigned char)l;
        }
        const std::vector<gsa::DbaChunk> plan =
            gsa::dba_plan(nhits, hq.data(), hs.data(), qoff.data(), off.data(), lane.data(), limit, unit);
        std::printf("plan %zu\n", plan.size());
        for (const gsa::DbaChunk& ch : plan)
        {
            std::printf("chunk %lld %lld %d\n", ch.codeBytes, ch.moveBytes, ch.cmax);
            for (const gsa::DbaHit& h : ch.hits)
                std::printf("H %d %d %d %d %lld %lld %lld %lld %lld %lld\n", h.hit, h.query, h.R, h.C, h.qOff, h.dbOff,
                            h.codeOff, h.codeLen, h.moveOff, h.moveLen);
            for (const gsa::DbaQuery& q : ch.queries) std::printf("Q %lld %d %d\n", q.off, q.R, q.index);
            for (const gsa::DbaTask& t : ch.tasks) std::printf("T %d %d\n", t.first, t.n);
            for (const gsa::DbaUnit& u : ch.units) std::printf("U %d %d %d\n", u.query, u.firstTask, u.ntasks);
            for (const gsa::DbaLaunch& l : ch.launches)
                std::printf("L %d %d %d %d %d %d %d\n", l.passes, l.firstUnit, l.nunits, l.firstQuery, l.nqueries,
                            l.firstTask, l.ntasks);
        }
        std::printf("end\n");
    }
    return 0;
}
