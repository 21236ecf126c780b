// Stand-alone driver over gpuseqalign_amd/csrc/nw_pair_overlap_trace_batch_plan.h (no HIP, no GPU): reads
// cases "TR limit seed npairs" followed by npairs lines "iEnd jEnd iStart jStart" (the end cell, and the
// start cell on row 0 or on column 0: iStart = 0 or jStart = 0, iStart < iEnd, jStart < jEnd) from standard
// input, runs the rounds gsa_align_batch_overlap_dev would run with a seeded stand-in for the walks -- a
// monotone path from the end cell to the start cell: at a chunk's upper boundary row b > iStart the walk
// stands on a column between jStart + 1 (jStart when iStart = 0) and the column it came from; once the
// boundary is at or above iStart with jStart = 0 the walk has reached column 0 and is done -- checks the
// plan's properties itself (a violation is reported on standard error and ends the program with status
// 1) and prints every round for tests/test_align_batch_overlap_plan.py, which checks them again on the
// output.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "nw_pair_overlap_trace_batch_plan.h"

namespace {

[[noreturn]] void bad(long long kase, const char* what)
{
    std::fprintf(stderr, "case %lld: %s\n", kase, what);
    std::exit(1);
}

unsigned long long next(unsigned long long& seed)
{
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    return seed >> 33;
}

struct In
{
    long long iEnd, jEnd, iStart, jStart;
};

}  // namespace

int main()
{
    long long TR, limit, kase = 0;
    unsigned long long seed;
    int npairs;
    while (std::scanf("%lld %lld %llu %d", &TR, &limit, &seed, &npairs) == 4)
    {
        std::vector<In> in((size_t)npairs);
        std::vector<gsa::BatchPairState> st((size_t)npairs);
        std::vector<long long> next_strip((size_t)npairs);
        for (int p = 0; p < npairs; ++p)
        {
            In& q = in[(size_t)p];
            if (std::scanf("%lld %lld %lld %lld", &q.iEnd, &q.jEnd, &q.iStart, &q.jStart) != 4) bad(kase, "short input");
            if (q.iEnd < 1 || q.jEnd < 1 || q.iStart < 0 || q.jStart < 0 || q.iStart >= q.iEnd || q.jStart >= q.jEnd ||
                (q.iStart != 0 && q.jStart != 0))
                bad(kase, "a pair of the input has no path");
            st[(size_t)p].tHi = gsa::overlap_end_strip(TR, q.iEnd);
            st[(size_t)p].J = q.jEnd;
            if (st[(size_t)p].tHi != (q.iEnd - 1) / TR) bad(kase, "the end strip is not i_end's");
            next_strip[(size_t)p] = st[(size_t)p].tHi;  // bottom-up: the strip a pair's next chunk must end on
            if (gsa::pair_strip_bytes(TR, q.jEnd) > limit) bad(kase, "a strip of the input exceeds the limit");
        }
        std::printf("case %d\n", npairs);
        std::vector<gsa::BatchChunk> chunks;
        long long rounds = 0;
        for (;;)
        {
            const long long used = gsa::batch_plan_round(TR, limit, st, &chunks);
            bool active = false;
            for (const gsa::BatchPairState& s : st) active = active || s.tHi >= 0;
            if (chunks.empty())
            {
                if (active) bad(kase, "a round with active pairs fills no strip");
                break;
            }
            ++rounds;
            if (used > limit) bad(kase, "a round's bytes exceed the limit");
            std::printf("round %lld\n", used);
            // the fixed order: remaining bytes descending, ties by index (over the pairs that got a chunk)
            for (size_t c = 1; c < chunks.size(); ++c)
            {
                const long long a = gsa::batch_pair_remaining(TR, st[(size_t)chunks[c - 1].pair]);
                const long long b = gsa::batch_pair_remaining(TR, st[(size_t)chunks[c].pair]);
                if (a < b || (a == b && chunks[c - 1].pair > chunks[c].pair)) bad(kase, "pairs out of order");
            }
            std::vector<std::pair<long long, long long>> spans;
            long long sum = 0;
            std::vector<char> seen((size_t)npairs, 0);
            for (const gsa::BatchChunk& b : chunks)
            {
                const gsa::BatchPairState& s = st[(size_t)b.pair];
                if (seen[(size_t)b.pair]) bad(kase, "a pair twice in a round");
                seen[(size_t)b.pair] = 1;
                if (b.c.tHi != next_strip[(size_t)b.pair] || b.c.tHi != s.tHi || b.c.tLo < 0 || b.c.tLo > b.c.tHi)
                    bad(kase, "a chunk is not the pair's next strips, bottom-up");
                if (b.c.tHi > (in[(size_t)b.pair].iEnd - 1) / TR) bad(kase, "a strip below i_end's is planned");
                if (b.c.J != s.J || b.c.stripBytes != gsa::pair_strip_bytes(TR, s.J) ||
                    b.c.codeBytes != (b.c.tHi - b.c.tLo + 1) * b.c.stripBytes)
                    bad(kase, "a chunk's columns or bytes");
                if (b.codeOff < 0 || b.codeOff + b.c.codeBytes > limit) bad(kase, "a chunk outside the round's bytes");
                for (long long t = b.c.tLo; t <= b.c.tHi; ++t)
                {
                    const long long o = b.codeOff + gsa::pair_code_off(b.c, t);
                    spans.push_back(std::make_pair(o, o + b.c.stripBytes));
                }
                sum += b.c.codeBytes;
                std::printf("chunk %d %lld %lld %lld %lld %lld %lld\n", b.pair, b.c.tLo, b.c.tHi, b.c.J, b.c.stripBytes,
                            b.c.codeBytes, b.codeOff);
            }
            if (sum != used) bad(kase, "the round's bytes are not the chunks' sum");
            std::sort(spans.begin(), spans.end());
            for (size_t a = 1; a < spans.size(); ++a)
                if (spans[a].first < spans[a - 1].second) bad(kase, "code ranges overlap");
            // one pair: overlap_plan_chunk's chunk exactly
            if (npairs == 1)
            {
                gsa::PairChunk c;
                const gsa::PairChunk& g = chunks[0].c;
                if (!gsa::overlap_plan_chunk(TR, st[0].tHi, st[0].J, limit, &c) || c.tLo != g.tLo || c.tHi != g.tHi ||
                    c.J != g.J || c.stripBytes != g.stripBytes || c.codeBytes != g.codeBytes || chunks[0].codeOff != 0)
                    bad(kase, "one pair: not overlap_plan_chunk's chunk");
            }
            // the walks
            for (const gsa::BatchChunk& b : chunks)
            {
                const In& q = in[(size_t)b.pair];
                gsa::BatchPairState& s = st[(size_t)b.pair];
                const long long stop = gsa::pair_chunk_stop_row(TR, b.c);
                long long i, j;
                bool done;
                if (stop <= q.iStart)
                {
                    // the start cell lies inside the chunk (or on its boundary): the walk ends there
                    i = q.iStart;
                    j = q.jStart;
                    done = true;
                }
                else
                {
                    // on the boundary, right of the start column, never right of where it came from
                    const long long lo = q.jStart + (q.iStart == 0 ? 0 : 1);
                    i = stop;
                    j = lo + (long long)(next(seed) % (unsigned long long)(s.J - lo + 1));
                    done = j == 0;  // (a start on row 0 at column 0 reached early)
                    if (done && q.iStart != 0) bad(kase, "the stand-in left its path");
                }
                if (!gsa::overlap_batch_advance(TR, b.c, i, j, done, &s)) bad(kase, "a walk neither done nor on its boundary");
                if (done)
                {
                    if (s.tHi != -1) bad(kase, "a finished pair is still active");
                    next_strip[(size_t)b.pair] = -1;
                    std::printf("done %d %lld %lld\n", b.pair, i, j);
                }
                else
                {
                    if (s.tHi != b.c.tLo - 1 || s.J != j || s.J < 1) bad(kase, "the next state is not (tLo - 1, j)");
                    next_strip[(size_t)b.pair] = s.tHi;
                }
            }
        }
        for (const gsa::BatchPairState& s : st)
            if (s.tHi >= 0) bad(kase, "a pair's walk did not end");
        std::printf("end %lld\n", rounds);
        ++kase;
    }
    std::printf("ok %lld\n", kase);
    return 0;
}
