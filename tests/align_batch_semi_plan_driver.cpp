// Stand-alone driver over gpuseqalign_amd/csrc/nw_pair_semi_trace_batch_plan.h (no HIP, no GPU): reads
// cases "TR limit seed npairs" followed by npairs lines "R jEnd jW" (0 <= jW < jEnd) from standard input,
// runs the rounds gsa_align_batch_semi_dev would run with a seeded stand-in for the walks -- a pair
// leaves its chunk at some column jW + 1 ... J of it; it is done once its chunk holds strip 0 -- checks
// the plan's properties itself (a violation is reported on standard error and ends the program with
// status 1) and prints every round for tests/test_align_batch_semi_plan.py, which checks them again on
// the output.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "nw_pair_semi_trace_batch_plan.h"

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

}  // namespace

int main()
{
    long long TR, limit, kase = 0;
    unsigned long long seed;
    int npairs;
    while (std::scanf("%lld %lld %llu %d", &TR, &limit, &seed, &npairs) == 4)
    {
        std::vector<gsa::BatchPairState> st((size_t)npairs);
        std::vector<long long> next_strip((size_t)npairs);
        for (int p = 0; p < npairs; ++p)
        {
            long long R, jEnd, jW;
            if (std::scanf("%lld %lld %lld", &R, &jEnd, &jW) != 3) bad(kase, "short input");
            if (R < 1 || jW < 0 || jEnd <= jW) bad(kase, "a pair of the input has no window");
            st[(size_t)p].tHi = gsa::pair_strips(TR, R) - 1;
            st[(size_t)p].J = jEnd;
            st[(size_t)p].jW = jW;
            next_strip[(size_t)p] = st[(size_t)p].tHi;  // bottom-up: the strip a pair's next chunk must end on
            if (gsa::pair_strip_bytes(TR, jEnd - jW) > limit) bad(kase, "a strip of the input exceeds the limit");
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
                if (b.c.J != s.J - s.jW || b.c.stripBytes != gsa::pair_strip_bytes(TR, s.J - s.jW) ||
                    b.c.codeBytes != (b.c.tHi - b.c.tLo + 1) * b.c.stripBytes)
                    bad(kase, "a chunk's window or bytes");
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
            // one pair: semi_plan_chunk's chunk exactly
            if (npairs == 1)
            {
                gsa::PairChunk c;
                const gsa::PairChunk& g = chunks[0].c;
                if (!gsa::semi_plan_chunk(TR, st[0].tHi, st[0].J, st[0].jW, limit, &c) || c.tLo != g.tLo || c.tHi != g.tHi ||
                    c.J != g.J || c.stripBytes != g.stripBytes || c.codeBytes != g.codeBytes || chunks[0].codeOff != 0)
                    bad(kase, "one pair: not semi_plan_chunk's chunk");
            }
            // the walks: a semi-global path always reaches row 0, so a pair is done only once its chunk
            // holds strip 0; else it stands on the chunk's upper boundary at a column of its window
            for (const gsa::BatchChunk& b : chunks)
            {
                gsa::BatchPairState& s = st[(size_t)b.pair];
                if (b.c.tLo == 0)
                {
                    s.tHi = -1;
                    next_strip[(size_t)b.pair] = -1;
                    std::printf("done %d\n", b.pair);
                    continue;
                }
                s.tHi = b.c.tLo - 1;
                s.J = s.jW + 1 + (long long)(next(seed) % (unsigned long long)b.c.J);  // the path never moves right
                next_strip[(size_t)b.pair] = s.tHi;
            }
        }
        for (const gsa::BatchPairState& s : st)
            if (s.tHi >= 0) bad(kase, "a pair was not filled up to strip 0");
        std::printf("end %lld\n", rounds);
        ++kase;
    }
    std::printf("ok %lld\n", kase);
    return 0;
}
