// Stand-alone driver over gpuseqalign_amd/csrc/nw_pair_trace_plan.h (no HIP, no GPU): reads cases
// "TR iEnd jEnd limit seed" from standard input and prints the chunks gsa_align_pair_dev would take,
// bottom-up, with a seeded stand-in for the walk: the column where the path leaves a chunk is some
// column 1 ... J of it.  tests/test_align_pair_plan.py asserts the plan's properties on the output.
#include <cstdio>

#include "nw_pair_trace_plan.h"

int main()
{
    long long TR, iEnd, jEnd, limit;
    unsigned long long seed;
    while (std::scanf("%lld %lld %lld %lld %llu", &TR, &iEnd, &jEnd, &limit, &seed) == 5)
    {
        const long long strips = gsa::pair_strips(TR, iEnd);
        std::printf("plan %lld\n", strips);
        long long tHi = strips - 1, J = jEnd;
        for (;;)
        {
            gsa::PairChunk c;
            if (!gsa::pair_plan_chunk(TR, tHi, J, limit, &c))
            {
                std::printf("nofit %lld %lld\n", tHi, gsa::pair_strip_bytes(TR, J));
                break;
            }
            std::printf("chunk %lld %lld %lld %lld %lld %lld\n", c.tLo, c.tHi, c.J, c.stripBytes, c.codeBytes,
                        gsa::pair_chunk_stop_row(TR, c));
            for (long long s = c.tLo; s <= c.tHi; ++s) std::printf("strip %lld %lld\n", s, gsa::pair_code_off(c, s));
            if (c.tLo == 0) break;
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            J = 1 + (long long)((seed >> 33) % (unsigned long long)c.J);  // the path never moves right
            tHi = c.tLo - 1;
        }
        std::printf("end\n");
    }
    return 0;
}
