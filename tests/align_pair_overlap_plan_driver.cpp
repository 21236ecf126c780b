// Stand-alone driver over gpuseqalign_amd/csrc/nw_pair_overlap_plan.h (no HIP, no GPU): reads cases
// "TR iEnd jEnd limit seed" from standard input and prints the chunks gsa_align_pair_overlap_dev would
// take, bottom-up from i_end's strip, with a seeded stand-in for the walk: it leaves a chunk on its
// upper boundary at some column 0 ... J of it (0: it has reached column 0 and is done), or, every fourth
// time, ends inside the chunk.  tests/test_align_pair_overlap_plan.py asserts the plan's properties on
// the output.
#include <cstdio>

#include "nw_pair_overlap_plan.h"

int main()
{
    long long TR, iEnd, jEnd, limit;
    unsigned long long seed;
    while (std::scanf("%lld %lld %lld %lld %llu", &TR, &iEnd, &jEnd, &limit, &seed) == 5)
    {
        std::printf("plan %lld %lld\n", gsa::pair_strips(TR, iEnd), gsa::overlap_end_strip(TR, iEnd));
        long long tHi = gsa::overlap_end_strip(TR, iEnd), J = jEnd;
        for (;;)
        {
            gsa::PairChunk c;
            if (!gsa::overlap_plan_chunk(TR, tHi, J, limit, &c))
            {
                std::printf("nofit %lld %lld\n", tHi, J >= 1 ? gsa::pair_strip_bytes(TR, J) : -1);
                break;
            }
            std::printf("chunk %lld %lld %lld %lld %lld %lld\n", c.tLo, c.tHi, c.J, c.stripBytes, c.codeBytes,
                        gsa::pair_chunk_stop_row(TR, c));
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            const bool inside = ((seed >> 20) & 3) == 0;  // the walk reached column 0 inside the chunk
            const long long i = inside ? gsa::pair_chunk_stop_row(TR, c) + 1 : gsa::pair_chunk_stop_row(TR, c);
            const long long j = inside ? 0 : (long long)((seed >> 33) % (unsigned long long)(c.J + 1));  // never moves right
            std::printf("walk %lld %lld\n", i, j);
            if (!gsa::overlap_walk_goes_on(TR, c, i, j)) break;
            J = j;
            tHi = c.tLo - 1;
        }
        std::printf("end\n");
    }
    return 0;
}
