// Stand-alone driver over gpuseqalign_amd/csrc/nw_pair_semi_plan.h (no HIP, no GPU): reads cases
// "TR R jEnd S pmax gape limit seed" from standard input and prints the window and the chunks
// gsa_align_pair_semi_dev would take, bottom-up from row R's strip to strip 0, with a seeded stand-in
// for the walk: the column where the path leaves a chunk is some column jW + 1 ... J of it.
// tests/test_align_pair_semi_plan.py asserts the window and the plan's properties on the output.
#include <cstdio>

#include "nw_pair_semi_plan.h"

int main()
{
    long long TR, R, jEnd, S, pmax, gape, limit;
    unsigned long long seed;
    while (std::scanf("%lld %lld %lld %lld %lld %lld %lld %llu", &TR, &R, &jEnd, &S, &pmax, &gape, &limit, &seed) == 8)
    {
        const long long strips = gsa::pair_strips(TR, R);
        const long long jW = gsa::semi_window(R, jEnd, S, pmax, gape);
        std::printf("plan %lld %lld\n", strips, jW);
        long long tHi = strips - 1, J = jEnd;
        for (;;)
        {
            gsa::PairChunk c;
            if (!gsa::semi_plan_chunk(TR, tHi, J, jW, limit, &c))
            {
                std::printf("nofit %lld %lld\n", tHi, gsa::pair_strip_bytes(TR, J - jW));
                break;
            }
            std::printf("chunk %lld %lld %lld %lld %lld %lld\n", c.tLo, c.tHi, c.J, c.stripBytes, c.codeBytes,
                        gsa::pair_chunk_stop_row(TR, c));
            if (c.tLo == 0) break;
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            J = jW + 1 + (long long)((seed >> 33) % (unsigned long long)c.J);  // the path never moves right
            tHi = c.tLo - 1;
        }
        std::printf("end\n");
    }
    return 0;
}
