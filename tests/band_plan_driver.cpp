// band_plan_driver.cpp -- a stand-alone program over gpuseqalign_amd/csrc/nw_band_plan.h
// (tests/test_align_pair_band_plan.py compiles and runs it).  Modes:
//   schedule   simulate the lockstep super-step schedule of nw_band.hip for every width W whose chain
//              length Wc + 63 falls on either side of a multiple of 64 (and a few small ones) and for
//              1, 2, NWV, NWV + 1 and 3 NWV + 1 strips, and check: every column a consumer reads was
//              written in a strictly earlier super-step and still stands in its ring; no wave holds two
//              strips at once; the workgroup's T and the bytes of codes are as stated.
//   plan R C lo hi             print the plan of one pair
//   cert R C lo hi pmax go ge S  print the certificate (lo, hi as given: the caller clamps)
// It exits 0 when every check holds and prints what it ran.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nw_band_plan.h"

using namespace gsa;

namespace {

long long g_checks = 0;

#define CHECK(c)                                                                        \
    do                                                                                  \
    {                                                                                   \
        ++g_checks;                                                                     \
        if (!(c))                                                                       \
        {                                                                               \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

struct Slot
{
    long long strip = -1, col = -1, g = -1;  // what stands in the slot: the strip's column, written in super-step g
};

// The schedule of one pair: R rows in `strips` strips, a band of W diagonals.
void simulate(long long strips, long long W)
{
    const long long R = strips * kBandTR - 3;
    BandPlan p;
    CHECK(band_plan(R, R + W - 1, 0, W - 1, &p));  // the diagonals 0 ... W - 1: the schedule depends on R and W only
    CHECK(p.W == W && p.strips == strips && p.waves == (int)band_min(kBandWaves, strips));
    CHECK(p.T == (strips - 1) * kBandLag + p.nq);
    const long long nq = p.nq, Wc = p.Wc, T = p.T;
    const int nwv = p.waves;
    CHECK(nq * 64 >= Wc + 63 && (nq - 1) * 64 < Wc + 63);  // the chain fits its super-steps, tightly
    CHECK(strips <= nwv || nq <= (long long)nwv * kBandLag);
    std::vector<Slot> ring((size_t)kBandWaves * kBandRingBlocks * 64);
    auto slot = [&](int w, long long g, int u) -> Slot& { return ring[((size_t)w * kBandRingBlocks + (size_t)(g % kBandRingBlocks)) * 64 + u]; };
    std::vector<long long> cur(nwv);  // the strip a wave runs, or runs next, as the kernel keeps it
    for (int w = 0; w < nwv; ++w) cur[w] = w;
    long long finished = 0, lastEnd = -1;
    for (long long g = 0; g < T; ++g)
    {
        // no wave holds two strips: of the strips of a wave, at most one has s lag <= g < s lag + nq
        for (int w = 0; w < nwv; ++w)
        {
            int live = 0;
            for (long long s = w; s < strips; s += nwv) live += (s * kBandLag <= g && g < s * kBandLag + nq) ? 1 : 0;
            CHECK(live <= 1);
        }
        // reads, at the start of the super-step
        for (int w = 0; w < nwv; ++w)
        {
            const long long s = cur[w], q = g - s * kBandLag;
            if (!(s < strips && q >= 0)) continue;
            CHECK(q < nq && s % nwv == w);
            if (s == 0) continue;
            const int pw = (w + nwv - 1) % nwv;
            if (q == 0)
            {
                // the cell above lane 0's first one: the producer's column TR - 1
                const Slot& v = slot(pw, g - kBandLag + kBandKR, 62);
                CHECK(v.strip == s - 1 && v.col == kBandTR - 1 && v.g < g);
            }
            for (int l = 0; l < 64; ++l)
            {
                const long long need = kBandTR + 64 * q + l;  // the producer's column under lane 0 at step 64 q + l
                if (need >= Wc) continue;                      // off the band for that row: the consumer masks it
                const long long gp = g - kBandLag + kBandKR + ((l + 63) >> 6);
                CHECK(gp >= 0 && gp < g);
                const Slot& v = slot(pw, gp, (l + 63) & 63);
                CHECK(v.strip == s - 1 && v.col == need && v.g == gp && v.g < g);
            }
        }
        // writes, during the super-step: lane 63 of every live strip
        for (int w = 0; w < nwv; ++w)
        {
            const long long s = cur[w], q = g - s * kBandLag;
            if (!(s < strips && q >= 0)) continue;
            for (int u = 0; u < 64; ++u)
            {
                Slot& v = slot(w, g, u);
                v.strip = s;
                v.col = 64 * q + u - 63;
                v.g = g;
            }
            if (q == nq - 1)
            {
                cur[w] += nwv;
                ++finished;
                lastEnd = g;
            }
        }
    }
    CHECK(finished == strips && lastEnd == T - 1);  // T is exactly what the last strip needs
}

void run_schedule()
{
    const long long stripsList[] = {1, 2, kBandWaves, kBandWaves + 1, 3 * kBandWaves + 1};
    long long widths = 0;
    for (long long W = 1; W <= kBandMaxWidth; ++W)
    {
        const long long chain = W + kBandTR - 1 + 63, m = chain % 64;
        const bool edge = m == 63 || m == 0 || m == 1;
        if (!(edge || W <= 4 || W == kBandMaxWidth || W == kBandMaxWidth - 1)) continue;
        ++widths;
        for (long long strips : stripsList) simulate(strips, W);
        // the bytes of codes, against the statement: strips x Wc x TR / 2
        BandPlan p;
        const long long R = 5 * kBandTR + 1;
        CHECK(band_plan(R, R + W - 1, 0, W - 1, &p));
        CHECK(p.W == W && p.Wc == W + kBandTR - 1 && p.strips == 6 && p.waves == 6);
        CHECK(p.stripBytes == p.Wc * (kBandTR / 2) && p.codeBytes == 6 * p.Wc * (kBandTR / 2));
        CHECK(p.T == 5 * kBandLag + p.nq && p.nq == (p.Wc + 63 + 63) / 64);
    }
    // the widest band keeps a wave free for its next strip; one more diagonal does not, and is refused
    BandPlan p;
    CHECK(band_plan(20000, 20000, -(kBandMaxWidth - 1) / 2, kBandMaxWidth / 2, &p) && p.W == kBandMaxWidth);
    CHECK(p.nq <= (long long)kBandWaves * kBandLag);
    CHECK(!band_plan(20000, 20000, -(kBandMaxWidth - 1) / 2 - 1, kBandMaxWidth / 2, &p));
    CHECK((kBandMaxWidth + 1 + kBandTR - 1 + 63 + 63) / 64 > (long long)kBandWaves * kBandLag);
    CHECK(kBandMaxWidth >= 4096 && kBandLag >= kBandKR + 2 && kBandRingBlocks == kBandLag - kBandKR + 1);

    // validity and clamping, by hand
    CHECK(band_valid(5, 9, 0, 4) && band_valid(9, 5, -4, 0) && band_valid(3, 3, 0, 0));
    CHECK(!band_valid(5, 9, 0, 3) && !band_valid(5, 9, 1, 4) && !band_valid(9, 5, -3, 0) && !band_valid(3, 3, 1, 0));
    int64_t lo = -100, hi = 100;
    band_clamp(5, 9, &lo, &hi);
    CHECK(lo == -5 && hi == 9);
    lo = -2, hi = 6;
    band_clamp(5, 9, &lo, &hi);
    CHECK(lo == -2 && hi == 6);
    CHECK(band_plan(700, 1000, -1000000, 1000000, &p) && p.lo == -700 && p.hi == 1000 && p.W == 1701 && p.strips == 3);
    CHECK(!band_plan(700, 1000, 0, 299, &p) && !band_plan(700, 1000, 1, 300, &p) && band_plan(700, 1000, 0, 300, &p));
    // 700 rows of 301 diagonals, by hand (TR = 256, lag 6): 3 strips of 556 columns, 10 super-steps each
    CHECK(p.W == 301 && p.Wc == 556 && p.nq == 10 && p.T == 22 && p.waves == 3 && p.codeBytes == 3 * 556 * 128);

    // the certificate, by hand: R = 10, C = 12 (D = 2), pmax 2, go -3, ge -1
    //   band -3 ... 5: U_hi = 2 (12 - 5 - 1) - 6 - 5 - (5 - 2) = -2; a = 4: U_lo = 2 (10 - 4) - 6 - 3 - (4 + 2 - 1) = -2
    CHECK(band_certificate(10, 12, -3, 5, 2, -3, -1, -1) == 1 && band_certificate(10, 12, -3, 5, 2, -3, -1, -2) == 0);
    //   band -1 ... 5: a = 2: U_lo = 2 (10 - 2) - 6 - 1 - (2 + 2 - 1) = 6, the larger of the two
    CHECK(band_certificate(10, 12, -1, 5, 2, -3, -1, 7) == 1 && band_certificate(10, 12, -1, 5, 2, -3, -1, 6) == 0);
    //   band -1 ... 12: the high side reaches the corner, U_lo = 6 alone
    CHECK(band_certificate(10, 12, -1, 12, 2, -3, -1, 7) == 1 && band_certificate(10, 12, -1, 12, 2, -3, -1, 6) == 0);
    //   band -10 ... 5: the low side reaches the corner, U_hi = -2 alone
    CHECK(band_certificate(10, 12, -10, 5, 2, -3, -1, -1) == 1 && band_certificate(10, 12, -10, 5, 2, -3, -1, -2) == 0);
    //   the whole matrix: nothing to leave
    CHECK(band_certificate(10, 12, -10, 12, 2, -3, -1, -1000000) == 1);
    //   a table without a positive value: pmax = 0, the minimal band 0 ... 2: U_hi = -6 - 2 - 0 = -8, a = 1: U_lo = -6 - 0 - 2 = -8
    CHECK(band_certificate(10, 12, 0, 2, 0, -3, -1, -8) == 0 && band_certificate(10, 12, 0, 2, 0, -3, -1, -7) == 1);
    std::printf("schedule ok widths %lld checks %lld max_width %lld\n", widths, g_checks, (long long)kBandMaxWidth);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc >= 2 && std::strcmp(argv[1], "schedule") == 0)
    {
        run_schedule();
        return 0;
    }
    if (argc == 6 && std::strcmp(argv[1], "plan") == 0)
    {
        BandPlan p;
        if (!band_plan(std::atoll(argv[2]), std::atoll(argv[3]), std::atoll(argv[4]), std::atoll(argv[5]), &p))
        {
            std::printf("refused\n");
            return 0;
        }
        std::printf("plan %lld %lld %lld %lld %lld %d %lld %lld %lld %lld\n", (long long)p.lo, (long long)p.hi, (long long)p.W,
                    (long long)p.Wc, (long long)p.strips, p.waves, (long long)p.nq, (long long)p.T, (long long)p.stripBytes,
                    (long long)p.codeBytes);
        return 0;
    }
    if (argc == 10 && std::strcmp(argv[1], "cert") == 0)
    {
        long long v[8];
        for (int k = 0; k < 8; ++k) v[k] = std::atoll(argv[2 + k]);
        std::printf("cert %d\n", band_certificate(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]));
        return 0;
    }
    std::fprintf(stderr, "usage: %s schedule | plan R C lo hi | cert R C lo hi pmax go ge S\n", argv[0]);
    return 2;
}
