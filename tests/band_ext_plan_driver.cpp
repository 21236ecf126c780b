// band_ext_plan_driver.cpp -- a stand-alone program over gpuseqalign_amd/csrc/nw_band_ext_plan.h
// (tests/test_align_pair_band_ext_plan.py compiles and runs it).  Modes:
//   check                        validity, trim, plan and certificate on hand-computed cases, and the trim's
//                                properties over every band of every pair with R, C <= 24
//   plan R C lo hi               print validity, the trimmed pair and its plan
//   cert R C lo hi pmax go ge S  print the certificate (lo, hi as given: the caller clamps)
// It exits 0 when every check holds and prints what it ran.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nw_band_ext_plan.h"

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

void run_check()
{
    // validity: the band holds (0, 0), whatever R and C
    CHECK(band_ext_valid(0, 0) && band_ext_valid(-3, 0) && band_ext_valid(0, 7) && band_ext_valid(-1000000, 1000000));
    CHECK(!band_ext_valid(1, 5) && !band_ext_valid(-5, -1) && !band_ext_valid(2, 1) && !band_ext_valid(1, 0));
    // the trim, by hand: 768 rows against 100 columns with lo = -20: rows beyond 120 hold no cell
    int64_t Ru = 0, Cu = 0;
    band_ext_trim(768, 100, -20, 5, &Ru, &Cu);
    CHECK(Ru == 120 && Cu == 100);
    band_ext_trim(100, 20000, -7, 30, &Ru, &Cu);
    CHECK(Ru == 100 && Cu == 130);
    band_ext_trim(100, 120, -100000, 100000, &Ru, &Cu);
    CHECK(Ru == 100 && Cu == 120);
    band_ext_trim(0, 9, -4, 4, &Ru, &Cu);
    CHECK(Ru == 0 && Cu == 4);
    // every band of every small pair: at most one side is cut, the band holds the trimmed corner, the
    // clamped band of the trimmed pair is that of the whole pair, and no cell of the band lies beyond
    for (int64_t R = 1; R <= 24; ++R)
        for (int64_t C = 1; C <= 24; ++C)
            for (int64_t lo = -R - 2; lo <= 0; ++lo)
                for (int64_t hi = 0; hi <= C + 2; ++hi)
                {
                    band_ext_trim(R, C, lo, hi, &Ru, &Cu);
                    int64_t clo = lo, chi = hi;
                    band_clamp(R, C, &clo, &chi);
                    CHECK(Ru >= 1 && Ru <= R && Cu >= 1 && Cu <= C && (Ru == R || Cu == C));
                    CHECK(band_valid(Ru, Cu, clo, chi));
                    int64_t tlo = clo, thi = chi;
                    band_clamp(Ru, Cu, &tlo, &thi);
                    CHECK(tlo == clo && thi == chi);
                    int64_t imax = 0, jmax = 0;
                    for (int64_t i = 0; i <= R; ++i)
                        for (int64_t j = 0; j <= C; ++j)
                            if (j - i >= lo && j - i <= hi)
                            {
                                imax = band_max(imax, i);
                                jmax = band_max(jmax, j);
                            }
                    CHECK(imax == Ru && jmax == Cu);  // the trim is tight
                    BandPlan p, q;
                    int64_t Rp = 0, Cp = 0;
                    CHECK(band_ext_plan(R, C, lo, hi, &Rp, &Cp, &p) && Rp == Ru && Cp == Cu);
                    CHECK(band_plan(Ru, Cu, clo, chi, &q));
                    CHECK(p.lo == clo && p.hi == chi && p.strips == q.strips && p.T == q.T && p.codeBytes == q.codeBytes);
                }
    // the plan of the trimmed pair, by hand: 3 TR rows, 100 columns, band -20 ... 5 -> one strip of 120 rows,
    // W = 26, Wc = 281, nq = ceil((281 + 63) / 64) = 6, T = 6
    BandPlan p;
    CHECK(band_ext_plan(3 * kBandTR, 100, -20, 5, &Ru, &Cu, &p));
    CHECK(Ru == 120 && Cu == 100 && p.strips == 1 && p.W == 26 && p.Wc == 26 + kBandTR - 1 && p.nq == 6 && p.T == 6);
    CHECK(p.codeBytes == p.Wc * (kBandTR / 2));
    // a band the global call refuses (it does not hold C - R) is planned here; one without (0, 0) is not
    CHECK(!band_plan(1000, 700, -10, 10, &p) && band_ext_plan(1000, 700, -10, 10, &Ru, &Cu, &p) && Ru == 710 && Cu == 700);
    CHECK(!band_ext_plan(1000, 700, 1, 10, &Ru, &Cu, &p) && !band_ext_plan(1000, 700, -10, -1, &Ru, &Cu, &p));
    CHECK(!band_ext_plan(0, 700, 0, 10, &Ru, &Cu, &p) && !band_ext_plan(700, 0, 0, 10, &Ru, &Cu, &p));
    // the width limit applies after clamping
    CHECK(band_ext_plan(20000, 20000, -(kBandMaxWidth - 1) / 2, kBandMaxWidth / 2, &Ru, &Cu, &p) && p.W == kBandMaxWidth);
    CHECK(!band_ext_plan(20000, 20000, -(kBandMaxWidth - 1) / 2 - 1, kBandMaxWidth / 2, &Ru, &Cu, &p));
    CHECK(band_ext_plan(100, 100, -1000000, 1000000, &Ru, &Cu, &p) && p.W == 201);

    // the certificate, by hand: R = 10, C = 12, pmax 2, go -3, ge -1
    //   band -3 ... 5: U_hi = 2 min(10, 12 - 5 - 1) - 3 - 5 = 4; a = 4: U_lo = 2 min(12, 10 - 4) - 3 - 3 = 6
    CHECK(band_ext_certificate(10, 12, -3, 5, 2, -3, -1, 7) == 1 && band_ext_certificate(10, 12, -3, 5, 2, -3, -1, 6) == 0);
    //   band -8 ... 5: a = 9: U_lo = 2 - 3 - 8 = -9; U_hi = 4 decides
    CHECK(band_ext_certificate(10, 12, -8, 5, 2, -3, -1, 5) == 1 && band_ext_certificate(10, 12, -8, 5, 2, -3, -1, 4) == 0);
    //   band -3 ... 12: the high side reaches the corner, U_lo = 6 alone
    CHECK(band_ext_certificate(10, 12, -3, 12, 2, -3, -1, 7) == 1 && band_ext_certificate(10, 12, -3, 12, 2, -3, -1, 6) == 0);
    //   band -10 ... 5: the low side reaches the corner, U_hi = 4 alone
    CHECK(band_ext_certificate(10, 12, -10, 5, 2, -3, -1, 5) == 1 && band_ext_certificate(10, 12, -10, 5, 2, -3, -1, 4) == 0);
    //   the whole matrix: nothing to leave; a score of 0 is certified there and only there with pmax > 0 ...
    CHECK(band_ext_certificate(10, 12, -10, 12, 2, -3, -1, 0) == 1);
    //   ... band 0 ... 0 on a long pair: U_hi = 2 min(10, 11) - 3 = 17
    CHECK(band_ext_certificate(10, 12, 0, 0, 2, -3, -1, 17) == 0 && band_ext_certificate(10, 12, 0, 0, 2, -3, -1, 18) == 1);
    //   a table without a positive value: U = go + ... < 0 <= S, always certified
    CHECK(band_ext_certificate(10, 12, 0, 0, 0, -3, -1, 0) == 1);
    //   min(R, .) binds: R = 3, C = 100, hi = 4: U_hi = 2 x 3 - 3 - 4 = -1
    CHECK(band_ext_certificate(3, 100, -3, 4, 2, -3, -1, 0) == 1);
    std::printf("check ok checks %lld max_width %lld\n", g_checks, (long long)kBandMaxWidth);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc >= 2 && std::strcmp(argv[1], "check") == 0)
    {
        run_check();
        return 0;
    }
    if (argc == 6 && std::strcmp(argv[1], "plan") == 0)
    {
        const long long R = std::atoll(argv[2]), C = std::atoll(argv[3]), lo = std::atoll(argv[4]), hi = std::atoll(argv[5]);
        BandPlan p;
        int64_t Ru = 0, Cu = 0;
        if (!band_ext_plan(R, C, lo, hi, &Ru, &Cu, &p))
        {
            std::printf("refused valid %d\n", band_ext_valid(lo, hi) ? 1 : 0);
            return 0;
        }
        std::printf("plan %lld %lld %lld %lld %lld %lld %lld %d %lld %lld %lld %lld\n", (long long)Ru, (long long)Cu, (long long)p.lo,
                    (long long)p.hi, (long long)p.W, (long long)p.Wc, (long long)p.strips, p.waves, (long long)p.nq, (long long)p.T,
                    (long long)p.stripBytes, (long long)p.codeBytes);
        return 0;
    }
    if (argc == 10 && std::strcmp(argv[1], "cert") == 0)
    {
        long long v[8];
        for (int k = 0; k < 8; ++k) v[k] = std::atoll(argv[2 + k]);
        std::printf("cert %d\n", band_ext_certificate(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]));
        return 0;
    }
    std::fprintf(stderr, "usage: %s check | plan R C lo hi | cert R C lo hi pmax go ge S\n", argv[0]);
    return 2;
}
