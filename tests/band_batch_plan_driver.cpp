// band_batch_plan_driver.cpp -- a stand-alone program over gpuseqalign_amd/csrc/nw_band_batch_plan.h
// (tests/test_align_batch_band_plan.py compiles and runs it).  Modes:
//   schedule   simulate the lockstep super-step schedule of a pair on a workgroup of 4, 8 and 16 waves --
//              the batch kernel's workgroup has that many whatever the pair's strips -- for every width
//              whose chain length falls on either side of a multiple of 64 up to the count's width
//              limit, the limit itself, the limit - 1 and (with no more strips than waves; with more it
//              must be refused) the limit + 1, and for 1, 2, nwv, nwv + 1 and 3 nwv + 1 strips, and
//              check: every ring entry a consumer reads unmasked, the diagonal's cell included, was
//              written by the producer strip in a strictly earlier super-step; no wave holds two strips
//              at once; T ends with the last strip.  Then the waves rule, the claim order and the round
//              plan on generated batches.
//   rounds limit b0 b1 ...     print the round plan of the code bytes b0, b1, ... (negative: no part)
//   waves forced s0 n0 s1 n1 ...  print the waves of a launch of pairs (strips, nq)
// It exits 0 when every check holds and prints what it ran.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nw_band_batch_plan.h"

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

// The schedule of one pair on nwv waves: R rows in `strips` strips, a band of W diagonals.  The ring
// starts with what a pair before left in it (strip -1 never matches).
void simulate(int nwv, long long strips, long long W)
{
    const long long R = strips * kBandTR - 3;
    BandPlan p;
    CHECK(band_plan(R, R + W - 1, 0, W - 1, &p));  // the diagonals 0 ... W - 1: the schedule depends on R and W only
    CHECK(p.W == W && p.strips == strips && p.T == (strips - 1) * kBandLag + p.nq);
    CHECK(band_waves_ok(nwv, strips, p.nq));
    const long long nq = p.nq, Wc = p.Wc, T = p.T;
    std::vector<Slot> ring((size_t)nwv * kBandRingBlocks * 64);
    auto slot = [&](int w, long long g, int u) -> Slot& { return ring[((size_t)w * kBandRingBlocks + (size_t)(g % kBandRingBlocks)) * 64 + u]; };
    std::vector<long long> cur((size_t)nwv);  // the strip a wave runs, or runs next, as the kernel keeps it
    for (int w = 0; w < nwv; ++w) cur[(size_t)w] = w;
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
            const long long s = cur[(size_t)w], q = g - s * kBandLag;
            if (!(s < strips && q >= 0)) continue;
            CHECK(q < nq && s % nwv == w);
            if (s == 0) continue;
            const int pw = (w + nwv - 1) % nwv;
            if (q == 0)
            {
                // the cell above lane 0's first one: the producer's column TR - 1, at [g - lag + KR][62]
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
            const long long s = cur[(size_t)w], q = g - s * kBandLag;
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
                cur[(size_t)w] += nwv;
                ++finished;
                lastEnd = g;
            }
        }
    }
    CHECK(finished == strips && lastEnd == T - 1);  // T is exactly what the last strip needs
}

long long nq_of(long long W) { return (W + kBandTR - 1 + 63 + 63) / 64; }

unsigned long long g_rng = 0x9e3779b97f4a7c15ull;
long long rnd(long long n)
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (long long)((g_rng >> 33) % (unsigned long long)n);
}

void check_rounds(const std::vector<int64_t>& bytes, int64_t limit)
{
    const BandBatchRounds r = band_batch_rounds(bytes, limit);
    const BandBatchRounds again = band_batch_rounds(bytes, limit);
    CHECK(r.rounds == again.rounds && r.nocode == again.nocode && r.roundOf == again.roundOf);  // deterministic
    std::vector<int> seen(bytes.size(), 0);
    int64_t peak = 0;
    for (size_t k = 0; k < r.rounds.size(); ++k)
    {
        int64_t sum = 0;
        CHECK(!r.rounds[k].empty());
        for (size_t m = 0; m < r.rounds[k].size(); ++m)
        {
            const int p = r.rounds[k][m];
            CHECK(p >= 0 && (size_t)p < bytes.size() && bytes[(size_t)p] >= 0 && bytes[(size_t)p] <= limit);
            CHECK(r.roundOf[(size_t)p] == (int)k);
            seen[(size_t)p] += 1;
            sum += bytes[(size_t)p];
            // within a round: code bytes descending, ties by index
            if (m > 0)
            {
                const int b = r.rounds[k][m - 1];
                CHECK(bytes[(size_t)b] > bytes[(size_t)p] || (bytes[(size_t)b] == bytes[(size_t)p] && b < p));
            }
        }
        CHECK(sum <= limit);
        peak = std::max(peak, sum);
        // first fit: no pair of a later round would still have fitted behind the pairs taken before it
        for (size_t k2 = k + 1; k2 < r.rounds.size(); ++k2)
            for (int p2 : r.rounds[k2])
            {
                int64_t before = 0;
                for (int p : r.rounds[k])
                    if (bytes[(size_t)p] > bytes[(size_t)p2] || (bytes[(size_t)p] == bytes[(size_t)p2] && p < p2))
                        before += bytes[(size_t)p];
                CHECK(before + bytes[(size_t)p2] > limit);
            }
    }
    CHECK(peak == r.peakBytes);
    for (int p : r.nocode)
    {
        CHECK(bytes[(size_t)p] > limit && r.roundOf[(size_t)p] == -2);
        seen[(size_t)p] += 1;
    }
    for (size_t p = 0; p < bytes.size(); ++p)
    {
        CHECK(seen[p] == (bytes[p] < 0 ? 0 : 1));  // exactly one place
        if (bytes[p] < 0) CHECK(r.roundOf[p] == -3);
    }
}

void run_schedule()
{
    long long sims = 0;
    for (int nwv : kBandBatchWaves)
    {
        const long long limit = band_waves_max_width(nwv);
        CHECK(nq_of(limit) == (long long)nwv * kBandLag && nq_of(limit + 1) == (long long)nwv * kBandLag + 1);
        const long long stripsList[] = {1, 2, nwv, nwv + 1, 3 * nwv + 1};
        for (long long W = 1; W <= limit + 1; ++W)
        {
            const long long chain = W + kBandTR - 1 + 63, m = chain % 64;
            const bool edge = m == 63 || m == 0 || m == 1;
            if (!(edge || W <= 4 || W >= limit - 1)) continue;
            if (W > kBandMaxWidth) continue;  // band_plan() refuses it on any count
            for (long long strips : stripsList)
            {
                if (W == limit + 1 && strips > nwv)
                {
                    CHECK(!band_waves_ok(nwv, strips, nq_of(W)));  // the wave would hold two strips: refused
                    continue;
                }
                simulate(nwv, strips, W);
                ++sims;
            }
        }
    }
    CHECK(band_waves_max_width(4) == 1218 && band_waves_max_width(8) == 2754 && band_waves_max_width(16) == 5826);
    CHECK(band_waves_max_width(kBandWaves) == kBandMaxWidth);

    // the waves rule: the smallest admissible count; pairs with strips <= nwv do not constrain it
    {
        const int64_t s1[] = {9, 3}, n1[] = {nq_of(1218), nq_of(5000)};
        CHECK(band_batch_waves(s1, n1, 2) == 4);  // 3 strips fit 4 waves whatever the width
        const int64_t s2[] = {9, 5}, n2[] = {nq_of(1218), nq_of(1219)};
        CHECK(band_batch_waves(s2, n2, 2) == 8);  // 5 strips at 1219: not on 4
        const int64_t s3[] = {9, 8}, n3[] = {nq_of(1218), nq_of(5826)};
        CHECK(band_batch_waves(s3, n3, 2) == 8);  // 8 strips fit 8 waves
        const int64_t s4[] = {9, 9}, n4[] = {nq_of(1218), nq_of(2755)};
        CHECK(band_batch_waves(s4, n4, 2) == 16);
        const int64_t s5[] = {17}, n5[] = {nq_of(2754)};
        CHECK(band_batch_waves(s5, n5, 1) == 8 && band_batch_pick_waves(4, s5, n5, 1) == 0);
        CHECK(band_batch_pick_waves(8, s5, n5, 1) == 8 && band_batch_pick_waves(16, s5, n5, 1) == 16);
        CHECK(band_batch_pick_waves(0, s5, n5, 1) == 8 && band_batch_pick_waves(5, s5, n5, 1) == 0);
        CHECK(band_batch_pick_waves(-4, s5, n5, 1) == 0 && band_batch_pick_waves(32, s5, n5, 1) == 0);
        CHECK(band_batch_waves(nullptr, nullptr, 0) == 4);
        for (int k = 0; k < 2000; ++k)
        {
            int64_t s[3], n[3];
            for (int m = 0; m < 3; ++m)
            {
                s[m] = 1 + rnd(40);
                n[m] = nq_of(1 + rnd(kBandMaxWidth));
            }
            const int w = band_batch_waves(s, n, 3);
            CHECK(w == 4 || w == 8 || w == 16);
            for (int m = 0; m < 3; ++m) CHECK(band_waves_ok(w, s[m], n[m]));
            for (int smaller : kBandBatchWaves)
            {
                if (smaller >= w) break;
                bool ok = true;
                for (int m = 0; m < 3; ++m) ok = ok && band_waves_ok(smaller, s[m], n[m]);
                CHECK(!ok);
            }
        }
    }

    // the claim order: T descending, ties by index, a permutation
    {
        const std::vector<int64_t> T = {7, 30, 7, 100, 30, 1};
        const std::vector<int> o = band_batch_order(T);
        const std::vector<int> want = {3, 1, 4, 0, 2, 5};
        CHECK(o == want);
    }

    // the round plan
    check_rounds({}, 100);
    check_rounds({-1, -1}, 100);
    {
        // one pair: the single call's plan -- codes iff they fit the limit
        const BandBatchRounds a = band_batch_rounds({500}, 500), b = band_batch_rounds({500}, 499);
        CHECK(a.rounds.size() == 1 && a.rounds[0] == std::vector<int>{0} && a.nocode.empty() && a.peakBytes == 500);
        CHECK(b.rounds.empty() && b.nocode == std::vector<int>{0} && b.peakBytes == 0 && b.roundOf[0] == -2);
        // by hand: limit 10 over 6 4 4 3 3 (-) 11 -> {6, 4}, {4, 3, 3}; 11 without codes
        const BandBatchRounds c = band_batch_rounds({4, 3, 6, 11, -1, 4, 3}, 10);
        CHECK(c.rounds.size() == 2 && c.rounds[0] == (std::vector<int>{2, 0}) && c.rounds[1] == (std::vector<int>{5, 1, 6}));
        CHECK(c.nocode == std::vector<int>{3} && c.peakBytes == 10 && c.roundOf[4] == -3);
    }
    for (int k = 0; k < 3000; ++k)
    {
        const size_t n = (size_t)rnd(12);
        const int64_t limit = 1 + rnd(1000);
        std::vector<int64_t> bytes(n);
        for (size_t p = 0; p < n; ++p) bytes[p] = rnd(8) == 0 ? -1 : rnd(3) == 0 ? limit - rnd(3) + 1 : rnd(1100);
        check_rounds(bytes, limit);
    }
    std::printf("schedule ok sims %lld checks %lld\n", sims, g_checks);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc >= 2 && std::strcmp(argv[1], "schedule") == 0)
    {
        run_schedule();
        return 0;
    }
    if (argc >= 3 && std::strcmp(argv[1], "rounds") == 0)
    {
        std::vector<int64_t> bytes;
        for (int k = 3; k < argc; ++k) bytes.push_back(std::atoll(argv[k]));
        const BandBatchRounds r = band_batch_rounds(bytes, std::atoll(argv[2]));
        std::printf("rounds %zu peak %lld of", r.rounds.size(), (long long)r.peakBytes);
        for (int v : r.roundOf) std::printf(" %d", v);
        std::printf("\n");
        return 0;
    }
    if (argc >= 3 && (argc - 3) % 2 == 0 && std::strcmp(argv[1], "waves") == 0)
    {
        std::vector<int64_t> s, n;
        for (int k = 3; k + 1 < argc; k += 2)
        {
            s.push_back(std::atoll(argv[k]));
            n.push_back(std::atoll(argv[k + 1]));
        }
        std::printf("waves %d\n", band_batch_pick_waves(std::atoi(argv[2]), s.data(), n.data(), s.size()));
        return 0;
    }
    std::fprintf(stderr, "usage: %s schedule | rounds limit b0 b1 ... | waves forced s0 n0 s1 n1 ...\n", argv[0]);
    return 2;
}
