// nw_band_plan.h -- the banded alignment of one long pair (gsa_score_band_dev, gsa_align_pair_band_dev;
// DESIGN.md 2.2p): the geometry of the strips, the lockstep schedule of the waves, the bytes of move
// codes and the optimality certificate.  HIP-free, so that a plain C++ program can check it
// (tests/band_plan_driver.cpp); used by nw_band.hip and gsa_score.hip.
//
// The band is the set of cells (i, j) with lo <= j - i <= hi.  Strip s holds the rows s TR + 1 ...
// (s + 1) TR, lane l of its wave the rows s TR + l KR + 1 ... s TR + (l + 1) KR.  The strip's column
// origin is o(s) = s TR + 1 + lo, the first in-band column of its first row; its last row ends at
// (s + 1) TR + hi, so the strip touches the Wc = W + TR - 1 columns from o(s).  Lane l runs one column
// behind lane l - 1: at the strip's step t it stands on column o(s) + t - l, and the chain of a strip is
// Wc + 63 steps, cut into nq super-steps of 64 steps with one workgroup barrier between super-steps.
// Strip s starts at the workgroup's super-step s lag on wave s mod NWV.
#pragma once
#include <stdint.h>

namespace gsa {

// Rows per lane: 4, so a lane's codes of a column are two bytes (8 rows per lane were measured and lost on
// narrow bands: DESIGN.md 2.2p).
constexpr int kBandKR = 4;
constexpr int kBandTR = 64 * kBandKR;      // rows of a strip
constexpr int kBandWaves = 16;             // NWV: waves of the workgroup
// Lane 0 of strip s + 1 at its step t needs row (s + 1) TR at column o(s + 1) + t = o(s) + TR + t, which
// lane 63 of strip s finishes at its step TR + t + 63, in its super-step KR + (t + 63) / 64, that is
// the workgroup's super-step s lag + KR + (t + 63) / 64.  The consumer stands in the workgroup's
// super-step (s + 1) lag + t / 64.  (t + 63) / 64 <= t / 64 + 1, with equality for every t that is no
// multiple of 64, so the producer's super-step is strictly earlier iff KR + 1 < lag.
constexpr int kBandLag = kBandKR + 2;
// The hand-off ring of a wave is indexed by the workgroup's super-step, not by the column: a consumer
// in super-step g reads what its producer wrote in the super-steps g - lag + KR (step 63 of it) and
// g - lag + KR + 1 (steps 0 ... 62), and the producer writes block g meanwhile.  lag - KR + 1 blocks
// keep the three apart, whichever strip of the producing wave wrote them.
constexpr int kBandRingBlocks = kBandLag - kBandKR + 1;
// A wave is free for its next strip (s + NWV) when strip s is done: nq <= NWV lag, that is
// W + TR - 1 + 63 <= 64 NWV lag.
constexpr int64_t kBandMaxWidth = 64ll * kBandWaves * kBandLag - kBandTR + 1 - 63;
static_assert(kBandMaxWidth >= 4096, "the width limit the interface promises");
static_assert(kBandLag >= kBandKR + 2, "a producer's super-step must be strictly earlier than its consumer's");
// Default of gsa_align_pair_band_dev's scratch_limit: bytes of move codes.
constexpr int64_t kBandScratch = 2ll << 30;

struct BandPlan
{
    int64_t lo = 0, hi = 0;  // the clamped band
    int64_t W = 0, Wc = 0;   // diagonals; columns a strip touches
    int64_t strips = 0;
    int waves = 0;           // waves of the workgroup: min(NWV, strips)
    int64_t nq = 0;          // super-steps of a strip
    int64_t T = 0;           // super-steps (barriers) of the workgroup
    int64_t stripBytes = 0;  // bytes of move codes of a strip: column j - o(s) at (j - o(s)) TR / 2
    int64_t codeBytes = 0;   // of all strips
};

inline int64_t band_min(int64_t a, int64_t b) { return a < b ? a : b; }
inline int64_t band_max(int64_t a, int64_t b) { return a > b ? a : b; }

// The band holds (0, 0) and (R, C): an alignment exists.
inline bool band_valid(int64_t R, int64_t C, int64_t lo, int64_t hi)
{
    return lo <= hi && lo <= band_min(0, C - R) && hi >= band_max(0, C - R);
}

// A valid band clamped to the matrix: diagonals below -R and above C hold no cell.
inline void band_clamp(int64_t R, int64_t C, int64_t* lo, int64_t* hi)
{
    *lo = band_max(*lo, -R);
    *hi = band_min(*hi, C);
}

// The plan of a pair with R, C >= 1.  False: the band is invalid, or wider than kBandMaxWidth after
// clamping.
inline bool band_plan(int64_t R, int64_t C, int64_t lo, int64_t hi, BandPlan* p)
{
    if (R < 1 || C < 1 || !band_valid(R, C, lo, hi)) return false;
    band_clamp(R, C, &lo, &hi);
    BandPlan b;
    b.lo = lo;
    b.hi = hi;
    b.W = hi - lo + 1;
    if (b.W > kBandMaxWidth) return false;
    b.Wc = b.W + kBandTR - 1;
    b.strips = (R + kBandTR - 1) / kBandTR;
    b.waves = (int)band_min(kBandWaves, b.strips);
    b.nq = (b.Wc + 63 + 63) / 64;
    b.T = (b.strips - 1) * kBandLag + b.nq;
    b.stripBytes = b.Wc * (kBandTR / 2);
    b.codeBytes = b.strips * b.stripBytes;
    *p = b;
    return true;
}

// The certificate: 1 iff the banded score S exceeds what any path that leaves the (clamped) band can
// reach.  Such a path on the high side holds at least hi + 1 letters of D and hi + 1 - (C - R) of I, in
// at least one run each, and at most C - hi - 1 diagonal steps; on the low side the mirror image with
// a = 1 - lo.  pmax: max(0, the largest table value).  A side the band reaches the matrix's corner on
// (hi = C, lo = -R) cannot be left.  Strict, so that ties are safe: then every optimal alignment of the
// unbanded problem lies in the band, and the walk's tie rule sees the same values.
inline int band_certificate(int64_t R, int64_t C, int64_t lo, int64_t hi, int64_t pmax, int64_t go, int64_t ge, int64_t S)
{
    const int64_t D = C - R;
    if (hi < C)
    {
        const int64_t U = pmax * (C - hi - 1) + 2 * go + hi * ge + (hi - D) * ge;
        if (S <= U) return 0;
    }
    if (lo > -R)
    {
        const int64_t a = 1 - lo;
        const int64_t U = pmax * (R - a) + 2 * go + (a - 1) * ge + (a + D - 1) * ge;
        if (S <= U) return 0;
    }
    return 1;
}

}  // namespace gsa
