// nw_band_dev.h -- the device code the banded kernels share: the table load, the
// lockstep super-steps of one pair on one workgroup, and the one-lane walk.  Included by nw_band.hip
// (one pair per workgroup of the grid) and by nw_band_batch.hip (a persistent grid whose workgroups
// claim pair after pair), so that both run the same body; nw_band_ext.hip and nw_band_ext_batch.hip run
// it in the extension mode (EXT).
//
// band_pair_fill sets every piece of per-strip state (s, Hp, E, hdiag, fLast, let, xnext, yo, and the
// extension mode's best values) anew when it is entered and ends every super-step, the last one
// included, with __syncthreads(): a workgroup may run it for one pair after another on the same ring,
// and in the extension mode on the same slots, if a barrier of the caller's stands between the pairs
// (thread 0 reads the slots last).  The ring holds
// (blockDim.x / 64) x kBandRingBlocks x 64 int2 and is passed in, so that a caller may size it by its
// waves.  No loop here polls anything: the fill's are bounded by T, 64 and KR, the walk's by R + C.
#pragma once
#include "nw_band.h"
#include "nw_lanes_trace.h"

namespace gsa {
namespace band_dev {

constexpr int KR = kBandKR, TR = kBandTR, LAG = kBandLag, RQ = kBandRingBlocks;
constexpr unsigned kWalkH = 4u;  // the walk's state H; inside a gap the state is the gap's source code

__device__ __forceinline__ int from_lane_above(int own, int src)
{
    // wave_shr:1 over the 64 lanes; lane 0 has no source and keeps `own`
    return __builtin_amdgcn_update_dpp(own, src, 0x138, 0xf, 0xf, false);
}

// sc (go + n ge) in wrapping arithmetic: cells far off the band form values that are thrown away
__device__ __forceinline__ int gap_run(int sc, int go, int n, int ge)
{
    return (int)((unsigned)sc * ((unsigned)go + (unsigned)n * (unsigned)ge));
}

// tab[x letter][y letter] = SC s(y, x) + tag "diagonal", by all threads of the workgroup; the caller
// puts a barrier behind it
template <bool CODES>
__device__ __forceinline__ void band_load_tab(int* tab, const int* subst, int ssz)
{
    constexpr int SC = CODES ? 4 : 1;
    for (int idx = threadIdx.x; idx < ssz * ssz; idx += blockDim.x)
    {
        const int xl = idx / ssz, yl = idx - xl * ssz;
        tab[idx] = SC * subst[yl * ssz + xl] + (CODES ? (int)kDbTraceDiag : 0);
    }
}

// A candidate end cell of the extension mode: the larger value wins, of equal values the smaller row
// (two lanes, or two waves, never hold the same row, so the column need not decide).
__device__ __forceinline__ void best_take(int& v, int& i, int& j, int ov, int oi, int oj)
{
    const bool take = ov > v || (ov == v && oi < i);
    v = take ? ov : v;
    i = take ? oi : i;
    j = take ? oj : j;
}

// The super-steps of pair d, by all threads of the workgroup.  ring: [wave][RQ][64].
//
// EXT (the extension mode, nw_band_ext.hip): the result is the largest H of the band
// and its first cell in row-major order, not H(R, C), and the band need not hold (R, C).  A lane keeps
// the best value of each of its KR rows with its column (strict >: columns ascend, so the first column
// of a row wins), folds them at the strip's last super-step into its running (value, i, j) (strict >:
// rows and the strips of a wave ascend), and behind the last super-step's barrier the lanes of a wave
// reduce theirs by shuffles, every wave writes one slot of `best` ([waves] int4 of LDS, the caller's),
// and behind one more barrier thread 0 takes the best slot and writes the four result words.  Values
// start from (0, (0, 0)): H(0, 0) = 0 is first in row-major order and no border cell exceeds it.
template <bool AFFINE, bool CODES, bool EXT = false>
__device__ __forceinline__ void band_pair_fill(const BandDesc& d, const int* tab, int2* ring, int ssz, int go, int ge,
                                               int4* best = nullptr)
{
    constexpr int SC = CODES ? 4 : 1;             // values are kept as SC v (+ tag)
    constexpr int NEG = -(1 << 29);               // minus infinity: SC x -2^27 with codes, -2^29 without
    constexpr int TF = CODES ? (int)kDbTraceF : 0;
    constexpr int NEGF = NEG | TF;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    const int goS = SC * go, geS = SC * ge;
    const int R = d.R, C = d.C, lo = d.lo, hi = d.hi;
    const int* const x = d.seqX;
    const int prodWave = (wave + nwv - 1) % nwv;
    int2* const ringOwn = ring + wave * (RQ * 64);
    const int2* const ringProd = ring + prodWave * (RQ * 64);

    int s = wave;  // the strip this wave runs, or runs next
    int yo[KR], Hp[KR], E[KR];
    int hdiag = NEG, fLast = NEGF, let = 0, xnext = 0;
    int bv[KR], bj[KR];            // EXT: the best value (as SC v) of each row of the strip, and its column
    int rv = 0, ri = 0, rj = 0;    // EXT: the lane's best over the strips it has finished
#pragma unroll
    for (int k = 0; k < KR; ++k)
    {
        yo[k] = 0;
        Hp[k] = NEG;
        E[k] = NEG;
        bv[k] = 0;
        bj[k] = 0;
    }

    for (int g = 0; g < d.T; ++g)
    {
        const int q = g - s * LAG;
        if (s < d.strips && q >= 0)
        {
            const int iT = s * TR;          // the row above the strip
            const int i0 = iT + lane * KR;  // this lane's rows: i0 + 1 ... i0 + KR
            const int o = iT + 1 + lo;      // the strip's first column
            const int tb = q * 64;
            if (q == 0)
            {
#pragma unroll
                for (int k = 0; k < KR; ++k)
                {
                    yo[k] = d.seqY[min(i0 + 1 + k, R)];
                    Hp[k] = NEG;
                    E[k] = NEG;
                    if (EXT)
                    {
                        bv[k] = 0;
                        bj[k] = 0;
                    }
                }
                // the cell above lane 0's first one, (iT, o - 1), lies on the band's lowest diagonal: the
                // producer's step 64 KR + 62.  The lanes below overwrite theirs before their first cell.
                const int jd = o - 1;
                hdiag = s == 0 ? 0 : ringProd[((g - LAG + KR) % RQ) * 64 + 62].x;
                if (jd < 0 || jd > C) hdiag = NEG;
                fLast = NEGF;
                let = 0;
                xnext = x[min(max(o + lane, 1), C)];
            }
            // the letters of this super-step's columns, and the load for the next one
            const int xblk = xnext;
            xnext = x[min(max(o + tb + 64 + lane, 1), C)];
            // the row above the strip at the column lane 0 stands on at step tb + lane
            int ah, af = NEGF;
            {
                const int j = o + tb + lane;
                if (s == 0)
                    ah = j == 0 ? 0 : gap_run(SC, go, j - 1, ge);  // row 0: E only
                else
                {
                    const int gp = g - LAG + KR + ((lane + 63) >> 6);
                    const int2 v = ringProd[(gp % RQ) * 64 + ((lane + 63) & 63)];
                    ah = v.x;
                    af = v.y;
                }
                if (j < 0 || j > C || j - iT < lo || j - iT > hi)
                {
                    ah = NEG;
                    af = NEGF;
                }
            }
            const int rowsLeft = R - i0 - 1;  // k <= rowsLeft: a row of the matrix
            unsigned char* const cw = CODES ? d.codes + (size_t)s * (size_t)d.stripBytes + lane * (KR / 2) : nullptr;

            for (int u = 0; u < 64; ++u)
            {
                const int cidx = tb + u - lane;  // the column's index in the strip
                const int j = o + cidx;
                let = from_lane_above(__builtin_amdgcn_readlane(xblk, u), let);
                const int hu0 = from_lane_above(__builtin_amdgcn_readlane(ah, u), Hp[KR - 1]);
                const int fu0 = AFFINE ? from_lane_above(__builtin_amdgcn_readlane(af, u), fLast) : 0;
                // rows k with kmin <= k <= kmax are cells of the band
                const int kmin = j - i0 - 1 - hi;
                const int kmax = (j < 0 || j > C) ? -1 : min(j - i0 - 1 - lo, rowsLeft);
                if (j == 0)
                {
                    // column 0: F only (the fill never reads F there)
#pragma unroll
                    for (int k = 0; k < KR; ++k)
                    {
                        const bool ok = k >= kmin && k <= kmax;
                        Hp[k] = ok ? gap_run(SC, go, i0 + k, ge) : NEG;
                        E[k] = NEG;
                    }
                    fLast = NEGF;
                }
                else
                {
                    const int* const trow = tab + let * ssz;
                    int hup = hu0, fup = fu0, hdg = hdiag;
                    unsigned acc = 0u;
#pragma unroll
                    for (int k = 0; k < KR; ++k)
                    {
                        const bool ok = k >= kmin && k <= kmax;
                        const int hp = Hp[k];
                        const int dg = hdg + trow[yo[k]];
                        int e, f, h;
                        unsigned nib = 0u;
                        if (AFFINE)
                        {
                            if (CODES)
                            {
                                const int eq = max(E[k] + geS, hp + (goS + 1));   // bit 0: opened
                                const int fq = max(fup + geS, hup + (goS + 2));   // bit 1: opened
                                e = eq & ~3;
                                f = (fq & ~3) | TF;
                                nib = ((unsigned)eq & 1u) | ((unsigned)fq & 2u);
                            }
                            else
                            {
                                e = max(E[k] + geS, hp + goS);
                                f = max(fup + geS, hup + goS);
                            }
                        }
                        else
                        {
                            e = hp + goS;
                            f = hup + (goS + TF);
                        }
                        h = max(max(dg, e), f);
                        if (CODES)
                        {
                            nib = (nib << 2) | ((unsigned)h & 3u);
                            acc |= nib << (4 * k);
                            h &= ~3;
                        }
                        h = ok ? h : NEG;
                        if (EXT)
                        {
                            // (a cell off the band holds NEG and never wins; with codes h is 4 v here)
                            const bool better = h > bv[k];
                            bv[k] = better ? h : bv[k];
                            bj[k] = better ? j : bj[k];
                        }
                        if (AFFINE)
                        {
                            E[k] = ok ? e : NEG;
                            fup = ok ? f : NEGF;
                        }
                        hdg = hp;
                        Hp[k] = h;
                        hup = h;
                    }
                    fLast = fup;
                    if (CODES && min(kmax, KR - 1) >= max(kmin, 0) && (unsigned)cidx < (unsigned)d.Wc)
                    {
                        const unsigned out = acc ^ (AFFINE ? 0xccccccccu : 0u);  // "opened" to "extended"
                        unsigned char* const at = cw + (size_t)cidx * (TR / 2);
                        static_assert(KR == 4, "a lane's codes of a column are one 16-bit store");
                        *reinterpret_cast<unsigned short*>(at) = (unsigned short)out;
                    }
                }
                hdiag = hu0;
                if (lane == 63) ringOwn[(g % RQ) * 64 + u] = make_int2(Hp[KR - 1], fLast);
                if (!EXT && j == C && rowsLeft >= 0 && rowsLeft < KR)
                {
                    int h = 0;
#pragma unroll
                    for (int k = 0; k < KR; ++k) h = k == rowsLeft ? Hp[k] : h;
                    d.result[0] = CODES ? h >> 2 : h;
                    d.result[1] = 1;
                }
            }
            if (EXT && q == d.nq - 1)
            {
#pragma unroll
                for (int k = 0; k < KR; ++k)
                {
                    const bool better = bv[k] > rv;
                    rv = better ? bv[k] : rv;
                    ri = better ? i0 + 1 + k : ri;
                    rj = better ? bj[k] : rj;
                }
            }
            if (q == d.nq - 1) s += nwv;
        }
        __syncthreads();
    }
    if (EXT)
    {
        // every strip is folded (the barrier above ended the last super-step): lanes, then waves
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            best_take(rv, ri, rj, __shfl_xor(rv, off, 64), __shfl_xor(ri, off, 64), __shfl_xor(rj, off, 64));
        if (lane == 0) best[wave] = make_int4(rv, ri, rj, 0);
        __syncthreads();
        if (threadIdx.x == 0)
        {
            for (int w = 1; w < nwv; ++w)
            {
                const int4 o = best[w];
                best_take(rv, ri, rj, o.x, o.y, o.z);
            }
            d.result[0] = CODES ? rv >> 2 : rv;
            d.result[2] = ri;
            d.result[3] = rj;
            d.result[1] = 1;
        }
    }
}

// One lane.  State kWalkH, or kDbTraceF / kDbTraceE inside a gap; every trip emits one move or ends
// the walk, so it takes at most R + C trips.
__device__ __forceinline__ void band_walk(const BandWalkArgs& a)
{
    const int* const x = a.seqX;
    const int* const y = a.seqY;
    unsigned char* const mv = a.moves;
    // the extension mode's walk starts on the end cell its fill found, behind it on the stream
    int i = a.start ? a.start[2] : a.R, j = a.start ? a.start[3] : a.C, n = 0;
    unsigned state = kWalkH;
    bool done = false, off = false;
    while (!done && !off)
    {
        if (j - i < a.lo || j - i > a.hi || i < 0 || j < 0)
        {
            off = true;
            break;
        }
        const bool border = i == 0 || j == 0;
        unsigned code = 0u;
        if (!border)
        {
            const int s = (i - 1) / TR, rr = (i - 1) - s * TR;
            const int l = rr / KR, k = rr - l * KR;
            const int cidx = j - (s * TR + 1 + a.lo);
            const size_t at = (size_t)s * (size_t)a.stripBytes + (size_t)cidx * (size_t)(TR / 2) + (size_t)(l * (KR / 2) + (k >> 1));
            code = ((unsigned)a.codes[at] >> (4 * (k & 1))) & 15u;
        }
        // row 0 is E only, column 0 F only
        const unsigned bsrc = i == 0 ? (j == 0 ? kDbTraceStop : kDbTraceE) : kDbTraceF;
        const unsigned src = border ? bsrc : (code & 3u);
        const unsigned eff = (state == kWalkH || border) ? src : state;
        const bool diag = eff == kDbTraceDiag, up = eff == kDbTraceF, left = eff == kDbTraceE;
        done = eff == kDbTraceStop;
        const bool ext = !border && ((up && (code & kDbTraceFExt)) || (left && (code & kDbTraceEExt)));
        const bool same = y[max(i, 1)] == x[max(j, 1)];
        const unsigned char op = diag ? (same ? '=' : 'X') : (up ? 'I' : 'D');
        if (!done) mv[n] = op;
        n += done ? 0 : 1;
        i -= (diag || up) ? 1 : 0;
        j -= (diag || left) ? 1 : 0;
        state = ext ? eff : kWalkH;
    }
    BandWalkRec o;
    o.i = i;
    o.j = j;
    o.state = state;
    o.n = n;
    o.done = done ? 1 : 0;
    o.offband = off ? 1 : 0;
    o.pad0 = o.pad1 = 0;
    *a.rec = o;
}

// The extension mode's walk (a.start is not null): a start cell outside the matrix is reported as off
// the band before any code is read; else band_walk.
__device__ __forceinline__ void band_walk_from_start(const BandWalkArgs& a)
{
    const int i = a.start[2], j = a.start[3];
    if (i < 0 || j < 0 || i > a.R || j > a.C)
    {
        BandWalkRec o;
        o.i = i;
        o.j = j;
        o.state = kWalkH;
        o.n = 0;
        o.done = 0;
        o.offband = 1;
        o.pad0 = o.pad1 = 0;
        *a.rec = o;
        return;
    }
    band_walk(a);
}

}  // namespace band_dev
}  // namespace gsa
