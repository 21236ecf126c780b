// nw_band.hip -- the banded alignment of one long pair (gsa_score_band_dev, gsa_align_pair_band_dev;
// DESIGN.md 2.2p): global alignment with linear or affine gaps inside the diagonals lo <= j - i <= hi.
//
// One workgroup of up to 16 waves takes a pair.  Strip s (rows s TR + 1 ... (s + 1) TR) runs on wave
// s mod NWV; lane l holds KR = 4 rows and runs one column behind lane l - 1, whose last row it takes
// with a wave-wide shift by one lane (DPP wave_shr:1), as nw_pair_trace.hip does.  The strip's columns
// start at o(s) = s TR + 1 + lo, so a strip sweeps W + TR - 1 columns and never the whole row.  Cells
// off the band, left of column 1, right of column C or below row R are kept at minus infinity; column
// 0 and row 0 take their border values where the band holds them.
//
// The waves run in lockstep super-steps of 64 column steps with one __syncthreads() between them
// (nw_band_plan.h): strip s starts at super-step s lag, which puts the row it needs from strip s - 1
// into strictly earlier super-steps.  That row goes through a ring in LDS per wave, written by lane
// 63 and read by the consumer's lanes once per super-step, 64 columns at a time; within the super-step
// the values and the 64 subject letters (loaded a super-step ahead) come out of registers by
// v_readlane.  No wave polls anything: every loop is bounded by T, 64 and KR.
//
// With CODES the cells are kept as 4 v + tag and the fill stores nw_lanes_trace.h's 4-bit codes in
// this one pass, strip-major; without, plain int32 values and nothing but H(R, C) is stored.  The
// walk is nw_pair_trace.hip's one-lane loop with the strip's own column origin.
#include "nw_band.h"

#include "nw_lanes_trace.h"
#include "nw_strip.h"

namespace gsa {

namespace {

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

template <bool AFFINE, bool CODES>
__global__ __launch_bounds__(64 * kBandWaves) void nw_band_kernel(const BandDesc* descs, const int* subst, int ssz, int go,
                                                                   int ge)
{
    constexpr int SC = CODES ? 4 : 1;             // values are kept as SC v (+ tag)
    constexpr int NEG = -(1 << 29);               // minus infinity: SC x -2^27 with codes, -2^29 without
    constexpr int TF = CODES ? (int)kDbTraceF : 0;
    constexpr int NEGF = NEG | TF;
    __shared__ int tab[32 * 32];
    __shared__ int2 ring[kBandWaves][RQ][64];
    // tab[x letter][y letter] = SC s(y, x) + tag "diagonal"
    for (int idx = threadIdx.x; idx < ssz * ssz; idx += blockDim.x)
    {
        const int xl = idx / ssz, yl = idx - xl * ssz;
        tab[idx] = SC * subst[yl * ssz + xl] + (CODES ? (int)kDbTraceDiag : 0);
    }
    __syncthreads();

    const BandDesc d = descs[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    const int goS = SC * go, geS = SC * ge;
    const int R = d.R, C = d.C, lo = d.lo, hi = d.hi;
    const int* const x = d.seqX;
    const int prodWave = (wave + nwv - 1) % nwv;

    int s = wave;  // the strip this wave runs, or runs next
    int yo[KR], Hp[KR], E[KR];
    int hdiag = NEG, fLast = NEGF, let = 0, xnext = 0;
#pragma unroll
    for (int k = 0; k < KR; ++k)
    {
        yo[k] = 0;
        Hp[k] = NEG;
        E[k] = NEG;
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
                }
                // the cell above lane 0's first one, (iT, o - 1), lies on the band's lowest diagonal: the
                // producer's step 64 KR + 62.  The lanes below overwrite theirs before their first cell.
                const int jd = o - 1;
                hdiag = s == 0 ? 0 : ring[prodWave][(g - LAG + KR) % RQ][62].x;
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
                    const int2 v = ring[prodWave][gp % RQ][(lane + 63) & 63];
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
                if (lane == 63) ring[wave][g % RQ][u] = make_int2(Hp[KR - 1], fLast);
                if (j == C && rowsLeft >= 0 && rowsLeft < KR)
                {
                    int h = 0;
#pragma unroll
                    for (int k = 0; k < KR; ++k) h = k == rowsLeft ? Hp[k] : h;
                    d.result[0] = CODES ? h >> 2 : h;
                    d.result[1] = 1;
                }
            }
            if (q == d.nq - 1) s += nwv;
        }
        __syncthreads();
    }
}

// One lane.  State kWalkH, or kDbTraceF / kDbTraceE inside a gap; every trip emits one move or ends
// the walk, so it takes at most R + C trips.
__global__ __launch_bounds__(64) void nw_band_walk_kernel(BandWalkArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int* const x = a.seqX;
    const int* const y = a.seqY;
    unsigned char* const mv = a.moves;
    int i = a.R, j = a.C, n = 0;
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

template <bool AFFINE, bool CODES>
hipError_t launch_fill(const BandDesc* descs, int npairs, int waves, const int* subst, int substsz, int go, int ge,
                       hipStream_t st)
{
    auto kern = nw_band_kernel<AFFINE, CODES>;
    hipError_t e = record_foot((const void*)kern, 0, 64 * waves, npairs);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(npairs), dim3(64 * waves), 0, st, descs, subst, substsz, go, ge);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_band(const BandDesc* descs, int npairs, int waves, const int* subst, int substsz, int go, int ge,
                       bool codes, const BandWalkArgs* w, hipEvent_t* ev, hipStream_t st)
{
    if (npairs < 1 || waves < 1 || waves > kBandWaves) return hipErrorInvalidValue;
    const bool affine = go != ge;
    if (ev) (void)hipEventRecord(ev[0], st);
    hipError_t e = codes ? (affine ? launch_fill<true, true>(descs, npairs, waves, subst, substsz, go, ge, st)
                                   : launch_fill<false, true>(descs, npairs, waves, subst, substsz, go, ge, st))
                         : (affine ? launch_fill<true, false>(descs, npairs, waves, subst, substsz, go, ge, st)
                                   : launch_fill<false, false>(descs, npairs, waves, subst, substsz, go, ge, st));
    if (e != hipSuccess) return e;
    if (ev) (void)hipEventRecord(ev[1], st);
    if (w)
    {
        hipLaunchKernelGGL(nw_band_walk_kernel, dim3(1), dim3(64), 0, st, *w);
        e = hipGetLastError();
    }
    if (ev) (void)hipEventRecord(ev[2], st);
    return e;
}

}  // namespace gsa
