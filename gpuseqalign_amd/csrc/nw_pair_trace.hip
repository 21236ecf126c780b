// nw_pair_trace.hip -- the alignment of one long pair (gsa_align_pair_dev): NW / SW
// with linear or affine gaps, traced on the device from the score launch's checkpoint rows.
//
// The K-rows score kernel leaves the bottom row of every ticket but the last in its hand-off granules
// (Hgo' and, affine, F', shifted; nw_krow.hip ks_drain).  With those rows exact, the strip of rows
// t TR + 1 ... (t + 1) TR depends on its checkpoint row and on column 0 only, so all strips of a chunk
// are filled at once, each by one wave, and no wave waits for another: no hand-off, no progress
// words, no spin loops.  Lane l of a strip's wave holds the rows l KR + 1 ... (l + 1) KR of the strip
// (KR = TR / 64) and runs one column behind lane l - 1, whose last row it takes with a wave-wide
// shift by one lane (DPP wave_shr:1); lane 0 reads the checkpoint row, one column ahead, and unshifts
// it as bidi_combine_kernel does.  A strip's chain is J + 63 steps.  Lanes outside their own columns
// are masked by EXEC.  Per cell the fill forms the 4-bit code of nw_lanes_trace.hip with the same
// tagged maximum (values kept as 4 v + tag); a lane's codes of a column are KR / 2 bytes, a strip's
// column 32 KR contiguous bytes.  The substitution values come from a copy of the table in LDS
// (4 s + 2, transposed), gathered by the lane's own row letters.
//
// The walk takes one lane: a nibble load and a move per trip, across strip boundaries by address
// arithmetic, until the path's first cell or the chunk's upper boundary, where it leaves the cell and
// its state for the next chunk.
#include "nw_pair_trace.h"

#include <algorithm>

#include "nw_lanes_trace.h"
#include "nw_strip.h"

namespace gsa {

namespace {

constexpr int kNegQ = -(1 << 29);  // 4 x "minus infinity" (-2^27), tag 0
constexpr unsigned kWalkH = 4u;    // the walk's state H; inside a gap the state is the gap's source code
constexpr int kFillWgsPerCu = 8;

__device__ __forceinline__ int from_lane_above(int own, int src)
{
    // wave_shr:1 over the 64 lanes; lane 0 has no source and keeps `own`
    return __builtin_amdgcn_update_dpp(own, src, 0x138, 0xf, 0xf, false);
}

template <int N>
struct __attribute__((aligned(4 * N))) CodesN
{
    unsigned w[N];
};

// The checkpoint row above strip s at column j, as 4 H (tag 0) and 4 F | F's tag: the low 32 bits of
// the granule, signed, H = Hgo' - (go - ge) + (i + j) ge, F = F' + (i + j) ge.  Local: the score
// kernel's F' has the zero floor folded in, so F here is max(F, 0); a walk is in state F only at
// cells with F = H > 0, and the floor adds at most 0 + ge <= 0 to the row below, never the winner.
template <bool AFFINE>
__device__ __forceinline__ int2 checkpoint(const unsigned long long* gh, const unsigned long long* gf, int j, int iT,
                                           int go, int ge)
{
    const int sh = (iT + j) * ge;
    const int h = (int)(unsigned)gh[j] - (go - ge) + sh;
    int2 r;
    r.x = 4 * h;
    r.y = AFFINE ? ((4 * ((int)(unsigned)gf[j] + sh)) | (int)kDbTraceF) : 0;
    return r;
}

template <bool LOCAL, bool AFFINE, int KR>
__global__ __launch_bounds__(64) void nw_pair_fill_kernel(PairFillArgs a)
{
    constexpr int TR = 64 * KR;
    constexpr int NW = KR / 8;  // dwords of codes per lane and column
    __shared__ int tab[32 * 32];
    const int ssz = a.substsz;
    // tab[x letter][y letter] = 4 s(y, x) + tag "diagonal"
    for (int idx = threadIdx.x; idx < ssz * ssz; idx += 64)
    {
        const int xl = idx / ssz, yl = idx - xl * ssz;
        tab[idx] = 4 * a.subst[yl * ssz + xl] + (int)kDbTraceDiag;
    }
    __syncthreads();

    const int lane = threadIdx.x;
    const int go = a.go, ge = a.ge;
    const int go4 = 4 * go, ge4 = 4 * ge;
    const int* const x = a.seqX;

    for (;;)
    {
        unsigned t = 0;
        if (lane == 0) t = atomicAdd(a.counter, 1u);
        t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= (unsigned)a.nstrips) break;
        const int s = a.tLo + (int)t;
        const int iT = s * TR;           // the checkpoint row (0: the border)
        const int i0 = iT + lane * KR;   // this lane's rows: i0 + 1 ... i0 + KR
        const int J = i0 < a.iEnd ? a.J : 0;  // lanes wholly below iEnd have no cells
        const bool ck = s > 0 && lane == 0;
        const unsigned long long* const gh = a.gran + (size_t)(s > 0 ? s - 1 : 0) * (size_t)a.granStride;
        const unsigned long long* const gf = a.gran2 + (size_t)(s > 0 ? s - 1 : 0) * (size_t)a.granStride;
        // this lane's codes of column j: cw + (j - 1) TR / 2
        unsigned char* const cw = a.codes + (size_t)t * (size_t)a.stripBytes + lane * (KR / 2);

        int yo[KR], Hp[KR], E[KR];  // the rows' letters, 4 H (tag 0), 4 E (tag 0)
#pragma unroll
        for (int k = 0; k < KR; ++k)
        {
            yo[k] = a.seqY[min(i0 + 1 + k, a.R)];
            Hp[k] = LOCAL ? 0 : go4 + (i0 + k) * ge4;  // column 0
            E[k] = kNegQ;
        }
        int hdiag = (LOCAL || i0 == 0) ? 0 : go4 + (i0 - 1) * ge4;  // H(i0, 0)
        int fLast = kNegQ | (int)kDbTraceF;
        // the letter and the row above of the next step, loaded one step ahead
        int letNext = (1 - lane >= 1 && 1 - lane <= J) ? x[1 - lane] : 0;
        int2 aboveNext = make_int2(0, kNegQ | (int)kDbTraceF);
        if (ck && J >= 1) aboveNext = checkpoint<AFFINE>(gh, gf, 1, iT, go, ge);

        for (int step = 1; step <= a.J + 63; ++step)
        {
            const int j = step - lane;
            const int let = letNext;
            int2 above = aboveNext;
            if (j + 1 >= 1 && j + 1 <= J)
            {
                letNext = x[j + 1];
                if (ck) aboveNext = checkpoint<AFFINE>(gh, gf, j + 1, iT, go, ge);
            }
            if (s == 0)
            {
                above.x = LOCAL ? 0 : go4 + (j - 1) * ge4;  // the border row: E only
                above.y = kNegQ | (int)kDbTraceF;
            }
            const int hu0 = from_lane_above(above.x, Hp[KR - 1]);
            const int fu0 = AFFINE ? from_lane_above(above.y, fLast) : 0;
            if (j >= 1 && j <= J)
            {
                const int* const trow = tab + let * ssz;
                int hup = hu0, fup = fu0, hdg = hdiag;
                unsigned acc[NW];
#pragma unroll
                for (int w = 0; w < NW; ++w) acc[w] = 0u;
#pragma unroll
                for (int k = 0; k < KR; ++k)
                {
                    const int hp = Hp[k];
                    const int d = hdg + trow[yo[k]];  // tag 2
                    int e, f, h;
                    unsigned nib;
                    if (AFFINE)
                    {
                        const int eq = max(E[k] + ge4, hp + (go4 + 1));  // bit 0: opened
                        const int fq = max(fup + ge4, hup + (go4 + 2));  // bit 1: opened
                        e = eq & ~3;                                     // tag 0
                        f = (fq & ~3) | (int)kDbTraceF;                  // tag 1
                        nib = ((unsigned)eq & 1u) | ((unsigned)fq & 2u);
                        E[k] = e;
                        fup = f;
                    }
                    else
                    {
                        e = hp + go4;
                        f = hup + (go4 + (int)kDbTraceF);
                        nib = 0u;
                    }
                    h = max(max(d, e), f);
                    if (LOCAL) h = max(h, (int)kDbTraceStop);
                    nib = (nib << 2) | ((unsigned)h & 3u);
                    acc[k / 8] |= nib << (4 * (k % 8));
                    h &= ~3;
                    hdg = hp;
                    Hp[k] = h;
                    hup = h;
                }
                fLast = fup;
                hdiag = hu0;
                // "opened" to "extended"
                const unsigned flip = AFFINE ? 0xccccccccu : 0u;
                CodesN<NW> out;
#pragma unroll
                for (int w = 0; w < NW; ++w) out.w[w] = acc[w] ^ flip;
                *reinterpret_cast<CodesN<NW>*>(cw + (size_t)(j - 1) * (TR / 2)) = out;
            }
        }
    }
}

// One lane.  State kWalkH, or kDbTraceF / kDbTraceE inside a gap; every trip of the loop emits one
// move or ends the walk, so the walk takes at most i_end + j_end trips over all chunks.
__global__ __launch_bounds__(64) void nw_pair_walk_kernel(PairWalkArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const PairWalkRec r = *a.rec;
    const int* const x = a.seqX;
    const int* const y = a.seqY;
    unsigned char* const mv = a.moves;
    const bool local = a.local != 0;
    const int ks = a.krShift, KR = 1 << ks, TRm = (64 << ks) - 1;
    int i = r.i, j = r.j, n = r.n;
    unsigned state = r.state;
    bool done = r.done != 0;
    while (!done && !(a.iStop > 0 && i == a.iStop && j > 0))
    {
        const bool border = i == 0 || j == 0;
        unsigned code = 0u;
        if (!border)
        {
            const int rr = (i - 1) & TRm, t = ((i - 1) >> (6 + ks)) - a.tLo;
            const int l = rr >> ks, k = rr & (KR - 1);
            const size_t at = (size_t)t * (size_t)a.stripBytes + (size_t)(j - 1) * (size_t)(32 << ks) +
                              (size_t)(l * (KR / 2) + (k >> 3) * 4);
            code = (*reinterpret_cast<const unsigned*>(a.codes + at) >> (4 * (k & 7))) & 15u;
        }
        // on the border: local H is 0 there (stop); global row 0 is E only, column 0 F only
        const unsigned bsrc = local ? kDbTraceStop : (i == 0 ? (j == 0 ? kDbTraceStop : kDbTraceE) : kDbTraceF);
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
    PairWalkRec o;
    o.i = i;
    o.j = j;
    o.state = state;
    o.n = n;
    o.done = done ? 1 : 0;
    o.pad0 = o.pad1 = o.pad2 = 0;
    *a.rec = o;
}

template <bool LOCAL, bool AFFINE, int KR>
hipError_t fill_grid(int nstrips, int* grid)
{
    auto kern = nw_pair_fill_kernel<LOCAL, AFFINE, KR>;
    int per_cu = 0, dev = 0, cus = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64, 0);
    if (e == hipSuccess) e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) *grid = std::max(1, std::min(nstrips, std::min(std::max(1, per_cu), kFillWgsPerCu) * std::max(1, cus)));
    return e;
}

template <bool LOCAL, bool AFFINE, int KR>
hipError_t launch_fill(const PairFillArgs& a, int grid, hipStream_t st)
{
    auto kern = nw_pair_fill_kernel<LOCAL, AFFINE, KR>;
    hipError_t e = record_foot((const void*)kern, 0, 64, grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64), 0, st, a);
    return hipGetLastError();
}

template <int KR>
hipError_t fill_grid_kr(int local, bool affine, int nstrips, int* grid)
{
    if (local) return affine ? fill_grid<true, true, KR>(nstrips, grid) : fill_grid<true, false, KR>(nstrips, grid);
    return affine ? fill_grid<false, true, KR>(nstrips, grid) : fill_grid<false, false, KR>(nstrips, grid);
}

template <int KR>
hipError_t launch_fill_kr(const PairFillArgs& a, int grid, hipStream_t st)
{
    const bool affine = a.go != a.ge;
    if (a.local) return affine ? launch_fill<true, true, KR>(a, grid, st) : launch_fill<true, false, KR>(a, grid, st);
    return affine ? launch_fill<false, true, KR>(a, grid, st) : launch_fill<false, false, KR>(a, grid, st);
}

hipError_t launch_pair_walk(const PairWalkArgs& w, hipStream_t st)
{
    hipLaunchKernelGGL(nw_pair_walk_kernel, dim3(1), dim3(64), 0, st, w);
    return hipGetLastError();
}

}  // namespace

hipError_t pair_fill_grid(int local, bool affine, int KR, int nstrips, int* grid)
{
    if (KR != 8 && KR != 16) return hipErrorInvalidValue;
    return KR == 8 ? fill_grid_kr<8>(local, affine, nstrips, grid) : fill_grid_kr<16>(local, affine, nstrips, grid);
}

hipError_t launch_pair_trace(const PairFillArgs& f, const PairWalkArgs& w, int KR, int grid, hipEvent_t* ev, hipStream_t st)
{
    if (KR != 8 && KR != 16) return hipErrorInvalidValue;
    if (ev) (void)hipEventRecord(ev[0], st);
    hipError_t e = KR == 8 ? launch_fill_kr<8>(f, grid, st) : launch_fill_kr<16>(f, grid, st);
    if (e != hipSuccess) return e;
    if (ev) (void)hipEventRecord(ev[1], st);
    e = launch_pair_walk(w, st);
    if (ev) (void)hipEventRecord(ev[2], st);
    return e;
}

}  // namespace gsa
