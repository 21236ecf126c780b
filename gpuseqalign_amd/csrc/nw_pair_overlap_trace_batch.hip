// nw_pair_overlap_trace_batch.hip -- the overlap (dovetail) alignments of a batch of long pairs
// (gsa_align_batch_overlap_dev): the strip fill of nw_pair_overlap_trace.hip over the
// strips of many pairs in one task space, and the pairs' walks side by side.
//
// The batched overlap score launch leaves the bottom row of every ticket but the last of every pair in
// the pair's own hand-off granules (PairDesc::granOff).  With those rows exact every strip of every pair
// depends on its checkpoint row and on the free column 0 only, so a round's strips, whatever pair they
// belong to, are tasks of one launch: a task table (pair, strip, code offset), sorted by column count
// descending so that the longest chains start first, one atomic counter, one wave per task.  No wave
// waits for another: no hand-off, no progress words, no spin loops; every loop is bounded by the width
// + 63 or by the task count.  The per-strip body is nw_overlap_fill_kernel's, kept here as a copy of its
// own so that that unit's kernels stay as they are -- the free row above strip 0 (H = 0, F = minus
// infinity), column 0 H = 0 and E = minus infinity in every row, set from the definition, only the rows
// up to the pair's end row filled -- with the pair's values read from a descriptor table per task, and
// every piece of per-task state set anew per task: one workgroup may run strips of different pairs back
// to back.
//
// The walks take one wave per pair (lane 0 walks), grid-strided when the grid is capped; the loop is
// nw_overlap_walk_kernel's on that pair's record, codes and moves: it stops on row 0, on column 0, or on
// its chunk's upper boundary.
#include "nw_pair_overlap_trace_batch.h"

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

// The checkpoint row above strip s at column j, as 4 H (tag 0) and 4 F | F's tag (nw_pair_overlap_trace.hip)
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

template <bool AFFINE, int KR>
__global__ __launch_bounds__(64) void nw_overlap_batch_fill_kernel(OverlapBatchFillArgs a)
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

    for (;;)
    {
        unsigned t = 0;
        if (lane == 0) t = atomicAdd(a.counter, 1u);
        t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= (unsigned)a.ntasks) break;
        const PairBatchTask task = a.tasks[t];
        const PairBatchDesc P = a.pairs[task.pair];
        const int W = P.J;  // the columns 1 ... W
        const int* const x = P.seqX;
        const int s = task.strip;
        const int iT = s * TR;              // the checkpoint row (0: the free row)
        const int i0 = iT + lane * KR;      // this lane's rows: i0 + 1 ... i0 + KR
        const int J = i0 < P.iEnd ? W : 0;  // lanes wholly below i_end have no cells
        const bool ck = s > 0 && lane == 0;
        const size_t grow = (size_t)P.granBase + (size_t)(s > 0 ? s - 1 : 0) * (size_t)P.granStride;
        const unsigned long long* const gh = a.gran + grow;
        const unsigned long long* const gf = a.gran2 + grow;
        // this lane's codes of column c: cw + (c - 1) TR / 2
        unsigned char* const cw = a.codes + (size_t)task.codeOff + lane * (KR / 2);

        int yo[KR], Hp[KR], E[KR];  // the rows' letters, 4 H (tag 0), 4 E (tag 0)
#pragma unroll
        for (int k = 0; k < KR; ++k)
        {
            yo[k] = P.seqY[min(i0 + 1 + k, P.iEnd)];
            Hp[k] = 0;  // the free column 0: H = 0, no gap runs along it
            E[k] = kNegQ;
        }
        int hdiag = 0;  // H(i0, 0)
        int fLast = kNegQ | (int)kDbTraceF;
        // the letter and the row above of the next step, loaded one step ahead
        int letNext = (1 - lane >= 1 && 1 - lane <= J) ? x[1 - lane] : 0;
        int2 aboveNext = make_int2(0, kNegQ | (int)kDbTraceF);
        if (ck && J >= 1) aboveNext = checkpoint<AFFINE>(gh, gf, 1, iT, go, ge);

        for (int step = 1; step <= W + 63; ++step)
        {
            const int c = step - lane;
            const int let = letNext;
            int2 above = aboveNext;
            if (c + 1 >= 1 && c + 1 <= J)
            {
                letNext = x[c + 1];
                if (ck) aboveNext = checkpoint<AFFINE>(gh, gf, c + 1, iT, go, ge);
            }
            if (s == 0)
            {
                above.x = 0;  // the free row: H = 0, no gap runs along it
                above.y = kNegQ | (int)kDbTraceF;
            }
            const int hu0 = from_lane_above(above.x, Hp[KR - 1]);
            const int fu0 = AFFINE ? from_lane_above(above.y, fLast) : 0;
            if (c >= 1 && c <= J)
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
                *reinterpret_cast<CodesN<NW>*>(cw + (size_t)(c - 1) * (TR / 2)) = out;
            }
        }
    }
}

// One wave per pair, lane 0 walks: nw_overlap_walk_kernel's loop on the pair's record, codes and moves.
// Every trip of the loop emits one move or ends the walk.
__global__ __launch_bounds__(64) void nw_overlap_batch_walk_kernel(OverlapBatchWalkArgs a)
{
    if (threadIdx.x != 0) return;
    const int ks = a.krShift, KR = 1 << ks, TRm = (64 << ks) - 1;
    for (int q = blockIdx.x; q < a.nwalks; q += gridDim.x)
    {
        const OverlapBatchWalk W = a.walks[q];
        const OverlapWalkRec r = a.recs[W.rec];
        const int* const x = W.seqX;
        const int* const y = W.seqY;
        unsigned char* const mv = W.moves;
        int i = r.i, j = r.j, n = r.n;
        unsigned state = r.state;
        bool done = r.done != 0;
        while (!done && !(W.iStop > 0 && i == W.iStop && j > 0))
        {
            if (i == 0 || j == 0)
            {
                done = true;  // on a free border: the overhang stays out of the alignment
                break;
            }
            const int rr = (i - 1) & TRm, t = ((i - 1) >> (6 + ks)) - W.tLo;
            const int l = rr >> ks, k = rr & (KR - 1);
            const size_t at = (size_t)t * (size_t)W.stripBytes + (size_t)(j - 1) * (size_t)(32 << ks) +
                              (size_t)(l * (KR / 2) + (k >> 3) * 4);
            const unsigned code = (*reinterpret_cast<const unsigned*>(W.codes + at) >> (4 * (k & 7))) & 15u;
            const unsigned src = code & 3u;
            const unsigned eff = state == kWalkH ? src : state;
            const bool diag = eff == kDbTraceDiag, up = eff == kDbTraceF, left_ = eff == kDbTraceE;
            const bool ext = (up && (code & kDbTraceFExt)) || (left_ && (code & kDbTraceEExt));
            const bool same = y[i] == x[j];
            mv[n] = diag ? (same ? '=' : 'X') : (up ? 'I' : 'D');
            n += 1;
            i -= (diag || up) ? 1 : 0;
            j -= (diag || left_) ? 1 : 0;
            state = ext ? eff : kWalkH;
        }
        if (i == 0 || j == 0) done = true;
        OverlapWalkRec o;
        o.i = i;
        o.j = j;
        o.state = state;
        o.n = n;
        o.done = done ? 1 : 0;
        o.pad0 = o.pad1 = o.pad2 = 0;
        a.recs[W.rec] = o;
    }
}

template <bool AFFINE, int KR>
hipError_t fill_grid(int ntasks, int maxWgs, int* grid)
{
    auto kern = nw_overlap_batch_fill_kernel<AFFINE, KR>;
    int per_cu = 0, dev = 0, cus = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64, 0);
    if (e == hipSuccess) e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    int g = std::max(1, std::min(ntasks, std::min(std::max(1, per_cu), kFillWgsPerCu) * std::max(1, cus)));
    if (maxWgs > 0) g = std::min(g, maxWgs);
    *grid = g;
    return hipSuccess;
}

template <bool AFFINE, int KR>
hipError_t launch_fill(const OverlapBatchFillArgs& a, int grid, hipStream_t st)
{
    auto kern = nw_overlap_batch_fill_kernel<AFFINE, KR>;
    hipError_t e = record_foot((const void*)kern, 0, 64, grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64), 0, st, a);
    return hipGetLastError();
}

template <int KR>
hipError_t launch_fill_kr(const OverlapBatchFillArgs& a, int grid, hipStream_t st)
{
    return a.go != a.ge ? launch_fill<true, KR>(a, grid, st) : launch_fill<false, KR>(a, grid, st);
}

}  // namespace

hipError_t overlap_batch_fill_grid(bool affine, int KR, int ntasks, int maxWgs, int* grid)
{
    if (KR != 8 && KR != 16) return hipErrorInvalidValue;
    if (KR == 8) return affine ? fill_grid<true, 8>(ntasks, maxWgs, grid) : fill_grid<false, 8>(ntasks, maxWgs, grid);
    return affine ? fill_grid<true, 16>(ntasks, maxWgs, grid) : fill_grid<false, 16>(ntasks, maxWgs, grid);
}

hipError_t launch_overlap_batch_trace(const OverlapBatchFillArgs& f, const OverlapBatchWalkArgs& w, int KR, int grid,
                                      int walkGrid, hipEvent_t* ev, hipStream_t st)
{
    if (KR != 8 && KR != 16) return hipErrorInvalidValue;
    if (grid < 1 || walkGrid < 1 || f.ntasks < 1 || w.nwalks < 1) return hipErrorInvalidValue;
    if (ev) (void)hipEventRecord(ev[0], st);
    hipError_t e = KR == 8 ? launch_fill_kr<8>(f, grid, st) : launch_fill_kr<16>(f, grid, st);
    if (e != hipSuccess) return e;
    if (ev) (void)hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(nw_overlap_batch_walk_kernel, dim3(walkGrid), dim3(64), 0, st, w);
    e = hipGetLastError();
    if (ev) (void)hipEventRecord(ev[2], st);
    return e;
}

}  // namespace gsa
