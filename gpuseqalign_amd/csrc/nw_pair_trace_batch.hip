// nw_pair_trace_batch.hip -- the alignments of a batch of long pairs (gsa_align_batch_dev; DESIGN.md
// 2.2j): the strips of many pairs in one task space, and the pairs' walks side by side.
//
// The batched K-rows score launch leaves the bottom row of every ticket but the last of every pair in
// the pair's own hand-off granules (PairDesc::granOff), so a round's strips, whatever pair they belong
// to, are tasks of one launch: a task table (pair, strip, code offset), sorted by column count
// descending so that the longest chains start first, one atomic counter, one wave per task.  No wave
// waits for another; every loop is bounded by J + 63 or by the task count.  A fill task is a ticket t of
// the counter: tasks[t] names the pair's descriptor, the strip and the codes' offset.  The strip fill is
// nw_pair_trace_dev.h's with the border kGlobal or kLocal, as in nw_pair_trace.hip; one workgroup may run
// strips of different pairs back to back.
//
// The walks take one wave per pair (lane 0 walks), grid-strided when the grid is capped: GSA_PAIR_WALK on
// that pair's record, codes and moves.
#include "nw_pair_trace_batch.h"

#include "nw_pair_trace_dev.h"

namespace gsa {

namespace {

using namespace pair_dev;

template <bool LOCAL, bool AFFINE, int KR>
__global__ __launch_bounds__(64) void nw_pair_batch_fill_kernel(PairBatchFillArgs a)
{
    __shared__ int tab[32 * 32];
    const int ssz = a.substsz;
    load_tab(tab, a.subst, ssz);
    __syncthreads();

    const int lane = threadIdx.x;
    for (;;)
    {
        unsigned t = 0;
        if (lane == 0) t = atomicAdd(a.counter, 1u);
        t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= (unsigned)a.ntasks) break;
        const PairBatchTask bt = a.tasks[t];
        const PairBatchDesc P = a.pairs[bt.pair];
        const int s = bt.strip;
        const size_t grow = (size_t)P.granBase + (size_t)(s > 0 ? s - 1 : 0) * (size_t)P.granStride;
        StripTask task;
        task.s = s;
        task.seqY = P.seqY;
        task.x = P.seqX;
        task.clampRow = P.R;
        task.lastRow = P.iEnd;
        task.W = P.J;
        task.jW = 0;
        task.gh = a.gran + grow;
        task.gf = a.gran2 + grow;
        task.cw = a.codes + (size_t)bt.codeOff;
        GSA_PAIR_STRIP_FILL((LOCAL ? kLocal : kGlobal), AFFINE, KR, task, tab, ssz, a.go, a.ge);
    }
}

__global__ __launch_bounds__(64) void nw_pair_batch_walk_kernel(PairBatchWalkArgs a)
{
    if (threadIdx.x != 0) return;
    const bool local = a.local != 0;
    for (int q = blockIdx.x; q < a.nwalks; q += gridDim.x)
    {
        const PairBatchWalk W = a.walks[q];
        const WalkTask w = {W.seqY, W.seqX, W.codes, W.stripBytes, a.krShift, W.tLo, W.iStop, 0, W.moves};
        GSA_PAIR_WALK(w, local, a.recs[W.rec]);
    }
}

template <int KR>
hipError_t fill_grid_kr(int local, bool affine, int ntasks, int maxWgs, int* grid)
{
    if (local)
        return affine ? fill_grid_for(nw_pair_batch_fill_kernel<true, true, KR>, ntasks, maxWgs, grid)
                      : fill_grid_for(nw_pair_batch_fill_kernel<true, false, KR>, ntasks, maxWgs, grid);
    return affine ? fill_grid_for(nw_pair_batch_fill_kernel<false, true, KR>, ntasks, maxWgs, grid)
                  : fill_grid_for(nw_pair_batch_fill_kernel<false, false, KR>, ntasks, maxWgs, grid);
}

template <int KR>
hipError_t launch_fill_kr(const PairBatchFillArgs& a, int local, int grid, hipStream_t st)
{
    const bool affine = a.go != a.ge;
    if (local)
        return affine ? launch_fill_for(nw_pair_batch_fill_kernel<true, true, KR>, a, grid, st)
                      : launch_fill_for(nw_pair_batch_fill_kernel<true, false, KR>, a, grid, st);
    return affine ? launch_fill_for(nw_pair_batch_fill_kernel<false, true, KR>, a, grid, st)
                  : launch_fill_for(nw_pair_batch_fill_kernel<false, false, KR>, a, grid, st);
}

}  // namespace

hipError_t pair_batch_fill_grid(int local, bool affine, int KR, int ntasks, int maxWgs, int* grid)
{
    if (KR != 8 && KR != 16) return hipErrorInvalidValue;
    return KR == 8 ? fill_grid_kr<8>(local, affine, ntasks, maxWgs, grid) : fill_grid_kr<16>(local, affine, ntasks, maxWgs, grid);
}

hipError_t launch_pair_batch_trace(const PairBatchFillArgs& f, int local, const PairBatchWalkArgs& w, int KR, int grid,
                                   int walkGrid, hipEvent_t* ev, hipStream_t st)
{
    if (KR != 8 && KR != 16) return hipErrorInvalidValue;
    if (grid < 1 || walkGrid < 1 || f.ntasks < 1 || w.nwalks < 1) return hipErrorInvalidValue;
    if (ev) (void)hipEventRecord(ev[0], st);
    hipError_t e = KR == 8 ? launch_fill_kr<8>(f, local, grid, st) : launch_fill_kr<16>(f, local, grid, st);
    if (e != hipSuccess) return e;
    if (ev) (void)hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(nw_pair_batch_walk_kernel, dim3(walkGrid), dim3(64), 0, st, w);
    e = hipGetLastError();
    if (ev) (void)hipEventRecord(ev[2], st);
    return e;
}

}  // namespace gsa
