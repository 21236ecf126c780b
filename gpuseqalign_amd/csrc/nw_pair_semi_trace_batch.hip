// nw_pair_semi_trace_batch.hip -- the semi-global alignments of a batch of long pairs
// (gsa_align_batch_semi_dev): the strips of many pairs in one task space, and the pairs'
// walks side by side.
//
// The batched semi-global score launch leaves the bottom row of every ticket but the last of every
// pair in the pair's own hand-off granules (PairDesc::granOff), so a round's strips, whatever pair they
// belong to, are tasks of one launch: a task table (pair, strip, code offset), sorted by window width
// descending so that the longest chains start first, one atomic counter, one wave per task.  No wave
// waits for another; every loop is bounded by the width + 63 or by the task count.  A fill task is a
// ticket t of the counter: tasks[t] names the pair's descriptor (with its window's jW), the strip and the
// codes' offset.  The strip fill is nw_pair_trace_dev.h's with the border kSemi, letters, checkpoint rows
// and codes addressed from jW, as in nw_pair_semi_trace.hip; one workgroup may run strips of different
// pairs back to back.
//
// The walks take one wave per pair (lane 0 walks), grid-strided when the grid is capped: GSA_SEMI_WALK on
// that pair's record, codes and moves.
#include "nw_pair_semi_trace_batch.h"

#include "nw_pair_trace_dev.h"

namespace gsa {

namespace {

using namespace pair_dev;

template <bool AFFINE, int KR>
__global__ __launch_bounds__(64) void nw_semi_batch_fill_kernel(SemiBatchFillArgs a)
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
        const SemiBatchDesc D = a.pairs[bt.pair];
        const PairBatchDesc& P = D.p;
        const int s = bt.strip, jW = D.jW;
        const size_t grow = (size_t)P.granBase + (size_t)(s > 0 ? s - 1 : 0) * (size_t)P.granStride + (size_t)jW;
        StripTask task;
        task.s = s;
        task.seqY = P.seqY;
        task.x = P.seqX + jW;
        task.clampRow = P.R;
        task.lastRow = P.R;
        task.W = P.J - jW;
        task.jW = jW;
        task.gh = a.gran + grow;
        task.gf = a.gran2 + grow;
        task.cw = a.codes + (size_t)bt.codeOff;
        GSA_PAIR_STRIP_FILL((kSemi), AFFINE, KR, task, tab, ssz, a.go, a.ge);
    }
}

__global__ __launch_bounds__(64) void nw_semi_batch_walk_kernel(SemiBatchWalkArgs a)
{
    if (threadIdx.x != 0) return;
    for (int q = blockIdx.x; q < a.nwalks; q += gridDim.x)
    {
        const SemiBatchWalk W = a.walks[q];
        const WalkTask w = {W.seqY, W.seqX, W.codes, W.stripBytes, a.krShift, W.tLo, W.iStop, W.jW, W.moves};
        GSA_SEMI_WALK(w, a.recs[W.rec]);
    }
}

template <int KR>
hipError_t launch_fill_kr(const SemiBatchFillArgs& a, int grid, hipStream_t st)
{
    return a.go != a.ge ? launch_fill_for(nw_semi_batch_fill_kernel<true, KR>, a, grid, st)
                        : launch_fill_for(nw_semi_batch_fill_kernel<false, KR>, a, grid, st);
}

}  // namespace

hipError_t semi_batch_fill_grid(bool affine, int KR, int ntasks, int maxWgs, int* grid)
{
    if (KR != 8 && KR != 16) return hipErrorInvalidValue;
    if (KR == 8)
        return affine ? fill_grid_for(nw_semi_batch_fill_kernel<true, 8>, ntasks, maxWgs, grid)
                      : fill_grid_for(nw_semi_batch_fill_kernel<false, 8>, ntasks, maxWgs, grid);
    return affine ? fill_grid_for(nw_semi_batch_fill_kernel<true, 16>, ntasks, maxWgs, grid)
                  : fill_grid_for(nw_semi_batch_fill_kernel<false, 16>, ntasks, maxWgs, grid);
}

hipError_t launch_semi_batch_trace(const SemiBatchFillArgs& f, const SemiBatchWalkArgs& w, int KR, int grid, int walkGrid,
                                   hipEvent_t* ev, hipStream_t st)
{
    if (KR != 8 && KR != 16) return hipErrorInvalidValue;
    if (grid < 1 || walkGrid < 1 || f.ntasks < 1 || w.nwalks < 1) return hipErrorInvalidValue;
    if (ev) (void)hipEventRecord(ev[0], st);
    hipError_t e = KR == 8 ? launch_fill_kr<8>(f, grid, st) : launch_fill_kr<16>(f, grid, st);
    if (e != hipSuccess) return e;
    if (ev) (void)hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(nw_semi_batch_walk_kernel, dim3(walkGrid), dim3(64), 0, st, w);
    e = hipGetLastError();
    if (ev) (void)hipEventRecord(ev[2], st);
    return e;
}

}  // namespace gsa
