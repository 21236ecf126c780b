// nw_pair_overlap_trace.hip -- the overlap (dovetail) alignment of one long pair
// (gsa_align_pair_overlap_dev): a suffix of either sequence against a prefix of the
// other, or either within the other, traced on the device from the score launch's checkpoint rows.
//
// The strip fill and the walk are nw_pair_trace_dev.h's.  A fill task is a ticket t of the chunk's atomic
// counter: strip tLo + t of the one pair in the arguments, its codes at t stripBytes.  The border is
// kOverlap: the row above strip 0 is the free row 0 (H = 0, F = minus infinity), and column 0 is free as
// well (H = 0, E = F = minus infinity in every row) -- set from the definition, not read from the score
// launch, whose F on column 0 is folded into a floor; only the rows 1 ... i_end are filled, and row
// letters clamp to i_end.
#include "nw_pair_overlap_trace.h"

#include "nw_pair_trace_dev.h"

namespace gsa {

namespace {

using namespace pair_dev;

template <bool AFFINE, int KR>
__global__ __launch_bounds__(64) void nw_overlap_fill_kernel(OverlapFillArgs a)
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
        if (t >= (unsigned)a.nstrips) break;
        const int s = a.tLo + (int)t;
        const size_t grow = (size_t)(s > 0 ? s - 1 : 0) * (size_t)a.granStride;
        StripTask task;
        task.s = s;
        task.seqY = a.seqY;
        task.x = a.seqX;
        task.clampRow = a.iEnd;
        task.lastRow = a.iEnd;
        task.W = a.J;
        task.jW = 0;
        task.gh = a.gran + grow;
        task.gf = a.gran2 + grow;
        task.cw = a.codes + (size_t)t * (size_t)a.stripBytes;
        GSA_PAIR_STRIP_FILL((kOverlap), AFFINE, KR, task, tab, ssz, a.go, a.ge);
    }
}

__global__ __launch_bounds__(64) void nw_overlap_walk_kernel(OverlapWalkArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const WalkTask w = {a.seqY, a.seqX, a.codes, a.stripBytes, a.krShift, a.tLo, a.iStop, 0, a.moves};
    GSA_OVERLAP_WALK(w, *a.rec);
}

template <int KR>
hipError_t launch_fill_kr(const OverlapFillArgs& a, int grid, hipStream_t st)
{
    return a.go != a.ge ? launch_fill_for(nw_overlap_fill_kernel<true, KR>, a, grid, st)
                        : launch_fill_for(nw_overlap_fill_kernel<false, KR>, a, grid, st);
}

}  // namespace

hipError_t overlap_fill_grid(bool affine, int KR, int nstrips, int* grid)
{
    if (KR != 8 && KR != 16) return hipErrorInvalidValue;
    if (KR == 8)
        return affine ? fill_grid_for(nw_overlap_fill_kernel<true, 8>, nstrips, 0, grid)
                      : fill_grid_for(nw_overlap_fill_kernel<false, 8>, nstrips, 0, grid);
    return affine ? fill_grid_for(nw_overlap_fill_kernel<true, 16>, nstrips, 0, grid)
                  : fill_grid_for(nw_overlap_fill_kernel<false, 16>, nstrips, 0, grid);
}

hipError_t launch_overlap_trace(const OverlapFillArgs& f, const OverlapWalkArgs& w, int KR, int grid, hipEvent_t* ev, hipStream_t st)
{
    if (KR != 8 && KR != 16) return hipErrorInvalidValue;
    if (f.J < 1 || f.iEnd < 1 || f.nstrips < 1 || f.tLo < 0 || f.tLo != w.tLo) return hipErrorInvalidValue;
    if (ev) (void)hipEventRecord(ev[0], st);
    hipError_t e = KR == 8 ? launch_fill_kr<8>(f, grid, st) : launch_fill_kr<16>(f, grid, st);
    if (e != hipSuccess) return e;
    if (ev) (void)hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(nw_overlap_walk_kernel, dim3(1), dim3(64), 0, st, w);
    e = hipGetLastError();
    if (ev) (void)hipEventRecord(ev[2], st);
    return e;
}

}  // namespace gsa
