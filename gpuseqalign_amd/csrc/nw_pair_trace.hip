// nw_pair_trace.hip -- the alignment of one long pair (gsa_align_pair_dev): NW / SW
// with linear or affine gaps, traced on the device from the score launch's checkpoint rows.
//
// The strip fill and the walk are nw_pair_trace_dev.h's.  A fill task is a ticket t of the chunk's atomic
// counter: strip tLo + t of the one pair in the arguments, its codes at t stripBytes.  The border is
// kGlobal or kLocal: row 0 and column 0 are gap runs from (0, 0), or 0 with every H floored at 0; row
// letters clamp to R, and only the lanes with rows up to iEnd have cells.
#include "nw_pair_trace.h"

#include "nw_pair_trace_dev.h"

namespace gsa {

namespace {

using namespace pair_dev;

template <bool LOCAL, bool AFFINE, int KR>
__global__ __launch_bounds__(64) void nw_pair_fill_kernel(PairFillArgs a)
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
        task.clampRow = a.R;
        task.lastRow = a.iEnd;
        task.W = a.J;
        task.jW = 0;
        task.gh = a.gran + grow;
        task.gf = a.gran2 + grow;
        task.cw = a.codes + (size_t)t * (size_t)a.stripBytes;
        GSA_PAIR_STRIP_FILL((LOCAL ? kLocal : kGlobal), AFFINE, KR, task, tab, ssz, a.go, a.ge);
    }
}

__global__ __launch_bounds__(64) void nw_pair_walk_kernel(PairWalkArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool local = a.local != 0;
    const WalkTask w = {a.seqY, a.seqX, a.codes, a.stripBytes, a.krShift, a.tLo, a.iStop, 0, a.moves};
    GSA_PAIR_WALK(w, local, *a.rec);
}

template <int KR>
hipError_t fill_grid_kr(int local, bool affine, int nstrips, int* grid)
{
    if (local)
        return affine ? fill_grid_for(nw_pair_fill_kernel<true, true, KR>, nstrips, 0, grid)
                      : fill_grid_for(nw_pair_fill_kernel<true, false, KR>, nstrips, 0, grid);
    return affine ? fill_grid_for(nw_pair_fill_kernel<false, true, KR>, nstrips, 0, grid)
                  : fill_grid_for(nw_pair_fill_kernel<false, false, KR>, nstrips, 0, grid);
}

template <int KR>
hipError_t launch_fill_kr(const PairFillArgs& a, int grid, hipStream_t st)
{
    const bool affine = a.go != a.ge;
    if (a.local)
        return affine ? launch_fill_for(nw_pair_fill_kernel<true, true, KR>, a, grid, st)
                      : launch_fill_for(nw_pair_fill_kernel<true, false, KR>, a, grid, st);
    return affine ? launch_fill_for(nw_pair_fill_kernel<false, true, KR>, a, grid, st)
                  : launch_fill_for(nw_pair_fill_kernel<false, false, KR>, a, grid, st);
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
