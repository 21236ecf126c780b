// nw_pair_semi_trace.hip -- the semi-global alignment of one long pair (gsa_align_pair_semi_dev;
// DESIGN.md 2.2k): the whole query within a long subject, traced on the device from the score launch's
// checkpoint rows.
//
// The strip fill and the walk are nw_pair_trace_dev.h's.  A fill task is a ticket t of the chunk's atomic
// counter: strip tLo + t of the one pair in the arguments, its codes at t stripBytes, over the column
// window jW + 1 ... J (nw_pair_semi_plan.h): letters, checkpoint rows and codes are addressed from jW.
// The border is kSemi: the row above strip 0 is the free row 0 (H = 0, F = minus infinity); column jW is
// the global column 0 with H(0, 0) = 0 if jW = 0, and minus infinity for the rows >= 1 otherwise; row
// letters clamp to R and all rows 1 ... R are filled.
#include "nw_pair_semi_trace.h"

#include "nw_pair_trace_dev.h"

namespace gsa {

namespace {

using namespace pair_dev;

template <bool AFFINE, int KR>
__global__ __launch_bounds__(64) void nw_semi_fill_kernel(SemiFillArgs a)
{
    __shared__ int tab[32 * 32];
    const int ssz = a.substsz;
    load_tab(tab, a.subst, ssz);
    __syncthreads();

    const int lane = threadIdx.x;
    const int jW = a.jW, W = a.J - a.jW;  // the window's columns are jW + 1 ... jW + W
    const int* const x = a.seqX + jW;     // x[c]: the letter of window column c
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
        task.x = x;
        task.clampRow = a.R;
        task.lastRow = a.R;
        task.W = W;
        task.jW = jW;
        task.gh = a.gran + grow + jW;
        task.gf = a.gran2 + grow + jW;
        task.cw = a.codes + (size_t)t * (size_t)a.stripBytes;
        GSA_PAIR_STRIP_FILL((kSemi), AFFINE, KR, task, tab, ssz, a.go, a.ge);
    }
}

__global__ __launch_bounds__(64) void nw_semi_walk_kernel(SemiWalkArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const WalkTask w = {a.seqY, a.seqX, a.codes, a.stripBytes, a.krShift, a.tLo, a.iStop, a.jW, a.moves};
    GSA_SEMI_WALK(w, *a.rec);
}

template <int KR>
hipError_t launch_fill_kr(const SemiFillArgs& a, int grid, hipStream_t st)
{
    return a.go != a.ge ? launch_fill_for(nw_semi_fill_kernel<true, KR>, a, grid, st)
                        : launch_fill_for(nw_semi_fill_kernel<false, KR>, a, grid, st);
}

}  // namespace

hipError_t semi_fill_grid(bool affine, int KR, int nstrips, int* grid)
{
    if (KR != 8 && KR != 16) return hipErrorInvalidValue;
    if (KR == 8)
        return affine ? fill_grid_for(nw_semi_fill_kernel<true, 8>, nstrips, 0, grid)
                      : fill_grid_for(nw_semi_fill_kernel<false, 8>, nstrips, 0, grid);
    return affine ? fill_grid_for(nw_semi_fill_kernel<true, 16>, nstrips, 0, grid)
                  : fill_grid_for(nw_semi_fill_kernel<false, 16>, nstrips, 0, grid);
}

hipError_t launch_semi_trace(const SemiFillArgs& f, const SemiWalkArgs& w, int KR, int grid, hipEvent_t* ev, hipStream_t st)
{
    if (KR != 8 && KR != 16) return hipErrorInvalidValue;
    if (f.J <= f.jW || f.jW < 0 || f.jW != w.jW) return hipErrorInvalidValue;
    if (ev) (void)hipEventRecord(ev[0], st);
    hipError_t e = KR == 8 ? launch_fill_kr<8>(f, grid, st) : launch_fill_kr<16>(f, grid, st);
    if (e != hipSuccess) return e;
    if (ev) (void)hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(nw_semi_walk_kernel, dim3(1), dim3(64), 0, st, w);
    e = hipGetLastError();
    if (ev) (void)hipEventRecord(ev[2], st);
    return e;
}

}  // namespace gsa
